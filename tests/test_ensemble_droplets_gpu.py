"""Ensembles whose members carry droplets (wx_ensemble_create_droplets): a member equals the same simulation on a handle of its own from
wx_create(X, Y, n_droplets) -- the droplet pool, the feedback / deposition textures, the lightning texel, every grid field, the iteration
counter and the diagnostics, bit for bit (NaNs compared as positions) under WX_OPT_SPLAT_ORDER 1, and under the default order wherever a
lone handle is reproducible itself; once against the CPU oracle directly; and wx_ensemble_particle_stats shows that the shared particle
launches are what ran. Every comparison is `==` unless a tolerance is stated."""
import os

import numpy as np
import pytest

import impulse_scenes as I
from test_ensemble_gpu import BRUSH, FIELDS, _perturbed, same_bits, same_diag

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_GRID = ("BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1")


def pool_of(drops, n):
    """n droplets: the first n of ``drops``, padded with inactive ones (random seeds as initRainDrops lays them out)."""
    d = np.ascontiguousarray(drops[:n], np.float32)
    if len(d) < n:
        rng = np.random.Generator(np.random.Philox(4242))
        pad = rng.random((n - len(d), 5)).astype(np.float32)
        pad[:, 2] -= np.float32(10.0)
        d = np.concatenate([d, pad])
    return d


class DropTwins:
    """An ensemble with droplets and one lone handle per member, given the same calls."""

    def __init__(self, pkg, specs):
        """specs: dicts with base, water, wall, drops (n x 5, the same n for all), u (uniform dict), iter0, options {option: value}."""
        self.pkg, E = pkg, pkg.engine
        Y, X = specs[0]["base"].shape[:2]
        n = len(specs[0]["drops"])
        self.X, self.Y, self.n = X, Y, n
        self.ens = E.Ensemble(len(specs), X, Y, n)
        self.lone = [E.Handle(X, Y, n) for _ in specs]
        self.u = [dict(s["u"]) for s in specs]
        for i, s in enumerate(specs):
            assert len(s["drops"]) == n
            for h in self.both(i):
                h.upload(s["base"], s["water"], s["wall"], s["drops"])
                for opt, val in s.get("options", {}).items():
                    h.set_option(opt, val)
                h.iter = s.get("iter0", 0)
            self.push(i)

    def both(self, i):
        return (self.ens[i], self.lone[i])

    def push(self, i, **changes):
        P = self.pkg.params
        self.u[i].update(changes)
        u = self.u[i]
        for h in self.both(i):
            h.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"], u.get("sounding_T"), u.get("sounding_W"), u.get("sounding_Vel"))

    def step(self, n):
        self.ens.step(n)
        for h in self.lone:
            h.step(n)

    def compare(self, where, members=None, fields=FIELDS, diag=True):
        for i in (range(len(self.lone)) if members is None else members):
            a, b = self.both(i)
            x, y = a.read_particles(), b.read_particles()
            assert same_bits(x, y), (where, "member", i, "droplets", int((x != y).sum()))
            for f in fields:
                x, y = a.read_rect(f), b.read_rect(f)
                assert same_bits(x, y), (where, "member", i, f, int((x != y).sum()) if x.shape == y.shape else "shape")
            assert a.iter == b.iter, (where, i)
            if diag:
                assert same_diag(a.diagnostics(), b.diagnostics()) is None, (where, i)
        if diag and members is None:
            for i, d in enumerate(self.ens.diagnostics()):
                assert same_diag(d, self.lone[i].diagnostics()) is None, (where, "wx_ensemble_diagnostics", i)

    def close(self):
        self.ens.close()
        for h in self.lone:
            h.close()


def _precip64(golden, **u_changes):
    g, u = golden("precip64")
    u = dict(u, quad_scale=0, enablePrecipitation=1, **u_changes)
    return g, u


def _order1(pkg):
    return {pkg.engine.Handle.OPT_SPLAT_ORDER: 1}


def test_members_equal_lone_handles_coupled(pkg, golden):
    """Five members of precip64 (64 x 64: TXn = 2 with a one-column tile), WX_OPT_SPLAT_ORDER 1, that differ in spawnChanceMult, fallSpeed,
    evapRate, temperature and iteration counter: 1 + 3 + 8 + 20 iterations (past one staging chunk of 16), everything compared after
    every step."""
    g, u = _precip64(golden)
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    specs = []
    for i, ch in enumerate((dict(), dict(spawnChanceMult=float(u["spawnChanceMult"]) * 3.0), dict(fallSpeed=float(u["fallSpeed"]) * 0.5),
                            dict(evapRate=float(u["evapRate"]) * 2.0), dict())):
        b, w, wl = _perturbed(g["in_base"], g["in_water"], g["in_wall"], i) if i == 4 else (g["in_base"], g["in_water"], g["in_wall"])
        specs.append(dict(base=b, water=w, wall=wl, drops=drops, u=dict(u, **ch), iter0=int(g["iter0"]) + 101 * i, options=_order1(pkg)))
    t = DropTwins(pkg, specs)
    try:
        for n in (1, 3, 8, 20):
            t.step(n)
            t.compare(("precip64", n))
        for i in range(5):
            assert np.abs(t.ens[i].read_rect("PRECIP_FB")).max() > 0 and np.abs(t.ens[i].read_rect("PRECIP_DEP")).max() > 0, i
        pools = [t.ens[i].read_particles() for i in range(5)]
        assert any(not same_bits(pools[0], p) for p in pools[1:])  # the members are different simulations
        assert t.ens.particle_stats()["member_iters_particles_batched"] == 5 * 32
        assert t.ens.stats()["member_iters_batched"] == 5 * 32 and t.ens.stats()["member_iters_solo"] == 0
    finally:
        t.close()


def test_one_member_against_the_oracle(pkg, oracle, golden):
    """Not through lone handles: member 1 of three runs precip64 under splat_order 1 for 1, 3 and 8 iterations and equals wx_oracle."""
    g, u = _precip64(golden, splat_order=1)
    X, Y = int(g["X"]), int(g["Y"])
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    other = _perturbed(g["in_base"], g["in_water"], g["in_wall"], 3)
    specs = [dict(base=other[0], water=other[1], wall=other[2], drops=drops, u=dict(u, spawnChanceMult=float(u["spawnChanceMult"]) * 2.0)),
             dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], drops=drops, u=u, options=_order1(pkg)),
             dict(base=other[0], water=other[1], wall=other[2], drops=drops, u=dict(u, **BRUSH), options=_order1(pkg))]
    t = DropTwins(pkg, specs)
    o = oracle.OracleSim(X, Y, len(drops))
    try:
        o.upload(g["in_base"], g["in_water"], g["in_wall"], drops)
        o.set_params(u)
        for n in (1, 3, 8):
            t.ens.step(n)
            o.step(n)
            m = t.ens[1]
            assert np.array_equal(m.read_particles(), o.field("DROPS")), n
            for f in ("PRECIP_FB", "PRECIP_DEP", "LIGHTNING") + ORACLE_GRID:
                assert same_bits(m.read_rect(f), o.field(f)), (n, f)
        assert np.abs(t.ens[1].read_rect("PRECIP_FB")).max() > 0 and np.abs(t.ens[1].read_rect("PRECIP_DEP")).max() > 0
        assert t.ens.particle_stats()["member_iters_particles_batched"] == 3 * 12
    finally:
        t.close()


def test_16_members_of_the_100x100_save(pkg, golden):
    """The reference's save (100 x 100, 400 droplets: no multiple of 256 or of a tile), 16 perturbed members, order 1, 20 + 30 iterations.
    Members 3 and 7 cross a multiple of 600 inside the run, at different iterations (the 600-iteration refresh of inactiveDroplets from
    texel (0,0)); the others do not."""
    g, u = golden("save100qa_precip")
    u = dict(u, quad_scale=0, enablePrecipitation=1)
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    assert len(drops) == 400
    iter0 = [1000 + 601 * i for i in range(16)]  # 1000 + 601 i mod 600 = 400 + i: nobody crosses within 50 iterations ...
    iter0[3], iter0[7] = 3 * 600 - 7, 9 * 600 - 33  # ... but these two: in the first step / in the second
    for i, v in enumerate(iter0):
        crosses = any((v + k) % 600 == 0 for k in range(50))
        assert crosses == (i in (3, 7)), (i, v)
    specs = []
    for i in range(16):
        b, w, wl = _perturbed(g["in_base"], g["in_water"], g["in_wall"], i)
        specs.append(dict(base=b, water=w, wall=wl, drops=drops, u=u, iter0=iter0[i], options=_order1(pkg)))
    t = DropTwins(pkg, specs)
    try:
        for n in (20, 30):
            t.step(n)
            t.compare(("save100", n), diag=False)
        t.compare("save100 diag", members=(0, 3, 7, 15), fields=())
        assert t.ens.particle_stats()["member_iters_particles_batched"] == 16 * 50
    finally:
        t.close()


def test_particle_launches_do_not_grow_with_the_ensemble(pkg, golden):
    g, u = _precip64(golden)
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    seen = {}
    for B in (1, 16):
        t = DropTwins(pkg, [dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], drops=drops, u=u) for _ in range(B)])
        try:
            t.ens.step(10)
            t.ens.sync()
            ps, st = t.ens.particle_stats(), t.ens.stats()
            assert ps["member_iters_particles_batched"] == 10 * B, ps
            # (the first iteration runs without feedback textures, the other nine with: one instantiation per iteration either way)
            assert st == {"member_iters_batched": 10 * B, "member_iters_solo": 0, "march_launches": 10}, st
            seen[B] = ps["particle_launches"]
        finally:
            t.close()
    assert seen[1] == seen[16] == 4 * 10, seen


def test_default_order_agrees_as_two_lone_runs_do(pkg, golden):
    """fp32 atomics in arrival order: after one iteration the pool is bit-equal (per-droplet arithmetic), the textures agree within the
    summation-order tolerance of test_particles_vs_oracle, and the inactive count in texel (0,0) -- integers -- is equal."""
    g, u = _precip64(golden)
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    specs = [dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], drops=drops, u=dict(u, **ch))
             for ch in (dict(), dict(fallSpeed=float(u["fallSpeed"]) * 0.5), dict(spawnChanceMult=float(u["spawnChanceMult"]) * 3.0))]
    t = DropTwins(pkg, specs)
    try:
        t.step(1)
        for i in range(3):
            a, b = t.both(i)
            assert same_bits(a.read_particles(), b.read_particles()), i
            fa, fb = a.read_rect("PRECIP_FB"), b.read_rect("PRECIP_FB")
            assert np.abs(fa - fb).max() <= 1e-7 * max(1.0, np.abs(fb).max()), i
            assert round(float(fa[0, 0, 0])) == round(float(fb[0, 0, 0])), i
            assert np.abs(a.read_rect("PRECIP_DEP") - b.read_rect("PRECIP_DEP")).max() <= 1e-7, i
            assert same_bits(a.read_rect("LIGHTNING"), b.read_rect("LIGHTNING")), i
    finally:
        t.close()


def _lone_droplet(X, Y, n):
    """impulse_scenes' droplet kind with ONE planted droplet left active in a pool of n: its sprite overlaps nobody's, sums are order-free."""
    base, water, wall, drops, _ = I.impulse_scene(X, Y, "droplet", background="terrain")
    pool = np.zeros((n, 5), np.float32)
    pool[:, 2] = -10.5
    pool[0] = drops[len(drops) // 2]
    return base, water, wall, pool


def test_default_order_lone_droplet_is_bit_exact(pkg):
    X, Y = 505, 77
    base, water, wall, pool = _lone_droplet(X, Y, 40)
    t = DropTwins(pkg, [dict(base=base, water=water, wall=wall, drops=pool, u=I.scene_uniforms("droplet", Y))])
    try:
        assert (t.ens[0].read_particles()[:, 2] >= 0).sum() == 1
        for n in (1, 11):
            t.step(n)
            t.compare(("lone droplet", n))
        assert np.abs(t.ens[0].read_rect("PRECIP_FB")[..., 1:]).max() > 0 or np.abs(t.ens[0].read_rect("PRECIP_DEP")).max() > 0
        assert t.ens.particle_stats() == {"member_iters_particles_batched": 12, "particle_launches": 48}
    finally:
        t.close()


def test_mixed_ensemble(pkg, golden):
    """n_droplets = 300: (a) precipitation on, order 1; (b) enablePrecipitation 0; (c) a brush held -- the other marching partition --
    with precipitation on, order 1; (d) WX_OPT_KERNEL_SET 0: solo, with its droplets, order 1; (e) order 0 with a lone droplet."""
    g, u = _precip64(golden)
    H = pkg.engine.Handle
    drops = pool_of(g["in_drops"], 300)
    lone = np.zeros((300, 5), np.float32)
    lone[:, 2] = -10.5
    lone[0] = (0.1, 0.2, 0.6, 0.0, 1.0)  # one active rain droplet aloft
    common = dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"])
    specs = [dict(common, drops=drops, u=u, options=_order1(pkg)),
             dict(common, drops=drops, u=dict(u, enablePrecipitation=0)),
             dict(common, drops=drops, u=dict(u, **BRUSH), options=_order1(pkg)),
             dict(common, drops=drops, u=u, options={H.OPT_SPLAT_ORDER: 1, H.OPT_KERNEL_SET: 0}),
             dict(common, drops=lone, u=dict(u, spawnChanceMult=0.0))]
    t = DropTwins(pkg, specs)
    try:
        for k, n in enumerate((2, 7)):
            t.step(n)
            t.compare(("mixed", n))
        assert np.array_equal(t.ens[1].read_particles(), drops)  # (b)'s pool is untouched
        st, ps = t.ens.stats(), t.ens.particle_stats()
        assert st["member_iters_solo"] == 9 and st["member_iters_batched"] == 4 * 9, st
        assert ps["member_iters_particles_batched"] == 3 * 9, ps
        assert ps["particle_launches"] == 9 * (4 + 2 * 2), ps  # the shared four + sort and run sums of (a) and (c)
    finally:
        t.close()


def test_precipitation_switched_off_and_on_between_steps(pkg, golden):
    """The hazard of host bookkeeping that runs ahead: the first iteration after precipitation was switched off still reads the feedback
    textures, and their one-time clear must be enqueued BEHIND its launch (a lone handle clears after the iteration).
    With the clear moved back in front of the launches (the memsets enqueued from the bookkeeping loop) the first comparison behind
    the switch, ('off', 1) of member 0, is the one expected to fail: its iteration then reads zeroed textures where the lone handle
    reads the last deposits."""
    g, u = _precip64(golden)
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    specs = [dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], drops=drops, u=u, options=_order1(pkg)) for _ in range(2)]
    specs[1]["u"] = dict(u, fallSpeed=float(u["fallSpeed"]) * 0.5)
    t = DropTwins(pkg, specs)
    try:
        t.step(5)
        t.compare(("on", 5))
        assert np.abs(t.ens[0].read_rect("PRECIP_FB")).max() > 0
        t.push(0, enablePrecipitation=0)
        for n in (1, 4):
            t.step(n)
            t.compare(("off", n))
        assert np.abs(t.ens[0].read_rect("PRECIP_FB")).max() == 0 and np.abs(t.ens[0].read_rect("PRECIP_DEP")).max() == 0
        t.push(0, enablePrecipitation=1)
        t.step(5)
        t.compare(("on again", 5))
        assert t.ens.particle_stats()["member_iters_particles_batched"] == 2 * 15 - 5
    finally:
        t.close()


@pytest.mark.parametrize("X,Y,B,n", [(57, 9, 3, 1), (2, 4, 2, 257), (505, 77, 1, 1000), (130, 50, 4, 256)])
def test_ragged_and_tiny(pkg, X, Y, B, n):
    S, P = pkg.synth, pkg.params
    base, water, wall = S.terrain_grid(X, Y)
    S.add_cloud_deck(water, wall)
    gui = P.merge_settings(None)
    gui["sunAngle"] = 40.0
    u = P.uniforms_from_gui(gui, Y, quad_scale=0, pass_mask=P.PASS_ALL)
    u["enablePrecipitation"] = 1
    u["spawnChanceMult"] = 5.0
    specs = []
    for i in range(B):
        d = S.init_rain_drops(n, seed=11 + i)
        d[: max(1, n // 3), :2] = np.random.Generator(np.random.Philox(5 + i)).uniform(-0.9, 0.9, (max(1, n // 3), 2)).astype(np.float32)
        d[: max(1, n // 3), 2:] = (0.5, 0.0, 1.0)  # a third of the pool is rain aloft
        b, w, wl = _perturbed(base, water, wall, i)
        specs.append(dict(base=b, water=w, wall=wl, drops=d, u=u, iter0=597 * i, options=_order1(pkg)))
    t = DropTwins(pkg, specs)
    try:
        t.step(6)
        t.compare(("ragged", X, Y, B, n))
        assert t.ens.particle_stats()["member_iters_particles_batched"] == 6 * B
    finally:
        t.close()


def test_wx_step_on_a_borrowed_member_and_init_droplets(pkg, golden):
    g, u = _precip64(golden)
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    specs = [dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], drops=drops, u=u, options=_order1(pkg)) for _ in range(3)]
    t = DropTwins(pkg, specs)
    try:
        for h in t.both(2):  # wx_init_droplets on a member: the pool of a lone handle with the same seed
            h.init_droplets(77)
        assert np.array_equal(t.ens[2].read_particles(), pkg.synth.init_rain_drops_hashed(len(drops), 77))
        t.step(3)
        t.compare("before")
        for h in t.both(1):  # wx_step on the borrowed member, between two ensemble steps
            h.step(2)
        t.compare("borrowed step", members=(1,))
        t.step(4)
        t.compare("after")
        assert t.ens[1].iter == t.ens[0].iter + 2
        assert t.ens.particle_stats()["member_iters_particles_batched"] == 3 * 7
    finally:
        t.close()


def test_check_launches_on_one_member(pkg, golden):
    g, u = _precip64(golden)
    H = pkg.engine.Handle
    drops = np.ascontiguousarray(g["in_drops"], np.float32)
    specs = [dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], drops=drops, u=u, options=_order1(pkg)) for _ in range(3)]
    specs[1]["options"] = {H.OPT_SPLAT_ORDER: 1, H.OPT_CHECK_LAUNCHES: 1}
    t = DropTwins(pkg, specs)
    try:
        t.step(4)
        t.compare("check launches")
    finally:
        t.close()


def test_weather_ensemble_from_save(pkg):
    path = os.path.join(ROOT, "tests", "golden", "save100.weathersandbox")
    sf = pkg.codec.load(path)
    H = pkg.engine.Handle
    mults = [0.00002, 0.0001, 0.001, 0.01]  # the `spawnChance` control is what sets the spawnChanceMult uniform (params.uniforms_from_gui)
    ens = pkg.sim.WeatherEnsemble.from_save(4, sf, overrides=[dict(spawnChance=m) for m in mults])
    lone = []
    try:
        assert ens.engine.n_droplets == len(sf.droplets) > 0
        for i, m in enumerate(mults):
            w = pkg.sim.WeatherSim.from_save(sf)
            w.verbose = False
            w.set_gui(spawnChance=m)
            assert ens[i].uniforms()["spawnChanceMult"] == w.uniforms()["spawnChanceMult"] == m
            lone.append(w)
            for s in (ens[i], w):
                s.handle.set_option(H.OPT_SPLAT_ORDER, 1)
        ens.step()
        for w in lone:
            w.step()
        pools = []
        for i, w in enumerate(lone):
            pools.append(ens[i].read_particles())
            assert same_bits(pools[-1], w.read_particles()), i
            for f in FIELDS:
                assert same_bits(ens[i].read_rect(f), w.read_rect(f)), (i, f)
            assert ens[i].iter_num == w.iter_num
        assert sum(not same_bits(pools[0], p) for p in pools[1:]) >= 2  # (on the CPU oracle all three differ from member 0's after this frame)
        n = int(lone[0].gui["IterPerFrame"])
        assert ens.particle_stats()["member_iters_particles_batched"] == 4 * n
    finally:
        ens.close()
        for w in lone:
            w.handle.close()
