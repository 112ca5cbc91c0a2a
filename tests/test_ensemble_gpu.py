"""Ensembles on the GPU (wx_ensemble_*): a member of an ensemble equals the same simulation on a handle of its own -- every readable
field, the iteration counter, wx_fastest_velocity, wx_diagnostics and every reported error, bit for bit (NaNs compared as positions) --
whatever its neighbours in the launch do; once against the CPU oracle directly; and wx_ensemble_stats shows that the shared launches
are what ran. Every comparison is `==`."""
import numpy as np
import pytest

import impulse_scenes as I
import surface_scenes as S

pytestmark = pytest.mark.gpu

FIELDS = ["BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1", "CURL", "VORT", "PRECIP_FB", "PRECIP_DEP",
          "LIGHTNING", "EMITTED"]
BRUSH = dict(userInputType=1, userInputValues=(0.4, 0.5, 0.3, 6.0))
NO_BRUSH = dict(userInputType=-1, userInputValues=(0.0, 0.0, 0.0, 0.0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


def same_diag(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if not (same_bits(x, y) if x.dtype.kind == "f" else np.array_equal(x, y)):
            return k
    return None


class Twins:
    """An ensemble and one lone handle per member, given the same calls."""

    def __init__(self, pkg, specs):
        """specs: dicts with X, Y implied by base; keys base, water, wall, u (uniform dict), iter0, options {option: value}."""
        self.pkg, E = pkg, pkg.engine
        Y, X = specs[0]["base"].shape[:2]
        self.X, self.Y = X, Y
        self.ens = E.Ensemble(len(specs), X, Y)
        self.lone = [E.Handle(X, Y, 0) for _ in specs]
        self.u = [dict(s["u"]) for s in specs]
        for i, s in enumerate(specs):
            for h in self.both(i):
                h.upload(s["base"], s["water"], s["wall"])
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

    def compare(self, where, members=None, fields=FIELDS, diag=True, fastest=True):
        for i in (range(len(self.lone)) if members is None else members):
            a, b = self.both(i)
            for f in fields:
                x, y = a.read_rect(f), b.read_rect(f)
                assert same_bits(x, y), (where, "member", i, f, int((x != y).sum()) if x.shape == y.shape else "shape")
            assert a.iter == b.iter, (where, i)
            if fastest:
                fa, fb = a.fastest_velocity(), b.fastest_velocity()
                assert same_bits(np.float32(fa), np.float32(fb)), (where, i, fa, fb)
            if diag:
                assert same_diag(a.diagnostics(), b.diagnostics()) is None, (where, i)
        if diag and members is None:
            for i, d in enumerate(self.ens.diagnostics()):
                assert same_diag(d, self.lone[i].diagnostics()) is None, (where, "wx_ensemble_diagnostics", i)

    def close(self):
        self.ens.close()
        for h in self.lone:
            h.close()


def _slider_uniforms(pkg, Y, seed):
    """Off-default sliders: every control of params.GUI_RANGES that the merged settings carry, drawn inside its GUI range."""
    P = pkg.params
    gui = P.merge_settings(None)
    rng = np.random.default_rng(seed)
    for name, (lo, hi) in P.GUI_RANGES.items():
        if name in gui and isinstance(gui[name], (int, float)) and not isinstance(gui[name], bool) and name not in ("simHeight", "IterPerFrame", "sunAngle"):
            gui[name] = float(lo + (hi - lo) * (0.15 + 0.7 * rng.random()))
    gui["sunAngle"] = 35.0
    u = P.uniforms_from_gui(gui, Y, quad_scale=0, pass_mask=P.PASS_ALL)
    u["enablePrecipitation"] = 0
    return u


def _five_members(pkg, X=505, Y=77):
    fast = I.impulse_scene(X, Y, "fast_vx")
    smoke = I.impulse_scene(X, Y, "smoke", offset=(3, 2))
    snow = S.surface_scene(X, Y, "snow")
    nowrap = S.surface_scene(X, Y, "smoke", offset=2)
    cloud = I.impulse_scene(X, Y, "cloud", offset=(1, 4), background="terrain")
    return [
        dict(base=fast[0], water=fast[1], wall=fast[2], u=I.scene_uniforms("fast_vx", Y)),                       # 0: fast cells -> its exact-path list
        dict(base=smoke[0], water=smoke[1], wall=smoke[2], u=dict(I.scene_uniforms("smoke", Y), **BRUSH)),       # 1: holds a brush for a while
        dict(base=snow[0], water=snow[1], wall=snow[2], u=S.scene_uniforms(Y), iter0=9997),                      # 2: crosses iteration 10 000
        dict(base=nowrap[0], water=nowrap[1], wall=nowrap[2], u=S.scene_uniforms(Y, wrap=False)),                # 3: wrapHorizontally off
        dict(base=cloud[0], water=cloud[1], wall=cloud[2], u=_slider_uniforms(pkg, Y, 7)),                       # 4: off-default sliders
    ]


def test_members_equal_lone_handles(pkg):
    """Five different members of 505 x 77 in ONE ensemble, stepped 3 + 10 + 10 + 1 with reads in between. The brush of member 1 is held
    for the first 13 iterations: two partitions per iteration while it is, one afterwards -- wx_ensemble_stats counts the launches."""
    t = Twins(pkg, _five_members(pkg))
    try:
        launches = 0
        for k, n in enumerate((3, 10, 10, 1)):
            if k == 2:
                t.push(1, **NO_BRUSH)
            t.step(n)
            launches += n * (2 if k < 2 else 1)
            if k == 0:  # member 0's planted velocities went through ITS exact path, its neighbours' lists stayed empty
                fv = [t.ens[i].fastest_velocity() for i in range(5)]
                assert fv[0] >= 2.0 and fv[2] == 0.0 and fv[3] == 0.0, fv
                assert [h.fastest_velocity() for h in t.lone] == fv
            t.compare(("step", k))
            st = t.ens.stats()
            assert st == {"member_iters_batched": 5 * sum((3, 10, 10, 1)[:k + 1]), "member_iters_solo": 0, "march_launches": launches}, st
        assert t.ens[2].iter == 9997 + 24 and t.ens[0].iter == 24
        # the borrowed members refuse what belongs to the ensemble
        for call in (lambda h: h.set_stream(0), lambda h: h.set_comm_stream(0), lambda h: h.tune_placement(1, 1)):
            with pytest.raises(pkg.engine.WxError) as ei:
                call(t.ens[3])
            assert ei.value.code == -5
    finally:
        t.close()


def test_one_member_against_the_oracle(pkg, oracle, golden):
    """Not through lone handles: member 1 of three runs a golden's inputs for 50 iterations and equals wx_oracle."""
    g, u = golden("synth64")
    u["enablePrecipitation"] = 0
    u["quad_scale"] = 0
    X, Y = int(g["X"]), int(g["Y"])
    other = I.impulse_scene(X, Y, "fast_vy")
    specs = [dict(base=other[0], water=other[1], wall=other[2], u=I.scene_uniforms("fast_vy", Y)),
             dict(base=g["in_base"], water=g["in_water"], wall=g["in_wall"], u=u, iter0=int(g["iter0"])),
             dict(base=other[0], water=other[1], wall=other[2], u=dict(I.scene_uniforms("fast_vy", Y), **BRUSH))]
    t = Twins(pkg, specs)
    o = oracle.OracleSim(X, Y, 0)
    try:
        o.upload(g["in_base"], g["in_water"], g["in_wall"], None)
        o.set_params(u)
        o.iter = int(g["iter0"])
        for n in (1, 9, 40):
            t.ens.step(n)
            o.step(n)
            for f in ("BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1"):
                assert same_bits(t.ens[1].read_rect(f), o.field(f)), (n, f)
        assert t.ens.stats()["member_iters_batched"] == 150
    finally:
        t.close()


def _perturbed(base, water, wall, i, seed=99):
    rng = np.random.Generator(np.random.Philox(seed + i))
    b = base.copy()
    air = wall[..., 1] != 0
    for ch in (0, 1):
        b[..., ch] += np.where(air, rng.standard_normal(b.shape[:2], dtype=np.float32) * np.float32(0.01), 0).astype(np.float32)
    b[..., 3] += np.where(air, np.float32(0.05 * i), 0).astype(np.float32)
    return b, water, wall


def test_64_members_of_the_100x100_save(pkg, golden):
    g, u = golden("save100raw")
    u["enablePrecipitation"] = 0
    specs = []
    for i in range(64):
        b, w, wl = _perturbed(g["in_base"], g["in_water"], g["in_wall"], i)
        specs.append(dict(base=b, water=w, wall=wl, u=u, iter0=int(g["iter0"]) + 37 * i))
    t = Twins(pkg, specs)
    try:
        for n in (20, 30):  # (30: more iterations than one staging buffer of the argument table holds)
            t.step(n)
            t.compare(("save100", n), diag=False, fields=["BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_0", "LIGHT_1", "BASE_DISP", "WATER_0", "CURL"])
        t.compare("save100 diag", members=(0, 31, 63))
        st = t.ens.stats()
        assert st["member_iters_batched"] == 64 * 50 and st["member_iters_solo"] == 0 and st["march_launches"] <= 2 * 50, st
    finally:
        t.close()


@pytest.mark.parametrize("bands", [0, 1, 2])
def test_8_members_of_2500x300_with_terrain(pkg, bands):
    X, Y = 2500, 300
    E = pkg.engine
    specs = []
    for i in range(8):
        base, water, wall = pkg.synth.terrain_grid(X, Y, seed=0.1 + 0.1 * i)
        b, w, wl = _perturbed(base, water, wall, i)
        specs.append(dict(base=b, water=w, wall=wl, u=S.scene_uniforms(Y), options={E.Handle.OPT_ROW_BANDS: bands}, iter0=95 + i))
    t = Twins(pkg, specs)
    try:
        for n in (1, 11):
            t.step(n)
            t.compare(("2500x300", bands, n), diag=False, fields=["BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_0", "LIGHT_1", "BASE_DISP", "WATER_0", "CURL", "WALL_DISP", "EMITTED"])
        st = t.ens.stats()
        assert st == {"member_iters_batched": 8 * 12, "member_iters_solo": 0, "march_launches": 12}, st
    finally:
        t.close()


@pytest.mark.parametrize("X,Y,B", [(57, 9, 3), (2, 4, 3), (505, 77, 1)])
def test_ragged_tiny_and_single(pkg, X, Y, B):
    specs = []
    for i in range(B):
        base, water, wall = pkg.synth.dry_grid(X, Y, seed=50 + i, flow_sigma=0.05)
        base[Y - 2, (3 * i + 1) % X, 0] = 1.3 + i  # a fast cell (the exact path) ...
        water[2, X // 2, 3] = 2.0 + i              # ... and some smoke
        water[Y - 2, :, 0] += np.float32(0.5 * (i + 1))
        specs.append(dict(base=base, water=water, wall=wall, u=I.scene_uniforms("smoke", Y), iter0=98 * i))
    t = Twins(pkg, specs)
    try:
        for n in (1, 2, 9):
            t.step(n)
            t.compare((X, Y, B, n))
        st = t.ens.stats()
        assert st == {"member_iters_batched": B * 12, "member_iters_solo": 0, "march_launches": 12}, st
    finally:
        t.close()


def test_members_that_do_not_qualify_run_solo(pkg):
    """One member on the dry pass mask, one on the per-pass kernel set: counted solo, equal to their lone handles, the rest batched."""
    E, P = pkg.engine, pkg.params
    specs = _five_members(pkg)
    specs[1]["u"] = dict(specs[1]["u"], **NO_BRUSH)
    specs[1]["u"]["pass_mask"] = P.PASS_DRY
    specs[3]["options"] = {E.Handle.OPT_KERNEL_SET: 0}
    t = Twins(pkg, specs)
    try:
        for n in (2, 5):
            t.step(n)
            t.compare(("solo", n))
        st = t.ens.stats()
        assert st == {"member_iters_batched": 3 * 7, "member_iters_solo": 2 * 7, "march_launches": 7}, st
    finally:
        t.close()


def test_an_overflowed_list_is_its_members_error(pkg):
    """WX_OPT_FIX_CAP 2 on the member with fast cells (nothing faults: the list refuses what it cannot hold and reports). The lone handle
    reports WX_E_STATE at its next blocking call; so does the member -- through its own call in one ensemble, through wx_ensemble_sync,
    which names it, in another -- and the other members equal their lone handles."""
    E = pkg.engine
    for via_sync in (False, True):
        specs = _five_members(pkg)[:4]
        specs = [specs[1], specs[2], specs[0], specs[3]]  # the fast member is member 2
        specs[0]["u"] = dict(specs[0]["u"], **NO_BRUSH)
        specs[2]["options"] = {E.Handle.OPT_FIX_CAP: 2}
        t = Twins(pkg, specs)
        try:
            t.step(2)
            with pytest.raises(E.WxError) as lone_err:
                t.lone[2].read_rect("BASE_CUR")
            assert lone_err.value.code == -5
            with pytest.raises(E.WxError) as ens_err:
                t.ens.sync() if via_sync else t.ens[2].read_rect("BASE_CUR")
            assert ens_err.value.code == -5
            want = str(lone_err.value).split(": ", 1)[1]
            if via_sync:
                assert "member 2: " + want in str(ens_err.value), (str(ens_err.value), want)
            else:
                assert str(ens_err.value) == str(lone_err.value)
            t.compare(("overflow", via_sync), members=(0, 1, 3))
            t.ens.sync()  # the report was consumed: once, as on the lone handle
        finally:
            t.close()


def test_wx_step_on_a_borrowed_member_between_ensemble_steps(pkg):
    t = Twins(pkg, _five_members(pkg)[1:4])
    try:
        t.step(3)
        for h in t.both(1):
            h.step(4)
        t.compare("after wx_step on member 1", members=(1,))
        for h in t.both(0):
            h.step(1)
        t.step(5)
        t.compare("after the next ensemble step")
        assert t.ens[1].iter == 9997 + 12 and t.ens[0].iter == 9 and t.ens[2].iter == 8
        st = t.ens.stats()
        assert st["member_iters_batched"] == 3 * 8 and st["member_iters_solo"] == 0, st
    finally:
        t.close()


def test_weather_ensemble_sweeps_a_slider(pkg):
    """sim.WeatherEnsemble: one synthetic scene, per-member setting overrides == WeatherSim members of their own."""
    W = pkg.sim
    X, Y = 256, 96
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    over = [{"wind": -0.5 + 0.25 * i, "dayNightCycle": False} for i in range(4)]
    we = W.WeatherEnsemble(4, X, Y, base, water, wall, None, over, sun_angle_deg=30.0)
    lone = [W.WeatherSim(X, Y, base, water, wall, None, o, sun_angle_deg=30.0) for o in over]
    try:
        we.step(7)
        for s in lone:
            s.step(7)
        for i in range(4):
            for f in ("BASE_CUR", "WATER_CUR", "BASE_DISP"):
                assert same_bits(we[i].read_rect(f), lone[i].read_rect(f)), (i, f)
        assert not same_bits(we[0].read_rect("BASE_CUR"), we[3].read_rect("BASE_CUR"))
        assert we.stats()["member_iters_batched"] == 28
    finally:
        we.close()


def test_check_launches_on_one_member(pkg):
    """WX_OPT_CHECK_LAUNCHES on ONE member: the shared launches of its partition are synchronised and checked one by one; same results."""
    E = pkg.engine
    specs = _five_members(pkg)
    specs[2]["options"] = {E.Handle.OPT_CHECK_LAUNCHES: 1}
    t = Twins(pkg, specs)
    try:
        for n in (2, 11):
            t.step(n)
            t.compare(("check_launches", n))
        st = t.ens.stats()
        assert st == {"member_iters_batched": 5 * 13, "member_iters_solo": 0, "march_launches": 2 * 13}, st
    finally:
        t.close()
