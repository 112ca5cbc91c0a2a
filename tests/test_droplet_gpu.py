"""Droplet life cycle, event by event, in the shipped splat order: every case of tests/droplet_scenes.py (a spawn, a lightning
request, an evaporation, a ground hit with its deposit, the 600-iteration refresh, a sprite walking across splat tiles ...) on a handle
against the CPU oracle, BIT FOR BIT after every step -- droplet records, the feedback texture with its mailbox texels (0,0) / (1,0),
the deposition texture, the lightning state and every grid field. tests/test_droplet_cpu.py shows on the oracle that each event happens
and that no texel of any compared iteration receives two deposits, which is what makes the default order (fp32 atomics) exact.
Besides equality: no texel outside the oracle's non-zero set is non-zero (a missed "zero this tile" item, named as such), both splat
orders give the same bits, a clone taken mid-cycle continues like its source, ensemble members equal lone handles, slab groups equal
the whole domain. Every comparison here is array_equal."""
import numpy as np
import pytest

import droplet_scenes as D

pytestmark = pytest.mark.gpu
CASES = D.cases()
GRID_FIELDS = ("BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1")
PARTICLE_FIELDS = ("PRECIP_FB", "PRECIP_DEP", "LIGHTNING")


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _handle(pkg, c, sc, order=None):
    E, P = pkg.engine, pkg.params
    cfg = D.CONFIGS[c["config"]]
    h = E.Handle(c["X"], c["Y"], len(sc["drops"]))
    h.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
    h.set_params(P.fill_struct(P.WxParams(), sc["u"]), sc["u"]["initial_T"])
    h.iter = sc["iter0"]
    h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
    h.set_option(h.OPT_ROW_BANDS, c.get("bands", 1))
    h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
    h.set_option(h.OPT_SPLAT_ORDER, cfg.get("splat_order", 0) if order is None else order)
    if sc["lightning0"]:
        h.set_lightning(np.asarray(sc["lightning0"], np.float32))
    return h


def _oracle(oracle, c, sc):
    o = oracle.OracleSim(c["X"], c["Y"], len(sc["drops"]))
    o.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
    o.set_params(dict(sc["u"], splat_order=D.CONFIGS[c["config"]].get("splat_order", 0)))
    o.iter = sc["iter0"]
    if sc["lightning0"]:
        o.set_lightning(sc["lightning0"])
    return o


def _compare(h, o, c, sc, where):
    """Handle against oracle: everything, bit for bit; a difference names the nearest site, the nearest droplet and their phases."""
    X = c["X"]
    cid = D.case_id(c)
    want = o.field("DROPS")
    got = h.read_particles()
    if not _same(got, want):
        k = int(np.nonzero((got != want).any(-1))[0][0])
        q = D.anchor_of(want[k], X, c["Y"]) if want[k, 2] >= 0 and abs(want[k, 0]) <= 1 and abs(want[k, 1]) <= 1 else None
        raise AssertionError(f"{cid} after {where} iterations: droplet {k} is {got[k].tolist()}, the oracle's {want[k].tolist()}; anchor {q}"
                             + (f" phases {D.phases(q[0], q[1], X)}" if q else "") + f"; expected of it: {sc['expect'].get(k)}")
    for f in PARTICLE_FIELDS + GRID_FIELDS:
        a, b = h.read_rect(f), o.field(f)
        b = b.reshape(a.shape) if f == "LIGHTNING" else b
        if f in ("PRECIP_FB", "PRECIP_DEP"):  # flag consistency first: it names the cause
            stray = (a != 0) & (b == 0)
            assert not stray.any(), f"{cid} after {where} iterations: {f} holds values where the oracle's is zero (a tile that was not zeroed): " \
                                    f"{D.describe(f, a, b, sc, X, want)}"
        assert _same(a, b), f"{cid} after {where} iterations: " + (D.describe(f, a, b, sc, X, want) if a.ndim == 3 and a.shape[0] > 1 else f"{f}: {a.ravel()} != {b.ravel()}")
    assert h.iter == o.iter, (cid, h.iter, o.iter)


def _run(pkg, oracle, c):
    sc = D.build_case(c)
    h, o = _handle(pkg, c, sc), _oracle(oracle, c, sc)
    try:
        calls, compare = D.schedule(c["config"], sc["n_iter"], sc["event_at"])
        done = 0
        for n, flag in calls:
            h.step(n, flag)
            o.step(n)
            done += n
            if done in compare:
                _compare(h, o, c, sc, done)
        assert done == sc["n_iter"] and compare[-1] == done
    finally:
        h.close()
        o.close()


@pytest.mark.parametrize("kind", D.KINDS + D.ORDER1_KINDS)
def test_event_equals_the_oracle_bit_for_bit(pkg, oracle, kind):
    """Every case of one kind: under every configuration on the ragged grid, on the aligned and the tiny grid (and the band grid); the
    order-1 kinds under WX_OPT_SPLAT_ORDER 1 on both kernel sets."""
    mine = [c for c in CASES if c["kind"] == kind]
    assert len(mine) >= (2 if kind in D.ORDER1_KINDS else len(D.CONFIG_CYCLE) + 1)
    for c in mine:
        _run(pkg, oracle, c)


@pytest.mark.parametrize("kind", D.KINDS)
def test_both_splat_orders_give_the_same_bits(pkg, kind):
    """The same case in the default order and under WX_OPT_SPLAT_ORDER 1 on two handles, after every iteration (it follows from the
    two oracle comparisons; a mismatch here names the order)."""
    c = next(c for c in CASES if c["kind"] == kind and c["config"] == "wet")
    sc = D.build_case(c)
    a, b = _handle(pkg, c, sc, order=0), _handle(pkg, c, sc, order=1)
    try:
        for it in range(sc["n_iter"]):
            a.step(1)
            b.step(1)
            assert _same(a.read_particles(), b.read_particles()), (D.case_id(c), it, "droplets")
            for f in PARTICLE_FIELDS + ("BASE_CUR", "WATER_CUR", "WALL_CUR"):
                x, y = a.read_rect(f), b.read_rect(f)
                assert _same(x, y), (D.case_id(c), it, D.describe(f, x, y, sc, c["X"]) if x.ndim == 3 and x.shape[0] > 1 else f)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("grid", ["ragged", "aligned"])
@pytest.mark.parametrize("clone_after", [1, 7])
def test_clone_taken_mid_cycle_continues_like_the_oracle(pkg, oracle, grid, clone_after):
    """wx_copy_state of the walk scene's handle in the default order into a fresh handle: after iteration 1 (the evaporated droplets'
    tiles were dirty in iteration 0 and are being zeroed: one iteration after they left; the walkers are airborne with their tiles
    dirty) and after iteration 7 (walker 1 has just left its upper tile row). Source and clone go on and both stay equal to the
    oracle: the clone carries dirty, fb_zero, the work-list parity and the pool's counters."""
    c = dict(next(c for c in CASES if c["kind"] == "walk" and c["grid"] == grid), config="wet")
    sc = D.build_case(c)
    h, o = _handle(pkg, c, sc), _oracle(oracle, c, sc)
    clone = None
    try:
        h.step(clone_after)
        o.step(clone_after)
        _compare(h, o, c, sc, clone_after)
        clone = pkg.engine.Handle(c["X"], c["Y"], len(sc["drops"]))
        clone.copy_from(h)
        _compare(clone, o, c, sc, f"{clone_after} (the clone, before it steps)")
        for it in range(clone_after, sc["n_iter"]):
            h.step(1)
            clone.step(1)
            o.step(1)
            _compare(h, o, c, sc, it + 1)
            _compare(clone, o, c, sc, f"{it + 1} (the clone)")
    finally:
        h.close()
        o.close()
        if clone is not None:
            clone.close()


ENSEMBLE_KINDS = ("spawn_rain", "lightning_granted", "ground_flat", "refresh", "walk")


def test_ensemble_members_of_five_kinds_equal_lone_handles(pkg, oracle):
    """Five members, each a different event kind (different uniforms, iteration counters 7 / 40 / 598, lightning states), in the default
    order: after every iteration every member equals its lone handle, member 0 the oracle; and the particle pass of every
    member-iteration shared its launches."""
    cs = [next(c for c in CASES if c["kind"] == k and c["grid"] == "ragged" and c["config"] == "wet") for k in ENSEMBLE_KINDS]
    scs = [D.build_case(c) for c in cs]
    E, P = pkg.engine, pkg.params
    X, Y = D.GRIDS["ragged"]
    ens = E.Ensemble(len(cs), X, Y, D.POOL)
    lone = [_handle(pkg, c, sc) for c, sc in zip(cs, scs)]
    o = _oracle(oracle, cs[0], scs[0])
    try:
        for i, sc in enumerate(scs):
            m = ens[i]
            m.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
            m.iter = sc["iter0"]
            m.set_params(P.fill_struct(P.WxParams(), sc["u"]), sc["u"]["initial_T"])
            if sc["lightning0"]:
                m.set_lightning(np.asarray(sc["lightning0"], np.float32))
        n_iter = 7
        for it in range(n_iter):
            ens.step(1)
            o.step(1)
            for i, h in enumerate(lone):
                h.step(1)
                assert _same(ens[i].read_particles(), h.read_particles()), (ENSEMBLE_KINDS[i], it, "droplets")
                for f in PARTICLE_FIELDS + GRID_FIELDS:
                    x, y = ens[i].read_rect(f), h.read_rect(f)
                    assert _same(x, y), (ENSEMBLE_KINDS[i], it, D.describe(f, x, y, scs[i], X) if x.ndim == 3 and x.shape[0] > 1 else f)
            if it < scs[0]["n_iter"]:
                _compare(ens[0], o, cs[0], scs[0], it + 1)
            assert ens.particle_stats()["member_iters_particles_batched"] == len(cs) * (it + 1), (it, ens.particle_stats())
    finally:
        ens.close()
        o.close()
        for h in lone:
            h.close()


@pytest.mark.parametrize("nslab", [2, 3])
@pytest.mark.parametrize("kind", ["spawn_snow", "spawn_wall", "ground_flat", "lightning_granted"])
def test_slab_group_equals_the_whole_domain(pkg, kind, nslab):
    """2 and 3 slabs on one GPU in exact mode, both splat orders, with the smallest halo the library takes with particles (64: halo and
    owned width are multiples of the splat tile, owned + 2 halo <= X -- so 256 columns for two slabs, 192 for three): the event placed
    in the last owned column of slab 0, in its first ghost column and mid-slab; every field and the lightning state of every slab equal
    the undecomposed handle bit for bit after every iteration of one exchange period (6), the pool at its end."""
    E, P = pkg.engine, pkg.params
    X, Y, halo = (256 if nslab == 2 else 192), 48, 64
    xo, period = X // nslab, 1 + (halo - 12) // 9
    for ox in (xo - 1, xo, xo // 2):
        for order in (0, 1):
            c = {"kind": kind, "grid": "aligned", "X": X, "Y": Y, "offset": [ox, 14], "lead": (ox + order) % 2, "config": "order1" if order else "wet"}
            sc = D.build_case(c)
            assert any(abs(s[0] - ox) <= 2 for s in sc["sites"]), (c, sc["sites"])  # (a flat column may be a column or two on)
            whole = _handle(pkg, c, sc)
            g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL, n_droplets=len(sc["drops"]))
            try:
                g.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
                g.set_params(P.fill_struct(P.WxParams(), sc["u"]), sc["u"]["initial_T"])
                g.set_option(E.Handle.OPT_SPLAT_ORDER, order)
                g.set_option(E.Handle.OPT_POOL_EXACT, 1)
                for s in g.slabs:
                    s.iter = sc["iter0"]
                    if sc["lightning0"]:
                        s.set_lightning(np.asarray(sc["lightning0"], np.float32))
                assert sc["event_at"] < period
                for it in range(period):
                    g.step(1)
                    whole.step(1)
                    for f in GRID_FIELDS + ("PRECIP_FB", "PRECIP_DEP"):
                        a, b = g.read(f), whole.read_rect(f)
                        if f == "PRECIP_FB":  # (a slab's feedback texture does not carry the mailbox texels: count and request live in its state)
                            b[0, :2] = 0
                            assert not a[0, :2].any()
                        assert _same(a, b), (kind, nslab, ox, order, it, D.describe(f, a, b, sc, X))
                    assert all(_same(s.lightning(), whole.lightning()) for s in g.slabs), (kind, nslab, ox, order, it)
                g.sync()
                assert _same(g.particles(), whole.read_particles()), (kind, nslab, ox, order, "droplets")
            finally:
                g.close()
                whole.close()
