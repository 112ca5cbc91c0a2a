"""Colliding deposits in the shipped splat order (WX_OPT_SPLAT_ORDER 0: one fp32 atomic per droplet and channel at the sprite's anchor)
against the CPU oracle in splat_order 1, which is the engine's own summation tree: the cases of tests/collision_scenes.py on a handle.

exact kinds   overlapping sprites, two droplets on one anchor, sprites over the mailbox texels, two lightning requests: at most two
              non-zero deposits per anchor and channel (tests/test_collision_cpu.py demands it of every iteration), fp32 addition
              commutes -- array_equal after every step, every field, coupled over 6 iterations;
membership    3 / 4 droplets on one isolated anchor: the footprint is uniform and its value is one of the oracle's orderings;
tiny          subnormal deposits and sums, in both orders;
dense         1500 droplets on a few anchors: the derived bound of oracle/wx_oracle.h (wxo_splat_audit), not a measured tolerance."""
import numpy as np
import pytest

import collision_scenes as K
import droplet_scenes as D

pytestmark = pytest.mark.gpu
CASES = K.cases()
GRID_FIELDS = ("BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1")
PARTICLE_FIELDS = ("PRECIP_FB", "PRECIP_DEP", "LIGHTNING")


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _setup(h, pkg, c, sc):
    P = pkg.params
    h.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
    h.set_params(P.fill_struct(P.WxParams(), sc["u"]), sc["u"]["initial_T"])
    h.iter = sc["iter0"]
    if sc["lightning0"]:
        h.set_lightning(np.asarray(sc["lightning0"], np.float32))


def _handle(pkg, c, sc, order=0):
    cfg = D.CONFIGS[c["config"]]
    h = pkg.engine.Handle(c["X"], c["Y"], len(sc["drops"]))
    _setup(h, pkg, c, sc)
    h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
    h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
    h.set_option(h.OPT_SPLAT_ORDER, order)
    return h


def _compare(h, o, c, sc, where, particle_textures=True):
    """Handle against oracle, bit for bit: droplets, the particle textures with texels (0,0) and (1,0), the lightning state, every grid field."""
    X, cid = c["X"], K.case_id(c)
    want, got = o.field("DROPS"), h.read_particles()
    if not _same(got, want):
        k = int(np.nonzero((got != want).any(-1))[0][0])
        raise AssertionError(f"{cid} after {where} iterations: droplet {k} is {got[k].tolist()}, the oracle's {want[k].tolist()}")
    for f in (PARTICLE_FIELDS if particle_textures else ("LIGHTNING",)) + GRID_FIELDS:
        a, b = h.read_rect(f), o.field(f)
        b = b.reshape(a.shape) if f == "LIGHTNING" else b
        assert _same(a, b), f"{cid} after {where} iterations: " + (D.describe(f, a, b, sc, X, want) if a.ndim == 3 and a.shape[0] > 1 else f"{f}: {a.ravel()} != {b.ravel()}")
    assert h.iter == o.iter, (cid, h.iter, o.iter)


def _run(pkg, oracle, c, order=0):
    sc = K.build_case(c)
    h, o = _handle(pkg, c, sc, order), K.oracle_for(oracle, c, sc)
    try:
        calls, compare = D.schedule(c["config"], sc["n_iter"], sc["event_at"])
        done = 0
        for n, flag in calls:
            h.step(n, flag)
            o.step(n)
            done += n
            if done in compare:
                _compare(h, o, c, sc, done)
        assert done == sc["n_iter"] == compare[-1]
    finally:
        h.close()
        o.close()


GROUPS = sorted({(c["kind"], c["placement"]) for c in CASES})


@pytest.mark.parametrize("kind,placement", GROUPS, ids=[f"{k}-{p}" for k, p in GROUPS])
def test_colliding_deposits_equal_order_1_bit_for_bit(pkg, oracle, kind, placement):
    """Every exact case of one kind at one placement, the device in the DEFAULT order under the case's configuration (marching / per-pass
    kernels; display, plain and MORE_TO_COME iterations), the oracle in order 1: array_equal after every step of six iterations."""
    mine = [c for c in CASES if (c["kind"], c["placement"]) == (kind, placement)]
    assert mine
    for c in mine:
        _run(pkg, oracle, c)


ENSEMBLE_CASES = (("pair", "seam", "flight"), ("overlap", "interior", "grow"), ("mailbox", "mailbox", "pair_lightning"), ("pair", "ragged_tile", "ground"),
                  ("overlap", "rim", "mixed"))


def test_ensemble_members_with_colliding_deposits_equal_the_oracle(pkg, oracle):
    """Five members, five colliding scenes (k_*_ens of csrc/wx_precip_ens.h), default order: every member equals ITS oracle run in
    order 1 after every iteration."""
    cs = [next(c for c in CASES if (c["kind"], c["placement"], c["variant"]) == k and c["grid"] == "ragged") for k in ENSEMBLE_CASES]
    scs = [K.build_case(c) for c in cs]
    X, Y = K.GRIDS["ragged"]
    ens = pkg.engine.Ensemble(len(cs), X, Y, D.POOL)
    os_ = [K.oracle_for(oracle, c, sc) for c, sc in zip(cs, scs)]
    try:
        for i, (c, sc) in enumerate(zip(cs, scs)):
            _setup(ens[i], pkg, c, sc)
        for it in range(K.N_ITER):
            ens.step(1)
            for i, o in enumerate(os_):
                o.step(1)
                _compare(ens[i], o, cs[i], scs[i], f"{it + 1} (member {i})")
            assert ens.particle_stats()["member_iters_particles_batched"] == len(cs) * (it + 1), (it, ens.particle_stats())
    finally:
        ens.close()
        for o in os_:
            o.close()


@pytest.mark.parametrize("kind,placement,variant", [("pair", "interior", "flight"), ("overlap", "seam", "dry")])
def test_clone_taken_between_two_colliding_iterations(pkg, oracle, kind, placement, variant):
    """wx_copy_state after three colliding iterations (anchors that held two deposits are being cleared, their tiles dirty): source and
    clone go on colliding and both stay equal to the oracle."""
    c = dict(next(c for c in CASES if (c["kind"], c["placement"], c["variant"]) == (kind, placement, variant) and c["grid"] == "ragged"), config="wet")
    sc = K.build_case(c)
    h, o = _handle(pkg, c, sc), K.oracle_for(oracle, c, sc)
    clone = None
    try:
        h.step(3)
        o.step(3)
        _compare(h, o, c, sc, 3)
        clone = pkg.engine.Handle(c["X"], c["Y"], len(sc["drops"]))
        clone.copy_from(h)
        _compare(clone, o, c, sc, "3 (the clone, before it steps)")
        for it in range(3, K.N_ITER):
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


MEMBERS = K.member_cases()


@pytest.mark.parametrize("c", MEMBERS, ids=[K.case_id(c) for c in MEMBERS])
def test_three_and_four_deposits_on_one_anchor_give_one_of_the_orderings(pkg, oracle, c):
    """n droplets on one isolated anchor, ONE iteration in the default order. Per channel the device's footprint is uniform and its value
    is one of the sequential sums the oracle gives over the orderings of the colliding records (n!/2 at most); outside the footprint
    the textures equal the oracle's (zero, and the inactive count); droplets, lightning state and grid fields are bit-exact."""
    sc = K.build_case(c)
    X, Y = c["X"], c["Y"]
    (q, r), cand, runs = K.member_candidates(oracle, c, sc)
    rows, cols = K.footprint(q, r, X, Y)
    h, o = _handle(pkg, c, sc), K.oracle_for(oracle, c, sc)
    try:
        h.step(1)
        o.step(1)
        _compare(h, o, c, sc, 1, particle_textures=False)
        fb, dep = h.read_rect("PRECIP_FB"), h.read_rect("PRECIP_DEP")
        ofb, odep = o.field("PRECIP_FB"), o.field("PRECIP_DEP")
        assert _same(fb[..., 3], ofb[..., 3])
        got = [fb[..., 0], fb[..., 1], fb[..., 2], dep[..., 0], dep[..., 1]]
        want = [ofb[..., 0], ofb[..., 1], ofb[..., 2], odep[..., 0], odep[..., 1]]
        for ch, (g, w) in enumerate(zip(got, want)):
            v = np.ascontiguousarray(g[rows, cols])
            bits = v.view(np.uint32)
            assert (bits == bits.flat[0]).all(), f"{K.case_id(c)} channel {ch}: the footprint is not uniform: {np.unique(v)}"
            assert int(bits.flat[0]) in cand[ch], (f"{K.case_id(c)} channel {ch}: the footprint holds {v.flat[0]!r} ({int(bits.flat[0]):#x}), no ordering of the "
                                                     f"deposits gives it: {sorted(hex(x) for x in cand[ch])}")
            g, w = g.copy(), w.copy()
            g[rows, cols] = 0
            w[rows, cols] = 0
            assert _same(g, w), f"{K.case_id(c)} channel {ch}: outside the footprint"
    finally:
        h.close()
        o.close()


TINY = K.tiny_cases()


@pytest.mark.parametrize("order", [1, 0], ids=["order1", "default_order"])
@pytest.mark.parametrize("c", TINY, ids=[K.case_id(c) for c in TINY])
def test_subnormal_deposits_equal_the_oracle(pkg, oracle, c, order):
    """One and two evaporating droplets of mass 1e-36 / 3e-37 on one anchor (vapour feedback mass / 144: subnormal addends and sums) and a
    ground hit with rain 5e-39. Order 1 adds them with plain additions; the default order hands them to the hardware's fp32 atomic
    (the build uses -munsafe-fp-atomics). Both must keep the subnormals as the oracle does."""
    _run(pkg, oracle, c, order)


def test_dense_shaft_lies_within_the_derived_bound(pkg, oracle):
    """1500 droplets over 5 x 4 cells: anchors with more than a hundred deposits. After the first iteration PRECIP_FB and PRECIP_DEP lie
    within sum_box gamma(n_a + 7) S_a of the exact (double) planes, texel by texel (+ u |out| on the two mailbox texels); droplets and
    grid fields are bit-exact (they read the previous feedback); the inactive count is exact. The second iteration: the oracle is given
    the device's particle textures -- the only state that differed -- so that this iteration's summation alone separates the two, and the
    same bound, now evaluated on the device's droplets, holds again."""
    c = K.dense_case()
    sc = K.build_case(c)
    X, Y = c["X"], c["Y"]
    h, o = _handle(pkg, c, sc), K.oracle_for(oracle, c, sc)
    try:
        for it in range(2):
            with oracle.SplatAudit(X, Y) as au:
                o.step(1)
            h.step(1)
            _compare(h, o, c, sc, it + 1, particle_textures=False)
            fb, dep = h.read_rect("PRECIP_FB"), h.read_rect("PRECIP_DEP")
            # the inactive count in texel (0,0), which no sprite of this scene covers: an integer below 2^24, exact
            assert fb[0, 0, 0] == au.exact[0, 0, 0] == np.floor(au.exact[0, 0, 0]) and K.DENSE_FILL <= fb[0, 0, 0] < 2 ** 24, (fb[0, 0], au.exact[0, 0])
            assert it or fb[0, 0, 0] == K.DENSE_FILL
            assert au.count.max() >= (100 if it == 0 else 50), au.count.max()
            ok, worst = K.within_bound(fb, dep, au.exact, au.bound)
            print(f"dense iteration {it + 1}: max n_a {int(au.count.max())}, worst |out - exact| / bound = {worst:.4f}")
            assert ok, f"iteration {it + 1}: the device's particle textures leave the derived bound: worst |out - exact| / bound = {worst}"
            assert _same(fb[..., 3], o.field("PRECIP_FB")[..., 3])
            o.view("PRECIP_FB")[:] = fb
            o.view("PRECIP_DEP")[:] = dep
    finally:
        h.close()
        o.close()
