"""Ensemble quantiles and ranks on the GPU (wx_ensemble_quantiles): the device result equals wx_ens_quant_cells on the members' read_rect
arrays and the definition of include/wxsim.h, written down as `reference` of tests/test_ensemble_quantiles_cpu.py -- every plane, both
supported fields, whole grids and ragged rectangles, all three interpolations, eight quantiles at once, the rank of a member outside
the selection, masks, non-finite and wall cells, members with droplets, on the staged (LDS) path up to its last member count and on the
streaming path from the first one behind it; the result does not depend on the order of the members; the call is ordered behind pending
steps, changes nothing, and refuses what the header says it refuses. Every comparison is `==` on bits (NaNs compared as positions)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import impulse_scenes as I
from test_ensemble_droplets_gpu import _order1, _precip64, pool_of
from test_ensemble_gpu import FIELDS, Twins, same_bits, same_diag
from test_ensemble_quantiles_cpu import INTERPS, P8, P_SEP, PLANES, SEPARATING_CELLS, check, planted, reference
from test_ensemble_statistics_gpu import EARLY, STAT_FIELDS, Stepped, make_ensemble, member_specs, rectangles

pytestmark = pytest.mark.gpu


def cut(planes, x, y, w, h):
    """The rectangle of every plane (q carries the quantile axis in front)."""
    return {k: np.ascontiguousarray(v[:, y:y + h, x:x + w] if k == "q" else v[y:y + h, x:x + w]) for k, v in planes.items()}


@pytest.fixture(scope="module")
def stepped(pkg):
    """Ensembles of B + 1 members -- B that are selected and member B, the one that is ranked --, stepped once and shared."""
    made = {}

    def get(X, Y, B, steps):
        if (X, Y, B, steps) not in made:
            made[(X, Y, B, steps)] = Stepped(pkg, X, Y, B + 1, steps)
        return made[(X, Y, B, steps)]

    yield get
    for s in made.values():
        s.ens.close()


def staged_limit(pkg):
    return pkg.engine.lib().wx_ens_quant_staged_members()


# (X, Y, number of selected members; "L": wx_ens_quant_staged_members(), the last count of the staged path, "L+1": the first of the
# streaming path; 64 + 1 = 65 is no power of two, so it also is the count above 64 that is none)
SIZES = [(57, 9, 1), (57, 9, 2), (57, 9, 3), (57, 9, 5), (57, 9, "L"), (57, 9, "L+1"), (130, 50, 5), (505, 77, 3)]


@pytest.mark.parametrize("X,Y,B", SIZES, ids=[f"{x}x{y}x{b}" for x, y, b in SIZES])
def test_device_equals_host_equals_definition(pkg, stepped, X, Y, B):
    L = staged_limit(pkg)
    assert L + 1 > 64 and (L + 1) & L != 0
    B = {"L": L, "L+1": L + 1}.get(B, B)
    t = stepped(X, Y, B, EARLY if Y == 9 else 12)  # (a 9-row grid is all wall after eight iterations: EARLY)
    sel = list(range(B))
    seen = dict(differ=False, some_wall=False, between=False)
    for field in STAT_FIELDS:
        for interp in INTERPS:
            want = reference(t.fields[field], t.walls, sel, P8, interp, B)
            host = pkg.engine.ens_quant_cells(t.fields[field], t.walls, P8, interp=interp, rank_of=B)
            check(host, want, (field, interp, "host function, whole grid"))
            for (x, y, w, h) in rectangles(X, Y):
                got = t.ens.quantiles(field, P8, x, y, w, h, interp=interp, rank_of=B)
                assert got["q"].shape == (8, h, w, 4) and got["n_wall"].shape == (h, w) and got["n_below"].dtype == np.int32
                check(got, cut(want, x, y, w, h), (field, interp, (x, y, w, h)))
            seen["differ"] |= bool((want["q"][0] != want["q"][1])[want["count"] > 1].any())
            seen["some_wall"] |= bool(((want["n_wall"] > 0) & (want["n_wall"] < B)).any())
            seen["between"] |= bool(((want["n_below"] > 0) & (want["n_below"] + want["n_equal"] < want["count"])).any())
        x, y, w, h = rectangles(X, Y)[1]  # the host function on the rectangle's own cells, as a host without the device call would
        sub = pkg.engine.ens_quant_cells([a[y:y + h, x:x + w] for a in t.fields[field]], [a[y:y + h, x:x + w] for a in t.walls], P8, rank_of=B)
        check(sub, cut(reference(t.fields[field], t.walls, sel, P8, "linear", B), x, y, w, h), (field, "host function, interior"))
    # the members are different simulations on different terrain: the order statistics are not trivial
    if B > 1:
        assert seen["differ"] and seen["some_wall"]
    if B >= 3:
        assert seen["between"]


@pytest.mark.parametrize("B", [5, "L+1"])
def test_planted_cells(pkg, B):
    """Nothing is stepped. Member 2 is uploaded with NaN / +Inf / -Inf in a few BASE_CUR cells, member 3 with a column of wall cells;
    one air cell holds ties (1, 2, 2, 3, 1, ...) with the ranked member on the tie, one holds -0.0 in every member."""
    B = staged_limit(pkg) + 1 if B == "L+1" else B
    X, Y = 57, 9
    specs = member_specs(pkg, X, Y, B + 1)
    bad = [(6, 20, 0, np.nan), (6, 21, 3, np.inf), (7, 40, 1, -np.inf), (5, 56, 2, np.nan), (8, 0, 0, np.inf)]  # (y, x, channel, value): rows that are air in every member
    for s in specs:
        s["base"], s["wall"] = s["base"].copy(), s["wall"].copy()
    for (y, x, c, v) in bad + [(6, 30, 0, 0), (6, 31, 1, 0)]:
        assert all(s["wall"][y, x, 1] != 0 for s in specs)
    for (y, x, c, v) in bad:
        specs[2]["base"][y, x, c] = v
    specs[3]["wall"][:, 10, 1] = 0
    ties = np.float32([[1.0, 2.0, 2.0, 3.0][i % 4] for i in range(B)])
    for i in range(B):
        specs[i]["base"][6, 30, 0] = ties[i]
        specs[i]["base"][6, 31, 1] = np.float32(-0.0)
    specs[B]["base"][6, 30, 0] = np.float32(2.0)
    specs[B]["base"][6, 31, 1] = np.float32(0.0)
    specs[B]["base"][6, 20, 0] = np.float32(np.nan)
    ens = make_ensemble(pkg, specs)
    try:
        fields, walls = [m.read_rect("BASE_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        for interp in INTERPS:
            want = reference(fields, walls, list(range(B)), P8, interp, B)
            got = ens.quantiles("BASE_CUR", P8, interp=interp, rank_of=B)
            check(got, want, ("planted", interp))
            check(pkg.engine.ens_quant_cells(fields, walls, P8, interp=interp, rank_of=B), want, ("planted, host", interp))
            for (y, x, c, v) in bad:
                assert got["count"][y, x, c] == B - 1 and got["n_wall"][y, x] == 0 and np.isfinite(got["q"][:, y, x, c]).all(), (y, x, c)
                assert all(got["count"][y, x, o] == B for o in range(4) if o != c)
            assert (got["n_wall"][:, 10] >= 1).all() and got["n_wall"][Y - 1, 10] == 1 and (got["count"][Y - 1, 10] == B - 1).all()
            s = np.sort(ties)
            assert got["q"][0, 6, 30, 0] == 1.0 and got["q"][1, 6, 30, 0] == 3.0 and got["q"][2, 6, 30, 0] == 2.0 and s[(B - 1) // 2] == 2.0 == s[B // 2]
            assert got["n_below"][6, 30, 0] == (ties < 2).sum() and got["n_equal"][6, 30, 0] == (ties == 2).sum() >= 2
            assert (got["q"][:, 6, 31, 1].view(np.uint32) == 0).all()  # +0.0, whatever the members' zeros look like
            assert got["n_below"][6, 31, 1] == 0 and got["n_equal"][6, 31, 1] == B
            assert got["n_below"][6, 20, 0] == -1 and got["n_equal"][6, 20, 0] == -1 and got["n_below"][6, 20, 1] >= 0  # the ranked member's NaN
    finally:
        ens.close()


def test_masks_and_a_single_member(pkg, stepped):
    t = stepped(57, 9, 5, EARLY)  # six members; 5 is the ranked one where a rank is asked for
    for field in STAT_FIELDS:
        f, w = t.fields[field], t.walls
        check(t.ens.quantiles(field, P8, members=[0, 2, 4], rank_of=5), reference(f, w, [0, 2, 4], P8, "linear", 5), (field, "members 0, 2, 4"))
        check(t.ens.quantiles(field, P8, 3, 2, 52, 4, members=np.array([True, False, True, False, True, False]), interp="higher", rank_of=1),
              cut(reference(f, w, [0, 2, 4], P8, "higher", 1), 3, 2, 52, 4), (field, "boolean mask"))
        check(t.ens.quantiles(field, P8), reference(f, w, None, P8), (field, "everybody, no rank"))
        for interp in INTERPS:
            one = t.ens.quantiles(field, P8, members=[3], interp=interp)
            check(one, reference(f, w, [3], P8, interp), (field, "member 3 alone"))
            assert set(one) == {"q", "count", "n_wall"}
            entered = (w[3][..., 1] != 0)[..., None] & np.isfinite(f[3])
            for j in range(8):  # every quantile of one value is that value (a -0.0 as +0.0)
                assert same_bits(one["q"][j][entered], (f[3] + np.float32(0))[entered])
                assert np.isnan(one["q"][j][~entered]).all()
            assert (one["count"] == entered).all() and entered.any() and not entered.all()


def test_the_order_of_the_members_does_not_matter(pkg):
    """The same five simulations uploaded as members 0 .. 4 and as members 4 .. 0: the same bits (the statistics call, a sum in member
    order by definition, cannot promise that)."""
    specs = member_specs(pkg, 57, 9, 5)
    a, b = make_ensemble(pkg, specs), make_ensemble(pkg, specs[::-1])
    try:
        a.step(EARLY)
        b.step(EARLY)
        for field in STAT_FIELDS:
            for interp in INTERPS:
                check(b.quantiles(field, P8, interp=interp), a.quantiles(field, P8, interp=interp), (field, interp, "reversed"))
            check(b.quantiles(field, P8, members=[3, 2, 1, 0], rank_of=4), a.quantiles(field, P8, members=[1, 2, 3, 4], rank_of=0), (field, "reversed, ranked"))
        assert np.isfinite(a.quantiles("BASE_CUR", (0.5,))["q"]).any()
    finally:
        a.close()
        b.close()


def test_ordered_behind_a_pending_step(pkg):
    """quantiles directly after step(3), no sync in between: the numbers are those of the state AFTER the three iterations (iterations 3
    and 6 of a 9-row grid: see EARLY)."""
    ens = make_ensemble(pkg, member_specs(pkg, 57, 9, 5))
    try:
        seen = []
        for field in STAT_FIELDS:
            ens.step(3)
            got = ens.quantiles(field, P8, rank_of=4)
            want = reference([m.read_rect(field) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members], None, P8, "linear", 4)
            check(got, want, (field, "directly behind step(3)"))
            seen.append(ens.quantiles("WATER_CUR", (0.5,))["q"][0])
            assert np.isfinite(seen[-1]).any()
        assert not same_bits(seen[0][:3], seen[1][:3])  # (the iterations in between change the state: an unordered read would show)
        assert [m.iter for m in ens.members] == [s.get("iter0", 0) + 6 for s in member_specs(pkg, 57, 9, 5)]
    finally:
        ens.close()


def test_changes_nothing(pkg):
    """Every readable field, the diagnostics, the iteration counters and wx_ensemble_stats are the same before and after quantile calls,
    and five further iterations still equal lone handles that never saw the calls."""
    t = Twins(pkg, member_specs(pkg, 57, 9, 5))
    try:
        t.step(EARLY)

        def snapshot():
            return ([[m.read_rect(f) for f in FIELDS] for m in t.ens.members], t.ens.diagnostics(), [m.iter for m in t.ens.members], t.ens.stats())

        a = snapshot()
        for field in STAT_FIELDS:
            t.ens.quantiles(field, P8, rank_of=2)
            t.ens.quantiles(field, (0.5,), 3, 2, 40, 5, members=[1, 3], interp="lower", want=("q", "n_wall"))
        b = snapshot()
        for i in range(5):
            for k, f in enumerate(FIELDS):
                assert same_bits(a[0][i][k], b[0][i][k]), (i, f)
            assert same_diag(a[1][i], b[1][i]) is None, i
        assert a[2] == b[2] and a[3] == b[3]
        t.ens.quantiles("BASE_CUR", P8)  # ... and directly in front of a step
        t.step(5)
        t.compare("after quantile calls")
    finally:
        t.close()


def test_members_with_droplets(pkg, golden):
    """Ensemble(4, 64, 64, 400), deterministic splat order, precipitation on: WATER_CUR after 16 iterations."""
    g, u = _precip64(golden)
    drops = pool_of(np.ascontiguousarray(g["in_drops"], np.float32), 400)
    specs = []
    for i in range(4):
        water = g["in_water"].copy()
        water[40:44, 8 * i:8 * i + 8, 3] += np.float32(0.5 * (i + 1))  # smoke of its own: the members differ from the first iteration on
        specs.append(dict(base=g["in_base"], water=water, wall=g["in_wall"], drops=drops, u=dict(u, spawnChanceMult=float(u["spawnChanceMult"]) * (1 + i)),
                          iter0=int(g["iter0"]) + 101 * i, options=_order1(pkg)))
    ens = make_ensemble(pkg, specs, 400)
    try:
        ens.step(16)
        got = ens.quantiles("WATER_CUR", P8)
        fields, walls = [m.read_rect("WATER_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        want = reference(fields, walls, None, P8)
        check(got, want, "droplets")
        check(ens.quantiles("WATER_CUR", P8, 5, 7, 50, 41, members=[1, 2], interp="higher", rank_of=3), cut(reference(fields, walls, (1, 2), P8, "higher", 3), 5, 7, 50, 41),
              "droplets, rectangle")
        assert ens.particle_stats()["member_iters_particles_batched"] == 4 * 16
        assert (want["q"][0] != want["q"][1]).any() and any(np.abs(m.read_rect("PRECIP_FB")).max() > 0 for m in ens.members)
    finally:
        ens.close()


PX, PY = 57, 9  # the grid `planted` is laid out on: its cell i is (y, x) = divmod(i, PX)


def uploaded_planted(pkg, B):
    """planted(B, 57 * 9) -- its planted cells and the separating cells in front (row 0), random float bit patterns and random walls
    behind -- uploaded as BASE and as WATER of B + 1 members (member B is the ranked one); nothing is stepped."""
    f, w = planted(B, PX * PY)
    ens = pkg.engine.Ensemble(B + 1, PX, PY, 0)
    for i in range(B + 1):
        ens[i].upload(f[i].reshape(PY, PX, 4), f[i].reshape(PY, PX, 4), w[i].reshape(PY, PX, 4))
    return ens


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_quantiles_gpu as T
out = {}
for B in (6, pkg.engine.lib().wx_ens_quant_staged_members() + 2):  # the staged and the streaming kernel; the last member is ranked
    ens = T.make_ensemble(pkg, T.member_specs(pkg, 57, 9, B))
    ens.step(2)
    for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR"):
        out[f"{B}_{f}"] = np.stack([m.read_rect(f) for m in ens.members])
    for f in ("BASE_CUR", "WATER_CUR"):
        for k, v in ens.quantiles(f, T.P8, rank_of=B - 1).items():
            out[f"{B}_{f}_{k}"] = v
    ens.close()
for B in (7, pkg.engine.lib().wx_ens_quant_staged_members() + 1):  # planted uploads, the separating cells among them, at their own quantile
    ens = T.uploaded_planted(pkg, B)
    for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR"):
        out[f"u{B}_{f}"] = np.stack([m.read_rect(f) for m in ens.members])
    for f in ("BASE_CUR", "WATER_CUR"):
        for k, v in ens.quantiles(f, (T.P_SEP, 0.5), rank_of=B).items():
            out[f"u{B}_{f}_{k}"] = v
    ens.close()
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernels give what THIS process's host function and
    the definition give on the values the members held (the simulation steps of the two builds differ, the order statistics do not:
    every product that feeds a sum or a difference is rounded on its own in every build)."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    dst = str(tmp_path / "fast.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, root, dst], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(dst)
    for B in (6, staged_limit(pkg) + 2):
        walls = list(d[f"{B}_WALL_CUR"])
        for f in STAT_FIELDS:
            fields = list(d[f"{B}_{f}"])
            got = {k: d[f"{B}_{f}_{k}"] for k in PLANES}
            check(got, pkg.engine.ens_quant_cells(fields, walls, P8, rank_of=B - 1), (B, f, "fast device vs exact host"))
            check(got, reference(fields, walls, None, P8, "linear", B - 1), (B, f, "fast device vs definition"))
            assert np.isfinite(got["q"]).any() and (got["q"][3] != got["q"][4]).any()
    # planted uploads on the staged and on the streaming path: the separating cells are the only data on which a g * d that the code
    # generator fused into the sum would show in the float32 quantile
    for B in (7, staged_limit(pkg) + 1):
        walls = list(d[f"u{B}_WALL_CUR"])
        for f in STAT_FIELDS:
            fields = list(d[f"u{B}_{f}"])
            assert all(a.view(np.uint32).tobytes() == b.reshape(PY, PX, 4).view(np.uint32).tobytes() for a, b in zip(fields, planted(B, PX * PY)[0]))
            got = {k: d[f"u{B}_{f}_{k}"] for k in PLANES}
            check(got, pkg.engine.ens_quant_cells(fields, walls, (P_SEP, 0.5), rank_of=B), (B, f, "planted: fast device vs exact host"))
            check(got, reference(fields, walls, None, (P_SEP, 0.5), "linear", B), (B, f, "planted: fast device vs definition"))
            for cell, _, _, defined, fused in SEPARATING_CELLS:
                assert (got["q"][0, 0, cell].view(np.uint32) == defined).all() and defined != fused and (got["count"][0, cell] == 2).all(), (B, f, cell)


def test_refusals(pkg):
    E = pkg.engine
    X, Y = 57, 9
    specs = member_specs(pkg, X, Y, 3)
    ens = make_ensemble(pkg, specs[:2] + [None])  # member 2 is never uploaded
    try:
        def refused(code, *a, **kw):
            with pytest.raises(E.WxError) as ei:
                ens.quantiles(*a, **kw)
            assert ei.value.code == code, (a, kw, str(ei.value))
            return str(ei.value)

        two = dict(members=[0, 1])
        msg = refused(-1, "CURL", (0.5,), **two)
        assert "WX_FIELD_BASE_CUR" in msg and "WX_FIELD_WATER_CUR" in msg
        for f in ("WALL_CUR", "BASE_DISP", "WATER_0", "LIGHT_0", "EMITTED"):
            refused(-1, f, (0.5,), **two)
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (X, 0, 1, 1)):
            assert "outside" in refused(-4, "BASE_CUR", (0.5,), *rect, **two)
        assert "[0, 1]" in refused(-1, "BASE_CUR", (0.5, float("nan")), **two)
        refused(-1, "BASE_CUR", (-0.25,), **two)
        refused(-1, "BASE_CUR", (1.5,), **two)
        assert "interp" in refused(-1, "BASE_CUR", (0.5,), interp=3, **two)
        assert "nobody" in refused(-1, "BASE_CUR", (0.5,), members=[])
        refused(-1, "BASE_CUR", (0.5,), members=np.zeros(3, bool))
        assert "rank_member" in refused(-1, "BASE_CUR", (0.5,), members=[0], rank_of=3)
        assert "rank_member" in refused(-1, "BASE_CUR", (0.5,), members=[0], rank_of=-2)
        assert "selected" in refused(-1, "BASE_CUR", (0.5,), members=[0, 1], rank_of=1)
        assert "rank_member" in refused(-1, "BASE_CUR", (0.5,), want=("q", "n_below"), **two)  # n_below without a ranked member
        st = E.WxEnsQuant()  # n_q > 0 without a q array, n_q out of range: the struct by hand
        st.n_q, st.rank_member = 1, -1
        mask = np.array([1, 1, 0], np.uint8)
        for n_q in (1, 9, -1):
            st.n_q = n_q
            assert E.lib().wx_ensemble_quantiles(ens._e, E.FIELD_IDS["BASE_CUR"], 0, 0, X, Y, mask.ctypes.data, C.byref(st)) == -1
        assert "member 2" in refused(-5, "BASE_CUR", (0.5,))
        assert "member 2" in refused(-5, "WATER_CUR", (0.5,), members=[0, 2])
        assert "member 2" in refused(-5, "WATER_CUR", (0.5,), members=[0, 1], rank_of=2)  # the ranked member was never uploaded
        # the ensemble works as before: the uploaded members are served, and with member 2 uploaded all three step and are served
        fields, walls = [ens[i].read_rect("BASE_CUR") for i in (0, 1)], [ens[i].read_rect("WALL_CUR") for i in (0, 1)]
        check(ens.quantiles("BASE_CUR", P8, **two), reference(fields, walls, None, P8), "two of three")
        check(ens.quantiles("BASE_CUR", P8, members=[0], rank_of=1), reference(fields, walls, [0], P8, "linear", 1), "one of three, ranked")
        s, P = specs[2], pkg.params
        ens[2].upload(s["base"], s["water"], s["wall"])
        ens[2].set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
        ens.step(2)
        fields, walls = [m.read_rect("WATER_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        check(ens.quantiles("WATER_CUR", P8, rank_of=2), reference(fields, walls, None, P8, "linear", 2), "all three")
        assert ens.stats()["member_iters_batched"] == 6
    finally:
        ens.close()


def test_an_overflowed_list_surfaces_here(pkg):
    """WX_OPT_FIX_CAP 2 on a member with fast cells: its report (WX_E_STATE) is what the quantile call returns, naming the member -- once."""
    E = pkg.engine
    X, Y = 505, 77
    fast = I.impulse_scene(X, Y, "fast_vx")
    specs = member_specs(pkg, X, Y, 3)
    specs[1] = dict(base=fast[0], water=fast[1], wall=fast[2], u=I.scene_uniforms("fast_vx", Y), options={E.Handle.OPT_FIX_CAP: 2})
    ens = make_ensemble(pkg, specs)
    try:
        ens.step(2)
        with pytest.raises(E.WxError) as ei:
            ens.quantiles("BASE_CUR", (0.5,))
        assert ei.value.code == -5 and "member 1: " in str(ei.value), str(ei.value)
        got = ens.quantiles("BASE_CUR", P8)  # the report was consumed
        check(got, reference([m.read_rect("BASE_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members], None, P8), "after the report")
    finally:
        ens.close()


def test_weather_ensemble_quantiles_and_median(pkg):
    """WeatherEnsemble.from_sim -> perturb -> step -> quantiles / median; the profile names the kernel."""
    W = pkg.sim
    X, Y, B = 128, 48, 5
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    sim = W.WeatherSim(X, Y, base, water, wall, None, {"dayNightCycle": False}, sun_angle_deg=30.0)
    sim.verbose = False
    we = None
    try:
        sim.step(6)
        we = W.WeatherEnsemble.from_sim(sim, B)
        we.perturb("BASE_CUR", (0.0, 0.0, 0.0, 0.5), scale=8, seed=3, members=[1, 2, 3])  # member 4 stays a clone of member 0
        we.step(2)
        we.engine[0].profile(True)
        out = we.quantiles("BASE_CUR", (0.1, 0.5, 0.9), members=[0, 1, 2, 3], rank_of=4)
        prof = we.engine[0].profile_read()
        assert prof["ensemble_quantiles"][1] == 1 and prof["ensemble_quantiles"][0] > 0
        assert set(out) == set(PLANES) and out["q"].shape == (3, Y, X, 4)
        raw = we.engine.quantiles("BASE_CUR", (0.1, 0.5, 0.9), members=[0, 1, 2, 3], rank_of=4)
        check(out, raw, "pass-through")
        med = we.median("BASE_CUR", members=[0, 1, 2, 3])
        assert same_bits(med, out["q"][1])
        st = we.statistics("BASE_CUR", members=[0, 1, 2, 3])
        n = st["count"]
        assert same_bits(n, out["count"]) and same_bits(st["n_wall"], out["n_wall"]) and (n == 0).any() and (n == 4).any()
        assert ((st["min"] <= med) & (med <= st["max"]))[n > 0].all() and np.isnan(med[n == 0]).all()
        assert ((out["q"][0] <= out["q"][1]) & (out["q"][1] <= out["q"][2]))[n > 0].all() and (out["q"][0] < out["q"][2]).any()
        # member 4 is member 0 stepped alike: wherever it entered, it ties with member 0 at least
        entered = (we[4].read_rect("WALL_CUR")[..., 1] != 0)[..., None] & np.isfinite(we[4].read_rect("BASE_CUR"))
        assert (out["n_equal"][entered] >= 1).all() and (out["n_equal"][~entered] == -1).all() and entered.any()
        assert same_bits(we[4].read_rect("BASE_CUR"), we[0].read_rect("BASE_CUR"))
        some = we.median("WATER_CUR", 2, 3, 20, 10, members=[0, 3], interp="lower")
        assert some.shape == (10, 20, 4) and same_bits(some, we.quantiles("WATER_CUR", (0.5,), 2, 3, 20, 10, members=[0, 3], interp="lower", want=("q",))["q"][0])
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
