"""Ensemble scores against a truth on the GPU (wx_ensemble_scores): the device result equals wx_ens_score_cells on the handles' read_rect
arrays and the definition of include/wxsim.h, written down as `reference` of tests/test_ensemble_scores_cpu.py -- every scalar, both
histograms and all three maps, both supported fields, whole grids and ragged rectangles, 1 to 64 selected members, the truth as a
member behind the selection, as a lone handle on its own stream and as a member of a second ensemble, planted cells for every reason a
cell-channel is not scored, the separating cells on both builds, masks, members with droplets; the call is ordered behind pending
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
from test_ensemble_scores_cpu import ALL, CASES, MAPS, check, planted, reference, scalars, separating_cells
from test_ensemble_statistics_gpu import STAT_FIELDS, Stepped, make_ensemble, member_specs, rectangles

pytestmark = pytest.mark.gpu

# Iterations before the comparison. The boundary pass grows the wall down from the top row of a grid of at most 50 rows, one row per
# iteration (test_ensemble_statistics_gpu.EARLY), and the terrain takes one to four rows at the bottom: the 9-row grids are compared after ONE
# iteration, the only count at which the truth is air in more than half of the cells for every member count below (measured on `reference`).
STEPS = {9: 1, 50: 12, 77: 12}


def cut(arrays, x, y, w, h):
    return [np.ascontiguousarray(a[y:y + h, x:x + w]) for a in arrays]


def limit(pkg):
    return pkg.engine.lib().wx_ens_score_max_members()


@pytest.fixture(scope="module")
def stepped(pkg):
    """Ensembles of B + 1 members -- B that are selected and member B, the truth --, stepped once and shared."""
    made = {}

    def get(X, Y, B, steps):
        if (X, Y, B, steps) not in made:
            made[(X, Y, B, steps)] = Stepped(pkg, X, Y, B + 1, steps)
        return made[(X, Y, B, steps)]

    yield get
    for s in made.values():
        s.ens.close()


def want_for(t, field, B, rect, members=None):
    x, y, w, h = rect
    sel = list(range(B)) if members is None else members
    return reference(cut(t.fields[field][:B], x, y, w, h), cut(t.walls[:B], x, y, w, h), cut([t.fields[field][B]], x, y, w, h)[0], cut([t.walls[B]], x, y, w, h)[0], sel)


SIZES = [(57, 9, 1), (57, 9, 2), (57, 9, 3), (57, 9, 5), (57, 9, "L"), (130, 50, 5), (505, 77, 3)]


@pytest.mark.parametrize("X,Y,B", SIZES, ids=[f"{x}x{y}x{b}" for x, y, b in SIZES])
def test_device_equals_host_equals_definition(pkg, stepped, X, Y, B):
    B = limit(pkg) if B == "L" else B
    t = stepped(X, Y, B, STEPS[Y])
    sel = list(range(B))
    most_bins = 0
    for field in STAT_FIELDS:
        for k, rect in enumerate(rectangles(X, Y)):
            x, y, w, h = rect
            want = want_for(t, field, B, rect)
            got = t.ens.scores(field, t.ens[B], x, y, w, h, members=sel, want=MAPS)
            assert got["error"].shape == (h, w, 4) and got["n_scored"].dtype == np.int64 and got["rank_low"].shape == (4, 65)
            check(got, want, (field, rect))
            host = pkg.engine.ens_score_cells(cut(t.fields[field][:B], *rect), cut(t.walls[:B], *rect), cut([t.fields[field][B]], *rect)[0], cut([t.walls[B]], *rect)[0])
            check(host, want, (field, rect, "host function"))
            if k == 0:  # the whole grid: the members are different simulations on different terrain, so the scores are not trivial
                print(field, (X, Y, B), "n_scored", want["n_scored"], "of", w * h, "n_overflow", want["n_overflow"], "bins", (want["rank_low"] > 0).sum(1))
                assert (2 * want["n_scored"] >= w * h).all() and (want["n_overflow"] == 0).all()
                assert (want["sum_crps"] > 0).any() and (want["sum_variance"] > 0).any() == (B > 1)
                most_bins = max(most_bins, int((want["rank_low"] > 0).sum(1).max()))
        # without the maps: the same scalars, and no map in the answer
        some = t.ens.scores(field, t.ens[B], members=sel)
        assert set(some) == set(ALL) - set(MAPS)
        check(some, scalars(want_for(t, field, B, (0, 0, X, Y))), (field, "scalars only"))
    if B >= 5:  # the rank histogram is one, and somewhere some members have a wall cell where others do not
        n_wall = np.sum([a[..., 1] == 0 for a in t.walls[:B]], 0)
        assert most_bins >= 3 and ((n_wall > 0) & (n_wall < B)).any()


def test_truth_as_a_lone_handle_and_as_a_member_of_another_ensemble(pkg):
    """The same simulation held three ways gives the same bits: as member 5 of the ensemble, as a lone handle on its own stream, and as
    a member of a second ensemble -- each with a step PENDING on its stream when the call comes: the call orders itself behind it."""
    E, P = pkg.engine, pkg.params
    X, Y, B = 57, 9, 5
    specs = member_specs(pkg, X, Y, B + 1)
    ens = make_ensemble(pkg, specs)
    other = make_ensemble(pkg, [specs[0], specs[B]])
    s = specs[B]
    lone = E.Handle(X, Y)
    try:
        lone.upload(s["base"], s["water"], s["wall"])
        lone.iter = s.get("iter0", 0)
        lone.set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
        rect = (3, 1, 50, 7)
        for field in STAT_FIELDS:
            ens.step(1), lone.step(1), other.step(1)  # no sync on any of the three streams
            a = ens.scores(field, lone, members=range(B), want=MAPS)
            b = ens.scores(field, other[1], *rect, members=range(B), want=MAPS)
            inside = ens.scores(field, ens[B], members=range(B), want=MAPS)
            f, w = [m.read_rect(field) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
            assert same_bits(lone.read_rect(field), f[B]) and same_bits(other[1].read_rect(field), f[B]) and lone.iter == ens[B].iter == other[1].iter
            check(inside, reference(f[:B], w[:B], f[B], w[B]), (field, "definition"))
            check(a, inside, (field, "lone handle"))
            check(b, reference(cut(f[:B], *rect), cut(w[:B], *rect), cut([f[B]], *rect)[0], cut([w[B]], *rect)[0]), (field, "member of another ensemble"))
            assert (inside["n_scored"] > 0).all()
            lone.step(1)  # the lone truth one iteration ahead, pending: the answer is the one against ITS state
            ahead = ens.scores(field, lone, members=range(B), want=MAPS)
            check(ahead, reference(f[:B], w[:B], lone.read_rect(field), lone.read_rect("WALL_CUR")), (field, "the truth stepped alone"))
            assert not same_bits(ahead["error"], inside["error"])
            ens.step(1), other.step(1)
    finally:
        ens.close()
        other.close()
        lone.close()


PX, PY = 57, 9  # the grid `planted` is laid out on: its cell i is (y, x) = divmod(i, PX)


def uploaded_planted(pkg, B):
    """planted(B, 57 * 9) -- its planted cells and the separating cells in front (rows 0 and 1), random float bit patterns and random
    walls behind -- uploaded as BASE and as WATER of B + 1 members (member B is the truth); nothing is stepped."""
    (f, w), (tf, tw) = planted(B, PX * PY)
    ens = pkg.engine.Ensemble(B + 1, PX, PY, 0)
    for i in range(B + 1):
        fi, wi = (f[i], w[i]) if i < B else (tf, tw)
        ens[i].upload(fi.reshape(PY, PX, 4), fi.reshape(PY, PX, 4), wi.reshape(PY, PX, 4))
    return ens


@pytest.mark.parametrize("B,members", [CASES[k] for k in (2, 4, 5, 6)] + [(70, CASES[7][1])], ids=["3", "7", "7-masked", "64", "70-masked"])
def test_planted_cells(pkg, B, members):
    """Nothing is stepped: the cells for every reason a cell-channel is not scored (the truth on a wall, NaN, Inf; no member's value
    enters; FLT_MAX members against a -FLT_MAX truth), ties with the truth on the tie, -0.0 against +0.0, identical members equal to the
    truth, magnitudes from 1e-38 to 1e38 in one rectangle, and the separating cells."""
    (f, w), (tf, tw) = planted(B, PX * PY)
    ens = uploaded_planted(pkg, B)
    try:
        shape = lambda d: {k: (v.reshape(PY, PX, 4) if k in MAPS else v) for k, v in d.items()}  # noqa: E731
        want = shape(reference(f, w, tf, tw, members))
        sel = range(B) if members is None else members
        for field in STAT_FIELDS:
            assert all(same_bits(ens[i].read_rect(field), f[i].reshape(PY, PX, 4)) for i in range(B))
            got = ens.scores(field, ens[B], members=sel, want=MAPS)
            check(got, want, ("planted", field))
        check(shape(pkg.engine.ens_score_cells(f, w, tf, tw, members=members)), want, "planted, host")
        assert (want["n_truth_excluded"] > 0).all() and (want["n_empty"] > 0).all() and want["n_overflow"][0] > 0 and (want["n_scored"] > 0).all()
        assert (want["rank_low"] != want["rank_high"]).any() and want["crps"][0, 0, 2].view(np.uint32) == 0
        if {0, 1, 2, 3, 4, 5, 6, 7} <= set(sel):
            for cell, which, _, _, defined, fused in separating_cells():
                assert (got[which][cell // PX, cell % PX].view(np.uint32) == defined).all() and defined != fused, cell
    finally:
        ens.close()


def test_mutation_the_crps_weight_is_2i_minus_n_plus_1(pkg):
    """(Named for the hand mutation `2*i - n` of DESIGN.md section 4.) Members 0 and 3 against a truth of 1 in every air cell:
    crps = 1.5 - 3 / 4 = 0.75 on the device (1.0 with the weights -2 and 0)."""
    X, Y = 57, 9
    b, wt, wl = I.impulse_scene(X, Y, "smoke", seed=1)[:3]
    ens = pkg.engine.Ensemble(3, X, Y, 0)
    try:
        for i, v in enumerate((0.0, 3.0, 1.0)):
            ens[i].upload(np.full_like(b, v), wt, wl)
        got = ens.scores("BASE_CUR", ens[2], members=[0, 1], want=("crps",))
        air = wl[..., 1] != 0
        assert air.any() and (got["crps"][air] == 0.75).all() and np.isnan(got["crps"][~air]).all() and (got["sum_crps"] == 0.75 * air.sum()).all()
    finally:
        ens.close()


def test_mutation_rank_high_counts_the_ties(pkg):
    """(Named for the hand mutation `rank_high[n_below]` of DESIGN.md section 4.) 1, 2, 2, 3 against a truth of 2 in every air cell:
    one below, two equal, on the device."""
    X, Y = 57, 9
    b, wt, wl = I.impulse_scene(X, Y, "smoke", seed=1)[:3]
    ens = pkg.engine.Ensemble(5, X, Y, 0)
    try:
        for i, v in enumerate((1.0, 2.0, 2.0, 3.0, 2.0)):
            ens[i].upload(np.full_like(b, v), wt, wl)
        got = ens.scores("BASE_CUR", ens[4], members=[0, 1, 2, 3])
        n = int((wl[..., 1] != 0).sum())
        assert n > 0 and (got["rank_low"][:, 1] == n).all() and (got["rank_high"][:, 3] == n).all() and got["rank_low"].sum() == 4 * n == got["rank_high"].sum()
    finally:
        ens.close()


def test_masks_and_a_single_member(pkg, stepped):
    t = stepped(57, 9, 5, STEPS[9])  # six members
    for field in STAT_FIELDS:
        f, w = t.fields[field], t.walls
        check(t.ens.scores(field, t.ens[5], members=[0, 2, 4], want=MAPS), reference(f, w, f[5], w[5], [0, 2, 4]), (field, "members 0, 2, 4"))
        got = t.ens.scores(field, t.ens[1], 3, 2, 52, 4, members=np.array([True, False, True, False, True, False]), want=MAPS)
        check(got, reference(cut(f, 3, 2, 52, 4), cut(w, 3, 2, 52, 4), cut([f[1]], 3, 2, 52, 4)[0], cut([w[1]], 3, 2, 52, 4)[0], [0, 2, 4]), (field, "boolean mask, truth 1"))
        check(t.ens.scores(field, t.ens[5], want=MAPS), reference(f, w, f[5], w[5], [0, 1, 2, 3, 4]), (field, "members=None leaves the truth out"))
        one = t.ens.scores(field, t.ens[0], members=[3], want=MAPS)
        check(one, reference(f, w, f[0], w[0], [3]), (field, "member 3 alone"))
        scored = ~np.isnan(one["crps"])
        assert scored.any() and (one["variance"][scored] == 0).all() and same_bits(one["crps"][scored], np.abs(one["error"][scored]))


def test_ordered_behind_a_pending_step(pkg):
    """scores directly after step(3), no sync in between: the numbers are those of the state AFTER the three iterations."""
    ens = make_ensemble(pkg, member_specs(pkg, 57, 9, 6))
    try:
        seen = []
        for field in STAT_FIELDS:
            ens.step(3)
            got = ens.scores(field, ens[5], want=MAPS)
            f, w = [m.read_rect(field) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
            check(got, reference(f[:5], w[:5], f[5], w[5]), (field, "directly behind step(3)"))
            seen.append(ens.scores("WATER_CUR", ens[5], want=("error",))["error"])
            assert np.isfinite(seen[-1]).any()
        assert not same_bits(seen[0][:3], seen[1][:3])  # (the iterations in between change the state: an unordered read would show)
        assert [m.iter for m in ens.members] == [s.get("iter0", 0) + 6 for s in member_specs(pkg, 57, 9, 6)]
    finally:
        ens.close()


def test_changes_nothing(pkg):
    """Every readable field, the diagnostics, the iteration counters and wx_ensemble_stats are the same before and after score calls,
    and five further iterations still equal lone handles that never saw the calls."""
    t = Twins(pkg, member_specs(pkg, 57, 9, 5))
    try:
        t.step(2)

        def snapshot():
            return ([[m.read_rect(f) for f in FIELDS] for m in t.ens.members], t.ens.diagnostics(), [m.iter for m in t.ens.members], t.ens.stats())

        a = snapshot()
        for field in STAT_FIELDS:
            t.ens.scores(field, t.ens[2], want=MAPS)
            t.ens.scores(field, t.ens[0], 3, 2, 40, 5, members=[1, 3], want=("crps",))
        b = snapshot()
        for i in range(5):
            for k, f in enumerate(FIELDS):
                assert same_bits(a[0][i][k], b[0][i][k]), (i, f)
            assert same_diag(a[1][i], b[1][i]) is None, i
        assert a[2] == b[2] and a[3] == b[3]
        t.ens.scores("BASE_CUR", t.ens[4])  # ... and directly in front of a step
        t.step(5)
        t.compare("after score calls")
    finally:
        t.close()


def test_members_with_droplets(pkg, golden):
    """Ensemble(4, 64, 64, 400), deterministic splat order, precipitation on: WATER_CUR after 16 iterations, member 3 the truth."""
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
        got = ens.scores("WATER_CUR", ens[3], want=MAPS)
        f, w = [m.read_rect("WATER_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        want = reference(f[:3], w[:3], f[3], w[3])
        check(got, want, "droplets")
        check(ens.scores("WATER_CUR", ens[0], 5, 7, 50, 41, members=[1, 2], want=MAPS),
              reference(cut(f, 5, 7, 50, 41), cut(w, 5, 7, 50, 41), cut([f[0]], 5, 7, 50, 41)[0], cut([w[0]], 5, 7, 50, 41)[0], [1, 2]), "droplets, rectangle")
        assert ens.particle_stats()["member_iters_particles_batched"] == 4 * 16
        assert (want["sum_variance"] > 0).any() and any(np.abs(m.read_rect("PRECIP_FB")).max() > 0 for m in ens.members)
    finally:
        ens.close()


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_scores_gpu as T
out = {}
for B in (8, 64):  # planted uploads, the separating cells among them: the device and the host function of this build
    ens = T.uploaded_planted(pkg, B)
    (f, w), (tf, tw) = T.planted(B, T.PX * T.PY)
    for field in ("BASE_CUR", "WATER_CUR"):
        for k, v in ens.scores(field, ens[B], members=range(B), want=T.MAPS).items():
            out[f"{B}_{field}_{k}"] = v
    for k, v in pkg.engine.ens_score_cells(f, w, tf, tw).items():
        out[f"{B}_host_{k}"] = v
    ens.close()
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernel and its host function give the definition's
    bits on the planted uploads -- the separating cells are the only data on which a product that the code generator fused into its sum
    would show in a float32 --, which are also THIS process's host function's."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    dst = str(tmp_path / "fast.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, root, dst], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(dst)
    for B in (8, 64):
        (f, w), (tf, tw) = planted(B, PX * PY)
        want = reference(f, w, tf, tw)
        check(pkg.engine.ens_score_cells(f, w, tf, tw), want, (B, "exact host vs definition"))
        check({k: d[f"{B}_host_{k}"] for k in ALL}, want, (B, "fast host vs definition"))
        for field in STAT_FIELDS:
            got = {k: (d[f"{B}_{field}_{k}"].reshape(PX * PY, 4) if k in MAPS else d[f"{B}_{field}_{k}"]) for k in ALL}
            check(got, want, (B, field, "fast device vs definition"))
            for cell, which, _, _, defined, fused in separating_cells():
                assert (got[which][cell].view(np.uint32) == defined).all() and defined != fused, (B, field, cell)


def test_refusals(pkg):
    E, P = pkg.engine, pkg.params
    X, Y = 57, 9
    specs = member_specs(pkg, X, Y, 4)
    ens = make_ensemble(pkg, specs[:3] + [None])  # member 3 is never uploaded
    small, slab, never = E.Handle(X + 7, Y), E.Handle(X - 16, Y, X_global=X, x0=8, halo=8), E.Handle(X, Y)
    try:
        def refused(code, *a, **kw):
            with pytest.raises(E.WxError) as ei:
                ens.scores(*a, **kw)
            assert ei.value.code == code, (a, kw, str(ei.value))
            return str(ei.value)

        two = dict(members=[0, 1])
        msg = refused(-1, "CURL", ens[2], **two)
        assert "WX_FIELD_BASE_CUR" in msg and "WX_FIELD_WATER_CUR" in msg
        for f in ("WALL_CUR", "BASE_DISP", "WATER_0", "LIGHT_0", "EMITTED"):
            refused(-1, f, ens[2], **two)
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (X, 0, 1, 1)):
            assert "outside" in refused(-4, "BASE_CUR", ens[2], *rect, **two)
        st, mask = E.WxEnsScore(), np.array([1, 1, 0, 0], np.uint8)  # a NULL truth, a NULL struct with a valid ensemble
        assert E.lib().wx_ensemble_scores(ens._e, None, E.FIELD_IDS["BASE_CUR"], 0, 0, X, Y, mask.ctypes.data, C.byref(st)) == -1
        assert E.lib().wx_ensemble_scores(ens._e, ens[2]._h, E.FIELD_IDS["BASE_CUR"], 0, 0, X, Y, mask.ctypes.data, None) == -1
        assert "nobody" in refused(-1, "BASE_CUR", ens[2], members=[])
        refused(-1, "BASE_CUR", ens[2], members=np.zeros(4, bool))
        assert "selected" in refused(-1, "BASE_CUR", ens[1], **two)             # the truth is a selected member
        assert "slab" in refused(-1, "BASE_CUR", slab, **two)
        assert "cells" in refused(-1, "BASE_CUR", small, **two)                  # a truth of another size
        assert "member 3" in refused(-5, "BASE_CUR", ens[2], members=[0, 3])     # a selected member never uploaded
        assert "truth" in refused(-5, "BASE_CUR", never, **two)                  # a truth never uploaded
        assert "truth" in refused(-5, "BASE_CUR", ens[3], **two)
        big = E.Ensemble(66, X, Y, 0)  # 65 selected: refused before anything is looked at (nobody is uploaded)
        try:
            with pytest.raises(E.WxError) as ei:
                big.scores("BASE_CUR", big[65])
            assert ei.value.code == -1 and "64" in str(ei.value)
        finally:
            big.close()
        # the ensemble works as before
        f, w = [ens[i].read_rect("BASE_CUR") for i in range(3)], [ens[i].read_rect("WALL_CUR") for i in range(3)]
        check(ens.scores("BASE_CUR", ens[2], want=MAPS, **two), reference(f[:2], w[:2], f[2], w[2]), "two of four")
        s = specs[3]
        ens[3].upload(s["base"], s["water"], s["wall"])
        ens[3].set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
        ens.step(2)
        f, w = [m.read_rect("WATER_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        check(ens.scores("WATER_CUR", ens[3], want=MAPS), reference(f[:3], w[:3], f[3], w[3]), "all four")
    finally:
        ens.close()
        for h in (small, slab, never):
            h.close()


def test_an_overflowed_list_surfaces_here(pkg):
    """WX_OPT_FIX_CAP 2 on a member with fast cells: its report (WX_E_STATE) is what the score call returns, naming the member -- once."""
    E = pkg.engine
    X, Y = 505, 77
    fast = I.impulse_scene(X, Y, "fast_vx")
    specs = member_specs(pkg, X, Y, 3)
    specs[1] = dict(base=fast[0], water=fast[1], wall=fast[2], u=I.scene_uniforms("fast_vx", Y), options={E.Handle.OPT_FIX_CAP: 2})
    ens = make_ensemble(pkg, specs)
    try:
        ens.step(2)
        with pytest.raises(E.WxError) as ei:
            ens.scores("BASE_CUR", ens[2])
        assert ei.value.code == -5 and "member 1: " in str(ei.value), str(ei.value)
        got = ens.scores("BASE_CUR", ens[2], want=MAPS)  # the report was consumed
        f, w = [m.read_rect("BASE_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        check(got, reference(f[:2], w[:2], f[2], w[2]), "after the report")
    finally:
        ens.close()


def test_weather_ensemble_scores(pkg):
    """WeatherEnsemble.from_sim -> perturb -> step -> scores against the nature run; the profile names the kernel."""
    W = pkg.sim
    X, Y, B = 128, 48, 5
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    sim = W.WeatherSim(X, Y, base, water, wall, None, {"dayNightCycle": False}, sun_angle_deg=30.0)
    sim.verbose = False
    we = None
    try:
        sim.step(6)
        we = W.WeatherEnsemble.from_sim(sim, B)
        we.perturb("BASE_CUR", (0.0, 0.0, 0.0, 0.5), scale=8, seed=3)
        we.step(2)
        sim.step(2)
        we.engine[0].profile(True)
        out = we.scores("BASE_CUR", sim, want=("crps",))
        prof = we.engine[0].profile_read()
        assert prof["ensemble_scores"][1] == 1 and prof["ensemble_scores"][0] > 0
        raw = we.engine.scores("BASE_CUR", sim.handle, want=("crps",))
        check({k: out[k] for k in raw if k != "crps"}, {k: raw[k] for k in raw if k != "crps"}, "pass-through")
        assert same_bits(out["maps"]["crps"], raw["crps"]) and set(out["maps"]) == {"crps"}
        n = raw["n_scored"].astype(np.float64)
        assert (n > 0).all() and same_bits(out["bias"], raw["sum_error"] / n) and same_bits(out["mae"], raw["sum_abs_error"] / n)
        assert same_bits(out["rmse"], np.sqrt(raw["sum_sq_error"] / n)) and same_bits(out["spread"], np.sqrt(raw["sum_variance"] / n))
        assert same_bits(out["crps"], raw["sum_crps"] / n) and same_bits(out["rank_histogram"], (raw["rank_low"] + raw["rank_high"]) / 2.0)
        assert out["spread"][3] > 0 and out["rmse"][3] > 0 and (out["rank_histogram"].sum(1) == n).all()
        inside = we.scores("WATER_CUR", we[4], 2, 3, 20, 10)  # a member as the truth: the others are scored
        assert (inside["sum_count"] == 4 * inside["n_scored"]).all()
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
