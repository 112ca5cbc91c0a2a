"""Ensemble scores against a truth (wx_ensemble_scores, wx_ens_score_cells, wx_ens_score_max_members; include/wxsim.h) without a GPU:
the header announces and declares the addition at the unchanged ABI version, both libraries export it, the argument checks answer
before any device is touched, and the pure host entry point -- the kernel's own per-cell function and wx_diag's integer bins -- equals
the definition in the header comment, which `reference` below writes down with np.sort over the member axis, float64 arithmetic with
ONE numpy operation per rounded operation, and math.fsum over the per-cell float32 values for the domain sums (deliberately not the
library's bins). Every comparison is `==` on bits, NaNs compared as positions."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_ensemble_statistics_cpu import FLT_MAX, hand_built, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_scores", "wx_ens_score_cells", "wx_ens_score_max_members"]
COUNTS = ("n_scored", "n_truth_excluded", "n_empty", "n_overflow", "sum_count")
SUMS = ("sum_error", "sum_abs_error", "sum_sq_error", "sum_variance", "sum_crps")
MAPS = ("error", "variance", "crps")
ALL = COUNTS + SUMS + ("rank_low", "rank_high") + MAPS
BINS = 65
E_INVALID = -1


def reference(fields, walls, truth_field, truth_wall, members=None, fuse=None):
    """The definition of include/wxsim.h, straight from its text. fields[i]: float32 (..., 4), walls[i]: int8 (..., 4), the truth's
    likewise; members: the selected member indices (None: all). Returns every entry of wx_ens_score, the maps in the arrays' shape.
    fuse ("Q" or "G", the separating cells' test only): that product contracted into its sum, evaluated exactly and rounded once."""
    sel = sorted(range(len(fields)) if members is None else members)
    v = np.stack([np.asarray(fields[i], np.float32) for i in sel])
    is_wall = np.stack([np.asarray(walls[i])[..., 1] == 0 for i in sel])
    tf = np.asarray(truth_field, np.float32)
    take = ~is_wall[..., None] & np.isfinite(v)
    n = take.sum(0)
    with np.errstate(all="ignore"):
        entered = np.where(take, np.where(v == 0, np.float32(0), v), np.float32(np.inf))  # an entered -0.0 is taken as +0.0
        s = np.sort(entered, axis=0).astype(np.float64)  # v(0) <= ... <= v(n-1) in front, what did not enter behind
        t_ok = (np.asarray(truth_wall)[..., 1] != 0)[..., None] & np.isfinite(tf)
        t = np.where(tf == 0, np.float32(0), tf).astype(np.float64)
        nd = n.astype(np.float64)
        zero = np.zeros(n.shape, np.float64)
        S = zero
        for i in range(len(sel)):  # ascending order, i = 0 first; the sums start at +0.0, so a + 0.0 for i >= n changes no bit
            S = S + np.where(i < n, s[i], 0.0)
        m = S / nd
        Q, A, G = zero, zero, zero
        for i in range(len(sel)):
            inside = i < n
            d = s[i] - m
            u = s[i] - t
            k = (2 * i - n + 1).astype(np.float64)
            if fuse == "Q":
                Q = np.where(inside, _fma(d, d, Q), Q)
            else:
                dd = d * d
                Q = Q + np.where(inside, dd, 0.0)
            A = A + np.where(inside, np.abs(u), 0.0)
            if fuse == "G":
                G = np.where(inside, _fma(k, u, G), G)
            else:
                ku = k * u
                G = G + np.where(inside, ku, 0.0)
        err = m - t
        var = Q / nd
        a = A / nd
        nn = nd * nd
        g = G / nn
        crps = a - g
        sq = err * err
        five = [x.astype(np.float32) for x in (err, np.abs(err), sq, var, crps)]
        below, equal = (take & (v < tf)).sum(0), (take & (v == tf)).sum(0)
    finite = np.all([np.isfinite(x) for x in five], axis=0)
    reason = np.where(~t_ok, 1, np.where(n < 1, 2, np.where(~finite, 3, 0)))
    scored = reason == 0
    out = {}
    for q, name in enumerate(("n_scored", "n_truth_excluded", "n_empty", "n_overflow")):
        out[name] = np.array([(reason[..., c] == q).sum() for c in range(4)], np.int64)
    out["sum_count"] = np.array([n[..., c][scored[..., c]].sum() for c in range(4)], np.int64)
    for name, x in zip(SUMS, five):
        out[name] = np.array([math.fsum(float(y) for y in x[..., c][scored[..., c]]) for c in range(4)], np.float64)
    out["rank_low"] = np.stack([np.bincount(below[..., c][scored[..., c]], minlength=BINS) for c in range(4)]).astype(np.int64)
    out["rank_high"] = np.stack([np.bincount((below + equal)[..., c][scored[..., c]], minlength=BINS) for c in range(4)]).astype(np.int64)
    for name, x in zip(MAPS, (five[0], five[3], five[4])):
        out[name] = np.where(scored, x, np.float32(np.nan)).astype(np.float32)
    return out


def _fma(a, b, c):
    """fma(a, b, c) element by element in exact rational arithmetic, rounded once; c where a, b or c is not finite."""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.array(c, np.float64)
    for idx in np.ndindex(a.shape):
        if np.isfinite(a[idx]) and np.isfinite(b[idx]) and np.isfinite(c[idx]):
            out[idx] = float(Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx])))
    return out


def check(got, want, where):
    assert set(got) == set(want), (where, sorted(got), sorted(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert same_bits(g, w), (where, k, g if g.size <= 8 else np.argwhere(~(g == w) & ~(np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64))))[:5].tolist(),
                                 w if w.size <= 8 else None)


def scalars(d):
    return {k: v for k, v in d.items() if k not in MAPS}


# SEPARATING CELLS: small member sets (and a truth) on which a build that contracts d_i * d_i into Q, or (2i - n + 1) * u_i into G,
# computes ANOTHER float32 vr / cr than the definition's separately rounded product and sum. Printed by
# `python tools/find_score_separators.py --seed 1` (numpy and exact rational arithmetic, no build of the library), not searched for at
# test time. The cr cells have the truth far above four small graded members, so that G's partial sums cancel in the last step of the
# walk: only there does a fused product show. err * err feeds a conversion and no sum: there is nothing to fuse it with, so it has no
# separating cell.
# (entered values' float32 bits in member order, the truth's, float32 bits of the defined result, of the fused result)
VARIANCE_SEPARATORS = [
    ([0x3FD00B9D, 0x40251FDF, 0xC03023EF, 0x3082F916, 0x359A44AF], 0x4014479F, 0x405291C0, 0x405291C1),
    ([0x4046B358, 0x3FF0CD50, 0x308CECE2, 0x35FA9D72, 0x3FF2D630], 0xC0584492, 0x3FBAEEA4, 0x3FBAEEA3),
    ([0x405BA7DB, 0x4042BDD0, 0x35ECB6FA, 0x30A282AB, 0x3FA0776F, 0x3FB9F4F6, 0x401A6133], 0x40383ACE, 0x3FCF50D1, 0x3FCF50D2),
]
CRPS_SEPARATORS = [
    ([0xB5EEE083, 0xB38A7A32, 0x31AC069B, 0x31C87879], 0x4073F144, 0x4073F144, 0x4073F145),
    ([0xB5E9ED96, 0xB3A555EC, 0x3185C5BE, 0x31E6F9ED], 0x406483B4, 0x406483B4, 0x406483B5),
    ([0xB5EAD44F, 0xB39FC1FE, 0x31AD39FE, 0x31C581CE], 0x406D7F7D, 0x406D7F7E, 0x406D7F7D),
    ([0xB5F1094D, 0xB386DA7D, 0x31AC6D83, 0x31FE4DD7], 0x405CF8E1, 0x405CF8E2, 0x405CF8E1),
]
SEP_FIRST = 24  # the cells of `planted` the separating cells occupy: SEP_FIRST .. (behind the quantile tests' 20 .. 23)
SEP_MEMBERS = 8  # members 0 .. 7 hold a separating cell's values (NaN behind its last): complete in every selection that holds them
SEP_CASES = [(8, None), (70, [i for i in range(70) if i not in (10, 11, 33, 45, 50, 69)])]  # ... as these two do


def separating_cells():
    """[(cell, which map, values, truth, defined, fused)]"""
    cells = [("variance",) + c for c in VARIANCE_SEPARATORS] + [("crps",) + c for c in CRPS_SEPARATORS]
    return [(SEP_FIRST + k, c[0], c[1], c[2], c[3], c[4]) for k, c in enumerate(cells)]


def planted(B, n_cells=64):
    """`hand_built` of the statistics test for B + 1 members -- random float bit patterns, random walls, its planted cells: all equal
    (0), subnormals with FLT_MAX (2), NaN / +Inf / -Inf among finite values (3), every member non-finite (4), every member wall (5), wall
    in some members only (6), -0.0 against +0.0 (7), ties (8) -- where member B is the TRUTH. Its planted cells: on the values (0: below
    all, above all, equal to all -- crps exactly +0.0 --, -Inf), a wall (1), NaN / +-FLT_MAX / 0 (2), on the ties (8), -0.0 and +0.0 against
    zeros of both signs (14), an overflow -- FLT_MAX members against a -FLT_MAX truth -- (15), one entered value (11), values from 1e-38 to
    1e38 in the cells from 32 on, and the separating cells from SEP_FIRST on. Returns (fields, walls) of the B members and the truth's."""
    f, w = hand_built(B + 1, n_cells)
    f, w = [a.copy() for a in f], [a.copy() for a in w]
    for i in range(B):
        w[i][11, 1] = 7 if i == 0 else 0
        f[i][11] = np.float32([3.5, -0.0, 1e-45, -FLT_MAX])
        f[i][14] = np.float32([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0][i % 6])
        w[i][14, 1] = 9
        f[i][15] = np.float32([FLT_MAX, FLT_MAX, -FLT_MAX, 1.0])
        w[i][15, 1] = 9
    r = f[B]
    w[B][[0, 2, 4, 5, 8, 11, 14, 15], 1] = 3
    r[4] = r[5] = np.float32(1.0)                 # a good truth where no member's value enters
    r[0] = np.float32([1.0, 2.0, 1.5, -np.inf])   # against 1.5 everywhere: below all, above all, equal to all, not finite
    w[B][1, 1] = 0                                # on a wall
    r[2] = np.float32([np.nan, FLT_MAX, -FLT_MAX, 0.0])
    r[8] = np.float32([-7.0, 9.0, 5.0, 4.999])    # equal to the tied minimum / maximum (B >= 3), to every member, below all
    r[11] = np.float32([3.5, 0.0, 0.0, FLT_MAX])  # n = 1: equal, equal (-0.0 == +0.0), a subnormal error, a squared error that overflows
    r[14] = np.float32([-0.0, 0.0, 1e-45, np.inf])
    r[15] = np.float32([-FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX])  # error 2 FLT_MAX: overflow; equal: scored; equal; a finite error whose square is not
    rng = np.random.Generator(np.random.Philox(77 + B))
    for cell in range(32, min(n_cells, 48)):      # any magnitude in one rectangle: the exact sum at work
        mag = np.float32(10.0) ** np.float32(rng.integers(-38, 19))
        for i in range(B + 1):
            f[i][cell] = (rng.standard_normal(4) * mag).astype(np.float32)
            w[i][cell, 1] = 5
    for cell, _, values, t, _, _ in separating_cells():
        if cell < n_cells:
            for i in range(B):
                f[i][cell] = np.uint32(values[i] if i < len(values) else 0x7FC00000).view(np.float32)
                w[i][cell, 1] = 5
            r[cell] = np.uint32(t).view(np.float32)
            w[B][cell, 1] = 5
    return (f[:B], w[:B]), (f[B], w[B])


CASES = [(1, None), (2, None), (3, None), (5, None), (7, None), (7, [0, 2, 3, 6]), (64, None), (70, [i for i in range(70) if i not in (0, 7, 33, 45, 50, 69)])]
IDS = ["1", "2", "3", "5", "7", "7-masked", "64", "70-masked"]


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_SCORES\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ENS_SCORE_BINS\s+65\b", hdr, re.M)
    E, L = pkg.engine, pkg.engine.lib()
    for n in NAMES:  # (libwxsim_fast.so's exports: the child process of test_the_tolerance_build_gives_the_same_bits looks them up)
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in E.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert callable(E.Ensemble.scores) and callable(pkg.sim.WeatherEnsemble.scores) and callable(E.ens_score_cells)
    assert "ensemble_scores" in [L.wx_kernel_name(k).decode() for k in range(L.wx_kernel_count())]
    assert L.wx_ens_score_max_members() == L.wx_ens_quant_staged_members() == E.Ensemble.SCORE_MAX_MEMBERS == 64 == E.ENS_SCORE_BINS - 1
    # the ctypes struct is the header's, member for member
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct wx_ens_score {"):hdr.index("} wx_ens_score;")].split("{", 1)[1], flags=re.S)
    names = [re.sub(r"[\*\s]|\[.*\]", "", n) for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(float|double|int64_t)\b", "", decl.strip()).split(",")]
    assert names == [f[0] for f in E.WxEnsScore._fields_] == list(ALL)
    assert C.sizeof(E.WxEnsScore) == 5 * 32 + 5 * 32 + 2 * 4 * BINS * 8 + 3 * 8 and E.WxEnsScore.error.offset == 320 + 8 * 4 * BINS * 2


def test_argument_checks_answer_without_a_device(pkg):
    L, E = pkg.engine.lib(), pkg.engine
    (f, w), (tf, tw) = planted(3, 16)
    fp, wp = (C.c_void_p * 3)(*[a.ctypes.data for a in f]), (C.c_void_p * 3)(*[a.ctypes.data for a in w])
    err = np.full((16, 4), -77, np.float32)

    def struct():
        st = E.WxEnsScore()
        st.error = err.ctypes.data
        st.n_scored[0] = -77
        return st

    good = struct()
    # the device entry point: NULL handles and a NULL struct answer before anything is looked at
    assert L.wx_ensemble_scores(None, None, 0, 0, 0, 1, 1, None, C.byref(good)) == E_INVALID
    assert L.wx_ensemble_scores(None, None, 0, 0, 0, 1, 1, None, None) == E_INVALID
    nobody, two = (C.c_uint8 * 3)(0, 0, 0), (C.c_uint8 * 3)(1, 0, 1)
    call = lambda st, n=3, fp=fp, wp=wp, t=tf.ctypes.data, twl=tw.ctypes.data, mask=None: L.wx_ens_score_cells(  # noqa: E731
        n, 16, fp, wp, t, twl, mask, None if st is None else C.byref(st))
    assert call(good) == 0 and (err != -77).all() and good.n_scored[0] >= 0
    err[:] = -77
    bad = struct()
    assert call(None) == E_INVALID
    assert call(bad, mask=nobody) == E_INVALID
    assert call(bad, n=0) == E_INVALID and call(bad, n=-1) == E_INVALID
    assert call(bad, fp=None) == E_INVALID and call(bad, wp=None) == E_INVALID
    assert call(bad, t=None) == E_INVALID and call(bad, twl=None) == E_INVALID
    hole = (C.c_void_p * 3)(f[0].ctypes.data, None, f[2].ctypes.data)
    assert call(bad, fp=hole) == E_INVALID                       # a selected member without cells
    assert (err == -77).all() and bad.n_scored[0] == -77         # a refused call writes nothing
    assert call(bad, fp=hole, mask=two) == 0 and bad.n_scored[0] >= 0  # an unselected one may be absent
    for kw in (dict(members=[]), dict(members=np.zeros(3, bool))):
        with pytest.raises(E.WxError) as ei:
            E.ens_score_cells(f, w, tf, tw, **kw)
        assert ei.value.code == E_INVALID, kw
    with pytest.raises(KeyError):
        E.ens_score_cells(f, w, tf, tw, want=("error", "median"))
    with pytest.raises(ValueError):
        E.ens_score_cells(f, w, tf[:8], tw[:8])
    assert set(E.ens_score_cells(f, w, tf, tw, want=())) == set(ALL) - set(MAPS)


def test_65_selected_members_are_refused(pkg):
    E = pkg.engine
    (f, w), (tf, tw) = planted(65, 32)
    with pytest.raises(E.WxError) as ei:
        E.ens_score_cells(f, w, tf, tw)
    assert ei.value.code == E_INVALID and "64" in str(ei.value)
    check(E.ens_score_cells(f, w, tf, tw, members=range(1, 65)), reference(f, w, tf, tw, range(1, 65)), "64 of 65")


def test_the_definition_on_values_worked_by_hand(pkg):
    """The reference itself, and the host function, against numbers anybody can check. Members 1, 2, 4, 9 against a truth of 3: mean 4,
    error 1, population variance (9 + 4 + 0 + 25) / 4 = 9.5, mean |x - t| = (2 + 1 + 1 + 6) / 4 = 2.5, sum over pairs |x_i - x_j| =
    1 + 3 + 8 + 2 + 7 + 5 = 26, crps = 2.5 - 26 / 16 = 0.875; two values below the truth, none equal."""
    air = [np.full((1, 4), 5, np.int8)] * 4
    f = [np.full((1, 4), x, np.float32) for x in (9.0, 1.0, 4.0, 2.0)]
    t = np.full((1, 4), 3.0, np.float32)
    want = reference(f, air, t, air[0])
    check(pkg.engine.ens_score_cells(f, air, t, air[0]), want, "by hand")
    assert want["error"][0, 0] == 1.0 and want["variance"][0, 0] == 9.5 and want["crps"][0, 0] == 0.875
    assert want["sum_error"][0] == 1.0 and want["sum_abs_error"][0] == 1.0 and want["sum_sq_error"][0] == 1.0 and want["sum_variance"][0] == 9.5 and want["sum_crps"][0] == 0.875
    assert want["n_scored"].tolist() == [1] * 4 and want["sum_count"].tolist() == [4] * 4
    assert want["rank_low"][0].tolist() == [0, 0, 1] + [0] * 62 == want["rank_high"][0].tolist()
    # one member: crps is the absolute error, the variance 0
    one = reference(f[:1], air[:1], t, air[0])
    check(pkg.engine.ens_score_cells(f[:1], air[:1], t, air[0]), one, "one member")
    assert one["crps"][0, 0] == 6.0 and one["variance"][0, 0] == 0.0 and one["error"][0, 0] == 6.0


def test_mutation_the_crps_weight_is_2i_minus_n_plus_1(pkg):
    """(Named for the hand mutation `2*i - n` of DESIGN.md section 4.) Members 0 and 3 against a truth of 1: mean |x - t| = 1.5,
    G = (-1)(-1) + (1)(2) = 3, crps = 1.5 - 3 / 4 = 0.75 (with the weights -2 and 0 it would be 1.0; members placed symmetrically
    around the truth would not tell the two apart)."""
    air = [np.full((1, 4), 5, np.int8)] * 2
    got = pkg.engine.ens_score_cells([np.full((1, 4), 0.0, np.float32), np.full((1, 4), 3.0, np.float32)], air, np.full((1, 4), 1.0, np.float32), air[0])
    assert got["crps"][0].tolist() == [0.75] * 4 and got["sum_crps"].tolist() == [0.75] * 4


def test_mutation_rank_high_counts_the_ties(pkg):
    """(Named for the hand mutation `rank_high[n_below]` of DESIGN.md section 4.) 1, 2, 2, 3 against a truth of 2: one below, two equal."""
    air = [np.full((1, 4), 5, np.int8)] * 4
    got = pkg.engine.ens_score_cells([np.full((1, 4), x, np.float32) for x in (1.0, 2.0, 2.0, 3.0)], air, np.full((1, 4), 2.0, np.float32), air[0])
    assert (got["rank_low"][:, 1] == 1).all() and (got["rank_high"][:, 3] == 1).all() and got["rank_low"].sum() == 4 == got["rank_high"].sum()


@pytest.mark.parametrize("B,members", CASES, ids=IDS)
def test_host_function_equals_the_definition(pkg, B, members):
    (f, w), (tf, tw) = planted(B)
    got = pkg.engine.ens_score_cells(f, w, tf, tw, members=members)
    want = reference(f, w, tf, tw, members)
    check(got, want, B)
    # the cases are what they claim to be
    sel = list(range(B)) if members is None else members
    n_sel = len(sel)
    sc = lambda m, cell, c: not np.isnan(want[m][cell, c])  # noqa: E731
    assert all(np.isnan(want[m][1]).all() for m in MAPS)                                   # the truth on a wall
    assert np.isnan(want["error"][0, 3]) and np.isnan(want["error"][2, 0])                 # the truth -Inf / NaN
    assert np.isnan(want["error"][5]).all() and np.isnan(want["error"][4]).all()           # every member wall / non-finite: empty
    assert want["error"][0].tolist()[:3] == [0.5, -0.5, 0.0] and (want["variance"][0, :3] == 0).all()
    assert want["crps"][0, 2].view(np.uint32) == 0 and want["crps"][0, 0] == 0.5           # identical members equal to the truth: +0.0
    assert np.isnan(want["error"][15, 0]) and sc("error", 15, 1) and want["error"][15, 1] == 0.0   # 2 FLT_MAX overflows; FLT_MAX - FLT_MAX scores
    assert np.isnan(want["error"][15, 3])                                                  # err = 1 + FLT_MAX is finite, its square is not
    assert want["n_overflow"][0] >= 1 and want["n_overflow"][3] >= 1 and want["n_truth_excluded"][3] >= 2 and (want["n_empty"] >= 1).all()
    assert (want["n_scored"] + want["n_truth_excluded"] + want["n_empty"] + want["n_overflow"] == 64).all()
    assert (want["rank_low"].sum(1) == want["n_scored"]).all() and (want["rank_high"].sum(1) == want["n_scored"]).all()
    assert not (want["crps"].view(np.uint32) == 0x80000000).any()
    if n_sel >= 3:
        assert (want["rank_low"] != want["rank_high"]).any()                               # ties with the truth on the tie
    if 0 in sel:
        assert want["error"][11].tolist()[:3] == [0.0, 0.0, float(np.float32(1e-45))] and np.isnan(want["error"][11, 3])  # n = 1: -0.0 == +0.0, a subnormal error (its square is 0), FLT_MAX^2
    mags = np.abs(want["variance"][32:48][~np.isnan(want["variance"][32:48])]).astype(np.float64)
    if n_sel >= 2:
        assert mags.max() / mags[mags > 0].min() > 1e30


def test_the_exact_sum_is_not_the_running_sum(pkg):
    """Built so that the plain float64 running sum of the per-cell values differs from math.fsum. One member against a truth of 0, so
    the error is the member's value. Errors 2^60, 1, -2^60, 1 in cell order: the running sum loses the first 1. Errors 2^27 and eight
    times 1.5: every 2.25 added to 2^54 is rounded up to 4. The library gives fsum's bits."""
    def run(errs):
        errs = np.float32(errs)
        f = [np.repeat(errs[:, None], 4, 1)]
        w = [np.full((len(errs), 4), 5, np.int8)]
        t = np.zeros((len(errs), 4), np.float32)
        got = pkg.engine.ens_score_cells(f, w, t, w[0])
        check(got, reference(f, w, t, w[0]), "running sum")
        return got

    def running(values):
        r = 0.0
        for e in values:
            r = r + float(e)
        return r

    errs = [2.0 ** 60, 1.0, -2.0 ** 60, 1.0]
    assert run(errs)["sum_error"][0] == math.fsum(errs) == 2.0 != running(errs)
    errs = [2.0 ** 27] + [1.5] * 8
    sq = [e * e for e in errs]
    assert run(errs)["sum_sq_error"][0] == math.fsum(sq) == 2.0 ** 54 + 16.0 != running(sq)  # (18 lies halfway: ties to even)


def test_the_order_of_the_members_does_not_matter(pkg):
    B = 70
    (f, w), (tf, tw) = planted(B)
    members = CASES[7][1]
    rng = np.random.Generator(np.random.Philox(5))
    first = pkg.engine.ens_score_cells(f, w, tf, tw, members=members)
    for _ in range(3):
        perm = rng.permutation(B)  # new position k holds old member perm[k]
        where = {int(old): k for k, old in enumerate(perm)}
        again = pkg.engine.ens_score_cells([f[i] for i in perm], [w[i] for i in perm], tf, tw, members=[where[i] for i in members])
        check(again, first, "permuted")
    # ... nor the order of the cells, in any scalar
    cells = rng.permutation(64)
    again = pkg.engine.ens_score_cells([a[cells] for a in f], [a[cells] for a in w], tf[cells], tw[cells], members=members)
    check(scalars(again), scalars(first), "cells permuted")


def test_separating_cells_separate(pkg):
    """Every committed cell, by exact arithmetic: the definition and the fused evaluation give the committed, DIFFERENT float32 values,
    in both directions for each product; in planted's data `reference` gives the definition's value; and the default library's host
    function equals `reference`."""
    u32 = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    assert len(VARIANCE_SEPARATORS) >= 2 and len(CRPS_SEPARATORS) >= 2
    for which, fuse, cells in (("variance", "Q", VARIANCE_SEPARATORS), ("crps", "G", CRPS_SEPARATORS)):
        above = below = 0
        for values, t, defined, fused in cells:
            assert len(values) <= SEP_MEMBERS
            f = [np.full((1, 4), np.uint32(b).view(np.float32), np.float32) for b in values]
            air = [np.full((1, 4), 5, np.int8)] * len(values)
            tf = np.full((1, 4), np.uint32(t).view(np.float32), np.float32)
            a, b = reference(f, air, tf, air[0])[which][0, 0], reference(f, air, tf, air[0], fuse=fuse)[which][0, 0]
            assert (u32(a), u32(b)) == (defined, fused) and defined != fused, (which, hex(u32(a)), hex(u32(b)))
            above, below = above + (b > a), below + (b < a)
        assert above >= 1 and below >= 1, which
    for B, members in SEP_CASES:
        (f, w), (tf, tw) = planted(B)
        want = reference(f, w, tf, tw, members)
        check(pkg.engine.ens_score_cells(f, w, tf, tw, members=members), want, ("separating", B))
        for cell, which, values, t, defined, fused in separating_cells():
            assert (want[which][cell].view(np.uint32) == defined).all(), (B, cell)


_FAST_LEG = """
import ctypes as C, sys, numpy as np
lib, src, dst = sys.argv[1:4]
L = C.CDLL(lib)
d = np.load(src)
f, w, tf, tw, mask = np.ascontiguousarray(d["f"]), np.ascontiguousarray(d["w"]), np.ascontiguousarray(d["tf"]), np.ascontiguousarray(d["tw"]), np.ascontiguousarray(d["mask"])
B, n = f.shape[:2]
class S(C.Structure):
    _fields_ = ([(k, C.c_int64 * 4) for k in %r] + [(k, C.c_double * 4) for k in %r] + [("rank_low", (C.c_int64 * 65) * 4), ("rank_high", (C.c_int64 * 65) * 4)]
                + [(k, C.c_void_p) for k in %r])
maps = {k: np.zeros((n, 4), np.float32) for k in %r}
st = S()
for k, a in maps.items():
    setattr(st, k, a.ctypes.data)
fp, wp = (C.c_void_p * B)(*[f[i].ctypes.data for i in range(B)]), (C.c_void_p * B)(*[w[i].ctypes.data for i in range(B)])
L.wx_ens_score_cells.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
assert L.wx_arith() == 1, "not the tolerance build"
for name in %r:
    getattr(L, name)
assert L.wx_ens_score_max_members() == 64
assert L.wx_ens_score_cells(B, n, fp, wp, tf.ctypes.data, tw.ctypes.data, mask.ctypes.data, C.byref(st)) == 0
out = dict(maps)
for k, _ in S._fields_[:10]:
    out[k] = np.array(getattr(st, k))
out["rank_low"] = np.array([list(r) for r in st.rank_low], np.int64)
out["rank_high"] = np.array([list(r) for r in st.rank_high], np.int64)
np.savez(dst, **out)
"""


def test_the_tolerance_build_gives_the_same_bits(pkg, tmp_path):
    """libwxsim_fast.so (contraction allowed everywhere else) on the data above, the separating cells among them: the per-cell function
    switches contraction off for itself. In a process of its own: a process holds one libwxsim."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    leg = _FAST_LEG % (list(COUNTS), list(SUMS), list(MAPS), list(MAPS), NAMES)
    for B, members in SEP_CASES:
        (f, w), (tf, tw) = planted(B)
        mask = np.isin(np.arange(B), list(range(B)) if members is None else members).astype(np.uint8)
        src, dst = str(tmp_path / f"in{B}.npz"), str(tmp_path / f"out{B}.npz")
        np.savez(src, f=np.stack(f), w=np.stack(w), tf=tf, tw=tw, mask=mask)
        subprocess.check_call([sys.executable, "-c", leg, fast, src, dst], timeout=120)
        got = dict(np.load(dst))
        check(got, pkg.engine.ens_score_cells(f, w, tf, tw, members=members), ("fast vs exact", B))
        check(got, reference(f, w, tf, tw, members), ("fast vs definition", B))
        for cell, which, _, _, defined, _ in separating_cells():
            assert (got[which][cell].view(np.uint32) == defined).all(), (B, cell)


def test_host_function_under_the_sanitizers(tmp_path):
    """tests/native/ens_score_main.cpp -- the per-cell header and a main() that runs wxs::score_cells over randomised buffers that end
    exactly at the last cell -- compiled stand-alone with AddressSanitizer and UBSan (host compiler, no device, no library) and run."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.call(["which", c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ens_score_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "ens_score_main.cpp")], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ens_score_main ok" in out.stdout
