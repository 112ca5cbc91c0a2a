"""Ensemble quantiles and ranks (wx_ensemble_quantiles, wx_ens_quant_cells, wx_ens_quant_staged_members; include/wxsim.h) without a
GPU: the header announces and declares the addition at the unchanged ABI version, both libraries export it, the argument checks answer
before any device is touched, and the pure host entry point -- the kernels' own per-cell function -- equals the definition in the
header comment, which `reference` below writes down with np.sort over the member axis and float64 arithmetic with ONE numpy operation
per rounded operation (not np.quantile, whose lerp is another formula). Every comparison is `==` on bits, NaNs compared as positions."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from test_ensemble_statistics_cpu import FLT_MAX, hand_built, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_quantiles", "wx_ens_quant_cells", "wx_ens_quant_staged_members"]
PLANES = ("q", "count", "n_wall", "n_below", "n_equal")
E_INVALID = -1
INTERPS = ("linear", "lower", "higher")
# the eight quantiles every comparison asks for at once (n_q = 8): both ends, the median, the 10 / 90 % band as float32 numbers that
# are no binary fractions, a third, the quartiles
P8 = tuple(float(np.float32(v)) for v in (0.0, 1.0, 0.5, 0.1, 0.9, 1.0 / 3.0, 0.25, 0.75))


def reference(fields, walls, members=None, p=P8, interp="linear", rank_of=None):
    """The per-cell function of include/wxsim.h, straight from its definition. fields[i]: float32 (..., 4), walls[i]: int8 (..., 4);
    members: the selected member indices (None: all but rank_of). Returns q (n_q, ..., 4), count, n_wall and, with rank_of, n_below /
    n_equal."""
    sel = sorted(i for i in (range(len(fields)) if members is None else members) if members is not None or i != rank_of)
    v = np.stack([fields[i] for i in sel])
    is_wall = np.stack([walls[i][..., 1] == 0 for i in sel])
    take = ~is_wall[..., None] & np.isfinite(v)
    out = {"count": take.sum(0).astype(np.int32), "n_wall": is_wall.sum(0).astype(np.int32)}
    n = out["count"]
    with np.errstate(all="ignore"):
        entered = np.where(take, np.where(v == 0, np.float32(0), v), np.float32(np.inf))  # an entered -0.0 is taken as +0.0
        s = np.sort(entered, axis=0)  # v(0) <= ... <= v(n-1) in front, what did not enter behind
        qs = []
        for pj in p:
            h = np.float64(np.float32(pj)) * (n - 1).astype(np.float64)
            k = np.floor(h)
            g = h - k
            ki = np.clip(k.astype(np.int64), 0, None)  # (n = 0: h = -p, not used)
            k1 = np.clip(np.minimum(ki + 1, n - 1), 0, None)
            vk, vk1 = np.take_along_axis(s, ki[None], 0)[0], np.take_along_axis(s, k1[None], 0)[0]
            if interp == "lower":
                r = vk
            elif interp == "higher":
                r = np.where(g > 0, vk1, vk)
            else:
                d = vk1.astype(np.float64) - vk.astype(np.float64)
                gd = g * d
                r = (vk.astype(np.float64) + gd).astype(np.float32)
            qs.append(np.where(n > 0, r, np.float32(np.nan)).astype(np.float32))
        out["q"] = np.stack(qs) if qs else np.zeros((0,) + n.shape, np.float32)
        if rank_of is not None:
            t = fields[rank_of]
            ok = (walls[rank_of][..., 1] != 0)[..., None] & np.isfinite(t)
            out["n_below"] = np.where(ok, (take & (v < t)).sum(0), -1).astype(np.int32)
            out["n_equal"] = np.where(ok, (take & (v == t)).sum(0), -1).astype(np.int32)
    return out


# SEPARATING CELLS of the linear interpolation: two values on which fma(g, d, v(k)) -- what a build computes that contracts the
# product into the sum -- gives ANOTHER float32 quantile than the definition's rounded g * d and rounded sum. The two doubles differ
# by one ulp, which the conversion shows only on a float32 rounding boundary (2^-29 per ulp for random data), and only if g * d is
# inexact at all: two values of like magnitude never separate. Printed by `python tools/find_variance_separators.py --seed 1`
# (numpy and exact rational arithmetic, no build of the library), not searched for at test time. n = 2, so h = g = P_SEP -- a
# quantile of its own: with the short fractions of P8 the result lies on a lattice on which the two evaluations never differ.
# (cell of `planted`; float32 bits of v(0) and v(1); float32 bits of the quantile by the definition; by the fused evaluation.)
# Member 1 holds v(1), member 2 holds v(0), every other member NaN: a cell is complete in every selection that holds members 1 and 2.
P_SEP = float(np.float32(0.3141592))
SEPARATING_CELLS = [
    (20, 0xBFEAD0FF, 0x33E593EA, 0xBFA10BF2, 0xBFA10BF1),  # fused above
    (21, 0xBFEAD11F, 0x33BA4FEC, 0xBFA10C08, 0xBFA10C07),  # fused above
    (22, 0xBFEAD42B, 0x33964E1D, 0xBFA10E1E, 0xBFA10E1F),  # fused below
    (23, 0xBFEAD49A, 0x33FEE024, 0xBFA10E6A, 0xBFA10E6B),  # fused below
]


def separating_cells_in(B, members=None):
    """The separating cells that are complete in a selection of planted(B)'s members 0 .. B - 1."""
    return SEPARATING_CELLS if B >= 3 and {1, 2} <= set(range(B) if members is None else members) else []


def two_quantiles(v0, v1, p):
    """(defined, fused) float32 linear quantile p of the two ascending values, one Python float operation per rounded operation."""
    h = float(np.float32(p)) * 1.0
    k = float(np.floor(h))
    g = h - k
    assert k == 0.0
    d = v1 - v0
    gd = g * d
    return np.float32(v0 + gd), np.float32(float(Fraction(g) * Fraction(d) + Fraction(v0)))


def planted(B, n_cells=64):
    """`hand_built` of the statistics test for B + 1 members -- random float bit patterns, random walls, and its planted cells: all
    equal (0), subnormals with FLT_MAX (2), one NaN / +Inf / -Inf among finite values (3), every member non-finite (4), every member
    wall (5), wall in some members only (6), -0.0 against +0.0 (7), ties (8) -- plus, in cells 11 .. 14: n = 1, n = 2, ties across k /
    k1 around the median, -0.0 and +0.0 in one cell. Member B is the one that is RANKED: in the planted cells its values lie below all,
    above all, equal to several, on a wall, and are NaN. Cells 15 .. 19 are hand_built's separating cells of the variance, 20 .. 23 the separating
    cells of the linear interpolation (SEPARATING_CELLS above)."""
    f, w = hand_built(B + 1, n_cells)
    for i in range(B):
        w[i][11, 1] = 7 if i == 0 else 0                                  # 11: one member's value enters
        w[i][12, 1] = 7 if i < 2 else 0                                   # 12: two (one if B = 1)
        f[i][11] = np.float32([3.5, -0.0, 1e-45, -FLT_MAX])
        f[i][12] = np.float32([1.0, -2.0, 0.0, FLT_MAX]) if i == 0 else np.float32([2.0, -2.0, -0.0, -FLT_MAX])
        f[i][13] = np.float32([1.0, 2.0, 2.0, 3.0][i % 4])                # 13: ties in the middle
        w[i][13, 1] = 9
        f[i][14] = np.float32([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0][i % 6])   # 14: zeros of both signs among the values
        w[i][14, 1] = 9
    r = f[B]
    w[B][[0, 8, 11, 12, 13, 14], 1] = 3
    r[0] = np.float32([1.0, 2.0, 1.5, -np.inf])   # against 1.5 everywhere: below all, above all, equal to all, not finite
    r[8] = np.float32([-7.0, 9.0, 5.0, 4.999])    # equal to the tied minimum / maximum (B >= 3), to every member, below all
    r[13] = np.float32([2.0, 2.5, 0.0, 3.0])      # equal to several, between, below all, equal to the maximum
    r[14] = np.float32([-0.0, 0.0, 1e-45, np.nan])  # a zero of either sign equals the zeros of both signs
    w[B][1, 1] = 0                                # on a wall
    r[2] = np.float32([np.nan, FLT_MAX, -FLT_MAX, 0.0])
    for cell, v0, v1, _, _ in SEPARATING_CELLS:   # 20 .. 23: the separating cells, the same values in all four channels
        if cell < n_cells:
            for i in range(B + 1):
                f[i][cell] = np.uint32({1: v1, 2: v0}.get(i, 0x7FC00000)).view(np.float32) if i < B else np.float32(np.nan)
                w[i][cell, 1] = 5
    return f, w


CASES = [(1, None), (2, None), (3, None), (7, None), (7, [0, 2, 3, 6]), (70, [i for i in range(70) if i not in (0, 33, 69)]), (300, None),
         (300, list(range(0, 300, 7)))]
IDS = ["1", "2", "3", "7", "7-masked", "70-masked", "300", "300-masked"]


def check(got, want, where):
    assert set(got) == set(want), (where, sorted(got), sorted(want))
    for k in want:
        assert same_bits(got[k], want[k]), (where, k, np.argwhere(~(got[k] == want[k]) & ~(np.isnan(got[k].astype(np.float64)) & np.isnan(want[k].astype(np.float64))))[:5].tolist())


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_QUANTILES\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ENS_QUANT_MAX\s+8\s*$", hdr, re.M)
    for name, value in (("LINEAR", 0), ("LOWER", 1), ("HIGHER", 2)):
        assert re.search(r"^#define\s+WX_QUANT_%s\s+%d\s*$" % (name, value), hdr, re.M)
        assert pkg.engine.QUANT_INTERP[name.lower()] == value
    E, L = pkg.engine, pkg.engine.lib()
    for n in NAMES:  # (libwxsim_fast.so's exports: the child process of test_the_tolerance_build_gives_the_same_bits looks them up)
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in E.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert callable(E.Ensemble.quantiles) and callable(pkg.sim.WeatherEnsemble.quantiles) and callable(pkg.sim.WeatherEnsemble.median) and callable(E.ens_quant_cells)
    assert "ensemble_quantiles" in [L.wx_kernel_name(k).decode() for k in range(L.wx_kernel_count())]
    staged = L.wx_ens_quant_staged_members()
    assert staged == E.Ensemble.QUANT_STAGED_MEMBERS and staged >= 8 and staged & (staged - 1) == 0
    # the ctypes struct is the header's, member for member
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct wx_ens_quant {"):hdr.index("} wx_ens_quant;")].split("{", 1)[1], flags=re.S)
    names = [re.sub(r"[\*\s]|\[.*\]", "", n) for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(float|int32_t)\b", "", decl.strip()).split(",")]
    assert names == [f[0] for f in E.WxEnsQuant._fields_] == ["n_q", "interp", "p", "rank_member"] + list(PLANES)
    assert C.sizeof(E.WxEnsQuant) == 48 + 5 * 8 and E.WxEnsQuant.q.offset == 48
    # the statistics call is what it was: the median is a call of its own, not a plane of wx_ens_stat
    assert "median" not in E.ENS_STAT_ALL and len(E.ENS_STAT_ALL) == 9


def test_argument_checks_answer_without_a_device(pkg):
    L, E = pkg.engine.lib(), pkg.engine
    f, w = planted(3, 16)  # members 0 .. 2 and the ranked member 3
    fp, wp = (C.c_void_p * 4)(*[a.ctypes.data for a in f]), (C.c_void_p * 4)(*[a.ctypes.data for a in w])
    q, cnt, below = np.full((2, 16, 4), -77, np.float32), np.full((16, 4), -77, np.int32), np.full((16, 4), -77, np.int32)

    def desc(**kw):
        st = E.WxEnsQuant()
        st.n_q, st.interp, st.rank_member = 2, 0, -1
        st.p[0], st.p[1] = 0.5, 1.0
        st.q, st.count = q.ctypes.data, cnt.ctypes.data
        for k, v in kw.items():
            if k == "p":
                st.p[1] = v
            else:
                setattr(st, k, v)
        return st

    good = desc()
    assert L.wx_ensemble_quantiles(None, 0, 0, 0, 1, 1, None, C.byref(good)) == E_INVALID
    assert L.wx_ensemble_quantiles(None, 0, 0, 0, 1, 1, None, None) == E_INVALID
    first3, nobody, all4 = (C.c_uint8 * 4)(1, 1, 1, 0), (C.c_uint8 * 4)(0, 0, 0, 0), (C.c_uint8 * 4)(1, 1, 1, 1)
    call = lambda st, n=4, fp=fp, wp=wp, mask=first3: L.wx_ens_quant_cells(n, 16, fp, wp, mask, None if st is None else C.byref(st))  # noqa: E731
    assert call(good) == 0 and (q != -77).all() and (cnt != -77).all()
    q[:], cnt[:] = -77, -77
    assert call(None) == E_INVALID
    for kw in (dict(n_q=-1), dict(n_q=9), dict(q=None), dict(p=float("nan")), dict(p=-1e-9), dict(p=1.0000001), dict(p=float("inf")), dict(interp=3), dict(interp=-1),
               dict(rank_member=4), dict(rank_member=-2), dict(rank_member=1), dict(n_below=below.ctypes.data), dict(n_equal=below.ctypes.data)):
        assert call(desc(**kw)) == E_INVALID, kw
    assert call(good, mask=nobody) == E_INVALID
    assert call(desc(rank_member=3), mask=None) == E_INVALID and call(desc(rank_member=3), mask=all4) == E_INVALID  # NULL selects everybody: the ranked member too
    assert call(good, n=0) == E_INVALID and call(good, n=-1) == E_INVALID
    assert call(good, fp=None) == E_INVALID and call(good, wp=None) == E_INVALID
    hole = (C.c_void_p * 4)(f[0].ctypes.data, None, f[2].ctypes.data, None)
    assert call(good, fp=hole) == E_INVALID                             # a selected member without cells
    assert call(desc(rank_member=3), fp=hole, mask=(C.c_uint8 * 4)(1, 0, 1, 0)) == E_INVALID   # ... the ranked member without cells
    assert (q == -77).all() and (cnt == -77).all() and (below == -77).all()  # a refused call writes nothing
    assert call(good, fp=hole, mask=(C.c_uint8 * 4)(1, 0, 1, 0)) == 0   # an unselected one may be absent
    assert call(desc(n_q=0, q=None)) == 0 and call(desc(rank_member=3, n_below=below.ctypes.data)) == 0 and (below != -77).all()
    for kw in (dict(members=[]), dict(rank_of=1, members=[0, 1]), dict(interp=7), dict(rank_of=4)):
        with pytest.raises(E.WxError) as ei:
            E.ens_quant_cells(f, w, (0.5,), **kw)
        assert ei.value.code == E_INVALID, kw
    with pytest.raises(E.WxError):
        E.ens_quant_cells(f, w, (0.5, 2.0))
    with pytest.raises(KeyError):
        E.ens_quant_cells(f, w, (0.5,), want=("q", "median"))
    with pytest.raises(ValueError):
        E.ens_quant_cells(f, w, (0.5,) * 9)


def test_the_definition_on_values_worked_by_hand(pkg):
    """The reference itself, and the host function, against numbers anybody can check: 1, 2, 4, 8 at p = 0.5 (h = 1.5: halfway between 2
    and 4), float32(0.1) of three values, and the lerp's own rounding -- v(k) + g (v(k1) - v(k)), not (1 - g) v(k) + g v(k1)."""
    definition = globals()["reference"]

    def reference(f, w, members, p, interp):  # both agree, then the numbers are asserted on one
        want = definition(f, w, members, p, interp)
        check(pkg.engine.ens_quant_cells(f, w, p, members=members, interp=interp), want, (p, interp))
        return want

    air = [np.full((1, 4), 5, np.int8)] * 4
    f = [np.full((1, 4), x, np.float32) for x in (8.0, 1.0, 4.0, 2.0)]
    for interp, want in (("linear", 3.0), ("lower", 2.0), ("higher", 4.0)):
        assert reference(f, air, None, (0.5,), interp)["q"][0, 0, 0] == want
    assert reference(f, air, None, (1.0 / 3.0,), "higher")["q"][0, 0, 0] == 4.0  # float32(1/3) * 3 is above 1 (g > 0) ...
    assert reference(f, air, None, (1.0 / 3.0,), "lower")["q"][0, 0, 0] == 2.0
    p01 = np.float64(np.float32(0.1))
    r = reference(f[:3], air[:3], None, (0.1,), "linear")["q"][0, 0, 0]   # 1, 4, 8: h = 0.2 (rounded up from float32): between 1 and 4
    assert r == np.float32(1.0 + (p01 * 2.0) * 3.0) and 1.6 < float(r) < 1.6001
    g = reference([np.full((1, 4), x, np.float32) for x in (1e-45, FLT_MAX)], air[:2], None, (0.75,), "linear")["q"][0, 0, 0]
    assert g == np.float32(np.float64(np.float32(1e-45)) + 0.75 * (np.float64(FLT_MAX) - np.float64(np.float32(1e-45))))


def test_separating_cells_separate(pkg):
    """Every committed cell, by exact arithmetic: the definition and the fused evaluation give the committed, DIFFERENT float32
    quantiles, in both directions; in planted's data `reference` gives the definition's value in exactly the complete cells; and
    the default library's host function equals `reference` at that p under every interpolation."""
    u32 = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    above = below = 0
    for cell, v0, v1, defined, fused in SEPARATING_CELLS:
        lo, hi = (float(np.uint32(b).view(np.float32)) for b in (v0, v1))
        a, b = two_quantiles(lo, hi, P_SEP)
        assert lo < hi and (u32(a), u32(b)) == (defined, fused) and defined != fused, (cell, hex(u32(a)), hex(u32(b)))
        assert abs(defined - fused) == 1  # neighbouring floats
        above, below = above + (b > a), below + (b < a)
    assert len(SEPARATING_CELLS) >= 2 and above >= 1 and below >= 1
    seen = 0
    for B, members in CASES[:6]:
        f, w = planted(B)
        for interp in INTERPS:
            want = reference(f, w, members, (P_SEP,), interp, B)
            check(pkg.engine.ens_quant_cells(f, w, (P_SEP,), members=members, interp=interp, rank_of=B), want, ("separating", B, interp))
        want = reference(f, w, members, (P_SEP, 0.0, 1.0), "linear", B)
        here = separating_cells_in(B, members)
        for cell, v0, v1, defined, fused in here:
            assert (want["q"][0, cell].view(np.uint32) == defined).all() and (want["count"][cell] == 2).all(), (B, cell)
            assert (want["q"][1, cell].view(np.uint32) == v0).all() and (want["q"][2, cell].view(np.uint32) == v1).all(), (B, cell)
            assert (want["n_below"][cell] == -1).all()  # (the ranked member holds a NaN there)
        for cell, _, _, _, _ in SEPARATING_CELLS:
            assert here or (want["count"][cell] < 2).all(), (B, cell)
        seen += len(here)
    assert seen == 3 * len(SEPARATING_CELLS)  # B = 3, 7 and 70 masked


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("B,members", CASES, ids=IDS)
def test_host_function_equals_the_definition(pkg, B, members, interp):
    f, w = planted(B)
    got = pkg.engine.ens_quant_cells(f, w, P8, members=members, interp=interp, rank_of=B)
    want = reference(f, w, members, P8, interp, B)
    check(got, want, (B, interp))
    # the cases are what they claim to be
    sel = list(range(B)) if members is None else members
    n_sel, q, n = len(sel), want["q"], want["count"]
    assert want["n_wall"][5] == n_sel and (n[5] == 0).all() and np.isnan(q[:, 5]).all()               # every member wall
    assert (n[4] == 0).all() and want["n_wall"][4] == 0 and np.isnan(q[:, 4]).all()                    # every member non-finite
    assert (q[:, 0] == 1.5).all() and (n[0] == n_sel).all()                                            # all equal: every quantile
    assert want["n_below"][0].tolist() == [0, n_sel, 0, -1] and want["n_equal"][0].tolist() == [0, 0, n_sel, -1]  # below all, above all, equal to all, not finite
    assert (want["n_below"][1] == -1).all() and (want["n_equal"][1] == -1).all()                       # the ranked member's cell is a wall
    assert want["n_below"][2, 0] == -1 and want["n_below"][2, 1] >= 0                                  # ... holds a NaN in one channel
    if 0 in sel:
        assert (n[11] == 1).all() and same_bits(q[:, 11], np.broadcast_to(np.float32([3.5, 0.0, 1e-45, -FLT_MAX]), (8, 4)).copy())  # n = 1: that value, -0.0 as +0.0
        if 1 in sel:
            assert (n[12] == 2).all() and q[2, 12].tolist() == ([1.5, -2.0, 0.0, 0.0] if interp == "linear" else [1.0 if interp == "lower" else 2.0, -2.0, 0.0, -FLT_MAX if interp == "lower" else FLT_MAX])
            assert q[2, 12, 2].view(np.uint32) == 0
    zeros = (np.stack([f[i][14] for i in sel]) == 0).sum(0)
    assert want["n_equal"][14, :2].tolist() == zeros[:2].tolist() and (want["n_below"][14, 3] == -1)    # -0.0 == 0.0 in the rank ...
    assert not (q[:, 14].view(np.uint32) == 0x80000000).any()                                          # ... and no quantile is a -0.0
    if B == 7 and members is None:
        assert n[3, 0] == 4 and q[0, 3, 0] == -3.0 and q[1, 3, 0] == 7.0                               # 2, -3, 0.25, 7 entered; NaN and the infinities did not
        assert want["n_wall"][6] == 3 and n[6, 0] == 4
        assert q[0, 8, 0] == -7.0 and q[3, 8, 0] == -7.0  # (p = 0.1 of seven: between v(0) and v(1), the tied minimum)
        assert want["n_equal"][8].tolist() == [2, 2, 7, 0] and want["n_below"][8].tolist() == [0, 5, 0, 0]
        assert q[2, 13, 0] == 2.0 and want["n_equal"][13].tolist() == [4, 0, 0, 1] and want["n_below"][13].tolist() == [2, 6, 0, 6]
        assert np.isfinite(q[:, 2]).all() and q[1, 2, 0] == FLT_MAX
    if B == 300:
        assert n.max() == n_sel and (want["n_below"] > 0).any() and ((want["n_below"] > 0) & (want["n_below"] < n)).any()


@pytest.mark.parametrize("B,members", [(7, None), (70, CASES[5][1])], ids=["7", "70-masked"])
def test_agrees_with_the_statistics(pkg, B, members):
    """What the two calls both know: p = 0 and p = 1 are min and max bit for bit (the +0.0 rule included) under every interpolation,
    count and n_wall are the same numbers, and the LOWER median of an odd number of values is np.median of the entered values."""
    f, w = planted(B)
    f, w = f[:B], w[:B]
    st = pkg.engine.ens_stat_cells(f, w, members=members, want=("min", "max", "count", "n_wall"))
    for interp in INTERPS:
        got = pkg.engine.ens_quant_cells(f, w, (0.0, 1.0, 0.5), members=members, interp=interp)
        assert set(got) == {"q", "count", "n_wall"}
        assert same_bits(got["q"][0], st["min"]) and same_bits(got["q"][1], st["max"]), interp
        assert same_bits(got["count"], st["count"]) and same_bits(got["n_wall"], st["n_wall"])
    med = pkg.engine.ens_quant_cells(f, w, (0.5,), members=members, interp="lower", want=("q",))["q"][0]
    sel = range(B) if members is None else members
    odd = 0
    for cell in range(64):
        for c in range(4):
            vals = [f[i][cell, c] + np.float32(0) for i in sel if w[i][cell, 1] != 0 and np.isfinite(f[i][cell, c])]  # (+ 0: -0.0 becomes +0.0)
            if len(vals) % 2 == 1:
                odd += 1
                assert same_bits(np.float32(np.median(np.float32(vals))).reshape(1), med[cell, c].reshape(1)), (cell, c)
    assert odd > 20


def test_the_order_of_the_members_does_not_matter(pkg):
    B = 70
    f, w = planted(B)
    members = CASES[5][1]
    rng = np.random.Generator(np.random.Philox(5))
    first = pkg.engine.ens_quant_cells(f, w, P8, members=members, rank_of=B)
    for _ in range(3):
        perm = rng.permutation(B + 1)  # new position k holds old member perm[k]
        where = {int(old): k for k, old in enumerate(perm)}
        again = pkg.engine.ens_quant_cells([f[i] for i in perm], [w[i] for i in perm], P8, members=[where[i] for i in members], rank_of=where[B])
        check(again, first, "permuted")


def test_unwanted_planes_are_left_alone(pkg):
    E, L = pkg.engine, pkg.engine.lib()
    f, w = planted(7)
    full = E.ens_quant_cells(f, w, P8[:3], rank_of=7)
    assert set(full) == set(PLANES) and full["q"].shape == (3, 64, 4) and full["n_wall"].shape == (64,)
    fp, wp = (C.c_void_p * 8)(*[a.ctypes.data for a in f]), (C.c_void_p * 8)(*[a.ctypes.data for a in w])
    mask = (C.c_uint8 * 8)(*([1] * 7 + [0]))
    for wanted in (("q",), ("count", "n_equal"), ("n_wall", "n_below"), ()):
        buf = {k: np.full(full[k].shape, 0x5A5A5A5A, np.uint32) for k in PLANES}
        st = E.WxEnsQuant()
        st.n_q, st.interp, st.rank_member = (3 if "q" in wanted else 0), 0, 7
        st.p[:3] = P8[:3]
        for k in wanted:
            setattr(st, k, buf[k].ctypes.data)
        assert L.wx_ens_quant_cells(8, 64, fp, wp, mask, C.byref(st)) == 0
        for k in PLANES:
            if k in wanted:
                assert same_bits(buf[k].view(full[k].dtype), full[k]), (wanted, k)
            else:
                assert (buf[k] == 0x5A5A5A5A).all(), (wanted, k)
    some = E.ens_quant_cells(f, w, P8[:3], rank_of=7, want=("q", "n_below"))
    assert set(some) == {"q", "n_below"} and same_bits(some["q"], full["q"]) and same_bits(some["n_below"], full["n_below"])
    assert set(E.ens_quant_cells(f[:7], w[:7], (0.5,))) == {"q", "count", "n_wall"}


_FAST_LEG = """
import ctypes as C, sys, numpy as np
lib, src, dst = sys.argv[1:4]
L = C.CDLL(lib)
d = np.load(src)
f, w, mask, p, interp, rank = np.ascontiguousarray(d["f"]), np.ascontiguousarray(d["w"]), d["mask"], d["p"], int(d["interp"]), int(d["rank"])
B, n = f.shape[:2]
class S(C.Structure):
    _fields_ = [("n_q", C.c_int32), ("interp", C.c_int32), ("p", C.c_float * 8), ("rank_member", C.c_int32)] + [(k, C.c_void_p) for k in %r]
out = {"q": np.zeros((len(p), n, 4), np.float32), "count": np.zeros((n, 4), np.int32), "n_wall": np.zeros(n, np.int32),
       "n_below": np.zeros((n, 4), np.int32), "n_equal": np.zeros((n, 4), np.int32)}
st = S()
st.n_q, st.interp, st.rank_member = len(p), interp, rank
st.p[:len(p)] = [float(x) for x in p]
for k, a in out.items():
    setattr(st, k, a.ctypes.data)
fp, wp = (C.c_void_p * B)(*[f[i].ctypes.data for i in range(B)]), (C.c_void_p * B)(*[w[i].ctypes.data for i in range(B)])
L.wx_ens_quant_cells.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
assert L.wx_arith() == 1, "not the tolerance build"
for name in %r:
    getattr(L, name)
assert L.wx_ens_quant_staged_members() == %d
assert L.wx_ens_quant_cells(B, n, fp, wp, mask.ctypes.data, C.byref(st)) == 0
np.savez(dst, **out)
"""


def test_the_tolerance_build_gives_the_same_bits(pkg, tmp_path):
    """libwxsim_fast.so (contraction allowed everywhere else) on the data above: the per-cell function switches contraction off for
    itself. In a process of its own: a process holds one libwxsim."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    leg = _FAST_LEG % (list(PLANES), NAMES, pkg.engine.Ensemble.QUANT_STAGED_MEMBERS)
    for B, members in ((7, None), (70, CASES[5][1])):
        f, w = planted(B)
        mask = np.isin(np.arange(B + 1), list(range(B)) if members is None else members).astype(np.uint8)
        for k, interp in enumerate(INTERPS):
            src, dst = str(tmp_path / f"in{B}_{k}.npz"), str(tmp_path / f"out{B}_{k}.npz")
            np.savez(src, f=np.stack(f), w=np.stack(w), mask=mask, p=np.float32(P8), interp=k, rank=B)
            subprocess.check_call([sys.executable, "-c", leg, fast, src, dst], timeout=120)
            got = dict(np.load(dst))
            check(got, pkg.engine.ens_quant_cells(f, w, P8, members=members, interp=interp, rank_of=B), ("fast vs exact", B, interp))
            check(got, reference(f, w, members, P8, interp, B), ("fast vs definition", B, interp))
        src, dst = str(tmp_path / f"in{B}_sep.npz"), str(tmp_path / f"out{B}_sep.npz")  # the separating cells' own quantile
        np.savez(src, f=np.stack(f), w=np.stack(w), mask=mask, p=np.float32([P_SEP]), interp=0, rank=B)
        subprocess.check_call([sys.executable, "-c", leg, fast, src, dst], timeout=120)
        got = dict(np.load(dst))
        check(got, reference(f, w, members, (P_SEP,), "linear", B), ("fast vs definition, separating", B))
        assert all((got["q"][0, cell].view(np.uint32) == defined).all() for cell, _, _, defined, _ in SEPARATING_CELLS)


def test_host_function_under_the_sanitizers(tmp_path):
    """tests/native/ens_quant_main.cpp -- the per-cell header and a main() that runs wxq::quant_cells over randomised buffers that end
    exactly at the last cell -- compiled stand-alone with AddressSanitizer and UBSan (host compiler, no device, no library) and run."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.call(["which", c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ens_quant_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "ens_quant_main.cpp")], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ens_quant_main ok" in out.stdout
