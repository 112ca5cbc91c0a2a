"""Ensemble statistics (wx_ensemble_statistics, wx_ens_stat_cells; include/wxsim.h) without a GPU: the header announces and declares the
addition at the unchanged ABI version, the library exports it, the argument checks answer before any device is touched, and the pure host
entry point -- the kernel's own per-cell function -- equals the definition in the header comment, which `reference` below writes down as
an explicit loop over the members in member order on float64 arrays: one `+` per entered value for S, one `-`, one `*` and one `+` for Q.
No np.sum, no np.var (pairwise summation is another order). Every comparison is `==` on bits, NaNs compared as positions."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_statistics", "wx_ens_stat_cells"]
PLANES = ("mean", "variance", "min", "max", "argmin", "argmax", "count", "n_above", "n_wall")
E_INVALID = -1
FLT_MAX = np.float32(3.4028234663852886e38)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


def _fma(a, b, c, where):
    """fma(a, b, c) element by element in exact rational arithmetic, rounded once (Python 3.10 has no math.fma); c where not `where`."""
    out = np.array(c, np.float64)
    for i in np.argwhere(where):
        i = tuple(i)
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def reference(fields, walls, members=None, threshold=(0, 0, 0, 0), fused=False):
    """The per-cell function of include/wxsim.h, straight from its definition. fields[i]: float32 (..., 4), walls[i]: int8 (..., 4);
    members: the selected member indices (None: all). Returns the nine planes. fused: NOT the definition -- Q = fma(d, d, Q), what a
    build computes that contracts the product into the sum; the separating cells below are where the two differ."""
    shape = fields[0].shape
    sel = sorted(range(len(fields)) if members is None else members)  # member order, 0 first
    thr = np.asarray(threshold, np.float32)
    S = np.zeros(shape, np.float64)
    n = np.zeros(shape, np.int32)
    n_above = np.zeros(shape, np.int32)
    n_wall = np.zeros(shape[:-1], np.int32)
    mn, mx = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    amn, amx = np.full(shape, -1, np.int32), np.full(shape, -1, np.int32)
    enters = {}
    with np.errstate(all="ignore"):
        for i in sel:
            v = fields[i]
            is_wall = walls[i][..., 1] == 0
            n_wall = n_wall + is_wall
            take = ~is_wall[..., None] & np.isfinite(v)
            enters[i] = take
            S = np.where(take, S + v.astype(np.float64), S)
            n = n + take
            lower, higher = take & (v < mn), take & (v > mx)  # strict: the smallest member index wins a tie; -0.0 == 0.0
            mn, amn = np.where(lower, v, mn), np.where(lower, np.int32(i), amn)
            mx, amx = np.where(higher, v, mx), np.where(higher, np.int32(i), amx)
            n_above = n_above + (take & (v > thr))
        m = np.where(n > 0, S / n.astype(np.float64), np.nan)
        Q = np.zeros(shape, np.float64)
        for i in sel:
            d = fields[i].astype(np.float64) - m
            if fused:
                Q = _fma(d, d, Q, enters[i])
                continue
            dd = d * d
            Q = np.where(enters[i], Q + dd, Q)
        var = np.where(n > 0, Q / n.astype(np.float64), np.nan).astype(np.float32)
        mn = np.where(n > 0, np.where(mn == 0, np.float32(0), mn), np.float32(np.nan)).astype(np.float32)
        mx = np.where(n > 0, np.where(mx == 0, np.float32(0), mx), np.float32(np.nan)).astype(np.float32)
    return {"mean": m.astype(np.float32), "variance": var, "min": mn, "max": mx, "argmin": amn, "argmax": amx, "count": n, "n_above": n_above,
            "n_wall": n_wall}


THRESHOLD = (0.5, -1.0, float("nan"), 1e-40)  # channel 2: a NaN threshold (n_above is 0 there); channel 3: a subnormal one
ORDER_VALUES = np.array([1e30, 1.0, -1e30, 1.0], np.float32)

# SEPARATING CELLS: sets of members on which Q = fma(d, d, Q) -- what a build computes that contracts the product into the sum -- gives
# ANOTHER float32 variance than the definition's rounded product and rounded sum. The two Q differ by an ulp or two of a double, which
# the conversion to float32 shows only where Q / n lies that close to a float32 rounding boundary: about B * 2^-29 per cell of random
# data, so no other data of this suite can tell the two apart. Printed by `python tools/find_variance_separators.py --seed 1` (a
# directed search in numpy and exact rational arithmetic; no build of the library is asked), not searched for at test time.
# (cell of hand_built; float32 bits of members 1, 2, ... of that cell; which of them is a WALL member, if any; the float32 bits of
# the variance by the definition; by the fused evaluation.) 0x7FC00000 is a NaN member: it does not enter, like the wall member.
# Members 0 and those behind the list hold NaN, so a cell is complete in every selection that holds members 1 .. len(bits).
SEPARATING_CELLS = [
    (15, [0x35C6BC5A, 0x3FB514E6, 0x30B54871, 0xBF8237EA, 0x40050901, 0x3FDE1EE1], None, 0x3F9E22D1, 0x3F9E22D2),  # 6 enter, fused above
    (16, [0x4042BDD0, 0x35ECB6FA, 0x405BA7DB, 0x401A6133, 0x30A282A6, 0x3FACC464], None, 0x3FEF3677, 0x3FEF3676),  # 6 enter, fused below
    (17, [0x3087B2EF, 0x3FDFF5E3, 0x35A3CA88, 0x7FC00000, 0x40726A7C, 0xC00A839B], None, 0x407DA828, 0x407DA829),  # 5 enter, a NaN member among them
    (18, [0x3FAFF34E, 0xC05221B2, 0x35A4AD17, 0xC0656B63, 0x4054539A, 0x30A9C8DA, 0xC00BD290, 0xC07F80DD, 0xBFBCEFD7], None,
     0x40AD1760, 0x40AD1761),                                                                                     # 9 enter: a group of 8 and a remainder
    (19, [0xC04FEFF8, 0x30BCF5C1, 0x40134D70, 0xC03A68D0, 0x401598E1, 0x42F60000, 0x3FDC66F0, 0xC06B3A30, 0xC0395A4C, 0x35C95242], 5,
     0x40B24FDA, 0x40B24FD9),                                                                                     # 9 enter, a wall member (123.0) among them
]


def separating_cells_in(B, members=None):
    """The separating cells that are complete in a selection of hand_built(B)'s members."""
    sel = set(range(B) if members is None else members)
    return [s for s in SEPARATING_CELLS if set(range(1, 1 + len(s[1]))) <= sel and len(s[1]) < B]


def two_variances(values):
    """(defined, fused) float32 variance of the values that enter, in member order, one Python float operation per rounded operation."""
    n = float(len(values))
    S = 0.0
    for v in values:
        S = S + v
    m = S / n
    Q = Qf = 0.0
    for v in values:
        d = v - m
        dd = d * d
        Q = Q + dd
        Qf = float(Fraction(d) * Fraction(d) + Fraction(Qf))
    return np.float32(Q / n), np.float32(Qf / n)


def hand_built(B, n_cells=64, seed=2024):
    """B members x n_cells cells: random float BIT PATTERNS (NaNs, infinities, subnormals and huge values included) with random walls,
    and one cell per case of the definition in front -- each written as far as B members reach."""
    rng = np.random.Generator(np.random.Philox(seed + B))
    f = rng.integers(0, 2**32, (B, n_cells, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    w = np.zeros((B, n_cells, 4), np.int8)
    w[..., 1] = np.where(rng.random((B, n_cells)) < 0.2, 0, rng.integers(1, 100, (B, n_cells))).astype(np.int8)
    w[..., 3] = rng.integers(0, 100, (B, n_cells)).astype(np.int8)

    def put(cell, values, channel=None):  # member i gets values[i % len(values)]; air in every member
        values = np.asarray(values, np.float32)
        for i in range(B):
            if channel is None:
                f[i, cell, :] = values[i % len(values)]
            else:
                f[i, cell, channel] = values[i % len(values)]
        w[:, cell, 1] = 5

    tiny = np.float32(1e-45)
    put(0, [1.5])                                                               # 0: all values equal
    put(1, list(ORDER_VALUES) + [0.0, 0.0, 0.0])                                # 1: the fixed-order sum differs from the sorted-order sum
    put(2, [tiny, FLT_MAX, -1e-40, FLT_MAX, 1.4e-45, -FLT_MAX, 3e-39])          # 2: subnormals together with FLT_MAX
    put(3, [2.0, np.nan, -3.0, np.inf, 0.25, -np.inf, 7.0])                     # 3: one NaN, one +Inf, one -Inf among finite values
    put(4, [np.nan, np.inf, -np.inf])                                           # 4: every member non-finite
    put(5, [1.0, 2.0, 3.0])
    w[:, 5, 1] = 0                                                              # 5: every member wall
    put(6, [4.0, -2.0, 8.0, 1.0, 0.5, -9.0, 3.0])
    w[[i for i in (1, 3, 4) if i < B], 6, 1] = 0                                # 6: wall in some members only
    put(7, [-0.0, 0.0], 0)                                                      # 7: -0.0 against +0.0, for both extremes
    put(7, [0.0, -0.0], 1)
    put(7, [-0.0, -1.0, -2.0], 2)                                               #    (the maximum is a -0.0: reported as +0.0)
    put(7, [1.0, -0.0, 0.0, 2.0], 3)                                            #    (the minimum is a -0.0 first met at member 1)
    put(8, [0.0, 1.0, -7.0, 2.0, 3.0, -7.0, 4.0], 0)                            # 8: ties on the minimum ...
    put(8, [0.0, 1.0, 9.0, 2.0, 3.0, 9.0, 4.0], 1)                              #    ... and on the maximum at members 2 and 5
    put(8, [5.0], 2)
    put(8, [5.0], 3)
    for c in range(4):                                                          # 9: equal to the threshold, just above, just below
        t = np.float32(THRESHOLD[c] if THRESHOLD[c] == THRESHOLD[c] else 1.0)
        put(9, [t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))], c)
    put(10, [1e30, -1e30, 3.0, 0.0], 2)                                         # 10: values of any size under the NaN threshold of channel 2
    # (11 .. 14 are the cells the quantiles' `planted` writes.) 15 .. 19: the separating cells, the same values in all four channels.
    # The quantile tests build `planted` on this function, so they inherit these five cells as well (there: six or nine finite values
    # of mixed magnitude among NaN members, one cell with a wall member); 20 .. 23 are `planted`'s own separating cells
    for cell, bits, wall_at, _, _ in SEPARATING_CELLS:
        if cell < n_cells:
            f[:, cell, :] = np.float32(np.nan)
            w[:, cell, 1] = 5
            for k, b in enumerate(bits[:B - 1]):
                f[1 + k, cell, :] = np.uint32(b).view(np.float32)
            if wall_at is not None and 1 + wall_at < B:
                w[1 + wall_at, cell, 1] = 0
    return [np.ascontiguousarray(f[i]) for i in range(B)], [np.ascontiguousarray(w[i]) for i in range(B)]


CASES = [(7, None), (1, None), (70, [i for i in range(70) if i not in (0, 33, 69)])]
# 8, 9 and 16 selected members of 16: one full group of the kernel's member loop (UNROLL = 8) and no remainder, a group and one, two groups
N_SEL_CASES = [(16, list(range(1, 9))), (16, list(range(1, 10))), (16, None)]


def check(got, want, where):
    assert set(got) == set(want), where
    for k in want:
        assert same_bits(got[k], want[k]), (where, k, np.argwhere(~(got[k] == want[k]) & ~(np.isnan(got[k].astype(np.float64)) & np.isnan(want[k].astype(np.float64))))[:5].tolist())


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_STATISTICS\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    assert "typedef struct wx_ens_stat {" in hdr and "} wx_ens_stat;" in hdr
    L = pkg.engine.lib()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in pkg.engine.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert callable(pkg.engine.Ensemble.statistics) and callable(pkg.sim.WeatherEnsemble.statistics) and callable(pkg.engine.ens_stat_cells)
    assert "ensemble_statistics" in [L.wx_kernel_name(k).decode() for k in range(L.wx_kernel_count())]
    # the ctypes struct is the header's, member for member
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct wx_ens_stat {"):hdr.index("} wx_ens_stat;")].split("{", 1)[1], flags=re.S)
    names = [re.sub(r"[\*\s]|\[.*\]", "", n) for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(float|int32_t)\b", "", decl.strip()).split(",")]
    assert names == [f[0] for f in pkg.engine.WxEnsStat._fields_] == list(PLANES) + ["threshold"]


def test_argument_checks_answer_without_a_device(pkg):
    L, E = pkg.engine.lib(), pkg.engine
    st = E.WxEnsStat()
    assert L.wx_ensemble_statistics(None, 0, 0, 0, 1, 1, None, C.byref(st)) == E_INVALID
    assert L.wx_ensemble_statistics(None, 0, 0, 0, 1, 1, None, None) == E_INVALID
    f, w = hand_built(3, 16)
    fp, wp = (C.c_void_p * 3)(*[a.ctypes.data for a in f]), (C.c_void_p * 3)(*[a.ctypes.data for a in w])
    count = np.full((16, 4), -77, np.int32)
    st.count = count.ctypes.data
    ones, zeros = (C.c_uint8 * 3)(1, 1, 1), (C.c_uint8 * 3)(0, 0, 0)
    assert L.wx_ens_stat_cells(3, 16, fp, wp, ones, C.byref(st)) == 0 and (count != -77).all()
    count[:] = -77
    for args in ((0, 16, fp, wp, None), (-1, 16, fp, wp, None), (3, 16, None, wp, None), (3, 16, fp, None, None), (3, 16, fp, wp, zeros)):
        assert L.wx_ens_stat_cells(*args, C.byref(st)) == E_INVALID, args[:2]
    assert L.wx_ens_stat_cells(3, 16, fp, wp, None, None) == E_INVALID
    hole = (C.c_void_p * 3)(f[0].ctypes.data, None, f[2].ctypes.data)  # a selected member without cells
    assert L.wx_ens_stat_cells(3, 16, hole, wp, None, C.byref(st)) == E_INVALID
    assert (count == -77).all()  # a refused call writes nothing
    assert L.wx_ens_stat_cells(3, 16, hole, wp, (C.c_uint8 * 3)(1, 0, 1), C.byref(st)) == 0  # ... an unselected one may be absent
    with pytest.raises(E.WxError) as ei:
        E.ens_stat_cells(f, w, members=[])
    assert ei.value.code == E_INVALID
    with pytest.raises(KeyError):
        E.ens_stat_cells(f, w, want=("mean", "median"))


def test_the_order_case_pins_the_order():
    """[1e30, 1, -1e30, 1] in member order sums to 1, in sorted order to 0: a sum in any other order fails the comparison below."""
    v = [np.float64(x) for x in ORDER_VALUES]
    fixed = sorted_sum = np.float64(0)
    for x in v:
        fixed = fixed + x
    for x in sorted(v):
        sorted_sum = sorted_sum + x
    assert fixed == 1.0 and sorted_sum == 0.0 and fixed != sorted_sum
    f, w = hand_built(7)
    r = reference(f, w, threshold=THRESHOLD)
    assert r["mean"][1, 0] == np.float32(1.0 / 7.0) and r["count"][1, 0] == 7


def test_separating_cells_separate(pkg):
    """Every committed cell, by exact arithmetic: the definition and the fused evaluation give the committed, DIFFERENT float32 variances;
    in hand_built's data `reference` and its fused variant differ in exactly these cells' variance and in no other plane; and the
    default library's host function gives the definition's value."""
    u32 = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    n_entered, above, below, interrupted = [], 0, 0, 0
    for cell, bits, wall_at, defined, fused in SEPARATING_CELLS:
        vals = np.array(bits, np.uint32).view(np.float32)
        enters = [k != wall_at and np.isfinite(v) for k, v in enumerate(vals)]
        a, b = two_variances([float(v) for v, e in zip(vals, enters) if e])
        assert (u32(a), u32(b)) == (defined, fused) and defined != fused, (cell, hex(u32(a)), hex(u32(b)))
        assert abs(defined - fused) == 1  # neighbouring floats: the two Q are an ulp or two of a double apart
        n_entered.append(sum(enters))
        above, below = above + (b > a), below + (b < a)
        interrupted += not all(enters) and enters[0] and enters[-1]
    assert len(SEPARATING_CELLS) >= 4 and above >= 1 and below >= 1 and max(n_entered) >= 9 and interrupted >= 1
    assert any(wall_at is not None for _, _, wall_at, _, _ in SEPARATING_CELLS)
    complete = [[15, 16, 17], [], [15, 16, 17, 18, 19], [15, 16, 17], [15, 16, 17, 18], [15, 16, 17, 18, 19]]
    for (B, members), cells in zip(CASES + N_SEL_CASES, complete):
        f, w = hand_built(B)
        want, other = reference(f, w, members, THRESHOLD), reference(f, w, members, THRESHOLD, fused=True)
        here = separating_cells_in(B, members)
        differ = np.zeros((64, 4), bool)
        for cell, _, _, defined, fused in here:
            assert (want["variance"][cell].view(np.uint32) == defined).all() and (other["variance"][cell].view(np.uint32) == fused).all(), (B, cell)
            differ[cell] = True
        assert np.array_equal(want["variance"].view(np.uint32) != other["variance"].view(np.uint32), differ) and np.isfinite(want["variance"][differ]).all(), B
        for k in PLANES:
            assert k == "variance" or same_bits(want[k], other[k]), (B, k)
        got = pkg.engine.ens_stat_cells(f, w, members=members, threshold=THRESHOLD)
        check(got, want, ("separating", B))
        assert [s[0] for s in here] == cells, (B, members)


@pytest.mark.parametrize("B,members", CASES, ids=["7", "1", "70-masked"])
def test_host_function_equals_the_definition(pkg, B, members):
    f, w = hand_built(B)
    got = pkg.engine.ens_stat_cells(f, w, members=members, threshold=THRESHOLD)
    want = reference(f, w, members, THRESHOLD)
    check(got, want, B)
    # the cases are what they claim to be
    n_sel = B if members is None else len(members)
    assert (want["n_above"][..., 2] == 0).all() and (want["count"][10, 2] == n_sel)
    assert want["n_wall"][5] == n_sel and (want["count"][5] == 0).all() and np.isnan(want["mean"][5]).all() and (want["argmin"][5] == -1).all()
    assert (want["count"][4] == 0).all() and want["n_wall"][4] == 0 and np.isnan(want["max"][4]).all() and np.isnan(want["variance"][4]).all()
    assert (want["variance"][0] == 0).all() and (want["mean"][0] == 1.5).all()
    if B == 7:
        assert want["count"][3, 0] == 4 and want["min"][3, 0] == -3.0 and want["max"][3, 0] == 7.0
        assert want["n_wall"][6] == 3 and want["count"][6, 0] == 4 and want["argmin"][6, 0] == 5 and want["argmax"][6, 0] == 2
        z = np.float32(0).view(np.uint32)
        assert (want["min"][7, :2].view(np.uint32) == z).all() and (want["max"][7, :3].view(np.uint32) == z).all()
        assert want["argmin"][7, 0] == 0 and want["argmax"][7, 1] == 0 and want["argmax"][7, 2] == 0 and want["argmin"][7, 3] == 1
        assert want["min"][7, 3].view(np.uint32) == z
        assert want["argmin"][8, 0] == 2 and want["argmax"][8, 1] == 2 and want["min"][8, 0] == -7.0 and want["max"][8, 1] == 9.0
        assert want["n_above"][9].tolist() == [2, 2, 0, 2] and want["count"][9].tolist() == [7, 7, 7, 7]  # (members 1 and 4 hold the value just above)
        assert np.isfinite(want["mean"][2]).all() and want["max"][2, 0] == FLT_MAX
    if B == 70:
        assert want["count"].max() == 67 and not np.isin(want["argmin"], (0, 33, 69)).any() and not np.isin(want["argmax"], (0, 33, 69)).any()


def test_unwanted_planes_are_left_alone(pkg):
    """NULL output pointers are honoured: all nine planes lie back to back in ONE poisoned buffer, only some are handed in; the regions of
    the others keep the poison, and the wanted planes are what the full call returns."""
    E, L = pkg.engine, pkg.engine.lib()
    f, w = hand_built(7)
    full = E.ens_stat_cells(f, w, threshold=THRESHOLD)
    n = 64
    fp, wp = (C.c_void_p * 7)(*[a.ctypes.data for a in f]), (C.c_void_p * 7)(*[a.ctypes.data for a in w])
    for wanted in (("variance", "argmax", "n_wall"), ("mean",), ("min", "count", "n_above"), ()):
        buf = np.full(n * (8 * 4 + 1), 0x5A5A5A5A, np.uint32)
        st, at = E.WxEnsStat(), {}
        for k, name in enumerate(PLANES):
            at[name] = slice(4 * n * k, 4 * n * k + (n if name == "n_wall" else 4 * n))
            if name in wanted:
                setattr(st, name, buf.ctypes.data + 4 * at[name].start)
        st.threshold[:] = THRESHOLD
        assert L.wx_ens_stat_cells(7, n, fp, wp, None, C.byref(st)) == 0
        for name in PLANES:
            part = buf[at[name]]
            if name in wanted:
                assert same_bits(part.view(full[name].dtype).reshape(full[name].shape), full[name]), (wanted, name)
            else:
                assert (part == 0x5A5A5A5A).all(), (wanted, name)
    # the Python layer returns the wanted planes only
    some = E.ens_stat_cells(f, w, threshold=THRESHOLD, want=("mean", "n_wall"))
    assert set(some) == {"mean", "n_wall"} and same_bits(some["mean"], full["mean"]) and same_bits(some["n_wall"], full["n_wall"])


_FAST_LEG = """
import ctypes as C, sys, numpy as np
lib, src, dst = sys.argv[1:4]
L = C.CDLL(lib)
d = np.load(src)
f, w, mask, thr = d["f"], d["w"], d["mask"], d["thr"]
B, n = f.shape[:2]
class S(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in %r] + [("threshold", C.c_float * 4)]
out = {k: np.zeros((n,) if k == "n_wall" else (n, 4), np.float32 if k in ("mean", "variance", "min", "max") else np.int32) for k in %r}
st = S()
for k, a in out.items():
    setattr(st, k, a.ctypes.data)
st.threshold[:] = [float(t) for t in thr]
fp, wp = (C.c_void_p * B)(*[f[i].ctypes.data for i in range(B)]), (C.c_void_p * B)(*[w[i].ctypes.data for i in range(B)])
L.wx_ens_stat_cells.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
assert L.wx_arith() == 1, "not the tolerance build"
assert L.wx_ens_stat_cells(B, n, fp, wp, mask.ctypes.data, C.byref(st)) == 0
np.savez(dst, **out)
""" % (list(PLANES), list(PLANES))


def test_the_tolerance_build_gives_the_same_bits(pkg, tmp_path):
    """libwxsim_fast.so (contraction allowed everywhere else) on the data above: the per-cell function switches contraction off for
    itself. In a process of its own: a process holds one libwxsim."""
    fast = pkg.engine.FAST_LIB_PATH
    if not os.path.exists(fast):
        pytest.skip("libwxsim_fast.so is not built")
    for B, members in CASES:
        f, w = hand_built(B)
        mask = np.ones(B, np.uint8) if members is None else np.isin(np.arange(B), members).astype(np.uint8)
        src, dst = str(tmp_path / f"in{B}.npz"), str(tmp_path / f"out{B}.npz")
        np.savez(src, f=np.stack(f), w=np.stack(w), mask=mask, thr=np.asarray(THRESHOLD, np.float32))
        subprocess.check_call([sys.executable, "-c", _FAST_LEG, fast, src, dst], timeout=120)
        got = dict(np.load(dst))
        check(got, pkg.engine.ens_stat_cells(f, w, members=members, threshold=THRESHOLD), ("fast", B))
        check(got, reference(f, w, members, THRESHOLD), ("fast vs definition", B))
