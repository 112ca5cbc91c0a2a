"""Diagnostics (include/wxsim.h: wx_diag) without a GPU: the binning function and the one rounding of wx_diag_finish against
math.fsum BIT FOR BIT, the merge laws, the per-cell rules through wx_diag_accumulate_cells (the kernel's own host/device function run
on the CPU), and the ctypes mirror of the struct."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E(pkg):
    pkg.engine.build()
    return pkg.engine


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def exact_sum(E, values, quantity="water", parts=1):
    v = np.asarray(values, np.float32).ravel()
    raw = E.diag_empty()
    for chunk in np.array_split(v, parts):
        raw = E.diag_accumulate(raw, quantity, chunk)
    return E.diag_finish(raw)["sum_water"][0]


def fsum32(values):
    v = np.asarray(values, np.float32).ravel()
    return math.fsum(float(x) for x in v[np.isfinite(v)])


CASES = {
    "normal": lambda r: r.normal(0, 1, 5000),
    "one_bin": lambda r: r.uniform(1.0, 1.9, 4096),  # exponent 127 only
    "all_16_bins": lambda r: np.concatenate([np.float32(2.0) ** np.arange(-126, 128, 1), -np.float32(2.0) ** np.arange(-126, 128, 3), r.normal(0, 1, 64)]),
    "cancel_huge": lambda r: [3e38, 1e-30, -3e38],
    "tenth_2p20": lambda r: np.full(1 << 20, 0.1, np.float32),
    "subnormals": lambda r: np.concatenate([np.arange(1, 200).astype(np.uint32).view(np.float32), [-0.0, 0.0], -np.arange(5, 90).astype(np.uint32).view(np.float32)]),
    "cancel_to_subnormal": lambda r: np.array([1.0, -1.0, 3.5e-42, 7e37, -7e37, 1e-3, -1e-3, -1.4e-45], np.float32),
    "wide_random": lambda r: (r.normal(0, 1, 3000) * np.float32(2.0) ** r.integers(-120, 120, 3000)).astype(np.float32),
    "minus_zero_only": lambda r: [-0.0, -0.0],
    "empty": lambda r: [],
    "max_floats": lambda r: np.full(1000, np.finfo(np.float32).max, np.float32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulate_finish_equals_fsum_bit_for_bit(E, name):
    with np.errstate(over="ignore"):
        v = np.asarray(CASES[name](np.random.default_rng(11)), np.float64).astype(np.float32)
    assert np.isfinite(v).all()
    got, want = exact_sum(E, v), fsum32(v)
    assert bits(got) == bits(want), (name, got, want)
    assert bits(exact_sum(E, v[::-1], parts=7)) == bits(want)  # any order, any split


def test_final_rounding_ties_go_to_even(E):
    # 2^53 + 1 lies exactly between two doubles: nearest-even gives 2^53; 2^53 + 3 gives 2^53 + 4; one more bit of weight breaks the tie upwards
    assert bits(exact_sum(E, [2.0 ** 53, 1.0])) == bits(2.0 ** 53) == bits(math.fsum([2.0 ** 53, 1.0]))
    assert bits(exact_sum(E, [2.0 ** 53, 2.0, 1.0])) == bits(2.0 ** 53 + 4) == bits(math.fsum([2.0 ** 53, 2.0, 1.0]))
    assert bits(exact_sum(E, [2.0 ** 53, 1.0, 2.0 ** -100])) == bits(2.0 ** 53 + 2)
    assert bits(exact_sum(E, [-(2.0 ** 53), -1.0])) == bits(-(2.0 ** 53))
    assert bits(exact_sum(E, [1.0, -1.0])) == bits(0.0)  # an exact zero is +0.0


def test_nonfinite_values_are_skipped_by_accumulate(E):
    v = np.array([1.5, np.nan, np.inf, -np.inf, 2.25], np.float32)
    assert bits(exact_sum(E, v)) == bits(3.75)


def test_accumulate_rejects_bad_arguments(E):
    L = E.lib()
    raw = E.WxDiagRaw()
    one = np.ones(1, np.float32)
    assert L.wx_diag_accumulate(None, 0, one.ctypes.data, 1) == -1
    assert L.wx_diag_accumulate(C.byref(raw), E.DIAG_QUANTITIES, one.ctypes.data, 1) == -1
    assert L.wx_diag_accumulate(C.byref(raw), -1, one.ctypes.data, 1) == -1
    assert L.wx_diag_accumulate(C.byref(raw), 0, None, 1) == -1
    assert L.wx_diag_finish(None, C.byref(E.WxDiag())) == -1 and L.wx_diag_finish(C.byref(raw), None) == -1
    assert L.wx_diag_merge(None, C.byref(raw)) == -1 and L.wx_diag_merge(C.byref(raw), None) == -1
    assert L.wx_diagnostics(None, C.byref(E.WxDiag())) == -1 and L.wx_group_diagnostics(None, C.byref(E.WxDiag())) == -1
    assert L.wx_diag_collect(None, C.byref(raw)) == -1


def test_merge_is_commutative_and_associative(E):
    rng = np.random.default_rng(5)
    v = (rng.normal(0, 1, 6000) * np.float32(2.0) ** rng.integers(-60, 60, 6000)).astype(np.float32)
    want = fsum32(v)
    cuts = np.sort(rng.choice(np.arange(1, len(v)), 5, replace=False))
    parts = [E.diag_accumulate(E.diag_empty(), "smoke", p) for p in np.split(v, cuts)]
    results = set()
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 4, 3]):
        left = E.diag_empty()
        for k in order:
            left = E.diag_merge(left, parts[k])
        results.add(left)
        right = parts[order[-1]]  # ... and grouped from the other end
        for k in order[-2::-1]:
            right = E.diag_merge(parts[k], right)
        results.add(right)
    assert len(results) == 1  # one representation per value: the merged BYTES are identical, not only the finished numbers
    assert bits(E.diag_finish(results.pop())["sum_water"][3]) == bits(want)
    assert E.diag_merge(parts[0], E.diag_empty()) == parts[0] == E.diag_merge(E.diag_empty(), parts[0])


def scene(rng, X, Y):
    base = rng.normal(0, 1, (Y, X, 4)).astype(np.float32)
    water = rng.uniform(0, 3, (Y, X, 4)).astype(np.float32)
    wall = np.zeros((Y, X, 4), np.int8)
    wall[..., 1] = rng.integers(0, 3, (Y, X))  # distance 0 = wall
    wall[..., 3] = rng.integers(-5, 120, (Y, X))
    water[..., 0] = np.where(wall[..., 1] == 0, 1111.0, water[..., 0])
    return base, water, wall


def reference(base, water, wall, x_of=None):
    """The same numbers from numpy masks and math.fsum (global x = x_of[column])."""
    Y, X = wall.shape[:2]
    xs = np.arange(X) if x_of is None else np.asarray(x_of)
    iswall = wall[..., 1] == 0
    air = ~iswall
    d = {"n_air": int(air.sum()), "n_wall": int(iswall.sum())}
    d["n_marker_mismatch"] = int(((water[..., 0] > 1000) != iswall).sum())
    d["n_negative_water"] = int((air & (water[..., 0] < 0)).sum())
    d["sum_vegetation"] = int(wall[..., 3][iswall].astype(np.int64).sum())
    for name, f in (("base", base), ("water", water)):
        nf = ~np.isfinite(f).all(axis=-1)
        d["n_nonfinite_" + name] = int(nf.sum())
        yy, xx = np.nonzero(nf)
        d["first_nonfinite_" + name] = min(((int(y), int(xs[x])) for y, x in zip(yy, xx)), key=lambda t: (t[0], t[1]), default=None)
        if d["first_nonfinite_" + name] is not None:
            d["first_nonfinite_" + name] = d["first_nonfinite_" + name][::-1]
        sums, mins, maxs, min_at, max_at = [], [], [], [], []
        for c in range(4):
            v = f[..., c]
            sums.append(math.fsum(float(t) for t in v[air & np.isfinite(v)]))
            ok = air & ~np.isnan(v)
            for best, vals, ats in ((np.min, mins, min_at), (np.max, maxs, max_at)):
                if not ok.any():
                    vals.append(None), ats.append(None)
                    continue
                m = best(v[ok])
                yy, xx = np.nonzero(ok & (v == m))
                y, x = min(zip(yy.tolist(), xs[xx].tolist()))
                vals.append(float(m)), ats.append((x, y))
        d["sum_" + name], d["min_" + name], d["max_" + name], d["min_" + name + "_at"], d["max_" + name + "_at"] = sums, mins, maxs, min_at, max_at
    d["sum_soil_moisture"] = math.fsum(float(t) for t in water[..., 2][iswall & np.isfinite(water[..., 2])])
    d["sum_snow"] = math.fsum(float(t) for t in water[..., 3][iswall & np.isfinite(water[..., 3])])
    return d


def cells_raw(E, base, water, wall, X, Y, cols):
    raw = E.diag_empty()
    for y in range(Y):
        raw = E.diag_accumulate_cells(raw, X, Y, cols[0], y, base[y, cols], water[y, cols], wall[y, cols])
    return raw


def assert_matches(got, want):
    for k, v in want.items():
        if isinstance(v, list) and v and isinstance(v[0], float):
            assert [bits(a) for a in got[k]] == [bits(b) for b in v] or got[k] == v, (k, got[k], v)  # (== also lets -0.0 meet 0.0 in an extreme)
        assert got[k] == v, (k, got[k], v)


def test_cells_on_the_cpu_match_numpy_and_fsum(E):
    X, Y = 150, 9
    base, water, wall = scene(np.random.default_rng(2), X, Y)
    got = E.diag_finish(cells_raw(E, base, water, wall, X, Y, np.arange(X)))
    assert_matches(got, reference(base, water, wall))
    assert got["n_droplets_active"] == 0 and got["sum_droplet_mass_x"] == 0.0


def test_planted_values_and_tie_rules_across_a_merge(E):
    X, Y = 96, 6
    base, water, wall = scene(np.random.default_rng(3), X, Y)
    wall[..., 1] = 1
    wall[0, :, 1] = 0
    water[0, :, 0] = 1111.0
    water[1:, :, 0] = np.minimum(np.abs(water[1:, :, 0]), 5.0)  # (scene() marked its own random walls)
    base[..., 3] = 280.0
    base[4, 70, 3] = base[2, 10, 3] = base[2, 80, 3] = 300.0  # the maximum three times: (10, 2) comes first in global order
    base[3, 5, 2] = -0.0
    base[..., 2] = np.where(base[..., 2] < 0, -base[..., 2], base[..., 2])
    base[3, 5, 2], base[3, 60, 2] = 0.0, -0.0                   # the minimum of P is a zero, twice, with either sign: (5, 3) wins
    base[1, 50, 0], base[5, 3, 1] = np.nan, np.inf              # first non-finite base cell: (50, 1)
    water[2, 90, 3], water[2, 20, 3] = -np.inf, np.nan          # first non-finite water cell: (20, 2); the minimum of smoke is -inf at (90, 2)
    water[4, 40, 0] = -2.5                                      # one negative total water
    water[0, 7, 0] = 12.0                                       # a wall cell without its marker
    water[5, 8, 0] = 2000.0                                     # an air cell with the marker
    base[1, 60:63, 0] = [3e38, -3e38, 1e-30]
    want = reference(base, water, wall)
    assert want["max_base_at"][3] == (10, 2) and want["min_base_at"][2] == (5, 3)
    assert want["first_nonfinite_base"] == (50, 1) and want["first_nonfinite_water"] == (20, 2)
    assert want["n_negative_water"] == 1 and want["n_marker_mismatch"] == 2 and want["min_water"][3] == -math.inf
    whole = cells_raw(E, base, water, wall, X, Y, np.arange(X))
    assert_matches(E.diag_finish(whole), want)
    # three disjoint column sets, merged in two orders: the bytes of the undecomposed pass
    parts = [cells_raw(E, base, water, wall, X, Y, np.arange(a, b)) for a, b in ((0, 11), (11, 75), (75, 96))]
    m1 = E.diag_merge(E.diag_merge(parts[0], parts[1]), parts[2])
    m2 = E.diag_merge(parts[2], E.diag_merge(parts[1], parts[0]))
    assert m1 == m2 == whole
    with pytest.raises(E.WxError):  # parts of two different domains do not merge
        E.diag_merge(whole, cells_raw(E, base, water, wall, X + 1, Y, np.arange(4)))


def test_no_air_cells_means_no_extremes(E):
    X, Y = 8, 4
    base, water, wall = scene(np.random.default_rng(4), X, Y)
    wall[..., 1] = 0
    got = E.diag_finish(cells_raw(E, base, water, wall, X, Y, np.arange(X)))
    assert got["n_air"] == 0 and got["n_wall"] == 32 and got["max_base"] == [None] * 4 and got["min_water_at"] == [None] * 4
    assert got["sum_base"] == [0.0] * 4 and got["first_nonfinite_base"] is None


def test_ctypes_structs_mirror_the_header(E):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    ctype_of = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(WX_DIAG_[A-Z]+)\s+(\d+)", hdr)}
    assert consts == {"WX_DIAG_QUANTITIES": E.DIAG_QUANTITIES, "WX_DIAG_BINS": E.DIAG_BINS}
    for cname, S in (("wx_diag", E.WxDiag), ("wx_diag_raw", E.WxDiagRaw)):
        body = hdr[hdr.index("typedef struct %s {" % cname):hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body.split("{", 1)[1], flags=re.S)
        fields = []
        for decl in body.split(";"):
            m = re.match(r"\s*(int64_t|uint64_t|double)\s+(.*)", decl.strip(), flags=re.S)
            if not m:
                assert not decl.strip(), decl  # doubles and 64-bit integers only
                continue
            for item in m.group(2).split(","):
                name = re.match(r"\s*(\w+)", item).group(1)
                t = ctype_of[m.group(1)]
                for dim in reversed(re.findall(r"\[(\w+)\]", item)):
                    t = t * int(consts.get(dim, dim) if not dim.isdigit() else dim)
                fields.append((name, t))
        assert [f[0] for f in fields] == [f[0] for f in S._fields_], cname
        assert [C.sizeof(f[1]) for f in fields] == [C.sizeof(f[1]) for f in S._fields_], cname
        assert C.sizeof(S) == sum(C.sizeof(f[1]) for f in fields)
    assert "#define WX_HAVE_DIAGNOSTICS 1" in hdr and E.lib().wx_abi_version() == 11
