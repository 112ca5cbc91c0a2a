"""The members' Gram matrix (wx_ensemble_gram, wx_ens_gram_cells, wx_ens_gram_max_members; include/wxsim.h) without a GPU: the header
announces and declares the addition at the unchanged ABI version, the library exports it, the kernel names are listed, the argument
checks answer before any device is touched, and the pure host entry point -- built from the kernels' own functions and wx_diag's integer
bins -- equals the definition in the header comment, which `reference` below restates independently: numpy float64 arithmetic,
`.astype(np.float32)` for the term, math.fsum per pair for the exact sum. Every comparison is `==` on bits."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ensemble_gram_shapes as GS
from test_ensemble_covariance_cpu import cov_members
from test_ensemble_statistics_cpu import FLT_MAX, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_gram", "wx_ens_gram_cells", "wx_ens_gram_max_members"]
E_INVALID, E_RANGE, E_STATE = -1, -4, -5
NAN, INF = float("nan"), float("inf")
B_, W_ = "BASE_CUR", "WATER_CUR"
CENTERS = ("mean", "none")
COUNTS = ("n_entered", "n_excluded", "n_overflow")
# (members of the ensemble, the selected ones): n = 2, 5, 9, 17, 33 and 64 -- one lane group and a remainder of the pre-pass's load
# groups, one pair tile and two and three, the cap -- two of them through a mask that skips members
SELECTIONS = [(2, None), (5, None), (11, [0, 1, 2, 4, 5, 7, 8, 9, 10]), (17, None), (33, None), (66, [i for i in range(66) if i not in (7, 40)])]


def selection(B, members):
    return list(range(B)) if members is None else sorted(int(i) for i in members)


def reference(fields, walls, X, Y, *, rect=None, members=None, center="mean"):
    """The definition of include/wxsim.h, straight from its text. Returns what engine.ens_gram_cells returns."""
    sel = selection(len(walls), members)
    n = len(sel)
    x0, y0, w, h = (0, 0, X, Y) if rect is None else rect
    f32 = np.stack([fields[k][y0:y0 + h, x0:x0 + w] for k in sel])  # (n, h, w, 4)
    air = np.all([walls[k][y0:y0 + h, x0:x0 + w, 1] != 0 for k in sel], axis=0)
    eligible = air[..., None] & np.isfinite(f32).all(axis=0)
    with np.errstate(all="ignore"):
        x = f32.astype(np.float64)
        S = np.zeros((h, w, 4))
        for k in range(n):  # member order, from +0.0
            S = S + x[k]
        xm = S / n if center == "mean" else np.zeros((h, w, 4))
        d = x - xm
        overflow = eligible & ~np.isfinite((d * d).astype(np.float32)).all(axis=0)
    entered = eligible & ~overflow
    gram = np.zeros((4, n, n))
    for c in range(4):
        dc = d[:, entered[..., c], c]  # (n, entered cells)
        for a in range(n):
            for b in range(a, n):
                with np.errstate(all="ignore"):
                    p = (dc[a] * dc[b]).astype(np.float32)
                assert np.isfinite(p).all()  # (the header's argument: the diagonal test is the whole test)
                gram[c, a, b] = gram[c, b, a] = math.fsum(p.astype(np.float64).tolist())
    return {"gram": gram, "n_entered": entered.sum(axis=(0, 1)).astype(np.int64), "n_excluded": (~eligible).sum(axis=(0, 1)).astype(np.int64),
            "n_overflow": overflow.sum(axis=(0, 1)).astype(np.int64), "members": sel}


def compare(got, want, where):
    """Bit for bit; a difference names channel and pair."""
    assert sorted(got) == sorted(want), where
    assert got["members"] == want["members"], where
    for k in COUNTS:
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, (where, k, got[k], want[k])
    a, b = got["gram"], want["gram"]
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64, where
    bad = a.view(np.uint64) != b.view(np.uint64)
    if bad.any():
        at = np.argwhere(bad)[:5].tolist()
        raise AssertionError((where, "channel, a, b:", at, [(float(a[tuple(i)]), float(b[tuple(i)])) for i in at], int(bad.sum())))


def check(pkg, fields, walls, X, Y, field, where, **kw):
    """engine.ens_gram_cells == reference, bit for bit; returns the host function's answer."""
    got = pkg.engine.ens_gram_cells(fields, walls, X, Y, field, **kw)
    compare(got, reference(fields, walls, X, Y, **kw), (where, kw))
    return got


# ---- THE PLANTED CELLS: nine cell kinds written into consecutive cells of a row. `sel`: the selected members, in order ----
BIG_A, BIG_B, BIG_M = np.float32(2.0 ** 64), np.float32(-(2.0 ** 64 - 2.0 ** 40)), np.float32(2.0 ** 39)
PLANTED = ("wall", "nan", "+inf", "-inf", "-0.0", "flt_max", "subnormal", "equal", "largest_finite")
N_PLANTED = len(PLANTED)


def row_cells(y, x0):
    return [(y, x0 + j) for j in range(N_PLANTED)]


def plant(fields, walls, sel, cells):
    """Cell cells[j] = (y, x) becomes planted cell j (an air cell with ordinary finite values everywhere, then the special ones), in
    the members `sel`. largest_finite: the members hold A, B, A, B, M, M ... with A = 2^64, B = -(2^64 - 2^40), M = 2^39 in channel 0:
    every partial sum is a multiple of 2^39 below 2^66, so the mean is exactly M and the deviations are +-s, s = 2^64 - 2^39, and 0;
    s*s = 2^128 - 2^104 + 2^78 converts to FLT_MAX, the largest finite float: on the diagonal it is not an overflow, and off the
    diagonal it is +-FLT_MAX. Without a centre A*A = 2^128 is an overflow. Returns {kind: (y, x)}."""
    n = len(sel)
    assert len(cells) == N_PLANTED
    at = dict(zip(PLANTED, cells))
    for k, i in enumerate(sel):
        for cell in cells:
            walls[i][cell + (1,)] = 5
            fields[i][cell] = np.float32([0.125 * (k + 1), -0.5 + 0.25 * k, 0.01 * (k % 3), 300.0 + k])
        fields[i][at["subnormal"] + (1,)] = np.float32((k + 1) * 1e-20)
        fields[i][at["equal"] + (2,)] = np.float32(0.75)
        fields[i][at["largest_finite"] + (0,)] = (BIG_A, BIG_B)[k % 2] if k < (4 if n >= 4 else 2) else BIG_M
    first, mid, last = sel[0], sel[n // 2], sel[-1]
    walls[mid][at["wall"] + (1,)] = 0
    fields[first][at["nan"] + (0,)] = NAN
    fields[last][at["+inf"] + (1,)] = INF
    fields[mid][at["-inf"] + (2,)] = -INF
    fields[first][at["-0.0"] + (3,)] = -0.0
    fields[last][at["flt_max"] + (0,)] = FLT_MAX
    return at


def planted_grid(B, members, X=70, Y=9, seed=5, field=B_):
    """Random members (a wall or a non-finite value in one member in one cell of twenty-five) with the planted cells in the first and in
    the last row, on both sides of the chunk boundary at x = 64. Returns (fields, walls, the planted rows)."""
    bases, waters, wl = cov_members(B, X, Y, seed=seed)
    fields = bases if field == B_ else waters
    sel = selection(B, members)
    for y in (0, Y - 1):
        plant(fields, wl, sel, row_cells(y, 60))
    return fields, wl, (0, Y - 1)


def planted_row(n, center):
    """The planted cells alone, one row of N_PLANTED cells: (fields, walls, {kind: x})."""
    fields = [np.zeros((1, N_PLANTED, 4), np.float32) for _ in range(n)]
    walls = [np.full((1, N_PLANTED, 4), 3, np.int8) for _ in range(n)]
    return fields, walls, plant(fields, walls, list(range(n)), row_cells(0, 0))


def planted_expectations(got, n, center):
    """What the planted cells of one row must give, whatever computed `got` = the result over exactly that row."""
    ent, exc, ovf = (got[k] for k in COUNTS)
    assert (ent + exc + ovf == N_PLANTED).all()
    # wall: all four channels; nan / +inf / -inf: one channel each
    assert exc.tolist() == [2, 2, 2, 1]
    # flt_max overflows with both centres; largest_finite only without a centre
    assert ovf.tolist() == [1 if center == "mean" else 2, 0, 0, 0]
    g = got["gram"]
    assert (g == np.swapaxes(g, 1, 2)).all() and (np.diagonal(g, axis1=1, axis2=2) >= 0).all() and np.isfinite(g).all()
    if center == "mean":  # channel 0: the ordinary cells' deviations are below 8, the largest-finite cell dominates exactly where it must
        big = [k for k in range(n) if k < (4 if n >= 4 else 2)]
        for a in big:
            for b in big:
                sign = 1.0 if (a - b) % 2 == 0 else -1.0
                assert abs(g[0, a, b] - sign * float(FLT_MAX)) <= float(FLT_MAX) * 2.0 ** -50, (a, b, g[0, a, b])


C_SIZES = {"int32_t": 4, "int64_t": 8, "float": 4, "double": 8}


def header_struct(hdr, tag):
    """[(member, bytes)] of `typedef struct tag { ... } tag;` as the header declares it: pointers are 8 bytes, arrays count whole."""
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct %s {" % tag):hdr.index("} %s;" % tag)].split("{", 1)[1], flags=re.S)
    out = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        ctype, names = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s+(.*)", decl, flags=re.S).groups()
        for name in names.split(","):
            m = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", name)
            out.append((m.group(2), 8 if m.group(1) else C_SIZES[ctype] * int(m.group(3) or 1)))
    return out


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.engine.lib()


def test_header_announces_and_library_exports(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    for name, v in (("WX_HAVE_ENSEMBLE_GRAM", 1), ("WX_ENS_GRAM_MAX_MEMBERS", 64), ("WX_GRAM_CENTER_MEAN", 0), ("WX_GRAM_CENTER_NONE", 1), ("WX_ABI_VERSION", 11)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, v), hdr, re.M), name
    E = pkg.engine
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in E.EXPORTS, n
        getattr(lib, n)
    assert lib.wx_abi_version() == 11 and lib.wx_ens_gram_max_members() == 64 == E.ENS_GRAM_MAX_MEMBERS and E.GRAM_CENTERS == {"mean": 0, "none": 1}
    assert callable(E.Ensemble.gram) and callable(E.ens_gram_cells)
    for m in ("gram", "distances", "medoid", "eofs"):
        assert callable(getattr(pkg.sim.WeatherEnsemble, m))
    names = [lib.wx_kernel_name(k).decode() for k in range(lib.wx_kernel_count())]
    assert names.count("ensemble_gram_centre") == 1 and names.count("ensemble_gram") == 1 and len(set(names)) == len(names)
    # the ctypes struct is the header's, member for member
    assert header_struct(hdr, "wx_ens_gram") == [(f[0], C.sizeof(f[1])) for f in E.WxEnsGram._fields_]
    assert C.sizeof(E.WxEnsGram) == 136 and E.WxEnsGram.gram.offset == 24 and E.WxEnsGram.n_entered.offset == 32 and E.WxEnsGram.n_selected.offset == 128
    # the kernels state their launch shape where a test can read it
    c = GS.caps()
    assert c["TILE"] ** 2 == c["WG"] and 64 % c["TILE"] == 0 and GS.jobs(64, c) == 40 and GS.jobs(16, c) == 4 and GS.jobs(17, c) == 12 and GS.jobs(64, c) <= c["MAX_WGS"]


def test_the_tall_case_takes_a_second_trip_in_both_kernels():
    c = GS.caps()
    X, Y = GS.tall_grid()
    assert 2 <= X and Y <= 65535  # (what wx_create accepts)
    chunks = -(-X // 64) * Y
    waves = GS.centre_workers(chunks, c)
    assert waves < chunks <= 2 * waves  # exactly two trips for the pre-pass's busiest waves
    slots = GS.pair_slots(chunks, GS.TALL_MEMBERS, c)
    assert slots * GS.jobs(GS.TALL_MEMBERS, c) <= c["MAX_WGS"] and chunks > 2 * slots  # ... and more for the pair kernel's slots
    first, last = GS.tall_planted_rows()
    rows = GS.tall_planted_block_rows()
    assert first + rows <= slots <= waves <= last and last + rows < Y  # a planted block in the first and in the last trip of both
    assert GS.TALL_MEMBERS % c["UNROLL"] == 3  # (three members: the remainder of the member walk alone)


def test_every_refusal_with_its_code(pkg, lib):
    E = pkg.engine
    B, X, Y = 3, 6, 5
    bases, _, walls = cov_members(B, X, Y, bad=0)
    ptrs = lambda arrs: (C.c_void_p * B)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    fp, lp = ptrs(bases), ptrs(walls)
    out = np.full((4, 64, 64), 7.0)

    def call(field=0, center=0, rect=(2, 1, 3, 3), n=B, fp=fp, lp=lp, mask=None, desc=True, gram=True, XY=(X, Y)):
        g = E.WxEnsGram()
        g.field, g.center = field, center
        g.x, g.y, g.w, g.h = rect
        g.gram = out.ctypes.data if gram else None
        g.n_selected = -5
        out[...] = 7.0
        rc = lib.wx_ens_gram_cells(C.byref(g) if desc else None, XY[0], XY[1], n, fp, lp, mask)
        assert rc == 0 or ((out == 7.0).all() and g.n_selected == -5 and g.n_entered[0] == 0)  # a refused call writes nothing
        assert rc != 0 or (g.n_selected == (n if mask is None else sum(mask)) and (out.reshape(-1)[:4 * g.n_selected ** 2] != 7.0).all())
        return rc

    assert call() == 0 and call(center=1) == 0 and call(field=3) == 0  # the good calls: the refusals are not vacuous
    # WX_E_INVALID
    assert lib.wx_ensemble_gram(None, C.byref(E.WxEnsGram()), None) == E_INVALID and lib.wx_ensemble_gram(None, None, None) == E_INVALID
    assert call(desc=False) == E_INVALID
    for field in (1, 2, 4, -1, 13):
        assert call(field=field) == E_INVALID, field
    for center in (2, -1, 99):
        assert call(center=center) == E_INVALID, center
    assert call(gram=False) == E_INVALID
    one, none, two = (C.c_uint8 * B)(0, 1, 0), (C.c_uint8 * B)(0, 0, 0), (C.c_uint8 * B)(1, 0, 1)
    assert call(mask=one) == E_INVALID and call(mask=none) == E_INVALID and call(mask=two) == 0  # MEAN: two members
    assert call(center=1, mask=one) == 0 and call(center=1, mask=none) == E_INVALID  # NONE: one member
    assert call(n=0) == E_INVALID and call(n=1) == E_INVALID and call(n=1, center=1) == 0
    assert call(fp=None) == E_INVALID and call(lp=None) == E_INVALID and call(XY=(0, Y)) == E_INVALID and call(XY=(X, 0)) == E_INVALID
    assert call(fp=ptrs([bases[0], None, bases[2]])) == E_INVALID and call(lp=ptrs([walls[0], walls[1], None])) == E_INVALID
    assert call(fp=ptrs([bases[0], None, bases[2]]), lp=ptrs([walls[0], None, walls[2]]), mask=two) == 0  # an absent unselected member
    many = 65
    fm, wm = (C.c_void_p * many)(*[bases[0].ctypes.data] * many), (C.c_void_p * many)(*[walls[0].ctypes.data] * many)
    for center in (0, 1):
        assert call(center=center, n=many, fp=fm, lp=wm) == E_INVALID
        assert call(center=center, n=many, fp=fm, lp=wm, mask=(C.c_uint8 * many)(*([1] * 64 + [0]))) == 0
    # WX_E_RANGE
    for rect in ((-1, 1, 3, 3), (2, -1, 3, 3), (2, 1, 0, 3), (2, 1, 3, 0), (4, 1, 3, 3), (2, 3, 3, 3), (0, 0, X + 1, 1)):
        assert call(rect=rect) == E_RANGE, rect
    with pytest.raises(E.WxError) as ei:
        E.ens_gram_cells(bases, walls, X, Y, B_, members=[1])
    assert ei.value.code == E_INVALID
    with pytest.raises(E.WxError) as ei:
        E.ens_gram_cells(bases, walls, X, Y, B_, rect=(0, 0, X, Y + 1))
    assert ei.value.code == E_RANGE


@pytest.mark.parametrize("B,members", SELECTIONS, ids=lambda v: None if isinstance(v, list) else str(v))
def test_host_function_equals_the_definition_on_random_members(pkg, B, members):
    X, Y = 70, 9
    n = len(selection(B, members))
    assert n in (2, 5, 9, 17, 33, 64)
    for field in (B_, W_):
        fields, wl, rows = planted_grid(B, members, X, Y, field=field)
        for center in CENTERS:
            for rect in (None, (3, 1, 64, Y - 2)) if field == B_ else (None,):
                got = check(pkg, fields, wl, X, Y, field, (B, field), rect=rect, members=members, center=center)
                w, h = (X, Y) if rect is None else rect[2:]
                assert (got["n_entered"] + got["n_excluded"] + got["n_overflow"] == w * h).all()
                # the condition on the random cases: a wrong entry test cannot hide behind empty sums
                assert (got["n_entered"] > 0.8 * w * h).all() and (got["n_excluded"] > 0).all() and (rect is not None or got["n_overflow"][0] >= 2)
                g = got["gram"]
                assert (g == np.swapaxes(g, 1, 2)).all() and (np.diagonal(g, axis1=1, axis2=2) > 0).all()


@pytest.mark.parametrize("n", [2, 3, 5, 64])
@pytest.mark.parametrize("center", CENTERS)
def test_planted_cells(pkg, n, center):
    fields, walls, at = planted_row(n, center)
    got = check(pkg, fields, walls, N_PLANTED, 1, B_, ("planted", n), center=center)
    planted_expectations(got, n, center)
    # the subnormal products: the cell alone, channel 1
    x = at["subnormal"][1]
    alone = check(pkg, fields, walls, N_PLANTED, 1, B_, ("subnormal", n), center=center, rect=(x, 0, 1, 1))
    tiny = alone["gram"][1]
    assert alone["n_entered"][1] == 1 and tiny[0, 0] > 0 and (np.abs(tiny) < 2.0 ** -100).all() and (np.abs(tiny[tiny != 0]) < 2.0 ** -126).any()
    assert all(float(np.float32(v)) == v for v in tiny.reshape(-1))  # one float each: a subnormal or a small normal float, exactly
    # the largest finite float, alone
    x = at["largest_finite"][1]
    alone = check(pkg, fields, walls, N_PLANTED, 1, B_, ("largest finite", n), center=center, rect=(x, 0, 1, 1))
    if center == "mean":
        assert alone["n_entered"][0] == 1 and alone["gram"][0, 0, 0] == float(FLT_MAX) and alone["gram"][0, 0, 1] == -float(FLT_MAX)
        assert n < 4 or alone["gram"][0, 0, 2] == float(FLT_MAX)  # off the diagonal
    else:
        assert alone["n_overflow"][0] == 1 and (alone["gram"][0] == 0).all()
    # -0.0 enters like 0.0
    x = at["-0.0"][1]
    alone = check(pkg, fields, walls, N_PLANTED, 1, B_, ("-0.0", n), center="none", rect=(x, 0, 1, 1))
    assert alone["n_entered"][3] == 1 and (alone["gram"][3, 0] == 0).all() and not np.signbit(alone["gram"][3]).any()


def test_equal_members_give_an_exact_zero_matrix_and_nothing_gives_plus_zero(pkg):
    X, Y, n = 13, 6, 5
    bases, _, wl = cov_members(1, X, Y, bad=3)
    fields, walls = [bases[0].copy() for _ in range(n)], [wl[0].copy() for _ in range(n)]
    got = check(pkg, fields, walls, X, Y, B_, "equal members", center="mean")
    assert (got["gram"].view(np.uint64) == 0).all() and (got["n_entered"] > 0).all()
    raw = check(pkg, fields, walls, X, Y, B_, "equal members, raw", center="none")
    assert (raw["gram"] > 0).all() and (raw["gram"] == raw["gram"][:, :1, :1]).all()
    for w in walls:
        w[..., 1] = 0
    got = check(pkg, fields, walls, X, Y, B_, "all walls", center="none")
    assert (got["gram"].view(np.uint64) == 0).all() and (got["n_excluded"] == X * Y).all()


def test_properties_symmetry_member_order_cell_order(pkg):
    E = pkg.engine
    B, X, Y = 9, 70, 9
    fields, wl, _ = planted_grid(B, None, X, Y)
    for center in CENTERS:
        whole = E.ens_gram_cells(fields, wl, X, Y, B_, center=center)
        g = whole["gram"]
        assert (g.view(np.uint64) == np.swapaxes(g, 1, 2).view(np.uint64)).all() and (np.diagonal(g, axis1=1, axis2=2) >= 0).all()
        assert (whole["n_entered"] + whole["n_excluded"] + whole["n_overflow"] == X * Y).all()
        # the cells in reverse order: the same bits
        rev = E.ens_gram_cells([f[::-1, ::-1] for f in fields], [w[::-1, ::-1] for w in wl], X, Y, B_, center=center)
        compare(rev, whole, ("reversed cells", center))
    # without a centre the members' order does not matter either: permuting them permutes the matrix bit for bit
    perm = [4, 0, 8, 2, 6, 1, 7, 3, 5]
    raw = E.ens_gram_cells(fields, wl, X, Y, B_, center="none")
    shuffled = E.ens_gram_cells([fields[i] for i in perm], [wl[i] for i in perm], X, Y, B_, center="none")
    assert same_bits(shuffled["gram"], raw["gram"][:, perm][:, :, perm])
    for k in COUNTS:
        assert np.array_equal(shuffled[k], raw[k])
    # a sub-selection is the sub-matrix only without a centre (with one, the mean changes)
    sub = E.ens_gram_cells(fields, wl, X, Y, B_, center="none", members=[1, 4, 6], rect=(0, 1, X, Y - 2))
    full = E.ens_gram_cells(fields, wl, X, Y, B_, center="none", rect=(0, 1, X, Y - 2))
    if np.array_equal(sub["n_entered"], full["n_entered"]):  # (only if no other member excludes a cell of the rectangle)
        assert same_bits(sub["gram"], full["gram"][:, [1, 4, 6]][:, :, [1, 4, 6]])


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_gram_cpu as T
out = {}
for j, (B, members, center) in enumerate(T.FAST_CASES):
    fields, wl, _ = T.planted_grid(B, members)
    got = pkg.engine.ens_gram_cells(fields, wl, 70, 9, T.B_, members=members, center=center)
    out["gram%d" % j] = got["gram"]
    for k in T.COUNTS:
        out["%s%d" % (k, j)] = got[k]
np.savez(sys.argv[2], **out)
"""
FAST_CASES = [(5, None, "mean"), (11, [0, 1, 2, 4, 5, 7, 8, 9, 10], "none"), (17, None, "mean")]


def test_the_tolerance_build_host_function_gives_the_same_bits(pkg, tmp_path):
    """libwxsim_fast.so (-ffp-contract=fast) in a process of its own: its host function gives the bits of this process's."""
    E = pkg.engine
    assert os.path.exists(E.FAST_LIB_PATH), "libwxsim_fast.so is built by __graft_entry__.build()"
    path = str(tmp_path / "fast.npz")
    out = subprocess.run([sys.executable, "-c", _FAST_LEG, ROOT, path], env=dict(os.environ, WXSIM_LIB=E.FAST_LIB_PATH), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    d = np.load(path)
    for j, (B, members, center) in enumerate(FAST_CASES):
        fields, wl, _ = planted_grid(B, members)
        want = E.ens_gram_cells(fields, wl, 70, 9, B_, members=members, center=center)
        assert same_bits(d["gram%d" % j], want["gram"]) and all(np.array_equal(d["%s%d" % (k, j)], want[k]) for k in COUNTS), (B, center)


def test_host_function_under_the_sanitizers(tmp_path):
    """tests/native/ens_gram_main.cpp -- the header and a main() that runs wxg::gram_cells over the planted cells and over randomised
    arrays that end exactly at the last cell -- compiled stand-alone with AddressSanitizer and UBSan (host compiler, no device, no
    library) and run."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.call(["which", c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ens_gram_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "ens_gram_main.cpp")], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ens_gram_main ok" in out.stdout
