"""Ensemble perturbation (wx_ensemble_perturb, wx_ens_perturb_cells; include/wxsim.h) without a GPU: the header announces and declares
the addition at the unchanged ABI version, the library exports it, the argument checks answer before any device is touched, and the pure
host entry point -- the kernel's own per-cell function -- equals the definition in the header comment, which `reference` below restates
in numpy: wrapping uint32 for the hash, float64 with ONE numpy operation per rounded operation for the rest. Every comparison is `==` on
bits, NaNs compared as positions."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_ensemble_statistics_cpu import FLT_MAX, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_perturb", "wx_ens_perturb_cells"]
E_INVALID, E_RANGE = -1, -4
NAN = float("nan")


def hash_u32(x):
    """common.glsl:103-111 on uint32 arrays (numpy wraps)."""
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x += x << np.uint32(10)
        x ^= x >> np.uint32(6)
        x += x << np.uint32(3)
        x ^= x >> np.uint32(11)
        x += x << np.uint32(15)
    return x


def node(seed, member, c, gx, gy):
    with np.errstate(over="ignore"):
        inner = hash_u32(np.uint32((4 * member + c) & 0xFFFFFFFF) + hash_u32(np.uint32(seed)))
        h = hash_u32(np.asarray(gx, np.uint32) + hash_u32(np.asarray(gy, np.uint32) + inner))
    k = (h >> np.uint32(8)).astype(np.float64)
    k = k - 8388608.0
    return k / 8388608.0


def noise(X, x, y, member, c, *, scale, seed, wrap_x):
    """r of the header at the absolute cells (x, y) (int64 arrays of one shape)."""
    gx, gy = x // scale, y // scale
    right, length = gx + 1, np.full(x.shape, scale, np.int64)
    if wrap_x:
        last = gx == (X - 1) // scale
        right = np.where(last, 0, right)
        length = np.where(last, X - gx * scale, length)
    tx = (x - gx * scale).astype(np.float64) / length.astype(np.float64)
    ty = (y - gy * scale).astype(np.float64) / np.float64(scale)
    u00, u10 = node(seed, member, c, gx, gy), node(seed, member, c, right, gy)
    u01, u11 = node(seed, member, c, gx, gy + 1), node(seed, member, c, right, gy + 1)
    sx, sy = 1.0 - tx, 1.0 - ty
    p00, p10, p01, p11 = sx * u00, tx * u10, sx * u01, tx * u11
    bottom, top = p00 + p10, p01 + p11
    qb, qt = sy * bottom, ty * top
    return qb + qt


def reference(fields, walls, X, Y, *, amplitude, mode=0, scale=1, seed=0, wrap_x=False, rect=None, members=None, lo=(NAN,) * 4, hi=(NAN,) * 4):
    """The definition of include/wxsim.h over the rectangle's cells of every member: new arrays."""
    x0, y0, w, h = (0, 0, X, Y) if rect is None else rect
    yy, xx = np.meshgrid(np.arange(y0, y0 + h, dtype=np.int64), np.arange(x0, x0 + w, dtype=np.int64), indexing="ij")
    out = []
    for i, (f, wl) in enumerate(zip(fields, walls)):
        if f is None or (members is not None and i not in members):
            out.append(None if f is None else f.copy())
            continue
        o = f.copy()
        air = wl[..., 1] != 0
        with np.errstate(all="ignore"):
            for c in range(4):
                a = np.float32(amplitude[c])
                if a == 0:
                    continue
                v = f[..., c]
                r = noise(X, xx, yy, i, c, scale=scale, seed=seed, wrap_x=wrap_x)
                ar = np.float64(a) * r
                if mode == 0:
                    d = v.astype(np.float64) + ar
                else:
                    fac = 1.0 + ar
                    d = v.astype(np.float64) * fac
                n = d.astype(np.float32)
                if lo[c] == lo[c]:
                    n = np.where(n < np.float32(lo[c]), np.float32(lo[c]), n)
                if hi[c] == hi[c]:
                    n = np.where(n > np.float32(hi[c]), np.float32(hi[c]), n)
                o[..., c] = np.where(air & np.isfinite(v) & np.isfinite(n), n, v)
        out.append(o)
    return out


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-40, 3e-39, FLT_MAX, -FLT_MAX, 1.0, -2.5, 290.0, 1e-3], np.float32)


def hand_built(B, X, Y, seed=11):
    """B members x (Y, X) cells: ordinary values, the special ones sprinkled over them, random walls (different per member)."""
    rng = np.random.Generator(np.random.Philox(seed + 1000 * B + X))
    f = (rng.standard_normal((B, Y, X, 4)) * np.array([0.3, 0.3, 0.01, 30.0]) + np.array([0, 0, 0, 280.0])).astype(np.float32)
    pick = rng.random((B, Y, X, 4)) < 0.25
    f[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
    w = np.zeros((B, Y, X, 4), np.int8)
    w[..., 1] = np.where(rng.random((B, Y, X)) < 0.2, 0, rng.integers(1, 100, (B, Y, X))).astype(np.int8)
    w[..., 3] = rng.integers(0, 100, (B, Y, X)).astype(np.int8)
    return [np.ascontiguousarray(f[i]) for i in range(B)], [np.ascontiguousarray(w[i]) for i in range(B)]


def check(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), (where, "member", i, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5].tolist())


def cut(arrs, rect):
    x, y, w, h = rect
    return [None if a is None else np.ascontiguousarray(a[y:y + h, x:x + w]) for a in arrs]


AMP = (0.05, 0.0, 1e-4, 2.0)  # channel 1 is not perturbed
CASES = [  # X, Y, B, keywords
    (37, 11, 3, dict(mode=0, scale=1)),
    (37, 11, 3, dict(mode=1, scale=3, seed=2024)),
    (37, 11, 3, dict(mode=0, scale=8, seed=5, wrap_x=True)),                      # 37 is no multiple of 8: a last interval of 5 cells
    (130, 40, 2, dict(mode=1, scale=64, seed=0xFFFFFFFF, wrap_x=True)),           # ... of 2 cells
    (37, 11, 3, dict(mode=0, scale=1000, seed=9)),                                # larger than the grid: one lattice cell
    (37, 11, 3, dict(mode=1, scale=1000, seed=9, wrap_x=True)),                   # ... closed on itself: constant in x
    (37, 11, 3, dict(mode=0, scale=3, seed=3, lo=(-0.01, NAN, NAN, 279.0), hi=(0.02, NAN, 0.0, NAN))),
    (37, 11, 17, dict(mode=0, scale=4, seed=77, members=[0, 3, 16])),             # a sparse mask
    (37, 11, 3, dict(mode=1, scale=2, seed=1, rect=(5, 2, 30, 7))),
]


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_PERTURB\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_HAVE_STATE_COPY\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    L = pkg.engine.lib()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in pkg.engine.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert callable(pkg.engine.Ensemble.perturb) and callable(pkg.sim.WeatherEnsemble.perturb) and callable(pkg.engine.ens_perturb_cells)
    assert "ensemble_perturb" in [L.wx_kernel_name(k).decode() for k in range(L.wx_kernel_count())]
    # the ctypes struct is the header's, member for member
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct wx_ens_perturb {"):hdr.index("} wx_ens_perturb;")].split("{", 1)[1], flags=re.S)
    names = [re.sub(r"[\*\s]|\[.*\]", "", n) for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(float|u?int32_t)\b", "", decl.strip()).split(",")]
    assert names == [f[0] for f in pkg.engine.WxEnsPerturb._fields_]
    assert C.sizeof(pkg.engine.WxEnsPerturb) == 9 * 4 + 12 * 4


def test_argument_checks_answer_without_a_device(pkg):
    L, E = pkg.engine.lib(), pkg.engine
    good = E._perturb_struct("BASE_CUR", AMP, "add", 3, 1, False, (0, 0, 8, 4), None, None)
    assert L.wx_ensemble_perturb(None, C.byref(good), None) == E_INVALID
    assert L.wx_ensemble_perturb(None, None, None) == E_INVALID
    f, w = hand_built(2, 8, 4)
    keep = [a.copy() for a in f]
    fp, wp = (C.c_void_p * 2)(*[a.ctypes.data for a in f]), (C.c_void_p * 2)(*[a.ctypes.data for a in w])
    call = lambda p, X=8, Y=4, n=2, fp=fp, wp=wp, mask=None: L.wx_ens_perturb_cells(None if p is None else C.byref(p), X, Y, n, fp, wp, mask)  # noqa: E731

    def variant(**kw):
        p = E._perturb_struct("BASE_CUR", AMP, "add", 3, 1, False, (0, 0, 8, 4), None, None)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert call(None) == E_INVALID
    for kw in (dict(field=8), dict(field=4), dict(field=-1), dict(mode=2), dict(mode=-1), dict(scale=0), dict(scale=-3)):
        assert call(variant(**kw)) == E_INVALID, kw
    for kw in (dict(x=1), dict(y=1), dict(x=-1), dict(y=-1), dict(w=0), dict(h=0), dict(w=9), dict(h=5), dict(x=8, w=1), dict(w=-2)):
        assert call(variant(**kw)) == E_RANGE, kw
    assert call(good, n=0) == E_INVALID and call(good, n=-1) == E_INVALID
    assert call(good, fp=None) == E_INVALID and call(good, wp=None) == E_INVALID
    assert call(good, mask=(C.c_uint8 * 2)(0, 0)) == E_INVALID
    hole = (C.c_void_p * 2)(f[0].ctypes.data, None)
    assert call(good, fp=hole) == E_INVALID
    for a, b in zip(f, keep):
        assert same_bits(a, b)  # a refused call writes nothing
    assert call(good, fp=hole, mask=(C.c_uint8 * 2)(1, 0)) == 0  # ... an unselected member may be absent
    assert not same_bits(f[0], keep[0]) and same_bits(f[1], keep[1])
    with pytest.raises(E.WxError) as ei:
        E.ens_perturb_cells(keep, w, 8, 4, "BASE_CUR", AMP, members=[])
    assert ei.value.code == E_INVALID
    with pytest.raises(E.WxError) as ei:
        E.ens_perturb_cells(cut(keep, (0, 0, 8, 2)), cut(w, (0, 0, 8, 2)), 8, 4, "WATER_CUR", AMP, rect=(0, 3, 8, 2))
    assert ei.value.code == E_RANGE


# (seed, member, channel, gx, gy) -> u, from the definition evaluated by hand (Python integers, no numpy)
KNOWN_NODES = [((0, 0, 0, 0, 0), -1.0), ((1, 0, 0, 0, 0), -0.9511572122573853), ((2024, 3, 1, 5, 7), 0.3997694253921509),
               ((0xFFFFFFFF, 16, 3, 2, 0), -0.17340087890625), ((12345, 69, 2, 1000, 299), 0.8502886295318604),
               ((7, 1, 0, 3, 2), 0.06379449367523193), ((7, 1, 1, 3, 2), 0.026430487632751465), ((7, 2, 0, 3, 2), -0.7734659910202026),
               ((8, 1, 0, 3, 2), -0.3614751100540161)]


@pytest.mark.parametrize("scale", [1, 5])
def test_known_node_values(pkg, scale):
    """v = 0, amplitude 1, mode 0 at a lattice node (tx = ty = 0): the new value is the node's u, a 24-bit fraction -- exact in float32."""
    for (seed, member, c, gx, gy), u in KNOWN_NODES:
        assert float(node(seed, member, c, gx, gy)) == u  # the restatement above agrees with the literal
        X, Y = gx * scale + 2, gy * scale + 2
        f = [None] * member + [np.zeros((1, 1, 4), np.float32)]
        w = [None] * member + [np.ones((1, 1, 4), np.int8)]
        amp = [0.0] * 4
        amp[c] = 1.0
        got = pkg.engine.ens_perturb_cells(f, w, X, Y, "WATER_CUR", amp, scale=scale, seed=seed, rect=(gx * scale, gy * scale, 1, 1), members=[member])
        assert float(got[member][0, 0, c]) == u, (seed, member, c, gx, gy)
        assert np.float32(u) == u and not got[member][0, 0, [k for k in range(4) if k != c]].any()


@pytest.mark.parametrize("X,Y,B,kw", CASES, ids=[str(i) for i in range(len(CASES))])
@pytest.mark.parametrize("field", ["BASE_CUR", "WATER_CUR"])
def test_host_function_equals_the_definition(pkg, field, X, Y, B, kw):
    f, w = hand_built(B, X, Y)
    kw = dict(kw)
    rect = kw.pop("rect", None)
    mode = kw.pop("mode")
    lo, hi = kw.pop("lo", (NAN,) * 4), kw.pop("hi", (NAN,) * 4)
    fin, win = (f, w) if rect is None else (cut(f, rect), cut(w, rect))
    got = pkg.engine.ens_perturb_cells(fin, win, X, Y, field, AMP, mode=("add", "mul")[mode], rect=rect, lo=lo, hi=hi, **kw)
    want = reference(fin, win, X, Y, amplitude=AMP, mode=mode, rect=rect, lo=lo, hi=hi, **kw)
    check(got, want, (field, kw))
    assert_what_a_perturbation_leaves_alone(got, fin, win, kw.get("members"), lo, hi)


def assert_what_a_perturbation_leaves_alone(got, fin, win, members, lo, hi):
    """The value-level assertions on `hand_built` members perturbed with AMP (tests/test_ensemble_perturb_gpu.py applies them to what
    the device holds): ``got`` after, ``fin`` / ``win`` the fields and walls before, over the same cells."""
    B = len(fin)
    for i in range(B):
        sel = members is None or i in members
        changed = got[i].view(np.uint32) != fin[i].view(np.uint32)
        assert changed.any() == sel, i
        # never a wall cell, never channel 1 (amplitude 0), never a non-finite value; and what was finite stays finite
        assert not changed[win[i][..., 1] == 0].any() and not changed[..., 1].any() and not changed[~np.isfinite(fin[i])].any()
        assert np.isfinite(got[i][np.isfinite(fin[i])]).all()
    if not np.isnan(lo[0]):
        ch = got[0][..., 0][(got[0].view(np.uint32) != fin[0].view(np.uint32))[..., 0]]
        assert ch.min() >= np.float32(lo[0]) and ch.max() <= np.float32(hi[0]) and (ch == np.float32(lo[0])).any() and (ch == np.float32(hi[0])).any()


PX, PY = 57, 9
# (field, keywords) of the planted runs: both modes, a lattice of 1 / 3 / 8 cells, wrap_x, both clamps, a rectangle, a sparse mask
PLANTED_RUNS = [("BASE_CUR", dict(mode=0, scale=1)), ("WATER_CUR", dict(mode=1, scale=3, seed=2024)), ("BASE_CUR", dict(mode=0, scale=8, seed=5, wrap_x=True)),
                ("WATER_CUR", dict(mode=0, scale=3, seed=3, lo=(-0.01, NAN, NAN, 279.0), hi=(0.02, NAN, 0.0, NAN))),
                ("BASE_CUR", dict(mode=1, scale=2, seed=1, rect=(5, 2, 30, 7))), ("WATER_CUR", dict(mode=0, scale=4, seed=77, members=[0, 2]))]


def planted_run(pkg, B, field, kw, perturb):
    """One planted run: `hand_built` members (NaN, +-Inf, -0.0, subnormals, +-FLT_MAX -- whose product with 1 + a r overflows and is
    refused -- sprinkled over ordinary values, walls that differ per member), ``perturb(fields, walls, field, keywords) -> fields
    after``, the host function's bits, and the CPU test's value-level assertions on the result."""
    f, w = hand_built(B, PX, PY)
    kw = dict(kw)
    rect, mode = kw.pop("rect", None), ("add", "mul")[kw.pop("mode")]
    lo, hi = kw.pop("lo", (NAN,) * 4), kw.pop("hi", (NAN,) * 4)
    if B == 17 and "members" in kw:
        kw["members"] = [0, 3, 16]
    cut = (lambda arrs: arrs) if rect is None else (lambda arrs: [np.ascontiguousarray(a[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]) for a in arrs])
    call = dict(mode=mode, rect=rect, lo=lo, hi=hi, **kw)
    got = cut(perturb(f, w, field, call))
    want = pkg.engine.ens_perturb_cells(cut(f), cut(w), PX, PY, field, AMP, **call)
    for i in range(B):
        assert same_bits(got[i], want[i]), (field, call, "member", i, np.argwhere(got[i].view(np.uint32) != want[i].view(np.uint32))[:4].tolist())
    assert_what_a_perturbation_leaves_alone(got, cut(f), cut(w), kw.get("members"), lo, hi)
    specials = [np.isin(a.view(np.uint32), SPECIALS.view(np.uint32)) for a in cut(f)]
    assert all(s.any() for s in specials) and any((g.view(np.uint32) != a.view(np.uint32))[s].any() for g, a, s in zip(got, cut(f), specials))  # the finite ones move


@pytest.mark.parametrize("B", [3, 17])
def test_planted_special_values_through_the_host_function(pkg, B):
    """(tests/test_ensemble_perturb_gpu.py runs the same through the kernel.)"""
    for field, kw in PLANTED_RUNS:
        planted_run(pkg, B, field, kw, lambda f, w, field, call: _pasted(pkg, f, w, field, call))


def _pasted(pkg, f, w, field, call):
    """The host function on the rectangle's cells, pasted back into whole grids."""
    rect = call["rect"]
    if rect is None:
        return pkg.engine.ens_perturb_cells(f, w, PX, PY, field, AMP, **call)
    x, y, rw, rh = rect
    new = pkg.engine.ens_perturb_cells(cut(f, rect), cut(w, rect), PX, PY, field, AMP, **call)
    out = [a.copy() for a in f]
    for o, n in zip(out, new):
        o[y:y + rh, x:x + rw] = n
    return out


def test_an_overflowing_result_is_refused_not_stored(pkg):
    f = [np.full((1, 4, 4), FLT_MAX, np.float32)]
    w = [np.ones((1, 4, 4), np.int8)]
    got = pkg.engine.ens_perturb_cells(f, w, 4, 1, "BASE_CUR", 1.0, mode="mul", seed=3)
    r = np.stack([noise(4, np.arange(4)[None], np.zeros((1, 4), np.int64), 0, c, scale=1, seed=3, wrap_x=False) for c in range(4)], -1)
    assert (r > 0).any() and (r < 0).any()
    assert (got[0][r > 0] == FLT_MAX).all() and (got[0][r < 0] < FLT_MAX).all() and np.isfinite(got[0]).all()
    check(got, reference(f, w, 4, 1, amplitude=(1.0,) * 4, mode=1, seed=3), "overflow")
    # ... clamped to +Inf is refused too, a NaN amplitude touches nothing
    assert same_bits(pkg.engine.ens_perturb_cells(f, w, 4, 1, "BASE_CUR", 0.5, lo=np.inf)[0], f[0])
    assert same_bits(pkg.engine.ens_perturb_cells(f, w, 4, 1, "BASE_CUR", NAN)[0], f[0])


def test_zero_amplitude_leaves_bits_alone(pkg):
    f, w = hand_built(3, 37, 11)
    for mode in ("add", "mul"):
        got = pkg.engine.ens_perturb_cells(f, w, 37, 11, "BASE_CUR", (0.0, -0.0, 0.0, 0.0), mode=mode, scale=3, lo=(0.0,) * 4, hi=(0.0,) * 4)
        check(got, f, mode)


def test_disjoint_rectangles_compose_to_their_union(pkg):
    X, Y = 37, 11
    f, w = hand_built(3, X, Y)
    kw = dict(mode="mul", scale=4, seed=21, wrap_x=True)
    whole = pkg.engine.ens_perturb_cells(f, w, X, Y, "WATER_CUR", AMP, **kw)
    parts = [a.copy() for a in f]
    for rect in ((0, 0, 20, Y), (20, 0, 17, 5), (20, 5, 17, 6)):
        x, y, ww, h = rect
        sub = pkg.engine.ens_perturb_cells(cut(parts, rect), cut(w, rect), X, Y, "WATER_CUR", AMP, rect=rect, **kw)
        for a, s in zip(parts, sub):
            a[y:y + h, x:x + ww] = s
    check(parts, whole, "three rectangles")


def test_a_members_noise_does_not_depend_on_the_mask(pkg):
    X, Y = 37, 11
    f, w = hand_built(5, X, Y)
    kw = dict(scale=3, seed=8)
    everybody = pkg.engine.ens_perturb_cells(f, w, X, Y, "BASE_CUR", AMP, **kw)
    some = pkg.engine.ens_perturb_cells(f, w, X, Y, "BASE_CUR", AMP, members=[1, 4], **kw)
    alone = pkg.engine.ens_perturb_cells([None, None, None, None, f[4]], [None, None, None, None, w[4]], X, Y, "BASE_CUR", AMP, members=[4], **kw)
    assert same_bits(some[1], everybody[1]) and same_bits(some[4], everybody[4]) and same_bits(alone[4], everybody[4])
    assert same_bits(some[0], f[0]) and same_bits(some[2], f[2]) and same_bits(some[3], f[3])
    zeros, air = [np.zeros((Y, X, 4), np.float32)] * 2, [np.ones((Y, X, 4), np.int8)] * 2
    z = pkg.engine.ens_perturb_cells(zeros, air, X, Y, "BASE_CUR", AMP, **kw)
    assert not same_bits(z[0], z[1]) and not same_bits(z[0][..., 0], z[0][..., 2] * np.float32(AMP[0] / AMP[2]))  # members and channels differ: both are in the hash
    # the index, not the position in the selection: member 4 selected second is not "member 1"
    as_one = pkg.engine.ens_perturb_cells([None, f[4]], [None, w[4]], X, Y, "BASE_CUR", AMP, members=[1], **kw)
    assert not same_bits(as_one[1], everybody[4])


def test_wrap_x_has_no_seam(pkg):
    """With wrap_x, x = X - 1 and x = 0 are neighbours on one lattice edge: the step across the seam is one cell's slope, |u_right -
    u_left| / len <= 2 / len per row, like every other step inside that interval -- without wrap_x it is a jump between unrelated nodes."""
    X, Y, scale = 37, 64, 8
    ys, c = np.arange(Y, dtype=np.int64), 0
    for member in range(4):
        r_last = noise(X, np.full(Y, X - 1, np.int64), ys, member, c, scale=scale, seed=5, wrap_x=True)
        r_zero = noise(X, np.zeros(Y, np.int64), ys, member, c, scale=scale, seed=5, wrap_x=True)
        length = X - ((X - 1) // scale) * scale
        # along a row, r is linear inside the last interval and reaches node 0's value at x = X: the seam step IS the interval's slope
        r_prev = noise(X, np.full(Y, X - 2, np.int64), ys, member, c, scale=scale, seed=5, wrap_x=True)
        assert length == 5 and np.allclose(r_zero - r_last, r_last - r_prev, rtol=0, atol=1e-12)
        assert np.abs(r_zero - r_last).max() <= 2.0 / length
    # the host function shows the same: periodic in x with period X
    f, w = [np.zeros((Y, X, 4), np.float32)], [np.ones((Y, X, 4), np.int8)]
    got = pkg.engine.ens_perturb_cells(f, w, X, Y, "BASE_CUR", (1.0, 0, 0, 0), scale=scale, seed=5, wrap_x=True)[0][..., 0].astype(np.float64)
    assert np.abs(got[:, 0] - got[:, X - 1]).max() <= 2.0 / 5 + 1e-6
    assert np.allclose(got[:, 0] - got[:, X - 1], got[:, X - 1] - got[:, X - 2], rtol=0, atol=1e-6)
    open_ = pkg.engine.ens_perturb_cells(f, w, X, Y, "BASE_CUR", (1.0, 0, 0, 0), scale=scale, seed=5, wrap_x=False)[0][..., 0].astype(np.float64)
    assert same_bits(open_[:, :32], got[:, :32]) and not same_bits(open_[:, 32:], got[:, 32:])
    assert not np.allclose(open_[:, 0] - open_[:, X - 1], open_[:, X - 1] - open_[:, X - 2], rtol=0, atol=1e-3)


_FAST_LEG = """
import ctypes as C, sys, numpy as np
lib, src, dst = sys.argv[1:4]
L = C.CDLL(lib)
d = np.load(src)
f, w, desc = np.ascontiguousarray(d["f"]), np.ascontiguousarray(d["w"]), d["desc"].tobytes()
B, Y, X = f.shape[:3]
p = C.create_string_buffer(desc, len(desc))
fp, wp = (C.c_void_p * B)(*[f[i].ctypes.data for i in range(B)]), (C.c_void_p * B)(*[w[i].ctypes.data for i in range(B)])
L.wx_ens_perturb_cells.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
assert L.wx_arith() == 1, "not the tolerance build"
assert L.wx_ens_perturb_cells(p, X, Y, B, fp, wp, None) == 0
np.save(dst, f)
"""


def test_the_tolerance_build_gives_the_same_bits(pkg, tmp_path):
    """libwxsim_fast.so (contraction allowed everywhere else): the per-cell function switches contraction off for itself. In a process of
    its own: a process holds one libwxsim."""
    fast = pkg.engine.FAST_LIB_PATH
    if not os.path.exists(fast):
        pytest.skip("libwxsim_fast.so is not built")
    X, Y, B = 37, 11, 3
    f, w = hand_built(B, X, Y)
    for k, (mode, scale, wrap) in enumerate(((0, 3, False), (1, 8, True))):
        desc = pkg.engine._perturb_struct("BASE_CUR", AMP, mode, scale, 99, wrap, (0, 0, X, Y), (-0.5, NAN, NAN, NAN), None)
        src, dst = str(tmp_path / f"in{k}.npz"), str(tmp_path / f"out{k}.npy")
        np.savez(src, f=np.stack(f), w=np.stack(w), desc=np.frombuffer(bytes(desc), np.uint8))
        subprocess.check_call([sys.executable, "-c", _FAST_LEG, fast, src, dst], timeout=120)
        got = list(np.load(dst))
        want = reference(f, w, X, Y, amplitude=AMP, mode=mode, scale=scale, seed=99, wrap_x=wrap, lo=(-0.5, NAN, NAN, NAN))
        check(got, want, ("fast vs definition", k))
        check(got, pkg.engine.ens_perturb_cells(f, w, X, Y, "BASE_CUR", AMP, mode=mode, scale=scale, seed=99, wrap_x=wrap, lo=(-0.5, NAN, NAN, NAN)), ("fast vs exact", k))


def test_host_function_under_the_sanitizers(tmp_path):
    """tests/native/ens_perturb_main.cpp -- the per-cell header and a main() that runs wxp::perturb_cells over randomised buffers that
    end exactly at the last cell -- compiled stand-alone with AddressSanitizer and UBSan (host compiler, no device, no library) and run."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.call(["which", c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ens_perturb_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "ens_perturb_main.cpp")], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ens_perturb_main ok" in out.stdout
