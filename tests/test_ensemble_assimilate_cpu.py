"""Ensemble assimilation (wx_ensemble_assimilate, wx_ens_assim_cells; include/wxsim.h) without a GPU: the header announces and declares
the addition at the unchanged ABI version, the library exports it, the argument checks answer before any device is touched, and the pure
host entry point -- the serial definition built from the kernels' own functions -- equals the definition in the header comment, which
`reference` below restates in plain Python: Python floats are doubles, ONE Python operation per rounded operation, math.sqrt, and
numpy only for the double -> float32 conversion. Every comparison of states is `==` on bits, NaNs compared as positions."""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_ensemble_statistics_cpu import FLT_MAX, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_assimilate", "wx_ens_assim_cells"]
E_INVALID, E_RANGE = -1, -4
NAN, INF = float("nan"), float("inf")
B_, W_ = "BASE_CUR", "WATER_CUR"


def f32(v):
    return float(np.float32(v))


def gc(z):
    """G of the header, by Horner, one rounding per operation."""
    if z >= 2.0:
        return 0.0
    if z <= 1.0:
        p = -0.25 * z + 0.5
        p = p * z + 0.625
        p = p * z - 5.0 / 3.0
        p = p * z
        p = p * z + 1.0
    else:
        p = (1.0 / 12.0) * z - 0.5
        p = p * z + 0.625
        p = p * z + 5.0 / 3.0
        p = p * z - 5.0
        p = p * z + 4.0
        p = p - (2.0 / 3.0) / z
    return 0.0 if p < 0.0 else p


def axis_weight(d, loc):
    return 1.0 if loc == 0.0 else gc(float(d) / loc)


def four(v, fill):
    if v is None:
        return [fill] * 4
    a = np.asarray(v, np.float64).ravel()
    return [f32(a[0])] * 4 if a.size == 1 else [f32(x) for x in a]


def reference(bases, waters, walls, X, Y, observations, *, loc=(0.0, 0.0), rect=None, members=None, wrap_x=False, gain_base=(0, 0, 0, 1),
              gain_water=0.0, lo_base=None, hi_base=None, lo_water=None, hi_water=None):
    """The definition of include/wxsim.h, straight from its text. Returns (bases, waters, results) like engine.ens_assim_cells."""
    sel = list(range(len(bases))) if members is None else sorted(int(i) for i in members)
    n = len(sel)
    nb = [None if a is None else np.array(a, np.float32) for a in bases]
    nw = [None if a is None else np.array(a, np.float32) for a in waters]
    rx, ry, rw, rh = (0, 0, X, Y) if rect is None else rect
    lx, ly = f32(loc[0]), f32(loc[1])
    state = ((nb, four(gain_base, 0.0), four(lo_base, NAN), four(hi_base, NAN)), (nw, four(gain_water, 0.0), four(lo_water, NAN), four(hi_water, NAN)))
    results = []
    for field, ox, oy, ch, value, R in observations:
        F = nb if field in (B_, 0) else nw
        t32 = [F[k][oy, ox, ch] for k in sel]
        if not all(walls[k][oy, ox, 1] != 0 for k in sel) or not all(np.isfinite(v) for v in t32):
            results.append({"applied": False, "prior_mean": NAN, "prior_var": NAN, "innovation": NAN, "alpha": NAN})
            continue
        t = [float(v) for v in t32]
        S = 0.0
        for v in t:
            S = S + v
        hm = S / n
        e = [v - hm for v in t]
        Q = 0.0
        for ek in e:
            Q = Q + ek * ek
        V = Q / (n - 1)
        R = f32(R)
        D = V + R
        innovation = f32(value) - hm
        alpha = 1.0 / (1.0 + math.sqrt(R / D))
        results.append({"applied": True, "prior_mean": hm, "prior_var": V, "innovation": innovation, "alpha": alpha})
        for y in range(ry, ry + rh):
            for x in range(rx, rx + rw):
                dx = abs(x - ox)
                if wrap_x:
                    dx = min(dx, X - dx)
                rho = axis_weight(dx, lx) * axis_weight(abs(y - oy), ly)
                if rho == 0.0 or not all(walls[k][y, x, 1] != 0 for k in sel):
                    continue
                for Fs, gain, lo, hi in state:
                    for c in range(4):
                        g = gain[c]
                        xs32 = [Fs[k][y, x, c] for k in sel]
                        if g == 0.0 or not all(np.isfinite(v) for v in xs32):
                            continue
                        xs = [float(v) for v in xs32]
                        Sx = 0.0
                        for v in xs:
                            Sx = Sx + v
                        xm = Sx / n
                        Cq = 0.0
                        for v, ek in zip(xs, e):
                            Cq = Cq + (v - xm) * ek
                        Cv = Cq / (n - 1)
                        w = g * rho
                        K = (w * Cv) / D
                        if K == 0.0 or not math.isfinite(K):
                            continue
                        a = K * innovation
                        b = alpha * K
                        for k, v, ek in zip(sel, xs, e):
                            with np.errstate(over="ignore", invalid="ignore"):
                                o = np.float32(v + (a - b * ek))
                            if lo[c] == lo[c] and o < lo[c]:
                                o = np.float32(lo[c])
                            if hi[c] == hi[c] and o > hi[c]:
                                o = np.float32(hi[c])
                            if np.isfinite(o):
                                Fs[k][y, x, c] = o
    return nb, nw, results


def members_of(B, X, Y, seed=7, walls=0.04):
    """B members of an X x Y grid: smooth fields plus member noise (so that covariances between cells are not all zero), different
    sparse walls per member over a common floor row."""
    rng = np.random.Generator(np.random.Philox(seed + 1000 * B))
    yy, xx = np.mgrid[0:Y, 0:X]
    bases, waters, wl = [], [], []
    for i in range(B):
        ph = rng.uniform(0, 6.28)
        sm = np.sin(xx / 3.0 + ph)[..., None] * np.cos(yy / 2.0 + ph)[..., None]
        b = (np.array([0.1, 0.05, 0.01, 300.0]) + sm * np.array([0.3, 0.2, 0.02, 2.5]) + rng.normal(0, 1, (Y, X, 4)) * np.array([0.05, 0.05, 0.005, 0.4])).astype(np.float32)
        w = np.abs(np.array([0.012, 0.001, 0.0, 0.3]) + sm * np.array([0.004, 0.001, 0.0, 0.2]) + rng.normal(0, 1, (Y, X, 4)) * np.array([0.001, 0.0005, 0.0, 0.05])).astype(np.float32)
        m = np.zeros((Y, X, 4), np.int8)
        m[..., 1] = np.where(rng.random((Y, X)) < walls, 0, rng.integers(1, 100, (Y, X)))
        m[0, :, 1] = 0
        m[..., 0] = rng.integers(0, 3, (Y, X))
        bases.append(b), waters.append(w), wl.append(m)
    return bases, waters, wl


def clear(wl, cells):
    for m in wl:
        for x, y in cells:
            m[y, x, 1] = 5


def check(pkg, bases, waters, wl, X, Y, obs, where, **kw):
    """engine.ens_assim_cells == reference, bit for bit, results included; returns the host function's answer."""
    gb, gw, gr = pkg.engine.ens_assim_cells(bases, waters, wl, X, Y, obs, **kw)
    rb, rw, rr = reference(bases, waters, wl, X, Y, obs, **kw)
    for i, (a, b, c, d) in enumerate(zip(gb, rb, gw, rw)):
        if a is None:
            assert b is None and c is None and d is None
            continue
        assert same_bits(a, b), (where, "base", i, np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:5].tolist())
        assert same_bits(c, d), (where, "water", i, np.argwhere(c.view(np.uint32) != d.view(np.uint32))[:5].tolist())
    assert len(gr) == len(rr) == len(obs)
    for j, (a, b) in enumerate(zip(gr, rr)):
        assert a["applied"] == b["applied"], (where, j)
        for k in ("prior_mean", "prior_var", "innovation", "alpha"):
            assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) or (a[k] != a[k] and b[k] != b[k]), (where, j, k, a[k], b[k])
    return gb, gw, gr


def changed(a, b):
    return np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_ASSIMILATE\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ENS_OBS_MAX\s+256\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    L, E = pkg.engine.lib(), pkg.engine
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in E.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert callable(E.Ensemble.assimilate) and callable(pkg.sim.WeatherEnsemble.assimilate) and callable(E.ens_assim_cells)
    names = [L.wx_kernel_name(k).decode() for k in range(L.wx_kernel_count())]
    assert names[-2:] == ["ensemble_assimilate_obs", "ensemble_assimilate"]
    # the ctypes structs are the header's, member for member
    for tag, cls, size in (("wx_ens_obs", E.WxEnsObs, 24), ("wx_ens_obs_result", E.WxEnsObsResult, 40), ("wx_ens_assim", E.WxEnsAssim, 7 * 4 + 24 * 4)):
        body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct %s {" % tag):hdr.index("} %s;" % tag)].split("{", 1)[1], flags=re.S)
        got = [re.sub(r"[\*\s]|\[.*\]", "", n) for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(float|double|u?int32_t)\b", "", decl.strip()).split(",")]
        assert got == [f[0] for f in cls._fields_], tag
        assert C.sizeof(cls) == size, tag
    assert E.ENS_OBS_MAX == 256


def test_every_refusal_with_its_code(pkg):
    L, E = pkg.engine.lib(), pkg.engine
    X, Y, B = 8, 4, 3
    bases, waters, wl = members_of(B, X, Y)
    keep = [a.copy() for a in bases + waters]
    ptrs = lambda arrs: (C.c_void_p * B)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    bp, wp, mp = ptrs(bases), ptrs(waters), ptrs(wl)
    good_obs = [(B_, 3, 2, 3, 300.0, 0.25), (W_, 1, 1, 0, 0.01, 1e-6)]

    def call(a=None, obs=good_obs, n_obs=None, X=X, Y=Y, n=B, bp=bp, wp=wp, mp=mp, mask=None, desc=True, have_obs=True, **kw):
        a = E._assim_struct((0, 0, 8, 4), (2.0, 1.0), False, (0, 0, 0, 1), 0.5, None, None, None, None) if a is None else a
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        o = E._obs_array(obs)
        res = (E.WxEnsObsResult * max(len(obs), 1))()
        return L.wx_ens_assim_cells(C.byref(a) if desc else None, len(obs) if n_obs is None else n_obs, o if have_obs else None, res, X, Y, n, bp, wp, mp, mask)

    assert call() == 0
    for a, b in zip(bases + waters, keep):  # (the good call changed something: the refusals below are not vacuous)
        a[...] = b
    # WX_E_INVALID
    assert L.wx_ensemble_assimilate(None, None, 1, None, None, None) == E_INVALID
    a0, o0 = E._assim_struct((0, 0, 8, 4), (0, 0), False, 1.0, 0.0, None, None, None, None), E._obs_array(good_obs)
    assert L.wx_ensemble_assimilate(None, C.byref(a0), 2, o0, None, None) == E_INVALID  # e NULL
    assert call(desc=False) == E_INVALID and call(have_obs=False) == E_INVALID
    assert call(n_obs=0) == E_INVALID and call(n_obs=-1) == E_INVALID
    assert call(obs=[good_obs[0]] * 257) == E_INVALID and call(obs=[good_obs[0]] * 256) == 0
    for a, b in zip(bases + waters, keep):
        a[...] = b
    for bad in ((1, 3, 2, 3, 300.0, 0.25), (4, 3, 2, 3, 300.0, 0.25), (-1, 3, 2, 3, 300.0, 0.25),  # field
                (B_, 3, 2, 4, 300.0, 0.25), (B_, 3, 2, -1, 300.0, 0.25),  # channel
                (B_, 3, 2, 3, NAN, 0.25), (B_, 3, 2, 3, INF, 0.25), (B_, 3, 2, 3, 300.0, NAN), (B_, 3, 2, 3, 300.0, INF),  # not finite
                (B_, 3, 2, 3, 300.0, 0.0), (B_, 3, 2, 3, 300.0, -1.0)):  # R <= 0
        assert call(obs=[good_obs[1], bad]) == E_INVALID, bad
    for kw in (dict(loc_x=NAN), dict(loc_y=INF), dict(loc_x=-1.0), dict(loc_y=-0.5), dict(gain_base=(2, NAN)), dict(gain_water=(0, INF)), dict(gain_water=(3, -INF))):
        assert call(**kw) == E_INVALID, kw
    assert call(mask=(C.c_uint8 * B)(0, 1, 0)) == E_INVALID and call(mask=(C.c_uint8 * B)(0, 0, 0)) == E_INVALID  # fewer than two members
    assert call(n=1) == E_INVALID and call(n=0) == E_INVALID
    assert call(bp=None) == E_INVALID and call(wp=None) == E_INVALID and call(mp=None) == E_INVALID
    assert call(bp=ptrs([bases[0], None, bases[2]])) == E_INVALID
    # WX_E_RANGE: the rectangle, an observation
    for kw in (dict(x=1), dict(y=1), dict(x=-1), dict(y=-1), dict(w=0), dict(h=0), dict(w=9), dict(h=5), dict(x=8, w=1), dict(w=-2)):
        assert call(**kw) == E_RANGE, kw
    for bad in ((B_, 8, 2, 3, 300.0, 0.25), (B_, -1, 2, 3, 300.0, 0.25), (W_, 3, 4, 0, 0.1, 0.25), (W_, 3, -1, 0, 0.1, 0.25)):
        assert call(obs=[good_obs[0], bad]) == E_RANGE, bad
    for a, b in zip(bases + waters, keep):
        assert same_bits(a, b)  # a refused call writes nothing
    assert call(bp=ptrs([bases[0], None, bases[2]]), mask=(C.c_uint8 * B)(1, 0, 1)) == 0  # an unselected member may be absent
    assert not same_bits(bases[0], keep[0]) and same_bits(bases[1], keep[1])
    with pytest.raises(E.WxError) as ei:
        E.ens_assim_cells(keep[:B], keep[B:], wl, X, Y, good_obs, members=[1])
    assert ei.value.code == E_INVALID
    with pytest.raises(E.WxError) as ei:
        E.ens_assim_cells(keep[:B], keep[B:], wl, X, Y, good_obs, rect=(0, 3, 8, 2))
    assert ei.value.code == E_RANGE


@pytest.mark.parametrize("B,members", [(2, None), (3, [0, 2]), (8, None), (17, None), (6, [5, 1, 3, 4])])
def test_host_function_equals_the_definition_on_random_members(pkg, B, members):
    X, Y = 23, 9
    bases, waters, wl = members_of(B, X, Y)
    rng = np.random.Generator(np.random.Philox(B))
    obs = []
    for j in range(7):
        x, y = int(rng.integers(0, X)), int(rng.integers(1, Y))
        obs.append((B_, x, y, 3, 300.0 + rng.normal(), 0.25) if j % 3 != 1 else (W_, x, y, 0, 0.012 + 0.002 * rng.normal(), 1e-6))
    obs.append((B_, obs[0][1], obs[0][2], 0, 0.3, 0.01))  # vx at the first observation's cell
    for kw in (dict(loc=(5.0, 2.5), gain_base=(0.5, 0, 0, 1), gain_water=(1, 0.25, 0, 0), wrap_x=True),
               dict(loc=(0.0, 3.0), rect=(2, 1, 19, 7), gain_base=1.0, gain_water=1.0, lo_water=0.0),
               dict(loc=(3.5, 0.0), rect=(20, 0, 3, 9), gain_water=(0, 0, 0, 1), hi_base=(NAN, NAN, NAN, 300.5))):
        _, _, res = check(pkg, bases, waters, wl, X, Y, obs, (B, members, kw), members=members, **kw)
        assert any(r["applied"] for r in res)


def planted(B=5, X=17, Y=7):
    bases, waters, wl = members_of(B, X, Y, seed=11, walls=0.0)
    return bases, waters, wl, X, Y


# THE PLANTED CASES. Each is a function of `run` -- run(bases, waters, walls, X, Y, observations, where, **keywords) -> (bases, waters,
# results) after the call -- that builds its arrays, hands them to `run` and applies the value-level assertions to what comes back.
# Here `run` is `check` (the host function, held to `reference`); tests/test_ensemble_assimilate_gpu.py hands in the device call on
# the same arrays. B = 5 members walk the kernels' remainder loop alone, B = 9 a load group of 8 and one member behind it.
def planted_skipped(run, B=5):
    bases, waters, wl, X, Y = planted(B)
    wl[2][3, 4, 1] = 0  # the observed cell is a wall in one member
    bases[1][2, 9, 3] = NAN
    bases[B - 1][4, 12, 3] = -INF
    obs = [(B_, 4, 3, 3, 301.0, 0.1), (B_, 9, 2, 3, 301.0, 0.1), (B_, 12, 4, 3, 301.0, 0.1)]
    gb, gw, res = run(bases, waters, wl, X, Y, obs, "skipped", gain_base=1.0, gain_water=1.0, loc=(4.0, 3.0))
    assert [r["applied"] for r in res] == [False] * 3 and all(r[k] != r[k] for r in res for k in ("prior_mean", "prior_var", "innovation", "alpha"))
    assert all(same_bits(a, b) for a, b in zip(gb + gw, bases + waters))


def planted_state_nan(run, B=5, member=3):
    bases, waters, wl, X, Y = planted(B)
    bases[member][3, 6, 0] = NAN
    obs = [(B_, 5, 3, 3, 301.5, 0.1)]
    gb, _, res = run(bases, waters, wl, X, Y, obs, "state nan", gain_base=1.0, loc=(4.0, 3.0))
    assert res[0]["applied"]
    ch = np.stack([changed(a, b) for a, b in zip(gb, bases)])  # (member, y, x, c)
    assert not ch[:, 3, 6, 0].any() and ch[:, 3, 6, 1:].all()


def planted_state_wall(run, B=5, member=3):
    """A state cell that is a wall in ONE member is left alone in all of them, in every channel (the entry test of the member walk)."""
    bases, waters, wl, X, Y = planted(B)
    wl[member][3, 6, 1] = 0
    obs = [(B_, 5, 3, 3, 301.5, 0.1)]
    gb, gw, res = run(bases, waters, wl, X, Y, obs, "state wall", gain_base=1.0, gain_water=1.0, loc=(4.0, 3.0))
    assert res[0]["applied"]
    ch = np.stack([changed(a, b) for a, b in zip(gb + gw, bases + waters)])
    assert not ch[:, 3, 6].any() and ch[:, 3, 7, 3].all() and not ch[:, 0].any()  # (row 0 is the floor: a wall in every member)


def planted_equal_members(run, B=5):
    bases, waters, wl, X, Y = planted(B)
    for b in bases:
        b[...] = bases[0]
        b[2, 3:9, 0] = -0.0
    obs = [(B_, 5, 3, 3, 305.0, 0.1)]
    gb, _, res = run(bases, waters, wl, X, Y, obs, "V = 0", gain_base=1.0)
    assert res[0]["applied"] and res[0]["prior_var"] == 0.0 and res[0]["alpha"] == 0.5
    assert all(same_bits(a, b) for a, b in zip(gb, bases))
    # members that differ in temperature only: C = 0 for vx, whose -0.0 keep their sign bit, while the temperature moves
    for i, b in enumerate(bases):
        b[..., 3] += np.float32(0.25 * i)
    gb, _, _ = run(bases, waters, wl, X, Y, obs, "C = 0", gain_base=1.0)
    assert all(same_bits(a[..., :3], b[..., :3]) for a, b in zip(gb, bases)) and all(np.signbit(a[2, 3:9, 0]).all() for a in gb)
    assert all(changed(a, b)[..., 3].any() for a, b in zip(gb, bases))


def planted_gain_zero_clamp_and_overflow(run, B=5):
    bases, waters, wl, X, Y = planted(B)
    obs = [(B_, 5, 3, 3, 303.0, 0.01)]
    gb, gw, _ = run(bases, waters, wl, X, Y, obs, "gain 0", gain_base=(1, 0, 1, 1), gain_water=(0, 1, 0, 1))
    for a, b in zip(gb, bases):
        assert not changed(a, b)[..., 1].any() and changed(a, b)[..., 3].any()
    for a, b in zip(gw, waters):
        assert not changed(a, b)[..., 0].any() and not changed(a, b)[..., 2].any() and changed(a, b)[..., 3].any()
    free, _, _ = run(bases, waters, wl, X, Y, obs, "no clamp", gain_base=1.0)
    gb, _, _ = run(bases, waters, wl, X, Y, obs, "clamp", gain_base=1.0, hi_base=(NAN, NAN, NAN, 300.75), lo_base=(0.05, NAN, NAN, NAN))
    # the clamp bites: where the unclamped update leaves the interval, the clamped one sits on its edge (untouched cells -- the floor --
    # are not clamped)
    hit_hi = hit_lo = 0
    for f, a, b in zip(free, gb, bases):
        ch = changed(a, b)
        assert (a[..., 3][ch[..., 3]] <= np.float32(300.75)).all() and (a[..., 0][ch[..., 0]] >= np.float32(0.05)).all()
        over, under = ch[..., 3] & (f[..., 3] > 300.75), ch[..., 0] & (f[..., 0] < 0.05)
        assert (a[..., 3][over] == np.float32(300.75)).all() and (a[..., 0][under] == np.float32(0.05)).all()
        hit_hi, hit_lo = hit_hi + int(over.sum()), hit_lo + int(under.sum())
    assert hit_hi > 0 and hit_lo > 0
    # a result that overflows float: the increment at the observed cell would carry member 0 beyond FLT_MAX, so it keeps its bits
    for i, b in enumerate(bases):  # (i % 5: members 5 .. repeat the factors of 0 .., so that every one stays a float)
        b[3, 5, 3] = FLT_MAX * np.float32(0.5 + 0.1 * (i % 5))
    obs = [(B_, 5, 3, 3, -float(FLT_MAX), 1e30)]
    gb, _, res = run(bases, waters, wl, X, Y, obs, "overflow", gain_base=(0, 0, 0, 1), gain_water=0.0, loc=(1.0, 1.0))
    assert res[0]["applied"]
    big = [(B_, 5, 3, 3, float(FLT_MAX), 1e-30)]
    for i, b in enumerate(bases):
        b[3, 5, 3] = -FLT_MAX * np.float32(0.5 + 0.1 * (i % 5))
        b[3, 6, 3] = FLT_MAX * np.float32(0.99 - 0.2 * (i % 5))  # correlated negatively and large: K * innovation leaves the float range
    gb, _, res = run(bases, waters, wl, X, Y, big, "overflow 2", gain_base=(0, 0, 0, 8), gain_water=0.0, loc=(1.5, 1.0))
    kept = [not changed(a, b)[3, 6, 3] for a, b in zip(gb, bases)]
    assert res[0]["applied"] and any(kept), kept


def planted_localization_edges_and_wrap(run, B=5):
    bases, waters, wl, X, Y = planted(B)
    obs = [(B_, 8, 3, 3, 302.0, 0.05)]
    for loc in ((0.0, 0.0), (3.0, 0.0), (0.0, 1.0), (3.0, 1.0)):
        gb, _, _ = run(bases, waters, wl, X, Y, obs, ("loc", loc), gain_base=1.0, loc=loc)
        ch = np.stack([changed(a, b)[..., 3] for a, b in zip(gb, bases)]).any(axis=0)
        ys, xs = np.nonzero(ch)
        # dx == loc is inside (G(1) = 5/24 > 0), dx == 2 loc is the first cell outside (G(2) = 0); row 0 is the floor
        assert (xs.min(), xs.max()) == ((3, 13) if loc[0] else (0, X - 1)), loc
        assert (ys.min(), ys.max()) == ((2, 4) if loc[1] else (1, Y - 1)), loc
        assert ch[3, 5] and ch[3, 11] and (not loc[0] or (not ch[3, 2] and not ch[3, 14]))
        if loc[1]:
            assert ch[2, 8] and ch[4, 8] and not ch[5, 8] and not ch[1, 8]
    assert abs(gc(1.0) - 5.0 / 24.0) < 1e-15
    assert gc(2.0) == 0.0 and gc(0.0) == 1.0
    # an observation at x = 0 reaches x = X - 1 with wrap_x, and not without
    obs = [(B_, 0, 3, 3, 302.0, 0.05)]
    for wrap in (True, False):
        gb, _, _ = run(bases, waters, wl, X, Y, obs, ("wrap", wrap), gain_base=1.0, loc=(2.0, 1.0), wrap_x=wrap)
        ch = np.stack([changed(a, b)[..., 3] for a, b in zip(gb, bases)]).any(axis=0)
        assert ch[3, 0] and ch[3, 3] and not ch[3, 4]
        assert ch[3, X - 1] == wrap and ch[3, X - 3] == wrap and not ch[3, X - 4]


def planted_observation_outside_the_rectangle_duplicates_and_overlap(run, B=5):
    bases, waters, wl, X, Y = planted(B)
    rect = (6, 1, 8, 5)
    obs = [(B_, 3, 3, 3, 302.0, 0.05),   # outside the rectangle, its footprint reaches in
           (B_, 8, 3, 3, 301.0, 0.05), (B_, 8, 3, 3, 300.0, 0.05),  # twice the same cell and channel
           (W_, 10, 4, 0, 0.011, 1e-7), (B_, 11, 3, 3, 299.5, 0.1)]  # overlapping footprints, two fields
    gb, gw, res = run(bases, waters, wl, X, Y, obs, "outside, duplicates, overlap", gain_base=1.0, gain_water=1.0, loc=(4.0, 2.0), rect=rect)
    assert all(r["applied"] for r in res)
    inside = np.zeros((Y, X), bool)
    inside[1:6, 6:14] = True
    for a, b in zip(gb + gw, bases + waters):
        assert not changed(a, b)[~inside].any() and changed(a, b)[inside].any()
    assert res[2]["prior_var"] < res[1]["prior_var"]  # the second of the pair sees what the first left
    assert res[2]["prior_mean"] != res[1]["prior_mean"]


# (case, the keywords that place the planted NaN / wall: inside the load group of 8 and in the remainder member behind it)
PLANTED = [(planted_skipped, [{}]), (planted_state_nan, [dict(member=3), dict(member=-1)]), (planted_state_wall, [dict(member=3), dict(member=-1)]),
           (planted_equal_members, [{}]), (planted_gain_zero_clamp_and_overflow, [{}]), (planted_localization_edges_and_wrap, [{}]),
           (planted_observation_outside_the_rectangle_duplicates_and_overlap, [{}])]
PLANTED_IDS = [f.__name__[len("planted_"):] for f, _ in PLANTED]


def test_planted_wall_and_nonfinite_observations_are_skipped(pkg):
    planted_skipped(functools.partial(check, pkg))


def test_planted_nan_in_a_state_cell_leaves_that_channel_in_all_members(pkg):
    planted_state_nan(functools.partial(check, pkg))


def test_planted_equal_members_change_nothing_and_keep_the_sign_of_zero(pkg):
    planted_equal_members(functools.partial(check, pkg))


def test_planted_gain_zero_clamp_and_overflow(pkg):
    planted_gain_zero_clamp_and_overflow(functools.partial(check, pkg))


def test_planted_localization_edges_and_wrap(pkg):
    planted_localization_edges_and_wrap(functools.partial(check, pkg))


def test_planted_observation_outside_the_rectangle_duplicates_and_overlap(pkg):
    planted_observation_outside_the_rectangle_duplicates_and_overlap(functools.partial(check, pkg))


@pytest.mark.parametrize("case,placements", PLANTED, ids=PLANTED_IDS)
def test_planted_cases_with_a_load_group_of_8_and_a_member_behind_it(pkg, case, placements):
    """Every planted case on B = 9 members (the cases above are B = 5), and a wall in one member's state cell on both."""
    for kw in placements:
        case(functools.partial(check, pkg), B=9, **kw)
    if case is planted_state_wall:
        case(functools.partial(check, pkg), B=5)


# tools/find_assimilate_separators.py: (product, the three members' float32 values, observed value, error variance, member 0 after:
# defined bits, fused bits) -- n = 3, the observed cell itself, gain 1. A build that contracted d_k*e_k into Cq ("cov") or b*e_k into
# the difference ("post") would give the fused bits.
SEPARATORS = [
    ('cov', (300.39617919921875, 299.92718505859375, 299.12335205078125), -1096.30615234375, 1.5118639469146729, 3091058731, 3091058730),
    ('cov', (299.3281555175781, 300.3117980957031, 302.3080749511719), -21.53132438659668, 0.16793817281723022, 3058700249, 3058700250),
    ('cov', (299.3281555175781, 300.3117980957031, 302.3080749511719), -21.531322479248047, 0.16793817281723022, 3048309118, 3048309120),
    ('post', (299.03839111328125, 299.3913269042969, 302.111083984375), -194.23715209960938, 1.8405283689498901, 3083205586, 3083205585),
    ('post', (299.03839111328125, 299.3913269042969, 302.111083984375), -194.2371368408203, 1.8405283689498901, 3077630258, 3077630257),
    ('post', (302.5293273925781, 300.25897216796875, 299.1073303222656), -132.00440979003906, 1.3161383867263794, 3053764362, 3053764363),
]
SEPARATOR_KW = dict(loc=(1.0, 1.0), gain_base=(0, 0, 0, 1), gain_water=0.0)  # a footprint of 3 x 3 cells: the planted cells do not meet


def separator_cell(i, y=20):
    return 10 + 12 * i, y


def plant_separators(bases, walls, y=20):
    """Separator i's values into channel 3 of cell separator_cell(i) of members 0 .. 2 (made an air cell there); returns the observations."""
    obs = []
    for i, (_, t, value, R, _, _) in enumerate(SEPARATORS):
        x, _ = separator_cell(i, y)
        for k in range(3):
            bases[k][y, x, 3] = np.float32(t[k])
            walls[k][y, x, 1] = 5
        obs.append((B_, x, y, 3, value, R))
    return obs


def test_planted_separators_of_the_two_fused_products(pkg):
    X, Y = 10 + 12 * len(SEPARATORS), 5
    bases, waters, wl = members_of(3, X, Y, seed=31, walls=0.0)
    obs = plant_separators(bases, wl, y=2)
    gb, _, res = check(pkg, bases, waters, wl, X, Y, obs, "separators", **SEPARATOR_KW)
    assert all(r["applied"] for r in res) and {s[0] for s in SEPARATORS} == {"cov", "post"}
    for i, (_, _, _, _, defined, fused) in enumerate(SEPARATORS):
        x, y = separator_cell(i, 2)
        assert int(gb[0][y, x, 3].view(np.uint32)) == defined != fused, (i, int(gb[0][y, x, 3].view(np.uint32)), defined, fused)


def test_one_call_with_n_observations_equals_n_calls_of_one(pkg):
    X, Y, B = 19, 8, 6
    bases, waters, wl = members_of(B, X, Y, seed=3)
    obs = [(B_, 4, 3, 3, 301.0, 0.2), (W_, 6, 4, 0, 0.012, 1e-6), (B_, 4, 3, 3, 300.0, 0.1), (B_, 7, 2, 0, 0.2, 0.01), (W_, 15, 6, 3, 0.3, 0.01), (B_, 5, 3, 3, 299.0, 0.3)]
    kw = dict(loc=(4.0, 2.0), gain_base=(1, 0, 0, 1), gain_water=(1, 0, 0, 0.5), members=[0, 1, 3, 4, 5], rect=(1, 1, 17, 7), wrap_x=True)
    clear(wl, [(4, 3), (6, 4), (7, 2), (15, 6)])  # (5, 3) stays as it is: a wall in one member
    ob, ow, ores = pkg.engine.ens_assim_cells(bases, waters, wl, X, Y, obs, **kw)
    sb, sw, sres = bases, waters, []
    for o in obs:
        sb, sw, r = pkg.engine.ens_assim_cells(sb, sw, wl, X, Y, [o], **kw)
        sres += r
    assert all(same_bits(a, b) for a, b in zip(ob + ow, sb + sw))
    assert [tuple(np.float64(list(r.values())[1:]).view(np.uint64)) for r in ores] == [tuple(np.float64(list(r.values())[1:]).view(np.uint64)) for r in sres]
    assert [r["applied"] for r in ores] == [True] * 5 + [all(m[3, 5, 1] != 0 for i, m in enumerate(wl) if i != 2)]


def test_two_disjoint_rectangles_equal_their_union(pkg):
    """What the rectangle leaves free: two disjoint rectangles in two calls equal their union in one. THE CONDITION: every call must see
    the priors the union call sees, so no observed channel that the filter updates may be split away from the observations that follow
    it -- an observed cell updated by the first call would hand the second call its posterior as a prior. That holds (a) for one
    observation whose cell lies in the rectangle taken LAST, (b) when the observed channel has gain 0, and (c) when every observed cell
    lies outside both rectangles. In those cases the order of the two calls is free as well."""
    X, Y, B = 19, 8, 5
    bases, waters, wl = members_of(B, X, Y, seed=5)
    E = pkg.engine
    left, right, union = (2, 1, 7, 6), (9, 1, 8, 6), (2, 1, 15, 6)

    def split(obs, order, **kw):
        b, w = bases, waters
        for rect in order:
            b, w, _ = E.ens_assim_cells(b, w, wl, X, Y, obs, rect=rect, **kw)
        ub, uw, _ = E.ens_assim_cells(bases, waters, wl, X, Y, obs, rect=union, **kw)
        assert any(changed(a, c)[:, 2:9].any() for a, c in zip(ub, bases)) and any(changed(a, c)[:, 9:17].any() for a, c in zip(ub, bases))
        return all(same_bits(a, c) for a, c in zip(ub + uw, b + w))

    many = [(B_, 4, 3, 3, 301.0, 0.2), (B_, 11, 4, 3, 300.0, 0.1), (B_, 8, 5, 3, 299.0, 0.3), (B_, 4, 3, 3, 300.5, 0.2)]
    assert split([(B_, 8, 3, 3, 301.0, 0.2)], (right, left), loc=(6.0, 3.0), gain_base=(1, 0, 0, 1), gain_water=(1, 0, 0, 0))  # (a)
    for order in ((left, right), (right, left)):
        assert split(many, order, loc=(6.0, 3.0), gain_base=(1, 1, 0, 0), gain_water=(1, 0, 0, 1))  # (b)
        outside = [(B_, 0, 3, 3, 301.0, 0.2), (B_, 18, 4, 3, 300.0, 0.1), (B_, 9, 7, 3, 299.0, 0.3), (B_, 1, 2, 3, 300.5, 0.2)]
        assert split(outside, order, loc=(0.0, 0.0), gain_base=1.0, gain_water=1.0)  # (c)
    assert not split(many, (left, right), loc=(6.0, 3.0), gain_base=(0, 0, 0, 1))  # the condition is needed


def test_analytic_posterior_mean_and_variance_at_the_observed_cell(pkg):
    """One observation, gain 1, the observed cell inside the rectangle, n = 8: in exact arithmetic the posterior mean of the observed
    channel is hm + (V / D) innovation and its sample variance V R / D (the square-root filter's identity (1 - alpha V / D)^2 = R / D).
    The bounds are derived here. Each o_k is ONE double -> float32 rounding of a double result: |o_k - exact_k| <= h + u, h = half the
    largest float32 spacing among the o_k, u the double-arithmetic error (a handful of operations on numbers of size s: u <= 64 eps64 s).
    Mean: |error| <= h + u. Variance: with delta_k = o_k - exact_k and d_k the exact posterior deviations, the computed deviations
    differ from d_k by at most 2 (h + u), so |error| <= sum(2 |d_k| 2 (h + u) + (2 (h + u))^2) / (n - 1)."""
    X, Y, B = 11, 6, 8
    for seed, (value, R) in enumerate([(301.3, 0.25), (298.0, 4.0), (300.2, 1e-3)]):
        bases, waters, wl = members_of(B, X, Y, seed=20 + seed, walls=0.0)
        gb, _, res = pkg.engine.ens_assim_cells(bases, waters, wl, X, Y, [(B_, 5, 3, 3, value, R)], gain_base=1.0, loc=(3.0, 2.0), rect=(2, 1, 7, 4))
        r = res[0]
        hm, V, innovation = r["prior_mean"], r["prior_var"], r["innovation"]
        Rd = f32(R)
        D = V + Rd
        post = np.array([float(a[3, 5, 3]) for a in gb])
        h = 0.5 * float(np.max(np.spacing(np.abs(np.float32(post)))))
        s = max(abs(hm), abs(innovation), float(np.max(np.abs(post))))
        err = h + 64 * np.finfo(np.float64).eps * s
        mean = math.fsum(post) / B
        assert abs(mean - (hm + (V / D) * innovation)) <= err, (seed, mean, hm + (V / D) * innovation, err)
        dev = post - mean
        var = math.fsum(dev * dev) / (B - 1)
        bound = (math.fsum(4.0 * (np.abs(dev) + 2 * err) * err) + B * (2 * err) ** 2) / (B - 1)
        assert abs(var - V * Rd / D) <= bound, (seed, var, V * Rd / D, bound)
        assert var < V


def test_twin_experiment_on_host_arrays(pkg):
    """Truth + 8 perturbed members, 6 temperature observations of the truth: the ensemble mean moves towards the truth at the observed
    cells (RMS error) and the spread there shrinks."""
    X, Y, B = 31, 12, 8
    rng = np.random.Generator(np.random.Philox(99))
    yy, xx = np.mgrid[0:Y, 0:X]
    truth = (300.0 + 3.0 * np.sin(xx / 5.0) * np.cos(yy / 4.0)).astype(np.float32)

    def smooth(seed):
        r = np.random.Generator(np.random.Philox(seed))
        a, p, q = r.normal(0, 1.0, 3), r.uniform(0, 6.28, 3), r.uniform(0, 6.28, 3)
        return sum(a[i] * np.sin(xx / (4.0 + 2 * i) + p[i]) * np.cos(yy / (3.0 + i) + q[i]) for i in range(3))

    bases, waters, wl = [], [], []
    for i in range(B):
        b = np.zeros((Y, X, 4), np.float32)
        b[..., 3] = truth + smooth(i).astype(np.float32) + np.float32(0.8)  # a common bias on top of the member noise
        m = np.zeros((Y, X, 4), np.int8)
        m[1:, :, 1] = 3
        bases.append(b), waters.append(np.zeros((Y, X, 4), np.float32)), wl.append(m)
    cells = [(4, 3), (10, 8), (15, 5), (21, 2), (26, 9), (29, 6)]
    obs = [(B_, x, y, 3, float(truth[y, x]) + 0.05 * rng.normal(), 0.01) for x, y in cells]
    gb, _, res = pkg.engine.ens_assim_cells(bases, waters, wl, X, Y, obs, loc=(8.0, 5.0), wrap_x=False)
    assert all(r["applied"] for r in res)

    def rmse_and_spread(members):
        t = np.stack([m[..., 3].astype(np.float64) for m in members])
        at = np.array([[t[k, y, x] for x, y in cells] for k in range(B)])
        tr = np.array([float(truth[y, x]) for x, y in cells])
        return math.sqrt(np.mean((at.mean(axis=0) - tr) ** 2)), at.var(axis=0, ddof=1)

    (e0, s0), (e1, s1) = rmse_and_spread(bases), rmse_and_spread(gb)
    assert e1 < 0.5 * e0, (e0, e1)
    assert (s1 < s0).all(), (s0, s1)


_FAST_LEG = r"""
import ctypes as C, sys
import numpy as np
L, d = C.CDLL(sys.argv[1]), np.load(sys.argv[2])
X, Y, B, n_obs = (int(v) for v in d["shape"])
arrs = {k: [np.array(d["%s%d" % (k, i)]) for i in range(B)] for k in "bwm"}
ptrs = lambda a: (C.c_void_p * B)(*[x.ctypes.data for x in a])
res = np.zeros(n_obs * 5, np.float64)
L.wx_ens_assim_cells.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
rc = L.wx_ens_assim_cells(d["desc"].tobytes(), n_obs, d["obs"].tobytes(), res.ctypes.data, X, Y, B, ptrs(arrs["b"]), ptrs(arrs["w"]), ptrs(arrs["m"]), None)
np.savez(sys.argv[3], rc=rc, res=res, **{"%s%d" % (k, i): arrs[k][i] for k in "bw" for i in range(B)})
"""


def test_the_tolerance_build_host_function_gives_the_same_bits(pkg, tmp_path):
    """libwxsim_fast.so (-ffp-contract=fast) in a process of its own: its host function equals the definition too."""
    E = pkg.engine
    assert os.path.exists(E.FAST_LIB_PATH), "libwxsim_fast.so is built by __graft_entry__.build()"
    X, Y, B = 23, 9, 6
    bases, waters, wl = members_of(B, X, Y)
    obs = [(B_, 4, 3, 3, 301.0, 0.2), (W_, 6, 4, 0, 0.012, 1e-6), (B_, 4, 3, 3, 300.0, 0.1), (B_, 20, 2, 0, 0.2, 0.01)]
    kw = dict(loc=(5.0, 2.5), gain_base=(0.5, 0, 0, 1), gain_water=(1, 0.25, 0, 0), wrap_x=True)
    desc = E._assim_struct((0, 0, X, Y), kw["loc"], True, kw["gain_base"], kw["gain_water"], None, None, None, None)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, shape=[X, Y, B, len(obs)], desc=np.frombuffer(bytes(desc), np.uint8), obs=np.frombuffer(bytes(E._obs_array(obs)), np.uint8),
             **{"%s%d" % (k, i): a[i] for k, a in (("b", bases), ("w", waters), ("m", wl)) for i in range(B)})
    out = subprocess.run([sys.executable, "-c", _FAST_LEG, E.FAST_LIB_PATH, inp, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.load(outp)
    want_b, want_w, want_r = reference(bases, waters, wl, X, Y, obs, **kw)
    assert int(got["rc"]) == 0
    for i in range(B):
        assert same_bits(got["b%d" % i], want_b[i]) and same_bits(got["w%d" % i], want_w[i]), i
    res = got["res"].reshape(len(obs), 5)
    for j, r in enumerate(want_r):
        assert res[j, 0].view(np.int64) & 0xFFFFFFFF == 1 and r["applied"]
        assert [float(v) for v in res[j, 1:]] == [r["prior_mean"], r["prior_var"], r["innovation"], r["alpha"]], j


def test_host_function_under_the_sanitizers(tmp_path):
    """tests/native/ens_assim_main.cpp -- the header and a main() that runs wxa::assim_cells over the planted cases above and over
    randomised grids that end exactly at the last cell -- compiled stand-alone with AddressSanitizer and UBSan (host compiler, no device,
    no library) and run."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.call(["which", c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ens_assim_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "ens_assim_main.cpp")], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ens_assim_main ok" in out.stdout
