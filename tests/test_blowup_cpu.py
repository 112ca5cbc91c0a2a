"""The blow-up scenes (tests/blowup_scenes.py) and the oracle's contract on them, without a GPU: the oracle under the undefined-behaviour
sanitizer over every scene (it must DEFINE what it computes on NaN, Inf and back-traces of 1e30 cells), the same numbers from two
builds and thread counts, the conversion pinned by a reference in Python integers, and the claims the GPU file relies on -- every kind
changes the state next to its sites, the planted NaN spreads, the grown scenes really overflow inside their run, and the lattice
offsets meet the lanes of the kernels' strips."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import blowup_scenes as B
import impulse_scenes as I
import surface_scenes as S
from test_impulse_cpu import _missing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERATIONS = 6

# what the child process runs (stdin): every case x ITERATIONS on the library WX_ORACLE_LIB names, one digest per case on stdout
_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = [%(root)r, %(root)r + "/oracle", %(root)r + "/tests"]
import numpy as np
import blowup_scenes as B
import surface_scenes as S
import wx_oracle
names = json.loads(sys.argv[1])
out = {}
def run(name, X, Y, scene, u, n, iter0=0):
    base, water, wall, drops, _ = scene
    o = wx_oracle.OracleSim(X, Y, 0 if drops is None else len(drops))
    o.upload(base, water, wall, drops)
    o.set_params(u)
    o.iter = iter0
    h = hashlib.sha256()
    for _ in range(n):
        o.step(1)
        for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_1", "BASE_DISP", "WATER_0") + (("DROPS", "PRECIP_FB") if drops is not None else ()):
            a = o.field(f)
            h.update(np.where(np.isnan(a), np.float32(np.nan), a).tobytes() if a.dtype.kind == "f" else a.tobytes())  # (one NaN: payloads are not compared)
    o.close()
    out[name] = h.hexdigest()
for c in B.cases():
    for dry in sorted({cfg.startswith("dry") for cfg in c["configs"]}):
        name = B.case_id(c) + ("-dry" if dry else "")
        if name in names:
            run(name, c["X"], c["Y"], B.build_case(c), B.scene_uniforms(c["Y"], dry=dry, wrap=c["wrap"]), %(n)d)
if "droplets" in names:
    run("droplets", 505, 77, B.droplet_scene(505, 77), B.scene_uniforms(77, precipitation=True), %(n)d)
for sp in B.GROWN_SPEEDS:
    if "grown%%d" %% sp in names:
        run("grown%%d" %% sp, B.GROWN_GRID[0], B.GROWN_GRID[1], B.grown_scene(B.GROWN_GRID[0], B.GROWN_GRID[1], sp), B.scene_uniforms(B.GROWN_GRID[1]), B.GROWN_ITERATIONS)
for kind in S.DIVISOR_KINDS:  # the fire divisor 0 / -10 (surface_scenes.divisor_scene), first iteration at iterNum 1000
    for variant in S.VARIANTS:
        if "%%s-%%s" %% (kind, variant) in names:
            b, w, wl, sites = S.divisor_scene(S.PHASE_GRID[0], S.PHASE_GRID[1], kind, offset=1, variant=variant)
            run("%%s-%%s" %% (kind, variant), S.PHASE_GRID[0], S.PHASE_GRID[1], (b, w, wl, None, sites), S.scene_uniforms(S.PHASE_GRID[1]), %(n)d, iter0=1000)
print(json.dumps(out))
"""


def _names():
    n = []
    for c in B.cases():
        n += [B.case_id(c) + ("-dry" if dry else "") for dry in sorted({cfg.startswith("dry") for cfg in c["configs"]})]
    return n + ["droplets"] + ["grown%d" % sp for sp in B.GROWN_SPEEDS] + [f"{k}-{v}" for k in S.DIVISOR_KINDS for v in S.VARIANTS]


def _child(names, lib=None, threads=None):
    env = dict(os.environ)
    if lib:
        env["WX_ORACLE_LIB"] = lib
    if threads:
        env["OMP_NUM_THREADS"] = str(threads)
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "n": ITERATIONS}, json.dumps(names)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_case_ids_are_unique():
    n = _names()
    assert len(set(n)) == len(n) and len(B.cases()) >= 120


def test_oracle_defines_every_scene_under_ubsan_and_two_builds_agree(oracle):
    """`make -C oracle ubsan` (-fsanitize=undefined,float-cast-overflow, every report fatal), one thread, -O1, in a child process: no
    report on any scene x 6 iterations (the grown scenes: their whole run) -- and its results are those of the optimised OpenMP build
    (NaN payloads aside)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ubsan"])
    names = _names()
    san = _child(names, lib="libwxoracle_ubsan.so", threads=1)
    ref = _child(names)
    assert set(san) == set(names) == set(ref)
    differing = [n for n in names if san[n] != ref[n]]
    assert not differing, differing[:10]


def test_conversion_reference():
    """The contract's conversion in Python integers, on the values that decide it."""
    assert B.f2i_sat(float("nan")) == 0 and B.f2i_sat(float("inf")) == 2 ** 31 - 1 and B.f2i_sat(-float("inf")) == -2 ** 31
    assert B.f2i_sat(2.0 ** 31 - 128) == 2 ** 31 - 128 and B.f2i_sat(2.0 ** 31) == 2 ** 31 - 1 and B.f2i_sat(-2.0 ** 31) == -2 ** 31
    assert B.f2i_sat(-3e9) == -2 ** 31 and B.f2i_sat(B.FLT_MAX) == 2 ** 31 - 1 and B.f2i_sat(-7.0) == -7
    assert B.add_wrap32(2 ** 31 - 1, 1) == -2 ** 31 and B.add_wrap32(-2 ** 31, -1) == 2 ** 31 - 1 and B.add_wrap32(5, -7) == -2


@pytest.mark.parametrize("kind", B.HUGE_KINDS)
@pytest.mark.parametrize("X", [505, 512, 1000])
def test_huge_back_traces_land_where_python_integers_say(oracle, kind, X):
    """The plain reference that pins the oracle's helper. The advection pass alone on a field whose every texel names its own column and
    row: a free-air cell with a velocity of +-1e4 .. +-FLT_MAX copies the texel its back-trace lands on (the weights are exactly 0 / 1) --
    column (huge_vx) or row (huge_vy) computed here in Python integers: saturate, add in 32 bits, wrap. Both signs of every magnitude:
    beyond 2^31 the C cast this replaces returned INT_MIN for both on x86, so the negative speeds (positive positions) are the sharp half."""
    Y = 77
    base, water, wall, _, sites = B.blowup_scene(X, Y, kind, offset=(3, 5))
    ch = 0 if kind == "huge_vx" else 1
    tag = (np.arange(X) % 251)[None, :] * 1e-3 + np.arange(Y)[:, None] * 1e-6
    planted = np.abs(base[..., ch]) >= 1e3
    assert planted.sum() == len(sites) >= 2 * len(B.HUGE_VALUES)
    base[..., ch] = np.where(planted, base[..., ch], tag).astype(np.float32)
    base[..., 1 - ch] = 0.0
    o = oracle.OracleSim(X, Y, 0)
    o.upload(base, water, wall)
    o.set_params(dict(B.scene_uniforms(Y), pass_mask=8))
    o.step(1)
    out = o.field("BASE_CUR")
    o.close()
    seen = set()
    for k, (x, y) in enumerate(sites):
        v = float(base[y, x, ch])
        assert v == float(np.float32(B.site_value(kind, k)))
        i0, i1, frac = B.tap_columns(x if ch == 0 else y, v, X if ch == 0 else Y)
        assert frac == 0.0, (v, frac)
        want = base[y, i0, 0] if ch == 0 else base[i0, x, 1]
        assert out[y, x, ch] == want, (k, x, y, v, i0, float(out[y, x, ch]), float(want))
        seen.add((abs(v), v > 0))
    assert len(seen) == 2 * len(B.HUGE_VALUES)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("background,placement", [("air", "free"), ("air", "wall1"), ("air", "wall2"), ("terrain", "surface")])
def test_every_kind_changes_the_state_and_spreads_as_the_stencil_does(oracle, kind, background, placement):
    """Against the background alone: after one iteration the state differs within one cell of EVERY site (a kernel that ignored the
    trigger would not pass), and nowhere further than the stencil carries it in one iteration -- three columns and rows, plus the
    column below a site (light) and, for the finite huge kinds, nowhere but next to the sites either: the far tap is read, not written.
    Non-finite kinds: the number of non-finite texels grows over three iterations, every site has one within a cell after each."""
    X, Y = (505, 133) if background == "terrain" else B.PHASE_GRID
    sc = B.blowup_scene(X, Y, kind, offset=(3, 5), background=background, placement=placement)
    bg = list(B.blowup_scene(X, Y, kind, offset=(3, 5), background=background, placement=placement))
    sites = sc[4]
    assert len(sites) >= 4, (kind, placement, len(sites))
    for name, i in (("base", 0), ("water", 1)):  # the background: the same scene (planted wall cells included) without the trigger
        clean = I.impulse_scene(X, Y, "smoke", offset=(3, 5), background=background, plant=False)[i]
        for x, y in sites:
            bg[i][y, x] = clean[y, x]
    u = B.scene_uniforms(Y)

    def run(scene, n):
        o = oracle.OracleSim(X, Y, 0)
        o.upload(*scene[:3])
        o.set_params(u)
        res = []
        for _ in range(n):
            o.step(1)
            res.append((o.field("BASE_CUR"), o.field("WATER_CUR")))
        o.close()
        return res
    a, b = run(sc, 3), run(bg, 1)
    changed = (B.contract_mismatch(a[0][0], b[0][0]) | B.contract_mismatch(a[0][1], b[0][1])).any(-1)
    near = np.zeros((Y, X), bool)
    healed = kind in ("nan_water0", "nan_water2", "nan_water3")  # the boundary pass clamps these channels with max(.., 0): a NaN is gone after it (both sides: fmaxf)
    for x, y in sites:
        assert healed or changed[max(0, y - 1):y + 2][:, [(x - 1) % X, x, (x + 1) % X]].any(), (kind, x, y)
        near[max(0, y - 4):y + 5, [(x + d) % X for d in range(-4, 5)]] = True
        near[:y, x] = True
    assert not (changed & ~near).any(), (kind, np.argwhere(changed & ~near)[:5])
    if kind in B.NONFINITE_KINDS and not healed:
        prev = None
        for it, (bb, ww) in enumerate(a):
            nf = ~(np.isfinite(bb).all(-1) & np.isfinite(ww).all(-1))
            for x, y in sites:
                assert nf[max(0, y - 1):y + 2][:, [(x - 1) % X, x, (x + 1) % X]].any(), (kind, it, x, y)
            assert prev is None or nf.sum() > prev.sum(), (kind, it)
            prev = nf
    elif kind in B.HUGE_KINDS:  # the sharp family: almost every texel is finite after an iteration, i.e. compared bit for bit
        assert np.isfinite(a[0][0]).mean() > 0.98


@pytest.mark.parametrize("speed", B.GROWN_SPEEDS)
def test_grown_scenes_overflow_inside_their_run(oracle, speed):
    X, Y = B.GROWN_GRID
    base, water, wall, _, sites = B.grown_scene(X, Y, speed)
    assert np.isfinite(base).all() and np.isfinite(water).all() and len(sites) >= 20
    o = oracle.OracleSim(X, Y, 0)
    o.upload(base, water, wall)
    o.set_params(B.scene_uniforms(Y))
    first = None
    for it in range(1, B.GROWN_ITERATIONS + 1):
        o.step(1)
        if not (np.isfinite(o.field("BASE_CUR")).all() and np.isfinite(o.field("WATER_CUR")).all()):
            first = it
            break
    o.close()
    assert first is not None and first + B.GROWN_PAST <= B.GROWN_ITERATIONS, first


def test_droplet_scene(oracle):
    """The non-finite droplets deposit nothing and fault nothing; the finite droplet in quiet air deposits its sprite."""
    X, Y = 505, 77
    base, water, wall, drops, _ = B.droplet_scene(X, Y)
    o = oracle.OracleSim(X, Y, len(drops))
    o.upload(base, water, wall, drops)
    o.set_params(B.scene_uniforms(Y, precipitation=True))
    o.step(1)
    fb, d = o.field("PRECIP_FB"), o.field("DROPS")
    o.close()
    assert np.isfinite(d[7]).all() and not np.isfinite(d[6][:2]).all()
    x7 = 3 * X // 4
    assert np.abs(fb[:, x7 - 8:x7 + 8]).sum() > 0


def test_lattice_offsets_meet_the_strip_lanes():
    """tests/test_impulse_cpu.py's accounting on this case list: per kind that runs the full offset list, the free-air sites meet the
    first three, the last three and an interior output lane of the strip the kernel under test writes (56 columns wet / pairs, 60 the
    one-iteration dry kernel) in some row, and the grid's edge columns with the wrap on and off."""
    X, Y = B.PHASE_GRID
    for kind, configs, strip in (("nan_vx", B.WET_CONFIGS, I.WET_STRIP), ("huge_vx", B.WET_CONFIGS, I.WET_STRIP), ("huge_vx", B.DRY_CONFIGS, I.DRY_STRIP)):
        mine = [c for c in B.cases() if c["kind"] == kind and c["placement"] == "free" and c["background"] == "air" and c["configs"] == list(configs)]
        sites = [s for c in mine for s in I.lattice_sites(X, Y, I.PITCH, c["offset"])]
        full = (X // strip) * strip
        lanes = {x % strip for x, _ in sites if x < full}
        assert lanes >= {0, 1, 2, strip - 3, strip - 2, strip - 1} and any(3 <= l < strip - 3 for l in lanes), (kind, strip, sorted(lanes))
        assert not [m for m in _missing(X, Y, sites, ("edges",), strip) if m[1] in (0, 1, X - 2, X - 1)], kind
        for wrap in (True, False):
            cols = {x for c in mine if c["wrap"] == wrap for x, _ in I.lattice_sites(X, Y, I.PITCH, c["offset"])}
            assert cols & {0, 1} and cols & {X - 2, X - 1}, (kind, wrap)


def test_contract_comparison_is_sharp():
    a = np.array([1.0, np.nan, np.inf, -np.inf, 0.0, 2.0], np.float32)
    assert not B.contract_mismatch(a, a.copy()).any()
    b = np.array([np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0, -np.inf, np.nan, -0.0, np.nan], np.float32)
    assert B.contract_mismatch(b, a).tolist() == [True, True, True, True, True, True]
    qnan = np.array([0x7fc00001], np.uint32).view(np.float32)
    assert not B.contract_mismatch(qnan, np.array([np.nan], np.float32)).any()  # payloads are not compared
