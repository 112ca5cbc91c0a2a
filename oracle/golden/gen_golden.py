#!/usr/bin/env python3
"""Generate golden vectors from the REFERENCE shaders (container-only; needs /root/reference + kaleido).

Runs oracle/golden/harness.js inside kaleido's HeadlessChrome/SwiftShader (software GL), which loads the
reference's shader files from /root/reference at run time, and stores inputs + outputs as small ``.npz``
fixtures under tests/golden/. Only data (arrays, uniform values) is stored -- no reference source.

SwiftShader caveat: advectionShader output is corrupted for air pixels that share a
2x2 pixel quad with a wall pixel when the pass is drawn as the reference's full-screen quad. The round-1 fixtures therefore
keep wall/air boundaries on even x and even y; the round-2 fixtures (save100raw, randwalls64p, lightning64, airplane64,
setup256) draw every pass as one GL_POINT per pixel instead (harness.js, job option `points`), which has no neighbouring
fragments to go wrong with, and put walls anywhere -- including the reference's unmodified save.

usage:  python oracle/golden/gen_golden.py [fixture ...]     (default: all)
"""
from __future__ import annotations

import base64
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import wxpkg  # noqa: E402

pkg = wxpkg.load_package()
OUT_DIR = os.path.join(ROOT, "tests", "golden")
REF_SAVE = "/root/reference/saves/100 X 100 Test.weathersandbox"


def kaleido_exe() -> str:
    import kaleido
    return os.path.join(os.path.dirname(kaleido.__file__), "executable", "kaleido")


def run_harness(job: dict, timeout: float = 600.0) -> dict:
    """One harness run; ``job`` is passed as gd.layout.wx."""
    req = {"data": {"data": [], "layout": {"wx": job}}, "format": "json", "width": job["X"], "height": job["Y"], "scale": 1}
    cmd = [kaleido_exe(), "plotly", "--plotlyjs=" + os.path.join(HERE, "harness.js"), "--disable-gpu",
           "--allow-file-access-from-files", "--disable-breakpad", "--disable-dev-shm-usage", "--no-sandbox"]
    p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    try:
        p.stdin.write((json.dumps(req) + "\n").encode())
        p.stdin.flush()
        t0 = time.time()
        result = None
        while time.time() - t0 < timeout:
            line = p.stdout.readline()
            if not line:
                break
            try:
                msg = json.loads(line.decode())
            except Exception:
                continue
            if "result" in msg and msg.get("result") is not None:
                result = msg
                break
            if msg.get("code", 0) != 0:
                raise RuntimeError(f"kaleido error: {msg}")
        if result is None:
            raise RuntimeError("no result from kaleido")
    finally:
        try:
            p.stdin.close()
        except Exception:
            pass
        p.kill()
        p.wait()
    res = result["result"]
    if isinstance(res, str):
        res = json.loads(res)
    if "error" in res:
        raise RuntimeError("harness: " + res["error"])
    return res


def _dec(s: str, dtype) -> np.ndarray:
    return np.frombuffer(base64.b64decode(s), dtype=dtype).copy()


def js_uniforms(u: dict) -> dict:
    o = {}
    for k, v in u.items():
        if k in ("initial_T", "sounding_T", "sounding_W", "sounding_Vel"):
            continue
        o[k] = list(v) if isinstance(v, tuple) else v
    return o


def run_fixture(name, X, Y, base, water, wall, drops, u, *, niter, dump_iters, perpass_iter=None, precip=False,
                iter0=0, keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1", "water_0", "base_disp"), points=False,
                dump_emitted=False, keep_particles=("drops", "lightning", "precip_fb", "precip_dep"), timeout=600.0, keep_perpass=None,
                uniform_changes=None, store_inputs=True):
    tmp = tempfile.mkdtemp(prefix="wxgold_")
    np.ascontiguousarray(base, np.float32).tofile(os.path.join(tmp, "base.f32"))
    np.ascontiguousarray(water, np.float32).tofile(os.path.join(tmp, "water.f32"))
    np.ascontiguousarray(wall, np.int8).tofile(os.path.join(tmp, "wall.i8"))
    n_drops = 0 if drops is None else len(drops)
    if n_drops:
        np.ascontiguousarray(drops, np.float32).tofile(os.path.join(tmp, "drops.f32"))
    job = {
        "X": X, "Y": Y, "n_drops": n_drops, "dir": "file://" + tmp + "/",
        "uniforms": js_uniforms(u), "initial_T": [float(v) for v in u["initial_T"]],
        "niter": niter, "dump_iters": list(dump_iters), "precip": bool(precip), "iter0": iter0, "points": bool(points),
        "dump_emitted": bool(dump_emitted),
    }
    if uniform_changes:  # {iteration of the run: {uniform: value}} (harness.js): absent from every older fixture's job
        job["uniform_changes"] = {str(k): js_uniforms(v) for k, v in uniform_changes.items()}
    if "sounding_T" in u:
        job["sounding"] = {k: [float(v) for v in u["sounding_" + k]] for k in ("T", "W", "Vel")}
    if perpass_iter is not None:
        job["perpass_iter"] = perpass_iter
    probe = run_harness({"X": X, "Y": Y, "probe": True, "n_drops": 0, "points": bool(points)})
    varyings = _dec(probe["probe"], np.float32).reshape(Y, X, 4)
    res = run_harness(job, timeout=timeout)
    print(f"[{name}] renderer={res['renderer']!r} err={res['err']} {res['niter']} it, "
          f"{res['ms_after_first']:.1f} ms after first -> {1000.0 * (res['niter'] - 1) / max(res['ms_after_first'], 1e-9):.1f} it/s")
    out = {
        "X": X, "Y": Y, "iter0": iter0, "niter": niter, "precip": int(bool(precip)),
        "in_base": np.asarray(base, np.float32).reshape(Y, X, 4), "in_water": np.asarray(water, np.float32).reshape(Y, X, 4),
        "in_wall": np.asarray(wall, np.int8).reshape(Y, X, 4),
        "initial_T": np.asarray(u["initial_T"], np.float32),
        # simShader.vert varyings (fragCoord.xy, texCoord.xy) as interpolated by the reference's rasteriser here
        "varyings": varyings,
        "uniforms_json": json.dumps(js_uniforms(u)),
        **({"sounding_" + k: np.asarray(u["sounding_" + k], np.float32) for k in ("T", "W", "Vel")} if "sounding_T" in u else {}),
        "renderer": res["renderer"], "its_per_s": 1000.0 * (res["niter"] - 1) / max(res["ms_after_first"], 1e-9),
        "points": int(bool(points)),  # 1: every pass drawn as one GL_POINT per pixel (see harness.js), 0: as the reference's quad
    }
    if uniform_changes:
        out["uniform_changes_json"] = json.dumps({str(k): js_uniforms(v) for k, v in uniform_changes.items()})
    if not store_inputs:  # (a family of runs on one scene keeps the scene once: see fx_tools64)
        for k in ("in_base", "in_water", "in_wall", "varyings"):
            del out[k]
    if n_drops:
        out["in_drops"] = np.asarray(drops, np.float32).reshape(n_drops, 5)
    shapes = {"curl": (Y, X), "vort": (Y, X, 2), "precip_dep": (Y, X, 2), "drops": (-1, 5), "precip_drops": (-1, 5), "lightning": (4,)}
    for it, d in res["dumps"].items():
        for k, v in d.items():
            if k not in keep and k not in keep_particles and not (dump_emitted and k == "emitted"):
                continue
            dt = np.int8 if "wall" in k else np.float32
            out[f"it{it}_{k}"] = _dec(v, dt).reshape(shapes.get(k, (Y, X, 4)))
    for k, v in res.get("perpass", {}).items():
        if keep_perpass is not None and k not in keep_perpass:
            continue
        dt = np.int8 if "wall" in k else np.float32
        out[f"pp_{k}"] = _dec(v, dt).reshape(shapes.get(k, (Y, X, 4)))
    if "inactiveDroplets" in res:
        out["inactiveDroplets"] = res["inactiveDroplets"]
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    return out


# ------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------
def save100_quad_aligned():
    """The reference's only save, with terrain snapped to even x/y: sea and coast thickened to rows 0-1,
    the 20-column island raised to rows 0-3."""
    sf = pkg.codec.load(REF_SAVE)
    base, water, wall = sf.base.copy(), sf.water.copy(), sf.wall.copy()
    air1 = wall[1, :, 1] != 0
    for arr in (base, water, wall):
        arr[1, air1] = arr[0, air1]
    island = ~air1
    for y in (2, 3):
        for arr in (base, water, wall):
            arr[y, island] = arr[1, island]
    return sf, base, water, wall


def fx_save100(precip: bool):
    sf, base, water, wall = save100_quad_aligned()
    gui = pkg.params.merge_settings(sf.settings)
    u = pkg.params.uniforms_from_gui(gui, sf.Y)
    name = "save100qa_precip" if precip else "save100qa"
    if precip:  # particle state / feedback over 50 iterations; grid fields are covered by save100qa
        return run_fixture(name, sf.X, sf.Y, base, water, wall, sf.droplets, u, niter=50, dump_iters=[1, 10, 50],
                           precip=True, keep=("base_cur",))
    return run_fixture(name, sf.X, sf.Y, base, water, wall, None, u,
                       niter=50, dump_iters=[1, 10, 50], perpass_iter=0, precip=False,
                       keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1"))


def synth_terrain(X, Y, rng, gui=None):
    """Quad-aligned terrain with every wall type, snow, vegetation, moist warm air and cloud. ``gui``: settings other than the
    defaults with the sun at 60 degrees (the air is then built on THEIR initial_T and dryLapse)."""
    if gui is None:
        gui = dict(pkg.params.GUI_DEFAULTS)
        gui["sunAngle"] = 60.0
    u = pkg.params.uniforms_from_gui(gui, Y)
    T0 = u["initial_T"]
    base = np.zeros((Y, X, 4), np.float32)
    water = np.zeros((Y, X, 4), np.float32)
    wall = np.zeros((Y, X, 4), np.int8)
    height = np.full(X, 2)
    height[8:20] = 4
    height[12:16] = 8
    height[28:40] = 2
    height[40:44] = 6
    types = np.full(X, 2)  # sea
    types[6:24] = 1  # land island with hill
    types[28:34] = 4  # urban
    types[34:40] = 6  # industrial
    types[40:44] = 1
    types[44:48] = 3  # fire
    types[48:52] = 5  # runway
    types[52:56] = 0  # inert
    for x in range(X):
        h = height[x]
        wall[:h, x, 0] = types[x]
        wall[:h, x, 1] = 0
        wall[:h, x, 2] = np.arange(-(h - 1), 1)
        wall[:h, x, 3] = {1: 60 + (x % 7) * 9, 3: 90, 4: 40, 6: 10}.get(int(types[x]), 0)
        wall[h:, x, 0] = types[x]
        wall[h:, x, 1] = np.minimum(np.arange(1, Y - h + 1), 127)
        wall[h:, x, 2] = np.minimum(np.arange(1, Y - h + 1), 127)
        if types[x] == 2:
            base[:h, x, 3] = 298.15 + 0.05 * (x % 5)
            water[:h, x, 0] = 1002.0
            water[:h, x, 2] = 100.0
        else:
            base[:h, x, 3] = 1000.0
            water[:h, x, 0] = 1001.0
            water[:h, x, 2] = 5.0 + (x % 11) * 3.0  # soil moisture
            water[:h, x, 3] = 12.0 if 12 <= x < 16 else 0.0  # snow on the hill
    yy = np.arange(Y)[:, None]
    air = wall[..., 1] != 0
    base[..., 3] = np.where(air, T0[:Y][:, None] + rng.normal(0, 0.3, (Y, X)).astype(np.float32) + 2.0 * np.exp(-((yy - 10) / 6.0) ** 2), base[..., 3])
    base[..., 0] = np.where(air, rng.normal(0, 0.02, (Y, X)), 0).astype(np.float32)
    base[..., 1] = np.where(air, rng.normal(0, 0.02, (Y, X)), 0).astype(np.float32)
    base[..., 2] = np.where(air, rng.normal(0, 0.002, (Y, X)), base[..., 2]).astype(np.float32)
    realT = base[..., 3] - ((yy + 0.5) / Y) * u["dryLapse"]
    maxw = (realT / 250.0) ** 17
    tot = maxw * (0.7 + 0.5 * rng.random((Y, X)))
    water[..., 0] = np.where(air, tot, water[..., 0]).astype(np.float32)
    water[..., 1] = np.where(air, np.maximum(tot - maxw, 0), water[..., 1]).astype(np.float32)
    water[..., 2] = np.where(air, 0.05 * rng.random((Y, X)), water[..., 2]).astype(np.float32)
    water[..., 3] = np.where(air, 0.3 * rng.random((Y, X)) * (yy < 14), water[..., 3]).astype(np.float32)
    water[4:6, 44:48, 3] = 5.0  # flames above the fire cells
    return gui, u, base, water, wall


def fx_synth64():
    rng = np.random.default_rng(1234)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    # iterations 95..104: crosses iterNum%100==0 (soil smoothing, vegetation, fire spread) and %20==0 (sea T)
    return run_fixture("synth64", X, Y, base, water, wall, None, u, niter=10, dump_iters=[1, 5, 6, 10],
                       perpass_iter=5, precip=False, iter0=95,
                       keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1", "water_0"))


def fx_sounding64():
    """Real-sounding forcing (advectionShader.frag:154-181 with soundingForcing != 0) + globalDrying + globalHeating inside
    an altitude window: the per-row arrays are what app.js:5444-5463 builds from a sounding (here: synthetic profiles)."""
    rng = np.random.default_rng(77)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    sim_h = float(gui["simHeight"])
    u["soundingForcing"] = 0.6
    u["globalDrying"] = 2e-5
    u["globalHeating"] = 1e-4
    u["globalEffectsStartAlt"] = 1500.0 / sim_h
    u["globalEffectsEndAlt"] = 9000.0 / sim_h
    y = np.arange(Y + 1, dtype=np.float64)
    real_t = 292.0 - 70.0 * y / Y + 3.0 * np.sin(y * 0.4)  # K, with an inversion-like wiggle
    u["sounding_T"] = (real_t + (y / Y) * u["dryLapse"]).astype(np.float32)  # realToPotentialT
    u["sounding_W"] = (((real_t - 4.0 - 6.0 * (y / Y)) / 250.0) ** 17).astype(np.float32)  # maxWater(dew point)
    u["sounding_Vel"] = (0.05 + 0.25 * y / Y).astype(np.float32)  # cells / iteration
    return run_fixture("sounding64", X, Y, base, water, wall, None, u, niter=10, dump_iters=[1, 10], perpass_iter=0, precip=False,
                       keep=("base_cur", "water_cur", "wall_cur"))


def fx_precip64():
    """Particle pass: hand-built droplet set over a cloudy field (spawn / grow / freeze / melt / deposit)."""
    rng = np.random.default_rng(99)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    yy = np.arange(Y)[:, None]
    air = wall[..., 1] != 0
    # dense cloud deck (warm below, cold above) so inactive droplets do spawn
    deck = air & (yy >= 14) & (yy < 40)
    water[..., 1] = np.where(deck, 1.2 + 2.5 * rng.random((Y, X)), water[..., 1]).astype(np.float32)
    water[..., 0] = np.where(deck, water[..., 0] + water[..., 1], water[..., 0]).astype(np.float32)
    u["spawnChanceMult"] = 0.02
    u["enablePrecipitation"] = 1
    n = 256
    drops = np.zeros((n, 5), np.float32)
    drops[:, 0] = rng.random(n)
    drops[:, 1] = rng.random(n)
    drops[:, 2] = -10.0 + rng.random(n)
    drops[:, 3] = rng.random(n)
    drops[:, 4] = rng.random(n)
    k = 96  # active ones
    drops[:k, 0] = rng.uniform(-0.98, 0.98, k)
    drops[:k, 1] = rng.uniform(-0.9, 0.9, k)
    drops[:k, 2] = rng.uniform(0.0, 0.6, k)  # water
    drops[:k, 3] = np.where(rng.random(k) < 0.5, rng.uniform(0.0, 0.8, k), 0.0)  # ice
    drops[:k, 4] = np.where(drops[:k, 3] > 0, rng.uniform(0.2, 1.0, k), 1.0)
    drops[:8, 2] = 0.01  # too small -> evaporate
    drops[:8, 3] = 0.01
    drops[8:16, 1] = -0.97  # inside the ground -> deposit
    drops[16:20, 1] = -0.999
    return run_fixture("precip64", X, Y, base, water, wall, drops, u, niter=4, dump_iters=[1, 2, 4],
                       perpass_iter=0, precip=True,
                       keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1"))


BRUSH_CASES = [
    # (name, userInputType, (x, y), intensity, iterations); wall-editing tools run ONE iteration: afterwards the
    # circular edit is no longer quad aligned and SwiftShader's advection bug would corrupt the golden
    ("temperature", 1, (0.30, 0.30), 0.5, 3), ("temperature_sea", 1, (0.02, 0.03), 0.5, 3), ("water", 2, (0.30, 0.45), 0.1, 3),
    ("water_neg", 2, (0.30, 0.45), -0.1, 3), ("smoke", 3, (0.60, 0.30), 0.05, 3), ("wind", 4, (0.50, 0.50), 0.8, 3),
    ("wholewidth_temp", 1, (-1.0, 0.40), 0.2, 3), ("wholewidth_wind", 4, (-1.0, 0.40), 0.8, 3),
    ("wall_inert", 10, (0.70, 0.40), 0.01, 1), ("wall_land", 11, (0.30, 0.30), 0.01, 1), ("wall_sea", 12, (0.55, 0.20), 0.01, 1),
    ("wall_remove", 10, (0.22, 0.10), -0.01, 1), ("fire", 13, (0.20, 0.13), 0.01, 1), ("fire_out", 13, (0.72, 0.05), -0.01, 1),
    ("urban", 14, (0.20, 0.13), 0.01, 1), ("runway", 15, (0.50, 0.05), 0.01, 1), ("industrial", 16, (0.66, 0.10), 0.01, 1),
    ("urban_remove", 14, (0.48, 0.03), -0.01, 1), ("moisture", 20, (0.20, 0.13), 0.5, 3), ("snow", 21, (0.20, 0.13), 0.5, 3),
    ("snow_remove", 21, (0.22, 0.15), -0.5, 3), ("vegetation", 22, (0.20, 0.13), 0.01, 3), ("vegetation_remove", 22, (0.20, 0.13), -0.01, 3),
]


def fx_brush64():
    """User-brush branch of advectionShader.frag:229-401: every tool once, on the synth64 terrain."""
    rng = np.random.default_rng(1234)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    probe = run_harness({"X": X, "Y": Y, "probe": True, "n_drops": 0})
    out = {"X": X, "Y": Y, "in_base": base, "in_water": water, "in_wall": wall, "initial_T": np.asarray(u["initial_T"], np.float32),
           "varyings": _dec(probe["probe"], np.float32).reshape(Y, X, 4), "cases": json.dumps([c[0] for c in BRUSH_CASES])}
    tmp = tempfile.mkdtemp(prefix="wxgold_")
    base.tofile(os.path.join(tmp, "base.f32"))
    water.tofile(os.path.join(tmp, "water.f32"))
    wall.tofile(os.path.join(tmp, "wall.i8"))
    for name, ut, (bx, by), inten, nit in BRUSH_CASES:
        uu = dict(u, userInputType=ut, userInputValues=(bx, by, inten, 6.0), userInputMove=(0.004, -0.002))
        job = {"X": X, "Y": Y, "n_drops": 0, "dir": "file://" + tmp + "/", "uniforms": js_uniforms(uu),
               "initial_T": [float(v) for v in u["initial_T"]], "niter": nit, "dump_iters": [nit], "precip": False, "iter0": 0}
        res = run_harness(job)
        d = res["dumps"][str(nit)]
        out[f"{name}_uniforms"] = json.dumps(js_uniforms(uu))
        out[f"{name}_niter"] = nit
        out[f"{name}_base"] = _dec(d["base_cur"], np.float32).reshape(Y, X, 4)
        out[f"{name}_water"] = _dec(d["water_cur"], np.float32).reshape(Y, X, 4)
        out[f"{name}_wall"] = _dec(d["wall_cur"], np.int8).reshape(Y, X, 4)
        changed = int((out[f"{name}_wall"] != wall).any(-1).sum())
        print(f"[brush64] {name}: type {ut}, {nit} it, err={res['err']}, wall cells changed vs input: {changed}")
    path = os.path.join(OUT_DIR, "brush64.npz")
    np.savez_compressed(path, **out)
    print(f"[brush64] wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def fx_randwalls64():
    """Random 2x2-aligned wall blocks of every type: floating islands, overhangs, caves, one-block-wide gaps, sea next to
    air (dyke rule), walls in the top rows (y wrap) -- the wall-geometry branches of boundaryShader.frag:155-196,
    :245-269 and :373-388 that smooth terrain never reaches. One iteration at iterNum = 100 (soil / snow smoothing, vegetation, fire spread branches)."""
    rng = np.random.default_rng(4242)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    nb = 70
    for _ in range(nb):
        bx, by = int(rng.integers(0, X // 2)) * 2, int(rng.integers(1, Y // 2)) * 2
        w, h = int(rng.integers(1, 4)) * 2, int(rng.integers(1, 3)) * 2
        t = int(rng.integers(0, 7))
        ys, xs = slice(by, min(by + h, Y)), slice(bx, min(bx + w, X))
        wall[ys, xs, 0] = t
        wall[ys, xs, 1] = 0
        wall[ys, xs, 2] = 0
        wall[ys, xs, 3] = int(rng.integers(0, 120))
        base[ys, xs, 0:2] = 0.0
        base[ys, xs, 3] = 298.15 if t == 2 else 1000.0
        water[ys, xs, 0] = 1002.0 if t == 2 else 1001.0
        water[ys, xs, 1] = 0.0
        water[ys, xs, 2] = float(rng.integers(0, 60))
        water[ys, xs, 3] = float(rng.integers(0, 3)) * 6.0
    # Only the per-pass dumps up to the boundary pass are usable: the boundary pass grows walls by one row (fill rules),
    # after which they are no longer quad aligned and SwiftShader's advection output is garbage.
    out = run_fixture("randwalls64", X, Y, base, water, wall, None, u, niter=1, dump_iters=[], perpass_iter=0, precip=False,
                      iter0=100, keep=())
    path = os.path.join(OUT_DIR, "randwalls64.npz")
    keep = {k: v for k, v in out.items() if not k.startswith("pp_") or k.split("_")[1] in ("velocity", "curl", "vort", "boundary")}
    np.savez_compressed(path, **keep)
    print(f"[randwalls64] trimmed to the passes before advection: {os.path.getsize(path) / 1024:.0f} KiB")
    return keep


# ------------------------------------------------------------------------------------------------
# round-2 fixtures: every pass drawn as GL_POINTS (harness.js `points`), which side-steps SwiftShader's mixed-quad bug, so
# walls no longer have to sit on even x / even y
# ------------------------------------------------------------------------------------------------
def fx_save100raw():
    """BASELINE configs[0]: the reference's UNMODIFIED save (one-row sea, 20 x 2 island: nothing quad aligned), 1000
    iterations, sun fixed at the saved angle, precipitation off. Early dumps carry everything, late ones the three
    state textures."""
    sf = pkg.codec.load(REF_SAVE)
    gui = pkg.params.merge_settings(sf.settings)
    u = pkg.params.uniforms_from_gui(gui, sf.Y)
    return run_fixture("save100raw", sf.X, sf.Y, sf.base, sf.water, sf.wall, None, u, niter=1000, dump_iters=[1, 10, 50, 200, 1000],
                       perpass_iter=0, precip=False, keep=("base_cur", "water_cur", "wall_cur"), points=True, timeout=1800.0)


def fx_randwalls64p():
    """Random 1-cell-granular wall blocks of every type (floating islands, overhangs, caves, one-cell gaps, sea next to air,
    walls in the top rows) through the WHOLE iteration for 12 iterations from iterNum = 95 (crosses % 100 and % 20): bilerpWall
    next to irregular walls, the wall branch of advection, pressure and lighting on real terrain."""
    rng = np.random.default_rng(777)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    for _ in range(90):
        bx, by = int(rng.integers(0, X)), int(rng.integers(2, Y))
        w, h = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        t = int(rng.integers(0, 7))
        ys, xs = slice(by, min(by + h, Y)), slice(bx, min(bx + w, X))
        wall[ys, xs, 0] = t
        wall[ys, xs, 1] = 0
        wall[ys, xs, 2] = 0
        wall[ys, xs, 3] = int(rng.integers(0, 120))
        base[ys, xs, 0:2] = 0.0
        base[ys, xs, 3] = 298.15 if t == 2 else 1000.0
        water[ys, xs, 0] = 1002.0 if t == 2 else 1001.0
        water[ys, xs, 1] = 0.0
        water[ys, xs, 2] = float(rng.integers(0, 60))
        water[ys, xs, 3] = float(rng.integers(0, 3)) * 6.0
    return run_fixture("randwalls64p", X, Y, base, water, wall, None, u, niter=12, dump_iters=[1, 2, 6, 12], perpass_iter=0, precip=False,
                       iter0=95, keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1", "water_0"), points=True,
                       dump_emitted=True)


def _emitted_scene(seed):
    """synth64's terrain (every wall type; irregular blocks would grow into the sky within 60 iterations) plus smoke plumes dense enough
    to glow (lightingShader.frag:143-148: opacity > 0.8 <=> smoke > 4)."""
    rng = np.random.default_rng(seed)
    X, Y = 64, 64  # (Y >= 50: below that the top row passes boundaryShader.frag:192's `texCoord.y < 0.99` and the sky fills with wall)
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    air = wall[..., 1] != 0
    for _ in range(12):  # smoke plumes, 0 .. 14 g/m3
        cx, cy, r = rng.integers(0, X), rng.integers(4, Y - 4), rng.integers(2, 6)
        yy, xx = np.mgrid[0:Y, 0:X]
        d = np.hypot(xx - cx, yy - cy)
        water[..., 3] = np.where(air & (d < r), np.maximum(water[..., 3], 14.0 * (1.0 - d / r)), water[..., 3]).astype(np.float32)
    return X, Y, gui, u, base, water, wall


def fx_emitted64():
    """The lighting pass's second render target (emittedLight, RGBA16F): daylight at -30 degrees for 80 iterations (sunlight has
    reached the ground: air scattering, cloud / precipitation reflection, ground reflection, smoke glow) and a sun 2 degrees above
    the horizon for 6 iterations (red sunlight colour, urban / industrial / runway night glow). Dumped together with the light
    textures one iteration earlier, so the pass can be checked on the reference's own inputs."""
    X, Y, gui, u, base, water, wall = _emitted_scene(31337)
    keep = ("base_cur", "water_cur", "wall_cur", "light_0", "light_1")
    u_day = dict(u)
    u_day["sunAngle"] = float(np.deg2rad(-30.0))
    day = run_fixture("emitted64_day", X, Y, base, water, wall, None, u_day, niter=80, dump_iters=[1, 40, 79, 80], precip=False, iter0=7,
                      keep=keep, points=True, dump_emitted=True)
    u_night = dict(u)
    u_night["sunAngle"] = float(np.deg2rad(88.0))
    night = run_fixture("emitted64_night", X, Y, base, water, wall, None, u_night, niter=6, dump_iters=[5, 6], precip=False, iter0=7,
                        keep=keep, points=True, dump_emitted=True)
    return day, night


def fx_lightning64():
    """Lightning: a cold, very dense cloud deck (cloud + precipitation > 2.5 below 0 C) and a large pool of inactive droplets,
    from iterNum = 40 (> the 30-iteration lock-out of a fresh lightning texture), so that precipitationShader.vert:121-140
    requests strikes and lightningLocationShader.frag:24-38 accepts single ones, rejects double ones and the lock-out holds.
    EVERY iteration is dumped (post-advection base / water, droplets, feedback, lightning texture): the oracle's particle pass is
    checked per iteration on the reference's own inputs, because the strike decision hashes temperature BITS."""
    rng = np.random.default_rng(2024)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    yy = np.arange(Y)[:, None]
    air = wall[..., 1] != 0
    deck = air & (yy >= 22) & (yy < 44)  # rows where the real temperature is below freezing
    water[..., 1] = np.where(deck, 4.0 + 5.0 * rng.random((Y, X)), water[..., 1]).astype(np.float32)
    water[..., 0] = np.where(deck, water[..., 0] + water[..., 1], water[..., 0]).astype(np.float32)
    water[..., 2] = np.where(deck, 1.0 * rng.random((Y, X)), water[..., 2]).astype(np.float32)
    u["spawnChanceMult"] = 0.02
    u["enablePrecipitation"] = 1
    n = 1024
    drops = np.zeros((n, 5), np.float32)
    drops[:, 0] = rng.random(n)
    drops[:, 1] = rng.random(n)
    drops[:, 2] = -10.0 + rng.random(n)
    drops[:, 3] = rng.random(n)
    drops[:, 4] = rng.random(n)
    u["inactiveDroplets"] = float(n)
    niter = 48
    return run_fixture("lightning64", X, Y, base, water, wall, drops, u, niter=niter, dump_iters=list(range(1, niter + 1)), precip=True,
                       iter0=40, keep=("base_disp", "water_cur"), points=True)


AIRPLANE_CASES = [
    # airplaneValues = (x, y, -, mode): mode < 0 dumps water (advectionShader.frag:436-439), mode > 0.9 is a crash (:441-456)
    ("airplane_dump", (0.4, 0.5, 0.7, -1.0)), ("airplane_crash_air", (0.6, 0.6, 0.0, 1.0)), ("airplane_crash_ground", (0.2, 0.09, 0.0, 1.0)),
]


def fx_airplane64():
    """Airplane inputs of advectionShader.frag:415-457 on the synth64 terrain, 2 iterations each."""
    rng = np.random.default_rng(1234)
    X, Y = 64, 48
    gui, u, base, water, wall = synth_terrain(X, Y, rng)
    probe = run_harness({"X": X, "Y": Y, "probe": True, "n_drops": 0, "points": True})
    out = {"X": X, "Y": Y, "in_base": base, "in_water": water, "in_wall": wall, "initial_T": np.asarray(u["initial_T"], np.float32),
           "varyings": _dec(probe["probe"], np.float32).reshape(Y, X, 4), "cases": json.dumps([c[0] for c in AIRPLANE_CASES]), "points": 1}
    tmp = tempfile.mkdtemp(prefix="wxgold_")
    base.tofile(os.path.join(tmp, "base.f32"))
    water.tofile(os.path.join(tmp, "water.f32"))
    wall.tofile(os.path.join(tmp, "wall.i8"))
    nit = 2
    for name, av in AIRPLANE_CASES:
        uu = dict(u, userInputType=-1, airplaneValues=av)
        job = {"X": X, "Y": Y, "n_drops": 0, "dir": "file://" + tmp + "/", "uniforms": js_uniforms(uu), "points": True,
               "initial_T": [float(v) for v in u["initial_T"]], "niter": nit, "dump_iters": [nit], "precip": False, "iter0": 0}
        res = run_harness(job)
        d = res["dumps"][str(nit)]
        out[f"{name}_uniforms"] = json.dumps(js_uniforms(uu))
        out[f"{name}_niter"] = nit
        out[f"{name}_base"] = _dec(d["base_cur"], np.float32).reshape(Y, X, 4)
        out[f"{name}_water"] = _dec(d["water_cur"], np.float32).reshape(Y, X, 4)
        out[f"{name}_wall"] = _dec(d["wall_cur"], np.int8).reshape(Y, X, 4)
        print(f"[airplane64] {name}: err={res['err']}, wall cells changed vs input: {int((out[f'{name}_wall'] != wall).any(-1).sum())}")
    path = os.path.join(OUT_DIR, "airplane64.npz")
    np.savez_compressed(path, **out)
    print(f"[airplane64] wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def fx_setup256():
    """The setup draw of a new simulation (setupShader.frag:36-92; uniforms app.js:5479-5485, 5732-5734) at 4096 x 96 (the noise
    terrain needs a few thousand columns to rise out of the sea) with the defaults synth.terrain_grid documents (seed 0.5,
    heightMult 0.3). Stored compactly: per-column wall height / type / vegetation / snow, per-row air state."""
    X, Y = 4096, 96
    gui = pkg.params.merge_settings(None)
    u = pkg.params.uniforms_from_gui(gui, Y)
    job = {"X": X, "Y": Y, "n_drops": 0, "points": True, "initial_T": [float(v) for v in u["initial_T"]],
           "setup": {"seed": 0.5, "heightMult": 0.3, "simHeight": float(gui["simHeight"]), "dryLapse": float(u["dryLapse"])}}
    res = run_harness(job)
    out = {"X": X, "Y": Y, "seed": 0.5, "heightMult": 0.3, "simHeight": float(gui["simHeight"]), "dryLapse": float(u["dryLapse"]),
           "initial_T": np.asarray(u["initial_T"], np.float32), "renderer": res["renderer"],
           "base": _dec(res["base"], np.float32).reshape(Y, X, 4), "water": _dec(res["water"], np.float32).reshape(Y, X, 4),
           "wall": _dec(res["wall"], np.int8).reshape(Y, X, 4)}
    path = os.path.join(OUT_DIR, "setup256.npz")
    # the output is column / row structured: keep the full wall texture (int8, compresses well) and float planes as they are
    np.savez_compressed(path, **out)
    print(f"[setup256] err={res['err']} wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB); wall cells: {int((out['wall'][..., 1] == 0).sum())}")
    return out


# ------------------------------------------------------------------------------------------------
# sliders64: the same physics at OTHER VALUES of the uniforms. Every earlier fixture runs at (nearly) the GUI's defaults, several of
# which are multiplicative identities (IR_rate = aboveZeroThreshold = 1); these scenes draw every control the simulation reads from
# the range the reference's GUI offers (params.GUI_RANGES), stratified over the family.
# ------------------------------------------------------------------------------------------------
SLIDERS64_N = 8
SLIDERS64_PRECIP = (1, 4, 7)       # precipitation on, hand-built droplets
SLIDERS64_NOWRAP = (0, 2, 4, 6)    # wrapHorizontally off, with an input at the x edge that the non-wrapping distance decides
SLIDERS64_SUN = (90.0, 60.0, 4.0, -8.0, 135.0, 176.5, 30.0, 188.0)  # noon exactly (the ray leaves through the top row), day, low sun, below the horizon (it enters from under row 0)
SLIDERS64_PRECIP_ONLY = ("aboveZeroThreshold", "subZeroThreshold", "spawnChance", "snowDensity", "fallSpeed", "growthRate0C", "growthRate_30C",
                         "freezingRate", "meltingRate", "evapRate", "meltingHeat")
# (tool, (x, y), intensity) held for the whole run in the scenes without wrap: brush64's encoding of userInputType / userInputValues
SLIDERS64_BRUSH = {0: (1, (0.02, 0.30), 0.04), 2: (12, (0.985, 0.12), 0.01), 4: (2, (0.01, 0.45), 0.02), 6: (4, (0.99, 0.50), 0.8)}


def sliders64_gui(k):
    """Settings of scene k: a Latin hypercube with a fixed seed over params.GUI_RANGES. Each control's range is cut into SLIDERS64_N
    strata -- the lowest 6 %, the highest 6 %, and equal parts of what lies between -- and every scene gets another one, so that over
    the family each control sits at its low end, at its high end and at interior values, never at its default. Controls only the
    particle pass reads get their low / high / one interior stratum in the three scenes that run it."""
    rng = np.random.default_rng(640048)
    R, D = pkg.params.GUI_RANGES, pkg.params.GUI_DEFAULTS
    n = SLIDERS64_N
    strata = [(0.0, 0.06)] + [(0.06 + 0.88 * i / (n - 2), 0.06 + 0.88 * (i + 1) / (n - 2)) for i in range(n - 2)] + [(0.94, 1.0)]
    guis = [dict(D) for _ in range(n)]
    for name, (lo, hi) in R.items():
        order = [int(i) for i in rng.permutation(n)]  # order[scene] = stratum
        if name in SLIDERS64_PRECIP_ONLY:  # low, high and an interior stratum inside the scenes with droplets
            want = [0, n - 1, 1 + int(rng.integers(0, n - 2))]
            rest = [i for i in range(n) if i not in want]
            order = [None] * n
            for sc, st in zip(SLIDERS64_PRECIP, [want[int(i)] for i in rng.permutation(3)]):
                order[sc] = st
            for sc, st in zip([i for i in range(n) if i not in SLIDERS64_PRECIP], [rest[int(i)] for i in rng.permutation(len(rest))]):
                order[sc] = st
        pos = rng.random(n)
        for sc in range(n):
            a, b = strata[order[sc]]
            f = a + (b - a) * float(pos[sc])
            v = lo + (hi - lo) * f
            if name in D and abs(v - float(D[name])) < 0.02 * (hi - lo):  # never the default itself
                v = float(D[name]) + (0.03 if f < 0.9 else -0.03) * (hi - lo)
            guis[sc][name] = float(v)
    g = guis[k]
    s, e = sorted((g["globalEffectsStartAlt"], g["globalEffectsEndAlt"]))  # the GUI keeps start <= end (app.js:3524-3544)
    g["globalEffectsStartAlt"], g["globalEffectsEndAlt"] = s * g["simHeight"], max(e, s + 0.25) * g["simHeight"] if e < s + 0.25 else e * g["simHeight"]
    g["globalEffectsEndAlt"] = min(g["globalEffectsEndAlt"], g["simHeight"])
    g["sunAngle"] = SLIDERS64_SUN[k]
    g["wrapHorizontally"] = k not in SLIDERS64_NOWRAP
    g["dynamicWaterTemperature"] = bool(k % 3)
    g["enablePrecipitation"] = k in SLIDERS64_PRECIP
    return g


def _sliders64_sounding(u, Y, seed):
    """Synthetic realWorldSounding_* rows (as fx_sounding64): soundingForcing acts in every scene."""
    y = np.arange(Y + 1, dtype=np.float64)
    real_t = 290.0 + seed - (70.0 - 2.0 * seed) * y / Y + 3.0 * np.sin(y * 0.4 + seed)
    u["sounding_T"] = (real_t + (y / Y) * u["dryLapse"]).astype(np.float32)
    u["sounding_W"] = (((real_t - 4.0 - 6.0 * (y / Y)) / 250.0) ** 17).astype(np.float32)
    u["sounding_Vel"] = ((0.05 + 0.25 * y / Y) * (1.0 if seed % 2 else -1.0)).astype(np.float32)


def _sliders64_drops(rng, n=256, k=96):
    """fx_precip64's hand-built droplet set, plus one heavy droplet already below the bottom edge (precipitationShader.vert's
    `newPos.y < -1.0` side of the deposit test) and a few right above the ground."""
    drops = np.zeros((n, 5), np.float32)
    drops[:, 0] = rng.random(n)
    drops[:, 1] = rng.random(n)
    drops[:, 2] = -10.0 + rng.random(n)
    drops[:, 3] = rng.random(n)
    drops[:, 4] = rng.random(n)
    drops[:k, 0] = rng.uniform(-0.98, 0.98, k)
    drops[:k, 1] = rng.uniform(-0.9, 0.9, k)
    drops[:k, 2] = rng.uniform(0.0, 0.6, k)
    drops[:k, 3] = np.where(rng.random(k) < 0.5, rng.uniform(0.0, 0.8, k), 0.0)
    drops[:k, 4] = np.where(drops[:k, 3] > 0, rng.uniform(0.2, 1.0, k), 1.0)
    drops[:8, 2] = 0.01
    drops[:8, 3] = 0.01
    drops[8:16, 1] = -0.97
    drops[16:20, 1] = -0.999
    drops[20] = (0.31, -1.0005, 0.3, 0.2, 0.7)  # left the domain through the bottom
    drops[21:28, 1] = rng.uniform(-0.8, -0.6, 7)  # rain / snow a few cells above the ground: falls in, deposits
    return drops


# Seeds of the scenes' random fields. The scenes with droplets run freely for 20 iterations, and an inactive droplet spawns when
# spawnChance > fract(pow(cloud * 10, 2)) (precipitationShader.vert:113) -- of values around 1000, so one ulp of the driver's pow()
# moves that threshold by 1e-4 and now and then a droplet decides differently (tests/test_oracle_golden.py, lightning64). These
# seeds are the first of 6400 + k, + 10, + 20 ... for which no decision of the run sits that close to its threshold.
SLIDERS64_SEED = {1: 6481, 4: 6414, 7: 6437}


def fx_sliders64(k, seed=None):
    rng = np.random.default_rng(SLIDERS64_SEED.get(k, 6400 + k) if seed is None else seed)
    X, Y = 64, 48
    gui = sliders64_gui(k)
    _, u, base, water, wall = synth_terrain(X, Y, rng, gui)
    _sliders64_sounding(u, Y, k)
    precip = k in SLIDERS64_PRECIP
    drops = None
    if precip:
        yy = np.arange(Y)[:, None]
        air = wall[..., 1] != 0
        deck = air & (yy >= 3) & (yy < 40)  # cloud deck from the warm rows (above 0 C up to row 8 or so) into the cold ones, denser than both thresholds' whole range
        water[..., 1] = np.where(deck, 2.2 + 2.5 * rng.random((Y, X)), water[..., 1]).astype(np.float32)
        water[..., 0] = np.where(deck, water[..., 0] + water[..., 1], water[..., 0]).astype(np.float32)
        drops = _sliders64_drops(rng)
        u["inactiveDroplets"] = float(20 * k)  # what the host counts every 600 iterations (app.js:5957-5966); 0 until then
    if k in SLIDERS64_BRUSH:
        tool, (bx, by), inten = SLIDERS64_BRUSH[k]
        u.update(userInputType=tool, userInputValues=(bx, by, inten, 6.0), userInputMove=(0.004, -0.002))
    if k == 2:
        u["airplaneValues"] = (0.995, 0.5, 0.7, -1.0)  # water dump in the last column: with wrap it would reach column 0
    # iterations 90..109 / 585..604: across iterNum % 100 == 0 and % 20 == 0
    return run_fixture(f"sliders64_{k:02d}", X, Y, base, water, wall, drops, u, niter=20, dump_iters=[1, 5, 20], perpass_iter=0,
                       precip=precip, iter0=585 if k % 2 else 90, keep=("base_cur", "water_cur", "wall_cur", "light_1"), points=True,
                       keep_particles=("drops", "precip_fb", "precip_dep"), keep_perpass=SLIDERS64_PERPASS)


SLIDERS64_PERPASS = ("velocity_base", "vort", "boundary_base", "boundary_water", "boundary_wall", "advection_base", "advection_water",
                     "advection_wall", "pressure_base", "lighting_light", "precip_fb", "precip_dep", "precip_drops")


def fx_sliders64_lightning():
    """fx_lightning64's cold dense deck and droplet pool under off-default settings, every iteration dumped: lightning requests
    (the 1-px sprite on texel (1,0)) with snowDensity / meltingHeat / subZeroThreshold / spawnChance away from their defaults."""
    rng = np.random.default_rng(6499)
    X, Y = 64, 48
    gui = sliders64_gui(SLIDERS64_PRECIP[1])
    gui.update(wrapHorizontally=True, sunAngle=60.0)
    _, u, base, water, wall = synth_terrain(X, Y, rng, gui)
    yy = np.arange(Y)[:, None]
    air = wall[..., 1] != 0
    realT = base[..., 3] - ((yy + 0.5) / Y) * u["dryLapse"]
    deck = air & (realT < 268.0) & (yy < Y - 4)
    water[..., 1] = np.where(deck, 4.0 + 5.0 * rng.random((Y, X)), water[..., 1]).astype(np.float32)
    water[..., 0] = np.where(deck, water[..., 0] + water[..., 1], water[..., 0]).astype(np.float32)
    water[..., 2] = np.where(deck, 1.0 * rng.random((Y, X)), water[..., 2]).astype(np.float32)
    u["spawnChanceMult"] = 0.02  # (as lightning64: far above the GUI's range, so that a pool of 1024 requests strikes within a few iterations)
    u["enablePrecipitation"] = 1
    n = 1024
    drops = np.zeros((n, 5), np.float32)
    drops[:, 0] = rng.random(n)
    drops[:, 1] = rng.random(n)
    drops[:, 2] = -10.0 + rng.random(n)
    drops[:, 3] = rng.random(n)
    drops[:, 4] = rng.random(n)
    u["inactiveDroplets"] = float(n)
    niter = 6
    return run_fixture("sliders64_lightning", X, Y, base, water, wall, drops, u, niter=niter, dump_iters=list(range(1, niter + 1)), precip=True,
                       iter0=40, keep=("base_disp", "water_cur"), points=True)



# ------------------------------------------------------------------------------------------------
# surface64: the slow physics of the surface row (boundaryShader.frag:305-480) -- vegetation growth, fire spread and burn-down, the
# industrial chimneys, dust, the sea's temperature reset. Drawn as GL_POINTS. Each scene is built so that the reference's own dumps
# show the event (tests/test_oracle_surface.py asserts it from them).
# ------------------------------------------------------------------------------------------------
def surface_terrain(X, Y, rng, height, types, veg, soil, snow, gui=None, sun=80.0, wind=0.02):
    """Hand-built terrain: per column the wall rows, surface type, vegetation, soil moisture and snow; quiet moist air above."""
    if gui is None:
        gui = dict(pkg.params.GUI_DEFAULTS)
        gui["sunAngle"] = sun
    u = pkg.params.uniforms_from_gui(gui, Y)
    T0 = u["initial_T"]
    base = np.zeros((Y, X, 4), np.float32)
    water = np.zeros((Y, X, 4), np.float32)
    wall = np.zeros((Y, X, 4), np.int8)
    for x in range(X):
        h, t = int(height[x]), int(types[x])
        wall[:, x, 0] = t
        wall[:h, x, 2] = np.arange(-(h - 1), 1)
        wall[:h, x, 3] = veg[x]
        wall[h:, x, 1] = np.minimum(np.arange(1, Y - h + 1), 127)
        wall[h:, x, 2] = np.minimum(np.arange(1, Y - h + 1), 127)
        base[:h, x, 3] = 298.15 if t == 2 else 1000.0
        water[:h, x, 0] = 1002.0 if t == 2 else 1001.0
        water[:h, x, 2] = 100.0 if t == 2 else soil[x]
        water[:h, x, 3] = 0.0 if t == 2 else snow[x]
    yy = np.arange(Y)[:, None]
    air = wall[..., 1] != 0
    base[..., 3] = np.where(air, T0[:Y][:, None] + rng.normal(0, 0.1, (Y, X)).astype(np.float32), base[..., 3])
    base[..., 0] = np.where(air, rng.normal(0, wind, (Y, X)), 0).astype(np.float32)
    base[..., 1] = np.where(air, rng.normal(0, wind, (Y, X)), 0).astype(np.float32)
    realT = base[..., 3] - ((yy + 0.5) / Y) * u["dryLapse"]
    water[..., 0] = np.where(air, (realT / 250.0) ** 17 * 0.6, water[..., 0]).astype(np.float32)
    return gui, u, base, water, wall


def _trim(name, out, keep_full, its):
    """Re-save a fixture with base / water kept at the dumps ``keep_full`` only (the wall texture at every dump)."""
    path = os.path.join(OUT_DIR, name + ".npz")
    dropped = tuple(f"it{it}_" for it in its if it not in keep_full)
    keep = {k: v for k, v in out.items() if k.endswith("wall_cur") or not k.startswith(dropped)}
    np.savez_compressed(path, **keep)
    print(f"[{name}] trimmed: {os.path.getsize(path) / 1024:.0f} KiB")


def fx_surface64_growth(it_growth=9_240_000, name="surface64_growth"):
    """Vegetation growth: flat and stepped land whose soil moisture makes every rate 1 .. 10 occur under full sunlight (and, soaked,
    rates beyond 100: interval 0), vegetation below and above the temperature cap. The sunlight needs Y iterations to come down, so
    the run starts 70 iterations before ``it_growth`` -- 9 240 000, the least common multiple of the ten intervals (exact as a float);
    10 000 in the second fixture, where rates 3 and 6 .. 9 must NOT grow."""
    rng = np.random.default_rng(8101)
    # 64 rows. With fewer than 50 the top row's texCoord.y is below 0.99, so boundaryShader's "wall above -> wall" rule (the row above the
    # top row is row 0, the ground) fills it, then the row under it: a ceiling comes down one row per iteration and no sunlight with it
    X, Y = 64, 64
    x = np.arange(X)
    height = np.where((x >= 40) & (x < 52), 4, 2) + np.where((x >= 44) & (x < 48), 3, 0)
    types = np.ones(X, np.int64)
    soil = 2.0 + 0.5 * x  # 2 .. 33.5: rate (int)(soil * sqrt(light) * 0.01) = 0 .. 11 at ~1270 W/m2
    soil[56:] = (150.0, 300.0, 450.0, 600.0, 800.0, 1000.0, 290.0, 285.0)  # rates 50 .. 350: (100 / rate) * 100 is 100 or 0
    veg = np.where(x % 3 == 0, 100, np.where(x % 3 == 1, 20, 45))  # above the cap (about 55 at 11 C), far below, below
    snow = np.zeros(X)
    gui, u, base, water, wall = surface_terrain(X, Y, rng, height, types, veg, soil, snow)
    pre = 70
    its = [pre, pre + 1, pre + 5]
    out = run_fixture(name, X, Y, base, water, wall, None, u, niter=pre + 5, dump_iters=its, precip=False, iter0=it_growth - pre,
                      keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1"), points=True)
    _trim(name, out, (pre + 1,), its)


def _fire_strip(rng, X=64, Y=48):
    """Flat land, two wall rows, vegetation 60, soil moisture 5 (spread divisor 10), quiet air."""
    return dict(height=np.full(X, 2), types=np.ones(X, np.int64), veg=np.full(X, 60), soil=np.full(X, 5.0), snow=np.zeros(X))


def fx_surface64_fire():
    """How a fire ENDS: vegetation 10 on soil moisture 1 burns every 4348th iteration (intensity 0.0023) down to 9 and back to land;
    rain above a fire and soaked soil under another put them out at once; a fourth keeps burning. Twelve iterations from iterNum 8690:
    8696 = 2 x 4348; 8700 smooths, but 87 is a multiple of no divisor here (10 beside the fires): nothing may spread."""
    rng = np.random.default_rng(8102)
    X, Y = 64, 48
    t = _fire_strip(rng)
    types, veg, soil = t["types"], t["veg"], t["soil"]
    types[12] = 3  # keeps burning: smoke and heat above it
    types[30], veg[30], soil[30] = 3, 10, 1.0  # burn-down
    types[34], veg[34] = 3, 90  # rain above it
    types[38], veg[38], soil[38] = 3, 60, 300.0  # soaked
    gui, u, base, water, wall = surface_terrain(X, Y, rng, t["height"], types, veg, soil, t["snow"], wind=0.005)
    water[2:6, 33:36, 2] = 3.0   # precipitation (display channel) over the fire at 34
    water[2:4, 11:14, 3] = 5.0   # flames
    its = [1, 5, 6, 7, 11, 12]
    out = run_fixture("surface64_fire", X, Y, base, water, wall, None, u, niter=12, dump_iters=its, precip=False, iter0=8690,
                      keep=("base_cur", "water_cur", "wall_cur"), points=True)
    _trim("surface64_fire", out, (1, 7, 12), its)


SPREAD_RINGS = ((5.0, 0.0), (15.0, 0.0), (5.0, 3.4), (22.0, 2.4))  # (soil moisture, snow) at distance 1 .. 4: divisors 10, 11, 12, 13


def fx_surface64_spread():
    """How a fire SPREADS, over four smoothing iterations: from iterNum 995 a fire at column 12 takes one cell each way at 1000, 1100,
    1200 and 1300, because the rings around it carry soil moisture / snow whose divisors `(int)(soil * 0.1 + snow * 0.5) + 10` are 10,
    11, 12 (dry, under snow) and 13 (moist, under snow) -- each a value that a wrong factor moves to another integer. A second fire
    between vegetation 20 (ignites) and 19 (never). Smoke of 4.9, 5.3 and 4.3 over vegetated land: above 4.5 ignites at 1000."""
    rng = np.random.default_rng(8104)
    X, Y = 64, 64  # (not 48: see fx_surface64_growth -- below 50 rows the ceiling comes down and the domain is solid after Y iterations)
    t = _fire_strip(rng)
    types, veg, soil, snow = t["types"], t["veg"], t["soil"], t["snow"]
    types[12] = 3
    for d, (so, sn) in enumerate(SPREAD_RINGS, start=1):
        for xx in (12 - d, 12 + d):
            soil[xx], snow[xx] = so, sn
    types[26] = 3
    veg[25], veg[27] = 20, 19
    gui, u, base, water, wall = surface_terrain(X, Y, rng, t["height"], types, veg, soil, snow, wind=0.005)
    water[2:4, 11:14, 3] = 5.0    # flames
    water[2:6, 36:43, 3] = 4.9    # smoke over vegetated land: above the threshold
    water[2:6, 45:52, 3] = 5.3
    water[2:6, 54:61, 3] = 4.3    # below it
    its = [5, 6, 105, 106, 205, 206, 305, 306, 310]
    out = run_fixture("surface64_spread", X, Y, base, water, wall, None, u, niter=310, dump_iters=its, precip=False, iter0=995,
                      keep=("base_cur", "water_cur", "wall_cur"), points=True, timeout=1200.0)
    _trim("surface64_spread", out, (5, 6, 310), its)


def fx_surface112_industry():
    """Industry, dust and the sea: industrial surface under the columns with x % 80 = 17 .. 30 in the first period AND the second
    (X = 112: the modulus is not the identity), urban cells with vegetation 100 beside it (caps 15 / 75), bare dry soil under wind
    (dust), sea cells uploaded at 600 K across iterNum 100 (a multiple of 20: reset to 25 C)."""
    rng = np.random.default_rng(8103)
    X, Y = 112, 40
    x = np.arange(X)
    height = np.full(X, 2)
    types = np.ones(X, np.int64)
    types[(x % 80 >= 17) & (x % 80 <= 30)] = 6
    types[(x >= 32) & (x < 38)] = 4
    types[(x >= 60) & (x < 72)] = 2
    veg = np.full(X, 100)
    veg[40:56] = np.where(x[40:56] % 2 == 0, 5, 12)  # bare (below 10) and not
    soil = np.full(X, 20.0)
    soil[40:56] = 1.0  # (the dust line does not read it: its "soil moisture" is channel 2 of the AIR cell, the precipitation there)
    snow = np.zeros(X)
    gui, u, base, water, wall = surface_terrain(X, Y, rng, height, types, veg, soil, snow)
    base[2:8, 38:58, 0] = 0.35  # wind over the bare soil
    water[2, [44, 46], 2] = 6.0  # precipitation of 5 and more in the first air cell of two bare columns: no dust there
    base[:2, 62:66, 3] = 600.0  # sea far above 500 K
    base[:2, 66:68, 3] = 499.0  # and just below: clamped, not reset
    return run_fixture("surface112_industry", X, Y, base, water, wall, None, u, niter=10, dump_iters=[1, 10], perpass_iter=0, precip=False, iter0=100,
                       keep=("base_cur", "water_cur", "wall_cur"), points=True, keep_perpass=("boundary_base", "boundary_water", "boundary_wall"))


# ------------------------------------------------------------------------------------------------
# tools64 / crash64: the wall-editing tools (advectionShader.frag:291-400) and the airplane crash (:444-457) over EVERY surface type,
# held and then RELEASED in one run (harness.js `uniform_changes`), with 20 iterations after the release. Drawn as GL_POINTS: a
# circular edit is not quad aligned. tests/test_oracle_tools.py asserts from these dumps alone that every edit happened where the
# shader says and nowhere else.
# ------------------------------------------------------------------------------------------------
TOOLS64_X = TOOLS64_Y = 64
TOOLS64_ITER0 = 990   # the held iterations are 990 ..; 1000 (fire spread: 10 is a multiple of the divisor 10 of soil moisture 5) falls inside the 20 after release
CRASH64_ITER0 = 997
TOOLS64_AFTER = 20
WALL_TOOLS = (10, 11, 12, 13, 14, 15, 16, 20, 21, 22)
# |intensity| per tool: the wall-type tools read its sign only; soil moisture moves by 10 x, snow by 0.5 x
TOOLS64_INTENSITY = {20: 0.7, 21: 3.0}
TOOLS64_VEG = (60, 0, 127, 1, 126)  # by x % 5: co-prime with the stretches' 4 and the period 28, so every type meets every value
# (centre x, centre y, radius) in cells, by held iterations. Held 1: over the first period of the terrain, the surface row well
# inside. Held 3: over the second period and centred BELOW the surface, so that towards its rim it removes buried cells and leaves
# the surface cell above them. tools64_discs() moves them by 1e-3 cells until no cell centre lies within 1e-5 (relative) of the rim.
TOOLS64_DISCS = {1: (14.31, 5.23, 14.6), 3: (42.27, 1.37, 14.9)}
TOOLS64_EXTRA = (("wholewidth", 10, -1, 1), ("wholewidth", 21, +1, 1), ("nowrap", 12, +1, 1), ("nowrap", 13, +1, 1), ("nowrap", 10, -1, 1))
TOOLS64_NOWRAP_DISC = (1.83, 4.61, 9.7)  # cut by x = 0; with the wrap on it would reach columns 56 .. 63 as well
TOOLS64_BAND = (2.07, 2.2)  # whole-width mode: centre row (cells) and half-width: rows 0 .. 3 (|dy| < 2.2)
RIM_MARGIN = 1e-5


def tools64_terrain():
    """Every surface type as a stretch of four columns, twice (columns 0 .. 27 and 28 .. 55: inert, land, sea, fire, urban, runway,
    industrial), then eight flat land columns. Four wall rows (three buried cells under every surface cell); the third column of a
    stretch is one row HIGHER in the first period, the third and fourth one row LOWER in the second (two columns: a pit ONE cell wide
    whose floor a tool turns into land blows up within three iterations, in the reference as in the oracle -- the air cell in it takes
    the whole soil moisture at once -- and a state with NaN is the blow-up tests' business, not this family's). Two floating blocks (rows 8 .. 9 over columns
    5 .. 6 and 45 .. 46): cells with air below them. Vegetation 60 / 0 / 127 / 1 / 126 by x % 5, soil moisture 5 / 30 / 80 by x % 3
    and snow 6 / 1 on two residues of x % 7 -- except on the first land stretch and the last eight columns, which keep soil moisture
    5 without snow (fire divisor 10: what is lit there spreads at iterNum 1000) and, the last eight, vegetation 60."""
    rng = np.random.default_rng(8201)
    X, Y = TOOLS64_X, TOOLS64_Y
    x = np.arange(X)
    types = np.where(x < 56, (x % 28) // 4, 1)
    height = np.full(X, 4)
    height[(x < 28) & (x % 4 == 2)] = 5
    height[(x >= 28) & (x < 56) & (x % 4 >= 2)] = 3
    veg = np.array(TOOLS64_VEG)[x % 5]
    soil = np.array((5.0, 30.0, 80.0))[x % 3]
    snow = np.where(x % 7 == 0, 6.0, np.where(x % 7 == 3, 1.0, 0.0))
    plain = ((x >= 4) & (x < 8)) | (x >= 56)
    soil[plain], snow[plain] = 5.0, 0.0
    veg[x >= 56] = 60
    gui, u, base, water, wall = surface_terrain(X, Y, rng, height, types, veg, soil, snow, wind=0.005)
    for cols in ((5, 6), (45, 46)):
        for xx in cols:
            wall[8:10, xx, 1] = 0
            wall[8:10, xx, 2] = (-1, 0)
            wall[8:10, xx, 3] = 60
            wall[10:, xx, 1] = np.minimum(np.arange(1, Y - 9), 127)
            wall[10:, xx, 2] = np.minimum(np.arange(1, Y - 9), 127)
            base[8:10, xx] = (0.0, 0.0, 0.0, 1000.0)
            water[8:10, xx] = (1001.0, 0.0, 5.0, 0.0)
    return gui, u, base, water, wall


def disc_distance(varyings, cx, cy, wrap):
    """advectionShader.frag:241-249 in float32 on the stored texCoords (square grid: the aspect factor is 1)."""
    f = np.float32
    tcx, tcy = varyings[..., 2].astype(f), varyings[..., 3].astype(f)
    a = f(cx)
    dx = np.abs(a - tcx)
    if wrap:  # absHorizontalDist (common.glsl:268-271)
        dx = np.minimum(np.minimum(dx, np.abs(f(1.0) + a - tcx)), f(1.0) - a + tcx)
    dy = f(cy) - tcy
    return np.sqrt(dx * dx + dy * dy, dtype=f)


def rim_clear(varyings, values, wrap):
    """No cell within RIM_MARGIN (relative) of the rim: `length()` / `sqrt` may round either way there."""
    r = np.float32(values[3]) * np.float32(1.0 / varyings.shape[0])
    if values[0] < -0.5:
        d = np.abs(np.float32(values[1]) - varyings[..., 3].astype(np.float32))
    else:
        d = disc_distance(varyings, values[0], values[1], wrap)
    return bool((np.abs(d.astype(np.float64) - float(r)) > RIM_MARGIN * float(r)).all())


def tools64_values(varyings, disc, inten, wrap=True):
    """userInputValues of a disc given in cells, nudged until the rim is clear."""
    cx, cy, r = disc
    for k in range(200):
        v = ((cx + 1e-3 * k) / TOOLS64_X, (cy + 1e-3 * k) / TOOLS64_Y, inten, r)
        if rim_clear(varyings, v, wrap):
            return tuple(float(np.float32(c)) for c in v)
    raise RuntimeError("no clear rim")


def _tools64_run(name, scene, u, varyings, tool, values, held, wrap=True, fields_at=None):
    gui, _, base, water, wall = scene
    assert rim_clear(varyings, values, wrap)
    uu = dict(u, userInputType=tool, userInputValues=values, userInputMove=(0.0, 0.0), wrapHorizontally=int(wrap))
    n = held + TOOLS64_AFTER
    its = sorted({held, held + 1, n})
    out = run_fixture(name, TOOLS64_X, TOOLS64_Y, base, water, wall, None, uu, niter=n, dump_iters=its, precip=False, iter0=TOOLS64_ITER0,
                      keep=("base_cur", "water_cur", "wall_cur"), points=True, uniform_changes={held: {"userInputType": -1}}, store_inputs=False)
    _trim(name, out, fields_at if fields_at is not None else ((held, n) if held == 1 else (n,)), its)
    return out


def _tools64_scene():
    scene = tools64_terrain()
    probe = run_harness({"X": TOOLS64_X, "Y": TOOLS64_Y, "probe": True, "n_drops": 0, "points": True})
    varyings = _dec(probe["probe"], np.float32).reshape(TOOLS64_Y, TOOLS64_X, 4)
    return scene, scene[1], varyings


def fx_tools64_in():
    """The scene of the tools64 / crash64 family, once: inputs, varyings, settings."""
    scene, u, varyings = _tools64_scene()
    path = os.path.join(OUT_DIR, "tools64_in.npz")
    np.savez_compressed(path, X=TOOLS64_X, Y=TOOLS64_Y, in_base=scene[2], in_water=scene[3], in_wall=scene[4], varyings=varyings,
                        initial_T=np.asarray(u["initial_T"], np.float32), uniforms_json=json.dumps(js_uniforms(u)), points=1)
    print(f"[tools64_in] wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def fx_tools64_quiet():
    """No tool at all: what the edited runs are compared WITH by the non-vacuity test (the tool acts on the wall texture the boundary
    pass of the same iteration wrote, which is this run's)."""
    scene, u, varyings = _tools64_scene()
    for wrap, name in ((True, "tools64_quiet"), (False, "tools64_quiet_nowrap")):
        out = run_fixture(name, TOOLS64_X, TOOLS64_Y, scene[2], scene[3], scene[4], None, dict(u, wrapHorizontally=int(wrap)), niter=3, dump_iters=[1, 3],
                          precip=False, iter0=TOOLS64_ITER0, keep=("base_cur", "water_cur", "wall_cur"), points=True, store_inputs=False)
        _trim(name, out, (1,), [1, 3])


def tools64_name(tool, sign, held, mode="disc"):
    return f"tools64_{'' if mode == 'disc' else mode + '_'}t{tool}{'p' if sign > 0 else 'n'}_h{held}"


def fx_tools64(tool, sign, held, mode="disc"):
    scene, u, varyings = _tools64_scene()
    inten = sign * TOOLS64_INTENSITY.get(tool, 0.01)
    if mode == "wholewidth":
        values = tools64_values(varyings, (-TOOLS64_X, TOOLS64_BAND[0], TOOLS64_BAND[1]), inten)
        values = (-1.0,) + values[1:]
        assert rim_clear(varyings, values, True)
    elif mode == "nowrap":
        values = tools64_values(varyings, TOOLS64_NOWRAP_DISC, inten, wrap=False)
    else:
        values = tools64_values(varyings, TOOLS64_DISCS[held], inten)
    return _tools64_run(tools64_name(tool, sign, held, mode), scene, u, varyings, tool, values, held, wrap=mode != "nowrap")


# (name, column, row) of the crash's centre cell: its 3 x 3 cells lie within 1.5 cells. Surface land (the flat stretch at the end),
# land with nothing but buried cells in reach, every other surface type, open air.
CRASH64_CASES = (("land", 59, 3), ("buried", 61, 1), ("inert", 1, 3), ("sea", 9, 3), ("fire", 13, 3), ("urban", 17, 3), ("runway", 21, 3),
                 ("industrial", 25, 3), ("air", 40, 30), ("stepped_land", 33, 3))


def fx_crash64(case):
    """airplaneValues[3] = 1 for ONE iteration (iterNum 997), then released; 23 iterations in all, across 1000."""
    scene, u, varyings = _tools64_scene()
    if case == "quiet":  # no plane: what the crashed runs' first iteration is compared with
        out = run_fixture("crash64_quiet", TOOLS64_X, TOOLS64_Y, scene[2], scene[3], scene[4], None, dict(u, userInputType=-1), niter=1, dump_iters=[1],
                          precip=False, iter0=CRASH64_ITER0, keep=("base_cur", "water_cur", "wall_cur"), points=True, store_inputs=False)
        return _trim("crash64_quiet", out, (1,), [1])
    name, cx, cy = next(c for c in CRASH64_CASES if c[0] == case)
    av = ((cx + 0.5) / TOOLS64_X, (cy + 0.5) / TOOLS64_Y, 0.0, 1.0)
    uu = dict(u, userInputType=-1, airplaneValues=av)
    its = [1, 2, 23]
    out = run_fixture("crash64_" + name, TOOLS64_X, TOOLS64_Y, scene[2], scene[3], scene[4], None, uu, niter=23, dump_iters=its, precip=False,
                      iter0=CRASH64_ITER0, keep=("base_cur", "water_cur", "wall_cur"), points=True,
                      uniform_changes={1: {"airplaneValues": (0.0, 0.0, 0.0, 0.0)}}, store_inputs=False)
    _trim("crash64_" + name, out, (1,) if name not in ("land", "air") else (1, 23), its)


TOOLS64_RUNS = [(t, s, h, "disc") for t in WALL_TOOLS for s in (+1, -1) for h in (1, 3)] + [(t, s, h, m) for m, t, s, h in TOOLS64_EXTRA]


# ------------------------------------------------------------------------------------------------
# sun64: the sun at the angles where the lighting pass's bilinear tap changes its columns and rows (tests/light_scenes.py has the
# classes): GUI 180 and GUI 0 (sin = +-1 in float32: columns x + 1, x + 2 / x - 1, x), the floats next below +-pi/2, -1e-30 (floor(sin a) = -1
# with weight 1.0 on the right column of the two) and +-float32(pi). No other family has them. 64 x 48 WITHOUT walls (light_scenes.light_scene:
# below 50 rows a ceiling would grow down as fast as the light enters), drawn as GL_POINTS; 48 iterations under GUI 60 let the light
# in -- it travels one row per iteration, and below the horizon nothing enters at all -- then `uniform_changes` turns the sun to the
# specimen (the angle alone: sunIntensity stays GUI 60's) and 8 more iterations run; the last two are dumped.
# ------------------------------------------------------------------------------------------------
SUN64 = ("gui180", "gui0", "below_half_pi", "neg_below_half_pi", "neg_tiny", "pi", "neg_pi")
SUN64_FILL, SUN64_UNDER = 48, 8
# a domain 3 km high instead of 12: without a floor the top row's upper neighbour is row 0 (REPEAT), and the step of the initial profile
# across that seam -- 40 K at 12 km -- is what the reference's fixed-point filter weights act on
SUN64_SIM_HEIGHT = 3000.0


def fx_sun64(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import light_scenes as L
    X, Y = 64, 48
    # (without the cells of smoke beyond 4: the bounds the fixtures are compared with are absolute, and the reference's fixed-point filter
    # weights move an advected 17 by 1e-5 within these 56 iterations)
    base, water, wall = L.light_scene(X, Y, thick_smoke=False, sim_height=SUN64_SIM_HEIGHT)
    u = L.scene_uniforms(Y, sim_height=SUN64_SIM_HEIGHT)
    n = SUN64_FILL + SUN64_UNDER
    return run_fixture("sun64_" + name, X, Y, base, water, wall, None, u, niter=n, dump_iters=[n - 1, n], precip=False, iter0=0,
                       keep=("base_cur", "water_cur", "wall_cur", "light_0", "light_1"), points=True,
                       uniform_changes={SUN64_FILL: {"sunAngle": float(L.angle_of(L.SPECIMENS[name][0]))}})


FIXTURES = {
    **{"sun64_" + n: (lambda n=n: fx_sun64(n)) for n in SUN64},
    "randwalls64": fx_randwalls64,
    "brush64": fx_brush64,
    "save100qa": lambda: fx_save100(False),
    "save100qa_precip": lambda: fx_save100(True),
    "synth64": fx_synth64,
    "sounding64": fx_sounding64,
    "precip64": fx_precip64,
    "save100raw": fx_save100raw,
    "randwalls64p": fx_randwalls64p,
    "lightning64": fx_lightning64,
    "emitted64": fx_emitted64,
    "airplane64": fx_airplane64,
    "setup256": fx_setup256,
    **{f"sliders64_{k:02d}": (lambda k=k: fx_sliders64(k)) for k in range(SLIDERS64_N)},
    "sliders64_lightning": fx_sliders64_lightning,
    "surface64_growth": fx_surface64_growth,
    "surface64_growth10k": lambda: fx_surface64_growth(10_000, "surface64_growth10k"),
    "surface64_fire": fx_surface64_fire,
    "surface64_spread": fx_surface64_spread,
    "surface112_industry": fx_surface112_industry,
    "tools64_in": fx_tools64_in,
    "tools64_quiet": fx_tools64_quiet,
    **{tools64_name(t, s, h, m): (lambda t=t, s=s, h=h, m=m: fx_tools64(t, s, h, m)) for t, s, h, m in TOOLS64_RUNS},
    **{"crash64_" + c[0]: (lambda c=c: fx_crash64(c[0])) for c in CRASH64_CASES},
    "crash64_quiet": lambda: fx_crash64("quiet"),
}

if __name__ == "__main__":
    names = sys.argv[1:] or list(FIXTURES)
    for nm in names:
        FIXTURES[nm]()
