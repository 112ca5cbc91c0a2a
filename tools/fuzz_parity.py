#!/usr/bin/env python3
"""Differential fuzzer: the HIP path (through the C ABI, default kernel set and options a host can pick) against the CPU oracle, BIT FOR
BIT, on randomly drawn cases -- grid size (tiny, ragged, a strip / a tile / a band border away from the launch shapes' corners), terrain,
flow speed (up to several cells per iteration: the exact paths), humidity / cloud / smoke / snow, settings (every slider inside the range
the reference's GUI offers), pass mask (all passes / the dry stencil), brush tool and airplane inputs, droplets in deterministic splat
order, the way a host cuts its iterations into steps, dry pairs on / off, row bands, waterTexture_0 on demand / stored. --mode group: the same
scenes cut into 2 .. 8 column slabs on this one GPU (the library's own halo exchange, random halo widths, overlapped / split / in-order
protocol, droplet pool in exact mode) against the undecomposed handle, bit for bit. --mode script: the scenes of oracle mode, but the HOST'S
CALL SEQUENCE is drawn as well (draw_script, from a generator of its own) -- 2 .. 5 steps, some cut into a WX_OVERLAP_MORE_TO_COME piece and
the rest, and between them any of SCRIPT_ACTIONS:
    read        a random subset (possibly empty) of all readable fields in random order, whole or a sub-rectangle, some twice in a row
                (both wall dtypes, EMITTED as binary16, VORT while the per-pass set ran, PRECIP_FB / PRECIP_DEP / LIGHTNING on every grid)
    particles   a range of the droplet pool                     stream      wx_stream_frame of a viewport == wx_read_rect of its fields
    option      KERNEL_SET, DRY_KERNEL, DRY_PAIRS, ROW_BANDS, WATER0_ON_DEMAND, CHECK_LAUNCHES, SPLAT_ORDER (stays 1) at any point
    params      sliders / sun angle / another initial_T row / brush / airplane / pass mask dry <-> all / precipitation / wrap
    iter        wx_set_iter on and next to multiples of 20, 100, 600      step0       a step of no iterations
    tune        wx_tune_placement(1-2 tries, 1-3 iterations): counter, every field, droplets, lightning and wx_pair_stats unchanged
    devwrite    devtools.seed_flow / seed_vortices / a torch write through wx_device_ptr(BASE_CUR), mirrored into the oracle's state;
                every field is compared afterwards (BASE_DISP and WATER_0 belong to the last display iteration, not to the edit)
    reupload    the current state uploaded again (droplets too)          lightning   wx_lightning_set, mirrored
    pair_stats, fastest, water_free, sync, profile (on / off + read)      calls with side effects, interleaved
--mode impulse: the impulse-lattice scenes of tests/impulse_scenes.py (lone single-cell triggers; grid, kind, pitch, offset and configuration
drawn by draw_impulse from a generator of its own), run by run_impulse_case.
After the last step everything is read. Fields are compared where both sides define them alike (CURL / VORT / EMITTED after a step that
ran the passes that store them). The recipe, script included, is printed and flushed BEFORE the case runs and reproduces the case alone.
A WxError other than the exact path's reported overflow is not expected: the run ends there (exit 2). This is not a tool to provoke
faults with: run it under `timeout`, and find the cause of a fault or hang from the recipe before starting the case again.

    python tools/fuzz_parity.py [--mode M] [--seed S] [--cases N] [--seconds T] [--max-cells C] [--only K] [--override JSON] [--sun-exact] [--check-launches]

Every case prints one line; a mismatch prints the case's recipe (the seed reproduces it: --seed S --only K) and the run exits 1 at the
end. The oracle is the checker (test infrastructure); nothing here is a product path."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import wxpkg  # noqa: E402

GRID_FIELDS = ["BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1"]
# Sliders of the reference's GUI: the table is params.GUI_RANGES (checked against app.js:3481-3745), shared with oracle/golden/gen_golden.py.
# SLIDERS are the 17 controls draw_case has always drawn from its main generator, in the table's order (the draws of existing seeds are
# pinned, tests/test_fuzz_draw_cpu.py). Four of them keep the interval this fuzzer has always used instead of the GUI's, on purpose:
# globalDrying / globalHeating ten / two times wider than the GUI (a superset), condensationRate from 0 (below the GUI's 0.001), and
# soundingForcing up to 0.001 only -- these scenes carry no realWorldSounding_* arrays, so the term relaxes towards zero profiles.
_GUI_RANGES = wxpkg.load_package().params.GUI_RANGES
FUZZ_INTERVALS = {"globalDrying": (0.0, 0.001), "globalHeating": (-0.002, 0.002), "condensationRate": (0.0, 0.01), "soundingForcing": (0.0, 0.001)}
SLIDERS = {k: FUZZ_INTERVALS.get(k, _GUI_RANGES[k]) for k in list(_GUI_RANGES)[:17]}
# The rest of what the simulation reads -- the precipitation folder and the start dialog's simHeight (dryLapse and initial_T) -- is drawn
# from a CHILD generator seeded by values the main one has already produced, so that adding it left every earlier draw where it was
# (draw_more_sliders, recipe key "sliders_more": draw_case's own recipe is byte for byte what it was; recipes without the key, the
# committed regressions, run as they always did). spawnChance is left out: the
# scenes with droplets fix spawnChanceMult at 0.01, two orders above the GUI's range, or grids this small would hardly ever spawn.
SLIDERS_MORE = {k: _GUI_RANGES[k] for k in ("aboveZeroThreshold", "subZeroThreshold", "snowDensity", "fallSpeed", "growthRate0C", "growthRate_30C",
                                            "freezingRate", "meltingRate", "evapRate", "simHeight")}


def _draw_more(seed_words, chance):
    r = np.random.default_rng([int(w) & 0x7FFFFFFF for w in seed_words])
    return {k: float(r.uniform(*SLIDERS_MORE[k])) for k in SLIDERS_MORE if r.random() < chance}


def draw_more_sliders(c):
    """Adds c["sliders_more"] to a case of draw_case (SLIDERS_MORE): a pure function of the case, no draw from its generator."""
    c["sliders_more"] = _draw_more([c["data_seed"], 0x51D], 0.35)
    return c


# The surface row's life cycle (tests/surface_scenes.py): surface types beyond land and sea on stretches of the terrain, vegetation /
# soil moisture / snow over their clamped ranges, and a first iteration just below a multiple of 100 / 1000 / 10 000 / the least common
# multiple of the growth intervals -- drawn like draw_more_sliders, as a function of the case (recipe key "surface").
SURFACE_TYPES = (1, 3, 4, 5, 6)  # land, fire, urban, runway, industrial
SURFACE_ITER_BASES = (100, 200, 1000, 2000, 10000, 30000, 9240000)


def draw_surface(c):
    """Adds c["surface"]: {"stretches": [[start, width (fractions of X), type, vegetation, soil moisture, snow], ...], "iter0": first
    iteration or None (keep the case's)}. No draw from the case's generator."""
    r = np.random.default_rng([int(c["data_seed"]) & 0x7FFFFFFF, 0x5FACE])
    n = int(r.integers(1, 7)) if c["terrain"] else 0
    st = [[float(r.random()), float(r.uniform(0.002, 0.15)), int(r.choice(SURFACE_TYPES)), int(r.integers(0, 128)),
           float(r.choice([0.0, 3.0, 5.0, 25.0, 250.0, 1000.0]) * r.random()), float(r.choice([0.0, 0.0, 30.0, 4000.0]) * r.random())] for _ in range(n)]
    it0 = int(r.choice(SURFACE_ITER_BASES)) - int(r.integers(0, 9)) if r.random() < 0.6 else None
    c["surface"] = {"stretches": st, "iter0": it0}
    return c


# Clone mid-run (wx_copy_state): after one of the case's steps the handle is copied into a SECOND handle with options of its own, both go
# on with the same calls, and the second is compared with the first after every further step -- bit for bit (droplets run under
# WX_OPT_SPLAT_ORDER 1 on both). Drawn like draw_more_sliders, as a function of the case (recipe key "clone"; recipes without it run as
# they always did).
def draw_clone(c):
    """Adds c["clone"]: None, or {"after_step": index into c["steps"], "pairs" / "bands" / "water0_on_demand": the second handle's own
    options, "used": whether the second handle holds another state before the copy}. No draw from the case's generator."""
    r = np.random.default_rng([int(c["data_seed"]) & 0x7FFFFFFF, 0xC10E])
    c["clone"] = None
    if r.random() < 0.5:
        c["clone"] = {"after_step": int(r.integers(0, len(c["steps"]))), "pairs": int(r.random() < 0.7), "bands": int(r.choice([0, 1, 2])),
                      "water0_on_demand": int(r.random() < 0.7), "used": bool(r.random() < 0.5)}
    return c


# The sun at an EXACT slider position: draw_case takes the angle from a continuum, which never hits GUI 0, 90 or 180 -- the positions at which
# sinf / cosf of the uniform are exactly +-1 or 0 and the bilinear tap of the lighting pass changes its columns (x + 1, x + 2 at GUI 180) and rows
# (y + 1, y + 2 at GUI 90); tests/light_scenes.py has the classes. Drawn like draw_more_sliders, as a function of the case (recipe key
# "sun_exact"; recipes without it run as they always did). The case keeps its drawn sun for the first step, which lets light in where that sun
# is up, and takes the exact position -- the angle alone, sunIntensity stays the drawn sun's: at GUI 0 and 180 it would be 0 -- from the second
# step on; a case of one step gets a second one.
SUN_EXACT = (-10.0, 0.0, 90.0, 180.0, 190.0, 90.0 - 1e-6, 90.0 + 1e-6, 180.0 - 1e-6, 180.0 + 1e-6)


def draw_sun_exact(c):
    """Adds c["sun_exact"] (degrees, one of SUN_EXACT). No draw from the case's generator."""
    r = np.random.default_rng([int(c["data_seed"]) & 0x7FFFFFFF, 0x50A])
    c["sun_exact"] = float(SUN_EXACT[int(r.integers(0, len(SUN_EXACT)))])
    if len(c["steps"]) == 1:
        c["steps"] = c["steps"] + [int(r.integers(1, 12))]
    return c


def sun_exact_uniforms(pkg, c, u, k_step):
    """``u`` with the exact angle from the case's second step on (None: nothing changes at this step)."""
    if c.get("sun_exact") is None or k_step != 1:
        return None
    return dict(u, sunAngle=float(np.float32(pkg.params.sun_from_angle(c["sun_exact"], 1.0)[0])))


CLONE_FIELDS = ["BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1", "CURL", "PRECIP_FB", "PRECIP_DEP", "LIGHTNING", "EMITTED"]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def compare_clone(h2, h, nd, done):
    """Mismatches between a clone and the handle it was copied from, after the same calls."""
    bad = [{"field": "clone:" + f, "after_iterations": done} for f in CLONE_FIELDS if not _same_bits(h2.read_rect(f), h.read_rect(f))]
    if nd and not _same_bits(h2.read_particles(), h.read_particles()):
        bad.append({"field": "clone:DROPS", "after_iterations": done})
    if h2.iter != h.iter:
        bad.append({"field": "clone:iter", "after_iterations": done})
    return bad


def case_iter0(c):
    it0 = (c.get("surface") or {}).get("iter0")
    return c["iter0"] if it0 is None else it0


def paint_surface(c, base, water, wall):
    """The stretches of c["surface"] on the LAND columns of a terrain: type up the whole column, vegetation / soil moisture / snow in its wall cells."""
    X = wall.shape[1]
    for start, width, t, veg, soil, snow in (c.get("surface") or {}).get("stretches", []):
        for x in (int(start * X) + np.arange(max(1, int(width * X)))) % X:
            if wall[0, x, 0] != 1:
                continue
            rows = wall[:, x, 1] == 0
            wall[:, x, 0] = t
            wall[rows, x, 3] = veg
            water[rows, x, 2] = soil
            water[rows, x, 3] = snow


def draw_case(rng, max_cells, big=False):
    c = {}
    kind = rng.choice(["tiny", "small", "small", "mid", "wide", "tall"])
    if big:  # (--big: the launch shapes of grids that fill the chip -- row bands per XCD, several rounds of segments, tail segments)
        X, Y = int(rng.integers(1000, 9000)), int(rng.integers(512, 2100))
    elif kind == "tiny":
        X, Y = int(rng.integers(2, 70)), int(rng.integers(4, 40))
    elif kind == "small":
        X, Y = int(rng.integers(40, 400)), int(rng.integers(12, 200))
    elif kind == "mid":
        X, Y = int(rng.integers(300, 1500)), int(rng.integers(100, 700))
    elif kind == "wide":
        X, Y = int(rng.integers(1500, 6000)), int(rng.integers(12, 120))
    else:
        X, Y = int(rng.integers(20, 200)), int(rng.integers(500, 1500))
    if rng.random() < 0.3:  # borders of strips (56 output columns), pair strips (48), tiles (64 x 16)
        X = max(2, int(rng.choice([56, 48, 64, 112, 96, 128, 168, 448])) * int(rng.integers(1, 4)) + int(rng.integers(-1, 2)))
    while X * Y > max_cells:
        X, Y = max(2, X // 2), max(4, Y * 3 // 4)
    c["X"], c["Y"] = X, Y
    c["dry"] = bool(rng.random() < 0.35)
    c["terrain"] = bool(Y >= 12 and rng.random() < (0.4 if c["dry"] else 0.9))
    c["tseed"], c["tmult"] = float(rng.random()), float(rng.uniform(0.05, 0.6))
    c["sigma"] = float(rng.choice([0.0, 0.05, 0.2, 0.35, 0.6, 1.2]) if c["dry"] else rng.choice([0.0, 0.05, 0.1, 0.2, 0.3, 0.45]))
    c["vortices"] = int(rng.integers(0, 4)) if rng.random() < 0.4 else 0
    c["moist"] = bool(rng.random() < 0.6)
    c["cloud"], c["smoke"], c["snow"] = bool(rng.random() < 0.4), bool(rng.random() < 0.3), bool(rng.random() < 0.3)
    c["sliders"] = {k: float(rng.uniform(*SLIDERS[k])) for k in SLIDERS if rng.random() < 0.35}
    c["sun"] = float(rng.uniform(-30.0, 210.0))
    c["wrap"] = bool(rng.random() < 0.85)
    c["quad_scale"] = int(rng.random() < 0.2)
    c["iter0"] = int(rng.choice([0, 1, 90, 599, 12345]))
    c["steps"] = [int(v) for v in rng.integers(1, 12, size=int(rng.integers(1, 4)))]
    c["brush"] = None
    if rng.random() < 0.3:
        c["brush"] = {"type": int(rng.integers(0, 24)), "values": [float(rng.random()), float(rng.random()), float(rng.uniform(-1, 1)), float(rng.uniform(1, 30))],
                      "move": [float(rng.uniform(-0.02, 0.02)), float(rng.uniform(-0.02, 0.02))]}
    c["airplane"] = [float(rng.random()), float(rng.random()), float(rng.random()), float(rng.choice([-1.0, 0.0, 1.0]))] if rng.random() < 0.15 else None
    c["drops"] = int(rng.integers(16, 3000)) if (not c["dry"] and Y >= 24 and rng.random() < 0.3) else 0
    c["pairs"] = int(rng.random() < 0.7)
    c["bands"] = int(rng.choice([0, 1, 1, 2]))
    c["kernel_set"] = int(rng.random() < 0.85)  # 1 = the row-marching kernels (default), 0 = one kernel per reference pass
    c["dry_kernel"] = int(rng.random() < 0.8)  # the dry stencil: row-marching (default) / LDS-tiled
    c["water0_on_demand"] = int(rng.random() < 0.7)
    c["data_seed"] = int(rng.integers(0, 2**31))
    c["brush_toggle"] = bool(rng.random() < 0.5)  # the brush is held down in every other step only (a host's mouse-up / mouse-down between frames)
    c["pieces"] = bool(rng.random() < 0.3)  # steps cut into two pieces, the first with WX_OVERLAP_MORE_TO_COME
    c["reupload"] = bool(rng.random() < 0.2)  # after the first step the current state is uploaded again (a host that edits the state: new ping-pong copies, on slabs a fresh exchange period and |vx| scan)
    c["subrect"] = bool(rng.random() < 0.3)  # also read a random sub-rectangle of every field (wx_read_rect's x / y / w / h)
    return c


def build_case(pkg, c):
    S, P = pkg.synth, pkg.params
    X, Y = c["X"], c["Y"]
    rng = np.random.default_rng(c["data_seed"])
    if c["terrain"]:
        base, water, wall = S.terrain_grid(X, Y, seed=c["tseed"], height_mult=c["tmult"])
    else:
        base, water, wall = S.dry_grid(X, Y)
    paint_surface(c, base, water, wall)
    air = wall[..., 1] != 0
    if c["sigma"] > 0:
        for ch in (0, 1):
            base[..., ch] += np.where(air, rng.normal(0, c["sigma"], (Y, X)), 0).astype(np.float32)
    if c["vortices"]:
        cs = [(float(rng.uniform(0, X)), float(rng.uniform(Y * 0.2, Y * 0.9))) for _ in range(c["vortices"])]
        S.add_vortices(base, wall, cs, radius=float(rng.uniform(3, 12)), peak=float(rng.uniform(0.8, 2.5)))
    base[..., 2] += np.where(air, rng.normal(0, 1e-3, (Y, X)), 0).astype(np.float32)
    base[..., 3] += np.where(air, rng.normal(0, 0.3, (Y, X)), 0).astype(np.float32)
    if c["moist"]:
        water[..., 0] = np.where(air, water[..., 0] * (1.0 + 0.5 * rng.random((Y, X))) + rng.random((Y, X)) * (2.0 if not c["terrain"] else 0.0), water[..., 0]).astype(np.float32)
    if c["cloud"]:
        blob = air & (rng.random((Y, X)) < 0.2)
        water[..., 1] += np.where(blob, rng.random((Y, X)) * 2.0, 0).astype(np.float32)
        water[..., 0] += np.where(blob, water[..., 1], 0).astype(np.float32)
    if c["smoke"]:
        water[..., 3] += np.where(air & (rng.random((Y, X)) < 0.1), rng.random((Y, X)) * 3.0, 0).astype(np.float32)
    if c["snow"]:
        water[..., 2] += np.where(air & (rng.random((Y, X)) < 0.1), rng.random((Y, X)) * 0.5, 0).astype(np.float32)
    gui = P.merge_settings(None)
    gui.update(c["sliders"])
    gui.update(c.get("sliders_more", {}))
    gui["sunAngle"] = c["sun"]
    gui["wrapHorizontally"] = c["wrap"]
    u = P.uniforms_from_gui(gui, Y, quad_scale=c["quad_scale"], pass_mask=P.PASS_DRY if c["dry"] else P.PASS_ALL)
    u["enablePrecipitation"] = 1 if c["drops"] else 0
    if c["brush"]:
        u["userInputType"] = c["brush"]["type"]
        u["userInputValues"] = tuple(c["brush"]["values"])
        u["userInputMove"] = tuple(c["brush"]["move"])
    if c["airplane"]:
        u["airplaneValues"] = tuple(c["airplane"])
    drops = None
    if c["drops"]:
        drops = S.init_rain_drops(c["drops"], seed=c["data_seed"] % 1000)
        u["splat_order"] = 1
        u["spawnChanceMult"] = 0.01
    return base, water, wall, u, drops


def run_case(pkg, E, wx_oracle, c):
    """One case on its own."""
    g = case_steps(pkg, E, wx_oracle, c)
    while True:
        try:
            next(g)
        except StopIteration as e:
            return e.value


def run_interleaved(pkg, E, wx_oracle, cases):
    """Several handles alive at once, their steps in turn (state that a handle shares with the process -- work lists, hint words, scratch
    sized by another handle -- would show here). Returns the (bad, info) of every case."""
    gens = [case_steps(pkg, E, wx_oracle, c) for c in cases]
    out = [None] * len(gens)
    while any(o is None for o in out):
        for i, g in enumerate(gens):
            if out[i] is None:
                try:
                    next(g)
                except StopIteration as e:
                    out[i] = e.value
    return out


def case_steps(pkg, E, wx_oracle, c):
    """Generator: yields after every step of the case; its return value is (mismatches, info)."""
    X, Y = c["X"], c["Y"]
    base, water, wall, u, drops = build_case(pkg, c)
    nd = 0 if drops is None else len(drops)
    h = E.Handle(X, Y, nd)
    o = wx_oracle.OracleSim(X, Y, nd)
    bad = []
    cl, h2 = c.get("clone"), None
    try:
        h.upload(base, water, wall, drops)
        o.upload(base, water, wall, drops)
        h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
        o.set_params(u)
        h.iter = case_iter0(c)
        o.iter = case_iter0(c)
        h.set_option(h.OPT_DRY_PAIRS, c["pairs"])
        h.set_option(h.OPT_ROW_BANDS, c["bands"])
        h.set_option(h.OPT_KERNEL_SET, c["kernel_set"])
        h.set_option(h.OPT_DRY_KERNEL, c["dry_kernel"])
        h.set_option(h.OPT_WATER0_ON_DEMAND, c["water0_on_demand"])
        if nd:
            h.set_option(h.OPT_SPLAT_ORDER, 1)
        rng = np.random.default_rng(c["data_seed"] ^ 0x5EED)
        for k_step, n in enumerate(c["steps"]):
            if sun_exact_uniforms(pkg, c, u, k_step) is not None:
                u = sun_exact_uniforms(pkg, c, u, k_step)
                for hh_ in (h, h2) if h2 is not None else (h,):
                    hh_.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
                o.set_params(u)
            if c.get("brush_toggle") and c["brush"] and k_step > 0:  # mouse up / down between two steps: new parameters on both sides
                u2 = dict(u, userInputType=(c["brush"]["type"] if k_step % 2 == 0 else -1))
                for hh_ in (h, h2) if h2 is not None else (h,):  # (a clone is given every call its source is given)
                    hh_.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u2), u["initial_T"])
                o.set_params(u2)
            if c.get("reupload") and k_step == 1 and not nd:
                st = [o.field(f) for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR")]
                for hh_ in (h, h2) if h2 is not None else (h,):
                    hh_.upload(*st)
                o.upload(*st)
            pieces = [n]
            if c.get("pieces") and n > 1:  # the step cut into pieces whose all but the last skip the display-side stores (WX_OVERLAP_MORE_TO_COME)
                k1 = int(rng.integers(1, n))
                pieces = [k1, n - k1]
            for i_p, k_p in enumerate(pieces):
                h.step(k_p, 4 if i_p + 1 < len(pieces) else 0)
                if h2 is not None:
                    h2.step(k_p, 4 if i_p + 1 < len(pieces) else 0)
            o.step(n)
            yield
            if h2 is not None:
                bad += compare_clone(h2, h, nd, h.iter - case_iter0(c))
            if cl and k_step == cl["after_step"] and h2 is None:  # the clone: a second handle under its own options, possibly holding an older state
                h2 = E.Handle(X, Y, nd)
                h2.set_option(h2.OPT_DRY_PAIRS, cl["pairs"])
                h2.set_option(h2.OPT_ROW_BANDS, cl["bands"])
                h2.set_option(h2.OPT_WATER0_ON_DEMAND, cl["water0_on_demand"])
                h2.set_option(h2.OPT_KERNEL_SET, c["kernel_set"])  # (VORT and the dry kernels' stale fields differ between the kernel sets: the same one)
                h2.set_option(h2.OPT_DRY_KERNEL, c["dry_kernel"])
                if nd:
                    h2.set_option(h2.OPT_SPLAT_ORDER, 1)
                if cl["used"]:
                    h2.upload(base, water, wall, drops)
                    h2.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
                    h2.step(3)
                h2.copy_from(h)
                bad += compare_clone(h2, h, nd, h.iter - case_iter0(c))
            if not c["dry"] and not np.array_equal(h.read_rect("CURL"), o.field("CURL"), equal_nan=True):
                bad.append({"field": "CURL", "after_iterations": h.iter - case_iter0(c)})
            if c.get("subrect"):
                x0, y0 = int(rng.integers(0, X)), int(rng.integers(0, Y))
                w, hh = int(rng.integers(1, X - x0 + 1)), int(rng.integers(1, Y - y0 + 1))
                for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR") + (() if c["dry"] else ("LIGHT_1", "BASE_DISP")):
                    a, b = h.read_rect(f, x0, y0, w, hh), o.field(f)[y0:y0 + hh, x0:x0 + w]
                    if not np.array_equal(a, b, equal_nan=True):
                        bad.append({"field": f + " sub-rectangle", "rect": [x0, y0, w, hh], "after_iterations": h.iter - case_iter0(c)})
            fields = list(GRID_FIELDS if not c["dry"] else ["BASE_CUR", "BASE_DISP", "WATER_CUR", "WATER_0", "WALL_CUR"])
            for f in fields:
                a, b = h.read_rect(f), o.field(f)
                if not np.array_equal(a, b, equal_nan=True):
                    ne = (a != b) & ~(np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)))
                    ys, xs = np.nonzero(ne.any(axis=-1))
                    bad.append({"field": f, "after_iterations": h.iter - case_iter0(c), "values": int(ne.sum()), "first": [int(xs[0]), int(ys[0])],
                                "max_abs": float(np.nanmax(np.abs(a.astype(np.float64) - b)))})
            if nd:
                for f, a, b in (("DROPS", h.read_particles(), o.field("DROPS")), ("PRECIP_FB", h.read_rect("PRECIP_FB"), o.field("PRECIP_FB")),
                                ("PRECIP_DEP", h.read_rect("PRECIP_DEP"), o.field("PRECIP_DEP")), ("LIGHTNING", h.read_rect("LIGHTNING"), o.field("LIGHTNING"))):
                    if not np.array_equal(a, b, equal_nan=True):
                        bad.append({"field": f, "after_iterations": h.iter - case_iter0(c), "values": int((a != b).sum())})
            if bad:
                break
        info = {"blown_up": not bool(np.isfinite(o.field("BASE_CUR")).all() and np.isfinite(o.field("WATER_CUR")).all() and np.abs(o.field("BASE_CUR")[..., :2]).max() < 1e4), "fastest": float(h.fastest_velocity()) if hasattr(h, "fastest_velocity") else None}
        try:
            info["pair_stats"] = h.pair_stats() if c["dry"] and c["pairs"] else None
        except Exception:
            info["pair_stats"] = None
    except E.WxError as e:  # an overflow of the exact path's list is REPORTED (a blown-up state), not a mismatch
        return [], {"error": str(e)}
    finally:
        h.close()
        o.close()
        if h2 is not None:
            h2.close()
    return bad, info


# ---- --mode script: the HOST's call sequence is drawn too (everything above draws the scene and runs one fixed script) ----
SCRIPT_FIELDS = ["BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "WALL_CUR:i32", "WALL_DISP:i32", "LIGHT_0", "LIGHT_1", "CURL", "VORT",
                 "PRECIP_FB", "PRECIP_DEP", "LIGHTNING", "EMITTED"]
SCRIPT_OPTIONS = ["KERNEL_SET", "DRY_KERNEL", "DRY_PAIRS", "ROW_BANDS", "WATER0_ON_DEMAND", "CHECK_LAUNCHES", "SPLAT_ORDER"]
# the action kinds a script is made of (run_script_case counts every one it performs, under these names)
SCRIPT_ACTIONS = ["read", "particles", "stream", "option", "params", "iter", "tune", "devwrite", "reupload", "pair_stats", "fastest", "water_free", "sync",
                  "profile", "lightning", "step0", "pieces"]
EXPECTED_ERROR = "the exact path holds"  # the one WxError a drawn scene may run into (a blown-up flow overflows the exact path's list): reported, nothing to compare


def _draw_rect(rng, X, Y):
    x0, y0 = int(rng.integers(0, X)), int(rng.integers(0, Y))
    return [x0, y0, int(rng.integers(1, X - x0 + 1)), int(rng.integers(1, Y - y0 + 1))]


def _draw_reads(rng, c):
    """A random subset (possibly empty) of the readable fields in random order; each whole or a sub-rectangle, some twice in a row."""
    names = [SCRIPT_FIELDS[i] for i in rng.permutation(len(SCRIPT_FIELDS))[:int(rng.integers(0, len(SCRIPT_FIELDS) + 1))]]
    return [{"field": f, "rect": _draw_rect(rng, c["X"], c["Y"]) if rng.random() < 0.3 else None, "twice": bool(rng.random() < 0.15)} for f in names]


def _draw_action(rng, c, kind):
    a = {"op": kind}
    if kind == "read":
        a["reads"] = _draw_reads(rng, c)
    elif kind == "particles":
        first = int(rng.integers(0, max(1, c["drops"])))
        a.update(first=first, count=int(rng.integers(0, max(1, c["drops"] - first + 1))))
    elif kind == "stream":
        a["rect"] = _draw_rect(rng, c["X"], c["Y"])
    elif kind == "option":
        o = str(rng.choice(SCRIPT_OPTIONS))
        a.update(opt=o, value=int(rng.integers(0, 3)) if o == "ROW_BANDS" else (1 if o == "SPLAT_ORDER" else int(rng.integers(0, 2))))
    elif kind == "params":  # the changes are applied, in this order, to the parameters in force (see _script_uniforms)
        ch = {}
        what = rng.choice(["sliders", "sun", "lapse", "brush", "airplane", "mask", "precip", "wrap"], size=int(rng.integers(1, 4)), replace=False)
        for w in what:
            if w == "sliders":
                ch["sliders"] = {k: float(rng.uniform(*SLIDERS[k])) for k in SLIDERS if rng.random() < 0.25}
                ch["sliders"].update(_draw_more([c["data_seed"], 0x5C2, sum(ch["sliders"].values()) * 1e9], 0.25))
            elif w == "sun":
                ch["sun"] = float(rng.uniform(-30.0, 210.0))
            elif w == "lapse":  # another initial_T row
                ch["lapse"] = float(rng.uniform(6.0, 11.0))
            elif w == "brush":
                ch["brush"] = None if rng.random() < 0.5 else {"type": int(rng.integers(0, 24)), "values": [float(rng.random()), float(rng.random()), float(rng.uniform(-1, 1)), float(rng.uniform(1, 30))],
                                                                "move": [float(rng.uniform(-0.02, 0.02)), float(rng.uniform(-0.02, 0.02))]}
            elif w == "airplane":
                ch["airplane"] = None if rng.random() < 0.5 else [float(rng.random()), float(rng.random()), float(rng.random()), float(rng.choice([-1.0, 0.0, 1.0]))]
            elif w == "mask":
                ch["dry"] = bool(rng.random() < 0.5)
            elif w == "precip":
                ch["precip"] = int(rng.random() < 0.5)
            else:
                ch["wrap"] = bool(rng.random() < 0.7)
        a["change"] = ch
    elif kind == "iter":  # on and next to the boundary pass's % 20 / % 100 schedules and the % 600 of the droplets, odd and even
        a["value"] = int(rng.choice([20, 100, 600, 1200, 12340]) * int(rng.integers(1, 4)) + int(rng.integers(-2, 3)))
    elif kind == "tune":
        a.update(tries=int(rng.integers(1, 3)), iters=int(rng.integers(1, 4)))
    elif kind == "devwrite":
        a.update(how=str(rng.choice(["eddies", "noise", "vortices", "scale"])), sigma=float(rng.choice([0.05, 0.2, 0.5])), seed=int(rng.integers(1, 1000)))
    elif kind == "profile":
        a["on"] = bool(rng.random() < 0.6)
    elif kind == "lightning":
        a["v"] = [float(rng.random()), float(rng.random()), float(rng.integers(0, 2000)), float(rng.random())]
    return a


def draw_script(rng, c):
    """The host script of --mode script for the case ``c`` of draw_case: 2 .. 5 steps and, in front of each and after the last, a random
    list of host actions (SCRIPT_ACTIONS). ``rng`` is a generator of ITS OWN, not draw_case's: the scene sequence of a seed is the same
    in every mode. The script becomes part of the recipe (c["script"]); run_script_case reads everything after the last step by itself."""
    kinds = [k for k in SCRIPT_ACTIONS if k != "pieces" and (c["drops"] or k != "particles")]
    weight = {"read": 6.0, "option": 3.0, "params": 3.0, "stream": 1.5, "iter": 1.5, "tune": 0.7, "devwrite": 1.0, "reupload": 0.7, "particles": 4.0}
    p = np.array([weight.get(k, 1.0) for k in kinds])
    script = []
    n_steps = int(rng.integers(2, 6))
    for k in range(n_steps + 1):
        for kind in rng.choice(kinds, size=int(rng.integers(0, 5)), p=p / p.sum()):
            script.append(_draw_action(rng, c, str(kind)))
        if k < n_steps:
            n = int(rng.integers(1, 9))
            script.append({"op": "step", "n": n, "first_piece": int(rng.integers(1, n)) if n > 1 and rng.random() < 0.3 else 0})
    c["script"] = script
    c["steps"] = [a["n"] for a in script if a["op"] == "step"]
    return c


def _script_uniforms(pkg, c, st):
    """The uniforms of the parameters in force: build_case's, with what the script's "params" actions changed since (``st``)."""
    P = pkg.params
    gui = P.merge_settings(None)
    gui.update(st["sliders"])
    gui["sunAngle"] = st["sun"]
    gui["wrapHorizontally"] = st["wrap"]
    if st["lapse"] is not None:
        gui["dryLapseRate"] = st["lapse"]
    u = P.uniforms_from_gui(gui, c["Y"], quad_scale=c["quad_scale"], pass_mask=P.PASS_DRY if st["dry"] else P.PASS_ALL)
    u["enablePrecipitation"] = 1 if (c["drops"] and st["precip"]) else 0
    if st["brush"]:
        u["userInputType"] = st["brush"]["type"]
        u["userInputValues"] = tuple(st["brush"]["values"])
        u["userInputMove"] = tuple(st["brush"]["move"])
    if st["airplane"]:
        u["airplaneValues"] = tuple(st["airplane"])
    if c["drops"]:
        u["splat_order"] = 1
        u["spawnChanceMult"] = 0.01
    return u


def _diff(field, a, b, it):
    ne = (a != b) & ~(np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)))
    idx = np.argwhere(ne)
    return {"field": field, "after_iterations": it, "values": int(ne.sum()), "first": [int(v) for v in idx[0][::-1]] if len(idx) else None}


def run_script_case(pkg, E, wx_oracle, c):
    """--mode script: one handle against the oracle through the host script c["script"] (draw_script). Returns (mismatches, info);
    info["actions"] counts the actions performed per kind, info["reads"] the field comparisons made. A WxError other than the exact
    path's reported overflow is NOT expected: it propagates (the caller stops the run there)."""
    X, Y = c["X"], c["Y"]
    base, water, wall, u, drops = build_case(pkg, c)
    nd = 0 if drops is None else len(drops)
    st = {"sliders": dict(c["sliders"], **c.get("sliders_more", {})), "sun": c["sun"], "wrap": c["wrap"], "lapse": None, "dry": c["dry"], "precip": 1, "brush": c["brush"], "airplane": c["airplane"]}
    u = _script_uniforms(pkg, c, st)
    h = E.Handle(X, Y, nd)
    o = wx_oracle.OracleSim(X, Y, nd)
    bad, count, n_reads = [], {k: 0 for k in SCRIPT_ACTIONS}, 0
    # what the LAST step ran decides which display-side fields mean the same on both sides: curl / vorticity are stored by the
    # iterations that run those passes (vorticity by the per-pass kernels only), the emitted-light image is made from what the last
    # lighting pass sampled (include/wxsim.h: zero once an iteration without that pass has run)
    last = {"stepped": False, "all": False, "per_pass": False, "lit_ever": False}
    kernel_set = c["kernel_set"]

    iters_done = 0

    def done():
        return iters_done

    def expect(field, rect):
        """(handle's array, oracle's array) of a read, or None where the two sides are not defined alike right now."""
        name, _, dt = field.partition(":")
        if name == "VORT" and not (last["stepped"] and last["all"] and last["per_pass"]):
            return None
        if name == "CURL" and last["stepped"] and not last["all"]:
            return None
        if name == "EMITTED" and last["lit_ever"] and not last["all"]:
            return None
        if name == "LIGHTNING":
            return h.read_rect("LIGHTNING"), o.field("LIGHTNING")
        x0, y0, w, hh = rect if rect else (0, 0, X, Y)
        b = o.field(name)[y0:y0 + hh, x0:x0 + w]
        if name == "EMITTED":
            b = b.astype(np.float16)
        if dt:
            return h.read_rect(name, x0, y0, w, hh, int32=True), b.astype(np.int32)
        return h.read_rect(name, x0, y0, w, hh), b

    def compare(field, rect=None, why="read"):
        nonlocal n_reads
        ab = expect(field, rect)
        if ab is None:
            return
        n_reads += 1
        if ab[0].dtype != ab[1].dtype or not np.array_equal(ab[0], ab[1], equal_nan=True):
            bad.append(dict(_diff(field, ab[0], ab[1], done()), rect=rect, during=why))

    def compare_everything(why):
        for f in SCRIPT_FIELDS:
            compare(f, None, why)
        if nd and not np.array_equal(h.read_particles(), o.field("DROPS"), equal_nan=True):
            bad.append({"field": "DROPS", "after_iterations": done(), "during": why})

    def set_params():
        nonlocal u
        u = _script_uniforms(pkg, c, st)
        h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
        o.set_params(u)

    try:
        h.upload(base, water, wall, drops)
        o.upload(base, water, wall, drops)
        set_params()
        h.iter = o.iter = c["iter0"]
        for k, v in (("DRY_PAIRS", c["pairs"]), ("ROW_BANDS", c["bands"]), ("KERNEL_SET", c["kernel_set"]), ("DRY_KERNEL", c["dry_kernel"]), ("WATER0_ON_DEMAND", c["water0_on_demand"])):
            h.set_option(getattr(h, "OPT_" + k), v)
        if nd:
            h.set_option(h.OPT_SPLAT_ORDER, 1)
        for a in c["script"]:
            op = a["op"]
            if op == "step":
                n, k1 = a["n"], a.get("first_piece", 0)
                if k1:  # the step cut into two pieces, the first with WX_OVERLAP_MORE_TO_COME (its last iteration stores no display-side field)
                    h.step(k1, 4)
                    h.step(n - k1)
                    count["pieces"] += 1
                else:
                    h.step(n)
                o.step(n)
                iters_done += n
                last.update(stepped=True, all=not st["dry"], per_pass=not kernel_set)
                last["lit_ever"] = last["lit_ever"] or not st["dry"]
                if c.get("verify_steps"):  # (--override '{"verify_steps": true}': everything after every step -- narrows a mismatch down to the step it begins in)
                    compare_everything("step")
                    if bad:
                        break
                continue
            if op == "particles" and not nd:
                continue
            count[op] += 1
            if op == "read":
                for r in a["reads"]:
                    for _ in range(2 if r["twice"] else 1):
                        compare(r["field"], r["rect"])
            elif op == "particles":
                d, d_ref = h.read_particles(a["first"], a["count"]), o.field("DROPS")[a["first"]:a["first"] + a["count"]]
                if not np.array_equal(d, d_ref, equal_nan=True):
                    k = int(np.argwhere((d != d_ref) & ~(np.isnan(d) & np.isnan(d_ref)))[0][0])
                    bad.append({"field": "DROPS", "range": [a["first"], a["count"]], "after_iterations": done(), "first": a["first"] + k, "handle": d[k].tolist(), "oracle": d_ref[k].tolist(),
                                "whole_pool_equal": bool(np.array_equal(h.read_particles(), o.field("DROPS"), equal_nan=True))})
            elif op == "stream":  # the streamed frame of a viewport == wx_read_rect of the same fields (those are compared with the oracle elsewhere)
                x0, y0, w, hh = a["rect"]
                h.stream_frame(x0, y0, w, hh)
                fr = {k: v.copy() for k, v in h.stream_wait().items()}
                for f, v in fr.items():
                    if not np.array_equal(v, h.read_rect(f, x0, y0, w, hh), equal_nan=True):
                        bad.append({"field": f + " streamed", "rect": a["rect"], "after_iterations": done()})
            elif op == "option":
                if a["opt"] == "SPLAT_ORDER" and not nd:
                    continue
                h.set_option(getattr(h, "OPT_" + a["opt"]), a["value"])
                if a["opt"] == "KERNEL_SET":
                    kernel_set = a["value"]
            elif op == "params":
                st.update({k: (dict(st["sliders"], **v) if k == "sliders" else v) for k, v in a["change"].items()})
                set_params()
            elif op == "iter":
                h.iter = o.iter = a["value"]
            elif op == "tune":  # state, iteration counter, every field and the pair counters are what they were (the oracle never moved)
                h.pair_stats()
                it = h.iter
                h.tune_placement(a["tries"], a["iters"])
                if h.iter != it:
                    bad.append({"field": "iter", "during": "tune", "before": it, "after": h.iter})
                ps = h.pair_stats()
                if ps != (0, 0):
                    bad.append({"field": "pair_stats", "during": "tune", "after": list(ps)})
                if not np.array_equal(h.lightning(), o.field("LIGHTNING")):
                    bad.append({"field": "lightning()", "during": "tune"})
                compare_everything("tune")
            elif op == "devwrite":  # the host edits velocities in place on the device (wx_device_ptr); the oracle gets the same BASE_CUR
                D = importlib.import_module(pkg.__name__ + ".devtools")
                if a["how"] == "vortices" and X >= 48 and Y >= 48:
                    D.seed_vortices(h, 2, peak=1.0 + a["sigma"], radius=2.5, seed=a["seed"])
                elif a["how"] == "scale":
                    h.sync()
                    D.field_tensor(h, "BASE_CUR")[1:, :, :2] *= 0.5
                    D.torch.cuda.synchronize()
                else:
                    D.seed_flow(h, a["sigma"], seed=a["seed"], kind="noise" if a["how"] == "noise" else "eddies")
                o.view("BASE_CUR")[...] = h.read_rect("BASE_CUR")
                compare_everything("devwrite")
            elif op == "reupload":
                state = [o.field(f) for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR")] + ([o.field("DROPS")] if nd else [])
                h.upload(*state)
                o.upload(*state)
                last.update(stepped=False, all=False, per_pass=False, lit_ever=False)
            elif op == "pair_stats":
                h.pair_stats()
            elif op == "fastest":
                h.fastest_velocity()
            elif op == "water_free":
                h.water_free()
            elif op == "sync":
                h.sync()
            elif op == "profile":
                h.profile(a["on"])
                h.profile_read()
            elif op == "lightning":
                h.set_lightning(a["v"])
                o.set_lightning(a["v"])
            elif op == "step0":  # (a step of no iterations still prepares the kernel set's layout of the light textures)
                h.step(0)
            if bad:
                break
        if not bad:
            compare_everything("end")
        ob = o.field("BASE_CUR")
        info = {"blown_up": not bool(np.isfinite(ob).all() and np.isfinite(o.field("WATER_CUR")).all() and np.abs(ob[..., :2]).max() < 1e4), "fastest": float(h.fastest_velocity()),
                "actions": count, "reads": n_reads}
    except E.WxError as e:
        if EXPECTED_ERROR not in str(e):
            raise
        return [], {"error": str(e), "actions": count, "reads": n_reads}
    finally:
        h.close()
        o.close()
    return bad, info


def draw_group(rng, c):
    """Extra draws of --mode group (after draw_case, so the scene sequence of a seed is the same in both modes)."""
    n = int(rng.choice([2, 2, 3, 4, 4, 5, 6, 8]))
    if c["drops"]:  # wx_create_slab: with particles halo and owned width are multiples of 64 (splat tiles), owned + 2 halo <= X
        halo = 64
        xo = max(64 if n > 2 else 128, -(-c["X"] // n // 64) * 64)
    else:  # (a halo narrower than the flow's dependency cone is refused by the first step: reported, not a mismatch)
        lo = 6 if c["sigma"] <= 0.05 and not c["vortices"] else (12 if c["sigma"] <= 0.3 and not c["vortices"] else 24)
        halo = int(rng.choice([h for h in (6, 12, 18, 24, 42, 48, 64) if h >= lo]))
        xo = max(halo, -(-c["X"] // n))
    c["X"] = n * xo
    # ("split" chose between two forms of the split iteration while there were two. Still drawn and recorded, so that a seed's cases and
    # their recipes stay what they were; nothing applies it any more)
    c.update(nslab=n, halo=halo, overlap=int(rng.random() < 0.6), split=int(rng.random() < 0.25), pool_exact=1, kernel_set=int(rng.random() < 0.9))
    c["steps"] = [int(v) for v in rng.integers(1, 2 * max(1, halo // 6) + 3, size=int(rng.integers(1, 4)))]
    return c


def run_group_case(pkg, E, c):
    """N slabs on this one GPU (wx_group_*: the library's own halo exchange, device-to-device copies) against the undecomposed handle, bit
    for bit -- SURVEY 8e's determinism check on random scenes, slab counts, halo widths, call boundaries, overlap modes. (The "split" key of a
    recipe is from the time a split iteration had a second form: ignored.)"""
    X, Y = c["X"], c["Y"]
    base, water, wall, u, drops = build_case(pkg, c)
    nd = 0 if drops is None else len(drops)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    g = whole = None
    bad = []
    try:
        g = E.Group(c["nslab"], X, Y, halo=c["halo"], devices=[0] * c["nslab"], transport=E.TRANSPORT_LOCAL, n_droplets=nd)
        whole = E.Handle(X, Y, nd)
        g.upload(base, water, wall, drops)
        whole.upload(base, water, wall, drops)
        g.set_params(p, u["initial_T"])
        whole.set_params(p, u["initial_T"])
        for hh in g.slabs + [whole]:
            hh.iter = c["iter0"]
        opts = [(E.Handle.OPT_DRY_PAIRS, c["pairs"]), (E.Handle.OPT_ROW_BANDS, c["bands"]), (E.Handle.OPT_DRY_KERNEL, c["dry_kernel"]), (E.Handle.OPT_KERNEL_SET, c["kernel_set"])]
        if nd:
            opts.append((E.Handle.OPT_SPLAT_ORDER, 1))
        for k, v in opts:
            g.set_option(k, v)
            whole.set_option(k, v)
        g.set_option(E.Handle.OPT_EXCHANGE_OVERLAP, c["overlap"])
        if nd:
            g.set_option(E.Handle.OPT_POOL_EXACT, c["pool_exact"])
        fields = ["BASE_CUR", "WATER_CUR", "WALL_CUR"] + ([] if c["dry"] else ["LIGHT_0", "LIGHT_1", "BASE_DISP", "WATER_0"]) + (["PRECIP_DEP"] if nd else [])
        done = 0
        for k_step, n in enumerate(c["steps"]):
            if c.get("reupload") and k_step == 1 and not nd:
                st = [whole.read_rect(f) for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR")]
                g.upload(*st)
                whole.upload(*st)
            if sun_exact_uniforms(pkg, c, u, k_step) is not None:
                u = sun_exact_uniforms(pkg, c, u, k_step)
                p = pkg.params.fill_struct(pkg.params.WxParams(), u)
                g.set_params(p, u["initial_T"])
                whole.set_params(p, u["initial_T"])
            if c.get("brush_toggle") and c["brush"] and k_step > 0:  # mouse up / down between two steps
                u2 = dict(u, userInputType=(c["brush"]["type"] if k_step % 2 == 0 else -1))
                p2 = pkg.params.fill_struct(pkg.params.WxParams(), u2)
                g.set_params(p2, u["initial_T"])
                whole.set_params(p2, u["initial_T"])
            g.step(n)
            whole.step(n)
            done += n
            for f in fields:
                a, b = g.read(f), whole.read_rect(f)
                if not np.array_equal(a, b, equal_nan=True):
                    ne = (a != b) & ~(np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)))
                    ys, xs = np.nonzero(ne.any(axis=-1))
                    bad.append({"field": f, "after_iterations": done, "values": int(ne.sum()), "first": [int(xs[0]), int(ys[0])]})
            if bad:
                break
        if nd and not bad:
            g.exchange()
            g.sync()
            d, d_ref = g.particles(), whole.read_particles()
            if not np.array_equal(d, d_ref, equal_nan=True):
                bad.append({"field": "DROPS", "after_iterations": done, "values": int((d != d_ref).sum())})
        wb = whole.read_rect("BASE_CUR")
        info = {"blown_up": not bool(np.isfinite(wb).all() and np.abs(wb[..., :2]).max() < 1e4), "fastest": float(np.abs(wb[..., :2]).max())}
    except E.WxError as e:  # reported: the exact path's list overflowed / a slab outran the |vx| bound its period was sized for (a blown-up state)
        return [], {"error": str(e)}
    finally:
        if g is not None:
            g.close()
        if whole is not None:
            whole.close()
    return bad, info


def run_setup_case(pkg, E, c):
    """--mode setup: the device-side initialisers (wx_setup_columns from 1-D descriptors, wx_setup_terrain with the shader's terrain noise on
    the device, wx_init_droplets) against the host generator + wx_upload: bit-identical textures (setup_terrain: all but the handful of
    columns whose height sits on a row boundary in the last bit of sin()), and the same run afterwards."""
    S = pkg.synth
    X, Y = c["X"], max(16, c["Y"])  # (wx_setup_terrain: at least 16 rows)
    snap = int([1, 2, 4][c["data_seed"] % 3])
    cloud = bool(c["cloud"])
    desc = S.terrain_columns(X, Y, seed=c["tseed"], height_mult=c["tmult"], snap=snap, cloud_deck=cloud)
    base, water, wall = S.terrain_grid(X, Y, seed=c["tseed"], height_mult=c["tmult"], snap=snap)
    if cloud:
        S.add_cloud_deck(water, wall)
    gui = pkg.params.merge_settings(None)
    gui["sunAngle"] = c["sun"]
    u = pkg.params.uniforms_from_gui(gui, Y, quad_scale=0)
    u["enablePrecipitation"] = 0
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    a, b, t = E.Handle(X, Y, 0), E.Handle(X, Y, 0), E.Handle(X, Y, 0)
    bad = []
    try:
        a.upload(base, water, wall)
        b.setup_columns(desc)
        t.setup_terrain(S.sounding_rows(Y, cloud_deck=cloud), seed=c["tseed"], height_mult=c["tmult"], snap=snap, sim_height=float(gui["simHeight"]))
        for hh in (a, b):
            hh.set_params(p, u["initial_T"])
        terr = np.zeros(X, bool)
        for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR"):
            terr |= (b.read_rect(f) != t.read_rect(f)).any(axis=(0, 2))
        if terr.sum() > max(4, X // 200):
            bad.append({"field": "terrain", "what": "setup_terrain vs setup_columns: %d of %d columns differ" % (int(terr.sum()), X)})
        for when in ("after setup", "after 5 iterations"):
            for f in ("BASE_CUR", "WATER_CUR", "WATER_0", "WALL_CUR", "LIGHT_0"):
                if not np.array_equal(a.read_rect(f), b.read_rect(f)):
                    bad.append({"field": f, "what": "setup_columns vs upload, " + when})
            if bad:
                break
            a.step(5)
            b.step(5)
        info = {"blown_up": False, "fastest": 0.0, "terrain_columns_differing": int(terr.sum())}
    except E.WxError as e:
        return [], {"error": str(e)}
    finally:
        for hh in (a, b, t):
            hh.close()
    return bad, info


# ---- --mode impulse: the impulse-lattice scenes of tests/impulse_scenes.py (lone single-cell triggers at every kernel phase) ----
# configuration name -> how the case is run: the dry stencil's pass mask, handle options, the iterations of each step, steps cut into
# WX_OVERLAP_MORE_TO_COME pieces
IMPULSE_CONFIGS = {
    # steps (1, 1, 3): the planted trigger meets the DISPLAY iteration (the last one of a step); (3, 2): a plain iteration; pieces: every
    # step is cut into a first iteration with WX_OVERLAP_MORE_TO_COME and the rest, so the trigger meets a piece that skips the display stores
    "wet": {}, "wet_plain": {"steps": (3, 2)}, "wet_stored": {"water0_on_demand": 0}, "wet_pieces": {"steps": (3, 2), "pieces": True}, "perpass": {"kernel_set": 0},
    "wet_bands0": {"bands": 0}, "wet_bands1": {"bands": 1}, "wet_bands2": {"bands": 2},
    "dry_single": {"dry": True, "pairs": 0}, "dry_single_plain": {"dry": True, "pairs": 0, "steps": (3, 2)}, "dry_perpass": {"dry": True, "kernel_set": 0},
    # pairs: iterations 1-2 and 3-4 are pairs, 5 runs the one-iteration kernel. A fresh handle's hint word starts at 1, so its first
    # pair runs the TAINT instantiation (launch_march_dry2), and so does the second while the first left entries. "prime": a quiet pair
    # on the background first -- its empty post pass sets the hint to 0 -- then the scene is uploaded into the SAME handle: the trigger
    # meets the PLAIN instantiation (first-iteration fast cells inline through global memory, second-iteration ones recorded lane by lane)
    "dry_pairs": {"dry": True, "pairs": 1, "steps": (2, 2, 1)}, "dry_pairs_plain": {"dry": True, "pairs": 1, "steps": (2, 2, 1), "prime": True},
    "dry_pairs_bands0": {"dry": True, "pairs": 1, "steps": (2, 2, 1), "bands": 0}, "dry_pairs_bands1": {"dry": True, "pairs": 1, "steps": (2, 2, 1), "bands": 1},
    "dry_pairs_bands2": {"dry": True, "pairs": 1, "steps": (2, 2, 1), "bands": 2},
    # droplets in the DEFAULT splat order (fp32 atomics): with lone sprites every texel receives one deposit -- order-free, so bit for bit
    "splat_atomic": {"splat_order": 0}, "splat_atomic_perpass": {"splat_order": 0, "kernel_set": 0},
}


def impulse_module():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    return importlib.import_module("impulse_scenes")


def draw_impulse(rng, I):
    """A generator of its own (draw_case and the pinned digests of its sequences are untouched): grid, kind, pitch, offset, configuration."""
    X = int(rng.choice([56, 60, 64, 112, 120, 448]) * int(rng.integers(2, 12)) + int(rng.integers(-2, 3))) if rng.random() < 0.5 else int(rng.integers(150, 3000))
    Y = int(rng.integers(24, 400))
    dry = bool(rng.random() < 0.4)
    kind = str(rng.choice(I.DRY_KINDS if dry else I.KINDS))
    pitch = list(I.DROPLET_PITCH) if kind == "droplet" else [int(rng.integers(I.MIN_DX + 1, 140)), int(rng.integers(I.MIN_DY + 1, 24))]
    cfgs = [k for k, v in IMPULSE_CONFIGS.items() if bool(v.get("dry")) == dry and (("splat_order" in v) == (kind == "droplet"))]
    return {"sweep": "drawn", "X": X, "Y": Y, "kind": kind, "pitch": pitch, "offset": [int(rng.integers(0, X)), int(rng.integers(0, pitch[1]))],
            "background": "air" if dry or rng.random() < 0.5 else "terrain", "config": str(rng.choice(cfgs))}


def run_impulse_case(pkg, E, wx_oracle, c, I=None):
    """One impulse-lattice case: the handle, configured as c["config"] says, against the oracle after every step -- every field both
    define, bit for bit; a mismatch names the nearest site and its phases. info: the sites, wx_fastest_velocity after the first step
    and what the oracle says it must be (wet marching kernel), wx_pair_stats, the launches of the pair kernel (profile counter) and the oracle's
    largest velocity in the first / second iterations of the pairs (the second always records tiles, the first while the TAINT instantiation runs), the iteration up to which the droplets' sprites stayed disjoint."""
    I = I or impulse_module()
    cfg = IMPULSE_CONFIGS[c["config"]]
    X, Y, kind, dry = c["X"], c["Y"], c["kind"], bool(cfg.get("dry"))
    base, water, wall, drops, sites = I.build_case(c)
    nd = 0 if drops is None else len(drops)
    u = I.scene_uniforms(kind, Y, dry=dry)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    h = E.Handle(X, Y, nd)
    o = wx_oracle.OracleSim(X, Y, nd)
    bad, info = [], {"sites": len(sites), "blown_up": False}
    try:
        marching = cfg.get("kernel_set", 1) == 1
        pairs = dry and marching and cfg.get("pairs", 1) == 1

        def options():
            h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
            h.set_option(h.OPT_DRY_KERNEL, 1)
            h.set_option(h.OPT_DRY_PAIRS, cfg.get("pairs", 1))
            h.set_option(h.OPT_ROW_BANDS, cfg.get("bands", 1))
            h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
            if nd:
                h.set_option(h.OPT_SPLAT_ORDER, cfg["splat_order"])

        if cfg.get("prime"):  # a quiet pair first: the handle hears of an empty exact-path list
            quiet = I.build_case(c, plant=False)
            h.upload(*quiet[:3])
            h.set_params(p, u["initial_T"])
            options()
            h.step(2)
            info["prime_pair_stats"] = h.pair_stats()  # (synchronises: the hint word is the host's to read at the next launch)
        h.upload(base, water, wall, drops)
        o.upload(base, water, wall, drops)
        h.set_params(p, u["initial_T"])
        o.set_params(u)
        h.iter = o.iter = 0
        options()
        if dry:
            info["water_free"] = h.water_free()
        if pairs:
            h.profile(True)
        if not dry and marching:  # what the exact path of the wet kernel must report after the first iteration: the largest post-boundary component
            t = wx_oracle.OracleSim(X, Y, 0)
            t.upload(base, water, wall)
            t.set_params(dict(u, pass_mask=7, enablePrecipitation=0))
            t.step(1)
            v = np.abs(t.field("BASE_CUR")[..., :2]).max()
            t.close()
            info["fastest_expected"] = float(v) if v >= np.float32(0.9) else 0.0
        fields = ["BASE_CUR", "BASE_DISP", "WATER_CUR", "WATER_0", "WALL_CUR"] if dry else list(GRID_FIELDS)
        done, v1, v2, exact = 0, 0.0, 0.0, True
        steps = cfg.get("steps", (1, 1, 3))
        for n in steps:
            if cfg.get("pieces") and n > 1:
                h.step(1, 4)
                h.step(n - 1)
            else:
                h.step(n)
            for k in range(n):
                before = o.field("DROPS") if nd else None
                in_pair = (k % 2 == 1) or (k + 1 < n)  # the host pairs iterations (0, 1), (2, 3) ... of a step; an odd one out runs alone
                if pairs and in_pair:  # the velocities the two iterations of a pair advect with
                    t = wx_oracle.OracleSim(X, Y, 0)
                    t.upload(o.field("BASE_CUR"), o.field("WATER_CUR"), o.field("WALL_CUR"))
                    t.set_params(dict(u, pass_mask=1))
                    t.step(1)
                    v = float(np.abs(t.field("BASE_CUR")[..., :2]).max())
                    v1, v2 = max(v1, v if k % 2 == 0 else 0.0), max(v2, v if k % 2 == 1 else 0.0)
                    t.close()
                o.step(1)
                if nd and exact and I.deposits_per_texel(before, o.field("DROPS"), X, Y) > 1:
                    exact = False
                    info["sprites_disjoint_until"] = done + k
            done += n
            if nd and not exact:  # two deposits in one texel: the atomic order decides the last bit from here on
                break
            for f in fields + (["PRECIP_FB", "PRECIP_DEP", "LIGHTNING"] if nd else []):
                a, b = h.read_rect(f), o.field(f)
                if not np.array_equal(a, b):
                    bad.append({"field": f, "after_iterations": done, "what": I.describe_difference(f, a, b, sites, X) if a.ndim == 3 else "differs"})
            if nd and not np.array_equal(h.read_particles(), o.field("DROPS")):
                bad.append({"field": "DROPS", "after_iterations": done})
            if done == steps[0] and not dry and marching:
                info["fastest"] = h.fastest_velocity()
            if bad:
                break
        if nd and exact:
            info["sprites_disjoint_until"] = done
        if pairs:
            info["pair_stats"], info["first_iteration_fastest"], info["second_iteration_fastest"] = h.pair_stats(), v1, v2
            info["first_iteration_fast"], info["second_iteration_fast"] = v1 >= 0.9, v2 >= 0.9
            info["pair_launches"] = h.profile_read().get("march_dry2_two_iterations_per_launch", (0.0, 0))[1]
        ob = o.field("BASE_CUR")
        info["blown_up"] = not bool(np.isfinite(ob).all() and np.abs(ob[..., :2]).max() < 1e4)
    finally:
        h.close()
        o.close()
    return bad, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=100000)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--max-cells", type=int, default=600000)
    ap.add_argument("--interleave", action="store_true", help="oracle mode: half of the cases run with a second handle alive, steps in turn")
    ap.add_argument("--big", action="store_true", help="grids of 1000-9000 x 512-2100 cells (use with --max-cells 8000000)")
    ap.add_argument("--mode", choices=["oracle", "group", "setup", "script", "impulse"], default="oracle",
                    help="oracle: one handle against the CPU oracle; group: N slabs against one handle; script: one handle against the oracle through a drawn host script")
    ap.add_argument("--only", type=int, default=-1, help="run only case K of the seed's sequence")
    ap.add_argument("--first", type=int, default=0, help="skip the cases before this one (they are still drawn: same sequence)")
    ap.add_argument("--last", type=int, default=1 << 30)
    ap.add_argument("--override", default="", help="JSON object merged into the recipe of every case that runs (bisecting a failure)")
    ap.add_argument("--sun-exact", action="store_true", help="oracle / group mode: draw_sun_exact on top of every case (the sun at an exact slider position from the second step on)")
    ap.add_argument("--check-launches", action="store_true", help="WX_OPT_CHECK_LAUNCHES 1: synchronise and check after every launch")
    a = ap.parse_args()
    pkg = wxpkg.load_package()
    E = pkg.engine
    E.lib().wx_set_option(None, E.Handle.OPT_PLACEMENT_SEARCH, 0)
    if a.check_launches:
        E.lib().wx_set_option(None, E.Handle.OPT_CHECK_LAUNCHES, 1)
    import wx_oracle
    wx_oracle.build()
    rng = np.random.default_rng(a.seed)
    rng_il = np.random.default_rng(a.seed + 1000003)  # (companions come from a sequence of their own: --seed S --only K still reproduces case K alone)
    rng_script = np.random.default_rng(a.seed + 2000003)  # (host scripts too: the scenes of --mode script are those of --mode oracle)
    totals = {k: 0 for k in SCRIPT_ACTIONS}
    t0 = time.time()
    failures, ran, reported, compared = [], 0, 0, 0
    if a.mode == "impulse":  # a generator, a loop and a summary of its own: draw_case's sequences are untouched
        I = impulse_module()
        n_bad = ran = 0
        for k in range(a.cases):
            c = draw_impulse(rng, I)
            if (a.only >= 0 and k != a.only) or k < a.first or c["X"] * c["Y"] > a.max_cells:
                continue
            if k > a.last or time.time() - t0 > a.seconds:
                break
            print(f"case {k} recipe: {json.dumps(c)}", flush=True)  # BEFORE it runs
            bad, info = run_impulse_case(pkg, E, wx_oracle, c, I)
            ran += 1
            n_bad += 1 if bad and not info["blown_up"] else 0
            print(f"case {k:4d} {c['X']:5d}x{c['Y']:<5d} {c['kind']:14s} {c['config']:20s} {json.dumps(info)}  {'MISMATCH ' + json.dumps(bad) if bad else 'ok'}", flush=True)
        print(json.dumps({"mode": a.mode, "seed": a.seed, "cases_run": ran, "mismatching_cases": n_bad, "seconds": round(time.time() - t0, 1)}))
        sys.exit(1 if n_bad else 0)
    for k in range(a.cases):
        c = draw_clone(draw_surface(draw_more_sliders(draw_case(rng, a.max_cells, a.big))))
        if a.mode == "group":
            c = draw_group(rng, c)
        if a.sun_exact and a.mode in ("oracle", "group"):
            c = draw_sun_exact(c)
        if a.mode == "script":
            c = draw_script(rng_script, c)
        if (a.only >= 0 and k != a.only) or k < a.first:
            continue
        if k > a.last:
            break
        if time.time() - t0 > a.seconds:
            break
        if a.override:
            c.update(json.loads(a.override))
        t1 = time.time()
        if a.mode == "oracle" and a.interleave and rng_il.random() < 0.5 and a.only < 0:  # this case and a second small one, handles alive together
            c2 = draw_more_sliders(draw_case(rng_il, min(a.max_cells, 60000)))
            (bad, info), (bad2, info2) = run_interleaved(pkg, E, wx_oracle, [c, c2])
            if bad2 and not info2.get("blown_up"):
                failures.append({"case": k, "interleaved_with": c, "recipe": c2, "mismatches": bad2})
                print("MISMATCH in the interleaved companion:", json.dumps(failures[-1]), flush=True)
        elif a.mode == "script":
            print(f"case {k} recipe: {json.dumps(c)}", flush=True)  # BEFORE it runs: a case that faults or hangs leaves its recipe behind
            try:
                bad, info = run_script_case(pkg, E, wx_oracle, c)
            except E.WxError as e:  # not the reported overflow of a blown-up scene: the run ends here (no retry, nothing further on the GPU)
                print(f"case {k}: UNEXPECTED ERROR {e}", flush=True)
                sys.exit(2)
            for kind, n in info["actions"].items():
                totals[kind] += n
        else:
            bad, info = run_case(pkg, E, wx_oracle, c) if a.mode == "oracle" else (run_group_case(pkg, E, c) if a.mode == "group" else run_setup_case(pkg, E, c))
        ran += 1
        reported += 1 if info.get("error") else 0
        compared += 0 if (info.get("error") or info.get("blown_up")) else 1
        if bad and info.get("blown_up"):  # NaN / inf / |v| > 1e4 cells per iteration (the reference blows up the same way): float -> int conversions out of range differ between CPU and GPU
            print(f"case {k}: state not finite, {len(bad)} fields differ -- not counted", flush=True)
            bad = []
        tag = "MISMATCH" if bad else ("reported: " + info["error"][:60] if info.get("error") else "ok")
        print(f"case {k:4d} {c['X']:5d}x{c['Y']:<5d} {'dry' if c['dry'] else 'wet'} sigma {c['sigma']:.2f} steps {c['steps']} drops {c['drops']:4d} brush "
              f"{c['brush']['type'] if c['brush'] else '-':>2} pairs {c['pairs']} bands {c['bands']} set {c['kernel_set']}{c['dry_kernel']}{' slabs %d halo %d overlap %d' % (c['nslab'], c['halo'], c['overlap']) if a.mode == 'group' else ''} fastest {info.get('fastest')}{' terrain columns differing %s' % info.get('terrain_columns_differing') if a.mode == 'setup' else ''}  {time.time() - t1:.1f}s  {tag}", flush=True)
        if bad:
            failures.append({"case": k, "recipe": c, "mismatches": bad})
            print(json.dumps(failures[-1]), flush=True)
    print(json.dumps(dict({"mode": a.mode, "seed": a.seed, "cases_run": ran, "cases_compared": compared, "mismatching_cases": len(failures),
                           "cases_ending_in_a_reported_error": reported, "seconds": round(time.time() - t0, 1)}, **({"actions": totals} if a.mode == "script" else {}))))
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
