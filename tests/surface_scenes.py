"""Surface impulse scenes: the lattice method of tests/impulse_scenes.py applied to the SURFACE ROW -- the slow physics of
boundary_cell (csrc/wx_cells.h, `wl[VERT_DISTANCE] == 0`): snow / soil-moisture smoothing, vegetation growth, fire spread, the
industrial chimneys, the urban / industrial vegetation caps.

That part of the iteration depends on `iterNum` (smoothing, growth and fire spread exist on iterations that are multiples of 100 only;
growth on multiples of `(100 / rate) * 100`; spread where `iterNum / 100` is a multiple of the cell's divisor), and the marching wet
kernel has a phase of its own for it: only on those iterations do the neighbours' soil moisture and snow travel between lanes
(wx_wet.h `smooth_iter`). A scene is a quiet background whose surface row is UNIFORM -- land, vegetation 60, soil moisture 5, no
snow -- plus ONE altered surface cell per lattice site along x (pitch 73). On a uniform row a wrong neighbour shows at once: the
smoothing of a lone heap moves 2 % of it into each neighbour, and nothing anywhere else.

A plain module like impulse_scenes (whose helpers it uses): numpy on top of synth.py, no fixture, no GPU. tests/test_surface_gpu.py
runs the case list, tests/test_surface_cpu.py accounts for the lanes it reaches on a smoothing iteration.
"""
from __future__ import annotations

import numpy as np

import impulse_scenes as I
import wxpkg

LAND, WATER, FIRE, URBAN, RUNWAY, INDUSTRIAL = 1, 2, 3, 4, 5, 6
KINDS = ("snow", "soil", "fire", "industrial", "urban", "growth", "smoke")
VARIANTS = ("flat", "stepped")
PITCH = I.PITCH[0]  # 73: co-prime with the strip width (56) and with the chimneys' period (80)
GROUND = 3          # wall rows of the flat background: rows 0 .. 2, the surface row is row 2
BACKGROUND = {"vegetation": 60, "soil": 5.0, "snow": 0.0}  # soil 5 -> fire divisor 10; vegetation 60 is above the growth cap of the surface air (55)
PHASE_GRID = I.PHASE_GRID  # 505 x 77
# Iterations whose first one IS a smoothing iteration: 100; 10 000 (growth rates 1, 2, 4, 5, 10 fire and `iterNum / 100` is a multiple of
# the background's fire divisor 10); 9 240 000, the least common multiple of the ten growth intervals (below 2^24: exact as a float).
SMOOTHING_ITERS = (100, 10_000, 9_240_000)
OFF_ITERS = (99, 101)  # 99: the SECOND iteration smooths (a display iteration of its own step); 101: no iteration of the run does
CHIMNEY_COLUMNS = (18, 22, 29)  # x % 80 of the cooling towers (VERT_DISTANCE 5) and the smoke stack (VERT_DISTANCE 6)


def site_columns(X, offset):
    """Columns of the sites: X // 73 of them from ``offset`` on, periodic."""
    return [(offset + i * PITCH) % X for i in range(max(1, X // PITCH))]


def site_value(kind, k):
    """What site ``k`` carries -- a pure function of kind and site number."""
    if kind == "snow":
        return 40.0 + 10.0 * (k % 5)
    if kind == "soil":
        return 200.0 + 100.0 * (k % 4)  # (growth rate 1 .. 4 once the light is there)
    if kind == "fire":
        return 80 + 10 * (k % 4)  # its vegetation
    if kind == "industrial":
        return 3 + k % 4  # cells of industrial surface (3 .. 6) from the column before the site on, under snow
    if kind == "urban":
        return 90 + 10 * (k % 3)  # vegetation above the cap of 75
    if kind == "growth":
        # (vegetation, soil moisture). The surface air is at 11 C: the cap is (int)(11 / 25 * 127) = 55, so 54 and 30 may grow, 56 may
        # not. Full sunlight is about 1250 W/m2, sqrt(light) * 0.01 = 0.35: soil 4, 7 .. 19 -> growth rates 1 .. 6
        return (54, 30, 54, 30, 56, 54)[k % 6], 4.0 + 3.0 * (k % 6)
    if kind == "smoke":
        return 4.5 + 0.5 * (k % 4)  # 4.5 itself does not ignite (> 4.5 does)
    raise ValueError(kind)


INDUSTRIAL_SNOW = 30.0  # on the industrial cells: they smooth towards their land neighbours, which must NOT count them in turn


def industrial_columns(X, x, v):
    """The ``v`` columns of an industrial stretch around site column x: from x - 1 on (so the site's left neighbour is industrial too:
    under a chimney column the column before it is there to stay quiet)."""
    return [(x - 1 + dx) % X for dx in range(v)]


def heights(X, variant):
    """Wall rows per column. "stepped": every ninth column is one row higher (its surface neighbours are not at VERT_DISTANCE 0:
    they leave the smoothing average) and every 31st one lower."""
    h = np.full(X, GROUND, np.int64)
    if variant == "stepped":
        x = np.arange(X)
        h[x % 9 == 4] += 1
        h[x % 31 == 7] -= 1
    elif variant != "flat":
        raise ValueError(variant)
    return h


def background(X, Y, variant="flat", seed=1234, flow_sigma=0.02):
    """-> base, water, wall, h. Land of uniform vegetation / soil moisture under air at rest on the start sounding, with the wall bytes
    the boundary pass keeps (type handed up the column, vertical and Manhattan distances)."""
    pkg = wxpkg.load_package()
    d = pkg.synth.sounding_rows(Y)
    h = heights(X, variant)
    yy = np.arange(Y)[:, None]
    is_wall = yy < h[None, :]
    air = ~is_wall
    base = np.zeros((Y, X, 4), np.float32)
    water = np.zeros((Y, X, 4), np.float32)
    wall = np.zeros((Y, X, 4), np.int8)
    base[..., 3] = np.where(air, d["T_air"][:, None], np.float32(1000.0))
    water[..., 0] = np.where(air, d["total_water"][:, None], np.float32(1001.0))
    water[..., 1] = np.where(air, d["cloud_water"][:, None], np.float32(0.0))
    water[..., 2] = np.where(is_wall, np.float32(BACKGROUND["soil"]), np.float32(0.0))
    water[..., 3] = np.where(is_wall, np.float32(BACKGROUND["snow"]), np.float32(0.0))
    rng = np.random.Generator(np.random.Philox(seed))
    for ch in (0, 1):
        base[..., ch] = np.where(air, rng.standard_normal((Y, X), dtype=np.float32) * np.float32(flow_sigma), 0).astype(np.float32)
    wall[..., 0] = LAND
    vdist = yy - h[None, :] + 1
    wall[..., 2] = np.clip(vdist, -127, 127).astype(np.int8)
    wall[..., 3] = np.where(is_wall, BACKGROUND["vegetation"], 0).astype(np.int8)
    # Manhattan distance to the nearest wall cell (steps of one row: the nearest wall is below, or beside within a column or two)
    dist = np.where(is_wall, 0, vdist)
    for dx in (-2, -1, 1, 2):
        hn = np.roll(h, -dx)
        dist = np.minimum(dist, np.where(is_wall, 0, np.maximum(yy - hn[None, :] + 1, 0) + abs(dx)))
    wall[..., 1] = np.clip(dist, 0, 127).astype(np.int8)
    return base, water, wall, h


def _set_type(wall, x, t):
    """Surface type ``t`` in column x: the wall cells and, as the boundary pass hands it up, the air above."""
    wall[:, x, 0] = t


def surface_scene(X, Y, kind, offset=0, variant="flat", plant=True, seed=1234):
    """-> base, water, wall, sites. ``sites``: the (x, y) of the altered SURFACE cells (y = the top wall row of the column), site k
    carries site_value(kind, k). ``plant=False``: the background alone."""
    if kind not in KINDS:
        raise ValueError(kind)
    base, water, wall, h = background(X, Y, variant, seed)
    sites = [(x, int(h[x]) - 1) for x in site_columns(X, offset)]
    for k, (x, y) in enumerate(sites if plant else ()):
        v = site_value(kind, k)
        if kind == "snow":
            water[:y + 1, x, 3] = v
        elif kind == "soil":
            water[:y + 1, x, 2] = v
        elif kind == "fire":
            _set_type(wall, x, FIRE)
            wall[:y + 1, x, 3] = v
        elif kind == "industrial":
            for xx in industrial_columns(X, x, v):
                _set_type(wall, xx, INDUSTRIAL)
                wall[:h[xx], xx, 3] = 100  # (capped to 15 by the first iteration)
                water[:h[xx], xx, 3] = INDUSTRIAL_SNOW
        elif kind == "urban":
            _set_type(wall, x, URBAN)
            wall[:y + 1, x, 3] = v
        elif kind == "growth":
            wall[:y + 1, x, 3] = v[0]
            water[:y + 1, x, 2] = v[1]
        elif kind == "smoke":
            water[y + 1:y + 4, x, 3] = v  # three air cells above the surface cell: what drifts in during the run stays above 4.5 for the smaller values only
    return base, water, wall, sites


def scene_uniforms(Y, wrap=True):
    """Default settings, the sun 10 degrees from the zenith, no precipitation."""
    P = wxpkg.load_package().params
    gui = P.merge_settings(None)
    gui["sunAngle"] = 80.0
    gui["wrapHorizontally"] = bool(wrap)
    u = P.uniforms_from_gui(gui, Y, quad_scale=0, pass_mask=P.PASS_ALL)
    u["enablePrecipitation"] = 0
    return u


# ---- blow-up kinds of the fire divisor (tests/test_blowup_*.py) ----
DIVISOR_KINDS = ("divisor_soil", "divisor_snow")


def divisor_scene(X, Y, kind, offset=0, variant="flat"):
    """An uploaded state whose surface neighbours carry soil moisture / snow far below zero (the ABI accepts it; a brush can leave it
    there). Each cell clamps its OWN value to >= 0 before it smooths, but reads its neighbours' unclamped: on a smoothing iteration the
    site between two such cells ends at 0.98 * 0 + 0.02 * avg, and `(int)(soil * 0.1 + snow * 0.5) + 10` -- the fire-spread divisor --
    becomes 0 (even sites: neighbours at -5250 soil / -1050 snow) or -10 (odd sites: -10 000 / -2050). Smoke above 4.5 sits over every
    site, so the divisor alone decides whether it ignites: not at all for 0 (`% 0` is undefined in GLSL: fixed to false), and at
    iterNum 1000 for -10 (10 % -10 == 0)."""
    if kind not in DIVISOR_KINDS:
        raise ValueError(kind)
    base, water, wall, h = background(X, Y, variant)
    sites = [(x, int(h[x]) - 1) for x in site_columns(X, offset)]
    ch, zero, negative = (2, -5250.0, -10000.0) if kind == "divisor_soil" else (3, -1050.0, -2050.0)
    for k, (x, y) in enumerate(sites):
        water[:y + 1, x, 2] = 0.0
        water[y + 1:y + 4, x, 3] = 6.0
        for xn in ((x - 1) % X, (x + 1) % X):
            water[:h[xn], xn, ch] = zero if k % 2 == 0 else negative
    return base, water, wall, sites


def divisor_sites_lit(X, sites, variant):
    """Which sites of a divisor scene ignite at iterNum 1000: the odd ones (divisor -10) -- and, stepped, a site on a raised or
    lowered column: neither neighbour is at VERT_DISTANCE 0 of its row, nothing is averaged, its divisor stays the background's 10."""
    h = heights(X, variant)
    return [k % 2 == 1 or (h[(x - 1) % X] != h[x] and h[(x + 1) % X] != h[x]) for k, (x, y) in enumerate(sites)]


def expected_divisor(kind, k):
    """The divisor of site k on the first iteration, in the shader's float arithmetic (the site's own value is 0, evaporation aside)."""
    factor, zero, negative = (np.float32(0.1), -5250.0, -10000.0) if kind == "divisor_soil" else (np.float32(0.5), -1050.0, -2050.0)
    v = np.float32(zero if k % 2 == 0 else negative) * np.float32(0.02)
    return int(v * factor) + 10


# ---- the case list ----
# configuration -> (key of tools/fuzz_parity.IMPULSE_CONFIGS, first iteration of the run, pre-roll). The schedule decides what kind of
# iteration the FIRST one is: steps (1, 1, 3) a display iteration, (3, 2) a plain one, pieces a WX_OVERLAP_MORE_TO_COME piece. With a
# pre-roll the run starts that many iterations EARLIER, stepped in one call, so that the named iteration is still the first of the
# schedule: sunlight comes down one row per iteration, and without it no vegetation grows (the growth kind: 80 iterations for 77 rows).
KERNEL_CONFIGS = ("wet", "wet_plain", "wet_pieces", "wet_stored", "perpass")
CONFIGS = {f"{kc}@{it}": (kc, it, 0) for it in SMOOTHING_ITERS for kc in KERNEL_CONFIGS}
CONFIGS.update({f"{kc}@{it}": (kc, it, 0) for it in OFF_ITERS for kc in ("wet", "wet_plain", "perpass")})
BAND_CONFIGS = {f"{kc}@{it}": (kc, it, 0) for it in (100, 10_000) for kc in ("wet_bands0", "wet_bands1", "wet_bands2")}
CONFIGS.update(BAND_CONFIGS)
GROWTH_GRID, GROWTH_PREROLL = PHASE_GRID, 80
GROWTH_CONFIGS = {f"{kc}@{it}+light": (kc, it, GROWTH_PREROLL) for it in (10_000, 9_240_000) for kc in ("wet", "wet_plain", "wet_pieces", "perpass")}
GROWTH_CONFIGS["wet@9240100+light"] = ("wet", 9_240_100, GROWTH_PREROLL)  # a smoothing iteration that is no multiple of any growth interval
CONFIGS.update(GROWTH_CONFIGS)
LANE_OFFSETS = (0, 1, 2, 3, 4)  # on 505 columns: strip phases 0, 1, 2 (first site) and 53, 54, 55 (fourth site) of the 56 output columns
BANDS_GRID = (2500, 300)        # low and wide: row bands; 2500 % 56 == 36, a ragged last strip
# site 0 on a chimney column, in the first period of 80 and in the sixth (x % 80 is not x); pitch 73 = 80 - 7 walks the other sites on
CHIMNEY_OFFSETS = tuple(c + 80 * j for c in CHIMNEY_COLUMNS for j in (0, 5))


def edge_offsets(X):
    """Offsets that put a site on columns 0, 1, X-2, X-1 (the wrap seam from both sides) and on the ragged last strip's first column."""
    cols = [0, 1, X - 2, X - 1]
    if X % I.WET_STRIP:
        cols.append((X // I.WET_STRIP) * I.WET_STRIP)
    return tuple(cols)


def _sweep(name, grid, kinds, offsets, variants, configs, wraps=(True,), requires=()):
    return {"name": name, "grid": grid, "kinds": tuple(kinds), "offsets": tuple(offsets), "variants": tuple(variants), "configs": tuple(configs),
            "wraps": tuple(wraps), "requires": tuple(requires)}


_MAIN = tuple(k for k in CONFIGS if k not in BAND_CONFIGS and k not in GROWTH_CONFIGS)
_NO_GROWTH = tuple(k for k in KINDS if k != "growth")  # (needs the light: its own sweep)
SWEEPS = (
    _sweep("lanes", PHASE_GRID, _NO_GROWTH, LANE_OFFSETS, ("flat",), _MAIN, requires=("lanes",)),
    _sweep("growth", GROWTH_GRID, ("growth",), LANE_OFFSETS, VARIANTS, tuple(GROWTH_CONFIGS), requires=("lanes",)),
    _sweep("lanes_stepped", PHASE_GRID, _NO_GROWTH, LANE_OFFSETS, ("stepped",), ("wet@100", "wet_plain@10000", "perpass@100", "wet@99")),
    _sweep("edges", PHASE_GRID, _NO_GROWTH, edge_offsets(PHASE_GRID[0]), VARIANTS, ("wet@100", "wet_plain@10000", "wet_pieces@100", "perpass@100"),
           wraps=(True, False), requires=("edges",)),
    _sweep("chimneys", PHASE_GRID, ("industrial",), CHIMNEY_OFFSETS, VARIANTS, ("wet@100", "wet_plain@101", "perpass@99"), requires=("chimneys",)),
    _sweep("bands", BANDS_GRID, ("snow", "soil", "fire"), edge_offsets(BANDS_GRID[0]), ("flat",), tuple(BAND_CONFIGS), requires=("edges",)),
)


def cases():
    out = []
    for sw in SWEEPS:
        for off in sw["offsets"]:
            for kind in sw["kinds"]:
                for variant in sw["variants"]:
                    for wrap in sw["wraps"]:
                        for config in sw["configs"]:
                            out.append({"sweep": sw["name"], "X": sw["grid"][0], "Y": sw["grid"][1], "kind": kind, "offset": int(off),
                                        "variant": variant, "wrap": bool(wrap), "config": config})
    return out


def build_case(c, **kw):
    return surface_scene(c["X"], c["Y"], c["kind"], offset=c["offset"], variant=c["variant"], **kw)


def first_smoothing_iteration(config):
    """Index (0-based) of the first iteration of a run under ``config`` that is a smoothing iteration, or None within five."""
    it0 = CONFIGS[config][1]  # (a pre-roll ends where this iteration begins)
    for k in range(5):
        if (it0 + k) % 100 == 0:
            return k
    return None


# ---- the walking fire: spread over several smoothing iterations, across a strip seam ----
def walking_fire_scene(X, Y, x0):
    """A fire at column x0 whose neighbours' soil moisture makes their divisors 10, 11, 12, 13 going outward on BOTH sides: from
    iterNum 995 on it takes one cell each way at iterations 1000, 1100, 1200 and 1300 (`iterNum / 100` = 10, 11, 12, 13)."""
    base, water, wall, h = background(X, Y, "flat")
    _set_type(wall, x0, FIRE)
    wall[:h[x0], x0, 3] = 100
    for d in range(1, 5):
        for x in ((x0 - d) % X, (x0 + d) % X):
            water[:h[x], x, 2] = 5.0 + 10.0 * (d - 1)  # 5, 15, 25, 35 -> divisor 10, 11, 12, 13
            wall[:h[x], x, 3] = 100
    return base, water, wall, [(x0, int(h[x0]) - 1)]


# ---- the runner ----
def run_scene(pkg, fuzz, oracle, scene, X, Y, kernel_config, iter0, steps, wrap=True, preroll=0):
    """(The runner of tests/test_surface_gpu.py and of the divisor test in tests/test_blowup_gpu.py; ``fuzz``: tools/fuzz_parity.)
    One scene, one handle configured as tools/fuzz_parity.IMPULSE_CONFIGS[kernel_config] says, against the oracle after every step.
    -> (mismatches, the oracle's final wall texture)."""
    base, water, wall, sites = scene
    cfg = fuzz.IMPULSE_CONFIGS[kernel_config]
    u = scene_uniforms(Y, wrap=wrap)
    h, o = pkg.engine.Handle(X, Y, 0), oracle.OracleSim(X, Y, 0)
    bad = []
    try:
        h.upload(base, water, wall)
        o.upload(base, water, wall)
        h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
        o.set_params(u)
        h.iter = o.iter = iter0 - preroll
        h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
        h.set_option(h.OPT_ROW_BANDS, cfg.get("bands", 1))
        h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
        done = -preroll
        for k, n in enumerate(((preroll,) if preroll else ()) + tuple(steps)):
            if cfg.get("pieces") and n > 1 and not (preroll and k == 0):
                h.step(1, 4)
                h.step(n - 1)
            else:
                h.step(n)
            o.step(n)
            done += n
            for f in fuzz.GRID_FIELDS:
                a, b = h.read_rect(f), o.field(f)
                if not np.array_equal(a, b):
                    bad.append({"field": f, "after_iterations": done, "what": I.describe_difference(f, a, b, sites, X)})
            if bad:
                break
        assert h.iter == o.iter
        return bad, o.field("WALL_CUR")
    finally:
        h.close()
        o.close()
