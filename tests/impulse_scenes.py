"""Impulse-lattice scenes: a quiet background plus SINGLE-CELL triggers so far apart that each one is alone in its wavefront rows.

The marching kernels (csrc/wx_wet.h, wx_march.h, wx_march2.h) switch their shortcuts by wave-uniform votes over one row of 64 lanes
(h_big, h_nowall, h_zw0), by lane windows and by per-tile flags. An off-by-one in any of them shows in one situation only: a LONE
trigger at one lane / row / tile phase with quiet neighbours, so that no other lane of the wave raises the same vote. The scenes here
put one trigger per site of a rectangular lattice; pitch and offset move the lattice through the phases, and the case lists below
(SWEEPS) are what tests/test_impulse_gpu.py runs, what tests/test_impulse_cpu.py accounts for and what tools/fuzz_parity.py
--mode impulse draws from. A plain module: pure numpy on top of synth.py, no fixture, no GPU.

Strip geometry the accounting is computed against (tests/test_impulse_cpu.py reads the constants from the kernel sources and
compares): the wet kernel and the pair kernel write 56 columns per wave (output lanes 4 .. 59), the one-iteration dry kernel 60
(lanes 2 .. 61); the pair kernel records 8 x 8 tiles; splat tiles are 64 x 16.
"""
from __future__ import annotations

import itertools

import numpy as np

import wxpkg

KINDS = ("smoke", "precip_visual", "cloud", "wall", "fast_vx", "fast_vy", "droplet", "T_spike", "P_spike")
DRY_KINDS = ("wall", "fast_vx", "fast_vy", "T_spike", "P_spike")  # kinds that leave the water-free state water-free: the dry kernels run
WET_KINDS = tuple(k for k in KINDS if k != "droplet")             # (droplets need a lattice of their own: a sprite is 12 x 12)
# 0.9 is the threshold of both exact paths, 3 cells the whole-pair repeat of wx_march2.h; no NaN / Inf sites
FAST_VALUES = (float(np.nextafter(np.float32(0.9), np.float32(0.0))), float(np.float32(0.9)), 1.3, 2.99, 3.0, 7.5)
# The dry kinds add two more: a lone spike loses nine tenths of its speed to the pressure step of its first iteration (the oracle: 7.5 ->
# 0.46), so only these are still beyond 0.9 (20 -> 1.1 .. 1.4) and beyond 3 cells (80 -> 4.5 .. 5.5) in the SECOND iteration of a pair --
# by then a cluster of a few cells around the site, no longer one cell. The wet state does not survive them (it blows up), so wet cases keep the six.
DRY_FAST_VALUES = FAST_VALUES + (20.0, 80.0)
WALL_TYPES = (0, 1, 2, 4, 5, 6)  # inert, land, water, urban, runway, industrial (fire burns out: its own schedule)
MIN_DX, MIN_DY = 72, 10          # two sites are at least 72 columns (periodic) OR 10 rows apart
PITCH = (73, 11)                 # co-prime with 56, 60, 64, 16 and 8
DROPLET_PITCH = (73, 29)         # a 12 x 12 sprite that falls and drifts for five iterations stays alone
WET_STRIP, DRY_STRIP, PAIR_STRIP, PAIR_TILE, SPLAT_TILE = 56, 60, 56, 8, (64, 16)


def lattice_sites(X, Y, pitch=PITCH, offset=(0, 1), y_min=1):
    """Sites (x, y) of the lattice: rows offset[1] + j * pitch[1] (from ``y_min`` up: row 0 is the floor), in every row X // pitch[0]
    sites from column offset[0] on, periodic in x -- so the gap across the seam is at least one pitch as well."""
    px, py = pitch
    ox, oy = offset
    n_x = max(1, X // px)
    ys = [y for y in range(oy % py, Y, py) if y >= y_min]
    return [((ox + i * px) % X, y) for y in ys for i in range(n_x)]


def isolation_violations(sites, X, min_dx=MIN_DX, min_dy=MIN_DY):
    """Pairs of sites closer than the spacing rule (periodic in x)."""
    bad = []
    s = sorted(sites, key=lambda p: (p[1], p[0]))
    for a in range(len(s)):
        for b in range(a + 1, len(s)):
            if s[b][1] - s[a][1] >= min_dy:
                break
            dx = abs(s[a][0] - s[b][0])
            if min(dx, X - dx) < min_dx:
                bad.append((s[a], s[b]))
    return bad


def site_value(kind, k, fast_values=None):
    """What site number ``k`` of a scene carries (a pure function of kind and site number: tests recompute it for their accounting)."""
    if kind in ("fast_vx", "fast_vy"):
        vals = FAST_VALUES if fast_values is None else tuple(fast_values)
        return (1.0 if k % 2 == 0 else -1.0) * vals[(k // 2) % len(vals)]
    if kind == "wall":
        return WALL_TYPES[k % len(WALL_TYPES)]
    if kind == "smoke":
        return 0.5 + 0.25 * (k % 7)
    if kind == "precip_visual":
        return 0.2 + 0.1 * (k % 5)
    if kind == "cloud":
        return 0.4 + 0.2 * (k % 4)
    if kind == "T_spike":
        return (1.0 if k % 2 == 0 else -1.0) * (0.5 + 0.5 * (k % 3))
    if kind == "P_spike":
        return (1.0 if k % 2 == 0 else -1.0) * 0.002 * (1 + k % 3)
    if kind == "droplet":  # (rain mass, snow mass): every third one is snow
        return (0.0, 0.3 + 0.1 * (k % 4)) if k % 3 == 2 else (0.3 + 0.1 * (k % 4), 0.0)
    raise ValueError(kind)


def _plant_wall(base, water, wall, x, y, wtype, dry):
    """One floating wall cell with the bytes the boundary pass would have left around it: distance 0 / vertical distance 0 in the cell,
    vertical distances and the type handed up the column above it, Manhattan distances around it."""
    Y, X = wall.shape[:2]
    base[y, x] = (0.0, 0.0, 0.0, 1000.0 if wtype != 2 else 288.15)
    water[y, x] = (1002.0 if wtype == 2 else 1001.0, 0.0, 0.0 if dry else (100.0 if wtype == 2 else 25.0), 0.0)
    wall[y, x] = (wtype, 0, 0, 0 if dry or wtype == 2 else 40)
    for yy in range(y + 1, Y):
        if wall[yy, x, 1] == 0:
            break
        wall[yy, x, 0] = wtype
        wall[yy, x, 2] = min(yy - y, 127)
    r = 126
    ys = np.arange(max(0, y - r), min(Y, y + r + 1))
    dxs = np.arange(-r, r + 1)
    xs = (x + dxs) % X
    d = np.abs(ys - y)[:, None] + np.abs(dxs)[None, :]
    cur = wall[np.ix_(ys, xs, [1])][..., 0].astype(np.int64)
    new = np.where(cur == 0, 0, np.minimum(cur, np.clip(d, 0, 127)))
    new[(ys == y)[:, None] & (dxs == 0)[None, :]] = 0
    wall[np.ix_(ys, xs, [1])] = new.astype(np.int8)[..., None]


def impulse_scene(X, Y, kind, pitch=None, offset=(0, 1), background="air", flow_sigma=0.05, fast_values=None, seed=1234, plant=True):
    """-> base, water, wall, drops, sites.

    ``background``: "air" -- an inert floor row under free air (synth.dry_grid: for the DRY_KINDS this is the agreed water-free state the
    dry kernels need), "terrain" -- synth.terrain_grid with the triggers kept above the ground (sites in or on it are dropped; the
    ground rows keep the kernels' no-wall vote false while the rows aloft decide). Both carry a slow flow of ``flow_sigma`` cells /
    iteration. ``sites`` is the list of (x, y) that carry a trigger, in planting order: site k carries site_value(kind, k).
    ``drops`` is None except for the droplet kind (one ACTIVE droplet per site, at the centre of its cell). ``plant=False`` returns the
    background alone (and the sites it would have planted): what the non-vacuity test steps next to the scene."""
    if kind not in KINDS:
        raise ValueError(kind)
    if Y < 4:
        raise ValueError("an impulse scene needs 4 rows")
    S = wxpkg.load_package().synth
    pitch = (DROPLET_PITCH if kind == "droplet" else PITCH) if pitch is None else tuple(pitch)
    if background == "air":
        base, water, wall = S.dry_grid(X, Y, seed=seed, flow_sigma=flow_sigma)
        ground = np.ones(X, np.int64)
    elif background == "terrain":
        base, water, wall = S.terrain_grid(X, Y)
        ground = (wall[..., 1] == 0).sum(0)
        rng = np.random.Generator(np.random.Philox(seed))
        air = wall[..., 1] != 0
        for ch in (0, 1):
            base[..., ch] += np.where(air, rng.standard_normal((Y, X), dtype=np.float32) * np.float32(flow_sigma), 0).astype(np.float32)
    else:
        raise ValueError(background)
    sites = [(x, y) for x, y in lattice_sites(X, Y, pitch, offset) if y >= ground[x]]
    dry = background == "air"
    for k, (x, y) in enumerate(sites if plant else ()):
        v = site_value(kind, k, fast_values)
        if kind == "smoke":
            water[y, x, 3] = v
        elif kind == "precip_visual":
            water[y, x, 2] = v
        elif kind == "cloud":
            water[y, x, 1] += np.float32(v)
            water[y, x, 0] += np.float32(v)
        elif kind == "wall":
            _plant_wall(base, water, wall, x, y, v, dry)
        elif kind in ("fast_vx", "fast_vy"):
            base[y, x, 0 if kind == "fast_vx" else 1] = v
        elif kind == "T_spike":
            base[y, x, 3] += np.float32(v)
        elif kind == "P_spike":
            base[y, x, 2] += np.float32(v)
    drops = None
    if kind == "droplet":
        drops = np.zeros((len(sites), 5), np.float32)
        drops[:, 2] = -10.5  # (plant=False: an all-inactive pool)
        for k, (x, y) in enumerate(sites if plant else ()):
            rain, snow = site_value(kind, k)
            drops[k] = (((x + 0.5) / X - 0.5) * 2.0, ((y + 0.5) / Y - 0.5) * 2.0, rain, snow, 1.0 if snow == 0.0 else 0.3)
    return base, water, wall, drops, sites


def scene_uniforms(kind, Y, dry=False):
    """The uniforms an impulse scene runs with: default settings, the sun up; ``dry`` = the dry stencil's pass mask. Droplets never
    spawn (spawnChanceMult 0): the pool holds the planted ones only."""
    P = wxpkg.load_package().params
    gui = P.merge_settings(None)
    gui["sunAngle"] = 40.0
    u = P.uniforms_from_gui(gui, Y, quad_scale=0, pass_mask=P.PASS_DRY if dry else P.PASS_ALL)
    u["enablePrecipitation"] = 1 if kind == "droplet" else 0
    if kind == "droplet":
        u["spawnChanceMult"] = 0.0
    return u


def sprite_windows(drops, X, Y):
    """(i0, j0) of the 12 x 12 sprites of droplet records (float32, as the splat computes them: pixel centres in [w - 6, w + 6))."""
    d = np.asarray(drops, np.float32)
    xw = (d[:, 0] + np.float32(1.0)) * np.float32(0.5) * np.float32(X)
    yw = (d[:, 1] + np.float32(1.0)) * np.float32(0.5) * np.float32(Y)
    return np.ceil(xw - np.float32(6.5)).astype(np.int64), np.ceil(yw - np.float32(6.5)).astype(np.int64)


def deposits_per_texel(drops_before, drops_after, X, Y):
    """Largest number of order-sensitive deposits any texel of the feedback textures received in the iteration that turned
    ``drops_before`` into ``drops_after``: droplets active before it splat a 12 x 12 sprite at their new position (clipped at the
    grid's edges), inactive ones add 1.0 to texel (0, 0) -- any number of those is one exact sum. 1 or less = order-free."""
    b, a = np.asarray(drops_before, np.float32), np.asarray(drops_after, np.float32)
    act = b[:, 2] >= 0
    cover = np.zeros((Y, X), np.int32)
    ok = (np.abs(a[:, 0]) <= 1) & (np.abs(a[:, 1]) <= 1)
    i0, j0 = sprite_windows(a, X, Y)
    for k in np.nonzero(act & ok)[0]:
        cover[max(0, j0[k]):max(0, min(Y, j0[k] + 12)), max(0, i0[k]):max(0, min(X, i0[k] + 12))] += 1
    n_inactive = int((~act).sum())
    cover[0, 0] += n_inactive if cover[0, 0] else min(n_inactive, 1)
    return int(cover.max())


# ---- phases ----
def site_phases(x, y, X):
    """The phases of a site the kernels' shortcuts depend on, for error messages and the accounting."""
    def strip(w):
        s0 = (X // w) * w
        return {"lane": x % w, "strip": x // w, "ragged": bool(X % w and x >= s0), "from_end": (min(X, (x // w + 1) * w) - 1 - x)}
    return {"wet56": strip(WET_STRIP), "dry60": strip(DRY_STRIP), "row_mod8": y % 8, "tile8": (x % 8, y % 8),
            "pair_tile": ((x % PAIR_STRIP) % 8, y % 8), "splat_tile": (x % SPLAT_TILE[0], y % SPLAT_TILE[1])}


def nearest_site(sites, x, y, X):
    def dist(s):
        dx = abs(s[0] - x)
        return min(dx, X - dx) + abs(s[1] - y)
    return min(sites, key=dist)


def describe_difference(field, a, b, sites, X):
    """First differing cell of a field, the nearest site and its phases (what an assertion message says)."""
    ne = (a != b)
    while ne.ndim > 2:
        ne = ne.any(-1)
    ys, xs = np.nonzero(ne)
    x, y = int(xs[0]), int(ys[0])
    s = nearest_site(sites, x, y, X) if sites else None
    return (f"{field}: {int((a != b).sum())} values differ, first cell (x={x}, y={y}): {a[y, x]} != {b[y, x]}; nearest site {s}"
            + (f" phases {site_phases(s[0], s[1], X)}" if s else ""))


# ---- the case lists (shared by the GPU test, the CPU accounting and the fuzzer) ----
def _edge_columns(X):
    cols = {0, 1, X - 2, X - 1}
    for w in (WET_STRIP, DRY_STRIP):
        if X % w:
            s0 = (X // w) * w
            cols |= {s0, min(s0 + 1, X - 1)}
    return sorted(cols)


LANE_OFFSETS_WET = (0, 1, 2, 3, 4)            # with pitch 73 on a 505-column grid: lanes 0, 1, 2 (first site of a row) and 53, 54, 55 (fourth) of a 56-column strip
LANE_OFFSETS_DRY = (0, 1, 2, 3, 4, 5, 6, 7)   # ... and 0, 1, 2 / 57, 58, 59 (fifth site) of a 60-column strip
ROW_OFFSETS = tuple(range(1, 12))             # every row of the grid is a lattice row of one of them
PHASE_GRID = (505, 77)                        # 9 strips of 56 + 1 column (X % 56 == 1), 8 of 60 + 25
PAIR_GRID_55 = (559, 45)                      # X % 56 == 55

# (what each one runs: tools/fuzz_parity.IMPULSE_CONFIGS)
WET_CONFIGS = ("wet", "wet_plain", "wet_stored", "wet_pieces", "perpass")
DRY_CONFIGS = ("dry_single", "dry_single_plain", "dry_pairs", "dry_pairs_plain", "dry_perpass")
ROW_KINDS_WET = ("smoke", "wall", "fast_vx", "fast_vy")  # on the big grids: one trigger per shortcut (NO_ZW, NO_WALL, the exact path)
ROW_KINDS_DRY = ("wall", "fast_vx", "fast_vy")


def config_strip(config):
    """Output columns per wave of the kernel that meets the trigger's first iteration under a configuration (None: the per-pass kernels
    have no strips)."""
    if "perpass" in config:
        return None
    return DRY_STRIP if config.startswith("dry_single") else (PAIR_STRIP if config.startswith("dry_pairs") else WET_STRIP)


def _sweep(name, grid, kinds, offsets, configs, background="air", pitch=None, requires=()):
    return {"name": name, "grid": grid, "kinds": tuple(kinds), "offsets": tuple(offsets), "configs": tuple(configs), "background": background,
            "pitch": pitch, "requires": tuple(requires)}


def _row_and_edge_offsets(X):
    """Eleven row offsets that make every row a lattice row, the column offset walking through the grid's edge columns."""
    cols = _edge_columns(X)
    return tuple((cols[k % len(cols)], oy) for k, oy in enumerate(ROW_OFFSETS))


# One entry = one family of scenes: EVERY kind x EVERY offset x EVERY configuration of it is a case. ``requires`` names what
# tests/test_impulse_cpu.py demands of the sites of each (kind, configuration) of the entry -- the lane requirement in the strip width of
# the kernel that configuration runs -- and of which no offset may be dropped without a loss.
PAIR_CONFIGS = ("dry_pairs", "dry_pairs_plain")
SWEEPS = (
    _sweep("lanes_wet", PHASE_GRID, WET_KINDS, itertools.product(LANE_OFFSETS_WET, ROW_OFFSETS), WET_CONFIGS, requires=("lanes",)),
    _sweep("lanes_dry", PHASE_GRID, DRY_KINDS, itertools.product(LANE_OFFSETS_DRY, ROW_OFFSETS), DRY_CONFIGS, requires=("lanes",)),
    _sweep("edges_wet", PHASE_GRID, WET_KINDS, _row_and_edge_offsets(PHASE_GRID[0])[:len(_edge_columns(PHASE_GRID[0]))], WET_CONFIGS, requires=("edges",)),
    _sweep("edges_dry", PHASE_GRID, DRY_KINDS, _row_and_edge_offsets(PHASE_GRID[0])[:len(_edge_columns(PHASE_GRID[0]))], DRY_CONFIGS, requires=("edges",)),
    # (the lane sweep reaches 54 of the 60 column phases of the one-iteration dry kernel; these three offsets add 21, 22, 34, 35, 36 and 47:
    # tests/test_impulse_cpu.py::test_phase_accounting_over_all_cases)
    _sweep("columns_dry", PHASE_GRID, DRY_KINDS, ((8, 1), (9, 5), (10, 9)), ("dry_single", "dry_single_plain")),
    _sweep("pair_55", PAIR_GRID_55, DRY_KINDS, _row_and_edge_offsets(PAIR_GRID_55[0]), PAIR_CONFIGS, requires=("rows", "edges")),
    _sweep("terrain", (505, 133), WET_KINDS, ((0, 1), (2, 5), (54, 9)), WET_CONFIGS, background="terrain"),  # (no requirement: a sample, outside the accounting)
    _sweep("bands_low", (2500, 300), ROW_KINDS_WET, _row_and_edge_offsets(2500), ("wet", "wet_pieces"), requires=("rows", "edges")),
    _sweep("bands_wide", (7990, 301), ("smoke", "wall", "fast_vx"), _row_and_edge_offsets(7990), ("wet",), requires=("rows", "edges")),
    _sweep("row_bands", (1100, 523), ROW_KINDS_WET, _row_and_edge_offsets(1100), ("wet_bands0", "wet_bands1", "wet_bands2"), requires=("rows", "edges")),
    _sweep("row_bands_dry", (1100, 523), ROW_KINDS_DRY, _row_and_edge_offsets(1100), ("dry_pairs_bands0", "dry_pairs_bands1", "dry_pairs_bands2"), requires=("rows",)),
    _sweep("droplets", (1100, 523), ("droplet",), ((1, 14), (5, 14), (8, 14), (1098, 27), (3, 3)), ("splat_atomic", "splat_atomic_perpass"),
           pitch=DROPLET_PITCH, requires=("splat_borders", "sprite_straddles")),
)


def cases():
    """Every (sweep name, grid, kind, pitch, offset, background, configuration) case, in a fixed order: the full product of each sweep.
    ``scene``: extra arguments of impulse_scene (the dry configurations plant DRY_FAST_VALUES)."""
    out = []
    for sw in SWEEPS:
        for off in sw["offsets"]:
            for kind in sw["kinds"]:
                for config in sw["configs"]:
                    c = {"sweep": sw["name"], "X": sw["grid"][0], "Y": sw["grid"][1], "kind": kind,
                         "pitch": list(sw["pitch"] or (DROPLET_PITCH if kind == "droplet" else PITCH)), "offset": [int(off[0]), int(off[1])],
                         "background": sw["background"], "config": config}
                    if config.startswith("dry") and kind in ("fast_vx", "fast_vy"):
                        c["scene"] = {"fast_values": list(DRY_FAST_VALUES)}
                    out.append(c)
    return out


def build_case(c, **kw):
    return impulse_scene(c["X"], c["Y"], c["kind"], pitch=c["pitch"], offset=c["offset"], background=c["background"], **dict(c.get("scene", {}), **kw))
