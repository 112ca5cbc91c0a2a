"""Blow-up scenes: the impulse lattice of tests/impulse_scenes.py with NON-FINITE and OVERFLOWING triggers -- the states the reference
reaches within a few brush strokes (it has no velocity clamp) and DESIGN.md section 3 defines: a float -> int conversion out of range is
the device's (NaN -> 0, saturated to INT_MIN / INT_MAX), then the modular wrap in 32-bit two's-complement arithmetic.

Three families, every one on a quiet background, one site per wavefront row (pitch 73 x 11):
  * NONFINITE_KINDS -- a NaN or an Inf planted in one channel of one cell. Compared under the contract: bit-identical where the oracle's
    value is finite, non-finite where the oracle's is (+Inf / -Inf by sign, NaN by being one).
  * HUGE_KINDS -- a FINITE velocity of 1e4 .. FLT_MAX cells / iteration. The back-trace lands on an integer position (the weights are
    exactly 0 / 1), so everything stays finite for an iteration and the family is compared bit for bit: the sharp one.
  * grown -- the 20 / 80 cells-per-iteration spikes on the WET state, which impulse_scenes leaves out because the state blows up: run
    until it does (tests/test_blowup_cpu.py asserts it happens inside the run).
Placements move the sites next to a planted wall cell (one / two cells away: the wall-aware interpolation replaces NaN weights by the
constants 0 / 1 there) and onto the first / second air row above the terrain. A plain module like impulse_scenes: pure numpy, no GPU.
"""
from __future__ import annotations

import numpy as np

import impulse_scenes as I

NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)
# finite speeds [cells / iteration]: far beyond 0.9, beyond any grid width, the last float below 2^31, 2^31 itself (the first that
# saturates), beyond 2^32, and where fragCoord - v has long lost every fraction bit
HUGE_VALUES = (1.0e4, 3.0e5, float(2 ** 31 - 128), float(2 ** 31), 3.0e9, 1.0e30, FLT_MAX)
# kind -> [(array, channel, value)]; a value of "+-" alternates +Inf / -Inf by site number
NONFINITE_KINDS = {
    "nan_vx": [("base", 0, NAN)], "nan_vy": [("base", 1, NAN)], "nan_both": [("base", 0, NAN), ("base", 1, NAN)], "inf_vx": [("base", 0, "+-")],
    "inf_vy": [("base", 1, "+-")], "nan_P": [("base", 2, NAN)], "nan_T": [("base", 3, NAN)], "inf_T": [("base", 3, "+-")],
    "nan_water0": [("water", 0, NAN)], "nan_water1": [("water", 1, NAN)], "nan_water2": [("water", 2, NAN)], "nan_water3": [("water", 3, NAN)],
}
HUGE_KINDS = ("huge_vx", "huge_vy")
KINDS = tuple(NONFINITE_KINDS) + HUGE_KINDS
# The water-free (dry) kernels never evaluate the water interpolation ("0 + t * (0 - 0) = 0 for finite weights"); with a NaN / Inf
# velocity the weights are NaN and the reference turns the zero water into NaN, which a water-free kernel cannot hold (DESIGN.md
# section 3). So on the water-free state the full contract is asked of the FINITE family (DRY_KINDS); the NaN kinds (DRY_NAN_KINDS) run
# through the same kernels compared wherever the oracle is FINITE -- where it routes a cell, and what a finite cell beside the NaN
# region computes, is pinned; what the device holds where the oracle has NaN is not. On a state that CARRIES water the dry pass mask
# runs the tiled kernel that stores water (wx_dry.h): every kind, full contract (``humid``).
DRY_KINDS = HUGE_KINDS
DRY_NAN_KINDS = ("nan_vx", "nan_vy", "nan_both", "nan_P", "nan_T")
PLACEMENTS = ("free", "wall1", "wall2")
_WALL_DIRS = ((1, 0), (-1, 0), (0, -1), (0, 1))


def site_value(kind, k):
    """What site ``k`` of a HUGE scene carries (sign by site number, magnitude walking through HUGE_VALUES)."""
    return (1.0 if k % 2 == 0 else -1.0) * HUGE_VALUES[(k // 2) % len(HUGE_VALUES)]


def blowup_scene(X, Y, kind, offset=(0, 1), background="air", placement="free", seed=1234, humid=False):
    """-> base, water, wall, drops (None), sites. The background and the lattice are impulse_scenes' (``background`` "air" / "terrain");
    ``placement``: "free" -- the lattice sites as they are; "wall1" / "wall2" -- a floating land cell planted one / two cells to the
    right of, left of, below, above the site (by site number); "surface" (terrain only) -- every site moved down its column onto the
    first (even sites) or second (odd sites) air row above the ground. ``humid``: 2 .. 2.06 g / kg of vapour in every air cell (by
    column: a wrong tap shows) -- a state that carries water, which the water-free kernels are not launched on."""
    if kind not in KINDS:
        raise ValueError(kind)
    base, water, wall, _, sites = I.impulse_scene(X, Y, "smoke", offset=offset, background=background, seed=seed, plant=False)
    if placement == "surface":
        if background != "terrain":
            raise ValueError("surface placement needs the terrain background")
        ground = (wall[..., 1] == 0).sum(0)
        rows = sorted({y for _, y in sites})
        sites = [(x, int(ground[x]) + k % 2) for k, (x, y) in enumerate(sites) if y == rows[len(rows) // 2] and ground[x] + 2 < Y]
    elif placement in ("wall1", "wall2"):
        d = int(placement[-1])
        keep = []
        for k, (x, y) in enumerate(sites):
            dx, dy = _WALL_DIRS[k % 4]
            wx_, wy = (x + d * dx) % X, y + d * dy
            if 1 <= wy < Y - 1 and wall[wy, wx_, 1] != 0 and wall[y, x, 1] > d:  # (free air around the site: the planted cell is THE wall next to it)
                I._plant_wall(base, water, wall, wx_, wy, 1, background == "air")
                keep.append((x, y))
        sites = keep
    elif placement != "free":
        raise ValueError(placement)
    if humid:
        air = wall[..., 1] != 0
        water[..., 0] = np.where(air, water[..., 0] + np.float32(2.0) + (np.arange(X) % 7).astype(np.float32)[None, :] * np.float32(0.01), water[..., 0])
    arrays = {"base": base, "water": water}
    for k, (x, y) in enumerate(sites):
        if kind in HUGE_KINDS:
            base[y, x, 0 if kind == "huge_vx" else 1] = site_value(kind, k)
        else:
            for name, ch, v in NONFINITE_KINDS[kind]:
                arrays[name][y, x, ch] = (INF if k % 2 == 0 else -INF) if v == "+-" else v
    return base, water, wall, None, sites


def droplet_scene(X, Y):
    """A pool of droplets with non-finite members over a quiet wet background with one NaN-velocity cell: records 0-5 have a NaN / +Inf /
    -Inf x position, a NaN y position, a NaN rain mass and an Inf snow mass; record 6 is an ordinary rain droplet INSIDE the NaN-velocity
    cell (its new position is NaN: it leaves no deposit), record 7 an ordinary one in quiet air. -> base, water, wall, drops, sites."""
    base, water, wall, _, _ = I.impulse_scene(X, Y, "smoke", background="air", plant=False)
    cx, cy = X // 2 + 3, Y // 2
    base[cy, cx, 0] = NAN
    drops = np.zeros((8, 5), np.float32)

    def pos(x, y):
        return ((x + 0.5) / X - 0.5) * 2.0, ((y + 0.5) / Y - 0.5) * 2.0
    qx, qy = pos(X // 4, Y // 2)
    drops[0] = (NAN, qy, 0.4, 0.0, 1.0)
    drops[1] = (INF, qy, 0.4, 0.0, 1.0)
    drops[2] = (-INF, qy, 0.4, 0.0, 1.0)
    drops[3] = (qx, NAN, 0.4, 0.0, 1.0)
    drops[4] = (qx, qy, NAN, 0.0, 1.0)
    drops[5] = (pos(X // 4 + 40, Y // 2)[0], qy, 0.0, INF, 0.3)
    drops[6] = pos(cx, cy) + (0.4, 0.0, 1.0)
    drops[7] = pos(3 * X // 4, Y // 2) + (0.4, 0.0, 1.0)
    return base, water, wall, drops, [(cx, cy)]


def grown_scene(X, Y, speed, background="air", offset=(3, 5)):
    """The spikes impulse_scenes keeps off the wet state: +-``speed`` cells / iteration (20 or 80) at every lattice site of the WET
    background. Nothing non-finite is planted; the oracle's state overflows within GROWN_ITERATIONS (tests/test_blowup_cpu.py)."""
    return I.impulse_scene(X, Y, "fast_vx", offset=offset, background=background, fast_values=(float(speed),))


GROWN_GRID = (505, 77)
GROWN_SPEEDS = (20.0, 80.0)
GROWN_ITERATIONS = 60  # the longest run a test makes: the first non-finite value appears earlier (asserted on the oracle)
GROWN_PAST = 5         # iterations compared past the first non-finite value


def scene_uniforms(Y, dry=False, wrap=True, precipitation=False):
    u = I.scene_uniforms("droplet" if precipitation else "smoke", Y, dry=dry)
    u["wrapHorizontally"] = 1 if wrap else 0
    return u


# ---- the contract ----
def contract_mismatch(a, b):
    """Boolean array: where ``a`` (the implementation) breaks the contract against ``b`` (the oracle). Floats: bit-identical where b is
    finite (so -0.0 != +0.0), NaN where b is NaN, the same infinity where b is infinite. Integers: equal."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != "f":
        return a != b
    bits_differ = a.view(np.uint32) != b.view(np.uint32)
    return np.where(np.isnan(b), ~np.isnan(a), bits_differ)


def describe(field, a, b, sites, X):
    bad = contract_mismatch(a, b)
    while bad.ndim > 2:
        bad = bad.any(-1)
    ys, xs = np.nonzero(bad)
    x, y = int(xs[0]), int(ys[0])
    s = I.nearest_site(sites, x, y, X) if sites else None
    return f"{field}: {int(contract_mismatch(a, b).sum())} values break the contract, first cell (x={x}, y={y}): {a[y, x]} against the oracle's {b[y, x]}; nearest site {s}"


# ---- the independent reference of the conversion (Python integers, no C) ----
def f2i_sat(v):
    """float32 -> int32 as the contract has it: NaN -> 0, saturating."""
    v = float(np.float32(v))
    if v != v:
        return 0
    if v >= 2.0 ** 31:
        return 2 ** 31 - 1
    if v <= -(2.0 ** 31):
        return -(2 ** 31)
    return int(v)  # (truncation; the callers pass floor values)


def add_wrap32(i, d):
    return (i + d + 2 ** 31) % 2 ** 32 - 2 ** 31


def tap_columns(x, v, X):
    """The two columns the back-trace of cell ``x`` with velocity ``v`` [cells / iteration] interpolates between, and the fraction, in
    float32 / Python-integer arithmetic: fragCoord = x + 0.5, st = fragCoord - v - 0.5, taps floor(st) and floor(st) + 1, each wrapped."""
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        st = f32(f32(f32(x) + f32(0.5)) - f32(v)) - f32(0.5)
        fl = np.floor(st)
        i0 = f2i_sat(fl)
        return i0 % X, add_wrap32(i0, 1) % X, float(f32(st - fl))


# ---- the case lists (shared by the CPU and the GPU file) ----
WET_CONFIGS = ("perpass", "wet", "wet_plain", "wet_stored", "wet_pieces")
DRY_CONFIGS = ("dry_perpass", "dry_single", "dry_single_plain", "dry_pairs", "dry_pairs_plain")
BAND_CONFIGS = ("wet_bands0", "wet_bands1", "wet_bands2")
# (tests/test_blowup_gpu.EXTRA_CONFIGS) the tiled dry kernel: on the water-free state (WX_OPT_DRY_KERNEL 0) and on a state that carries water
DRY_NAN_CONFIGS = ("dry_single", "dry_single_plain", "dry_pairs", "dry_pairs_plain", "dry_fused")
DRY_WATER_CONFIGS = ("dry_fused_water",)
PHASE_GRID = I.PHASE_GRID  # 505 x 77: X % 56 == 1, X % 60 == 25
# lattice offsets: with pitch 73 on 505 columns the sites of offsets 0 .. 4 meet the first three and the last three output lanes of a
# 56-column strip and an interior one (tests/test_impulse_cpu.py's accounting, reused by tests/test_blowup_cpu.py); 503 / 504: the
# edge columns X-2, X-1 (and 0, 1 through the offsets above)
OFFSETS = ((0, 1), (1, 4), (2, 7), (3, 10), (4, 2), (503, 5), (504, 8))
OFFSETS_DRY = OFFSETS + ((5, 3), (6, 6), (7, 9))


def cases():
    """Every case as a dict: grid, kind, offset, background, placement, wrap, the configurations that run it."""
    out = []
    X, Y = PHASE_GRID

    def add(kind, offset, background, placement, wrap, configs, grid=(X, Y), humid=False, compare="contract"):
        out.append({"X": grid[0], "Y": grid[1], "kind": kind, "offset": list(offset), "background": background, "placement": placement, "wrap": wrap,
                    "configs": list(configs), "humid": humid, "compare": compare})
    for kind in KINDS:
        wet_offsets = OFFSETS if kind in ("nan_vx", "huge_vx", "huge_vy", "nan_T") else OFFSETS[::3]
        for k, off in enumerate(wet_offsets):
            add(kind, off, "air", "free", k % 2 == 0, WET_CONFIGS)
        if kind in DRY_KINDS:
            for k, off in enumerate(OFFSETS_DRY if kind == "huge_vx" else OFFSETS_DRY[::3]):
                add(kind, off, "air", "free", k % 2 == 0, DRY_CONFIGS)
            add(kind, (2, 5), "air", "wall1", True, DRY_CONFIGS)
        if kind in DRY_NAN_KINDS:  # (compare "finite": wherever the oracle is finite)
            for k, off in enumerate(OFFSETS_DRY if kind == "nan_vx" else OFFSETS_DRY[::3]):
                add(kind, off, "air", "free", k % 2 == 0, DRY_NAN_CONFIGS, compare="finite")
            add(kind, (2, 5), "air", "wall1", True, DRY_NAN_CONFIGS, compare="finite")
            add(kind, (5, 8), "air", "wall2", True, DRY_NAN_CONFIGS, compare="finite")
        for k, (off, placement) in enumerate((((0, 2), "free"), ((504, 6), "free"), ((1, 3), "wall1"), ((4, 6), "wall2"))):
            add(kind, off, "air", placement, k != 1, DRY_WATER_CONFIGS, humid=True)
        for placement in ("wall1", "wall2"):
            add(kind, (1, 3) if placement == "wall1" else (4, 6), "air", placement, True, WET_CONFIGS)
        add(kind, (2, 5), "terrain", "free", True, WET_CONFIGS, grid=(505, 133))
        add(kind, (3, 1), "terrain", "surface", True, WET_CONFIGS, grid=(505, 133))
    for kind in ("nan_vx", "huge_vx", "nan_T"):
        add(kind, (1098, 7), "air", "free", True, BAND_CONFIGS, grid=(1100, 523))
    return out


def build_case(c):
    return blowup_scene(c["X"], c["Y"], c["kind"], offset=c["offset"], background=c["background"], placement=c["placement"], humid=c["humid"])


def case_id(c):
    return f"{c['kind']}-{c['background']}-{c['placement']}-{c['offset'][0]}.{c['offset'][1]}-{'wrap' if c['wrap'] else 'nowrap'}-{c['X']}x{c['Y']}{'-humid' if c['humid'] else ''}"
