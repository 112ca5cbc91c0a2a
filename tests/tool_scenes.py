"""Wall-tool scenes: the brush of advectionShader.frag:229-401 with a WALL tool (userInputType 10 .. 22, both signs of the intensity)
and the airplane crash (:444-457), held for one or three iterations over a background whose surface row repeats the seven surface
types, then released and stepped 20 iterations further -- in the manner of tests/surface_scenes.py, whose helpers it uses.

The background: stretches of four columns of inert, land, sea, fire, urban, runway, industrial (period 28: a disc of radius 15 holds
every type and leaves every type outside), three wall rows (two buried cells under every surface cell), vegetation 60 / 0 / 127 / 1 /
126 by x % 5, soil moisture 5 / 30 / 80 by x % 3, snow on two residues of x % 7. "stepped": the second column of every stretch one row
higher in the even periods, the third and fourth one row lower in the odd ones. (Two: a pit ONE cell wide whose floor a tool turns into land blows up within three iterations, in
the reference as in the oracle; blown-up states are tests/blowup_scenes.py's.)

A case is (tool, sign, placement, held). A placement puts the disc's rim, on the surface row, exactly between two columns -- so that
the last edited column and the first untouched one lie on either side of a strip seam of the marching kernels (56 columns wet and
pairs, 60 one-iteration dry), of the ragged last strip, of the wrap seam (wrap on and off: off, the disc is cut by the edge) and of
columns 0, 1, X-2, X-1. The case list is the full product; tests/test_tools_cpu.py accounts for what it reaches, tests/test_tools_gpu.py
runs it.
"""
from __future__ import annotations

import numpy as np

import impulse_scenes as I
import surface_scenes as S
import wxpkg

INERT, LAND, WATER, FIRE, URBAN, RUNWAY, INDUSTRIAL = range(7)
WALL_TOOLS = (10, 11, 12, 13, 14, 15, 16, 20, 21, 22)
SIGNS = (+1, -1)
HELD = (1, 3)
AFTER = 20
STRETCH, PERIOD = 4, 28
GROUND = S.GROUND  # 3 wall rows: the flat surface row is row 2
VEG = (60, 0, 127, 1, 126)
SOIL = (5.0, 30.0, 80.0)
INTENSITY = {20: 0.7, 21: 3.0}  # |intensity|: soil moisture moves by 10 x, snow by 0.5 x; the type tools read the sign only
GRID = (169, 52)  # 3 x 56 + 1: wet seams at 56 and 112, a ragged last strip of ONE column; one-iteration dry seams at 60 and 120, a ragged strip of 49
BANDS_GRID = S.BANDS_GRID
HALF_WIDTH = 15.0  # of the disc on the flat surface row, in cells: the rim falls on column boundaries at both ends
CENTRE_ROW = 3.3   # cells: row 0 is inside (a removal must leave it), and so are the raised and the lowered surface cells
RIM_MARGIN = 1e-5
VARIANTS = ("flat", "stepped")


def column_types(X):
    return (np.arange(X) % PERIOD) // STRETCH


def heights(X, variant):
    h = np.full(X, GROUND, np.int64)
    if variant == "stepped":
        x = np.arange(X)
        even = (x // PERIOD) % 2 == 0
        h[even & (x % STRETCH == 1)] = GROUND + 1          # every type raised in the even periods ...
        h[~even & (x % STRETCH >= 2)] = GROUND - 1         # ... and lowered, two columns wide, in the odd ones
        h[x >= (X // PERIOD) * PERIOD] = GROUND            # (the incomplete last period stays flat: nothing odd across the wrap seam)
    elif variant != "flat":
        raise ValueError(variant)
    return h


def background(X, Y, variant="flat", seed=1234, dry=False):
    """-> base, water, wall, h. surface_scenes.background's air (at rest on the start sounding, a slow random flow) over the typed
    terrain, with the wall bytes the boundary pass keeps. ``dry``: the water-free state the water-free kernels need -- no vapour, no
    soil moisture, no snow, no vegetation."""
    base, water, wall, _ = S.background(X, Y, "flat", seed)
    h, t, x = heights(X, variant), column_types(X), np.arange(X)
    yy = np.arange(Y)[:, None]
    is_wall = yy < h[None, :]
    for c in np.nonzero(h < GROUND)[0]:  # a lowered column: the cell above its new surface takes the air of the cell above
        base[h[c]:GROUND, c], water[h[c]:GROUND, c] = base[GROUND, c], water[GROUND, c]
    sea = (t == WATER)[None, :] & is_wall
    base[..., :3] = np.where(is_wall[..., None], np.float32(0.0), base[..., :3])
    base[..., 3] = np.where(is_wall, np.where(sea, np.float32(288.15), np.float32(1000.0)), base[..., 3])
    water[..., 0] = np.where(is_wall, np.where(sea, np.float32(1002.0), np.float32(1001.0)), water[..., 0])
    water[..., 1] = np.where(is_wall, np.float32(0.0), water[..., 1])
    soil = np.array(SOIL, np.float32)[x % 3]
    snow = np.where(x % 7 == 0, 6.0, np.where(x % 7 == 3, 1.0, 0.0)).astype(np.float32)
    water[..., 2] = np.where(is_wall, np.where(sea, np.float32(100.0), soil[None, :]), water[..., 2])
    water[..., 3] = np.where(is_wall, np.where(sea, np.float32(0.0), snow[None, :]), water[..., 3])
    wall[..., 0] = t[None, :]
    vdist = yy - h[None, :] + 1
    wall[..., 2] = np.clip(vdist, -127, 127).astype(np.int8)
    wall[..., 3] = np.where(is_wall, np.array(VEG)[x % 5][None, :], 0).astype(np.int8)
    dist = np.where(is_wall, 0, vdist)
    for dx in (-2, -1, 1, 2):
        hn = np.roll(h, -dx)
        dist = np.minimum(dist, np.where(is_wall, 0, np.maximum(yy - hn[None, :] + 1, 0) + abs(dx)))
    wall[..., 1] = np.clip(dist, 0, 127).astype(np.int8)
    if dry:
        water[...] = np.where(is_wall[..., None], water * np.float32([1, 0, 0, 0]), np.float32(0.0))
        wall[..., 3] = 0
    return base, water, wall, h


# ---- placements ----
def placements(X):
    """name -> (left rim, wrap). The disc covers the surface columns [left, left + 30) (mod X with the wrap on; cut by the edge with
    it off): column left - 1 is the last one outside, left + 29 the last one inside."""
    w = 2 * int(HALF_WIDTH)
    wet, dry = I.WET_STRIP, I.DRY_STRIP
    ragged_wet, ragged_dry = (X // wet) * wet, (X // dry) * dry
    p = {"right@dry_seam": (dry - w, True), "left@wet_seam": (wet, True), "right@ragged_dry": (ragged_dry - w, True),
         "right@ragged_wet": (ragged_wet - w, True), "right@wrap": (X - w, True), "right@col0|1": (X - w + 1, True), "right@col1|2": (X - w + 2, True),
         "left@wrap": (0, True), "left@col0|1": (1, True), "left@X-2|X-1": (X - 1, True),
         "nowrap_right@X-2|X-1": (X - w - 1, False), "nowrap_right@edge": (X - w, False), "nowrap_cut_right": (X - w + 1, False),
         "nowrap_left@col0|1": (1, False), "nowrap_left@edge": (0, False), "nowrap_cut_left": (-1, False)}
    return p


def texcoords(X, Y):
    f = np.float32
    return ((np.arange(X, dtype=f) + f(0.5)) / f(X))[None, :], ((np.arange(Y, dtype=f) + f(0.5)) / f(Y))[:, None]


def brush_distance(X, Y, values, wrap):
    """advectionShader.frag:239-249 in float32: -> distance in texCoord.y units, radius."""
    f = np.float32
    tcx, tcy = texcoords(X, Y)
    a = f(values[0])
    dx = np.abs(a - tcx)
    if wrap:
        dx = np.minimum(np.minimum(dx, np.abs(f(1.0) + a - tcx)), f(1.0) - a + tcx)
    dx = dx * (f(1.0 / Y) / f(1.0 / X))
    dy = f(values[1]) - tcy
    return np.sqrt(dx * dx + dy * dy, dtype=f), f(values[3]) * f(1.0 / Y)


def rim_clear(X, Y, values, wrap):
    d, r = brush_distance(X, Y, values, wrap)
    return bool((np.abs(d.astype(np.float64) - float(r)) > RIM_MARGIN * float(r)).all())


def inside(X, Y, values, wrap):
    d, r = brush_distance(X, Y, values, wrap)
    return d < r


def brush_values(X, Y, left, wrap, inten, hw=HALF_WIDTH):
    """userInputValues of the placement: the radius grown in steps of 1e-3 cells until no cell lies within RIM_MARGIN of the rim."""
    dy = CENTRE_ROW - (GROUND - 0.5)
    for k in range(200):
        r = float(np.hypot(hw, dy)) + 1e-3 * k
        v = tuple(float(np.float32(c)) for c in ((left + hw) % X / X if wrap else (left + hw) / X, CENTRE_ROW / Y, inten, r))
        if rim_clear(X, Y, v, wrap):
            return v
    raise RuntimeError("no clear rim")


def scene_uniforms(Y, wrap=True, dry=False):
    P = wxpkg.load_package().params
    u = S.scene_uniforms(Y, wrap=wrap)
    if dry:
        u["pass_mask"] = P.PASS_DRY
    return u


def tool_uniforms(c, dry=False):
    """-> uniforms while the tool is held, uniforms after release. A case may name its disc itself: "left" (the first surface column
    inside, wrap on) and "hw" (half width) in place of "placement"."""
    left, wrap = (c["left"], True) if "left" in c else placements(c["X"])[c["placement"]]
    u = scene_uniforms(c["Y"], wrap=wrap, dry=dry)
    inten = c["sign"] * INTENSITY.get(c["tool"], 0.01)
    held = dict(u, userInputType=c["tool"], userInputValues=brush_values(c["X"], c["Y"], left, wrap, inten, c.get("hw", HALF_WIDTH)), userInputMove=(0.0, 0.0))
    return held, dict(held, userInputType=-1)


# ---- the case list: the full product ----
# kernel configuration (tools/fuzz_parity.IMPULSE_CONFIGS) by position in the product, so that every (tool, sign) meets every one:
# the LAST held iteration is a display iteration ("wet": the held iterations are one step), a WX_OVERLAP_MORE_TO_COME piece followed by
# plain ones ("wet_pieces", held 3), with waterTexture_0 stored, on the per-pass kernels
CONFIG_CYCLE = ("wet", "wet_stored", "perpass", "wet_pieces", "wet_plain")
ITER0 = 990  # 1000 -- fire spread where the divisor is 10 -- falls into the 20 iterations after release


def cases(grid=GRID):
    out = []
    X, Y = grid
    for ti, tool in enumerate(WALL_TOOLS):
        for si, sign in enumerate(SIGNS):
            for pi, name in enumerate(placements(X)):
                for hi, held in enumerate(HELD):
                    out.append({"X": X, "Y": Y, "tool": tool, "sign": sign, "placement": name, "held": held, "variant": VARIANTS[(pi + hi) % 2],
                                "config": CONFIG_CYCLE[(ti + si + pi + 2 * hi) % len(CONFIG_CYCLE)]})
    return out


def build_case(c, dry=False):
    return background(c["X"], c["Y"], c["variant"], dry=dry)


def cell_classes(wall):
    """name -> mask, as tests/test_oracle_tools.cell_classes: the surface cell of every type, buried wall cells, air."""
    is_wall = wall[..., 1] == 0
    above_air = np.roll(wall[..., 1], -1, axis=0) != 0
    c = {f"surface_{t}": is_wall & above_air & (wall[..., 0] == t) for t in range(7)}
    c["buried"] = is_wall & ~above_air
    c["air"] = ~is_wall
    return c


# ---- the crash ----
def crash_values(X, Y, x, y):
    return ((x + 0.5) / X, (y + 0.5) / Y, 0.0, 1.0)


NO_PLANE = (0.0, 0.0, 0.0, 0.0)


# ---- the runner ----
def run_case(pkg, fuzz, oracle, c, after=AFTER, iter0=ITER0):
    """One case on a handle configured as tools/fuzz_parity.IMPULSE_CONFIGS[c["config"]] against the oracle, bit for bit on every grid
    field after the held iterations and ``after`` iterations after release. -> mismatches, the oracle's wall texture after the held
    iterations and at the end."""
    base, water, wall, _ = build_case(c)
    cfg = fuzz.IMPULSE_CONFIGS[c["config"]]
    held_u, free_u = tool_uniforms(c)
    X, Y = c["X"], c["Y"]
    h, o = pkg.engine.Handle(X, Y, 0), oracle.OracleSim(X, Y, 0)
    bad, walls = [], []
    try:
        h.upload(base, water, wall)
        o.upload(base, water, wall)
        h.iter = o.iter = iter0
        h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
        h.set_option(h.OPT_ROW_BANDS, c.get("bands", cfg.get("bands", 1)))
        h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
        for u, n in ((held_u, c["held"]), (free_u, after)):
            h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
            o.set_params(u)
            if cfg.get("pieces") and n > 1:
                h.step(1, 4)
                h.step(n - 1)
            elif c["config"] == "wet_plain" and n > 2:  # the tool's last iteration inside a step would need a release inside it: the FIRST held ones are plain
                h.step(n - 1)
                h.step(1)
            else:
                h.step(n)
            o.step(n)
            walls.append(o.field("WALL_CUR"))
            for f in fuzz.GRID_FIELDS:
                a, b = h.read_rect(f), o.field(f)
                if not np.array_equal(a, b):
                    bad.append({"field": f, "after": "held" if u is held_u else "release", "cells": int((a != b).any(-1).sum()),
                                "first": [int(v) for v in np.argwhere((a != b).any(-1))[0]]})
            if bad:
                break
        assert h.iter == o.iter
        return bad, walls
    finally:
        h.close()
        o.close()
