"""Scenes and case lists of the velocity-watch tests (tests/test_vx_watch_cpu.py accounts for them on the oracle,
tests/test_vx_watch_gpu.py runs them on the card). Plain numpy on top of tests/impulse_scenes.py: no fixture, no GPU.

The watch (VxTrack, csrc/wx_tile.h) keeps the largest |vx| the marching kernels produce INSIDE an iteration -- the post-boundary
velocity of the wet kernel, the velocity pass's output of the dry ones -- and wx_slab_vx_take hands it out (0 below 0.5). The oracle
supplies that intermediate through its pass mask: from its state before iteration k a throw-away OracleSim steps once with the mask
of the family (STAGE below) and max |BASE_CUR[..., 0]| is what the kernel must have recorded, bit for bit. Kernels that do not track
(per-pass set, tiled dry kernel) leave the state to a scan at take time: the oracle's BASE_CUR after the last iteration.

A scene is the quiet background of impulse_scenes (air over an inert floor, a flow of 0.05 cells / iteration) plus ONE planted cell.
"""
from __future__ import annotations

import numpy as np

import impulse_scenes as I

HALF = np.float32(0.5)
SMALL, PHASE, BANDS = (169, 52), I.PHASE_GRID, (2500, 300)  # 169 = 3 x 56 + 1 = 2 x 60 + 49: a ragged last strip for both strip widths

# ---- kernel families: how a handle is configured (tools/fuzz_parity.py's options) and stepped ----
# calls: (iterations, wx_step_overlap flags) per call; stage: the oracle's pass mask of the measured velocity (None: the state is
# scanned at take time); strip: output columns per wave; kernel: what the "once per kernel family" assertions group by.
FAMILIES = {
    "wet_display": {"dry": False, "kernel": "wet", "strip": I.WET_STRIP, "stage": 7, "calls": ((1, 0),)},        # the trigger meets the iteration that stores the display fields
    "wet_plain": {"dry": False, "kernel": "wet", "strip": I.WET_STRIP, "stage": 7, "calls": ((2, 0),)},          # ... a plain iteration (the second one displays)
    "wet_piece": {"dry": False, "kernel": "wet", "strip": I.WET_STRIP, "stage": 7, "calls": ((1, 4),)},          # ... a WX_OVERLAP_MORE_TO_COME piece
    "dry_single": {"dry": True, "kernel": "dry1", "strip": I.DRY_STRIP, "stage": 1, "pairs": 0, "calls": ((1, 0),)},
    "dry_pairs_taint": {"dry": True, "kernel": "dry2", "strip": I.PAIR_STRIP, "stage": 1, "pairs": 1, "calls": ((2, 0),)},  # a fresh handle: TAINT
    "dry_pairs_plain": {"dry": True, "kernel": "dry2", "strip": I.PAIR_STRIP, "stage": 1, "pairs": 1, "calls": ((2, 0),), "prime": True},
    "perpass": {"dry": False, "kernel": "scan", "strip": None, "stage": None, "kernel_set": 0, "calls": ((1, 0),)},
    "dry_tiled": {"dry": True, "kernel": "scan", "strip": None, "stage": None, "pairs": 0, "dry_kernel": 0, "calls": ((1, 0),)},
}
LANE_GROUPS = ("domain_edges", "first_lanes", "last_lanes", "interior", "ragged")
SIGNED = (1.3, -1.3, 3.0, -3.0, 7.5, -7.5)
# the scan families look at the state AFTER the iteration: a lone spike loses nine tenths of its speed to the pressure step, so only
# these are still beyond 0.5 there (the CPU file asserts it)
SECOND_ITERATION_SPIKE = 0.9  # a pressure spike: |vx| ~ 0.88 next to it in the first iteration, ~ 1.4 in the second
SIGNED_SCAN = {"perpass": (20.0, -20.0), "dry_tiled": (40.0, -40.0)}


def lane_columns(X, strip):
    """group -> columns: the domain's edge columns; output lanes 0, 1, 2 and the last three of a whole strip (the second one: strip 0's
    first lanes are the domain's edge); one interior lane; the first and the last column of the ragged last strip."""
    out = {"domain_edges": (0, 1, X - 2, X - 1)}
    if strip is None:
        out["interior"] = (X // 2,)
        return out
    out["first_lanes"] = (strip, strip + 1, strip + 2)
    out["last_lanes"] = (2 * strip - 3, 2 * strip - 2, 2 * strip - 1)
    out["interior"] = (strip + strip // 2,)
    if X % strip > 1:  # (its last column is X - 1, an edge column already; a ragged strip of ONE column is that column)
        out["ragged"] = ((X // strip) * strip,)
    return out


def dry_segments(X, Y, strip):
    """Row segments [lo, hi) of the two dry marching kernels on a LOW grid whose height is no multiple of 8 (no row bands): both launch
    functions take their minimum of 8 rows per segment, whatever the device (tests/test_vx_watch_cpu.py holds this to march_seg_rows
    through a host-only harness and to launch_march_dry2's arithmetic, the wet kernel's segments to the launch-shape harness)."""
    assert Y % 8 != 0 and Y < 8 * 3 * 8 and ((X + strip - 1) // strip) * Y < 4096
    return [(lo, min(lo + 8, Y)) for lo in range(0, Y, 8)]


# rows 1 and Y-2, the last row of a segment and the first of the next -- for the 8-row segments of the dry kernels (7 | 8) and for the
# 2-row segments of the wet kernel on these grids (every odd row is a last, every even one a first)
ROWS = {SMALL: (1, 7, 8, 50), PHASE: (38,)}

# The wet kernel's row segments on 2500 x 300 under the three WX_OPT_ROW_BANDS modes, as literals (tests/test_vx_watch_cpu.py compares
# them with the launch-shape harness): mode 0 cuts the whole height into one table of segments; modes 1 and 2 cut it into eight row bands
# [k Y / 8, (k + 1) Y / 8) of 37 or 38 rows, each into the same table of segments counted from the band's first row and clipped to the band.
BAND_TABLES = {
    0: (False, (0, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 60, 65, 70, 75, 80, 85, 90, 95, 100, 105, 110, 115, 120, 125, 130, 135, 140, 145, 150, 155, 160, 163, 165, 168, 170, 173, 175, 178, 180, 183, 185, 188, 190, 193, 195, 198, 200, 203, 205, 208, 210, 213, 215, 218, 220, 223, 225, 228, 230, 233, 235, 238, 241, 242, 243, 244, 246, 247, 248, 249, 251, 252, 253, 254, 256, 257, 258, 259, 261, 262, 263, 264, 266, 267, 268, 269, 271, 272, 273, 274, 276, 277, 278, 279, 281, 282, 283, 284, 285, 286, 287, 288, 289, 290, 291, 292, 293, 294, 295, 296, 297, 298, 299, 300)),
    1: (True, (0, 4, 9, 13, 17, 21, 26, 30, 34, 36, 37, 38)),
    2: (True, (0, 4, 9, 13, 17, 21, 26, 30, 34, 36, 37, 38)),
}
BAND_COLUMNS = (BANDS[0] - 1, 0, 1, 55, 56, 1250, 2463, 2464)  # the domain's edges, a strip border, an interior lane, the ragged strip's border (44 x 56 = 2464)


def band_segments(mode, Y=BANDS[1]):
    """Row segments [lo, hi) of the wet kernel on the band grid under a ROW_BANDS mode, absolute rows, empty ones dropped."""
    banded, starts = BAND_TABLES[mode]
    if not banded:
        return [(lo, hi) for lo, hi in zip(starts, starts[1:])]
    out = []
    for k in range(8):
        b_lo, b_hi = k * Y // 8, (k + 1) * Y // 8
        out += [(b_lo + lo, min(b_lo + hi, b_hi)) for lo, hi in zip(starts, starts[1:]) if b_lo + lo < b_hi]
    return out


def band_border_rows(mode, Y=BANDS[1]):
    """Every row that is the last row of a segment or the first row of the next one, for every border between two segments (but the
    floor row 0 and the top row Y-1, the domain's edge rows: the lists of part A plant in rows 1 .. Y-2)."""
    rows = set()
    for lo, hi in band_segments(mode, Y):
        if lo > 0:
            rows |= {lo - 1, lo}
    return sorted(r for r in rows if 1 <= r <= Y - 2)


def value_cases():
    """A.values: both signs of 1.3, 3.0 and 7.5 go round the lane x row product (whole_cases); these are the cases of their own."""
    return ({"name": "vy_only", "vx": 0.0, "vy": 3.0}, {"name": "below_half", "pair": "half", "side": 0}, {"name": "above_half", "pair": "half", "side": 1})


def whole_cases():
    """Part A: every (family, column, row, value) case on whole-domain handles, in a fixed order. 169 x 52: every column of every lane
    group x every row of ROWS, the six signed values going round so that every column meets both signs and every family every value;
    505 x 77: one case per family; 2500 x 300: under each band mode one case per row next to a segment border of the wet kernel,
    and one case of the pair kernel."""
    out = []
    X, Y = SMALL
    for fam, f in FAMILIES.items():
        vals = SIGNED if f["stage"] is not None else SIGNED_SCAN[fam]
        rows = ROWS[SMALL] if f["strip"] else (1, Y - 2)
        k = 0
        for group, cols in lane_columns(X, f["strip"]).items():
            for x in cols:
                for y in rows:
                    out.append({"family": fam, "X": X, "Y": Y, "x": x, "y": y, "vx": vals[k % len(vals)], "vy": 0.0, "group": group})
                    k += 1
        for v in value_cases():
            if f["stage"] is None and "pair" in v:
                continue  # (the scan's comparison is exact: its 0.5 is an uploaded value, test_scan_compares_exactly)
            c = {"family": fam, "X": X, "Y": Y, "x": X // 2 + 3, "y": 20, "vx": 0.0, "vy": 0.0, "group": v["name"]}
            if "pair" in v:
                c["vx"] = STRADDLES[(v["pair"], f["stage"])][v["side"]]
            else:
                c["vx"], c["vy"] = v["vx"], v["vy"]
            out.append(c)
        if f["kernel"] == "dry2":  # the pair kernel's SECOND iteration at the lanes next to a strip border: a pressure spike, whose flow is faster
            # in the second iteration than in the first (a planted vx only slows down: its first iteration would hide the second)
            w = f["strip"]
            for k, x in enumerate((w, w + 1, w + 2, w + 3, 2 * w - 4, 2 * w - 3, 2 * w - 2, 2 * w - 1)):
                out.append({"family": fam, "X": X, "Y": Y, "x": x, "y": (8, 20)[k % 2], "vx": 0.0, "vy": 0.0, "dP": SECOND_ITERATION_SPIKE, "group": "second_iteration"})
    X, Y = PHASE
    for fam, f in FAMILIES.items():
        # (the scan families: next to the floor, where a spike keeps more of its speed over a whole iteration)
        out.append({"family": fam, "X": X, "Y": Y, "x": X - 1, "y": ROWS[PHASE][0] if f["stage"] is not None else 1,
                    "vx": -3.0 if f["stage"] is not None else SIGNED_SCAN[fam][0], "vy": 0.0, "group": "phase_grid"})
    X, Y = BANDS
    for mode in (0, 1, 2):  # the wet kernel: one lone cell in every row next to a border between two segments, the columns and values going round
        for k, y in enumerate(band_border_rows(mode)):
            out.append({"family": "wet_display", "X": X, "Y": Y, "x": BAND_COLUMNS[k % len(BAND_COLUMNS)], "y": y, "vx": SIGNED[k % len(SIGNED)], "vy": 0.0,
                        "group": "bands%d" % mode, "bands": mode})
        out.append({"family": "dry_pairs_taint", "X": X, "Y": Y, "x": X - 1, "y": 112, "vx": 3.0, "vy": 0.0, "group": "bands%d" % mode, "bands": mode})
    return out


def background(X, Y):
    base, water, wall, _, _ = I.impulse_scene(X, Y, "fast_vx", plant=False)
    return base, water, wall


def whole_scene(c, bg=None):
    """-> base, water, wall of a part-A case (``bg``: the background of its grid, left unchanged)."""
    base, water, wall = bg if bg is not None else background(c["X"], c["Y"])
    base = base.copy()
    if c["vx"] != 0.0:
        base[c["y"], c["x"], 0] = c["vx"]
    if c["vy"] != 0.0:
        base[c["y"], c["x"], 1] = c["vy"]
    if c.get("dP"):
        base[c["y"], c["x"], 2] += np.float32(c["dP"])
    return base, water, wall


def uniforms(family, Y):
    return I.scene_uniforms("fast_vx", Y, dry=FAMILIES[family]["dry"])


def stage_vx(wx_oracle, o, u, stage):
    """|vx| of the measured stage of the iteration the oracle ``o`` is about to run, [Y, X] float32 (``o`` is left alone)."""
    t = wx_oracle.OracleSim(o.X, o.Y, 0, X_global=o.X_global, x_off=o.x_off)
    try:
        t.upload(o.field("BASE_CUR"), o.field("WATER_CUR"), o.field("WALL_CUR"))
        t.set_params(dict(u, pass_mask=stage, enablePrecipitation=0))
        t.iter = o.iter
        t.step(1)
        return np.abs(t.field("BASE_CUR")[..., 0])
    finally:
        t.close()


def reference(wx_oracle, scene, u, family, calls=None, X_global=None, x_off=0):
    """What the watch of ``family`` must have seen over ``calls`` (default: the family's) from the uploaded ``scene``:
    -> (per-iteration [Y, X] arrays of the measured |vx|, the oracle's BASE_CUR after the last iteration). For the scan families the
    list holds one array: |vx| of the final state."""
    f = FAMILIES[family]
    base, water, wall = scene
    Y, X = base.shape[:2]
    o = wx_oracle.OracleSim(X, Y, 0, X_global=X_global, x_off=x_off)
    try:
        o.upload(base, water, wall)
        o.set_params(u)
        o.iter = 0
        seen = []
        for n, _ in (calls or f["calls"]):
            for _ in range(n):
                if f["stage"] is not None:
                    seen.append(stage_vx(wx_oracle, o, u, f["stage"]))
                o.step(1)
        final = o.field("BASE_CUR")
        if f["stage"] is None:
            seen = [np.abs(final[..., 0])]
        return seen, final
    finally:
        o.close()


def expected_take(seen, columns=None):  # columns: None, or one index array per iteration
    """The float32 wx_slab_vx_take must return: the maximum over the iterations (over ``columns`` of each), 0.0 below 0.5."""
    m = np.float32(0.0)
    for j, a in enumerate(seen):
        m = max(m, np.float32((a if columns is None else a[:, columns[j]]).max()))
    return np.float32(m) if m >= HALF else np.float32(0.0)


def bits(v):
    return int(np.float32(v).view(np.int32))


# ---- part B: lone slab handles ----
SLAB = {"X_owned": 256, "X_global": 512, "halo": 12, "Y": 40, "x0s": (0, 256)}
SLAB_LOCAL = SLAB["X_owned"] + 2 * SLAB["halo"]  # 280 columns: five strips of 56 (0 .. 4), five of 60 (the last one ragged)
MUST_SEE = (8, 35, 244, 271)     # local columns inside the contract's zone (c < 3 * halo or c >= 280 - 3 * halo), not in the outermost cone
NEVER_RECORDED = (64, 140, 215)  # one column in each unwatched strip (1, 2, 3), for 56- and for 60-column strips alike
SLAB_FAMILIES = tuple(FAMILIES)  # every family of part A runs on a lone slab (wet_plain and the pairs: the two iterations of the period)
INTERIOR_LIMIT = float(max(1, 2 * SLAB["halo"] - 8))  # 16 cells / iteration


def zone_class(c, halo=SLAB["halo"], X=SLAB_LOCAL, cone=6):
    """must_see | never | either | ghost_front (the outermost ``cone`` columns, never compared) of a local column, for BOTH strip widths."""
    if c < cone or c >= X - cone:
        return "ghost_front"
    if c < 3 * halo or c >= X - 3 * halo:
        return "must_see"
    for w in (I.WET_STRIP, I.DRY_STRIP):
        zl, zr = (3 * halo + w - 1) // w, (X - 3 * halo) // w
        if not zl <= c // w < zr:
            return "either"
        # (a watched wave sees the columns it loads beyond its strip too: 4 on either side in the wet and in the pair kernel, 2 in the
        # one-iteration dry kernel; twice that is left out here)
        reach = 8 if w == I.WET_STRIP else 4
        if c - reach < zl * w or c + reach >= zr * w:
            return "either"
    return "never"


def slab_window(x0):
    """Global columns of the local array of the slab that owns [x0, x0 + X_owned)."""
    return (x0 - SLAB["halo"] + np.arange(SLAB_LOCAL)) % SLAB["X_global"]


def slab_scene(c_local, x0, vx):
    """-> whole-domain (base, water, wall) with ONE cell planted at local column ``c_local`` of the slab at x0, row 20."""
    base, water, wall = background(SLAB["X_global"], SLAB["Y"])
    base = base.copy()
    base[20, slab_window(x0)[c_local], 0] = vx
    return base, water, wall


def slab_cases():
    """Part B's lone sites: (family, local column, x0, planted vx, class); the x0 and the sign alternate along each list."""
    out = []
    for fam in SLAB_FAMILIES:
        vals = SIGNED if FAMILIES[fam]["stage"] is not None else SIGNED_SCAN[fam]
        for k, c in enumerate(MUST_SEE + NEVER_RECORDED):
            out.append({"family": fam, "c": c, "x0": SLAB["x0s"][k % 2], "vx": vals[(k + 2) % len(vals)], "class": zone_class(c)})
    return out


# ---- straddling pairs (tools/find_watch_straddles.py prints them; kept as literals) ----
# (threshold name, stage) -> (planted vx whose measured-stage value is just below the threshold, ... just at or above it). "half": part
# A's straddle site on 169 x 52; "period", "period7", "interior": part B's, at MUST_SEE[1] / NEVER_RECORDED[1] of the slab at x0 = 0.
STRADDLES = {
    ("half", 7): (0.5796446204185486, 0.5796446800231934),
    ("half", 1): (0.5000000596046448, 0.5000001192092896),
    ("period", 7): (5.822981834411621, 5.822982311248779),
    ("period", 1): (1.0000001192092896, 1.000000238418579),
    ("period7", 7): (6.502232074737549, 6.502232551574707),
    ("period7", 1): (2.000000238418579, 2.000000476837158),
    ("interior", 7): (11.738944053649902, 11.738945007324219),
    ("interior", 1): (16.000001907348633, 16.000003814697266),
}
STRADDLE_SITES = {"half": ("whole", SMALL[0] // 2 + 3, 20, 0.5), "period": ("slab", MUST_SEE[1], 20, 1.0), "period7": ("slab", MUST_SEE[1], 20, 2.0),
                  "interior": ("slab", NEVER_RECORDED[1], 20, INTERIOR_LIMIT)}


def straddle_scene(name, vx):
    kind, x, y, _ = STRADDLE_SITES[name]
    if kind == "whole":
        return whole_scene({"X": SMALL[0], "Y": SMALL[1], "x": x, "y": y, "vx": vx, "vy": 0.0})
    return slab_scene(x, 0, vx)


def straddle_measured(wx_oracle, name, stage, vx):
    """The measured-stage |vx| maximum of the first iteration of a straddle scene (slabs: the oracle runs the whole domain)."""
    kind = STRADDLE_SITES[name][0]
    scene = straddle_scene(name, vx)
    Y = scene[0].shape[0]
    u = I.scene_uniforms("fast_vx", Y, dry=stage == 1)
    o = wx_oracle.OracleSim(scene[0].shape[1], Y, 0)
    try:
        o.upload(*scene)
        o.set_params(u)
        o.iter = 0
        a = stage_vx(wx_oracle, o, u, stage)
    finally:
        o.close()
    return np.float32(a.max()) if kind == "whole" else np.float32(a[:, slab_window(0)].max())


def valid_columns(n_iterations):
    """Per iteration of a period that started with fresh ghost columns: the local columns whose measured-stage velocity a lone slab
    computes exactly (iteration j has lost 6 j columns per side to the front of invalid ghost columns; the stage itself reaches up to
    4 columns further: velocity, curl, vorticity and boundary pass of the wet kernel)."""
    return [np.arange(6 * j + 4, SLAB_LOCAL - 6 * j - 4) for j in range(n_iterations)]


def scan_zone_columns():
    """The columns k_vx_scan records on a slab (the contract's zone, in columns) that one iteration has left exact."""
    h = SLAB["halo"]
    return [np.concatenate([np.arange(6, 3 * h), np.arange(SLAB_LOCAL - 3 * h, SLAB_LOCAL - 6)])]


def slab_local_oracle(wx_oracle, scene, x0, u, family):
    """What the slab itself computes, ghost front included: the oracle on the LOCAL array, periodic across its 280 columns like the
    kernels' loads (-> reference()'s list, in local columns). Only to show that the columns left out of the comparison stay quiet."""
    idx = slab_window(x0)
    local = tuple(np.ascontiguousarray(a[:, idx]) for a in scene)
    return reference(wx_oracle, local, u, family)[0]


# ---- the dry pair kernel's exact paths: the planted 20 / 80 spikes of impulse_scenes.DRY_FAST_VALUES on 505 x 77 ----
SPIKED_OFFSET = (0, 1)  # with this lattice the pair of iterations 3 and 4 is faster in its SECOND iteration (tests/test_vx_watch_cpu.py)


# ---- part D: the ring protocol ----
RING = {"X": 1024, "Y": 64, "halo": 42, "slabs": 2, "iterations": 30, "offsets": (50, 126)}


def ring_scene(wet):
    """-> (base, water, wall), uniforms: the quiet background with one broad jet per slab, between one and two halo widths inside the
    slab's left edge and moving inwards -- a 6 x 2 core of 2.4 cells / iteration over a block of 1.5."""
    X, Y = RING["X"], RING["Y"]
    base, water, wall = background(X, Y)
    base = base.copy()
    xo = X // RING["slabs"]
    for b in range(RING["slabs"]):
        x = b * xo + RING["offsets"][0]
        base[RING_BLOCK[0]:RING_BLOCK[1], x:x + RING_BLOCK[2], 0] = 1.5
        base[36:38, x:x + 6, 0] = 2.4
    return (base, water, wall), I.scene_uniforms("fast_vx", Y, dry=not wet)


RING_BLOCK = (33, 41, 16)  # rows [33, 41), 16 columns


# ---- part C: the sizing arithmetic, restated from the text of include/wxsim.h ----
def sizing(v, halo, particles=False):
    """-> (cone, period, refused), one numpy operation per rounded operation: the coming period assumes |vx| < 1.25 v + 0.25;
    cone = 6 + floor(that) once it reaches 1 (+Inf counts as +Inf); period = halo / cone
    iterations -- with particles cone columns for the first iteration, cone + 3 for every further one, cone + 1 kept in the last:
    min(15, 1 + (halo - 2 cone - 1) / (cone + 3)). Refused (WX_E_STATE) where cone > halo, with particles where 2 cone + 1 > halo."""
    bound = np.float32(np.float32(v) * np.float32(1.25)) + np.float32(0.25)
    cone = 6.0
    if bound >= np.float32(1.0):
        cone = 6.0 + float(np.floor(bound))  # (+Inf for a flow that has blown up: no halo is wide enough)
    if cone > halo or (particles and 2 * cone + 1 > halo):
        return None, None, True
    cone = int(cone)
    period = min(15, 1 + (halo - 2 * cone - 1) // (cone + 3)) if particles else halo // cone
    return cone, period, False


def ring_model(v_uploaded, per_iteration, halo):
    """The ring protocol of wx_group_step, one iteration per call -> ([(cone, period) after call k], [exchange records]).
    Bootstrap from the uploaded state's maximum; an exchange after max(1, period) iterations; the period that starts at an exchange
    is sized by `known` (the bootstrap's value) while no roll has completed, afterwards by the maximum of the two latest completed
    rolls -- the roll of the exchange itself completes a period later; a roll is the maximum of the measured |vx| since the previous
    exchange, 0 below 0.5."""
    def half(v):
        return np.float32(v) if np.float32(v) >= HALF else np.float32(0.0)
    known = half(v_uploaded)
    cone, period, _ = sizing(known, halo)
    rolls, since, acc, out, exchanges = [], 0, np.float32(0.0), [], []
    for k, m in enumerate(per_iteration):
        reached = bool(np.float32(m) >= np.float32(cone - 5))
        acc = max(acc, half(m))
        since += 1
        if since >= max(1, period):
            v = max(rolls[-2:]) if rolls else known
            exchanges.append({"after_iteration": k, "sized_by": float(v), "older_decides": len(rolls) >= 2 and rolls[-2] > rolls[-1], "roll": float(acc)})
            rolls.append(acc)
            acc, since = np.float32(0.0), 0
            cone, period, _ = sizing(v, halo)
        out.append({"cone": cone, "period": period, "reached_limit": reached})
    return out, exchanges


# ---- part B's last case: a group of 2 slabs at the same geometry, one iteration per call ----
# A lone cell only slows down; a PRESSURE spike of A accelerates the cells next to it for a few iterations (|vx| ~ A in the first one).
# name -> (local column of slab 1, A, the call in which the oracle shows |vx| >= 1.0 for the first time): call 2 is the iteration
# before the exchange (edge strips first), call 3 the one after it (edge strips last); the bootstrap sees a flow below 0.5: cone 6.
# The right-hand watched strip (4) is the SECOND strip range of a split launch, the first unwatched one (1) the first strip of the interior
# launch: a strip index counted from the launch's first strip would take the one for unwatched and the other for watched.
GROUP_SITES = {"reported_in_call_2": (MUST_SEE[1], 0.9, 2), "reported_in_call_3": (MUST_SEE[1], 0.7, 3), "reported_in_call_2_right": (MUST_SEE[2], 0.9, 2),
               "never_recorded": (NEVER_RECORDED[1], 0.9, None), "never_recorded_first_interior_strip": (80, 0.9, None)}  # (80: strip 1 of both widths, and so is all its flow spreads to in four iterations)
GROUP_CALLS = 4


def group_scene(name):
    c_local, A, _ = GROUP_SITES[name]
    base, water, wall = background(SLAB["X_global"], SLAB["Y"])
    base = base.copy()
    base[20, slab_window(SLAB["X_owned"])[c_local], 2] += np.float32(A)
    return base, water, wall


# ---- the band grid: the oracle on a window of columns ----
CROP = 128  # columns of the window, the site in its middle; the outermost 16 on either side are left out (the window is periodic across its own width)


def cropped_reference(wx_oracle, c, bg):
    """reference() of a lone-cell case on a WIDE grid, on the 128 columns around the site alone (the oracle as a slab of the domain:
    X_global and the window's first global column). One iteration's stencils are local and every row-dependent quantity is kept, so
    the window's middle columns hold the bits of the whole grid (tests/test_vx_watch_cpu.py compares a sample, and shows the whole
    background below 0.5 once). -> per-iteration arrays [Y, 96]."""
    X = c["X"]
    first = (c["x"] - CROP // 2) % X
    idx = (first + np.arange(CROP)) % X
    scene = tuple(np.ascontiguousarray(a[:, idx]) for a in whole_scene(c, bg))
    seen, _ = reference(wx_oracle, scene, uniforms(c["family"], c["Y"]), c["family"], X_global=X, x_off=first)
    return [a[:, 16:CROP - 16] for a in seen]
