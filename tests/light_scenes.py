"""Light-lattice scenes: every class of the sun ray's bilinear tap at every seam of the kernels that serve it.

The lighting pass is the one direction-dependent stencil of the iteration: lighting_cell (csrc/wx_cells.h) takes its sunlight from a
bilinear tap at texel + (sin a, cos a) of the source light texture, and which columns (x + dx0, x + dx0 + 1) and rows (y + fv, y + fv + 1,
clamped) that touches depends on the float32 values floorf(sinf(a)) and floorf(cosf(a)) -- the host's u.sun_dx0 / u.sun_fv (wxsim.hip).
SPECIMENS are the angles (as bit patterns of the float32 ``sunAngle`` uniform) that realise the eight (dx0, fv) classes that exist, among
them the exact slider positions GUI 0, 90 and 180; tap_class() restates the host's computation with the C library's sinf / cosf.

A case = a grid, a variant (wrap, quad_scale, planted fast cells) and a specimen: the scene is FILLED with light for fill_iterations(Y)
iterations under the day specimen FILL (light enters from the top row, one row per iteration; below the horizon nothing enters, and
wx_upload resets light), then the uniform changes to the specimen under test and N_UNDER more iterations run. sunIntensity keeps one
positive value throughout (the C ABI takes it independently of the angle). tests/test_light_cpu.py shows that every claimed seam column
and row of every case holds cells at which a neighbouring tap class would give another value; tests/test_light_gpu.py compares the
engine with the oracle bit for bit. A plain module: numpy on top of synth.py and the oracle, no fixture, no GPU.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import functools

import numpy as np

import wxpkg

# ---- specimens -------------------------------------------------------------------------------------------------------------------
# name -> (bits of the float32 sunAngle uniform, (dx0, fv) it must have, what it is)
SPECIMENS = {
    "gui40": (0xBF5F66F9, (-1, 0), "GUI 40: the sun of every other structured suite (control)"),
    "gui140": (0x3F5F66F9, (0, 0), "GUI 140"),
    "noon": (0x00000000, (0, 1), "GUI 90, exactly overhead: rows y+1, y+2"),
    "neg_tiny": (0x8DA24260, (-1, 1), "-1e-30: floor(sin a) is -1 and al = sin a + 1 rounds to 1.0 -- all the weight on column x"),
    "gui180": (0x3FC90FE0, (1, -1), "GUI 180: sinf gives exactly 1.0, columns x+1, x+2"),
    "gui0": (0xBFC90FE0, (-1, -1), "GUI 0"),
    "below_half_pi": (0x3FC90FDA, (1, 0), "the float below pi/2: sin still rounds to 1.0, cos stays positive"),
    "neg_below_half_pi": (0xBFC90FDA, (-1, 0), "its negative"),
    "gui188": (0x3FDAEF27, (0, -1), "GUI 188, below the horizon"),
    "gui_m8": (0xBFDAEF27, (-1, -1), "GUI -8, below the horizon"),
    "pi": (0x40490FDB, (-1, -1), "float32(pi): the day/night clock at midnight"),
    "neg_pi": (0xC0490FDB, (0, -1), "-float32(pi)"),
    "gui176_5": (0x3FC13E31, (0, 0), "GUI 176.5: |a| > 85 degrees, night glow and a red sun"),
    "gui3_5": (0xBFC13E31, (-1, 0), "GUI 3.5: the same from the other side"),
}
GUI_POSITIONS = {"gui40": 40.0, "gui140": 140.0, "noon": 90.0, "gui180": 180.0, "gui0": 0.0, "gui188": 188.0, "gui_m8": -8.0, "gui176_5": 176.5, "gui3_5": 3.5}
FILL = 0xBF060A96            # GUI 60, the day specimen every scene is filled under
FILL_GUI = 60.0
N_UNDER = 6                  # iterations under the specimen under test; compared after the first and after the last
GLOW_SPECIMENS = ("gui180", "gui0", "below_half_pi", "neg_below_half_pi", "gui188", "gui_m8", "pi", "neg_pi", "gui176_5", "gui3_5")  # |a| > 85 degrees
ONE_PER_CLASS = ("gui40", "gui140", "noon", "neg_tiny", "gui180", "gui0", "below_half_pi", "gui188")  # one specimen of each (dx0, fv)
ONE_PER_FV = ("gui140", "noon", "gui188", "gui180")  # one specimen of each fv class, and GUI 180
DAY_SWEEP = (-10.0, 0.0, 3.5, 40.0, 90.0, 140.0, 176.5, 180.0, 188.0)  # GUI positions the sweep across the day walks, there and back
WET_STRIP, WET_FIRST_LANE, WET_RING_ROWS, WET_PAD = 56, 4, 4, 1  # csrc/wx_wet.h: WOUT, WLO, WL, WPAD (tests/test_light_cpu.py compares)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.restype, _f.argtypes = ctypes.c_float, [ctypes.c_float]
_F = np.float32


def angle_of(bits):
    return _F(np.uint32(bits).view(np.float32))


def bits_of_gui(deg):
    """The sunAngle uniform of a GUI position as params.sun_from_angle makes it and ctypes rounds it into wx_params."""
    P = wxpkg.load_package().params
    return int(_F(P.sun_from_angle(float(deg), 1.0)[0]).view(np.uint32))


def tap_class(bits):
    """(dx0, fv, al, be) of the uniform branch (wxsim.hip: fill of u.sun_dx0 .. u.sun_w11), with the libm the host and the oracle call."""
    a = float(angle_of(bits))
    ox, oy = _F(0.0) + _F(_libm.sinf(a)), _F(0.0) + _F(_libm.cosf(a))
    fu, fv = np.floor(ox), np.floor(oy)
    return int(fu), int(fv), _F(ox - fu), _F(oy - fv)


def tap_weights(al, be):
    one = _F(1.0)
    return (one - al) * (one - be), al * (one - be), (one - al) * be, al * be  # w00 w10 w01 w11


def sun_tap(L, cls):
    """The sunlight tap of oracle/wx_oracle.c light_linear_sun on a [Y, X] float32 plane for EVERY cell, class ``cls`` = (dx0, fv, al, be):
    the same four products summed in the same order, in float32."""
    dx0, fv, al, be = cls
    Y, X = L.shape
    ys, xs = np.arange(Y), np.arange(X)
    j0, j1 = np.clip(ys + fv, 0, Y - 1), np.clip(ys + fv + 1, 0, Y - 1)
    i0, i1 = (xs + dx0) % X, (xs + dx0 + 1) % X
    w00, w10, w01, w11 = tap_weights(_F(al), _F(be))
    L = L.astype(np.float32)
    t00, t10, t01, t11 = L[np.ix_(j0, i0)], L[np.ix_(j0, i1)], L[np.ix_(j1, i0)], L[np.ix_(j1, i1)]
    return ((w00 * t00 + w10 * t10) + w01 * t01) + w11 * t11


def neighbour_classes(cls):
    dx0, fv, al, be = cls
    return {"dx0-1": (dx0 - 1, fv, al, be), "dx0+1": (dx0 + 1, fv, al, be), "fv-1": (dx0, fv - 1, al, be), "fv+1": (dx0, fv + 1, al, be)}


# ---- grids and scenes ------------------------------------------------------------------------------------------------------------
BAND_GRID = (113, 128)  # two strips and a ragged column; 128 rows: the lowest grid with row bands under ROW_BANDS 1 (tests/test_light_cpu.py reads the rule)
SLAB_GRID = (256, 64)
GRIDS = {"57x9": (57, 9), "2x4": (2, 4), "169x52": (169, 52), "505x77": (505, 77), "bands": BAND_GRID, "slabs": SLAB_GRID}
_SURFACE_CYCLE = (1, 2, 4, 1, 2, 5, 1, 2, 6)  # land, sea, urban, land, sea, runway, land, sea, industrial: blocks of columns


# Grids lower than 50 rows carry NO walls at all (free air, periodic in y as the textures are): boundaryShader.frag turns an air cell under a
# wall into wall wherever texCoord.y < 0.99, the top row's upper neighbour is the floor row (REPEAT), and (Y - 0.5) / Y < 0.99 below 50
# rows -- a ceiling grows down from the top one row per iteration, as fast as the light enters, and after Y iterations the grid is solid.
FLOORLESS_BELOW = 50


def fill_iterations(Y):
    """Light travels one row per iteration: Y iterations, rounded up to an even number (the light textures' ping-pong is back where it started)."""
    return Y + (Y & 1)


def surface_types(X, Y):
    """Per column: the surface type (stretches of five columns through _SURFACE_CYCLE) and the wall rows (none below FLOORLESS_BELOW)."""
    S = wxpkg.load_package().synth
    blk = 5 if X >= 40 else 1
    types = np.array([_SURFACE_CYCLE[(x // blk) % len(_SURFACE_CYCLE)] for x in range(X)], np.int8)
    if Y >= FLOORLESS_BELOW:
        _, _, w = S.terrain_grid(X, Y)
        nrows = (w[..., 1] == 0).sum(0).astype(np.int64)
        # (the default terrain is two rows thick on grids this low: every stretch of land is raised by 0, 2 or 4 rows on top of it, so
        # that air lies next to walls sideways as well)
        nrows = np.where(types == 2, np.minimum(nrows, 2), np.minimum(nrows + 2 * ((np.arange(X) // (3 * blk)) % 3), Y // 3))
    else:
        types[:], nrows = 0, np.zeros(X, np.int64)
    return types, nrows


def light_scene(X, Y, seed=4711, thick_smoke=True, sim_height=None):
    """-> base, water, wall. The terrain heights of synth.terrain_grid under stretches of sea, land, urban, runway and industrial surface
    (setupShader.frag's wall cells), and in the air a seeded dense field of cloud, precipitation mass and smoke that differs from column
    to column and row to row -- amplitudes chosen so that a cell takes a few 1 / Y of the light whatever the grid's height (the shader's
    cellHeightCompensation is 300 / Y) -- some cells of smoke beyond 4 (the fire glow of the emitted light), and a flow of 0.05 cells per
    iteration. ``thick_smoke=False`` leaves the cells beyond 4 out (the reference fixtures: their bounds are absolute ones, set at values of order 1)."""
    S = wxpkg.load_package().synth
    types, nrows = surface_types(X, Y)
    gui = wxpkg.load_package().params.merge_settings(None)
    if sim_height is not None:
        gui["simHeight"] = float(sim_height)
    snd = S.sounding_rows(Y, gui)
    yy = np.arange(Y)[:, None]
    is_wall = yy < nrows[None, :]
    sea = (types == 2)[None, :] & is_wall
    land = is_wall & ~sea
    air = ~is_wall
    base, water, wall = np.zeros((Y, X, 4), np.float32), np.zeros((Y, X, 4), np.float32), np.zeros((Y, X, 4), np.int8)
    base[..., 3] = np.where(air, snd["T_air"][:, None], np.where(sea, _F(298.15), _F(1000.0)))
    water[..., 0] = np.where(air, snd["total_water"][:, None], np.where(sea, _F(1002.0), _F(1001.0)))
    water[..., 1] = np.where(air, snd["cloud_water"][:, None], _F(0.0))
    water[..., 2] = np.where(sea, _F(100.0), np.where(land, _F(25.0), _F(0.0)))
    wall[..., 0] = types[None, :]
    vdist = yy - nrows[None, :] + 1
    wall[..., 2] = np.clip(vdist, -127, 127)
    wall[..., 1] = np.where(is_wall, 0, np.clip(vdist, 1, 127))
    wall[..., 3] = np.where(land, 60, 0)
    if Y < FLOORLESS_BELOW:
        wall[..., 1] = wall[..., 2] = 127
    rng = np.random.Generator(np.random.Philox(seed))
    u = [rng.random((Y, X), dtype=np.float32) for _ in range(8)]
    frac = _F(0.5 if X * Y >= 100 else 1.0)  # (a grid of a few cells: every cell carries all three)
    cloud = np.where(air & (u[0] < frac), u[1] * _F(0.03), 0).astype(np.float32)
    water[..., 1] += cloud
    water[..., 0] += cloud
    water[..., 2] += np.where(air & (u[2] < frac), u[3] * _F(0.15), 0).astype(np.float32)
    water[..., 3] += np.where(air & (u[4] < frac), u[5] * _F(0.1), 0).astype(np.float32)
    # thick smoke, the fire glow of the emitted light: one cell in every fifth column, walking through the rows (on the grid nine rows high, where
    # such a cell takes ALL the light and the column below it is dark, none of them is a strip border or an edge column)
    for x in range(3, X, 5) if thick_smoke else ():
        y = int(nrows[x]) + 1 + (5 * x) % max(1, Y - 4 - int(nrows[x]))
        water[y, x, 3] = _F(6.0 + 0.2 * Y) + u[7][y, x] * _F(4.0)  # (a lone cell spreads: 12.6 is 4.3 after 50 iterations and 3.2 after 100)
    for ch in (0, 1):
        base[..., ch] = np.where(air, rng.standard_normal((Y, X), dtype=np.float32) * _F(0.05), 0)
    return base, water, wall


def scene_uniforms(Y, bits=FILL, wrap=1, quad_scale=0, sim_height=None):
    """Default settings with precipitation off; sunIntensity is GUI 60's whatever the angle; ``bits``: the sunAngle uniform."""
    P = wxpkg.load_package().params
    gui = P.merge_settings(None)
    gui["sunAngle"] = FILL_GUI
    gui["wrapHorizontally"] = bool(wrap)
    if sim_height is not None:
        gui["simHeight"] = float(sim_height)
    u = P.uniforms_from_gui(gui, Y, quad_scale=quad_scale)
    u["enablePrecipitation"] = 0
    u["sunAngle"] = float(angle_of(bits))
    return u


# ---- seams -----------------------------------------------------------------------------------------------------------------------
def edge_columns(X):
    return sorted({0, 1 % X, (X - 2) % X, X - 1})


def strip_border_columns(X, w=WET_STRIP):
    """The two columns on either side of every border between two strips of ``w`` output columns (the tap reaches x - 1 .. x + 2)."""
    return sorted({c for s in range(w, X, w) for c in (s - 2, s - 1, s, s + 1) if 0 <= c < X})


def band_border_rows(Y):
    """Rows y with a band border of the eight row bands within the tap's reach y - 1 .. y + 2 (the last lit row is Y - 2)."""
    return sorted({r for k in range(1, 8) for r in range(k * Y // 8 - 2, k * Y // 8 + 2) if 0 <= r < Y - 1})


def slab_cut_columns(X, nslab):
    xo = X // nslab
    return sorted({(k * xo + d) % X for k in range(nslab) for d in (-2, -1, 0, 1)})


def fast_cell_sites(X, Y, wall):
    """Where the fast-cell variant plants vx = 1.3: air cells on the first strip border and at the edge columns, seven to eleven rows above
    the ground (where the low grids' short segments have their borders) -- a handful, each with quiet neighbours."""
    cols = list(dict.fromkeys([0, X - 1] + ([WET_STRIP - 1, WET_STRIP] if X > WET_STRIP else []) + [1, X - 2]))[:6]
    sites = []
    for k, x in enumerate(cols):
        g = int((wall[:, x, 1] == 0).sum())
        y = min(Y - 3, g + 7 + 2 * (k % 3))  # (beyond the five rows of the surface wind smoothing, which would take a third of the speed)
        if wall[y, x, 1] != 0:
            sites.append((x, y))
    return sites


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# configuration -> what tests/test_light_gpu.py runs it with: handle options, the iterations of each step, MORE_TO_COME pieces, variant
CONFIGS = {
    "wet": {"steps": (1, N_UNDER - 1)}, "wet_plain": {"steps": (N_UNDER,), "compare_first": False},
    "wet_pieces": {"steps": (N_UNDER,), "pieces": True, "compare_first": False}, "wet_stored": {"steps": (1, N_UNDER - 1), "water0_on_demand": 0},
    "perpass": {"steps": (1, N_UNDER - 1), "kernel_set": 0},
    "quad": {"steps": (1, N_UNDER - 1), "quad_scale": 1}, "nowrap": {"steps": (1, N_UNDER - 1), "wrap": 0},
    "fast": {"steps": (1, N_UNDER - 1), "fast": True},
    "bands0": {"steps": (1, N_UNDER - 1), "bands": 0}, "bands1": {"steps": (1, N_UNDER - 1), "bands": 1}, "bands2": {"steps": (1, N_UNDER - 1), "bands": 2},
}
PLAN = (  # (grid, configurations, specimens)
    ("57x9", ("wet", "wet_plain", "wet_pieces", "wet_stored", "perpass", "quad", "nowrap", "fast"), tuple(SPECIMENS)),
    ("2x4", ("wet", "perpass", "nowrap"), tuple(SPECIMENS)),
    ("169x52", ("wet", "wet_plain", "wet_pieces", "wet_stored", "perpass", "quad", "nowrap", "fast"), tuple(SPECIMENS)),
    ("505x77", ("wet", "perpass", "nowrap", "fast"), tuple(SPECIMENS)),
    ("bands", ("bands0", "bands1", "bands2"), ONE_PER_FV),
)


def variant_of(config):
    cfg = CONFIGS[config]
    return (int(cfg.get("wrap", 1)), int(cfg.get("quad_scale", 0)), bool(cfg.get("fast", False)))


def claimed_rows(Y, specimen, grid=None):
    """The rows a case claims. On the low grids every row in which a neighbouring class CAN show, by the pass's own rules:
    - above: the top row holds sunIntensity and the row below it takes no absorption (lightingShader.frag:63), so light rows Y - 2 and
      Y - 1 are uniform in x and equal -- a tap whose first row y + fv is Y - 2 or higher reads the same value under every class;
    - below, for a tap that looks down (fv = -1): the lowest row clamps (y - 1 and y - 2 are both row 0), so row 0 reads the same rows under
      fv - 1; with be = 0 the tap is row y - 1 alone and row 1 reads row 0 under both. Where the grid has a floor the wall rows (0 and 1
      under the sea, which alone passes light on: 0.9 of its tap; land returns 0) go dark within a few iterations of such a tap -- it
      reaches land within five columns, or the clamped row -- so there the claims begin one row higher, at the first air row over the sea.
      With fv = 0 and be below 2^-20 row 0 differs from its clamped neighbour class by less than an ulp.
    On the band grid: the rows within the tap's reach of a band border."""
    dx0, fv, al, be = tap_class(SPECIMENS[specimen][0])
    ground = 0 if Y < FLOORLESS_BELOW else 1
    first = ground + (2 if be == 0 else 1) if fv < 0 else (1 if fv == 0 and be < 2.0 ** -20 else 0)
    last = min(Y - 2, Y - 3 - fv)
    rows = band_border_rows(Y) if grid == "bands" else range(Y)
    return [y for y in rows if first <= y <= last]


def cases():
    """Every (grid, configuration, specimen) with the seams it claims: ``columns`` (strip borders of width 56, the edge columns -- the
    light tap repeats in x whether or not the flow wraps) and ``rows`` (claimed_rows)."""
    out = []
    for grid, configs, specimens in PLAN:
        X, Y = GRIDS[grid]
        cols = sorted(set(edge_columns(X)) | set(strip_border_columns(X)))
        for config in configs:
            for sp in specimens:
                out.append({"grid": grid, "X": X, "Y": Y, "config": config, "specimen": sp, "variant": variant_of(config), "columns": cols,
                            "rows": claimed_rows(Y, sp, grid)})
    return out


def slab_cases():
    """The slab runs of tests/test_light_gpu.py: the specimens that read to the right (dx0 >= 0) on SLAB_GRID, claiming the columns on
    either side of every cut of the 2- and the 4-slab decomposition (and the rows of the plain cases)."""
    X, Y = SLAB_GRID
    cols = sorted(set(slab_cut_columns(X, 2)) | set(slab_cut_columns(X, 4)))
    return [{"grid": "slabs", "X": X, "Y": Y, "config": "slabs", "specimen": sp, "variant": (1, 0, False), "columns": cols, "rows": claimed_rows(Y, sp)}
            for sp, (_, (dx0, _), _) in SPECIMENS.items() if dx0 >= 0]


def tap_dependent(wall):
    """Cells whose light output is a function of the sunlight tap: air, and the wall cells of sea (0.9 of the tap; land returns 0); not the top row."""
    m = (wall[..., 1] != 0) | (wall[..., 0] == 2)
    m[-1, :] = False
    return m


def distinguishing_cells(run, specimen, which="last"):
    """[Y, X] bool: tap-dependent cells at which the tap of the specimen's class on the source light of the first / last iteration differs
    from the tap of EACH of the four neighbouring classes (dx0 +- 1, fv +- 1)."""
    cls = tap_class(SPECIMENS[specimen][0])
    src = run["source_" + which]
    good = sun_tap(src, cls)
    m = tap_dependent(run[which]["WALL_CUR"])
    for nc in neighbour_classes(cls).values():
        m &= good != sun_tap(src, nc)
    return m


# ---- the oracle's side: one fill per grid, one run per (grid, variant, specimen) ---------------------------------------------------
ORACLE_STATE = ("BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1", "CURL", "VORT", "PRECIP_FB", "PRECIP_DEP", "EMITTED")
COMPARED = ("LIGHT_0", "LIGHT_1", "BASE_CUR", "WATER_CUR", "WALL_CUR", "BASE_DISP", "WATER_0")


def _oracle():
    import wx_oracle
    wx_oracle.build()
    return wx_oracle


def _snapshot(o):
    return {f: o.field(f) for f in ORACLE_STATE}


def oracle_from(state, X, Y, it):
    """A second oracle instance in the state ``state`` (a snapshot after an EVEN number of iterations: the light ping-pong of a fresh
    instance)."""
    o = _oracle().OracleSim(X, Y, 0)
    o.upload(state["BASE_CUR"], state["WATER_CUR"], state["WALL_CUR"])
    for f in ORACLE_STATE:
        o.view(f)[...] = state[f]
    o.iter = it
    return o


@functools.lru_cache(maxsize=None)
def oracle_fill(grid):
    """The scene of a grid filled under FILL: (scene, snapshot of the oracle after fill_iterations(Y)). Shared; leave it unchanged."""
    X, Y = GRIDS[grid]
    scene = light_scene(X, Y)
    o = _oracle().OracleSim(X, Y, 0)
    o.upload(*scene)
    o.set_params(scene_uniforms(Y))
    o.iter = 0
    o.step(fill_iterations(Y))
    st = _snapshot(o)
    o.close()
    return scene, st


def plant_fast(base, sites):
    for k, (x, y) in enumerate(sites):
        base[y, x, 0] = _F(1.3 if k % 2 == 0 else -1.3)


@functools.lru_cache(maxsize=None)
def fast_expected(grid, specimen):
    """What wx_fastest_velocity must report after the first iteration of the fast variant: the largest velocity component behind the
    boundary pass (the oracle stepped with the first three passes only), 0 below 0.9."""
    X, Y = GRIDS[grid]
    _, st = oracle_fill(grid)
    o = oracle_from(st, X, Y, fill_iterations(Y))
    try:
        plant_fast(o.view("BASE_CUR"), fast_cell_sites(X, Y, st["WALL_CUR"]))
        o.set_params(dict(scene_uniforms(Y, SPECIMENS[specimen][0]), pass_mask=7))
        o.step(1)
        v = float(np.abs(o.field("BASE_CUR")[..., :2]).max())
        return v if v >= _F(0.9) else 0.0
    finally:
        o.close()


@functools.lru_cache(maxsize=None)
def oracle_run(grid, variant, specimen):
    """{"first": fields after the first iteration under the specimen, "last": after N_UNDER, "source_first" / "source_last": the source
    sunlight plane [Y, X] those iterations' lighting passes read}. Fields: COMPARED and EMITTED (unrounded). Shared; leave it unchanged."""
    X, Y = GRIDS[grid]
    wrap, quad, fast = variant
    scene, st = oracle_fill(grid)
    n0 = fill_iterations(Y)
    o = oracle_from(st, X, Y, n0)
    try:
        if fast:
            plant_fast(o.view("BASE_CUR"), fast_cell_sites(X, Y, st["WALL_CUR"]))
        o.set_params(scene_uniforms(Y, SPECIMENS[specimen][0], wrap, quad))
        out = {}
        o.step(1)
        out["first"] = {f: o.field(f) for f in COMPARED + ("EMITTED",)}
        out["source_first"] = o.field("LIGHT_0")[..., 0]   # iteration n0 is even: it read light 0 and wrote light 1
        o.step(N_UNDER - 1)
        out["last"] = {f: o.field(f) for f in COMPARED + ("EMITTED",)}
        out["source_last"] = o.field("LIGHT_1" if N_UNDER % 2 == 0 else "LIGHT_0")[..., 0]
        return out
    finally:
        o.close()


# ---- messages --------------------------------------------------------------------------------------------------------------------
def describe_cell(x, y, X, Y, borders=()):
    """Output lane and strip of a column in the wet kernel's strips, the row's distance from the nearest of ``borders`` (segment or
    band borders, where the caller knows them; else floor and top)."""
    bs = sorted(set(borders) | {0, Y - 1})
    return (f"cell (x={x}, y={y}): strip {x // WET_STRIP} output lane {WET_FIRST_LANE + x % WET_STRIP}, {X - 1 - x} columns from the right edge, "
            f"row {min(abs(y - b) for b in bs)} from the nearest border of {bs}")


def describe_difference(field, a, b, X, Y, specimen, borders=()):
    ne = a != b
    while ne.ndim > 2:
        ne = ne.any(-1)
    ys, xs = np.nonzero(ne)
    x, y = int(xs[0]), int(ys[0])
    dx0, fv, al, be = tap_class(SPECIMENS[specimen][0])
    return (f"{field}: {int(ne.sum())} cells differ under {specimen} (dx0 {dx0}, fv {fv}, al {float(al):.8g}, be {float(be):.8g}); first "
            f"{describe_cell(x, y, X, Y, borders)}: {a[y, x]} != {b[y, x]}; columns {sorted(set(xs.tolist()))[:12]} rows {sorted(set(ys.tolist()))[:12]}")
