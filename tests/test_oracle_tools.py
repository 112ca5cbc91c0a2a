"""CPU oracle vs the reference's own output on the WALL-EDITING TOOLS (advectionShader.frag:291-400, userInputType 10 .. 22, both signs
of the intensity) and the AIRPLANE CRASH (:444-457), over every surface type, held for one or three iterations, RELEASED, and run
20 iterations further (tests/golden/tools64_*.npz, crash64_*.npz; recipe in oracle/golden/gen_golden.py, drawn as GL_POINTS on 64 x 64;
one scene for the whole family, tools64_in.npz).

First, from the reference's dumps ALONE (no oracle): per tool, sign and cell class the edit happened where the shader says and nowhere
else. The table below is written from the shader's text. "Before the edit" is the wall texture of the same iteration of a run without
any tool (tools64_quiet*.npz, crash64_quiet.npz): the advection pass edits what the boundary pass of that iteration wrote. Then the
oracle against every dump: walls bit for bit, fields within the bounds tests/test_oracle_sliders.py states."""
import json
import os

import numpy as np
import pytest

from test_oracle_sliders import ULP_T

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INERT, LAND, WATER, FIRE, URBAN, RUNWAY, INDUSTRIAL = range(7)
DISTANCE, VERT_DISTANCE, VEGETATION = 1, 2, 3  # wall bytes (byte 0: the type)
WALL_TOOLS = (10, 11, 12, 13, 14, 15, 16, 20, 21, 22)
AFTER = 20
RIM_MARGIN = 1e-5


def tool_name(tool, sign, held, mode="disc"):
    return f"tools64_{'' if mode == 'disc' else mode + '_'}t{tool}{'p' if sign > 0 else 'n'}_h{held}"


DISC_RUNS = [(t, s, h, "disc") for t in WALL_TOOLS for s in (+1, -1) for h in (1, 3)]
EXTRA_RUNS = [(10, -1, 1, "wholewidth"), (21, +1, 1, "wholewidth"), (12, +1, 1, "nowrap"), (13, +1, 1, "nowrap"), (10, -1, 1, "nowrap")]
TOOL_RUNS = [tool_name(*r) for r in DISC_RUNS + EXTRA_RUNS]
CRASH_CASES = ("land", "buried", "inert", "sea", "fire", "urban", "runway", "industrial", "air", "stepped_land")
CRASH_RUNS = ["crash64_" + c for c in CRASH_CASES]

# ---- the table, from advectionShader.frag:291-400 -------------------------------------------------------------------------------
# positive intensity. 10 / 11 / 12 make EVERY cell of the brush a wall cell of their type (:297-309, :354-365). The others act on a
# wall cell (DISTANCE == 0) of an admitted type with no wall cell above it:
ADMITTED = {13: (LAND,), 14: (LAND, RUNWAY, INDUSTRIAL), 15: (LAND, URBAN, INDUSTRIAL), 16: (LAND, URBAN, RUNWAY),
            20: (INERT, LAND, FIRE, URBAN, RUNWAY, INDUSTRIAL), 21: (LAND, URBAN, INDUSTRIAL), 22: (LAND, FIRE, URBAN, INDUSTRIAL)}
BECOMES = {10: INERT, 11: LAND, 12: WATER, 13: FIRE, 14: URBAN, 15: RUNWAY, 16: INDUSTRIAL}
# negative intensity, on every wall cell whatever lies above it (:367-398): 13 .. 16 turn their own type back into land, 20 / 21 add
# the (negative) intensity to every wall cell's soil moisture / snow, 22 lowers the vegetation to 0 at the least, 10 / 11 / 12 remove
# the cell unless it is in row 0
REVERTS = {13: FIRE, 14: URBAN, 15: RUNWAY, 16: INDUSTRIAL}


def scene():
    return np.load(os.path.join(GOLDEN_DIR, "tools64_in.npz"))


def load_run(name):
    """-> fixture, uniforms at the start, {iterations done: {uniform: new value}}."""
    g, s = np.load(os.path.join(GOLDEN_DIR, name + ".npz")), scene()
    u = json.loads(str(g["uniforms_json"]))
    u["initial_T"] = s["initial_T"]
    for k in ("userInputValues", "userInputMove", "airplaneValues"):
        u[k] = tuple(u[k])
    changes = {int(k): {n: (tuple(v) if isinstance(v, list) else v) for n, v in c.items()}
               for k, c in json.loads(str(g["uniform_changes_json"])).items()} if "uniform_changes_json" in g.files else {}
    return g, u, changes


def dump_iterations(g):
    return sorted(int(k[2:].split("_")[0]) for k in g.files if k.startswith("it") and k.endswith("_wall_cur"))


def play(g, u, changes, set_params, step, read):
    """The run of a fixture on any implementation: uniforms replaced after the iterations ``changes`` names (harness.js
    `uniform_changes`), ``read()`` after every dump iteration. Shared with tests/test_gpu_parity.py."""
    its, out, done = dump_iterations(g), {}, 0
    set_params(u)
    for e in sorted(set(its) | set(changes)):
        if e > done:
            step(e - done)
            done = e
        if e in changes:
            u = dict(u, **changes[e])
            set_params(u)
        if e in its:
            out[e] = read()
    return out


def check_fields(out, g):
    """``out``: dump -> (base, water, wall). Walls bit for bit at every dump; fields, where the fixture keeps them, within
    tests/test_oracle_sliders.py's bounds: v, P 5e-7 up to 5 iterations and 1e-6 beyond, T 4 ulp, vapour / cloud 5e-5, the other two
    water channels 1e-6 / 2e-6."""
    bad = []
    for it in dump_iterations(g):
        b, w, wl = out[it]
        if not np.array_equal(wl, g[f"it{it}_wall_cur"]):
            bad.append((it, "wall", int((wl != g[f"it{it}_wall_cur"]).any(-1).sum())))
        if f"it{it}_base_cur" not in g.files:
            continue
        rb, rw = g[f"it{it}_base_cur"], g[f"it{it}_water_cur"]
        few = it <= 5
        checks = [("v,P", np.abs(b[..., :3] - rb[..., :3]).max(), 5e-7 if few else 1e-6), ("T", np.abs(b[..., 3] - rb[..., 3]).max(), 4 * ULP_T),
                  ("vapour_cloud", np.abs(w[..., :2] - rw[..., :2]).max(), 5e-5), ("precip_smoke", np.abs(w[..., 2:] - rw[..., 2:]).max(), 1e-6 if few else 2e-6)]
        print(json.dumps({"dump": it, **{k: float(e) for k, e, _ in checks}}))
        bad += [(it, k, float(e), tol) for k, e, tol in checks if not e <= tol]
    return bad


def oracle_dumps(oracle, g, u, changes):
    s = scene()
    X, Y = int(s["X"]), int(s["Y"])
    o = oracle.OracleSim(X, Y, 0)
    o.upload(s["in_base"], s["in_water"], s["in_wall"])
    o.iter = int(g["iter0"])
    try:
        return play(g, u, changes, lambda uu: o.set_params(dict(uu, varyings=s["varyings"], subpixel_bits=4)), o.step,
                    lambda: (o.field("BASE_CUR"), o.field("WATER_CUR"), o.field("WALL_CUR")))
    finally:
        o.close()


# ---- where the brush is, in the shader's float32 arithmetic on the stored texCoords ---------------------------------------------
def brush_distance(varyings, values, wrap):
    """-> distance (the row distance in whole-width mode), radius. advectionShader.frag:234-253; common.glsl:268-271."""
    f = np.float32
    tcx, tcy = varyings[..., 2].astype(f), varyings[..., 3].astype(f)
    r = f(values[3]) * f(1.0 / varyings.shape[0])
    if values[0] < -0.5:
        return np.abs(f(values[1]) - tcy), r
    a = f(values[0])
    dx = np.abs(a - tcx)
    if wrap:
        dx = np.minimum(np.minimum(dx, np.abs(f(1.0) + a - tcx)), f(1.0) - a + tcx)
    dy = f(values[1]) - tcy
    return np.sqrt(dx * dx + dy * dy, dtype=f), r  # (square grid: the aspect factor is 1)


def in_brush(varyings, values, wrap):
    """The rim margin, asserted (the recipe chose the centre for it): no cell within 1e-5 (relative) of the radius, where `length()`
    may round either way -- so no cell is left out of any comparison."""
    d, r = brush_distance(varyings, values, wrap)
    assert (np.abs(d.astype(np.float64) - float(r)) > RIM_MARGIN * float(r)).all()
    return d < r


def expected_edit(tool, sign, pre, inside, row):
    """Wall bytes after one held iteration, from the table: -> expected wall, mask of cells whose soil moisture / snow the tool
    changes, mask of removed cells, mask of cells set to a wall (10 / 11 / 12)."""
    exp = pre.astype(np.int64)
    is_wall = pre[..., DISTANCE] == 0
    above_air = np.roll(pre[..., DISTANCE], -1, axis=0) != 0
    none = np.zeros(inside.shape, bool)
    fields, removed, made = none, none, none
    if sign > 0:
        if tool in (10, 11, 12):
            made = inside
            exp[made, 0], exp[made, DISTANCE] = BECOMES[tool], 0
        else:
            hit = inside & is_wall & above_air & np.isin(pre[..., 0], ADMITTED[tool])
            if tool in BECOMES:
                exp[hit, 0] = BECOMES[tool]
            elif tool == 22:
                exp[hit, VEGETATION] += 1
            else:
                fields = hit
    else:
        hit = inside & is_wall
        if tool in REVERTS:
            exp[hit & (pre[..., 0] == REVERTS[tool]), 0] = LAND
        elif tool == 22:
            exp[hit, VEGETATION] = np.maximum(exp[hit, VEGETATION] - 1, 0)
        elif tool in (20, 21):
            fields = hit
        else:
            removed = hit & (row >= 1)
            exp[removed, DISTANCE] = 255
    return exp, fields, removed, made


def cell_classes(pre):
    """name -> mask: the surface cell of every type, flat and beside a step; buried wall cells (a wall cell above); air."""
    is_wall = pre[..., DISTANCE] == 0
    above_air = np.roll(pre[..., DISTANCE], -1, axis=0) != 0
    c = {f"surface_{t}": is_wall & above_air & (pre[..., 0] == t) for t in range(7)}
    c["buried"] = is_wall & ~above_air
    c["air"] = ~is_wall
    return c


# ---- non-vacuity: the reference's dumps alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,sign,held,mode", [r for r in DISC_RUNS + EXTRA_RUNS if r[2] == 1])
def test_the_reference_edited_where_the_shader_says(tool, sign, held, mode):
    g, u, changes = load_run(tool_name(tool, sign, held, mode))
    s = scene()
    wrap = mode != "nowrap"
    assert int(u["wrapHorizontally"]) == int(wrap) and int(u["userInputType"]) == tool and changes == {1: {"userInputType": -1}}
    assert (u["userInputValues"][2] > 0) == (sign > 0)
    q = np.load(os.path.join(GOLDEN_DIR, "tools64_quiet.npz" if wrap else "tools64_quiet_nowrap.npz"))
    pre, post = q["it1_wall_cur"], g["it1_wall_cur"]
    inside = in_brush(s["varyings"], u["userInputValues"], wrap)
    Y, X = inside.shape
    row = np.arange(Y)[:, None] + np.zeros(X, np.int64)
    if mode == "disc":  # every class of cell lies inside the disc and outside it
        for name, m in cell_classes(pre).items():
            assert (m & inside).any() and (m & ~inside).any(), name
    if mode == "nowrap":  # the disc is cut by the x edge: with the wrap on it would reach the last columns
        assert inside[:, 0].any() and not inside[:, X // 2:].any() and brush_distance(s["varyings"], u["userInputValues"], True)[0][:, -1].min() < u["userInputValues"][3] / Y
    exp, fields, removed, made = expected_edit(tool, sign, pre, inside, row)
    # 127 + 1 in an RGBA8I attachment and 255 in the distance byte are the two values the format cannot hold: compared below
    over = exp > 127
    assert np.array_equal(post[~over], exp[~over].astype(np.int8)), np.argwhere((post != exp) & ~over)[:8]
    assert (post[over] == 127).all()  # the conversion saturates (LABNOTES section 2): a removed cell's distance byte, vegetation 127 + 1
    assert not (post != pre).any(-1)[~inside].any()  # nothing outside the brush
    b, w, qb, qw = g["it1_base_cur"], g["it1_water_cur"], q["it1_base_cur"], q["it1_water_cur"]
    inten = np.float32(u["userInputValues"][2])
    if tool in (20, 21):
        ch, delta = (2, inten * np.float32(10.0)) if tool == 20 else (3, inten * np.float32(0.5))
        assert fields.sum() >= 10
        assert np.array_equal(w[fields][:, ch], qw[fields][:, ch] + delta)
        assert np.array_equal(w[~fields], qw[~fields])  # every type outside the list, every cell with a wall above (positive sign), all air
        if sign > 0:  # each type outside the list was there to be refused, and so was a buried cell of an admitted type
            cl = cell_classes(pre)
            for t in set(range(7)) - set(ADMITTED[tool]):
                assert (cl[f"surface_{t}"] & inside & ~fields).any(), t
            assert (cl["buried"] & inside & np.isin(pre[..., 0], ADMITTED[tool]) & ~fields).any()
    if tool in BECOMES and sign > 0 and tool >= 13 or tool == 22 or (tool in REVERTS and sign < 0):
        changed = (post != pre).any(-1)
        cl = cell_classes(pre)
        if sign > 0:
            for t in range(7):
                m = cl[f"surface_{t}"] & inside & ~over.any(-1)  # (vegetation 127 + 1 stays 127: no change to see)
                if mode != "disc" and not m.any():
                    continue
                assert m.any() and changed[m].all() == (t in ADMITTED[tool]) and changed[m].any() == (t in ADMITTED[tool]), t
            assert not changed[cl["buried"]].any() and not changed[cl["air"]].any()
        elif tool in REVERTS:
            assert changed[inside & (pre[..., DISTANCE] == 0) & (pre[..., 0] == REVERTS[tool])].all() and changed.sum() >= 8
            assert changed[cl["buried"]].any()  # the removal side does not ask what lies above
        else:  # vegetation down: every wall cell with vegetation; 0 stays 0
            m = inside & (pre[..., DISTANCE] == 0)
            assert np.array_equal(changed[m], pre[m][:, VEGETATION] > 0) and (pre[m][:, VEGETATION] == 0).any() and (pre[m][:, VEGETATION] == 1).any()
    if tool == 22 and sign > 0:
        assert over.any() and (pre[over[..., VEGETATION], VEGETATION] == 127).all()
    if made.any():
        assert made.sum() >= 100 and (pre[made][:, DISTANCE] != 0).sum() >= 40 and (pre[made][:, DISTANCE] == 0).sum() >= 30
        T_new = np.float32(u["waterTemperature"]) if tool == 12 else np.float32(1000.0)
        assert (b[made][:, 3] == T_new).all() and (w[made][:, 0] == (1002.0 if tool == 12 else 1001.0)).all()
        if tool == 11:
            assert (w[made][:, 2] == 25.0).all()
        else:
            assert np.array_equal(w[made][:, 2], qw[made][:, 2])
        assert np.array_equal(post[made][:, 2:], pre[made][:, 2:])  # vertical distance and vegetation stay for the boundary pass to redo
    if removed.any():
        above_wall = np.roll(pre[..., DISTANCE], -1, axis=0) == 0
        assert (removed & above_wall).sum() >= 10 and (removed & ~above_wall).sum() >= 5  # buried cells too, whatever lies above
        assert (inside & (pre[..., DISTANCE] == 0) & (row == 0)).any() and not removed[0].any()  # row 0 stays
        T0 = np.asarray(s["initial_T"], np.float32)
        assert np.array_equal(b[removed][:, 3], T0[row[removed]])  # the start sounding of its row
        assert (w[removed] == 0).all()
        end = g[f"it{1 + AFTER}_wall_cur"]
        assert (end[removed][:, DISTANCE] != 0).sum() >= removed.sum() // 2  # still air 20 iterations on (a cell under an overhang fills again)


@pytest.mark.parametrize("held", [1, 3])
def test_a_fire_lit_by_the_tool_burns_and_spreads_in_the_reference(held):
    """Tool 13 lights the surface land of the brush; on the land that keeps soil moisture 5 and no snow (fire divisor 10) it is still
    burning 20 iterations after release, and iterNum 1000 -- inside those 20 -- spread it to neighbours the brush never lit."""
    g, u, _ = load_run(tool_name(13, +1, held))
    lit, end = g[f"it{held}_wall_cur"], g[f"it{held + AFTER}_wall_cur"]
    assert int(g["iter0"]) + held <= 1000 < int(g["iter0"]) + held + AFTER
    q = np.load(os.path.join(GOLDEN_DIR, "tools64_quiet.npz"))[f"it{held}_wall_cur"]
    new = (lit[..., 0] == FIRE) & (q[..., 0] != FIRE) & (lit[..., DISTANCE] == 0)
    assert new.sum() >= 3 and (q[new][:, 0] == LAND).all()
    still = new & (end[..., 0] == FIRE)
    assert still.sum() >= 2
    spread = (end[..., 0] == FIRE) & (end[..., DISTANCE] == 0) & (lit[..., 0] == LAND) & (lit[..., DISTANCE] == 0)
    assert spread.any()
    w = g[f"it{held + AFTER}_water_cur"]
    assert (w[np.roll(still, 1, axis=0)][:, 3] > 0.05).sum() >= 2  # smoke in the air cell above them (none where the vegetation is 0 or 1)


def test_vegetation_steps_accumulate_in_the_reference():
    """Held for three iterations: + 3 and - 3, stopping at the ends of the byte (127 stays 127, 0 stays 0)."""
    q = np.load(os.path.join(GOLDEN_DIR, "tools64_quiet.npz"))["it3_wall_cur"]
    s = scene()
    for sign in (+1, -1):
        g, u, _ = load_run(tool_name(22, sign, 3))
        inside = in_brush(s["varyings"], u["userInputValues"], True)
        post = g["it3_wall_cur"]
        if sign > 0:
            m = inside & (q[..., DISTANCE] == 0) & (np.roll(q[..., DISTANCE], -1, axis=0) != 0) & (q[..., 0] == LAND)
            assert m.sum() >= 4 and np.array_equal(post[m][:, VEGETATION], np.minimum(q[m][:, VEGETATION].astype(int) + 3, 127))
            assert (q[m][:, VEGETATION] >= 126).any()
        else:
            m = inside & (q[..., DISTANCE] == 0) & (q[..., 0] == LAND)  # (urban and industrial cells are capped by the boundary pass besides)
            assert np.array_equal(post[m][:, VEGETATION], np.maximum(q[m][:, VEGETATION].astype(int) - 3, 0)) and (q[m][:, VEGETATION] == 1).any()


@pytest.mark.parametrize("case", CRASH_CASES)
def test_the_crash_lit_the_surface_land_and_nothing_else(case):
    """advectionShader.frag:444-457 from the reference's dumps: of the cells within 1.5 cells of the plane a WALL cell changes only if
    it is land at VERT_DISTANCE 0 (it becomes fire); an air cell becomes the fire ball."""
    g, u, changes = load_run("crash64_" + case)
    q = np.load(os.path.join(GOLDEN_DIR, "crash64_quiet.npz"))
    s = scene()
    assert u["airplaneValues"][3] == 1.0 and changes == {1: {"airplaneValues": (0.0, 0.0, 0.0, 0.0)}} and int(u["userInputType"]) == -1
    Y, X = s["in_wall"].shape[:2]
    d, _ = brush_distance(s["varyings"], (u["airplaneValues"][0], u["airplaneValues"][1], 0.0, 0.0), True)
    d = d * np.float32(Y)
    assert (np.abs(d - 1.5) > 0.05).all()
    near = d < 1.5
    assert near.sum() == 9
    pre, post = q["it1_wall_cur"], g["it1_wall_cur"]
    lit = near & (pre[..., DISTANCE] == 0) & (pre[..., 0] == LAND) & (pre[..., VERT_DISTANCE] == 0)
    exp = pre.copy()
    exp[lit, 0] = FIRE
    assert np.array_equal(post, exp)
    air = near & (pre[..., DISTANCE] != 0)
    b, w, qw = g["it1_base_cur"], g["it1_water_cur"], q["it1_water_cur"]
    assert (b[air][:, 3] == np.float32(50.0 + 273.15)).all() and np.array_equal(w[air][:, 3], qw[air][:, 3] + np.float32(10.0))
    assert np.array_equal(w[~air], qw[~air])
    want = {"land": (3, 3), "stepped_land": (3, 4), "buried": (0, 0), "air": (0, 9)}  # (cells lit, cells of fire ball)
    assert case not in want or (int(lit.sum()), int(air.sum())) == want[case]
    surface = near & (pre[..., DISTANCE] == 0) & (pre[..., VERT_DISTANCE] == 0)
    other = {"inert": INERT, "sea": WATER, "fire": FIRE, "urban": URBAN, "runway": RUNWAY, "industrial": INDUSTRIAL}
    if case in other:  # a surface cell of that type was under the plane, and stayed what it was (a fire that had burnt down to land is land)
        assert (pre[surface][:, 0] == other[case]).any() and air.any() and (post[surface & (pre[..., 0] != LAND)][:, 0] == pre[surface & (pre[..., 0] != LAND)][:, 0]).all()
    if case == "buried":
        assert (pre[near][:, 0] == LAND).all() and (pre[near][:, DISTANCE] == 0).all() and (pre[near][:, VERT_DISTANCE] < 0).all()
    if case == "land":  # iterNum 997: it burns, and at 1000 takes the neighbour on either side
        end = g["it23_wall_cur"]
        fire = (end[..., 0] == FIRE) & (end[..., DISTANCE] == 0) & (end[..., VERT_DISTANCE] == 0)
        assert fire[lit].all() and set(np.nonzero(fire.any(0))[0].tolist()) >= {57, 58, 59, 60, 61} and not fire[:, [56, 62]].any()
        assert (g["it23_water_cur"][np.roll(lit, 1, axis=0)][:, 3] > 0.05).all()


# ---- the oracle against every dump ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TOOL_RUNS + CRASH_RUNS + ["tools64_quiet", "tools64_quiet_nowrap", "crash64_quiet"])
def test_oracle_reproduces_the_reference_on_the_wall_tools(oracle, name):
    g, u, changes = load_run(name)
    assert int(g["points"]) == 1 and int(g["X"]) == int(g["Y"]) == 64
    out = oracle_dumps(oracle, g, u, changes)
    assert check_fields(out, g) == []
