"""What the case list of tests/tool_scenes.py reaches, computed from the list itself and from the CPU oracle -- no GPU: every
(tool, sign) meets every class of cell inside and outside the disc; the disc's rim, on the surface row, falls on a seam of the
56-column strips, of the 60-column strips, on the ragged last strip of either, on the wrap seam with the wrap on and off and on
columns 0, 1, X-2, X-1; no cell lies within 1e-5 of a rim; no placement is spare; every (tool, sign) meets every kernel
configuration; on the oracle every scene stays finite and slow, and the facts of tests/test_oracle_tools.py's table -- written from
the shader -- hold for these scenes as they do for the reference's dumps."""
import numpy as np
import pytest

import impulse_scenes as I
import test_oracle_tools as R
import tool_scenes as T

CASES = T.cases()
X, Y = T.GRID


def _surface_inside(c):
    """Per column: is the flat surface row's cell inside the disc?"""
    left, wrap = T.placements(c["X"])[c["placement"]]
    v = T.brush_values(c["X"], c["Y"], left, wrap, 0.01)
    return T.inside(c["X"], c["Y"], v, wrap)[T.GROUND - 1]


def _flips(row):
    """Column boundaries b (1 .. X, X = the wrap seam) where column b - 1 and column b % X differ."""
    return {b for b in range(1, len(row) + 1) if row[b - 1] != row[b % len(row)]}


def test_the_case_list_is_the_full_product():
    keys = {(c["tool"], c["sign"], c["placement"], c["held"]) for c in CASES}
    assert len(keys) == len(CASES) == len(T.WALL_TOOLS) * 2 * len(T.placements(X)) * len(T.HELD)
    for tool in T.WALL_TOOLS:
        for sign in T.SIGNS:
            mine = [c for c in CASES if c["tool"] == tool and c["sign"] == sign]
            assert {c["config"] for c in mine} == set(T.CONFIG_CYCLE) and {c["variant"] for c in mine} == set(T.VARIANTS)
            assert {(c["config"], c["held"]) for c in mine} >= {("wet_pieces", 3), ("wet_plain", 3), ("wet", 1), ("perpass", 1), ("wet_stored", 3)}


def test_every_rim_is_on_a_seam_and_no_placement_is_spare():
    wet, dry = I.WET_STRIP, I.DRY_STRIP
    want = {"wet_seam": {wet, 2 * wet}, "dry_seam": {dry, 2 * dry}, "ragged_wet": {(X // wet) * wet}, "ragged_dry": {(X // dry) * dry}, "wrap": {X},
            "col0|1": {1}, "col1|2": {2}, "X-2|X-1": {X - 1}}
    met_on, met_off, used = set(), set(), set()
    for name, (left, wrap) in T.placements(X).items():
        c = {"X": X, "Y": Y, "placement": name}
        row = _surface_inside(c)
        assert row.sum() in ((30,) if wrap or 0 <= left <= X - 30 else (29,)), (name, int(row.sum()))
        flips = _flips(row) if wrap else {b for b in _flips(row) if b != X} | ({X} if row[0] != row[-1] else set())
        side = lambda b: "left" if row[b % X] else "right"  # the rim at boundary b: the disc begins there, or ends
        mine = {(side(b), k) for k, seams in want.items() for b in flips & seams}
        if not wrap and (left < 0 or left + 30 > X):
            mine.add(("left" if left < 0 else "right", "cut"))  # part of the disc lies beyond the edge: with the wrap on it would come back in at the other side
        assert mine, name
        if not (mine <= (met_on if wrap else met_off)):
            used.add(name)
        (met_on if wrap else met_off).update(mine)
        assert T.rim_clear(X, Y, T.brush_values(X, Y, left, wrap, 0.01), wrap)
    assert {k for _, k in met_on} == set(want), set(want) - {k for _, k in met_on}
    assert {("left", "wrap"), ("right", "wrap"), ("left", "col0|1"), ("right", "X-2|X-1"), ("left", "X-2|X-1"), ("right", "col0|1")} <= met_on  # the wrap seam and its neighbours from both sides
    assert {("left", "wrap"), ("right", "wrap"), ("right", "X-2|X-1"), ("left", "col0|1"), ("left", "cut"), ("right", "cut")} <= met_off  # wrap off: the rim AT the edge from both sides, and a disc the edge cuts
    assert used == set(T.placements(X)), set(T.placements(X)) - used  # each placement brought a seam or side the ones before it had not
    cut = T.placements(X)["nowrap_cut_right"]
    on, off = (T.inside(X, Y, T.brush_values(X, Y, cut[0], w, 0.01), w)[T.GROUND - 1] for w in (True, False))
    assert on[0] and not off[0] and on[1:].tolist() == off[1:].tolist()  # what the wrap decides: column 0


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_every_disc_meets_every_class_of_cell_inside_and_outside(variant):
    base, water, wall, h = T.background(X, Y, variant)
    assert set(np.unique(wall[..., 3][wall[..., 1] == 0])) >= {0, 1, 60, 126, 127} and (water[..., 3][wall[..., 1] == 0] > 0).any()
    classes = T.cell_classes(wall)
    assert all(m.any() for m in classes.values())
    if variant == "stepped":
        assert not any(h[c] < h[c - 1] and h[c] < h[(c + 1) % X] for c in range(X))  # no pit one cell wide
        t = T.column_types(X)
        assert {int(v) for v in t[h == T.GROUND + 1]} == set(range(7)) == {int(v) for v in t[h == T.GROUND - 1]}  # every type raised and lowered somewhere
    for name, (left, wrap) in T.placements(X).items():
        m_in = T.inside(X, Y, T.brush_values(X, Y, left, wrap, 0.01), wrap)
        for cname, m in classes.items():
            assert (m & m_in).any() and (m & ~m_in).any(), (name, cname)


def _run(oracle, c, scene, u_held, u_free, after):
    o = oracle.OracleSim(c["X"], c["Y"], 0)
    try:
        o.upload(*scene[:3])
        o.iter = T.ITER0
        o.set_params(u_held)
        o.step(1)
        first = (o.field("BASE_CUR"), o.field("WATER_CUR"), o.field("WALL_CUR"))
        if c["held"] > 1:
            o.step(c["held"] - 1)
        o.set_params(u_free)
        vmax = 0.0
        for _ in range(after):
            o.step(1)
            b = o.field("BASE_CUR")
            assert np.isfinite(b).all() and np.isfinite(o.field("WATER_CUR")).all(), c
            vmax = max(vmax, float(np.abs(b[..., :2]).max()))
        return first, o.field("WALL_CUR"), vmax
    finally:
        o.close()


@pytest.mark.parametrize("tool", T.WALL_TOOLS)
@pytest.mark.parametrize("sign", T.SIGNS)
def test_scenes_stay_finite_and_the_table_holds_on_the_oracle(oracle, tool, sign):
    """Every case of one (tool, sign) on the oracle: finite after every iteration, slower than the 2 cells per iteration a slab halo of
    12 carries; and after the first held iteration the wall texture is the table's edit of a run without the tool, the seeds of a
    new wall (1000 K / soil moisture 25 / waterTemperature) and of a removed cell (the start sounding of its row, no water) included."""
    mine = [c for c in CASES if c["tool"] == tool and c["sign"] == sign]
    quiet = {}
    for c in mine:
        scene = T.build_case(c)
        held, free = T.tool_uniforms(c)
        left, wrap = T.placements(c["X"])[c["placement"]]
        k = (c["variant"], wrap)
        if k not in quiet:
            quiet[k] = _run(oracle, dict(c, held=1), scene, free, free, 0)[0]
        (b, w, post), end, vmax = _run(oracle, c, scene, held, free, T.AFTER)
        assert vmax < 2.0, (c, vmax)
        qb, qw, pre = quiet[k]
        m_in = T.inside(c["X"], c["Y"], held["userInputValues"], wrap)
        row = np.arange(c["Y"])[:, None] + np.zeros(c["X"], np.int64)
        exp, fields, removed, made = R.expected_edit(tool, sign, pre, m_in, row)
        assert np.array_equal(post, np.minimum(exp, 127).astype(np.int8)), c
        ch, delta = {20: (2, 10.0), 21: (3, 0.5)}.get(tool, (2, 0.0))
        moved = qw.copy()
        moved[fields, ch] += np.float32(held["userInputValues"][2]) * np.float32(delta)
        keep = ~(made | removed)
        assert np.array_equal(w[keep], moved[keep]), c
        if made.any():
            assert (b[made][:, 3] == (np.float32(held["waterTemperature"]) if tool == 12 else 1000.0)).all() and (tool != 11 or (w[made][:, 2] == 25.0).all())
        if removed.any():
            assert np.array_equal(b[removed][:, 3], np.asarray(held["initial_T"], np.float32)[row[removed]]) and (w[removed] == 0).all() and not removed[0].any()
        if tool == 13 and sign > 0 and c["placement"] == "left@wet_seam":
            lit = (post[..., 0] == R.FIRE) & (pre[..., 0] == R.LAND)
            assert lit.any() and ((end[..., 0] == R.FIRE) & lit).any()  # still burning 20 iterations after release


def test_the_crash_on_the_oracle_lights_surface_land_only(oracle):
    base, water, wall, h = T.background(X, Y, "stepped")
    t = T.column_types(X)
    o = oracle.OracleSim(X, Y, 0)
    o.upload(base, water, wall)
    o.iter = 997
    o.set_params(T.scene_uniforms(Y))
    o.step(1)
    pre = o.field("WALL_CUR")  # without a plane: what the boundary pass of iteration 997 leaves
    o.close()
    for x in (6, 1, 9, 13, 17, 21, 25, 34):  # land beside its raised column, the other six types, land beside its lowered columns
        for y in (int(h[x]) - 1, int(h[x]) - 2, 20):  # the surface cell, the buried one under it, open air
            u = dict(T.scene_uniforms(Y), airplaneValues=T.crash_values(X, Y, x, y))
            o = oracle.OracleSim(X, Y, 0)
            o.upload(base, water, wall)
            o.iter = 997
            o.set_params(u)
            o.step(1)
            post = o.field("WALL_CUR")
            o.set_params(dict(u, airplaneValues=T.NO_PLANE))
            o.step(4)
            end = o.field("WALL_CUR")
            o.close()
            near = (np.abs(np.arange(X)[None, :] - x) <= 1) & (np.abs(np.arange(Y)[:, None] - y) <= 1)
            changed = (post != pre).any(-1)
            want = near & (pre[..., 1] == 0) & (pre[..., 0] == R.LAND) & (pre[..., 2] == 0)
            assert np.array_equal(changed, want) and (post[want][:, 0] == R.FIRE).all(), (x, y)
            if t[x] == R.LAND and y == h[x] - 1:
                assert want.sum() >= 2 and (end[want][:, 0] == R.FIRE).any()  # lit at 997, burning at 1001 (vegetation 0 and 1 burn down at once)
