"""The surface scenes (tests/surface_scenes.py) checked without a GPU: which output lanes of the wet kernel's 56-column strips the case
list of tests/test_surface_gpu.py meets ON A SMOOTHING ITERATION (computed from the list: no offset is spare), that the edge and
chimney columns are met, and -- on the oracle the device is compared with -- that every event the scenes exist for HAPPENS and reaches
the neighbouring columns: the exchange between lanes mattered."""
import os
import sys

import numpy as np
import pytest

import impulse_scenes as I
import surface_scenes as S

W = I.WET_STRIP
LANES = (0, 1, 2, W - 3, W - 2, W - 1)  # strip phases of output lanes 4, 5, 6, 57, 58, 59


def _run(oracle, scene, Y, iter0, n, wrap=True):
    base, water, wall = scene[:3]
    X = base.shape[1]
    o = oracle.OracleSim(X, Y, 0)
    try:
        o.upload(base, water, wall)
        o.set_params(S.scene_uniforms(Y, wrap=wrap))
        o.iter = iter0
        o.step(n)
        return o.field("BASE_CUR"), o.field("WATER_CUR"), o.field("WALL_CUR")
    finally:
        o.close()


def _groups(sw):
    cs = [c for c in S.cases() if c["sweep"] == sw["name"]]
    out = {}
    for c in cs:
        out.setdefault((c["kind"], c["variant"], c["wrap"], c["config"]), []).append(c)
    return out


def _lane_misses(X, offsets):
    full = (X // W) * W
    have = {x % W for off in offsets for x in S.site_columns(X, off) if x < full}
    return [ph for ph in LANES if ph not in have] + ([] if any(3 <= ph < W - 3 for ph in have) else ["interior"])


def test_geometry():
    assert np.gcd(S.PITCH, W) == 1 and np.gcd(S.PITCH, 80) == 1
    assert len(S.cases()) >= 1400
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_parity
    for sw in S.SWEEPS:  # every configuration the list names exists, here and in the runner's table
        assert all(k in S.CONFIGS and S.CONFIGS[k][0] in fuzz_parity.IMPULSE_CONFIGS for k in sw["configs"])


@pytest.mark.parametrize("name", [sw["name"] for sw in S.SWEEPS if "lanes" in sw["requires"]])
def test_every_kind_meets_the_strip_lanes_on_a_smoothing_iteration(name):
    """Per (kind, variant, configuration): the sites of the cases that plant THIS kind under THIS configuration meet output lanes
    4, 5, 6, 57, 58, 59 and an interior one; with any one offset left out, something is lost. Every configuration whose first
    iteration smooths is among them, under the display / plain / MORE_TO_COME schedule, stored waterTexture_0 and per-pass."""
    sw = next(s for s in S.SWEEPS if s["name"] == name)
    X = sw["grid"][0]
    groups = _groups(sw)
    assert {k[0] for k in groups} == set(sw["kinds"])
    for key, cs in groups.items():
        offs = [c["offset"] for c in cs]
        assert sorted(offs) == sorted(sw["offsets"])
        assert _lane_misses(X, offs) == [], key
        for drop in offs:
            assert _lane_misses(X, [o for o in offs if o != drop]) != [], (key, "offset", drop, "is spare")
    smoothing_first = {S.CONFIGS[k[3]][:2] for k in groups if S.first_smoothing_iteration(k[3]) == 0}
    its = {it for _, it in smoothing_first}
    assert its >= ({10_000, 9_240_000} if name == "growth" else set(S.SMOOTHING_ITERS))
    for it in its - {9_240_100}:
        assert {kc for kc, i in smoothing_first if i == it} >= ({"wet", "wet_plain", "wet_pieces", "perpass"} | (set() if name == "growth" else {"wet_stored"}))
    if name == "lanes":  # ... and OFF a smoothing iteration: it comes second (99), or not at all (101)
        assert {S.first_smoothing_iteration(k[3]) for k in groups} == {0, 1, None}


@pytest.mark.parametrize("name", [sw["name"] for sw in S.SWEEPS if "edges" in sw["requires"]])
def test_edge_columns(name):
    sw = next(s for s in S.SWEEPS if s["name"] == name)
    X = sw["grid"][0]
    for key, cs in _groups(sw).items():
        cols = {x for c in cs for x in S.site_columns(X, c["offset"])}
        assert cols >= {0, 1, X - 2, X - 1, (X // W) * W}, key
        assert S.first_smoothing_iteration(key[3]) == 0
    assert {k[2] for k in _groups(sw)} == set(sw["wraps"])
    assert X % W != 0  # a ragged last strip


def test_chimney_columns_are_met_and_act(oracle):
    """The chimneys sweep puts industrial cells under x % 80 == 18, 22 and 29 in the first period of 80 columns and beyond it; on the
    oracle the cooling towers add 0.25 of vapour five cells up and the stack smoke six cells up -- and nothing under x % 80 == 28."""
    sw = next(s for s in S.SWEEPS if s["name"] == "chimneys")
    X, Y = sw["grid"]
    met = set()
    for off in sw["offsets"]:
        for variant in sw["variants"]:
            scene = S.surface_scene(X, Y, "industrial", offset=off, variant=variant)
            quiet = S.surface_scene(X, Y, "industrial", offset=off, variant=variant, plant=False)
            (b, w, wl), (b0, w0, _) = _run(oracle, scene, Y, 100, 1), _run(oracle, quiet, Y, 100, 1)
            h = S.heights(X, variant)
            for x in range(X):
                if scene[2][0, x, 0] != S.INDUSTRIAL:
                    continue
                y5, y6 = h[x] + 4, h[x] + 5  # air cells at VERT_DISTANCE 5 and 6
                if x % 80 in (18, 22):
                    assert w[y5, x, 0] > w0[y5, x, 0] + 0.2, (off, variant, x)
                    met.add((x % 80, x >= 80))
                elif x % 80 == 29:
                    assert w[y6, x, 3] > w0[y6, x, 3] + 0.005, (off, variant, x)
                    met.add((29, x >= 80))
                else:
                    assert abs(w[y5, x, 0] - w0[y5, x, 0]) < 0.05 and w[y6, x, 3] < w0[y6, x, 3] + 0.005, (off, variant, x)
                    met.add(("none", x % 80))
    assert met >= {(c, far) for c in S.CHIMNEY_COLUMNS for far in (False, True)}
    assert ("none", 28) in met and ("none", 23) in met  # (neighbours of the stack and of a tower: an off-by-one column would show)


@pytest.mark.parametrize("kind", [k for k in S.KINDS if k != "growth"])
@pytest.mark.parametrize("variant", S.VARIANTS)
def test_the_trigger_reaches_its_neighbours_on_smoothing_iterations_only(oracle, kind, variant):
    """Non-vacuity: on a smoothing iteration (10 000: the fire divisor of the background divides 100) the oracle's surface row differs
    from a run without the trigger in the columns NEXT TO the sites -- what the lanes exchange mattered -- and at 101 it does not."""
    X, Y = S.PHASE_GRID
    h = S.heights(X, variant)
    for off in (0, 3):
        scene, quiet = S.surface_scene(X, Y, kind, offset=off, variant=variant), S.surface_scene(X, Y, kind, offset=off, variant=variant, plant=False)
        reached = {}
        for it0 in (10_000, 101):
            a, q = _run(oracle, scene, Y, it0, 1), _run(oracle, quiet, Y, it0, 1)
            n = 0
            for k, (x, y) in enumerate(scene[3]):
                for xn in ((x - 1) % X, (x + 1) % X):
                    if h[xn] != h[x]:
                        continue  # (stepped: that neighbour is not at VERT_DISTANCE 0 of the same row -- no exchange, asserted below)
                    yn = h[xn] - 1
                    n += int((a[1][yn, xn, 2:] != q[1][yn, xn, 2:]).any() or (a[2][yn, xn] != q[2][yn, xn]).any())
            reached[it0] = n
            if kind == "smoke":  # (it acts on the cell below it: above 4.5 -- site values 5, 5.5, 6, not 4.5 itself -- the site ignites, at 10 000 only)
                lit = [int(a[2][y, x, 0]) == S.FIRE for x, y in scene[3]]
                assert lit == [it0 == 10_000 and S.site_value(kind, k) > 4.5 for k in range(len(lit))], (it0, lit)
            if kind == "industrial":
                # the stretch's end cells smooth towards the land beside them (their snow falls by 2 % of the difference), the land
                # cells beside the stretch do NOT count them (no snow arrives there), the inner cells have no neighbour to average
                for k, (x, y) in enumerate(scene[3]):
                    cols = S.industrial_columns(X, x, S.site_value(kind, k))
                    for xi in (cols[0], cols[-1]):
                        out = (xi - 1) % X if xi == cols[0] else (xi + 1) % X
                        if h[out] == h[xi] and it0 == 10_000:
                            assert a[1][h[xi] - 1, xi, 3] < np.float32(S.INDUSTRIAL_SNOW) * np.float32(0.985)
                            assert a[1][h[out] - 1, out, 3] == 0.0
                        elif it0 == 101:
                            assert a[1][h[xi] - 1, xi, 3] > np.float32(S.INDUSTRIAL_SNOW) * np.float32(0.999)  # (a trace melts)
                    assert all(a[2][h[xi] - 1, xi, 3] == 15 for xi in cols)
        if kind in ("smoke", "industrial"):
            continue
        if kind == "urban":  # (an urban cell stays IN its neighbours' average and carries the background's soil: it shows in its own cell only)
            assert reached == {10_000: 0, 101: 0}
            a, q = _run(oracle, scene, Y, 100, 1), _run(oracle, quiet, Y, 100, 1)
            assert all(a[2][y, x, 3] == 75 and a[2][y, x, 0] == S.URBAN for x, y in scene[3])
        else:
            assert reached[10_000] >= len(scene[3]) and reached[101] == 0, (kind, variant, off, reached)


def test_stepped_neighbours_leave_the_average(oracle):
    X, Y = S.PHASE_GRID
    h = S.heights(X, "stepped")
    seen = 0
    for off in range(9):
        scene, quiet = S.surface_scene(X, Y, "snow", offset=off, variant="stepped"), S.surface_scene(X, Y, "snow", offset=off, variant="stepped", plant=False)
        a, q = _run(oracle, scene, Y, 100, 1), _run(oracle, quiet, Y, 100, 1)
        for x, y in scene[3]:
            for xn in ((x - 1) % X, (x + 1) % X):
                if h[xn] != h[x]:
                    assert np.array_equal(a[1][h[xn] - 1, xn], q[1][h[xn] - 1, xn])
                    seen += 1
    assert seen >= 6


def test_growth_fires_by_rate_and_interval(oracle):
    """Sites of growth rate 1 .. 6 (soil moisture 4 .. 19 under full sunlight), vegetation below the temperature cap except for rate 5:
    at iterNum 10 000 rates 1, 2, 4 grow (intervals 10 000, 5000, 2500; 3300 and 1600 do not divide it), at 9 240 000 rates 3 and 6
    too, at 9 240 100 none -- `(100 / rate) * 100`, not `10000 / rate`."""
    X, Y = S.GROWTH_GRID
    scene = S.surface_scene(X, Y, "growth", offset=2)
    grown = {}
    for it in (10_000, 9_240_000, 9_240_100):
        _, w, wl = _run(oracle, scene, Y, it - S.GROWTH_PREROLL, S.GROWTH_PREROLL + 1)
        grown[it] = [int(wl[y, x, 3]) - int(scene[2][y, x, 3]) for x, y in scene[3]]
    assert len(scene[3]) == 6
    assert grown == {10_000: [1, 1, 0, 1, 0, 0], 9_240_000: [1, 1, 1, 1, 0, 1], 9_240_100: [0] * 6}, grown


def test_the_fire_walks(oracle):
    X, Y = S.PHASE_GRID
    for x0 in (55, 504):
        scene = S.walking_fire_scene(X, Y, x0)
        y = scene[3][0][1]
        o = oracle.OracleSim(X, Y, 0)
        o.upload(*scene[:3])
        o.set_params(S.scene_uniforms(Y))
        o.iter = 995
        widths = []
        for n in (5, 1, 99, 1, 99, 1, 99, 1, 4):
            o.step(n)
            widths.append(int((o.field("WALL_CUR")[y, :, 0] == S.FIRE).sum()))
        o.close()
        assert widths == [1, 3, 3, 5, 5, 7, 7, 9, 9], widths


@pytest.mark.parametrize("kind", S.DIVISOR_KINDS)
def test_divisor_scenes_make_the_divisor_zero_and_negative(oracle, kind):
    """The state after the first iteration (iterNum 1000) carries, in every site, soil moisture / snow that make the fire divisor 0
    (even sites: no ignition, `% 0` is false) and -10 (odd sites: 10 % -10 == 0, they ignite)."""
    X, Y = S.PHASE_GRID
    scene = S.divisor_scene(X, Y, kind, offset=1)
    _, w, wl = _run(oracle, scene, Y, 1000, 1)
    for k, (x, y) in enumerate(scene[3]):
        assert S.expected_divisor(kind, k) == (0 if k % 2 == 0 else -10)
        assert wl[y, x, 0] == (S.LAND if k % 2 == 0 else S.FIRE), (k, w[y, x])
    for variant, off in (("stepped", 0), ("stepped", 2), ("stepped", 4), ("flat", 0)):  # (what tests/test_blowup_gpu.py expects of the device's run)
        sc = S.divisor_scene(X, Y, kind, offset=off, variant=variant)
        _, _, wl2 = _run(oracle, sc, Y, 1000, 5)
        assert [int(wl2[y, x, 0]) == S.FIRE for x, y in sc[3]] == S.divisor_sites_lit(X, sc[3], variant), (variant, off)
    assert S.divisor_sites_lit(X, S.divisor_scene(X, Y, kind, offset=0, variant="stepped")[3], "stepped")[4]  # a raised site is among them
    # ... and with the neighbours at the background's values every site ignites (divisor 10 divides 10): the divisor alone decided
    quiet = S.divisor_scene(X, Y, kind, offset=1)
    for x, y in quiet[3]:
        quiet[1][:y + 1, [(x - 1) % X, (x + 1) % X], 2:] = (S.BACKGROUND["soil"], S.BACKGROUND["snow"])
    _, _, wl = _run(oracle, quiet, Y, 1000, 1)
    assert all(wl[y, x, 0] == S.FIRE for x, y in quiet[3])
