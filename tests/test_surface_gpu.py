"""Surface life cycle on the device: the lone surface cells of tests/surface_scenes.py (a snow heap, a soil-moisture spike, a fire, an
industrial stretch under the chimney columns, an urban cell, a cell one growth step from its cap, smoke above 4.5) against the CPU
oracle, bit for bit on every field both define -- with the trigger's first iteration ON a smoothing iteration (iterNum 100, 10 000,
9 240 000: the marching wet kernel's `smooth_iter` exchange between lanes exists on those only) and off it (99, 101), in a display
iteration, a plain one and a WX_OVERLAP_MORE_TO_COME piece, with stored and on-demand waterTexture_0, on the per-pass kernels, under
ROW_BANDS 0 / 1 / 2 on a low wide grid, at the strip seams, the wrap seam (wrap on and off) and the ragged last strip; a fire that
walks four cells each way across a strip seam over 310 iterations; slab groups with the site at a slab seam, stepped across an
exchange period that contains a smoothing iteration. tests/test_surface_cpu.py accounts for what the case list reaches."""
import json
import os
import sys

import numpy as np
import pytest

import impulse_scenes as I
import surface_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CASES = S.cases()


@pytest.fixture(scope="module")
def fuzz(pkg):
    import fuzz_parity
    pkg.engine.build()
    return fuzz_parity


@pytest.mark.parametrize("sweep,kind", sorted({(c["sweep"], c["kind"]) for c in CASES}))
def test_lone_surface_cells_vs_oracle(pkg, oracle, fuzz, sweep, kind):
    """Every case of one sweep and kind. A mismatch stops at its first case and prints the recipe (surface_scenes.build_case rebuilds it)."""
    mine = [c for c in CASES if c["sweep"] == sweep and c["kind"] == kind]
    assert mine
    fires = 0
    for c in mine:
        kc, iter0, preroll = S.CONFIGS[c["config"]]
        scene = S.build_case(c)
        bad, wall = S.run_scene(pkg, fuzz, oracle, scene, c["X"], c["Y"], kc, iter0, fuzz.IMPULSE_CONFIGS[kc].get("steps", (1, 1, 3)), wrap=c["wrap"], preroll=preroll)
        assert not bad, json.dumps({"recipe": c, "mismatches": bad})
        fires += int(((wall[..., 0] == S.FIRE) & (wall[..., 2] == 0)).sum())
    if kind == "fire":
        assert fires >= len(mine)  # (what spread where is the CPU test's: here only that the fires were still there to be compared)
    print(json.dumps({"sweep": sweep, "kind": kind, "cases": len(mine)}))


@pytest.mark.parametrize("kernel_config", ["wet", "wet_stored", "perpass"])
@pytest.mark.parametrize("x0", [55, 56, 111, 504, 0])
def test_a_fire_walks_across_the_seams(pkg, oracle, fuzz, kernel_config, x0):
    """surface_scenes.walking_fire_scene from iterNum 995: one cell each way at 1000, 1100, 1200 and 1300 -- across the seam between two
    56-column strips (x0 55 / 56 / 111) and across the wrap seam (504 / 0), compared after every stage."""
    X, Y = S.PHASE_GRID
    scene = S.walking_fire_scene(X, Y, x0)
    bad, wall = S.run_scene(pkg, fuzz, oracle, scene, X, Y, kernel_config, 995, (5, 1, 99, 1, 99, 1, 99, 1, 4))
    assert not bad, json.dumps({"x0": x0, "mismatches": bad})
    y = scene[3][0][1]
    assert [int(wall[y, (x0 + d) % X, 0]) for d in range(-5, 6)] == [S.LAND] + [S.FIRE] * 9 + [S.LAND]


@pytest.mark.parametrize("nslab", [2, 4, 8])
@pytest.mark.parametrize("kind", ["snow", "soil", "fire", "smoke"])
def test_surface_cells_on_slabs_equal_the_whole_domain(pkg, nslab, kind):
    """A slab group on one GPU (halo 12) against the undecomposed handle: a site in the last owned column of a slab, in its first
    ghost column and mid-slab, stepped from iterNum 9 995 across iteration 10 000 (smoothing; fire and smoke spread) in steps that
    put it inside an exchange period and at its start."""
    E = pkg.engine
    X, Y, halo = 1008, 77, 12
    xo = X // nslab
    u = S.scene_uniforms(Y)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    for ox, steps in ((xo - 1, (3, 4, 3)), (xo, (5, 1, 4)), (xo // 2, (7, 3)), (X - 1, (5, 5))):
        base, water, wall, sites = S.surface_scene(X, Y, kind, offset=ox)
        g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
        whole = E.Handle(X, Y, 0)
        try:
            g.upload(base, water, wall)
            whole.upload(base, water, wall)
            g.set_params(p, u["initial_T"])
            whole.set_params(p, u["initial_T"])
            for h in g.slabs:
                h.iter = 9995
            whole.iter = 9995
            for n in steps:
                g.step(n)
                whole.step(n)
                for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_1", "WATER_0"):
                    a, b = g.read(f), whole.read_rect(f)
                    assert np.array_equal(a, b), (nslab, ox, I.describe_difference(f, a, b, sites, X))
            if kind == "fire":
                w = whole.read_rect("WALL_CUR")
                assert all(w[y, (x + d) % X, 0] == S.FIRE for x, y in sites for d in (-1, 0, 1))  # it did cross the seam
        finally:
            g.close()
            whole.close()
