"""Impulse-lattice parity: lone single-cell triggers (tests/impulse_scenes.py) at every lane, row and tile phase of the marching
kernels, on every kernel configuration, against the CPU oracle bit for bit -- every field both sides define, after 1, 2 and 5
iterations (pairs: 2, 4, 5; schedules that put the trigger into a plain iteration: 3, 5). The case list is impulse_scenes.cases(); tests/test_impulse_cpu.py accounts for the phases it reaches. The
runner is tools/fuzz_parity.py's (--mode impulse soaks drawn lattices with it). Besides equality: the rare paths RAN where the ABI can
say so (wx_fastest_velocity, wx_pair_stats), and the default splat order (fp32 atomics) equals the oracle exactly while the
sprites of the lone droplets stay disjoint."""
import json
import os
import sys

import numpy as np
import pytest

import impulse_scenes as I

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = I.cases()


@pytest.fixture(scope="module")
def fuzz(pkg):
    import fuzz_parity
    pkg.engine.build()
    return fuzz_parity


def _check(fuzz, c, bad, info):
    assert not info["blown_up"], (c, info)
    assert not bad, json.dumps({"recipe": c, "mismatches": bad, "info": info})
    if "fastest" in info:  # the wet marching kernel's exact path saw exactly the cells the oracle says are fast
        assert info["fastest"] == info["fastest_expected"], (c, info)
    if "water_free" in info:
        assert info["water_free"], (c, info)  # the dry kinds leave the agreed water-free state water-free: the water-free kernels run
    if "pair_stats" in info:
        fixed, repeated = info["pair_stats"]
        assert info["pair_launches"] >= 2, (c, info)  # the pair kernel is what ran (no silent fall-back to single iterations)
        assert info.get("prime_pair_stats", (0, 0)) == (0, 0), (c, info)
        assert fixed % 81 == 0, (c, info)  # 9 x 9 outputs per recorded tile
        if info["second_iteration_fast"]:  # no exact path inside the march for those: recorded (or the pair repeated whole)
            assert fixed > 0 or repeated > 0, (c, info)
        if fixed > 0 or repeated > 0:  # ... and nothing is recorded in a flow that stays below 0.9 (first-iteration cells: the TAINT instantiation)
            assert info["second_iteration_fast"] or info["first_iteration_fast"], (c, info)
    if c["kind"] == "droplet":
        assert info["sprites_disjoint_until"] >= 1, (c, info)


@pytest.mark.parametrize("sweep,kind", sorted({(c["sweep"], c["kind"]) for c in CASES}))
def test_lone_triggers_vs_oracle(pkg, oracle, fuzz, sweep, kind):
    """Every case of one sweep and kind (every offset under every configuration of the sweep). A mismatch stops the test at its first
    case and prints the recipe: impulse_scenes.build_case(recipe) rebuilds the scene, tools/fuzz_parity.run_impulse_case runs it alone."""
    mine = [c for c in CASES if c["sweep"] == sweep and c["kind"] == kind]
    assert mine
    seen = {}
    for c in mine:
        bad, info = fuzz.run_impulse_case(pkg, pkg.engine, oracle, c, I)
        _check(fuzz, c, bad, info)
        r = seen.setdefault(c["config"], {"cases": 0, "fastest_max": 0.0, "cells_recomputed": 0, "pairs_repeated": 0, "second_iteration_fastest": 0.0, "disjoint": []})
        r["cases"] += 1
        r["fastest_max"] = max(r["fastest_max"], info.get("fastest", 0.0))
        r["cells_recomputed"] += info.get("pair_stats", (0, 0))[0]
        r["pairs_repeated"] += info.get("pair_stats", (0, 0))[1]
        r["second_iteration_fastest"] = max(r["second_iteration_fastest"], info.get("second_iteration_fastest", 0.0))
        if info.get("sprites_disjoint_until") is not None:
            r["disjoint"].append(info["sprites_disjoint_until"])
    for config, r in seen.items():
        cfg = fuzz.IMPULSE_CONFIGS[config]
        wet_march = not cfg.get("dry") and cfg.get("kernel_set", 1) == 1 and kind != "droplet"
        if kind in ("fast_vx", "fast_vy") and wet_march:
            assert r["fastest_max"] >= 2.0, (config, r)  # the planted 7.5 / 3.0 / 2.99 cells went through the wet kernel's exact path
        if kind in ("fast_vx", "fast_vy") and cfg.get("dry") and cfg.get("pairs", 1) and cfg.get("kernel_set", 1):
            # (tests/test_impulse_cpu.py pins it on the oracle) the 20 / 80 sites are still fast in a SECOND iteration: the pair kernel's own exact path ran
            assert r["second_iteration_fastest"] >= 0.9 and r["cells_recomputed"] > 0, (config, r)
        if kind in ("T_spike", "P_spike", "smoke", "cloud", "precip_visual", "wall"):
            assert r["fastest_max"] == 0.0 and r["cells_recomputed"] == 0 and r["pairs_repeated"] == 0, (config, r)  # these stay on the common path
        if kind == "droplet":
            assert max(r["disjoint"]) >= 5, (config, r)  # the whole coupled run was compared exactly
    print(json.dumps({"sweep": sweep, "kind": kind, "by_config": seen}))


@pytest.mark.parametrize("nslab", [2, 3])
@pytest.mark.parametrize("kind", ["smoke", "wall", "fast_vx", "fast_vy", "cloud"])
def test_lone_triggers_on_slabs_equal_the_whole_domain(pkg, fuzz, nslab, kind):
    """A slab group on one GPU (wx_group_*, halo 12) against the undecomposed handle: the lattice moved so that sites fall on the
    first and the last owned column of a slab, into its ghost columns and next to the seam. Fast cells stay below 3 cells / iteration
    (a halo of 12 columns carries a cone of 9)."""
    E = pkg.engine
    X, Y, halo = 1008, 77, 12
    xo = X // nslab
    u = I.scene_uniforms(kind, Y)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    for ox in (0, xo - 1, xo, xo - halo, xo + halo - 1, X - 1):
        base, water, wall, _, sites = I.impulse_scene(X, Y, kind, offset=(ox, 3 + ox % 7), fast_values=(0.9, 1.3, 2.0, 2.9))
        g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
        whole = E.Handle(X, Y, 0)
        try:
            g.upload(base, water, wall)
            whole.upload(base, water, wall)
            g.set_params(p, u["initial_T"])
            whole.set_params(p, u["initial_T"])
            for n in (1, 1, 3):
                g.step(n)
                whole.step(n)
                for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_0", "LIGHT_1", "BASE_DISP", "WATER_0"):
                    a, b = g.read(f), whole.read_rect(f)
                    assert np.array_equal(a, b), (nslab, ox, I.describe_difference(f, a, b, sites, X))
        finally:
            g.close()
            whole.close()
