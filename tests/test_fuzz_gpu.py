"""The differential fuzzer (tools/fuzz_parity.py) as a bounded test: a fixed seed's first cases in its modes -- one handle against the CPU
oracle, N slabs against one handle, one handle against the oracle through a drawn HOST SCRIPT (reads in any order, options / parameters /
iteration counter changed mid-run, placement searches and device-side writes between steps), bit for bit -- and the recipes of what the
fuzzer found (tests/golden/fuzz_group_regressions.json, fuzz_script_regressions.json: data, i.e. the drawn parameters of those cases)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


SCRIPT_CASES = 200


@pytest.fixture(scope="module")
def fuzz(pkg):
    import fuzz_parity
    return fuzz_parity


def _run(fuzz, pkg, oracle, mode, seed, n_cases, max_cells=250000):
    rng = np.random.default_rng(seed)
    ran = compared = 0
    for k in range(n_cases):
        c = fuzz.draw_more_sliders(fuzz.draw_case(rng, max_cells))
        if mode == "group":
            c = fuzz.draw_group(rng, c)
            bad, info = fuzz.run_group_case(pkg, pkg.engine, c)
        else:
            bad, info = fuzz.run_case(pkg, pkg.engine, oracle, c)
        ran += 1
        if info.get("error") or info.get("blown_up"):  # a reported overflow / a state that left the number range: nothing to compare
            continue
        compared += 1
        assert not bad, json.dumps({"mode": mode, "seed": seed, "case": k, "recipe": c, "mismatches": bad})
    return ran, compared


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzz_one_handle_against_the_oracle(pkg, oracle, fuzz, seed):
    ran, compared = _run(fuzz, pkg, oracle, "oracle", seed, 150)
    assert compared >= 120, (ran, compared)


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzz_slabs_against_one_handle(pkg, oracle, fuzz, seed):
    ran, compared = _run(fuzz, pkg, oracle, "group", seed, 150)
    assert compared >= 100, (ran, compared)


@pytest.mark.parametrize("seed", [21, 22])
def test_fuzz_surface_life_cycle_against_the_oracle(pkg, oracle, fuzz, seed):
    """Drawn cases with fuzz_parity.draw_surface on top: fire / urban / runway / industrial stretches, vegetation, soil moisture and
    snow over their ranges, the first iteration just below (or on) a multiple of 100 / 1000 / 10 000 / 9 240 000. Seeds of their own:
    the cases of the tests above are what they were."""
    rng = np.random.default_rng(seed)
    compared = smoothing = 0
    for k in range(120):
        c = fuzz.draw_surface(fuzz.draw_more_sliders(fuzz.draw_case(rng, 120000)))
        bad, info = fuzz.run_case(pkg, pkg.engine, oracle, c)
        if info.get("error") or info.get("blown_up"):
            continue
        compared += 1
        it0 = fuzz.case_iter0(c)
        smoothing += int(c["terrain"] and not c["dry"] and any((it0 + j) % 100 == 0 for j in range(sum(c["steps"]))))
        assert not bad, json.dumps({"seed": seed, "case": k, "recipe": c, "mismatches": bad})
    assert compared >= 90 and smoothing >= 15, (compared, smoothing)


@pytest.mark.parametrize("mode,seed", [("oracle", 31), ("oracle", 32), ("group", 33), ("group", 34)])
def test_fuzz_sun_at_exact_slider_positions(pkg, oracle, fuzz, mode, seed):
    """Drawn cases with fuzz_parity.draw_sun_exact on top: from the second step on the sun stands at GUI -10, 0, 90, 180, 190 or within
    1e-6 degrees of 90 / 180 -- the positions the continuum of draw_case never hits, where the lighting pass's tap reads columns x + 1, x + 2
    or rows y + 1, y + 2 (tests/light_scenes.py). Seeds of their own: the cases of the tests above are what they were."""
    rng = np.random.default_rng(seed)
    compared, wet, seen = 0, 0, set()
    for k in range(60):
        c = fuzz.draw_more_sliders(fuzz.draw_case(rng, 60000))
        if mode == "group":
            c = fuzz.draw_group(rng, c)
        c = fuzz.draw_sun_exact(c)
        assert c["sun_exact"] in fuzz.SUN_EXACT and len(c["steps"]) >= 2
        bad, info = fuzz.run_group_case(pkg, pkg.engine, c) if mode == "group" else fuzz.run_case(pkg, pkg.engine, oracle, c)
        if info.get("error") or info.get("blown_up"):
            continue
        compared += 1
        wet += int(not c["dry"])
        seen.add(c["sun_exact"]) if not c["dry"] else None
        assert not bad, json.dumps({"mode": mode, "seed": seed, "case": k, "recipe": c, "mismatches": bad})
    assert compared >= 40 and wet >= 20 and len(seen) >= 7, (compared, wet, sorted(seen))


def test_fuzz_regressions_of_round_6(pkg, fuzz):
    recs = json.load(open(os.path.join(ROOT, "tests", "golden", "fuzz_group_regressions.json")))
    assert len(recs) >= 3
    for r in recs:
        bad, info = fuzz.run_group_case(pkg, pkg.engine, r["recipe"])
        assert not info.get("error"), info
        assert not bad, json.dumps({"recipe": r["recipe"], "mismatches": bad})


@pytest.mark.parametrize("seed", [13, 14])
def test_fuzz_host_scripts_against_the_oracle(pkg, oracle, fuzz, seed):
    """--mode script: the scenes of the seed's oracle mode, each driven through a host script drawn from a generator of its own. Every
    kind of host action occurs at least ten times over the run (the runner counts what it performed)."""
    rng, rng_script = np.random.default_rng(seed), np.random.default_rng(seed + 2000003)
    compared, reads, actions = 0, 0, {k: 0 for k in fuzz.SCRIPT_ACTIONS}
    for k in range(SCRIPT_CASES):
        c = fuzz.draw_script(rng_script, fuzz.draw_more_sliders(fuzz.draw_case(rng, 250000)))
        bad, info = fuzz.run_script_case(pkg, pkg.engine, oracle, c)
        for kind, n in info["actions"].items():
            actions[kind] += n
        if info.get("error") or info.get("blown_up"):
            continue
        compared += 1
        reads += info["reads"]
        assert not bad, json.dumps({"mode": "script", "seed": seed, "case": k, "recipe": c, "mismatches": bad})
    assert compared >= SCRIPT_CASES * 4 // 5, compared
    assert reads >= 20 * compared, (reads, compared)
    assert min(actions.values()) >= 10, actions


def test_fuzz_script_regressions(pkg, oracle, fuzz):
    """What --mode script found: BASE_DISP after a device-side write to BASE_CUR, the feedback texture's alpha after the particles
    were switched off."""
    recs = json.load(open(os.path.join(ROOT, "tests", "golden", "fuzz_script_regressions.json")))
    assert len(recs) >= 2
    for r in recs:
        bad, info = fuzz.run_script_case(pkg, pkg.engine, oracle, r["recipe"])
        assert not info.get("error") and not info.get("blown_up"), info
        assert not bad, json.dumps({"why": r["why"], "mismatches": bad})
