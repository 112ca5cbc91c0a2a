"""The drawing of tools/fuzz_parity.py, pinned without a GPU: the seeds the GPU tests run (tests/test_fuzz_gpu.py) keep drawing the
cases they drew before the host-script layer existed, and a script is a pure function of its seed."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_parity  # noqa: E402

# sha256 of json.dumps(recipes, sort_keys=True) of the first 150 cases, computed on the commit before --mode script was added
DIGESTS = {
    ("oracle", 11): "14b4973b6cb14562e38c81bf86e38b30778e9d9c23f694caefc7a48c0d26a1a0",
    ("oracle", 12): "886ce2e8a4357a7ba9bad50cba93844dc6ff18a82f8340551c9829e96ae6ff0a",
    ("group", 11): "989c98d1b2e4633a41dfd7d8b96a90558297484cc359e002aeca198e906a176c",
    ("group", 12): "2d8ccbb581f3d88f9ac170b9e5d491365702a64d323ef636cf5d09d02bb92012",
}


# sha256 of json.dumps of the "surface" entries draw_surface adds to the first 150 cases of seed 11
SURFACE_DIGEST = "73dc00380a0eefaecfb41cf57eee0e2dcb43c441c29c7fa9809c53dc84878195"


def _recipes(mode, seed, n=150):
    rng, rng_script = np.random.default_rng(seed), np.random.default_rng(seed + 2000003)
    out = []
    for _ in range(n):
        c = fuzz_parity.draw_case(rng, 250000)
        if mode == "group":
            c = fuzz_parity.draw_group(rng, c)
        if mode == "script":
            c = fuzz_parity.draw_script(rng_script, c)
        out.append(c)
    return out


@pytest.mark.parametrize("mode,seed", sorted(DIGESTS))
def test_existing_seeds_draw_the_cases_they_drew(mode, seed):
    assert hashlib.sha256(json.dumps(_recipes(mode, seed), sort_keys=True).encode()).hexdigest() == DIGESTS[(mode, seed)]


def test_the_added_sliders_come_from_the_shared_table_and_cover_it():
    """One table of GUI ranges (params.GUI_RANGES): the fuzzer's 17 first sliders are its first 17 entries (four with the fuzzer's own,
    stated interval), the added ones (draw_more_sliders: a function of the case, no draw from its generator, so the digests above
    hold) lie inside the GUI's range, every one of them within 300 cases, and a recipe without the key -- the committed regressions --
    draws none."""
    R = fuzz_parity._GUI_RANGES
    assert list(fuzz_parity.SLIDERS) == list(R)[:17] and set(fuzz_parity.SLIDERS_MORE) <= set(R)
    assert {k for k in fuzz_parity.SLIDERS if fuzz_parity.SLIDERS[k] != R[k]} == set(fuzz_parity.FUZZ_INTERVALS)
    assert not (set(fuzz_parity.SLIDERS) | set(fuzz_parity.SLIDERS_MORE)) - set(fuzz_parity.wxpkg.load_package().params.GUI_DEFAULTS)
    seen = {}
    more = lambda n: [fuzz_parity.draw_more_sliders(c)["sliders_more"] for c in _recipes("oracle", 11, n)]
    for sm in more(300):
        for k, v in sm.items():
            lo, hi = R[k]
            assert lo <= v <= hi
            seen.setdefault(k, []).append((v - lo) / (hi - lo))
    assert set(seen) == set(fuzz_parity.SLIDERS_MORE)
    assert all(min(v) < 0.1 and max(v) > 0.9 for v in seen.values())
    assert more(20) == more(20) and all("sliders_more" not in c for c in _recipes("oracle", 11, 20))
    for f in ("fuzz_group_regressions.json", "fuzz_script_regressions.json"):
        with open(os.path.join(ROOT, "tests", "golden", f)) as fh:
            assert all("sliders_more" not in r["recipe"] for r in json.load(fh))


def test_scripts_are_a_function_of_the_seed_and_leave_the_scenes_alone():
    a, b = _recipes("script", 13), _recipes("script", 13)
    assert json.dumps(a) == json.dumps(b) and json.dumps(a) != json.dumps(_recipes("script", 14))
    plain = _recipes("oracle", 13)
    for c, p in zip(a, plain):  # the scene of a script case is the oracle mode's: only the script and the step list it implies are new
        assert {k: v for k, v in c.items() if k not in ("script", "steps")} == {k: v for k, v in p.items() if k != "steps"}
        assert c["steps"] == [s["n"] for s in c["script"] if s["op"] == "step"] and 2 <= len(c["steps"]) <= 5
        assert all(s["op"] in fuzz_parity.SCRIPT_ACTIONS + ["step"] for s in c["script"])
    kinds = {s["op"] for c in a for s in c["script"]}
    assert kinds == set(fuzz_parity.SCRIPT_ACTIONS + ["step"]) - {"pieces"}, kinds
    assert any(s.get("first_piece") for c in a for s in c["script"])
    json.loads(json.dumps(a))  # a recipe is plain JSON: it alone reproduces the case


def test_the_surface_draw_is_a_function_of_the_case_and_reaches_the_life_cycle():
    """draw_surface adds the recipe key "surface" without a draw from the case's generator (the digests above hold, recipes without the
    key run as before), is pinned by a digest of its own, and over 300 cases reaches every surface type, vegetation on both sides of
    the fire floor (20) and the bare-soil limit (10), soaked and dry soil, snow, and a first iteration at most 8 below a multiple of
    100, 1000, 10 000 and 9 240 000 -- among them runs that START on such a multiple."""
    cs = [fuzz_parity.draw_surface(c)["surface"] for c in _recipes("oracle", 11, 300)]
    assert cs == [fuzz_parity.draw_surface(c)["surface"] for c in _recipes("oracle", 11, 300)]
    assert hashlib.sha256(json.dumps(cs[:150], sort_keys=True).encode()).hexdigest() == SURFACE_DIGEST
    assert all("surface" not in c for c in _recipes("oracle", 11, 20))
    st = [s for c in cs for s in c["stretches"]]
    assert {s[2] for s in st} == set(fuzz_parity.SURFACE_TYPES)
    veg, soil, snow = [s[3] for s in st], [s[4] for s in st], [s[5] for s in st]
    assert min(veg) < 10 and any(10 <= v < 20 for v in veg) and max(veg) > 100 and 0 <= min(veg) and max(veg) <= 127
    assert min(soil) == 0.0 and max(soil) > 500.0 and max(soil) <= 1000.0 and max(snow) > 1000.0 and max(snow) <= 4000.0
    its = [c["iter0"] for c in cs if c["iter0"] is not None]
    assert 100 < len(its) < 250
    for base in (100, 1000, 10000, 9240000):
        assert any(0 < (-i) % base <= 8 for i in its) and any(i % base == 0 for i in its), base
    c = fuzz_parity.draw_surface(_recipes("oracle", 11, 1)[0])
    assert fuzz_parity.case_iter0(c) == (c["iter0"] if c["surface"]["iter0"] is None else c["surface"]["iter0"])
    for f in ("fuzz_group_regressions.json", "fuzz_script_regressions.json"):
        with open(os.path.join(ROOT, "tests", "golden", f)) as fh:
            assert all("surface" not in r["recipe"] for r in json.load(fh))
