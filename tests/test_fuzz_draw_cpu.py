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
