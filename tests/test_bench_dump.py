"""bench.py --dump-outputs: the arrays the timed path computed in its last step, reproducible from the arguments alone -- two runs
with the same arguments write the same bytes (whatever the placement search kept and however long the clock conditioning took), --steps
is the number of timed iterations, and a grid too large for the dump's budget is written as a seeded cell sample plus row / column sums."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WET_FIELDS = ["BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_0", "LIGHT_1", "BASE_DISP", "WATER_0", "WALL_DISP", "CURL", "EMITTED"]


def test_conditioning_count_is_a_function_of_the_arguments():
    import bench
    n = bench.conditioning_iterations(16384 * 2048, 10, "wet")
    assert n == 450 and n % 10 == 0  # 0.25 s at 60 000 Mcell-steps/s, whole frames
    assert bench.conditioning_iterations(16384 * 2048, 7, "wet") == 448
    assert bench.conditioning_iterations(32768 * 4096, 10, "dry") == 470
    assert bench.conditioning_iterations(100 * 100, 10, "wet") == 10000  # launch-bound grids: 25 us per iteration


def test_a_plain_run_takes_no_side_measurement(monkeypatch):
    """Without --full every side measurement is off, whatever --no-... options are given; the still-state iterations the timed state
    descends from are run with and without it, and --no-extras alone leaves them out."""
    import bench

    def parsed(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()

    def off(a):
        return [a.no_cpu_baseline, a.no_pmc, a.no_north_star, a.no_arith_fast, a.no_extras]

    a = parsed("--gpus", "1", "--steps", "20", "--warmup", "5")
    assert not a.full and all(off(a)) and a.still_prelude and (a.steps, a.warmup, a.tune, a.frame) == (20, 5, 20, 10)
    a = parsed("--full")
    assert a.full and not any(off(a)) and a.still_prelude
    a = parsed("--full", "--no-pmc", "--no-extras")
    assert off(a) == [False, True, False, False, True] and not a.still_prelude
    a = parsed("--no-extras")
    assert all(off(a)) and not a.still_prelude


def _bench(out_dir, steps, grid, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3", "--X", str(grid[0]), "--Y", str(grid[1]),
           "--no-cpu-baseline", "--no-pmc", "--no-north-star", "--no-arith-fast", "--tune", "2", "--dump-outputs", str(out_dir)] + list(extra)
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    d = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])
    arrays = {f[:-4]: np.load(os.path.join(str(out_dir), f)) for f in sorted(os.listdir(str(out_dir)))}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) == d["dump_outputs"]["bytes"] <= 64 << 20
    assert d["steps"] == steps and d["flow"]["end_of_timed_region"]["rms_v"] > 0.01  # the fluid moved
    return d, arrays


@pytest.mark.gpu
def test_dump_is_reproducible_and_steps_sets_the_timed_iterations(tmp_path):
    X, Y = 512, 128
    d1, a1 = _bench(tmp_path / "a", 7, (X, Y), "--no-extras")
    d2, a2 = _bench(tmp_path / "b", 7, (X, Y), "--no-extras")
    d3, a3 = _bench(tmp_path / "c", 12, (X, Y), "--no-extras")
    assert sorted(a1) == sorted(WET_FIELDS) and d1["dump_outputs"]["cells"] == "all"
    for f in WET_FIELDS:
        assert a1[f].dtype == np.float32 and a1[f].shape == (Y, X, 1 if f == "CURL" else 4), f
        assert a1[f].tobytes() == a2[f].tobytes(), f
    assert np.isfinite(a1["BASE_CUR"]).all() and np.abs(a1["BASE_CUR"][..., :2]).max() > 0.01 and np.abs(a1["LIGHT_1"]).max() > 0
    assert d1["dump_outputs"]["iteration"] == d2["dump_outputs"]["iteration"] == d3["dump_outputs"]["iteration"] - 5
    assert a1["BASE_CUR"].tobytes() != a3["BASE_CUR"].tobytes()


@pytest.mark.gpu
def test_dump_of_a_large_grid_is_a_seeded_sample_with_sums_over_every_cell(tmp_path):
    """With the still-state iterations that run on the timed handle before the fluid is seeded, like the default command -- a plain
    run, and one with the side measurements that --full times around them and after the dump (at_rest, frame_1): the same bytes."""
    X, Y = 1024, 256
    d1, a1 = _bench(tmp_path / "a", 20, (X, Y))
    d2, a2 = _bench(tmp_path / "b", 20, (X, Y), "--full")
    assert "at_rest" in d2 and "frame_1" in d2 and not {"at_rest", "frame_1", "hbm_ceiling", "configs", "cpu_baseline", "north_star_dry", "arith_fast"} & set(d1)
    assert d1["dump_outputs"]["iteration"] == d2["dump_outputs"]["iteration"] == 2 * (3 + 10000 + 20)  # still, then moving: warm-up + conditioning + steps
    assert sorted(a1) == sorted(a2) == sorted(WET_FIELDS + [f + s for f in WET_FIELDS for s in ("_colsum", "_rowsum")])
    K = (32 << 20) // (4 * 37)
    assert K < X * Y
    for f in WET_FIELDS:
        ch = 1 if f == "CURL" else 4
        assert a1[f].shape == (K, ch) and a1[f + "_colsum"].shape == (X, ch) and a1[f + "_rowsum"].shape == (Y, ch), f
        assert a1[f + "_colsum"].dtype == np.float64 and np.allclose(a1[f + "_colsum"].sum(0), a1[f + "_rowsum"].sum(0), rtol=1e-9, atol=1e-9), f
    for k in a1:
        assert a1[k].tobytes() == a2[k].tobytes(), k
    # the sampled cells: the wall type of a cell is in the terrain generator's hands, so the sample can be re-drawn here
    import wxpkg
    pkg = wxpkg.load_package()
    cells = np.sort(np.random.default_rng(0).choice(X * Y, K, replace=False))
    wall = pkg.synth.terrain_grid(X, Y)[2]
    assert np.array_equal(a1["WALL_CUR"][:, 1] != 0, wall.reshape(X * Y, 4)[cells][:, 1] != 0)
