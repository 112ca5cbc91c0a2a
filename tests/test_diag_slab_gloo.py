"""``SlabSim.diagnostics`` (one rank per process, torch.distributed): three gloo ranks on the CPU, each contributing the raw integers of
its own columns -- made here by the kernel's per-cell function on the CPU (wx_diag_accumulate_cells) -- all-gathered, merged in rank
order and rounded locally: every rank gets the numbers of the undecomposed domain; and a rank whose pass fails still takes part in
the one collective, so that all ranks raise instead of hanging."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, WORLD = 90, 7, 3


def _scene():
    rng = np.random.default_rng(8)
    base = (rng.normal(0, 1, (Y, X, 4)) * 2.0 ** rng.integers(-40, 40, (Y, X, 4))).astype(np.float32)
    water = rng.uniform(0, 3, (Y, X, 4)).astype(np.float32)
    wall = np.zeros((Y, X, 4), np.int8)
    wall[..., 1] = rng.integers(0, 3, (Y, X))
    water[..., 0] = np.where(wall[..., 1] == 0, 1111.0, water[..., 0])
    base[3, 40, 1] = np.nan
    return base, water, wall


def _raw(E, cols):
    base, water, wall = _scene()
    raw = E.diag_empty()
    for y in range(Y):
        raw = E.diag_accumulate_cells(raw, X, Y, cols[0], y, base[y, cols], water[y, cols], wall[y, cols])
    return raw


class _Engine:
    def __init__(self, E, rank, fail):
        self.E, self.rank, self.fail = E, rank, fail

    def diagnostics_raw(self):
        if self.fail:
            raise self.E.WxError(-5, "planted failure of this rank's pass")
        xo = X // WORLD
        return _raw(self.E, np.arange(self.rank * xo, (self.rank + 1) * xo))


def _worker(rank, world, port, fail_rank, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wxpkg
    pkg = wxpkg.load_package()
    from weather_sandbox_amd import slab
    s = slab.SlabSim.__new__(slab.SlabSim)  # (the collective alone: no exchange buffers, no device)
    s.engine, s.rank, s.world, s._stage, s.send = _Engine(pkg.engine, rank, rank == fail_rank), rank, world, False, [torch.zeros(1)]
    try:
        res = {"ok": s.diagnostics()}
    except Exception as ex:
        res = {"error": type(ex).__name__ + ": " + str(ex)}
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("fail_rank", [-1, 1])
def test_three_ranks_get_the_undecomposed_numbers_or_all_raise(pkg, tmp_path, fail_rank):
    E = pkg.engine
    E.build()
    mp.spawn(_worker, args=(WORLD, _free_port(), fail_rank, str(tmp_path)), nprocs=WORLD, join=True)
    res = [json.load(open(os.path.join(str(tmp_path), f"r{r}.json"))) for r in range(WORLD)]
    if fail_rank < 0:
        want = json.loads(json.dumps(E.diag_finish(_raw(E, np.arange(X)))))  # (tuples -> lists, as the ranks' results travelled)
        assert want["n_nonfinite_base"] == 1 and want["first_nonfinite_base"] == [40, 3]
        assert all(r == {"ok": want} for r in res)
    else:
        assert all("error" in r for r in res), res
        assert "planted failure" in res[fail_rank]["error"] and all("rank(s) [1]" in res[r]["error"] for r in range(WORLD) if r != fail_rank)
