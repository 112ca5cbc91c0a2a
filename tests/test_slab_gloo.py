"""Multi-process (world_size 2 and 3, gloo, CPU) test of the slab decomposition + ring halo exchange.

The driver under test is the product's ``slab.SlabSim`` (exchange pattern, iterations-per-exchange logic, slab
geometry); the compute engine plugged into it here is the CPU oracle (tests may use the oracle as checker), so
the test proves: N slabs + halo exchange == the undecomposed domain, BIT FOR BIT, for all grid fields.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pool_model import ModelPoolEngine  # the numpy model of the pool kernels, shared with tests/test_pool_exchange_*.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HALO_FIELDS = ("BASE_CUR", "WATER_CUR", "LIGHT_0", "LIGHT_1", "WALL_CUR")


class OracleSlabEngine:
    """slab-engine interface on top of the CPU oracle (x_off / X_global geometry, numpy halo pack)."""

    def __init__(self, wx_oracle, X_global, Y, x0, X_owned, halo):
        self.halo, self.Y = halo, Y
        self.X = X_owned + 2 * halo
        self.sim = wx_oracle.OracleSim(self.X, Y, 0, X_global=X_global, x_off=x0 - halo)

    def upload(self, base, water, wall):
        self.sim.upload(base, water, wall)

    def set_params(self, u):
        self.sim.set_params(u)

    def new_buffer(self):
        n = self.halo * self.Y * (4 * 16 + 4)
        return torch.zeros(n, dtype=torch.uint8)

    def _cols(self, side, pack):
        h, X = self.halo, self.X
        if pack:
            return slice(h, 2 * h) if side == 0 else slice(X - 2 * h, X - h)
        return slice(0, h) if side == 0 else slice(X - h, X)

    def pack(self, side, buf):
        c = self._cols(side, True)
        parts = [np.ascontiguousarray(self.sim.view(f)[:, c]).view(np.uint8).reshape(-1) for f in HALO_FIELDS]
        buf.copy_(torch.from_numpy(np.concatenate(parts)))

    def unpack(self, side, buf):
        c = self._cols(side, False)
        raw = buf.numpy()
        off = 0
        for f in HALO_FIELDS:
            v = self.sim.view(f)
            n = self.Y * self.halo * v.shape[2] * v.dtype.itemsize
            v[:, c] = raw[off:off + n].view(v.dtype).reshape(self.Y, self.halo, v.shape[2])
            off += n

    def step(self, n):
        self.sim.step(n)

    def sync(self):
        pass


def _worker(rank, world, port, X, Y, halo, n_iter, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wx_oracle
    import wxpkg
    pkg = wxpkg.load_package()
    from weather_sandbox_amd import slab
    base, water, wall, u = _problem(pkg, X, Y)
    x0, xo = slab.slab_columns(X, rank, world)
    idx = (x0 - halo + np.arange(xo + 2 * halo)) % X
    eng = OracleSlabEngine(wx_oracle, X, Y, x0, xo, halo)
    eng.upload(np.ascontiguousarray(base[:, idx]), np.ascontiguousarray(water[:, idx]), np.ascontiguousarray(wall[:, idx]))
    eng.set_params(u)
    drv = slab.SlabSim(eng, rank, world, halo)
    assert drv.iters_per_exchange == halo // 6
    drv.step(n_iter)
    drv.step(3)  # a second call that does not line up with the exchange period
    owned = {f: eng.sim.field(f)[:, halo:halo + xo] for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_0", "LIGHT_1", "WATER_0")}
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **owned)
    dist.barrier()
    dist.destroy_process_group()


def _problem(pkg, X, Y):
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    rng = np.random.default_rng(11)
    air = wall[..., 1] != 0
    base[..., 0] += np.where(air, rng.normal(0, 0.2, (Y, X)), 0).astype(np.float32)  # |v| up to ~0.8: widest cone
    base[..., 1] += np.where(air, rng.normal(0, 0.1, (Y, X)), 0).astype(np.float32)
    water[..., 0] *= np.where(air, 1.0 + 0.4 * rng.random((Y, X)), 1.0).astype(np.float32)
    gui = pkg.params.merge_settings(None)
    gui["sunAngle"] = 35.0
    u = pkg.params.uniforms_from_gui(gui, Y, quad_scale=1)  # x-dependent fragCoord: exercises x_off / X_global
    u["enablePrecipitation"] = 0
    return base, water, wall, u


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world,halo", [(2, 12), (3, 6), (2, 7)])
def test_slabs_equal_whole_domain(pkg, oracle, tmp_path, world, halo):
    X, Y, n_iter = 96, 48, 8
    mp.spawn(_worker, args=(world, _free_port(), X, Y, halo, n_iter, str(tmp_path)), nprocs=world, join=True)
    base, water, wall, u = _problem(pkg, X, Y)
    ref = oracle.OracleSim(X, Y, 0)
    ref.upload(base, water, wall)
    ref.set_params(u)
    ref.step(n_iter + 3)
    xo = X // world
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        for f in got.files:
            assert np.array_equal(got[f], ref.field(f)[:, r * xo:(r + 1) * xo]), f"rank {r} field {f}"


def test_slab_geometry(pkg):
    from weather_sandbox_amd import slab
    assert slab.slab_columns(16384, 3, 8) == (6144, 2048)
    with pytest.raises(ValueError):
        slab.slab_columns(100, 0, 3)
    with pytest.raises(ValueError):
        slab.SlabSim(object(), 0, 2, 4)


def _rec(px, active, tag):
    return np.array([px, 0.1 * tag, 0.5 if active else -2.5 - tag, 0.0 if active else 0.25, 1.0], np.float32)


def _particle_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wxpkg
    wxpkg.load_package()
    from weather_sandbox_amd import slab
    X, halo, n = 256 * world, 64, 8
    eng = ModelPoolEngine(rank, world, n, X, halo)
    drv = slab.SlabSim(eng, rank, world, halo)
    assert drv.particles and drv.iters_per_exchange == 1 + (64 - 12) // 9 == 6
    px = lambda col: np.float32((col + 0.5) / X * 2 - 1)
    xo, last = X // world, world - 1
    P = eng.pool
    # --- the state every rank holds at the START of the period, then what "happened" during it, rank by rank (scripted) ---
    # 0: active deep inside rank 0, nothing happens: only rank 0 tracks it
    P[0] = _rec(px(100), True, 0)
    eng.remote[0] = rank != 0
    # 1: active near rank 0's right edge, drifted into rank 1's owned columns during the period; both processed it to the end (rank 1
    #    as ghost copy first, rank 0 as ghost copy last): ownership passes to rank 1, rank 0 keeps a ghost copy
    P[1] = _rec(px(xo + 2), True, 1)
    eng.remote[1] = rank not in (0, 1)
    # 2: inactive everywhere; rank 0 spawns it in iteration 2 (owned), the LAST rank spawns a phantom from its stale record in iteration 5
    P[2] = _rec(px(10), False, 2)
    if rank == 0:
        P[2] = _rec(px(100), True, 2)
        eng.flips[2], eng.meta[2] = 1 << 2, 0x80 | 9
    elif rank == last and world > 2:
        P[2] = _rec(px(last * xo + 120), True, 22)
        eng.flips[2], eng.meta[2] = 1 << 5, 0x80 | 9
    # 3: active in rank 1's owned columns, deposits in iteration 4: everybody must get the new inactive record
    P[3] = _rec(px(xo + 100), True, 3)
    eng.remote[3] = rank != 1
    if rank == 1:
        P[3] = _rec(px(xo + 100), False, 33)
        eng.flips[3], eng.meta[3] = 1 << 4, 0x80 | 9
    # 4: active in rank 0's owned columns next to rank 1: evaporates in iteration 3 (both see it), re-spawns in iteration 6 in rank 1's
    #    owned columns far from the edge (only rank 1 sees that): rank 1's longer history wins
    P[4] = _rec(px(xo - 5), True, 4)
    eng.remote[4] = rank not in (0, 1)
    if rank == 0:
        P[4] = _rec(px(xo - 5), False, 44)
        eng.flips[4], eng.meta[4] = 1 << 3, 0x80 | 9
    elif rank == 1:
        P[4] = _rec(px(xo + 130), True, 45)
        eng.flips[4], eng.meta[4] = (1 << 3) | (1 << 6), 0x80 | 9
    # 5: inactive, nothing happens
    P[5] = _rec(px(7), False, 5)
    # 6: active on rank 1 within `halo` columns of rank 0: rank 0 must keep / get a ghost copy with rank 1's current record
    P[6] = _rec(px(xo + 20), True, 6) if rank == 1 else _rec(px(xo + 12), True, 6)
    eng.remote[6] = rank not in (0, 1)
    # 7: spawned by rank 1 inside the overlap with rank 0 in iteration 1 (both process it; only rank 1 has it in its owned columns)
    P[7] = _rec(px(3), False, 7)
    if rank in (0, 1):
        P[7] = _rec(px(xo + 30), True, 7)
        eng.flips[7] = 1 << 1
        eng.meta[7] = (0x80 | 9) if rank == 1 else 9
    eng.strike = np.array([0.1 * rank, 0.2, 40.0 + rank, 1.5], np.float32) if rank > 0 else np.zeros(4, np.float32)
    drv.step(drv.iters_per_exchange)  # one full period -> exchange()
    np.savez(os.path.join(out_dir, f"p{rank}.npz"), pool=eng.pool, remote=eng.remote, strike=eng.strike, periods=eng.periods, refreshed=eng.refreshed)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_pool_exchange(tmp_path, world):
    """slab.SlabSim.exchange() with particles over gloo, on a scripted period: after the exchange every active droplet is owned by
    the rank whose columns contain it, neighbours hold ghost copies of the ones near the common edge, everybody else has it marked
    remote; status flips reach every rank; a phantom spawn from a stale record loses against the earlier real one; the longer flip
    history wins; the latest lightning strike reaches everybody."""
    mp.spawn(_particle_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [np.load(os.path.join(str(tmp_path), f"p{r}.npz")) for r in range(world)]
    X = 256 * world
    xo = X // world
    px = lambda col: np.float32((col + 0.5) / X * 2 - 1)
    for r in range(world):
        pool, remote = res[r]["pool"], res[r]["remote"]
        # 0: only rank 0
        assert remote[0] == (r != 0)
        # 1: owner rank 1 with ITS record; rank 0 keeps a ghost copy of it (2 columns from the edge); others remote
        assert remote[1] == (r not in (0, 1))
        if r in (0, 1):
            assert np.array_equal(pool[1], _rec(px(xo + 2), True, 1))
        # 2: rank 0's spawn wins everywhere; the phantom is gone; far ranks have it remote, rank 0 tracks it
        assert remote[2] == (r != 0)
        if r == 0:
            assert np.array_equal(pool[2], _rec(px(100), True, 2))
        # 3: inactive with rank 1's record on every rank
        assert not remote[3] and np.array_equal(pool[3], _rec(px(xo + 100), False, 33))
        # 4: rank 1's longer history: active at column xo + 130 (outside the halo of rank 0: remote there)
        assert remote[4] == (r != 1)
        if r == 1:
            assert np.array_equal(pool[4], _rec(px(xo + 130), True, 45))
        # 5: untouched inactive record
        assert not remote[5] and np.array_equal(pool[5], _rec(px(7), False, 5))
        # 6: rank 1's record, ghost copy on rank 0
        assert remote[6] == (r not in (0, 1))
        if r in (0, 1):
            assert np.array_equal(pool[6], _rec(px(xo + 20), True, 6))
        # 7: owner rank 1, ghost on rank 0, everybody else learned that it is active elsewhere
        assert remote[7] == (r not in (0, 1))
        assert np.allclose(res[r]["strike"], [0.1 * (world - 1), 0.2, 40.0 + world - 1, 1.5])
        assert int(res[r]["periods"]) == 1 and list(res[r]["refreshed"]) == [False]
