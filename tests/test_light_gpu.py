"""Lighting parity around the compass: every class of the sun ray's bilinear tap (tests/light_scenes.py: the eight (dx0, fv) classes,
the exact slider positions GUI 0, 90 and 180 among the specimens) at every strip, segment, band, wrap, slab and member seam of the
kernels that serve the tap -- the marching wet kernel's LDS ring, k_wet_fix, k_lighting, both k_emitted instantiations, slab handles
over their ghost columns, ensemble members with a sun each -- bit for bit against the CPU oracle. A case fills the scene with light
under a day sun, switches the uniform and runs light_scenes.N_UNDER iterations; LIGHT_0, LIGHT_1, BASE_CUR, WATER_CUR, WALL_CUR,
BASE_DISP, WATER_0 are compared exactly and EMITTED against the oracle's values rounded once to binary16, after the first and after the
last of them. tests/test_light_cpu.py shows that a wrong column or row at a claimed seam could not agree by accident."""
import importlib

import numpy as np
import pytest

import light_scenes as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(pkg):
    pkg.engine.build()
    return pkg.engine


def _params(pkg, u):
    return pkg.params.fill_struct(pkg.params.WxParams(), u)


@pytest.fixture(scope="module")
def filled(pkg, E, oracle):
    """grid name -> a handle holding the grid's scene after the fill (default options), checked against the oracle's; every case
    branches from it with wx_copy_state. One fill per grid and module."""
    cache = {}

    def get(grid):
        if grid not in cache:
            X, Y = L.GRIDS[grid]
            scene, st = L.oracle_fill(grid)
            u = L.scene_uniforms(Y)
            h = E.Handle(X, Y, 0)
            h.upload(*scene)
            h.set_params(_params(pkg, u), u["initial_T"])
            h.iter = 0
            h.step(L.fill_iterations(Y))
            for f in L.COMPARED:
                a = h.read_rect(f)
                assert np.array_equal(a, st[f]), "after the fill: " + L.describe_difference(f, a, st[f], X, Y, "gui40")
            cache[grid] = h
        return cache[grid]
    yield get
    for h in cache.values():
        h.close()


def _compare(read, want, X, Y, sp, tag, borders=(), emitted=True):
    for f in L.COMPARED:
        a = read(f)
        assert np.array_equal(a, want[f]), f"{tag}: " + L.describe_difference(f, a, want[f], X, Y, sp, borders)
    if emitted:
        a, b = read("EMITTED"), want["EMITTED"].astype(np.float16)
        assert a.dtype == np.float16 and np.array_equal(a, b), f"{tag}: " + L.describe_difference("EMITTED", a, b, X, Y, sp, borders)


def _emitted_rectangles(h, want, X, Y, sp, tag):
    """Rectangle reads of the emitted light: from one strip border to another, and the last column alone."""
    e = want["EMITTED"].astype(np.float16)
    w = L.WET_STRIP
    for x0, y0, ww, hh in ((w, 0, min(w, X - w), Y), (0, 2, min(2 * w, X), Y - 3), (X - 1, 0, 1, Y), (w, Y - 2, min(w, X - w), 2)):
        if ww < 1 or x0 >= X:
            continue
        a = h.read_rect("EMITTED", x0, y0, ww, hh)
        assert np.array_equal(a, e[y0:y0 + hh, x0:x0 + ww]), f"{tag}: EMITTED rectangle {(x0, y0, ww, hh)} under {sp}"
    assert np.array_equal(h.read_rect("EMITTED"), e), f"{tag}: EMITTED whole after the rectangles under {sp}"


def _branch(pkg, E, src, grid, config, sp):
    """A handle under the configuration's options in the filled state, the specimen's uniforms set (and the fast cells planted)."""
    cfg = L.CONFIGS[config]
    X, Y = L.GRIDS[grid]
    wrap, quad, fast = L.variant_of(config)
    h = E.Handle(X, Y, 0)
    try:
        h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
        h.set_option(h.OPT_ROW_BANDS, cfg.get("bands", 1))
        h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
        h.copy_from(src)
        if fast:
            D = importlib.import_module(pkg.__name__ + ".devtools")
            h.sync()
            t = D.field_tensor(h, "BASE_CUR")
            for k, (x, y) in enumerate(L.fast_cell_sites(X, Y, L.oracle_fill(grid)[1]["WALL_CUR"])):
                t[y, x, 0] = 1.3 if k % 2 == 0 else -1.3
            D.torch.cuda.synchronize()
        u = L.scene_uniforms(Y, L.SPECIMENS[sp][0], wrap, quad)
        h.set_params(_params(pkg, u), u["initial_T"])
    except Exception:
        h.close()
        raise
    return h


def _run_case(pkg, E, src, grid, config, sp, borders=()):
    cfg = L.CONFIGS[config]
    X, Y = L.GRIDS[grid]
    ref = L.oracle_run(grid, L.variant_of(config), sp)
    h = _branch(pkg, E, src, grid, config, sp)
    tag = f"{grid} {config}"
    try:
        done = 0
        for n in cfg["steps"]:
            if cfg.get("pieces"):  # the first iteration under the specimen is a piece that skips the display stores
                h.step(1, 4)
                h.step(n - 1)
            else:
                h.step(n)
            done += n
            if done == 1 and cfg.get("compare_first", True):
                _compare(h.read_rect, ref["first"], X, Y, sp, tag + " first iteration", borders)
                if cfg.get("fast"):  # k_wet_fix's own accessor lit these cells and their upper neighbours: the exact path ran
                    assert h.fastest_velocity() == L.fast_expected(grid, sp) >= 0.9, (tag, sp, h.fastest_velocity(), L.fast_expected(grid, sp))
        assert done == L.N_UNDER
        _compare(h.read_rect, ref["last"], X, Y, sp, tag + " last iteration", borders)
        if config in ("wet", "perpass"):  # k_emitted<planar> / k_emitted<interleaved>
            _emitted_rectangles(h, ref["last"], X, Y, sp, tag)
    finally:
        h.close()


PLAN = [(grid, config) for grid, configs, _ in L.PLAN for config in configs]


@pytest.mark.parametrize("grid,config", PLAN)
def test_every_tap_class_vs_oracle(pkg, E, oracle, filled, grid, config):
    """One grid under one configuration, every specimen of its plan. A mismatch names the cell, its output lane and strip, its row's
    distance from the nearest border and the specimen's class."""
    specimens = [s for g, cs, sps in L.PLAN if g == grid and config in cs for s in sps]
    assert specimens
    Y = L.GRIDS[grid][1]
    borders = [k * Y // 8 for k in range(1, 8)] if grid == "bands" else ()
    for sp in specimens:
        _run_case(pkg, E, filled(grid), grid, config, sp, borders)


def test_members_with_a_sun_each(pkg, E, oracle, filled):
    """One ensemble whose eight members carry one specimen of each (dx0, fv) class IN ONE LAUNCH; then once more with the specimens
    rotated by one member (per-member set_params): every member against the oracle run of its specimen."""
    grid = "169x52"
    X, Y = L.GRIDS[grid]
    src = filled(grid)
    ens = E.Ensemble(len(L.ONE_PER_CLASS), X, Y)
    try:
        for rot in (0, 1):
            mine = [L.ONE_PER_CLASS[(i + rot) % len(L.ONE_PER_CLASS)] for i in range(len(L.ONE_PER_CLASS))]
            for h, sp in zip(ens.members, mine):
                h.copy_from(src)
                u = L.scene_uniforms(Y, L.SPECIMENS[sp][0])
                h.set_params(_params(pkg, u), u["initial_T"])
            for n, which in ((1, "first"), (L.N_UNDER - 1, "last")):
                ens.step(n)
                for i, (h, sp) in enumerate(zip(ens.members, mine)):
                    _compare(h.read_rect, L.oracle_run(grid, (1, 0, False), sp)[which], X, Y, sp, f"member {i} rotation {rot} {which} iteration")
    finally:
        ens.close()


def _slab_specimens():
    return [s for s, (_, (dx0, _), _) in L.SPECIMENS.items() if dx0 >= 0]


@pytest.mark.parametrize("nslab,halo", [(2, 12), (4, 6)])
def test_slab_handles_every_class_that_reads_to_the_right(pkg, E, oracle, filled, nslab, halo):
    """Slab handles on one GPU with the ring exchange of test_slab_handles_equal_whole_domain: the specimens with dx0 >= 0 take their
    light from the RIGHT ghost columns (dx0 = -1, all the other suites run, needs the left ones only). Slabs cannot be copied into, so
    each specimen fills its own. Against the undecomposed handle AND the oracle; EMITTED is read after the exchange."""
    import torch
    grid = "slabs"
    X, Y = L.GRIDS[grid]
    scene, _ = L.oracle_fill(grid)
    xo, per = X // nslab, halo // 6
    uf = L.scene_uniforms(Y)

    def ring(slabs, bufs, n):
        done = 0
        while done < n:
            k = min(per, n - done)
            for h in slabs:
                h.step(k)
            done += k
            for r, h in enumerate(slabs):
                h.halo_pack(0, bufs[r][0].data_ptr())
                h.halo_pack(1, bufs[r][1].data_ptr())
            for h in slabs:
                h.sync()
            for r, h in enumerate(slabs):
                h.halo_unpack(0, bufs[(r - 1) % nslab][1].data_ptr())
                h.halo_unpack(1, bufs[(r + 1) % nslab][0].data_ptr())
            for h in slabs:
                h.sync()

    for sp in _slab_specimens():
        ref = L.oracle_run(grid, (1, 0, False), sp)
        whole = _branch(pkg, E, filled(grid), grid, "wet", sp)
        slabs, bufs = [], []
        try:
            for r in range(nslab):
                h = E.Handle(xo, Y, 0, X_global=X, x0=r * xo, halo=halo)
                slabs.append(h)
                idx = (r * xo - halo + np.arange(xo + 2 * halo)) % X
                h.upload(*[np.ascontiguousarray(a[:, idx]) for a in scene])
                h.set_params(_params(pkg, uf), uf["initial_T"])
                bufs.append([torch.empty(h.halo_bytes(), dtype=torch.uint8, device="cuda") for _ in range(2)])
            ring(slabs, bufs, L.fill_iterations(Y))
            us = L.scene_uniforms(Y, L.SPECIMENS[sp][0])
            for h in slabs:
                h.set_params(_params(pkg, us), us["initial_T"])

            def read(f):
                return np.concatenate([h.read_rect(f, halo, 0, xo, Y) for h in slabs], axis=1)
            for n, which in ((1, "first"), (L.N_UNDER - 1, "last")):
                ring(slabs, bufs, n)
                whole.step(n)
                tag = f"{nslab} slabs halo {halo} {which} iteration (slab cuts at columns {[k * xo for k in range(nslab)]})"
                _compare(read, ref[which], X, Y, sp, tag + " vs the oracle")
                _compare(read, {f: whole.read_rect(f) for f in L.COMPARED}, X, Y, sp, tag + " vs the whole domain", emitted=False)
                assert np.array_equal(read("EMITTED"), whole.read_rect("EMITTED")), (tag, sp)
        finally:
            whole.close()
            for h in slabs:
                h.close()


@pytest.mark.parametrize("nslab,halo", [(2, 12), (4, 6)])
def test_slab_group_with_the_suns_that_read_to_the_right(pkg, E, oracle, nslab, halo):
    """The library's own slab group (local transport, its own exchange periods) under GUI 140 and GUI 180."""
    grid = "slabs"
    X, Y = L.GRIDS[grid]
    scene, _ = L.oracle_fill(grid)
    uf = L.scene_uniforms(Y)
    for sp in ("gui140", "gui180"):
        ref = L.oracle_run(grid, (1, 0, False), sp)
        g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
        try:
            g.upload(*scene)
            g.set_params(_params(pkg, uf), uf["initial_T"])
            g.step(L.fill_iterations(Y))
            us = L.scene_uniforms(Y, L.SPECIMENS[sp][0])
            g.set_params(_params(pkg, us), us["initial_T"])
            for n, which in ((1, "first"), (L.N_UNDER - 1, "last")):
                g.step(n)
                _compare(g.read, ref[which], X, Y, sp, f"group of {nslab} halo {halo} {which} iteration", emitted=False)
        finally:
            g.close()


def test_sweep_across_the_day(pkg, E, oracle, filled):
    """The day/night driver's pattern with the exact positions included: the angle changes before EVERY iteration, GUI -10 .. 188 and
    back, one set_params each; the oracle is driven alike. Compared after every iteration."""
    grid = "169x52"
    X, Y = L.GRIDS[grid]
    _, st = L.oracle_fill(grid)
    o = L.oracle_from(st, X, Y, L.fill_iterations(Y))
    h = E.Handle(X, Y, 0)
    try:
        h.copy_from(filled(grid))
        for k, deg in enumerate(L.DAY_SWEEP + L.DAY_SWEEP[-2::-1]):
            u = L.scene_uniforms(Y, L.bits_of_gui(deg))
            h.set_params(_params(pkg, u), u["initial_T"])
            o.set_params(u)
            h.step(1)
            o.step(1)
            want = {f: o.field(f) for f in L.COMPARED + ("EMITTED",)}
            for f in L.COMPARED:
                a = h.read_rect(f)
                assert np.array_equal(a, want[f]), f"sweep step {k} (GUI {deg}): {f}: {int((a != want[f]).sum())} values differ"
            assert np.array_equal(h.read_rect("EMITTED"), want["EMITTED"].astype(np.float16)), f"sweep step {k} (GUI {deg}): EMITTED"
    finally:
        h.close()
        o.close()
