"""The wall-editing tools and the airplane crash on the device: the case list of tests/tool_scenes.py -- every wall tool with both
signs over every surface type, the disc's rim on the strip seams, the wrap seam and the edge columns, held for one or three
iterations -- against the CPU oracle, bit for bit on every grid field after the held iterations and again 20 iterations after release:
what an edited wall texture does afterwards is carried by the handle's brush-free launch decisions (the QUIET instantiation of the
marching wet kernel, the wall-dependent shortcuts, the dry pairs, the re-measured air rows). Besides the marching wet kernel in its
display / plain / WX_OVERLAP_MORE_TO_COME iterations, stored and on-demand waterTexture_0 and the per-pass kernels: ROW_BANDS 0 / 1 / 2
on 2500 x 300, the dry pass mask, slab groups, ensembles, and edits held across a smoothing iteration.
tests/test_tools_cpu.py accounts for what the case list reaches."""
import json
import os
import sys

import numpy as np
import pytest

import tool_scenes as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CASES = T.cases()
FIELDS = ("BASE_CUR", "BASE_DISP", "WATER_CUR", "WATER_0", "WALL_CUR", "LIGHT_0", "LIGHT_1")
PAIR_KERNEL = "march_dry2_two_iterations_per_launch"


@pytest.fixture(scope="module")
def fuzz(pkg):
    import fuzz_parity
    pkg.engine.build()
    return fuzz_parity


def _params(pkg, u):
    return pkg.params.fill_struct(pkg.params.WxParams(), u)


@pytest.mark.parametrize("tool", T.WALL_TOOLS)
@pytest.mark.parametrize("sign", T.SIGNS)
def test_wall_tools_vs_oracle(pkg, oracle, fuzz, tool, sign):
    """Every placement and both hold lengths of one (tool, sign). A mismatch stops at its first case and prints the recipe
    (tool_scenes.run_case runs it alone)."""
    mine = [c for c in CASES if c["tool"] == tool and c["sign"] == sign]
    assert len(mine) == len(T.placements(T.GRID[0])) * len(T.HELD)
    edited = 0
    for c in mine:
        bad, walls = T.run_case(pkg, fuzz, oracle, c)  # (a mismatch ends the run: one wall texture then, not two)
        assert not bad, json.dumps({"recipe": c, "mismatches": bad})
        edited += int((walls[0] != T.build_case(c)[2]).any(-1).sum())
    assert edited > 0 or tool in (20, 21)  # (the two tools that write no wall byte)
    print(json.dumps({"tool": tool, "sign": sign, "cases": len(mine), "wall_cells_differing_from_the_upload": edited}))


@pytest.mark.parametrize("bands", [0, 1, 2])
def test_wall_tools_under_row_bands(pkg, oracle, fuzz, bands):
    """ROW_BANDS 0 / 1 / 2 on 2500 x 300 (ragged last strip of 36 columns): every (tool, sign) under one of the three modes, the disc's
    right rim on the first column of the ragged strip, its left rim on the wrap seam in turn."""
    X, Y = T.BANDS_GRID
    k = 0
    for ti, tool in enumerate(T.WALL_TOOLS):
        for si, sign in enumerate(T.SIGNS):
            if (ti + si) % 3 != bands:
                continue
            c = {"X": X, "Y": Y, "tool": tool, "sign": sign, "placement": ("right@ragged_wet", "left@wrap")[k % 2], "held": (3, 1)[k % 2], "variant": "stepped",
                 "config": "wet", "bands": bands}
            k += 1
            bad, _ = T.run_case(pkg, fuzz, oracle, c)
            assert not bad, json.dumps({"recipe": c, "mismatches": bad})
    assert k >= 6


def test_wall_tools_under_the_dry_pass_mask(pkg, oracle):
    """WX_PASS_DRY on the water-free background: while a wall tool is held the wall texture can change in every iteration, so no
    two-iterations-per-launch kernel may run (profile counter: none), whatever the tool leaves water-free; after release the handle
    takes its brush-free dry steps. Equal to the oracle after the held iterations and 20 iterations on, whichever kernel ran."""
    X, Y = T.GRID
    pairs_after = {}
    for ti, tool in enumerate(T.WALL_TOOLS):
        for sign in T.SIGNS:
            c = {"X": X, "Y": Y, "tool": tool, "sign": sign, "placement": ("right@dry_seam", "right@ragged_dry", "left@wrap")[ti % 3], "held": (3, 1, 2)[ti % 3],
                 "variant": T.VARIANTS[ti % 2]}
            base, water, wall, _ = T.build_case(c, dry=True)
            held_u, free_u = T.tool_uniforms(c, dry=True)
            h, o = pkg.engine.Handle(X, Y, 0), oracle.OracleSim(X, Y, 0)
            try:
                h.upload(base, water, wall)
                o.upload(base, water, wall)
                h.iter = o.iter = T.ITER0
                h.set_option(h.OPT_DRY_KERNEL, 1)
                h.set_option(h.OPT_DRY_PAIRS, 1)
                h.profile(True)
                for u, n in ((held_u, c["held"]), (free_u, T.AFTER)):
                    h.set_params(_params(pkg, u), u["initial_T"])
                    o.set_params(u)
                    h.step(n)
                    o.step(n)
                    launched = h.profile_read().get(PAIR_KERNEL, (0.0, 0))[1]
                    if u is held_u:
                        assert launched == 0, (c, launched)
                    for f in ("BASE_CUR", "BASE_DISP", "WATER_CUR", "WATER_0", "WALL_CUR"):
                        assert np.array_equal(h.read_rect(f), o.field(f)), (c, f, "held" if u is held_u else "release")
                pairs_after[(tool, sign)] = launched
            finally:
                h.close()
                o.close()
    print(json.dumps({"pair_launches_after_release": {f"{t}{'+' if s > 0 else '-'}": n for (t, s), n in pairs_after.items()}}))


SLAB_TOOLS = ((10, -1), (11, +1), (12, +1), (13, +1), (16, +1), (14, -1), (20, +1), (21, -1), (22, +1), (22, -1))


@pytest.mark.parametrize("overlap", [0, 1], ids=["in_order", "overlapped"])
@pytest.mark.parametrize("nslab", [2, 4, 8])
def test_wall_tools_on_slabs_equal_the_whole_domain(pkg, nslab, overlap):
    """A slab group on one GPU (halo 12) against the undecomposed handle: the disc straddles the last owned / first ghost column of a
    slab, lies wholly inside a ghost region (half width 5), or mid-slab; held for 3 iterations, released, 20 more in steps that put the
    release inside an exchange period. The ten (tool, sign) pairs of SLAB_TOOLS go round the three positions."""
    E = pkg.engine
    X, Y, halo = 1008, 77, 12
    xo = X // nslab
    k = nslab + 3 * overlap
    for pos, (left, hw) in enumerate(((xo - 15, 15.0), (xo + 1, 5.0), (xo // 2 - 15, 15.0), (X - 15, 15.0))):
        for j in range(3 if pos < 3 else 1):
            tool, sign = SLAB_TOOLS[(k + 4 * pos + j) % len(SLAB_TOOLS)]
            c = {"X": X, "Y": Y, "tool": tool, "sign": sign, "left": left, "hw": hw, "held": 3, "variant": "stepped"}
            base, water, wall, _ = T.build_case(c)
            held_u, free_u = T.tool_uniforms(c)
            g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
            whole = E.Handle(X, Y, 0)
            try:
                g.set_option(E.Handle.OPT_EXCHANGE_OVERLAP, overlap)
                g.upload(base, water, wall)
                whole.upload(base, water, wall)
                for hh in g.slabs + [whole]:
                    hh.iter = T.ITER0
                for u, steps in ((held_u, (3,)), (free_u, (1, 6, 13))):
                    g.set_params(_params(pkg, u), u["initial_T"])
                    whole.set_params(_params(pkg, u), u["initial_T"])
                    for n in steps:
                        g.step(n)
                        whole.step(n)
                        for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_1", "WATER_0"):
                            a, b = g.read(f), whole.read_rect(f)
                            assert np.array_equal(a, b), (c, f, int((a != b).any(-1).sum()), [int(v) for v in np.argwhere((a != b).any(-1))[0]])
            finally:
                g.close()
                whole.close()


def test_wall_tools_and_a_crash_on_members_of_an_ensemble(pkg, oracle):
    """Five members of 169 x 52 in one ensemble: two hold different wall tools (released after 3 and after 6 iterations), a third has
    an airplane crash in its first iteration, two are quiet. Every member equals its lone handle after every step, member 0 equals the
    oracle, and wx_ensemble_stats accounts for every member-iteration."""
    import test_ensemble_gpu as EN
    X, Y = T.GRID
    scenes = [T.background(X, Y, v, seed=s) for v, s in (("stepped", 1), ("flat", 2), ("stepped", 3), ("flat", 4), ("stepped", 5))]
    c0 = {"X": X, "Y": Y, "tool": 11, "sign": +1, "placement": "left@wet_seam", "held": 3}
    c1 = {"X": X, "Y": Y, "tool": 10, "sign": -1, "placement": "right@wrap", "held": 6}
    quiet = T.scene_uniforms(Y)
    x, y = 4, int(scenes[2][3][4]) - 1  # a surface land cell of member 2 with vegetation 126 (column 6 carries vegetation 0: lit, it burns down at once)
    us = [T.tool_uniforms(c0)[0], T.tool_uniforms(c1)[0], dict(quiet, airplaneValues=T.crash_values(X, Y, x, y)), quiet, dict(quiet)]
    t = EN.Twins(pkg, [dict(base=s[0], water=s[1], wall=s[2], u=u, iter0=997) for s, u in zip(scenes, us)])
    o = oracle.OracleSim(X, Y, 0)
    try:
        o.upload(*scenes[0][:3])
        o.iter = 997
        o.set_params(us[0])
        total = 0
        for k, n in enumerate((1, 2, 3, 20)):
            t.step(n)
            o.step(n)
            total += n
            t.compare(("step", k), fields=EN.FIELDS[:8])
            for f in FIELDS:
                assert np.array_equal(t.ens[0].read_rect(f), o.field(f)), (k, f)
            if k == 0:
                t.push(2, airplaneValues=T.NO_PLANE)
                w = t.ens[2].read_rect("WALL_CUR")
                assert w[y, x, 0] == T.FIRE and w[y - 1, x, 0] == T.LAND  # the crash lit the surface cell, not the buried one
            if k == 1:
                t.push(0, userInputType=-1)
                o.set_params(dict(us[0], userInputType=-1))
            if k == 2:
                t.push(1, userInputType=-1)
        st = t.ens.stats()
        assert st["member_iters_batched"] + st["member_iters_solo"] == 5 * total and st["march_launches"] >= total, st
        assert scenes[2][2][y, x, 3] == 126 and scenes[2][2][y, x, 0] == T.LAND
        assert t.ens[2].read_rect("WALL_CUR")[y, x, 0] == T.FIRE  # still burning, across iteration 1000
    finally:
        t.close()
        o.close()


@pytest.mark.parametrize("config", ["wet", "wet_stored", "wet_pieces", "perpass"])
def test_edits_held_across_a_smoothing_iteration(pkg, oracle, fuzz, config):
    """A tool held over iterations 99, 100, 101 -- the marching kernel's lane exchange of soil moisture and snow (`smooth_iter`) meets a
    surface row edited in the same call -- and a crash at 999, so that iteration 1000 smooths, and spreads, what it lit."""
    X, Y = T.GRID
    for tool, sign, placement in ((20, +1, "left@wet_seam"), (21, +1, "right@wrap"), (21, -1, "left@col0|1"), (13, +1, "right@dry_seam"), (11, +1, "right@ragged_wet"), (10, -1, "left@wrap")):
        c = {"X": X, "Y": Y, "tool": tool, "sign": sign, "placement": placement, "held": 3, "variant": "stepped", "config": config}
        bad, _ = T.run_case(pkg, fuzz, oracle, c, iter0=99)
        assert not bad, json.dumps({"recipe": c, "mismatches": bad})
    cfg = fuzz.IMPULSE_CONFIGS[config]
    base, water, wall, hgt = T.background(X, Y, "stepped")
    for x in (6, 55, 56, 168):  # land; the last column of a strip and the first of the next; the last column
        y = int(hgt[x]) - 1
        u = dict(T.scene_uniforms(Y), airplaneValues=T.crash_values(X, Y, x, y))
        h, o = pkg.engine.Handle(X, Y, 0), oracle.OracleSim(X, Y, 0)
        try:
            h.upload(base, water, wall)
            o.upload(base, water, wall)
            h.iter = o.iter = 999
            h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
            h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
            for uu, n in ((u, 1), (dict(u, airplaneValues=T.NO_PLANE), 1), (dict(u, airplaneValues=T.NO_PLANE), 19)):
                h.set_params(_params(pkg, uu), uu["initial_T"])
                o.set_params(uu)
                h.step(n)
                o.step(n)
                for f in FIELDS:
                    assert np.array_equal(h.read_rect(f), o.field(f)), (config, x, f, n)
        finally:
            h.close()
            o.close()
