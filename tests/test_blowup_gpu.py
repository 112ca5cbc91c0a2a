"""Blow-up parity: non-finite and overflowing state (tests/blowup_scenes.py) stepped through the kernels, through the C ABI only, against
the CPU oracle under the contract of DESIGN.md section 3: (a) every float bit-identical where the oracle's is finite and non-finite
where the oracle's is (the same infinity; NaN payloads are not compared), (b) integer outputs equal. What runs what:
  * every kind, full contract: marching wet (display / plain / MORE_TO_COME piece, stored / on-demand waterTexture_0), per-pass, row
    bands 0 / 1 / 2 (three kinds), and the tiled dry kernel on a state that carries water (dry pass mask, k_fused_dry<true>);
  * the finite huge_* family, full contract while the state is finite: one-iteration dry kernel, dry pairs in both instantiations,
    per-pass dry;
  * the NaN kinds through the water-free kernels (one-iteration, pairs in both instantiations, tiled): compared WHEREVER THE ORACLE IS
    FINITE -- the reference makes NaN water of NaN weights, which those kernels cannot hold, so what they keep where the oracle has
    NaN is not compared -- plus: the exact paths ran (wx_pair_stats, the profile counters say which kernel);
  * slab groups (wet, and the dry mask with pairs on / off): a NaN vx anywhere in a slab is REPORTED. No slab run is compared with one
    handle on a blown-up state: every kind here is a violation of the slabs' velocity bound by design.
Reported, (d): the census of wx_diagnostics equals numpy on the read-back of stepped states (per-pass and marching), wx_fastest_velocity
is +Inf once a NaN or Inf velocity went through the wet exact path, an overflowing exact-path list stays the reported WX_E_STATE.
Nothing here is meant to crash: every access a non-finite index can reach is a bounds-checked stage or a wrapped global read."""
import json
import os
import sys

import numpy as np
import pytest

import blowup_scenes as B
import impulse_scenes as I

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CASES = B.cases()
# configurations besides tools/fuzz_parity.IMPULSE_CONFIGS: the tiled dry kernel (wx_dry.h) -- chosen by WX_OPT_DRY_KERNEL 0 on the
# water-free state, and by the state itself when it carries water under the dry pass mask (that instantiation stores the water texture)
EXTRA_CONFIGS = {"dry_fused": {"dry": True, "dry_kernel": 0, "pairs": 0, "kernel": "fused_dry_vel_advect_pressure"},
                 "dry_fused_water": {"dry": True, "water": True, "kernel": "fused_dry_vel_advect_pressure"}}
OVERFLOW = "the exact path holds"  # the one error a blown-up scene may run into: reported, the run ends there


@pytest.fixture(scope="module")
def fuzz(pkg):
    import fuzz_parity
    pkg.engine.build()
    return fuzz_parity


def _census(h, fields):
    """wx_diagnostics on the stepped state against numpy on the read-back (tests/test_diag_cpu.reference): the non-finite census, its
    first locations, the cell counts."""
    from test_diag_cpu import reference
    d, want = h.diagnostics(), reference(fields["BASE_CUR"], fields["WATER_CUR"], fields["WALL_CUR"])
    for k in ("n_nonfinite_base", "n_nonfinite_water", "first_nonfinite_base", "first_nonfinite_water", "n_air", "n_wall", "n_negative_water"):
        assert d[k] == want[k], (k, d[k], want[k])
    return {k: d[k] for k in ("n_nonfinite_base", "n_nonfinite_water")}


def run_config(pkg, fuzz, oracle, scene, X, Y, config, wrap=True, steps=None, background=None, census=False, compare="contract", fix_cap=0, stop_past_nonfinite=None):
    """One scene under one configuration (tools/fuzz_parity.IMPULSE_CONFIGS, EXTRA_CONFIGS) against the oracle after every step. -> info;
    asserts the contract -- ``compare`` "finite": wherever the oracle is finite (blowup_scenes.DRY_NAN_KINDS). A reported overflow of
    the exact-path list ends the comparison (info["reported"]); everything read before it was compared. ``fix_cap``: WX_OPT_FIX_CAP."""
    E = pkg.engine
    cfg = dict(fuzz.IMPULSE_CONFIGS, **EXTRA_CONFIGS)[config]
    dry = bool(cfg.get("dry"))
    base, water, wall, drops, sites = scene
    nd = 0 if drops is None else len(drops)
    u = B.scene_uniforms(Y, dry=dry, wrap=wrap, precipitation=nd > 0)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    h, o = E.Handle(X, Y, nd), oracle.OracleSim(X, Y, nd)
    info = {"config": config, "compared_steps": 0, "nonfinite_compared": 0, "reported": None, "finite_where_oracle_is_not": 0, "nonfinite_steps": 0}
    try:
        def options():
            h.set_option(h.OPT_KERNEL_SET, cfg.get("kernel_set", 1))
            h.set_option(h.OPT_DRY_KERNEL, cfg.get("dry_kernel", 1))
            h.set_option(h.OPT_DRY_PAIRS, cfg.get("pairs", 1))
            h.set_option(h.OPT_ROW_BANDS, cfg.get("bands", 1))
            h.set_option(h.OPT_WATER0_ON_DEMAND, cfg.get("water0_on_demand", 1))
            if nd:
                h.set_option(h.OPT_SPLAT_ORDER, 0)
        if cfg.get("prime"):  # a quiet pair on the background first: the trigger meets the PLAIN instantiation of the pair kernel
            h.upload(*background[:3])
            h.set_params(p, u["initial_T"])
            options()
            h.step(2)
            assert h.pair_stats() == (0, 0)
        h.upload(base, water, wall, drops)
        o.upload(base, water, wall, drops)
        h.set_params(p, u["initial_T"])
        o.set_params(u)
        h.iter = o.iter = 0
        options()
        if fix_cap:
            h.set_option(h.OPT_FIX_CAP, fix_cap)
        if dry:
            assert h.water_free() == (not cfg.get("water")), config  # (which decides between the water-free kernels and the tiled one that stores water)
        if cfg.get("kernel") or (dry and cfg.get("kernel_set", 1) == 1):
            h.profile(True)
        fields = ["BASE_CUR", "BASE_DISP", "WATER_CUR", "WATER_0", "WALL_CUR"] if dry else list(fuzz.GRID_FIELDS)
        done = 0
        for n in (steps or cfg.get("steps", (1, 1, 3))):
            try:
                if cfg.get("pieces") and n > 1:
                    h.step(1, 4)
                    h.step(n - 1)
                else:
                    h.step(n)
                got = {f: h.read_rect(f) for f in fields + (["PRECIP_FB", "PRECIP_DEP", "LIGHTNING"] if nd else [])}
                got_drops = h.read_particles() if nd else None
            except E.WxError as e:
                assert OVERFLOW in str(e), str(e)  # (d): the reported error it is today, nothing else
                info["reported"] = str(e)[:80]
                break
            o.step(n)
            done += n
            if dry and not cfg.get("water") and compare == "contract" and not np.isfinite(o.field("BASE_CUR")).all():
                break  # (the finite family on the water-free kernels: the full contract while the state is finite -- the first step of every case is)
            for f, a in got.items():
                b = o.field(f)
                bad = B.contract_mismatch(a, b)
                if compare == "finite" and a.dtype.kind == "f":
                    info["finite_where_oracle_is_not"] += int((np.isfinite(a) & ~np.isfinite(b)).sum())
                    bad &= np.isfinite(b)
                assert not bad.any(), json.dumps({"config": config, "compare": compare, "after_iterations": done, "what": B.describe(f, np.where(bad, a, b), b, sites, X) if a.ndim == 3 else f})
                if a.dtype.kind == "f" and f in ("BASE_CUR", "WATER_CUR"):
                    info["nonfinite_compared"] += int((~np.isfinite(b)).sum())
            if nd:
                assert not B.contract_mismatch(got_drops, o.field("DROPS")).any(), (config, done)
            info["compared_steps"] += 1
            if stop_past_nonfinite is not None and (info["nonfinite_steps"] or not np.isfinite(o.field("BASE_CUR")).all()):
                info["nonfinite_steps"] += 1
                if info["nonfinite_steps"] > stop_past_nonfinite:
                    break
            if census and info["compared_steps"] == 1:
                info["census"] = _census(h, got)
            if info["compared_steps"] == 1 and not dry and cfg.get("kernel_set", 1) == 1:
                info["fastest"] = h.fastest_velocity()
        if dry and cfg.get("pairs", 1) and cfg.get("kernel_set", 1) == 1 and not cfg.get("water") and info["reported"] is None:
            info["pair_stats"] = h.pair_stats()
        if cfg.get("kernel") or (dry and cfg.get("kernel_set", 1) == 1):
            info["launches"] = {k: v[1] for k, v in h.profile_read().items() if "dry" in k and v[1]}
            if cfg.get("kernel"):
                assert info["launches"].get(cfg["kernel"], 0) > 0, (config, info)  # the kernel the configuration is there for is what ran
    finally:
        h.close()
        o.close()
    return info


@pytest.mark.parametrize("kind", B.KINDS)
def test_blown_up_state_vs_oracle(pkg, oracle, fuzz, kind):
    """Every case of one kind under every configuration of the case. Non-vacuity: the first step of every run was compared (no overflow
    of the list before anything was read), non-finite texels were among the compared ones for every kind that plants or produces them,
    and the finite texels around the sites differ from the quiet background (tests/test_blowup_cpu.py, on the oracle they are compared with)."""
    mine = [c for c in CASES if c["kind"] == kind]
    assert mine
    seen = []
    for c in mine:
        scene = B.build_case(c)
        background = I.impulse_scene(c["X"], c["Y"], "smoke", offset=c["offset"], background=c["background"], plant=False)
        for k, config in enumerate(c["configs"]):
            info = run_config(pkg, fuzz, oracle, scene, c["X"], c["Y"], config, wrap=c["wrap"], background=background, census=(k == 0 or config == "wet"), compare=c["compare"])
            assert info["compared_steps"] >= 1, (B.case_id(c), info)
            healed = kind in ("nan_water0", "nan_water2", "nan_water3")
            if kind in B.NONFINITE_KINDS and not healed:
                assert info["nonfinite_compared"] > 0, (B.case_id(c), info)
            if kind in ("nan_vx", "nan_vy", "nan_both", "inf_vx", "inf_vy") and "fastest" in info:
                assert info["fastest"] == float("inf"), (B.case_id(c), info)  # (d): a non-finite velocity went through the exact path, and says so
            if kind in B.HUGE_KINDS and "fastest" in info:
                assert info["fastest"] >= 1.0e4, (B.case_id(c), info)
            if config in ("dry_pairs", "dry_pairs_plain") and c["compare"] == "finite":
                assert "pair_stats" in info and info["launches"].get("march_dry2_two_iterations_per_launch", 0) > 0, (B.case_id(c), info)
            if config.startswith("dry_single") and c["compare"] == "finite":
                assert info["launches"].get("march_dry_vel_advect_pressure", 0) > 0, (B.case_id(c), info)
            if "pair_stats" in info and kind != "nan_T":  # (the dry stencil has no buoyancy -- that is the boundary pass: a NaN T is advected but never becomes a velocity)
                assert info["pair_stats"][0] > 0 or info["pair_stats"][1] > 0, (B.case_id(c), info)  # tiles recomputed or the pair repeated whole
            seen.append({k2: v for k2, v in info.items() if k2 != "census"})
    print(json.dumps({"kind": kind, "runs": len(seen), "reported_overflows": sum(1 for s in seen if s["reported"]),
                      "steps_compared": sum(s["compared_steps"] for s in seen), "finite_where_oracle_is_not": sum(s["finite_where_oracle_is_not"] for s in seen)}))


def test_nonfinite_droplets(pkg, oracle, fuzz):
    """Droplets with a NaN / Inf position or mass, and a finite droplet inside a NaN-velocity cell: no deposit address is made from
    them (the clip test fails for a NaN), the records and the feedback textures are the oracle's."""
    X, Y = 505, 77
    for config in ("splat_atomic", "splat_atomic_perpass"):
        info = run_config(pkg, fuzz, oracle, B.droplet_scene(X, Y), X, Y, config, steps=(1, 1))
        assert info["compared_steps"] >= 1 and info["nonfinite_compared"] > 0, info


@pytest.mark.parametrize("speed", B.GROWN_SPEEDS)
@pytest.mark.parametrize("config", ["wet", "perpass"])
def test_grown_blow_up_vs_oracle(pkg, oracle, fuzz, speed, config):
    """Nothing non-finite planted: the 20 / 80 cells-per-iteration spikes on the wet state, compared after EVERY iteration until the
    oracle's state has overflowed and GROWN_PAST iterations beyond. The marching kernel runs with an exact-path list that cannot
    overflow (WX_OPT_FIX_CAP: three entries per cell), so BOTH configurations are compared on the grown non-finite states."""
    X, Y = B.GROWN_GRID
    info = run_config(pkg, fuzz, oracle, B.grown_scene(X, Y, speed), X, Y, config, steps=(1,) * B.GROWN_ITERATIONS, fix_cap=3 * X * Y + 64,
                      stop_past_nonfinite=B.GROWN_PAST)
    assert info["reported"] is None and info["nonfinite_steps"] == B.GROWN_PAST + 1 and info["nonfinite_compared"] > 0, info
    assert info["compared_steps"] >= 5 + B.GROWN_PAST, info
    print(json.dumps(info))


@pytest.mark.parametrize("nslab", [2, 4, 8])
@pytest.mark.parametrize("where", ["watched_zone", "deep_inside"])
@pytest.mark.parametrize("mode", ["wet", "dry_single", "dry_pairs"])
def test_slabs_report_a_nonfinite_vx(pkg, mode, nslab, where):
    """A slab group on one GPU with a NaN vx in one cell -- in the watched zone next to a slab edge (the scan of the uploaded state sees
    it), or in the middle of a slab (only the marching kernel that steps it can: the wet one, the one-iteration dry one, the dry pair
    kernel). The velocity watch counts a NaN as +Inf, so the group REPORTS it -- no halo is wide enough for it -- where fmaxf made the
    blown-up neighbour pass for a calm one and the slab read ghost columns unreported."""
    E = pkg.engine
    X, Y, halo = 2016, 45, 12
    xo = X // nslab
    base, water, wall, _, _ = I.impulse_scene(X, Y, "smoke", plant=False)
    x = xo + 3 if where == "watched_zone" else xo + xo // 2
    base[20, x, 0] = np.nan
    u = B.scene_uniforms(Y, dry=mode != "wet")
    g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
    try:
        g.set_option(E.Handle.OPT_DRY_PAIRS, 1 if mode == "dry_pairs" else 0)
        g.upload(base, water, wall)
        g.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
        with pytest.raises(E.WxError) as ei:
            g.step(2)
            g.sync()
            g.step(2)
            g.sync()
        assert "vx" in str(ei.value), str(ei.value)
    finally:
        g.close()


@pytest.mark.parametrize("variant", ["flat", "stepped"])
@pytest.mark.parametrize("kind", ["divisor_soil", "divisor_snow"])
def test_fire_divisor_zero_and_negative_vs_oracle(pkg, oracle, fuzz, kind, variant):
    """surface_scenes.divisor_scene: uploaded soil moisture / snow far below zero make the fire-spread divisor of the sites 0 (`% 0`:
    fixed to false, guarded on both sides -- no integer division by zero is executed) and -10 (ignites at iterNum 1000), under smoke
    that would light every site. Wet marching (display / plain / MORE_TO_COME, stored waterTexture_0, row bands) and per-pass, lattice
    offsets that put the sites on the first and last output lanes of a strip, bit for bit."""
    import surface_scenes as S
    X, Y = S.PHASE_GRID
    for off in (0, 2, 4):
        scene = S.divisor_scene(X, Y, kind, offset=off, variant=variant)
        for config in B.WET_CONFIGS + B.BAND_CONFIGS[:2]:
            bad, wall = S.run_scene(pkg, fuzz, oracle, scene, X, Y, config, 1000, fuzz.IMPULSE_CONFIGS[config].get("steps", (1, 1, 3)))
            assert not bad, json.dumps({"kind": kind, "variant": variant, "offset": off, "config": config, "mismatches": bad})
            lit = [int(wall[y, x, 0]) == S.FIRE for x, y in scene[3]]
            assert lit == S.divisor_sites_lit(X, scene[3], variant), (config, lit)
