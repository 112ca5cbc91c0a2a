"""Ensembles (wx_ensemble_*, include/wxsim.h) without a GPU: the header announces and declares the feature, the library exports it, the
argument checks answer before any device is touched, a missing device is an error (no CPU fallback), and the share-of-chip launch
shape of a member (csrc/wx_wet.h: wet_launch_shape_member, through a small host-only harness) covers every row exactly once for every
(grid, members) of a sweep and is the lone handle's shape for a lone member."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["wx_ensemble_create", "wx_ensemble_destroy", "wx_ensemble_last_error", "wx_ensemble_count", "wx_ensemble_member", "wx_ensemble_step",
         "wx_ensemble_sync", "wx_ensemble_diagnostics", "wx_ensemble_stats"]
E_INVALID, E_DEVICE = -1, -2


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    assert "typedef struct wx_ensemble wx_ensemble;" in hdr
    L = pkg.engine.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in pkg.engine.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert hasattr(pkg.engine, "Ensemble") and hasattr(pkg.sim, "WeatherEnsemble")


def test_create_checks_arguments_before_it_looks_for_a_device(pkg):
    L = pkg.engine.lib()
    for args in ((0, 100, 100), (-3, 100, 100), (4, 1, 100), (4, 100, 3), (4, 100, 70000), (4, 65535 * 16 + 1, 100), (70000, 100, 100)):
        e = C.c_void_p(0x1234)
        assert L.wx_ensemble_create(*args, C.byref(e)) == E_INVALID, args
        assert not e.value, args  # *out is cleared
        assert b"wx_ensemble_create" in L.wx_ensemble_last_error(None), args
    assert L.wx_ensemble_create(4, 100, 100, None) == E_INVALID


def test_null_handles_are_refused(pkg):
    L = pkg.engine.lib()
    a = C.c_int64(7)
    assert L.wx_ensemble_step(None, 1) == E_INVALID
    assert L.wx_ensemble_sync(None) == E_INVALID
    assert L.wx_ensemble_diagnostics(None, None) == E_INVALID
    assert L.wx_ensemble_stats(None, C.byref(a), None, None) == E_INVALID and a.value == 7
    assert L.wx_ensemble_count(None) == 0
    assert not L.wx_ensemble_member(None, 0)
    L.wx_ensemble_destroy(None)  # a no-op
    assert isinstance(L.wx_ensemble_last_error(None), bytes)


def test_without_a_device_create_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal needs a machine without one")
    L = pkg.engine.lib()
    e = C.c_void_p()
    assert L.wx_ensemble_create(4, 100, 100, C.byref(e)) == E_DEVICE
    assert not e.value
    assert b"no CPU fallback" in L.wx_ensemble_last_error(None)
    with pytest.raises(pkg.engine.WxError) as ei:
        pkg.engine.Ensemble(4, 100, 100)
    assert ei.value.code == E_DEVICE


# ---- the share-of-chip launch shape ----
GRIDS = [(100, 100), (2500, 300), (16000, 500), (505, 77), (57, 9), (2, 4), (64, 8), (256, 96), (1000, 600), (4096, 1024), (130, 50), (57, 511)]
MEMBERS = [1, 2, 3, 5, 8, 16, 64, 257, 4096]


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("ens_shape") / "ensemble_shape_harness")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "ensemble_shape_harness.hip")])
    args = [str(v) for g in GRIDS for m in MEMBERS for v in (g[0], g[1], m)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("WX_WET_")}
    return json.loads(subprocess.check_output([exe] + args, env=env))


def test_member_segments_cover_every_row_once(shapes):
    assert len(shapes) == len(GRIDS) * len(MEMBERS) * 3
    for sh in shapes:
        X, Y, m = sh["X"], sh["Y"], sh["member"]
        st, n = m["start"], m["n_seg"]
        assert m["n_strips"] == (X + 55) // 56
        assert 1 <= n <= 128 and len(st) == n + 1 and st[0] == 0, sh
        assert all(b > a for a, b in zip(st, st[1:])), sh  # ascending, no empty segment: no gap, no overlap
        height = (Y + 7) // 8 if m["bands"] else Y  # (the table of a band is clipped to the band's own height by the kernel)
        assert st[-1] == height, sh
        if m["bands"]:
            for k in range(8):
                lo, hi = k * Y // 8, (k + 1) * Y // 8
                assert 0 < hi - lo <= height, sh
        assert m["bands"] == sh["lone"]["bands"], sh  # the share decides segment heights, never bands against column blocks
        assert m["groups_x"] % 8 == 0 and m["groups_x"] >= 8, sh  # blockIdx.x & 7 stays the XCD
        assert 1 <= sh["share"] <= sh["capacity"], sh


def test_a_lone_member_gets_the_lone_handles_shape(shapes):
    seen = 0
    for sh in shapes:
        if sh["members"] == 1:
            assert sh["share"] == sh["capacity"] and sh["member"] == sh["lone"], sh
            seen += 1
    assert seen == len(GRIDS) * 3


def test_the_share_shrinks_with_the_ensemble_and_segments_grow_at_the_benchmark_shapes(shapes):
    """By construction (wet_member_share): the share is capacity / members, never below one wave slot per strip, so it cannot grow with
    the ensemble. The segment COUNT is not monotonic in it (the tail shape of wet_launch_shape switches on and off with the capacity:
    100 x 100 cuts 50 segments alone and 75 as one of two), so that is not asserted; what the share is for is: at the sizes and member
    counts tools/ensemble_bench.py measures, a member marches taller segments (fewer warm-up rows per row) than the lone handle."""
    by = {}
    for sh in shapes:
        by.setdefault((sh["X"], sh["Y"], sh["bands_mode"]), []).append(sh)
    for key, group in by.items():
        group.sort(key=lambda s: s["members"])
        for a, b in zip(group, group[1:]):
            assert b["share"] <= a["share"], key
        for s in group:
            assert s["share"] >= min(s["capacity"], s["member"]["n_strips"]), key
            assert s["share"] == max(s["capacity"] // s["members"], min(s["capacity"], s["member"]["n_strips"])) or s["members"] == 1, key
    for (X, Y, members) in ((100, 100, 64), (2500, 300, 8), (16000, 500, 2)):
        sh = next(s for s in shapes if (s["X"], s["Y"], s["members"], s["bands_mode"]) == (X, Y, members, 1))
        assert sh["member"]["n_seg"] < sh["lone"]["n_seg"], sh
