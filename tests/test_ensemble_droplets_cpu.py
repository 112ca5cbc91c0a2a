"""Ensembles with droplets (wx_ensemble_create_droplets, wx_ensemble_particle_stats; include/wxsim.h) without a GPU: the header announces
and declares the addition at the unchanged ABI version, the library exports it, the argument checks answer before any device is touched,
and a missing device is an error (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_ensemble_create_droplets", "wx_ensemble_particle_stats"]
E_INVALID, E_DEVICE = -1, -2


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_DROPLETS\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    L = pkg.engine.lib()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in pkg.engine.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    assert "members are created with n_droplets = 0" not in hdr and "and the particle pass" not in hdr  # the refusals of the droplet-free ensemble
    import inspect
    assert "n_droplets" in inspect.signature(pkg.engine.Ensemble.__init__).parameters
    assert "droplets" in inspect.signature(pkg.sim.WeatherEnsemble.__init__).parameters
    assert hasattr(pkg.engine.Ensemble, "particle_stats") and hasattr(pkg.sim.WeatherEnsemble, "particle_stats")


def test_create_droplets_checks_arguments_before_it_looks_for_a_device(pkg):
    L = pkg.engine.lib()
    for args in ((0, 100, 100, 4), (4, 1, 100, 4), (4, 100, 3, 4), (4, 100, 100, -1), (70000, 100, 100, 4)):
        e = C.c_void_p(0x1234)
        assert L.wx_ensemble_create_droplets(*args, C.byref(e)) == E_INVALID, args
        assert not e.value, args  # *out is cleared
        assert b"wx_ensemble_create_droplets" in L.wx_ensemble_last_error(None), args
    assert L.wx_ensemble_create_droplets(4, 100, 100, 4, None) == E_INVALID
    # the older entry point keeps naming itself
    e = C.c_void_p(0x1234)
    assert L.wx_ensemble_create(0, 100, 100, C.byref(e)) == E_INVALID and not e.value
    assert b"wx_ensemble_create:" in L.wx_ensemble_last_error(None)


def test_particle_stats_refuses_a_null_ensemble(pkg):
    L = pkg.engine.lib()
    a, b = C.c_int64(7), C.c_int64(9)
    assert L.wx_ensemble_particle_stats(None, C.byref(a), C.byref(b)) == E_INVALID
    assert (a.value, b.value) == (7, 9)
    assert L.wx_ensemble_particle_stats(None, None, None) == E_INVALID


def test_without_a_device_create_droplets_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal needs a machine without one")
    L = pkg.engine.lib()
    e = C.c_void_p(0x1234)
    assert L.wx_ensemble_create_droplets(4, 100, 100, 400, C.byref(e)) == E_DEVICE
    assert not e.value
    assert b"no CPU fallback" in L.wx_ensemble_last_error(None)
    with pytest.raises(pkg.engine.WxError) as ei:
        pkg.engine.Ensemble(4, 100, 100, 400)
    assert ei.value.code == E_DEVICE
