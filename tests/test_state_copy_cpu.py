"""wx_copy_state / wx_ensemble_broadcast (include/wxsim.h) without a GPU: the header announces and declares the addition at the unchanged
ABI version, the library exports it, the Python layers carry it, and NULL arguments answer before any device is touched."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wx_copy_state", "wx_ensemble_broadcast"]
E_INVALID = -1


def test_header_announces_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "wxsim.h")).read()
    assert re.search(r"^#define\s+WX_HAVE_STATE_COPY\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_HAVE_ENSEMBLE_PERTURB\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+WX_ABI_VERSION\s+11\s*$", hdr, re.M)
    L = pkg.engine.lib()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in pkg.engine.EXPORTS, n
        getattr(L, n)
    assert L.wx_abi_version() == 11
    E, W = pkg.engine, pkg.sim
    for f in (E.Handle.copy_from, E.Ensemble.broadcast, W.WeatherSim.copy_from, W.WeatherEnsemble.from_sim, W.WeatherEnsemble.broadcast):
        assert callable(f)
    assert len(E.EXPORTS) == len(set(E.EXPORTS))


def test_null_arguments_answer_without_a_device(pkg):
    L = pkg.engine.lib()
    assert L.wx_copy_state(None, None) == E_INVALID
    assert L.wx_ensemble_broadcast(None, 0, None) == E_INVALID
    assert L.wx_ensemble_broadcast(None, -1, None) == E_INVALID
