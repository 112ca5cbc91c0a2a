"""ctypes binding of libwxsim.so (the C ABI of include/wxsim.h).

This is the ONLY compute path of the package: if the HIP library is missing or no GPU is present the
calls fail loudly (RuntimeError) -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

from .params import WxParams

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# WXSIM_LIB: another build of the same sources -- the tolerance build FAST_LIB_PATH (`make -C csrc fast`, SURVEY Appendix A's opt-in fast
# arithmetic; lib().wx_arith() says which one is loaded) or a tuning variant. The default is the parity build.
FAST_LIB_PATH = os.path.join(CSRC, "libwxsim_fast.so")
LIB_PATH = os.environ.get("WXSIM_LIB") or os.path.join(CSRC, "libwxsim.so")

FIELD_IDS = {
    "BASE_CUR": 0, "BASE_DISP": 1, "WATER_0": 2, "WATER_CUR": 3, "WALL_CUR": 4, "WALL_DISP": 5,
    "LIGHT_0": 6, "LIGHT_1": 7, "CURL": 8, "VORT": 9, "PRECIP_FB": 10, "PRECIP_DEP": 11, "LIGHTNING": 12, "EMITTED": 13,
}
FIELD_CHANNELS = {"CURL": 1, "VORT": 2, "PRECIP_DEP": 2}
DTYPE_F32, DTYPE_I8, DTYPE_I32, DTYPE_F16 = 0, 1, 2, 3

# every symbol include/wxsim.h declares
EXPORTS = [
    "wx_create", "wx_create_slab", "wx_destroy", "wx_last_error", "wx_abi_version", "wx_upload", "wx_set_params",
    "wx_step", "wx_sync", "wx_get_iter", "wx_set_iter", "wx_read_rect", "wx_read_particles", "wx_set_stream",
    "wx_device_ptr", "wx_local_width", "wx_halo_bytes", "wx_halo_message_bytes", "wx_halo_pack", "wx_halo_unpack", "wx_halo_pack_both", "wx_halo_unpack_both", "wx_profile",
    "wx_profile_read", "wx_kernel_count", "wx_kernel_name", "wx_slab_set_rank", "wx_slab_period_begin", "wx_pool_event_bytes",
    "wx_pool_edge_bytes", "wx_pool_events_pack", "wx_pool_events_apply", "wx_pool_edges_pack", "wx_pool_edges_apply", "wx_pool_flags", "wx_lightning_get", "wx_lightning_set", "wx_setup_columns", "wx_setup_terrain", "wx_init_droplets", "wx_fastest_velocity",
    "wx_stream_bytes", "wx_host_alloc", "wx_host_free", "wx_stream_frame", "wx_stream_wait", "wx_set_comm_stream", "wx_step_overlap",
    "wx_set_option", "wx_water_free", "wx_slab_assert_water_free", "wx_tune_placement",
    "wx_comm_unique_id", "wx_comm_init", "wx_exchange", "wx_slab_step", "wx_group_create", "wx_group_destroy", "wx_group_last_error",
    "wx_group_count", "wx_group_transport", "wx_group_slab", "wx_group_agree", "wx_group_step", "wx_group_sync", "wx_group_set_option",
    "wx_group_exchange", "wx_slab_vx_take", "wx_slab_set_vx_bound", "wx_slab_cone", "wx_slab_period", "wx_pair_stats", "wx_placement_info", "wx_arith",
    "wx_diag_collect", "wx_diag_merge", "wx_diag_finish", "wx_diag_accumulate", "wx_diag_accumulate_cells", "wx_diagnostics", "wx_group_diagnostics",
    "wx_ensemble_create", "wx_ensemble_destroy", "wx_ensemble_last_error", "wx_ensemble_count", "wx_ensemble_member", "wx_ensemble_step",
    "wx_ensemble_sync", "wx_ensemble_diagnostics", "wx_ensemble_stats", "wx_ensemble_create_droplets", "wx_ensemble_particle_stats",
    "wx_ensemble_statistics", "wx_ens_stat_cells",
    "wx_copy_state", "wx_ensemble_broadcast", "wx_ensemble_perturb", "wx_ens_perturb_cells",
    "wx_ensemble_quantiles", "wx_ens_quant_cells", "wx_ens_quant_staged_members",
    "wx_ensemble_scores", "wx_ens_score_cells", "wx_ens_score_max_members",
    "wx_ensemble_assimilate", "wx_ens_assim_cells",
    "wx_ensemble_prior_save", "wx_ensemble_prior_drop", "wx_ensemble_inflate", "wx_ens_inflate_cells",
    "wx_ensemble_covariance", "wx_ens_cov_cells",
    "wx_ensemble_neighbourhood", "wx_ens_nbhd_cells", "wx_ens_nbhd_max_radius",
    "wx_ensemble_gram", "wx_ens_gram_cells", "wx_ens_gram_max_members",
]


class WxDiag(C.Structure):
    """``wx_diag`` of include/wxsim.h, field for field (tests/test_diag_cpu.py compares the two)."""
    _fields_ = [
        ("iter", C.c_int64), ("n_air", C.c_int64), ("n_wall", C.c_int64), ("n_marker_mismatch", C.c_int64), ("n_negative_water", C.c_int64),
        ("n_nonfinite_base", C.c_int64), ("n_nonfinite_water", C.c_int64),
        ("first_nonfinite_base_x", C.c_int64), ("first_nonfinite_base_y", C.c_int64),
        ("first_nonfinite_water_x", C.c_int64), ("first_nonfinite_water_y", C.c_int64),
        ("sum_base", C.c_double * 4), ("sum_water", C.c_double * 4), ("sum_soil_moisture", C.c_double), ("sum_snow", C.c_double),
        ("sum_vegetation", C.c_int64),
        ("min_base", C.c_double * 4), ("max_base", C.c_double * 4), ("min_water", C.c_double * 4), ("max_water", C.c_double * 4),
        ("min_base_x", C.c_int64 * 4), ("min_base_y", C.c_int64 * 4), ("max_base_x", C.c_int64 * 4), ("max_base_y", C.c_int64 * 4),
        ("min_water_x", C.c_int64 * 4), ("min_water_y", C.c_int64 * 4), ("max_water_x", C.c_int64 * 4), ("max_water_y", C.c_int64 * 4),
        ("n_droplets_active", C.c_int64), ("n_droplets_nonfinite", C.c_int64),
        ("sum_droplet_mass_x", C.c_double), ("sum_droplet_mass_y", C.c_double),
    ]


DIAG_QUANTITIES, DIAG_BINS = 12, 16
# quantity numbers of wx_diag_accumulate (WX_DIAG_QUANTITIES): base and water channels over the air cells, the two wall-cell sums, the droplets
DIAG_Q = {"vx": 0, "vy": 1, "pressure": 2, "temperature": 3, "water": 4, "cloud": 5, "precipitation": 6, "smoke": 7,
          "soil_moisture": 8, "snow": 9, "droplet_mass_x": 10, "droplet_mass_y": 11}


class WxDiagRaw(C.Structure):
    """``wx_diag_raw``: what leaves the device (integers only); ``bytes(raw)`` is what the hosts exchange and merge."""
    _fields_ = [
        ("x_global", C.c_int64), ("y_rows", C.c_int64), ("iter", C.c_int64), ("count", C.c_int64 * 10),
        ("first_nonfinite", C.c_uint64 * 2), ("key_max", C.c_uint64 * 8), ("key_min", C.c_uint64 * 8),
        ("bin_hi", (C.c_int64 * DIAG_BINS) * DIAG_QUANTITIES), ("bin_lo", (C.c_uint64 * DIAG_BINS) * DIAG_QUANTITIES),
    ]


DIAG_RAW_BYTES = C.sizeof(WxDiagRaw)


def _diag_dict(d: WxDiag) -> dict:
    """wx_diag as a dict under the same names; every ``*_x`` / ``*_y`` pair becomes one ``*_at`` = (x, y) or None, an absent extreme is None."""
    def at(x, y):
        return (int(x), int(y)) if x >= 0 else None
    out = {}
    for name, _ in WxDiag._fields_:
        if name.endswith(("_x", "_y")) and not name.startswith("sum_"):
            continue
        v = getattr(d, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    out["first_nonfinite_base"] = at(d.first_nonfinite_base_x, d.first_nonfinite_base_y)
    out["first_nonfinite_water"] = at(d.first_nonfinite_water_x, d.first_nonfinite_water_y)
    for k in ("min_base", "max_base", "min_water", "max_water"):
        xs, ys = getattr(d, k + "_x"), getattr(d, k + "_y")
        out[k + "_at"] = [at(xs[c], ys[c]) for c in range(4)]
        out[k] = [out[k][c] if xs[c] >= 0 or out[k][c] == out[k][c] else None for c in range(4)]
    return out


def _raw_of(b) -> WxDiagRaw:
    if isinstance(b, WxDiagRaw):
        return b
    if len(b) != DIAG_RAW_BYTES:
        raise ValueError(f"a wx_diag_raw has {DIAG_RAW_BYTES} bytes, got {len(b)}")
    return WxDiagRaw.from_buffer_copy(bytes(b))


def diag_empty() -> bytes:
    """The empty set: a zero-filled wx_diag_raw."""
    return bytes(DIAG_RAW_BYTES)


def diag_merge(a, b) -> bytes:
    """wx_diag_merge over ``bytes``: the union of two disjoint sets of cells of one domain (associative and commutative, bit for bit)."""
    ra, rb = _raw_of(a), _raw_of(b)
    rc = lib().wx_diag_merge(C.byref(ra), C.byref(rb))
    if rc != 0:
        raise WxError(rc, "wx_diag_merge: the two parts disagree about geometry or iteration")
    return bytes(ra)


def diag_finish(raw) -> dict:
    """wx_diag_finish over ``bytes``: every sum rounded once (== math.fsum of the values that went in)."""
    r, d = _raw_of(raw), WxDiag()
    rc = lib().wx_diag_finish(C.byref(r), C.byref(d))
    if rc != 0:
        raise WxError(rc, "wx_diag_finish")
    return _diag_dict(d)


def diag_accumulate(raw, quantity, values) -> bytes:
    """wx_diag_accumulate over ``bytes``: float32 ``values`` added to the bins of ``quantity`` (a number or a DIAG_Q name) on the CPU."""
    r = _raw_of(raw)
    v = np.ascontiguousarray(values, np.float32).ravel()
    rc = lib().wx_diag_accumulate(C.byref(r), int(DIAG_Q.get(quantity, quantity)), v.ctypes.data, v.size)
    if rc != 0:
        raise WxError(rc, f"wx_diag_accumulate: quantity {quantity}")
    return bytes(r)


def diag_accumulate_cells(raw, X_global: int, Y: int, x: int, y: int, base, water, wall) -> bytes:
    """wx_diag_accumulate_cells over ``bytes``: the kernel's per-cell function on the CPU over a run of cells (n, 4) of row ``y`` from column ``x``."""
    r = _raw_of(raw)
    b, w = np.ascontiguousarray(base, np.float32).reshape(-1, 4), np.ascontiguousarray(water, np.float32).reshape(-1, 4)
    wl = np.ascontiguousarray(wall, np.int8).reshape(-1, 4)
    if not (len(b) == len(w) == len(wl)):
        raise ValueError("base, water and wall must hold the same number of cells")
    rc = lib().wx_diag_accumulate_cells(C.byref(r), int(X_global), int(Y), int(x), int(y), len(b), b.ctypes.data, w.ctypes.data, wl.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_diag_accumulate_cells: bad geometry or range")
    return bytes(r)


class WxEnsStat(C.Structure):
    """``wx_ens_stat`` of include/wxsim.h: caller-owned output planes (NULL = not wanted) and the four thresholds."""
    _fields_ = [
        ("mean", C.c_void_p), ("variance", C.c_void_p), ("min", C.c_void_p), ("max", C.c_void_p), ("argmin", C.c_void_p), ("argmax", C.c_void_p),
        ("count", C.c_void_p), ("n_above", C.c_void_p), ("n_wall", C.c_void_p), ("threshold", C.c_float * 4),
    ]


# the planes of wx_ens_stat: name, element type, channels per cell
ENS_STAT_PLANES = (("mean", np.float32, 4), ("variance", np.float32, 4), ("min", np.float32, 4), ("max", np.float32, 4), ("argmin", np.int32, 4),
                   ("argmax", np.int32, 4), ("count", np.int32, 4), ("n_above", np.int32, 4), ("n_wall", np.int32, 1))
ENS_STAT_ALL = tuple(name for name, _, _ in ENS_STAT_PLANES)


def _ens_stat_struct(shape, threshold, want):
    """A wx_ens_stat over fresh arrays of ``shape`` + (4,) (n_wall: ``shape``) for the planes named in ``want``, and those arrays by name."""
    unknown = set(want) - set(ENS_STAT_ALL)
    if unknown:
        raise KeyError(f"no such plane of wx_ens_stat: {sorted(unknown)} (there are {ENS_STAT_ALL})")
    st, planes = WxEnsStat(), {}
    for name, dt, ch in ENS_STAT_PLANES:
        if name in want:
            planes[name] = np.zeros(tuple(shape) + ((ch,) if ch > 1 else ()), dt)
            setattr(st, name, planes[name].ctypes.data)
    st.threshold[:] = [float(t) for t in threshold]
    return st, planes


def _member_mask(n: int, members) -> Optional[np.ndarray]:
    """``members``: None (all), member indices, or n booleans -> the n bytes wx_ensemble_statistics / wx_ens_stat_cells take."""
    if members is None:
        return None
    m = np.asarray(members)
    if m.dtype == np.bool_:
        if m.shape != (n,):
            raise ValueError(f"a boolean member mask has one entry per member ({n})")
        return np.ascontiguousarray(m, np.uint8)
    mask = np.zeros(n, np.uint8)
    for i in m.ravel():
        if not 0 <= int(i) < n:
            raise IndexError(f"member {int(i)} of {n}")
        mask[int(i)] = 1
    return mask


def ens_stat_cells(fields, walls, *, members=None, threshold=(0, 0, 0, 0), want=ENS_STAT_ALL) -> dict:
    """wx_ens_stat_cells: the statistics kernel's per-cell function on the CPU. ``fields[i]`` / ``walls[i]``: member i's cells, float32
    (..., 4) and int8 (..., 4) of one common shape (what ``read_rect`` returns); the planes come back in that shape."""
    f = [np.ascontiguousarray(a, np.float32) for a in fields]
    wl = [np.ascontiguousarray(a, np.int8) for a in walls]
    n = len(f)
    if n < 1 or len(wl) != n or any(a.shape != f[0].shape or a.shape[-1:] != (4,) for a in f + wl):
        raise ValueError("one (..., 4) field and one (..., 4) wall array per member, all of one shape")
    shape = f[0].shape[:-1]
    st, planes = _ens_stat_struct(shape, threshold, want)
    fp, wp = (C.c_void_p * n)(*[a.ctypes.data for a in f]), (C.c_void_p * n)(*[a.ctypes.data for a in wl])
    mask = _member_mask(n, members)
    rc = lib().wx_ens_stat_cells(n, int(np.prod(shape, dtype=np.int64)), fp, wp, None if mask is None else mask.ctypes.data, C.byref(st))
    if rc != 0:
        raise WxError(rc, "wx_ens_stat_cells: no member selected")
    return planes


class WxEnsPerturb(C.Structure):
    """``wx_ens_perturb`` of include/wxsim.h, member for member."""
    _fields_ = [
        ("field", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("mode", C.c_int32), ("scale", C.c_int32),
        ("wrap_x", C.c_int32), ("seed", C.c_uint32), ("amplitude", C.c_float * 4), ("lo", C.c_float * 4), ("hi", C.c_float * 4),
    ]


PERTURB_MODES = {"add": 0, "mul": 1}


def _four(v, fill):
    """A scalar or up to four per-channel values (None: ``fill``) as four floats."""
    if v is None:
        return [fill] * 4
    a = np.asarray(v, np.float64).ravel()
    if a.size == 1:
        return [float(a[0])] * 4
    if a.size != 4:
        raise ValueError("one value or one per channel (4)")
    return [float(x) for x in a]


def _perturb_struct(field, amplitude, mode, scale, seed, wrap_x, rect, lo, hi) -> WxEnsPerturb:
    p = WxEnsPerturb()
    p.field = int(FIELD_IDS.get(field, field))
    p.x, p.y, p.w, p.h = [int(v) for v in rect]
    p.mode = int(PERTURB_MODES.get(mode, mode))
    p.scale, p.wrap_x, p.seed = int(scale), 1 if wrap_x else 0, int(seed) & 0xFFFFFFFF
    p.amplitude[:] = _four(amplitude, 0.0)
    p.lo[:] = _four(lo, float("nan"))
    p.hi[:] = _four(hi, float("nan"))
    return p


def ens_perturb_cells(fields, walls, X: int, Y: int, field, amplitude, *, mode="add", scale=1, seed=0, wrap_x=False, rect=None, members=None,
                      lo=None, hi=None) -> list:
    """wx_ens_perturb_cells: the perturbation kernel's per-cell function on the CPU. ``fields[i]`` / ``walls[i]``: member i's cells of the
    rectangle ``rect`` = (x, y, w, h) (None: the whole X x Y grid), float32 (h, w, 4) and int8 (h, w, 4); an unselected member's entries
    may be None. Returns new arrays (the selected members' perturbed, the others as given); the arguments are not changed."""
    rect = (0, 0, int(X), int(Y)) if rect is None else tuple(int(v) for v in rect)
    n = len(fields)
    mask = _member_mask(n, members)
    shape = (max(rect[3], 0), max(rect[2], 0), 4)
    out = [None if a is None else np.array(a, np.float32, order="C") for a in fields]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    if n < 1 or len(wl) != n or any(a is not None and a.shape != shape for a in out + wl):
        raise ValueError(f"one {shape} field and one {shape} wall array per member")
    fp = (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in out])
    wp = (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in wl])
    p = _perturb_struct(field, amplitude, mode, scale, seed, wrap_x, rect, lo, hi)
    rc = lib().wx_ens_perturb_cells(C.byref(p), int(X), int(Y), n, fp, wp, None if mask is None else mask.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_ens_perturb_cells: bad descriptor, rectangle outside the grid, or no member selected")
    return out


ENS_OBS_MAX = 256


class WxEnsObs(C.Structure):
    """``wx_ens_obs`` of include/wxsim.h: one scalar observation of one channel of one cell."""
    _fields_ = [("field", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("channel", C.c_int32), ("value", C.c_float), ("error_var", C.c_float)]


class WxEnsObsResult(C.Structure):
    """``wx_ens_obs_result`` of include/wxsim.h: what the call says about one observation."""
    _fields_ = [("applied", C.c_int32), ("pad", C.c_int32), ("prior_mean", C.c_double), ("prior_var", C.c_double), ("innovation", C.c_double),
                ("alpha", C.c_double)]


class WxEnsAssim(C.Structure):
    """``wx_ens_assim`` of include/wxsim.h, member for member."""
    _fields_ = [
        ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("wrap_x", C.c_int32), ("loc_x", C.c_float), ("loc_y", C.c_float),
        ("gain_base", C.c_float * 4), ("gain_water", C.c_float * 4),
        ("lo_base", C.c_float * 4), ("hi_base", C.c_float * 4), ("lo_water", C.c_float * 4), ("hi_water", C.c_float * 4),
    ]


def _assim_struct(rect, loc, wrap_x, gain_base, gain_water, lo_base, hi_base, lo_water, hi_water) -> WxEnsAssim:
    a = WxEnsAssim()
    a.x, a.y, a.w, a.h = [int(v) for v in rect]
    a.wrap_x = 1 if wrap_x else 0
    a.loc_x, a.loc_y = float(loc[0]), float(loc[1])
    a.gain_base[:], a.gain_water[:] = _four(gain_base, 0.0), _four(gain_water, 0.0)
    nan = float("nan")
    a.lo_base[:], a.hi_base[:], a.lo_water[:], a.hi_water[:] = _four(lo_base, nan), _four(hi_base, nan), _four(lo_water, nan), _four(hi_water, nan)
    return a


def _obs_array(observations):
    """``(field, x, y, channel, value, error_var)`` tuples (field: a name or a WX_FIELD_* number) as an array of wx_ens_obs."""
    obs = (WxEnsObs * max(len(observations), 1))()
    for j, (field, x, y, channel, value, error_var) in enumerate(observations):
        obs[j].field, obs[j].x, obs[j].y, obs[j].channel = int(FIELD_IDS.get(field, field)), int(x), int(y), int(channel)
        obs[j].value, obs[j].error_var = float(value), float(error_var)
    return obs


def _obs_results(res, n: int) -> list:
    return [{"applied": bool(r.applied), "prior_mean": r.prior_mean, "prior_var": r.prior_var, "innovation": r.innovation, "alpha": r.alpha}
            for r in res[:n]]


def ens_assim_cells(bases, waters, walls, X: int, Y: int, observations, *, loc=(0.0, 0.0), rect=None, members=None, wrap_x=False,
                    gain_base=(0, 0, 0, 1), gain_water=0.0, lo_base=None, hi_base=None, lo_water=None, hi_water=None):
    """wx_ens_assim_cells: the serial ensemble square-root filter of include/wxsim.h on the CPU, literally as defined. ``bases[i]`` /
    ``waters[i]`` / ``walls[i]``: member i's WHOLE grid, float32 (Y, X, 4) and int8 (Y, X, 4); an unselected member's entries may be
    None. ``observations``: ``(field, x, y, channel, value, error_var)`` tuples, taken in order. Returns (new bases, new waters, one
    result dict per observation); the arguments are not changed."""
    rect = (0, 0, int(X), int(Y)) if rect is None else tuple(int(v) for v in rect)
    n = len(bases)
    mask = _member_mask(n, members)
    shape = (int(Y), int(X), 4)
    nb = [None if a is None else np.array(a, np.float32, order="C") for a in bases]
    nw = [None if a is None else np.array(a, np.float32, order="C") for a in waters]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    if n < 1 or len(nw) != n or len(wl) != n or any(a is not None and a.shape != shape for a in nb + nw + wl):
        raise ValueError(f"one {shape} base, water and wall array per member")
    ptrs = lambda arrs: (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    a = _assim_struct(rect, loc, wrap_x, gain_base, gain_water, lo_base, hi_base, lo_water, hi_water)
    obs, res = _obs_array(observations), (WxEnsObsResult * max(len(observations), 1))()
    rc = lib().wx_ens_assim_cells(C.byref(a), len(observations), obs, res, int(X), int(Y), n, ptrs(nb), ptrs(nw), ptrs(wl),
                                  None if mask is None else mask.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_ens_assim_cells: bad descriptor or observation, rectangle or observation outside the grid, or fewer than two members selected")
    return nb, nw, _obs_results(res, len(observations))


INFLATE_MODES = {"const": 0, "rtps": 1, "rtpp": 2}


class WxEnsInflate(C.Structure):
    """``wx_ens_inflate`` of include/wxsim.h, member for member."""
    _fields_ = [
        ("field", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("mode", C.c_int32),
        ("coef", C.c_float * 4), ("lambda_lo", C.c_float), ("lambda_hi", C.c_float), ("lo", C.c_float * 4), ("hi", C.c_float * 4),
        ("lambda_out", C.c_void_p),
    ]


def _inflate_struct(field, coef, mode, rect, lambda_bounds, lo, hi, lambda_out=None) -> WxEnsInflate:
    p = WxEnsInflate()
    p.field = int(FIELD_IDS.get(field, field))
    p.x, p.y, p.w, p.h = [int(v) for v in rect]
    p.mode = int(INFLATE_MODES.get(mode, mode))
    p.coef[:] = _four(coef, 1.0 if p.mode == 0 else 0.0)
    nan = float("nan")
    lb = (None, None) if lambda_bounds is None else lambda_bounds
    p.lambda_lo, p.lambda_hi = [nan if v is None else float(v) for v in lb]
    p.lo[:], p.hi[:] = _four(lo, nan), _four(hi, nan)
    p.lambda_out = None if lambda_out is None else lambda_out.ctypes.data
    return p


def ens_inflate_cells(fields, walls, field, coef, *, mode="const", priors=None, members=None, lambda_bounds=None, lo=None, hi=None, want_lambda=False):
    """wx_ens_inflate_cells: covariance inflation (``mode`` "const": ``coef`` = lambda per channel, 1 = untouched) or relaxation to the
    prior ("rtps", "rtpp": ``coef`` = alpha, 0 = untouched) over the members, on the CPU, literally as include/wxsim.h defines it.
    ``fields[i]`` / ``walls[i]`` / ``priors[i]``: member i's cells, float32 (..., 4), int8 (..., 4) and float32 (..., 4) of one common
    shape; an unselected member's entries may be None, and so may ``priors`` in mode "const". Returns new arrays (the arguments are not
    changed), or with ``want_lambda`` (new arrays, the map of the lambda applied: NaN where a channel was left alone)."""
    n = len(fields)
    mask = _member_mask(n, members)
    out = [None if a is None else np.array(a, np.float32, order="C") for a in fields]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    pr = [None] * n if priors is None else [None if a is None else np.ascontiguousarray(a, np.float32) for a in priors]
    have = [a for a in out if a is not None]
    if n < 1 or len(wl) != n or len(pr) != n or not have or any(a is not None and (a.shape != have[0].shape or a.shape[-1:] != (4,)) for a in out + wl + pr):
        raise ValueError("one (..., 4) field, wall and (in the relaxation modes) prior array per member, all of one shape")
    shape = have[0].shape[:-1]
    lam = np.zeros(tuple(shape) + (4,), np.float32) if want_lambda else None
    ptrs = lambda arrs: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    p = _inflate_struct(field, coef, mode, (0, 0, 1, 1), lambda_bounds, lo, hi, lam)
    rc = lib().wx_ens_inflate_cells(C.byref(p), n, int(np.prod(shape, dtype=np.int64)), ptrs(out), ptrs(wl), None if priors is None else ptrs(pr),
                                    None if mask is None else mask.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_ens_inflate_cells: bad descriptor, a missing array of a selected member, or fewer than two members selected")
    return (out, lam) if want_lambda else out


ENS_COV_MAX = 8
COV_SOURCES = {"current": 0, "prior": 1}
COV_PLANES = ("cov", "corr", "slope", "variance")


class WxEnsCovPred(C.Structure):
    """``wx_ens_cov_pred`` of include/wxsim.h, member for member: one scalar predictor."""
    _fields_ = [("kind", C.c_int32), ("field", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("channel", C.c_int32), ("pad", C.c_int32),
                ("values", C.c_void_p)]


class WxEnsCovResult(C.Structure):
    """``wx_ens_cov_result`` of include/wxsim.h: what the call says about one predictor."""
    _fields_ = [("valid", C.c_int32), ("pad", C.c_int32), ("mean", C.c_double), ("variance", C.c_double)]


class WxEnsCov(C.Structure):
    """``wx_ens_cov`` of include/wxsim.h, member for member: what is asked for and the caller-owned output planes (NULL = not wanted)."""
    _fields_ = [
        ("field", C.c_int32), ("source", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("n_pred", C.c_int32), ("pad", C.c_int32),
        ("cov", C.c_void_p), ("corr", C.c_void_p), ("slope", C.c_void_p), ("variance", C.c_void_p),
    ]


def _cov_predictors(predictors, n_members: int):
    """``(field, x, y, channel)`` tuples (a point of the members' current state; field: a name) or sequences / arrays of one number per
    member, as an array of wx_ens_cov_pred. Returns (the array, the float64 arrays it points into)."""
    preds = (WxEnsCovPred * max(len(predictors), 1))()
    keep = []
    for j, p in enumerate(predictors):
        if isinstance(p, (tuple, list)) and len(p) == 4 and isinstance(p[0], str):
            preds[j].kind = 0
            preds[j].field, preds[j].x, preds[j].y, preds[j].channel = int(FIELD_IDS.get(p[0], -1)), int(p[1]), int(p[2]), int(p[3])
        else:
            v = np.ascontiguousarray(p, np.float64).reshape(-1)
            if v.size != n_members:
                raise ValueError(f"predictor {j}: {v.size} numbers for {n_members} members (one per member, by member index)")
            keep.append(v)
            preds[j].kind, preds[j].values = 1, v.ctypes.data
    return preds, keep


def _cov_struct(field, source, rect, n_pred: int, want):
    for name in want:
        if name not in COV_PLANES:
            raise ValueError(f"want: {name!r} is none of {COV_PLANES}")
    c = WxEnsCov()
    c.field, c.source = int(FIELD_IDS.get(field, field)), int(COV_SOURCES.get(source, source))
    c.x, c.y, c.w, c.h = [int(v) for v in rect]
    c.n_pred = int(n_pred)
    h, w, k = max(c.h, 0), max(c.w, 0), max(min(c.n_pred, ENS_COV_MAX), 0)
    planes = {name: np.zeros(((h, w, 4) if name == "variance" else (k, h, w, 4)), np.float32) for name in COV_PLANES if name in want}
    for name, a in planes.items():
        setattr(c, name, a.ctypes.data)
    return c, planes


def _cov_results(res, n: int) -> list:
    return [{"valid": bool(r.valid), "mean": r.mean, "variance": r.variance} for r in res[:n]]


def ens_cov_cells(bases, waters, walls, X: int, Y: int, field, predictors, *, source="current", rect=None, members=None, priors=None,
                  want=COV_PLANES) -> dict:
    """wx_ens_cov_cells: the covariance, correlation and sensitivity maps of include/wxsim.h on the CPU, literally as defined.
    ``bases[i]`` / ``waters[i]`` / ``walls[i]``: member i's WHOLE grid, float32 (Y, X, 4) and int8 (Y, X, 4); an unselected member's
    entries may be None, and so may a whole list that neither the state nor a point predictor needs. ``priors[i]``: the (h, w, 4) cells
    of ``rect`` of member i's snapshot (``source`` "prior" only). ``predictors``: ``(field name, x, y, channel)`` tuples or one number
    per member. Returns the planes named in ``want`` -- cov, corr, slope: (n_pred, h, w, 4); variance: (h, w, 4) -- and ``results``."""
    rect = (0, 0, int(X), int(Y)) if rect is None else tuple(int(v) for v in rect)
    n = len(walls)
    mask = _member_mask(n, members)
    shape, pshape = (int(Y), int(X), 4), (max(rect[3], 0), max(rect[2], 0), 4)
    conv = lambda arrs, t: None if arrs is None else [None if a is None else np.ascontiguousarray(a, t) for a in arrs]  # noqa: E731
    nb, nw, wl, pr = conv(bases, np.float32), conv(waters, np.float32), conv(walls, np.int8), conv(priors, np.float32)
    for arrs, shp in ((nb, shape), (nw, shape), (wl, shape), (pr, pshape)):
        if arrs is not None and (len(arrs) != n or any(a is not None and a.shape != shp for a in arrs)):
            raise ValueError(f"one {shape} base, water and wall array and (source prior) one {pshape} prior array per member")
    if n < 1:
        raise ValueError("no members")
    ptrs = lambda arrs: None if arrs is None else (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    preds, keep = _cov_predictors(predictors, n)
    c, planes = _cov_struct(field, source, rect, len(predictors), want)
    res = (WxEnsCovResult * max(len(predictors), 1))()
    rc = lib().wx_ens_cov_cells(C.byref(c), preds, res, int(X), int(Y), n, ptrs(nb), ptrs(nw), ptrs(wl), ptrs(pr), None if mask is None else mask.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_ens_cov_cells: bad descriptor or predictor, rectangle or point outside the grid, a missing array, or fewer than two members selected")
    planes["results"] = _cov_results(res, len(predictors))
    del keep
    return planes


ENS_GRAM_MAX_MEMBERS = 64
GRAM_CENTERS = {"mean": 0, "none": 1}


class WxEnsGram(C.Structure):
    """``wx_ens_gram`` of include/wxsim.h, member for member: what is asked for, the caller-owned matrix and the counts."""
    _fields_ = [
        ("field", C.c_int32), ("center", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("gram", C.c_void_p),
        ("n_entered", C.c_int64 * 4), ("n_excluded", C.c_int64 * 4), ("n_overflow", C.c_int64 * 4),
        ("n_selected", C.c_int32), ("pad", C.c_int32),
    ]


def _gram_struct(field, center, rect, n_sel: int):
    """A wx_ens_gram whose matrix is a fresh (4, n_sel, n_sel) float64 array. Returns (the struct, the array)."""
    g = WxEnsGram()
    g.field, g.center = int(FIELD_IDS.get(field, field)), int(GRAM_CENTERS.get(center, center))
    g.x, g.y, g.w, g.h = [int(v) for v in rect]
    gram = np.zeros((4, n_sel, n_sel), np.float64)
    g.gram = gram.ctypes.data
    return g, gram


def _gram_dict(g: WxEnsGram, gram: np.ndarray, sel) -> dict:
    return {"gram": gram, "n_entered": np.array(g.n_entered[:], np.int64), "n_excluded": np.array(g.n_excluded[:], np.int64),
            "n_overflow": np.array(g.n_overflow[:], np.int64), "members": [int(i) for i in sel]}


def _selected(n: int, members) -> list:
    mask = _member_mask(n, members)
    return list(range(n)) if mask is None else [i for i in range(n) if mask[i]]


def ens_gram_cells(fields, walls, X: int, Y: int, field, *, rect=None, members=None, center="mean") -> dict:
    """wx_ens_gram_cells: the members' Gram matrix of include/wxsim.h on the CPU, literally as defined. ``fields[i]`` / ``walls[i]``:
    member i's WHOLE grid of ``field``, float32 (Y, X, 4), and its wall texels, int8 (Y, X, 4); an unselected member's entries may be
    None. Returns ``gram`` (4, n, n) float64 over the selected members in ascending index, ``n_entered`` / ``n_excluded`` /
    ``n_overflow`` (4 each) and ``members``."""
    rect = (0, 0, int(X), int(Y)) if rect is None else tuple(int(v) for v in rect)
    n = len(walls)
    if n < 1 or len(fields) != n:
        raise ValueError("one field and one wall array per member")
    shape = (int(Y), int(X), 4)
    fl = [None if a is None else np.ascontiguousarray(a, np.float32) for a in fields]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    if any(a is not None and a.shape != shape for a in fl + wl):
        raise ValueError(f"one {shape} field and wall array per member")
    mask = _member_mask(n, members)
    sel = _selected(n, members)
    g, gram = _gram_struct(field, center, rect, len(sel))
    ptrs = lambda arrs: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    rc = lib().wx_ens_gram_cells(C.byref(g), int(X), int(Y), n, ptrs(fl), ptrs(wl), None if mask is None else mask.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_ens_gram_cells: a bad field or centre, a rectangle outside the grid, a missing array, or too few or too many members selected")
    return _gram_dict(g, gram, sel)


ENS_QUANT_MAX = 8
QUANT_INTERP = {"linear": 0, "lower": 1, "higher": 2}


class WxEnsQuant(C.Structure):
    """``wx_ens_quant`` of include/wxsim.h, member for member: what is asked for and the caller-owned output planes (NULL = not wanted)."""
    _fields_ = [
        ("n_q", C.c_int32), ("interp", C.c_int32), ("p", C.c_float * ENS_QUANT_MAX), ("rank_member", C.c_int32),
        ("q", C.c_void_p), ("count", C.c_void_p), ("n_wall", C.c_void_p), ("n_below", C.c_void_p), ("n_equal", C.c_void_p),
    ]


# the planes of wx_ens_quant: name, element type, channels per cell (q: n_q planes in front)
ENS_QUANT_PLANES = (("q", np.float32, 4), ("count", np.int32, 4), ("n_wall", np.int32, 1), ("n_below", np.int32, 4), ("n_equal", np.int32, 4))
ENS_QUANT_ALL = tuple(name for name, _, _ in ENS_QUANT_PLANES)


def _ens_quant_struct(shape, p, interp, rank_of, want):
    """A wx_ens_quant over fresh arrays of ``shape`` + (4,) (q: (n_q,) + ``shape`` + (4,); n_wall: ``shape``) for the planes named in
    ``want`` (None: all that make sense -- n_below / n_equal only with ``rank_of``), and those arrays by name."""
    if want is None:
        want = tuple(k for k in ENS_QUANT_ALL if rank_of is not None or k not in ("n_below", "n_equal"))
    unknown = set(want) - set(ENS_QUANT_ALL)
    if unknown:
        raise KeyError(f"no such plane of wx_ens_quant: {sorted(unknown)} (there are {ENS_QUANT_ALL})")
    ps = [float(v) for v in np.asarray(p, np.float32).ravel()]
    if len(ps) > ENS_QUANT_MAX:
        raise ValueError(f"at most {ENS_QUANT_MAX} quantiles per call")
    st, planes = WxEnsQuant(), {}
    st.n_q = len(ps) if "q" in want else 0
    st.interp = int(QUANT_INTERP.get(interp, interp))
    st.p[:len(ps)] = ps
    st.rank_member = -1 if rank_of is None else int(rank_of)
    for name, dt, ch in ENS_QUANT_PLANES:
        if name in want:
            planes[name] = np.zeros(((st.n_q,) if name == "q" else ()) + tuple(shape) + ((ch,) if ch > 1 else ()), dt)
            setattr(st, name, planes[name].ctypes.data)
    return st, planes


def _quant_mask(n: int, members, rank_of) -> Optional[np.ndarray]:
    """The member mask of a quantile call: with ``rank_of`` and no ``members`` the selection is everybody but the ranked member."""
    if members is None and rank_of is not None and 0 <= int(rank_of) < n:
        mask = np.ones(n, np.uint8)
        mask[int(rank_of)] = 0
        return mask
    return _member_mask(n, members)


def ens_quant_cells(fields, walls, p, *, members=None, interp="linear", rank_of=None, want=None) -> dict:
    """wx_ens_quant_cells: the quantile kernels' per-cell function on the CPU. ``fields[i]`` / ``walls[i]``: member i's cells, float32
    (..., 4) and int8 (..., 4) of one common shape (what ``read_rect`` returns; an unselected member's entries may be None); ``p``: up
    to 8 quantiles in [0, 1]. Returns ``q`` (n_q, ..., 4), ``count``, ``n_wall`` and -- with ``rank_of`` -- ``n_below``, ``n_equal``."""
    f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in fields]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    n = len(f)
    have = [a for a in f + wl if a is not None]
    if n < 1 or len(wl) != n or not have or any(a.shape != have[0].shape or a.shape[-1:] != (4,) for a in have):
        raise ValueError("one (..., 4) field and one (..., 4) wall array per member, all of one shape")
    shape = have[0].shape[:-1]
    st, planes = _ens_quant_struct(shape, p, interp, rank_of, want)
    fp = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in f])
    wp = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in wl])
    mask = _quant_mask(n, members, rank_of)
    rc = lib().wx_ens_quant_cells(n, int(np.prod(shape, dtype=np.int64)), fp, wp, None if mask is None else mask.ctypes.data, C.byref(st))
    if rc != 0:
        raise WxError(rc, "wx_ens_quant_cells: bad quantiles, interpolation or rank member, an absent member, or no member selected")
    return planes


ENS_SCORE_BINS = 65
ENS_SCORE_COUNTS = ("n_scored", "n_truth_excluded", "n_empty", "n_overflow", "sum_count")
ENS_SCORE_SUMS = ("sum_error", "sum_abs_error", "sum_sq_error", "sum_variance", "sum_crps")
ENS_SCORE_MAPS = ("error", "variance", "crps")


class WxEnsScore(C.Structure):
    """``wx_ens_score`` of include/wxsim.h, member for member: the scalars the call fills and the caller-owned maps (NULL = not wanted)."""
    _fields_ = ([(k, C.c_int64 * 4) for k in ENS_SCORE_COUNTS] + [(k, C.c_double * 4) for k in ENS_SCORE_SUMS]
                + [("rank_low", (C.c_int64 * ENS_SCORE_BINS) * 4), ("rank_high", (C.c_int64 * ENS_SCORE_BINS) * 4)] + [(k, C.c_void_p) for k in ENS_SCORE_MAPS])


def _ens_score_struct(shape, want):
    """A wx_ens_score whose maps named in ``want`` are fresh float32 arrays of ``shape`` + (4,), and those arrays by name."""
    unknown = set(want) - set(ENS_SCORE_MAPS)
    if unknown:
        raise KeyError(f"no such map of wx_ens_score: {sorted(unknown)} (there are {ENS_SCORE_MAPS})")
    st, maps = WxEnsScore(), {}
    for name in ENS_SCORE_MAPS:
        if name in want:
            maps[name] = np.zeros(tuple(shape) + (4,), np.float32)
            setattr(st, name, maps[name].ctypes.data)
    return st, maps


def _ens_score_dict(st: WxEnsScore, maps: dict) -> dict:
    out = {k: np.array(getattr(st, k), np.int64) for k in ENS_SCORE_COUNTS}
    out.update({k: np.array(getattr(st, k), np.float64) for k in ENS_SCORE_SUMS})
    out["rank_low"] = np.array([list(r) for r in st.rank_low], np.int64)
    out["rank_high"] = np.array([list(r) for r in st.rank_high], np.int64)
    out.update(maps)
    return out


def ens_score_cells(fields, walls, truth_field, truth_wall, *, members=None, want=ENS_SCORE_MAPS) -> dict:
    """wx_ens_score_cells: the score kernel's per-cell function and exact domain sums on the CPU. ``fields[i]`` / ``walls[i]``: member
    i's cells, float32 (..., 4) and int8 (..., 4) of one common shape (an unselected member's entries may be None); ``truth_field`` /
    ``truth_wall``: the truth's cells in that shape. Returns the entries of wx_ens_score: per channel n_scored, n_truth_excluded,
    n_empty, n_overflow, sum_count (int64), sum_error, sum_abs_error, sum_sq_error, sum_variance, sum_crps (float64), rank_low /
    rank_high (4, 65), and the maps named in ``want`` (error, variance, crps: (..., 4) float32, NaN where not scored)."""
    f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in fields]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    tf, tw = np.ascontiguousarray(truth_field, np.float32), np.ascontiguousarray(truth_wall, np.int8)
    n = len(f)
    have = [a for a in f + wl if a is not None] + [tf, tw]
    if n < 1 or len(wl) != n or any(a.shape != tf.shape or a.shape[-1:] != (4,) for a in have):
        raise ValueError("one (..., 4) field and one (..., 4) wall array per member and for the truth, all of one shape")
    shape = tf.shape[:-1]
    st, maps = _ens_score_struct(shape, want)
    fp = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in f])
    wp = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in wl])
    mask = _member_mask(n, members)
    rc = lib().wx_ens_score_cells(n, int(np.prod(shape, dtype=np.int64)), fp, wp, tf.ctypes.data, tw.ctypes.data, None if mask is None else mask.ctypes.data, C.byref(st))
    if rc != 0:
        raise WxError(rc, f"wx_ens_score_cells: no member or more than {Ensemble.SCORE_MAX_MEMBERS} selected, or a selected member absent")
    return _ens_score_dict(st, maps)


ENS_NBHD_MAX_RADIUS = 32
ENS_NBHD_MAX_SCALES = 8
ENS_NBHD_COUNTS = ("n_scored", "n_unscored")
ENS_NBHD_SUMS = ("sum_d2", "sum_f2", "sum_o2")
ENS_NBHD_TOTALS = ("ev_f", "n_f", "ev_o", "n_o")
ENS_NBHD_MAPS = ("nep", "obs_fraction")


class WxEnsNbhd(C.Structure):
    """``wx_ens_nbhd`` of include/wxsim.h, member for member: the event, the rectangle, the scales and the caller-owned maps (NULL = not wanted)."""
    _fields_ = [("field", C.c_int32), ("channel", C.c_int32), ("threshold", C.c_float), ("above", C.c_int32), ("wrap_x", C.c_int32),
                ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("n_scales", C.c_int32),
                ("rx", C.c_int32 * ENS_NBHD_MAX_SCALES), ("ry", C.c_int32 * ENS_NBHD_MAX_SCALES), ("nep", C.c_void_p), ("obs_fraction", C.c_void_p)]


class WxEnsNbhdResult(C.Structure):
    """``wx_ens_nbhd_result`` of include/wxsim.h: the counts and exact sums per scale, the point totals of the rectangle."""
    _fields_ = ([(k, C.c_int64 * ENS_NBHD_MAX_SCALES) for k in ENS_NBHD_COUNTS] + [(k, C.c_double * ENS_NBHD_MAX_SCALES) for k in ENS_NBHD_SUMS]
                + [(k, C.c_int64) for k in ENS_NBHD_TOTALS])


def _ens_nbhd_struct(field, channel, threshold, scales, above, wrap_x, rect, want):
    """A wx_ens_nbhd for ``scales`` = [(rx, ry), ...] (a single number r is (r, r)) whose maps named in ``want`` are fresh float32
    arrays (n_scales, h, w), and those arrays by name."""
    unknown = set(want) - set(ENS_NBHD_MAPS)
    if unknown:
        raise KeyError(f"no such map of wx_ens_nbhd: {sorted(unknown)} (there are {ENS_NBHD_MAPS})")
    pairs = [(int(s), int(s)) if np.ndim(s) == 0 else (int(s[0]), int(s[1])) for s in scales]
    a, maps = WxEnsNbhd(), {}
    a.field, a.channel, a.threshold = int(FIELD_IDS.get(field, field)), int(channel), float(threshold)
    a.above, a.wrap_x = int(bool(above)), int(bool(wrap_x))
    a.x, a.y, a.w, a.h = [int(v) for v in rect]
    a.n_scales = len(pairs)
    for s, (rx, ry) in enumerate(pairs[:ENS_NBHD_MAX_SCALES]):
        a.rx[s], a.ry[s] = rx, ry
    for name in ENS_NBHD_MAPS:
        if name in want:
            maps[name] = np.zeros((max(min(len(pairs), ENS_NBHD_MAX_SCALES), 0), max(a.h, 0), max(a.w, 0)), np.float32)
            setattr(a, name, maps[name].ctypes.data)
    return a, maps


def _ens_nbhd_dict(a: WxEnsNbhd, res: WxEnsNbhdResult, maps: dict) -> dict:
    n = max(min(a.n_scales, ENS_NBHD_MAX_SCALES), 0)
    out = {k: np.array(getattr(res, k), np.int64)[:n] for k in ENS_NBHD_COUNTS}
    out.update({k: np.array(getattr(res, k), np.float64)[:n] for k in ENS_NBHD_SUMS})
    out.update({k: int(getattr(res, k)) for k in ENS_NBHD_TOTALS})
    out.update(maps)
    return out


def ens_nbhd_cells(fields, walls, X: int, Y: int, field, channel, threshold, scales, truth_field=None, truth_wall=None, *, above=True, rect=None,
                   members=None, wrap_x=False, want=ENS_NBHD_MAPS) -> dict:
    """wx_ens_nbhd_cells: neighbourhood ensemble probabilities and the sums of the fractions skill score on the CPU, literally as
    include/wxsim.h defines them. ``fields[i]`` / ``walls[i]``: member i's whole grid, float32 (Y, X, 4) and int8 (Y, X, 4) (an
    unselected member's entries may be None); ``truth_field`` / ``truth_wall``: the truth's, or None for the forecast product alone.
    ``scales``: up to 8 (rx, ry) half-widths, 0 .. 32. Returns per scale n_scored, n_unscored (int64), sum_d2, sum_f2, sum_o2
    (float64), the totals ev_f, n_f, ev_o, n_o of ``rect`` = (x, y, w, h) (None: the whole grid), and the maps named in ``want`` (nep,
    obs_fraction: (n_scales, h, w) float32, NaN where the window holds no counted cell)."""
    f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in fields]
    wl = [None if a is None else np.ascontiguousarray(a, np.int8) for a in walls]
    tf = None if truth_field is None else np.ascontiguousarray(truth_field, np.float32)
    tw = None if truth_wall is None else np.ascontiguousarray(truth_wall, np.int8)
    n = len(f)
    have = [a for a in f + wl + [tf, tw] if a is not None]
    if n < 1 or len(wl) != n or any(a.shape != (Y, X, 4) for a in have):
        raise ValueError("one (Y, X, 4) field and one (Y, X, 4) wall array per member and for the truth")
    if tf is None:
        want = tuple(k for k in want if k != "obs_fraction")
    a, maps = _ens_nbhd_struct(field, channel, threshold, scales, above, wrap_x, (0, 0, X, Y) if rect is None else rect, want)
    res = WxEnsNbhdResult()
    fp = (C.c_void_p * n)(*[None if x is None else x.ctypes.data for x in f])
    wp = (C.c_void_p * n)(*[None if x is None else x.ctypes.data for x in wl])
    mask = _member_mask(n, members)
    rc = lib().wx_ens_nbhd_cells(C.byref(a), C.byref(res), int(X), int(Y), n, fp, wp, None if tf is None else tf.ctypes.data, None if tw is None else tw.ctypes.data,
                                 None if mask is None else mask.ctypes.data)
    if rc != 0:
        raise WxError(rc, "wx_ens_nbhd_cells: a bad field, channel, threshold, scale or rectangle, a wrapped window wider than the grid, an absent member, or no member selected")
    return _ens_nbhd_dict(a, res, maps)


def build(force: bool = False, fast: bool = False) -> str:
    """Compile libwxsim.so (``fast``: the tolerance build libwxsim_fast.so) for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "wxsim.h"))
    fast = fast or os.path.abspath(LIB_PATH) == os.path.abspath(FAST_LIB_PATH)
    target = FAST_LIB_PATH if fast else os.path.join(CSRC, "libwxsim.so")
    if os.path.abspath(LIB_PATH) not in (os.path.abspath(target),) and not fast:
        return LIB_PATH  # (a tuning variant named by WXSIM_LIB: built by its own make target)
    stale = (not os.path.exists(target)) or any(os.path.getmtime(f) > os.path.getmtime(target) for f in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", os.path.basename(target)])
    return target


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the simulation step.")
    try:
        # PyTorch ships its own libamdhip64.so.7: import it FIRST so that the process holds a single HIP runtime
        # (libwxsim.so's NEEDED libamdhip64.so.7 then resolves to the already loaded one). Loading ours first and
        # torch second gives two runtimes, and the second one finds "no ROCm-capable device".
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.wx_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.wx_create_slab.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.wx_destroy.argtypes = [vp]
    L.wx_destroy.restype = None
    L.wx_last_error.argtypes = [vp]
    L.wx_last_error.restype = C.c_char_p
    L.wx_abi_version.restype = i32
    L.wx_arith.restype = i32
    L.wx_upload.argtypes = [vp, vp, vp, vp, vp]
    L.wx_set_params.argtypes = [vp, C.POINTER(WxParams), vp, vp, vp, vp]
    L.wx_step.argtypes = [vp, i32]
    L.wx_step_overlap.argtypes = [vp, i32, C.c_uint]
    L.wx_set_comm_stream.argtypes = [vp, vp]
    L.wx_sync.argtypes = [vp]
    L.wx_set_option.argtypes = [vp, i32, i32]
    L.wx_water_free.argtypes = [vp]
    L.wx_tune_placement.argtypes = [vp, i32, i32, vp, vp]
    L.wx_slab_assert_water_free.argtypes = [vp, i32]
    L.wx_get_iter.argtypes = [vp]
    L.wx_get_iter.restype = i64
    L.wx_set_iter.argtypes = [vp, i64]
    L.wx_read_rect.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32]
    L.wx_read_particles.argtypes = [vp, i32, i32, vp]
    L.wx_set_stream.argtypes = [vp, vp]
    L.wx_device_ptr.argtypes = [vp, i32]
    L.wx_device_ptr.restype = vp
    L.wx_local_width.argtypes = [vp]
    L.wx_halo_bytes.argtypes = [vp]
    L.wx_halo_bytes.restype = C.c_size_t
    L.wx_halo_message_bytes.argtypes = [vp]
    L.wx_halo_message_bytes.restype = C.c_size_t
    L.wx_halo_pack.argtypes = [vp, i32, vp]
    L.wx_halo_unpack.argtypes = [vp, i32, vp]
    L.wx_halo_pack_both.argtypes = [vp, vp, vp]
    L.wx_halo_unpack_both.argtypes = [vp, vp, vp]
    L.wx_profile.argtypes = [vp, i32]
    L.wx_profile_read.argtypes = [vp, i32, vp, vp]
    L.wx_kernel_count.restype = i32
    L.wx_kernel_name.argtypes = [i32]
    L.wx_kernel_name.restype = C.c_char_p
    L.wx_slab_set_rank.argtypes = [vp, i32]
    L.wx_slab_period_begin.argtypes = [vp]
    L.wx_pool_event_bytes.argtypes = [vp]
    L.wx_pool_event_bytes.restype = C.c_size_t
    L.wx_pool_edge_bytes.argtypes = [vp]
    L.wx_pool_edge_bytes.restype = C.c_size_t
    L.wx_pool_events_pack.argtypes = [vp, vp]
    L.wx_pool_events_apply.argtypes = [vp, vp, i32, C.c_size_t]
    L.wx_pool_edges_pack.argtypes = [vp, vp, vp, i32]
    L.wx_pool_edges_apply.argtypes = [vp, vp]
    L.wx_pool_flags.argtypes = [vp, vp]
    L.wx_lightning_get.argtypes = [vp, vp]
    L.wx_lightning_set.argtypes = [vp, vp]
    L.wx_setup_columns.argtypes = [vp] + [vp] * 8
    L.wx_init_droplets.argtypes = [vp, C.c_uint32]
    L.wx_fastest_velocity.argtypes = [vp, C.POINTER(C.c_float)]
    L.wx_placement_info.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.wx_pair_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.wx_slab_vx_take.argtypes = [vp, C.POINTER(C.c_float)]
    L.wx_slab_set_vx_bound.argtypes = [vp, C.c_float]
    L.wx_slab_cone.argtypes = [vp]
    L.wx_slab_period.argtypes = [vp]
    L.wx_setup_terrain.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_double] + [vp] * 4
    L.wx_stream_bytes.argtypes = [i32, i32]
    L.wx_stream_bytes.restype = C.c_size_t
    L.wx_host_alloc.argtypes = [C.c_size_t]
    L.wx_host_alloc.restype = vp
    L.wx_host_free.argtypes = [vp]
    L.wx_host_free.restype = None
    L.wx_stream_frame.argtypes = [vp, i32, i32, i32, i32, vp]
    L.wx_stream_wait.argtypes = [vp]
    L.wx_comm_unique_id.argtypes = [vp]
    L.wx_comm_init.argtypes = [vp, vp, i32, i32]
    L.wx_exchange.argtypes = [vp]
    L.wx_slab_step.argtypes = [vp, i32]
    L.wx_group_create.argtypes = [i32, vp, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.wx_group_destroy.argtypes = [vp]
    L.wx_group_destroy.restype = None
    L.wx_group_last_error.argtypes = [vp]
    L.wx_group_last_error.restype = C.c_char_p
    L.wx_group_count.argtypes = [vp]
    L.wx_group_transport.argtypes = [vp]
    L.wx_group_slab.argtypes = [vp, i32]
    L.wx_group_slab.restype = vp
    L.wx_group_agree.argtypes = [vp]
    L.wx_group_step.argtypes = [vp, i32]
    L.wx_group_sync.argtypes = [vp]
    L.wx_group_set_option.argtypes = [vp, i32, i32]
    L.wx_group_exchange.argtypes = [vp]
    L.wx_diag_collect.argtypes = [vp, vp]
    L.wx_diag_merge.argtypes = [vp, vp]
    L.wx_diag_finish.argtypes = [vp, vp]
    L.wx_diag_accumulate.argtypes = [vp, i32, vp, C.c_size_t]
    L.wx_diag_accumulate_cells.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.wx_diagnostics.argtypes = [vp, vp]
    L.wx_group_diagnostics.argtypes = [vp, vp]
    L.wx_ensemble_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.wx_ensemble_create_droplets.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.wx_ensemble_particle_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.wx_ensemble_destroy.argtypes = [vp]
    L.wx_ensemble_destroy.restype = None
    L.wx_ensemble_last_error.argtypes = [vp]
    L.wx_ensemble_last_error.restype = C.c_char_p
    L.wx_ensemble_count.argtypes = [vp]
    L.wx_ensemble_member.argtypes = [vp, i32]
    L.wx_ensemble_member.restype = vp
    L.wx_ensemble_step.argtypes = [vp, i32]
    L.wx_ensemble_sync.argtypes = [vp]
    L.wx_ensemble_diagnostics.argtypes = [vp, vp]
    L.wx_ensemble_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.wx_ensemble_statistics.argtypes = [vp, i32, i32, i32, i32, i32, vp, C.POINTER(WxEnsStat)]
    L.wx_ens_stat_cells.argtypes = [i32, C.c_size_t, vp, vp, vp, C.POINTER(WxEnsStat)]
    L.wx_copy_state.argtypes = [vp, vp]
    L.wx_ensemble_broadcast.argtypes = [vp, i32, vp]
    L.wx_ensemble_perturb.argtypes = [vp, C.POINTER(WxEnsPerturb), vp]
    L.wx_ens_perturb_cells.argtypes = [C.POINTER(WxEnsPerturb), i32, i32, i32, vp, vp, vp]
    L.wx_ensemble_quantiles.argtypes = [vp, i32, i32, i32, i32, i32, vp, C.POINTER(WxEnsQuant)]
    L.wx_ens_quant_cells.argtypes = [i32, C.c_size_t, vp, vp, vp, C.POINTER(WxEnsQuant)]
    L.wx_ens_quant_staged_members.argtypes = []
    L.wx_ens_quant_staged_members.restype = i32
    L.wx_ensemble_scores.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, C.POINTER(WxEnsScore)]
    L.wx_ens_score_cells.argtypes = [i32, C.c_size_t, vp, vp, vp, vp, vp, C.POINTER(WxEnsScore)]
    L.wx_ens_score_max_members.argtypes = []
    L.wx_ens_score_max_members.restype = i32
    L.wx_ensemble_assimilate.argtypes = [vp, C.POINTER(WxEnsAssim), i32, vp, vp, vp]
    L.wx_ens_assim_cells.argtypes = [C.POINTER(WxEnsAssim), i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.wx_ensemble_prior_save.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    L.wx_ensemble_prior_drop.argtypes = [vp, i32]
    L.wx_ensemble_inflate.argtypes = [vp, C.POINTER(WxEnsInflate), vp]
    L.wx_ens_inflate_cells.argtypes = [C.POINTER(WxEnsInflate), i32, C.c_size_t, vp, vp, vp, vp]
    L.wx_ensemble_covariance.argtypes = [vp, C.POINTER(WxEnsCov), vp, vp, vp]
    L.wx_ens_cov_cells.argtypes = [C.POINTER(WxEnsCov), vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.wx_ensemble_neighbourhood.argtypes = [vp, vp, C.POINTER(WxEnsNbhd), vp, C.POINTER(WxEnsNbhdResult)]
    L.wx_ens_nbhd_cells.argtypes = [C.POINTER(WxEnsNbhd), C.POINTER(WxEnsNbhdResult), i32, i32, i32, vp, vp, vp, vp, vp]
    L.wx_ens_nbhd_max_radius.argtypes = []
    L.wx_ens_nbhd_max_radius.restype = i32
    L.wx_ensemble_gram.argtypes = [vp, C.POINTER(WxEnsGram), vp]
    L.wx_ens_gram_cells.argtypes = [C.POINTER(WxEnsGram), i32, i32, i32, vp, vp, vp]
    L.wx_ens_gram_max_members.argtypes = []
    L.wx_ens_gram_max_members.restype = i32
    _lib = L
    return L


def set_default_option(option: int, value: int):
    """wx_set_option(NULL, ...): the default of handles created afterwards (kernel set, dry kernel, row bands, exact-path capacity)."""
    rc = lib().wx_set_option(None, int(option), int(value))
    if rc != 0:
        raise ValueError(f"wx_set_option(NULL, {option}, {value}) -> {rc}")


# The C library reads no environment variable. The test-suite and the experiment scripts select the kernel set etc. per process
# through these variables, which THIS wrapper turns into wx_set_option defaults before it creates a handle.
_ENV_OPTIONS = (("WX_FUSED", 3, 1), ("WX_DRY_MARCH", 4, 1), ("WX_WET_BANDS", 5, 1), ("WX_WET_FIX_CAP", 6, 0))


def _apply_env_defaults():
    for name, opt, dflt in _ENV_OPTIONS:
        v = os.environ.get(name)
        set_default_option(opt, dflt if v is None else (min(int(v), 1) if opt in (3, 4) else int(v)))


class WxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libwxsim error {code}: {msg}")
        self.code = code


class Handle:
    """Thin RAII wrapper of a ``wx_sim*``."""

    def __init__(self, X: int, Y: int, n_droplets: int = 0, *, X_global: Optional[int] = None, x0: int = 0, halo: int = 0):
        L = lib()
        h = C.c_void_p()
        _apply_env_defaults()
        if X_global is None:
            rc = L.wx_create(X, Y, n_droplets, C.byref(h))
        else:
            rc = L.wx_create_slab(X_global, Y, x0, X, halo, n_droplets, C.byref(h))
        if rc != 0:
            raise WxError(rc, (L.wx_last_error(None) or b"").decode())
        self._h = h
        self.X_owned, self.Y, self.n_droplets, self.halo = X, Y, n_droplets, halo
        self.X = L.wx_local_width(h)
        self.generation = 0  # bumped whenever device pointers obtained earlier become invalid (tune_placement)
        self._stepped = False

    @classmethod
    def _borrowed(cls, ptr, X_owned: int, Y: int, halo: int, owner, n_droplets: int = 0) -> "Handle":
        """A slab of a Group: the group destroys it (``owner`` is kept alive as long as this wrapper is)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(ptr)
        self._owner = owner
        self.X_owned, self.Y, self.n_droplets, self.halo = X_owned, Y, n_droplets, halo
        self.X = lib().wx_local_width(self._h)
        self.generation = 0
        self._stepped = False
        return self

    def _chk(self, rc: int):
        if rc != 0:
            raise WxError(rc, (lib().wx_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_owner", None) is not None:  # a group's slab
            self._h = None
            return
        if getattr(self, "_h", None):
            lib().wx_destroy(self._h)  # (waits for a streamed frame in flight)
            self._h = None
            if getattr(self, "_pin", None) is not None:
                lib().wx_host_free(self._pin[0])
                self._pin = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----
    def upload(self, base, water, wall, drops=None):
        n = self.X * self.Y * 4
        base = np.ascontiguousarray(base, np.float32).reshape(-1)
        water = np.ascontiguousarray(water, np.float32).reshape(-1)
        wall = np.ascontiguousarray(wall, np.int8).reshape(-1)
        if not (base.size == water.size == wall.size == n):
            raise ValueError(f"grid arrays must hold {self.Y}x{self.X}x4 values")
        d = None
        if drops is not None and self.n_droplets > 0:
            drops = np.ascontiguousarray(drops, np.float32).reshape(-1)
            if drops.size != self.n_droplets * 5:
                raise ValueError("drops must hold n_droplets x 5 values")
            d = drops.ctypes.data
        self._chk(lib().wx_upload(self._h, base.ctypes.data, water.ctypes.data, wall.ctypes.data, d))

    def set_params(self, p: WxParams, initial_T=None, snd_T=None, snd_W=None, snd_Vel=None):
        arrs = []
        for a in (initial_T, snd_T, snd_W, snd_Vel):
            if a is None:
                arrs.append(None)
            else:
                a = np.ascontiguousarray(a, np.float32)
                if a.size < self.Y + 1:
                    raise ValueError("profile arrays need Y+1 entries")
                arrs.append(a)
        ptr = [None if a is None else a.ctypes.data for a in arrs]
        self._chk(lib().wx_set_params(self._h, C.byref(p), *ptr))

    OVERLAP_EDGES_FIRST, OVERLAP_EDGES_LAST = 1, 2

    def step(self, n: int = 1, overlap: int = 0):
        """n iterations; ``overlap`` (slab handles with a comm stream): OVERLAP_EDGES_FIRST -- edge strips of the last iteration
        first, so that the halo can be packed and sent while the interior computes; OVERLAP_EDGES_LAST -- interior strips of the
        first iteration first, the edge strips once the ghost columns have arrived (wx_step_overlap)."""
        if not self._stepped and n > 0:  # (the first step of a big whole-domain handle may move the planes: WX_OPT_PLACEMENT_SEARCH)
            self._stepped = True
            self.generation += 1
        if overlap:
            self._chk(lib().wx_step_overlap(self._h, int(n), int(overlap)))
        else:
            self._chk(lib().wx_step(self._h, int(n)))

    def sync(self):
        self._chk(lib().wx_sync(self._h))

    def copy_from(self, src: "Handle"):
        """wx_copy_state: this handle becomes a complete device-side clone of ``src`` (same X, Y and droplet count, same device; lone
        handles or ensemble members alike) -- every field, the droplet pool, iteration counter, parameters; the options stay this
        handle's own. Blocks like ``sync`` on both; device pointers of this handle obtained earlier dangle."""
        self.generation += 1
        self._chk(lib().wx_copy_state(self._h, src._h))
        self._stepped = self._stepped or src._stepped

    def tune_placement(self, tries: int = 6, iters_per_try: int = 30):
        """wx_tune_placement: try ``tries`` further device allocations for the handle's planes, keep the fastest; returns
        (ms per iteration of the first candidate, of the winner). The state is unchanged."""
        a, b = C.c_float(0), C.c_float(0)
        self.generation += 1  # (the planes move: every cached view of device memory -- device_ptr, devtools.field_tensor -- dangles)
        self._chk(lib().wx_tune_placement(self._h, int(tries), int(iters_per_try), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def water_free(self) -> bool:
        """Did the last upload find this handle's cells water-free (wx_water_free)?"""
        return bool(lib().wx_water_free(self._h))

    def slab_assert_water_free(self, agreed: bool):
        """The host's assertion that EVERY slab of the domain was uploaded water-free (wx_slab_assert_water_free)."""
        self._chk(lib().wx_slab_assert_water_free(self._h, 1 if agreed else 0))

    OPT_SPLAT_ORDER, OPT_CHECK_LAUNCHES, OPT_KERNEL_SET, OPT_DRY_KERNEL, OPT_ROW_BANDS, OPT_FIX_CAP, OPT_POOL_EXACT, OPT_EXCHANGE_OVERLAP, OPT_DRY_PAIRS = 1, 2, 3, 4, 5, 6, 7, 8, 10  # (9: retired, not reused)
    OPT_PLACEMENT_SEARCH = 12  # tries of the handle's one placement search, run inside the first step of big whole-domain handles (0: never)
    OPT_WATER0_ON_DEMAND = 11  # waterTexture_0 made when asked for (default 1) instead of stored by every frame's last iteration

    def set_option(self, option: int, value: int):
        """wx_set_option: OPT_SPLAT_ORDER 1 = deterministic particle splats (sorted, droplet-index order); OPT_CHECK_LAUNCHES 1 =
        synchronise and check after every kernel launch."""
        self._chk(lib().wx_set_option(self._h, int(option), int(value)))

    @property
    def iter(self) -> int:
        return lib().wx_get_iter(self._h)

    @iter.setter
    def iter(self, v: int):
        self._chk(lib().wx_set_iter(self._h, int(v)))

    # ---- readback ----
    def read_rect(self, field: str, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, *, int32: bool = False):
        w = self.X - x if w is None else w
        h = self.Y - y if h is None else h
        if field == "LIGHTNING":
            out = np.zeros(4, np.float32)
            self._chk(lib().wx_read_rect(self._h, 12, 0, 0, 1, 1, out.ctypes.data, DTYPE_F32))
            return out
        ch = FIELD_CHANNELS.get(field, 4)
        if field.startswith("WALL"):
            out = np.zeros((max(h, 0), max(w, 0), ch), np.int32 if int32 else np.int8)
            dt = DTYPE_I32 if int32 else DTYPE_I8
        elif field == "EMITTED":  # RGBA16F emittedLight, in its own format
            out = np.zeros((max(h, 0), max(w, 0), 4), np.float16)
            dt = DTYPE_F16
        else:
            out = np.zeros((max(h, 0), max(w, 0), ch), np.float32)
            dt = DTYPE_F32
        self._chk(lib().wx_read_rect(self._h, FIELD_IDS[field], x, y, w, h, out.ctypes.data, dt))
        return out

    def read_particles(self, first: int = 0, count: Optional[int] = None):
        count = self.n_droplets - first if count is None else count
        out = np.zeros((max(count, 0), 5), np.float32)
        self._chk(lib().wx_read_particles(self._h, first, count, out.ctypes.data))
        return out

    # ---- diagnostics (wx_diag: replaces the reference's commented-out conservation block app.js:6736-6762) ----
    def diagnostics(self) -> dict:
        """Exact sums, extremes, census and non-finite report of the owned columns, computed on the device (wx_diagnostics): the members
        of ``wx_diag`` by name, locations as global (x, y) or None. Changes nothing in the handle."""
        d = WxDiag()
        self._chk(lib().wx_diagnostics(self._h, C.byref(d)))
        return _diag_dict(d)

    def diagnostics_raw(self) -> bytes:
        """wx_diag_collect: the unrounded integers of this handle's owned columns, to be merged with other slabs' (diag_merge, diag_finish)."""
        r = WxDiagRaw()
        self._chk(lib().wx_diag_collect(self._h, C.byref(r)))
        return bytes(r)

    # ---- plumbing ----
    def set_stream(self, stream_ptr: int):
        self._chk(lib().wx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_comm_stream(self, stream_ptr: int):
        """Run wx_halo_pack / wx_halo_unpack on this stream (the one the host issues send / recv on), event-fenced against compute."""
        self._chk(lib().wx_set_comm_stream(self._h, C.c_void_p(stream_ptr)))

    def device_ptr(self, field: str) -> int:
        return lib().wx_device_ptr(self._h, FIELD_IDS[field])

    def halo_bytes(self) -> int:
        return lib().wx_halo_bytes(self._h)

    def halo_message_bytes(self) -> int:
        """What a halo message of the current period occupies at the front of a wx_halo_bytes buffer (the base texture alone between slabs
        of the agreed water-free dry stencil)."""
        return lib().wx_halo_message_bytes(self._h)

    def halo_pack(self, side: int, dev_ptr: int):
        self._chk(lib().wx_halo_pack(self._h, side, C.c_void_p(dev_ptr)))

    def halo_unpack(self, side: int, dev_ptr: int):
        self._chk(lib().wx_halo_unpack(self._h, side, C.c_void_p(dev_ptr)))

    def halo_pack_both(self, dev_left: int, dev_right: int):
        """Both sides in one launch (a second small launch would queue behind the marching kernel's thousands of workgroups)."""
        self._chk(lib().wx_halo_pack_both(self._h, C.c_void_p(dev_left), C.c_void_p(dev_right)))

    def halo_unpack_both(self, dev_left: int, dev_right: int):
        self._chk(lib().wx_halo_unpack_both(self._h, C.c_void_p(dev_left), C.c_void_p(dev_right)))

    # ---- display streaming (wx_stream_frame): one pinned buffer per Handle, re-used while the viewport size is unchanged
    STREAM_FIELDS = (("BASE_DISP", np.float32, 4), ("WATER_CUR", np.float32, 4), ("WALL_DISP", np.int8, 4), ("LIGHT_0", np.float32, 4),
                     ("CURL", np.float32, 1), ("PRECIP_FB", np.float32, 4), ("EMITTED", np.float16, 4))

    def stream_frame(self, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None):
        """Start the asynchronous copy of the display fields of a viewport; returns immediately."""
        w = self.X - x if w is None else w
        h = self.Y - y if h is None else h
        L = lib()
        nbytes = L.wx_stream_bytes(w, h)
        if getattr(self, "_pin", None) is None or self._pin[1] != nbytes:
            if getattr(self, "_pin", None) is not None:
                L.wx_host_free(self._pin[0])
            p = L.wx_host_alloc(nbytes)
            if not p:
                raise MemoryError(f"wx_host_alloc({nbytes})")
            self._pin = (p, nbytes)
        self._chk(L.wx_stream_frame(self._h, x, y, w, h, C.c_void_p(self._pin[0])))
        self._frame = (w, h)

    def stream_wait(self):
        """Wait for the frame started by stream_frame(); returns {field: array} views of the pinned buffer."""
        self._chk(lib().wx_stream_wait(self._h))
        w, h = self._frame
        raw = (C.c_char * self._pin[1]).from_address(self._pin[0])
        out, off = {}, 0
        for name, dt, ch in self.STREAM_FIELDS:
            n = w * h * ch
            out[name] = np.frombuffer(raw, dtype=dt, count=n, offset=off).reshape(h, w, ch)
            off += n * np.dtype(dt).itemsize
        return out

    def setup_columns(self, desc, drops=None):
        """Device-side initialiser from the 1-D descriptors of ``synth.terrain_columns`` (wx_setup_columns)."""
        want = {"wall_rows": (np.int32, self.X), "sea": (np.uint8, self.X), "veg_noise": (np.float64, self.X), "snow": (np.float32, self.X),
                "T_air": (np.float32, self.Y), "total_water": (np.float32, self.Y), "cloud_water": (np.float32, self.Y)}
        arrs = []
        for k, (dt, n) in want.items():
            a = np.ascontiguousarray(desc[k], dt)
            if a.shape != (n,):
                raise ValueError(f"setup_columns: {k} has shape {a.shape}, expected ({n},)")
            arrs.append(a)
        dp = None
        if drops is not None:
            drops = np.ascontiguousarray(drops, np.float32)
            if drops.shape != (self.n_droplets, 5):
                raise ValueError("setup_columns: drops must be (n_droplets, 5) float32")
            dp = drops.ctypes.data_as(C.c_void_p)
        self._chk(lib().wx_setup_columns(self._h, *[a.ctypes.data_as(C.c_void_p) for a in arrs], dp))

    def setup_terrain(self, sounding, seed: float = 0.5, height_mult: float = 0.3, snap: int = 2, sim_height: float = 12000.0, drops=None):
        """New simulation generated entirely on the device (wx_setup_terrain): ``sounding`` = the per-row arrays of
        ``synth.sounding_rows`` (or any dict with T_air / total_water / cloud_water), terrain from the setup shader's noise."""
        arrs = []
        for k in ("T_air", "total_water", "cloud_water"):
            a = np.ascontiguousarray(sounding[k], np.float32)
            if a.shape != (self.Y,):
                raise ValueError(f"setup_terrain: {k} has shape {a.shape}, expected ({self.Y},)")
            arrs.append(a)
        dp = None
        if drops is not None:
            drops = np.ascontiguousarray(drops, np.float32)
            if drops.shape != (self.n_droplets, 5):
                raise ValueError("setup_terrain: drops must be (n_droplets, 5) float32")
            dp = drops.ctypes.data_as(C.c_void_p)
        self._chk(lib().wx_setup_terrain(self._h, float(seed), float(height_mult), int(snap), float(sim_height), *[a.ctypes.data_as(C.c_void_p) for a in arrs], dp))

    def fastest_velocity(self) -> float:
        """Largest |velocity component| [cells / iteration] the exact path of the marching wet kernel saw since the last call (0: none >= 0.9)."""
        v = C.c_float(0)
        self._chk(lib().wx_fastest_velocity(self._h, C.byref(v)))
        return float(v.value)

    def placement_info(self):
        """(ms per iteration on the first allocations, on the kept ones) of the handle's placement search, or None if none has run."""
        a, b = C.c_float(0), C.c_float(0)
        return (float(a.value), float(b.value)) if lib().wx_placement_info(self._h, C.byref(a), C.byref(b)) == 1 else None

    def pair_stats(self):
        """(cells recomputed by the pair kernel's exact path, pairs repeated whole) since the last call; resets both; synchronises."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(lib().wx_pair_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- slabs exact at any speed (include/wxsim.h): the hosts of all slabs agree on a |vx| bound per exchange period ----
    def slab_vx_take(self) -> float:
        """Largest |vx| this slab has seen since the last take (0 below 0.5 cells / iteration); synchronises."""
        v = C.c_float(0)
        self._chk(lib().wx_slab_vx_take(self._h, C.byref(v)))
        return float(v.value)

    def slab_set_vx_bound(self, v_measured: float):
        """v_measured = the maximum over ALL slabs: sizes the coming exchange period (cone = 6 + floor(1.25 v + 0.25) once that reaches 1)."""
        self._chk(lib().wx_slab_set_vx_bound(self._h, C.c_float(float(v_measured))))

    @property
    def slab_cone(self) -> int:
        return int(lib().wx_slab_cone(self._h))

    @property
    def slab_period(self) -> int:
        return int(lib().wx_slab_period(self._h))

    def init_droplets(self, seed: int = 1):
        """initRainDrops() on the device (wx_init_droplets): a fresh all-inactive pool, a pure function of the seed."""
        self._chk(lib().wx_init_droplets(self._h, C.c_uint32(int(seed) & 0xFFFFFFFF)))

    # ---- particles on slabs (device pointers; see include/wxsim.h) ----
    def slab_set_rank(self, rank: int):
        self._chk(lib().wx_slab_set_rank(self._h, rank))

    def slab_period_begin(self):
        self._chk(lib().wx_slab_period_begin(self._h))

    def pool_event_bytes(self) -> int:
        return lib().wx_pool_event_bytes(self._h)

    def pool_edge_bytes(self) -> int:
        return lib().wx_pool_edge_bytes(self._h)

    def pool_events_pack(self, dev_buf: int):
        self._chk(lib().wx_pool_events_pack(self._h, C.c_void_p(dev_buf)))

    def pool_events_apply(self, dev_bufs: int, n_ranks: int, stride_bytes: int = 0):
        self._chk(lib().wx_pool_events_apply(self._h, C.c_void_p(dev_bufs), int(n_ranks), int(stride_bytes)))

    def pool_edges_pack(self, dev_left: int, dev_right: int, refresh_inactive: bool = False):
        self._chk(lib().wx_pool_edges_pack(self._h, C.c_void_p(dev_left), C.c_void_p(dev_right), 1 if refresh_inactive else 0))

    def pool_edges_apply(self, dev_buf: int):
        self._chk(lib().wx_pool_edges_apply(self._h, C.c_void_p(dev_buf)))

    def pool_flags(self) -> np.ndarray:
        """Per droplet: 0 tracked by another rank, 1 inactive, 2 active in this rank's owned columns, 3 ghost copy."""
        out = np.zeros(self.n_droplets, np.uint8)
        self._chk(lib().wx_pool_flags(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def lightning(self) -> np.ndarray:
        out = np.zeros(4, np.float32)
        self._chk(lib().wx_lightning_get(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_lightning(self, v):
        v = np.ascontiguousarray(v, np.float32)
        self._chk(lib().wx_lightning_set(self._h, v.ctypes.data_as(C.c_void_p)))

    # ---- the halo exchange inside the library (one rank per process; see include/wxsim.h) ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: 128 bytes that rank 0 hands to every other rank (any side channel: torch.distributed, a file, MPI)."""
        buf = C.create_string_buffer(128)
        rc = lib().wx_comm_unique_id(buf)
        if rc != 0:
            raise WxError(rc, (lib().wx_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != 128:
            raise ValueError("the unique id has 128 bytes")
        self._chk(lib().wx_comm_init(self._h, C.c_char_p(unique_id), int(rank), int(world)))

    def exchange(self):
        """Ring halo exchange over RCCL (pack, send / recv, unpack), enqueued on the handle's comm stream."""
        self._chk(lib().wx_exchange(self._h))

    def slab_step(self, n: int):
        """n iterations with an exchange every halo / 6 iterations, overlapped with compute (wx_slab_step)."""
        self._chk(lib().wx_slab_step(self._h, int(n)))

    def profile(self, enable: bool):
        self._chk(lib().wx_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        L = lib()
        n = L.wx_kernel_count()
        ms = (C.c_float * n)()
        cnt = (C.c_int * n)()
        self._chk(L.wx_profile_read(self._h, n, ms, cnt))
        return {L.wx_kernel_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(n) if cnt[k] > 0}


TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_LOCAL = 0, 1, 2


class Group:
    """N column slabs of one periodic domain in THIS process (wx_group_*): one handle per slab -- on N devices with RCCL between them,
    or several per device with device-to-device copies -- stepped together with the halo exchange inside the library."""

    def __init__(self, n_slabs: int, X_global: int, Y: int, halo: int = 42, devices=None, transport: int = TRANSPORT_AUTO, n_droplets: int = 0):
        L = lib()
        g = C.c_void_p()
        _apply_env_defaults()
        dev = None
        if devices is not None:
            dev = (C.c_int * n_slabs)(*[int(d) for d in devices])
        rc = L.wx_group_create(int(n_slabs), dev, int(X_global), int(Y), int(halo), int(n_droplets), int(transport), C.byref(g))
        if rc != 0:
            raise WxError(rc, (L.wx_group_last_error(None) or b"").decode())
        self._g = g
        self.n, self.X, self.Y = n_slabs, X_global, Y
        self.halo = halo if n_slabs > 1 else 0
        self.xo = X_global // n_slabs
        self.transport = L.wx_group_transport(g)
        self.n_droplets = n_droplets
        self.slabs = [Handle._borrowed(L.wx_group_slab(g, i), self.xo, Y, self.halo, self, n_droplets) for i in range(n_slabs)]

    def _chk(self, rc: int):
        if rc != 0:
            raise WxError(rc, (lib().wx_group_last_error(self._g) or b"").decode())

    def columns(self, i: int) -> np.ndarray:
        """Global column of every local column of slab i (owned + ghost columns, periodic)."""
        return (i * self.xo - self.halo + np.arange(self.xo + 2 * self.halo)) % self.X

    def upload(self, base, water, wall, drops=None):
        """Whole-domain arrays (Y, X, 4) cut into the slabs' local arrays; ``drops`` = the WHOLE droplet pool, handed to every slab."""
        for i, h in enumerate(self.slabs):
            idx = self.columns(i)
            h.upload(np.ascontiguousarray(base[:, idx]), np.ascontiguousarray(water[:, idx]), np.ascontiguousarray(wall[:, idx]), drops)
        self._chk(lib().wx_group_agree(self._g))

    def set_option(self, option: int, value: int):
        self._chk(lib().wx_group_set_option(self._g, int(option), int(value)))

    def exchange(self):
        """An exchange now (wx_group_exchange): afterwards every active droplet is owned by exactly one slab."""
        self._chk(lib().wx_group_exchange(self._g))

    def particles(self) -> np.ndarray:
        """The whole droplet pool assembled from the slabs (call right after an exchange: inside a period a droplet near an edge is held
        by two slabs): an active droplet's record comes from the slab that owns it, an inactive one's is the same everywhere."""
        d = [h.read_particles() for h in self.slabs]
        if self.n == 1:
            return d[0]
        f = np.stack([h.pool_flags() for h in self.slabs])
        if ((f == 2).sum(0) > 1).any():
            raise RuntimeError("Group.particles: a droplet is owned by two slabs (call exchange() first)")
        out = d[0].copy()
        for k in range(self.n):
            out[f[k] == 2] = d[k][f[k] == 2]
        return out

    def set_params(self, p: WxParams, initial_T=None, snd_T=None, snd_W=None, snd_Vel=None):
        for h in self.slabs:
            h.set_params(p, initial_T, snd_T, snd_W, snd_Vel)

    def step(self, n: int = 1):
        self._chk(lib().wx_group_step(self._g, int(n)))

    def sync(self):
        self._chk(lib().wx_group_sync(self._g))

    def diagnostics(self) -> dict:
        """wx_group_diagnostics: every slab's pass on its own device, merged: bit for bit the numbers of the undecomposed domain. With
        droplets: call it where an exchange has just been applied (after ``exchange()``, or after a ``step`` whose iteration count ends
        on a multiple of the slabs' period) -- in between a droplet that crossed a slab edge may be counted by neither or both slabs."""
        d = WxDiag()
        self._chk(lib().wx_group_diagnostics(self._g, C.byref(d)))
        return _diag_dict(d)

    def read(self, field: str) -> np.ndarray:
        """The whole domain's field assembled from the slabs' owned columns."""
        return np.concatenate([h.read_rect(field, self.halo, 0, self.xo, self.Y) for h in self.slabs], axis=1)

    def close(self):
        if getattr(self, "_g", None):
            for h in self.slabs:
                h._h = None
            lib().wx_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ensemble:
    """B independent whole-domain simulations of one size (wx_ensemble_*): ``members`` are borrowed ``Handle``s -- upload, set_params,
    set_option, read_rect, read_particles ... exactly as on any handle --, ``step`` advances all of them in one marching launch per
    iteration, and the ``n_droplets`` droplets of each in one set of particle launches."""

    def __init__(self, n_members: int, X: int, Y: int, n_droplets: int = 0):
        L = lib()
        e = C.c_void_p()
        _apply_env_defaults()
        if n_droplets:
            rc = L.wx_ensemble_create_droplets(int(n_members), int(X), int(Y), int(n_droplets), C.byref(e))
        else:
            rc = L.wx_ensemble_create(int(n_members), int(X), int(Y), C.byref(e))
        if rc != 0:
            raise WxError(rc, (L.wx_ensemble_last_error(None) or b"").decode())
        self._e = e
        self.n, self.X, self.Y = L.wx_ensemble_count(e), X, Y
        self.n_droplets = int(n_droplets)
        self.members = [Handle._borrowed(L.wx_ensemble_member(e, i), X, Y, 0, self, self.n_droplets) for i in range(self.n)]

    def _chk(self, rc: int):
        if rc != 0:
            raise WxError(rc, (lib().wx_ensemble_last_error(self._e) or b"").decode())

    def __len__(self):
        return self.n

    def __getitem__(self, i: int) -> Handle:
        return self.members[i]

    def step(self, n: int = 1):
        self._chk(lib().wx_ensemble_step(self._e, int(n)))
        for h in self.members:
            h._stepped = True

    def sync(self):
        self._chk(lib().wx_ensemble_sync(self._e))

    def diagnostics(self) -> list:
        """wx_ensemble_diagnostics: one dict per member (what ``Handle.diagnostics`` returns for it)."""
        d = (WxDiag * self.n)()
        self._chk(lib().wx_ensemble_diagnostics(self._e, d))
        return [_diag_dict(d[i]) for i in range(self.n)]

    def stats(self) -> dict:
        """wx_ensemble_stats: member-iterations that shared a launch / ran their own path, and marching launches issued, so far."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(lib().wx_ensemble_stats(self._e, C.byref(a), C.byref(b), C.byref(c)))
        return {"member_iters_batched": a.value, "member_iters_solo": b.value, "march_launches": c.value}

    def particle_stats(self) -> dict:
        """wx_ensemble_particle_stats: member-iterations whose particle pass shared its launches, and particle launches issued, so far."""
        a, b = C.c_int64(), C.c_int64()
        self._chk(lib().wx_ensemble_particle_stats(self._e, C.byref(a), C.byref(b)))
        return {"member_iters_particles_batched": a.value, "particle_launches": b.value}

    def statistics(self, field: str, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, *, members=None,
                   threshold=(0, 0, 0, 0), want=ENS_STAT_ALL) -> dict:
        """wx_ensemble_statistics: per cell of the rectangle, over the selected members (None: all; member indices; or one boolean
        per member), the planes named in ``want`` -- mean, variance, min, max (float32), argmin, argmax, count, n_above (int32), all
        (h, w, 4), and n_wall (h, w). ``field``: BASE_CUR or WATER_CUR. Computed on the device in one launch; blocks like ``sync``."""
        w = self.X - x if w is None else w
        h = self.Y - y if h is None else h
        st, planes = _ens_stat_struct((max(h, 0), max(w, 0)), threshold, want)
        mask = _member_mask(self.n, members)
        self._chk(lib().wx_ensemble_statistics(self._e, FIELD_IDS[field], int(x), int(y), int(w), int(h), None if mask is None else mask.ctypes.data, C.byref(st)))
        return planes

    QUANT_STAGED_MEMBERS = 64  # wx_ens_quant_staged_members(): the largest selection the LDS path of ``quantiles`` takes

    def quantiles(self, field: str, p, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, *, members=None,
                  interp="linear", rank_of=None, want=None) -> dict:
        """wx_ensemble_quantiles: per cell of the rectangle, over the selected members, the quantiles ``p`` (up to 8 numbers in [0, 1];
        ``interp`` "linear", "lower" or "higher") as ``q`` (n_q, h, w, 4) float32, ``count`` (h, w, 4) and ``n_wall`` (h, w); with
        ``rank_of`` = r, a member outside the selection (``members`` None: everybody but r), also ``n_below`` / ``n_equal`` (h, w, 4):
        how many entered values lie below / equal member r's (-1 where r's cell is wall or its value not finite). ``want``: the planes
        to compute (default: all of these). ``field``: BASE_CUR or WATER_CUR. One launch on the device; blocks like ``sync``."""
        w = self.X - x if w is None else w
        h = self.Y - y if h is None else h
        st, planes = _ens_quant_struct((max(h, 0), max(w, 0)), p, interp, rank_of, want)
        mask = _quant_mask(self.n, members, rank_of)
        self._chk(lib().wx_ensemble_quantiles(self._e, FIELD_IDS[field], int(x), int(y), int(w), int(h), None if mask is None else mask.ctypes.data, C.byref(st)))
        return planes

    SCORE_MAX_MEMBERS = 64  # wx_ens_score_max_members(): the largest selection ``scores`` takes

    def scores(self, field: str, truth: "Handle", x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, *, members=None,
               want=()) -> dict:
        """wx_ensemble_scores: the selected members (None: all but ``truth`` if it is a member of this ensemble) scored against the
        ``truth`` handle -- a lone ``Handle``, an unselected member, a member of another ensemble -- over the rectangle of ``field``
        (BASE_CUR or WATER_CUR). Returns the entries of wx_ens_score (``ens_score_cells``): exact domain sums of error, absolute
        error, squared error, variance and CRPS per channel, the counts, the rank histograms, and the maps named in ``want`` (error,
        variance, crps: (h, w, 4)). One launch on the device, a few hundred bytes back; blocks like ``sync``."""
        w = self.X - x if w is None else w
        h = self.Y - y if h is None else h
        st, maps = _ens_score_struct((max(h, 0), max(w, 0)), want)
        mask = _member_mask(self.n, members)
        if members is None:
            inside = [i for i, m in enumerate(self.members) if m is truth or (m._h.value == truth._h.value)]
            if inside:
                mask = np.ones(self.n, np.uint8)
                mask[inside] = 0
        self._chk(lib().wx_ensemble_scores(self._e, truth._h, FIELD_IDS[field], int(x), int(y), int(w), int(h), None if mask is None else mask.ctypes.data, C.byref(st)))
        return _ens_score_dict(st, maps)

    def broadcast(self, src: int, members=None):
        """wx_ensemble_broadcast: every selected member (None: all others) becomes a device-side clone of member ``src``
        (``Handle.copy_from``); one wait at the end."""
        mask = _member_mask(self.n, members)
        for i, h in enumerate(self.members):
            if i != int(src) and (mask is None or mask[i]):
                h.generation += 1
        self._chk(lib().wx_ensemble_broadcast(self._e, int(src), None if mask is None else mask.ctypes.data))

    def perturb(self, field: str, amplitude, *, mode="add", scale: int = 1, seed: int = 0, wrap_x: bool = False, rect=None, members=None, lo=None, hi=None):
        """wx_ensemble_perturb: smooth noise r in [-1, 1) -- a function of (seed, member index, channel, cell), bilinear on a lattice of
        ``scale`` cells -- added to (``mode`` "add": v + a r) or multiplied into ("mul": v (1 + a r)) ``field`` (BASE_CUR or WATER_CUR)
        of the selected members inside ``rect`` = (x, y, w, h) (None: the whole grid), in one launch. ``amplitude``, ``lo``, ``hi``: one
        value or one per channel (amplitude 0: channel untouched; lo / hi None: no clamp). Wall cells and non-finite values are left
        alone. Blocks like ``statistics``."""
        rect = (0, 0, self.X, self.Y) if rect is None else rect
        p = _perturb_struct(field, amplitude, mode, scale, seed, wrap_x, rect, lo, hi)
        mask = _member_mask(self.n, members)
        self._chk(lib().wx_ensemble_perturb(self._e, C.byref(p), None if mask is None else mask.ctypes.data))

    def assimilate(self, observations, *, loc=(0.0, 0.0), rect=None, members=None, wrap_x=False, gain_base=(0, 0, 0, 1), gain_water=0.0,
                   lo_base=None, hi_base=None, lo_water=None, hi_water=None) -> list:
        """wx_ensemble_assimilate: the selected members (at least two) pulled towards point observations -- ``(field, x, y, channel,
        value, error_var)`` tuples, taken in order -- by a serial ensemble square-root filter, on the device, in three launches at most.
        ``loc`` = (half-width in x, in y) of the Gaspari-Cohn localization in cells (0: none along that axis), ``rect`` = (x, y, w, h) the
        cells that may change (None: the whole grid), ``gain_base`` / ``gain_water``: one value or one per channel of the two state
        fields (0: untouched, 1: the full update; default: temperature only), ``lo_*`` / ``hi_*``: clamps (None: none). Returns one dict
        per observation (applied, prior_mean, prior_var, innovation, alpha). Blocks like ``perturb``."""
        rect = (0, 0, self.X, self.Y) if rect is None else rect
        a = _assim_struct(rect, loc, wrap_x, gain_base, gain_water, lo_base, hi_base, lo_water, hi_water)
        obs, res = _obs_array(observations), (WxEnsObsResult * max(len(observations), 1))()
        mask = _member_mask(self.n, members)
        self._chk(lib().wx_ensemble_assimilate(self._e, C.byref(a), len(observations), obs, res, None if mask is None else mask.ctypes.data))
        return _obs_results(res, len(observations))

    def save_prior(self, field: str, rect=None, members=None):
        """wx_ensemble_prior_save: a device-side snapshot of ``rect`` = (x, y, w, h) (None: the whole grid) of ``field`` (BASE_CUR or
        WATER_CUR) of the selected members -- what ``inflate`` in the modes "rtps" and "rtpp" relaxes to. One slot per field: the next
        save replaces it, ``drop_prior`` frees it (n x w x h x 16 bytes of device memory). One launch; blocks like ``statistics``."""
        x, y, w, h = (0, 0, self.X, self.Y) if rect is None else rect
        mask = _member_mask(self.n, members)
        self._chk(lib().wx_ensemble_prior_save(self._e, int(FIELD_IDS.get(field, field)), int(x), int(y), int(w), int(h), None if mask is None else mask.ctypes.data))

    def drop_prior(self, field: str):
        """wx_ensemble_prior_drop: frees the snapshot of ``field`` (nothing happens if there is none)."""
        self._chk(lib().wx_ensemble_prior_drop(self._e, int(FIELD_IDS.get(field, field))))

    def inflate(self, field: str, coef, *, mode="const", rect=None, members=None, lambda_bounds=None, lo=None, hi=None, want_lambda=False):
        """wx_ensemble_inflate: the spread of the selected members (at least two) of ``field`` (BASE_CUR or WATER_CUR) inside ``rect`` =
        (x, y, w, h) (None: the whole grid) put back, in one launch. ``mode`` "const": the deviations from the ensemble mean times
        ``coef`` (lambda, one value or one per channel; 1: channel untouched). "rtps": relaxation to prior spread, lambda = 1 + alpha
        (sb - sa) / sa per cell with ``coef`` = alpha (0: untouched) and ``lambda_bounds`` = (lowest, highest) lambda (None: none).
        "rtpp": relaxation to prior perturbations, (1 - alpha) x' + alpha xb'. The two relaxation modes read the snapshot that
        ``save_prior`` took of the same field and members. ``lo`` / ``hi``: clamps (None: none). Cells that are a wall or hold a
        non-finite value in any selected member are left alone. With ``want_lambda`` ("const", "rtps") the (h, w, 4) map of the lambda
        applied comes back, NaN where a channel was left alone. Blocks like ``perturb``."""
        rect = (0, 0, self.X, self.Y) if rect is None else rect
        lam = np.zeros((max(int(rect[3]), 0), max(int(rect[2]), 0), 4), np.float32) if want_lambda else None
        p = _inflate_struct(field, coef, mode, rect, lambda_bounds, lo, hi, lam)
        mask = _member_mask(self.n, members)
        self._chk(lib().wx_ensemble_inflate(self._e, C.byref(p), None if mask is None else mask.ctypes.data))
        return lam

    def covariance(self, field: str, predictors, *, source="current", rect=None, members=None, want=COV_PLANES) -> dict:
        """wx_ensemble_covariance: for every cell and channel of ``rect`` = (x, y, w, h) (None: the whole grid) of ``field`` (BASE_CUR
        or WATER_CUR) the sample covariance, over the selected members (at least two), between the members' values and up to 8 scalar
        ``predictors`` -- ``(field name, x, y, channel)``: the members' own current value at a point; or one number per member (by
        member index): a forecast metric --, all in one pass over the members. ``source`` "current": the field as it is now; "prior": the
        snapshot ``save_prior`` took of it. Returns the planes named in ``want`` -- ``cov``, ``corr`` (clamped to [-1, 1]), ``slope``
        (cov / var of the cell: the ensemble sensitivity dJ/dx): (n_pred, h, w, 4) float32; ``variance``: (h, w, 4) -- NaN where a cell
        is a wall or holds a non-finite value in any selected member, and ``results``: one dict per predictor (valid, mean, variance).
        Changes nothing; two launches; blocks like ``statistics``."""
        rect = (0, 0, self.X, self.Y) if rect is None else rect
        preds, keep = _cov_predictors(predictors, self.n)
        c, planes = _cov_struct(field, source, rect, len(predictors), want)
        res = (WxEnsCovResult * max(len(predictors), 1))()
        mask = _member_mask(self.n, members)
        self._chk(lib().wx_ensemble_covariance(self._e, C.byref(c), preds, res, None if mask is None else mask.ctypes.data))
        planes["results"] = _cov_results(res, len(predictors))
        del keep
        return planes

    def gram(self, field: str, rect=None, members=None, center="mean") -> dict:
        """wx_ensemble_gram: the selected members (at most 64) seen in member space -- per channel the n x n matrix of the exact sums,
        over the cells of ``rect`` = (x, y, w, h) (None: the whole grid) of ``field`` (BASE_CUR or WATER_CUR), of the float terms
        (d_a d_b) of the members' deviations from their mean (``center`` "mean"; at least two members) or of their raw values
        ("none"). A cell-channel enters if the cell is an air cell and the value finite in every selected member and no squared
        deviation overflows a float. Returns ``gram`` (4, n, n) float64, exactly symmetric, the members in ascending index;
        ``n_entered`` / ``n_excluded`` / ``n_overflow`` (4 each, adding up to w * h) and ``members``. Changes nothing; two launches;
        blocks like ``statistics``."""
        rect = (0, 0, self.X, self.Y) if rect is None else rect
        mask = _member_mask(self.n, members)
        sel = _selected(self.n, members)
        g, gram = _gram_struct(field, center, rect, len(sel))
        self._chk(lib().wx_ensemble_gram(self._e, C.byref(g), None if mask is None else mask.ctypes.data))
        return _gram_dict(g, gram, sel)

    def neighbourhood(self, field: str, channel: int, threshold: float, scales, truth: Optional["Handle"] = None, *, above: bool = True, rect=None,
                      members=None, wrap_x: bool = False, want=("nep",)) -> dict:
        """wx_ensemble_neighbourhood: the event "channel ``channel`` of ``field`` (BASE_CUR or WATER_CUR) above (``above`` False:
        below) ``threshold``" counted over the selected members (None: all but ``truth`` if it is a member of this ensemble; any
        number) and summed over boxes of the ``scales`` -- up to 8 (rx, ry) half-widths, 0 .. 32; a single number r is (r, r) -- around
        every cell of ``rect`` = (x, y, w, h) (None: the whole grid); windows reach outside the rectangle, around the seam with
        ``wrap_x``. Against ``truth`` -- a lone ``Handle``, an unselected member, a member of another ensemble -- the raw material of
        the fractions skill score per scale: n_scored, n_unscored, the exact sums sum_d2, sum_f2, sum_o2, and the point totals ev_f,
        n_f, ev_o, n_o. The maps named in ``want``: ``nep`` (n_scales, h, w), the neighbourhood ensemble probability, and
        ``obs_fraction``, the truth's fraction (NaN where a window holds no counted cell). ``truth`` None: nep and ev_f / n_f alone.
        The members are read once, two launches; changes nothing; blocks like ``sync``."""
        rect = (0, 0, self.X, self.Y) if rect is None else rect
        a, maps = _ens_nbhd_struct(field, channel, threshold, scales, above, wrap_x, rect, want)
        res = WxEnsNbhdResult()
        mask = _member_mask(self.n, members)
        if members is None and truth is not None:
            inside = [i for i, m in enumerate(self.members) if m is truth or (m._h.value == truth._h.value)]
            if inside:
                mask = np.ones(self.n, np.uint8)
                mask[inside] = 0
        self._chk(lib().wx_ensemble_neighbourhood(self._e, None if truth is None else truth._h, C.byref(a), None if mask is None else mask.ctypes.data, C.byref(res)))
        return _ens_nbhd_dict(a, res, maps)

    def close(self):
        if getattr(self, "_e", None):
            for h in self.members:
                h._h = None
            lib().wx_ensemble_destroy(self._e)
            self._e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
