#!/usr/bin/env python3
"""Times an ensemble (wx_ensemble_step) against what a host does without one: B handles from wx_create stepped round-robin in frames
of 10 iterations in one process. Prints ONE JSON line.

    python tools/ensemble_bench.py --mode ensemble                        # this checkout's ensemble, the three shapes
    python tools/ensemble_bench.py --mode handles --root ../parent        # the baseline, run from a checkout of the parent commit
    python tools/ensemble_bench.py --mode ensemble --shapes 100x100x1,100x100x8,100x100x64     # how the time grows with B

Shapes are XxYxB. 100 x 100 runs the reference's own save (tests/golden/save100raw.npz), the other sizes the setup-pass terrain; every
member gets a moving fluid of its own (devtools.seed_flow, seed = member index) -- as bench.py seeds its `configs`. Before every timed
region the chip is conditioned with untimed frames for a quarter of a second (bench.py: condition_clocks); a region is at least
--steps iterations of every member; --repeats regions are timed and all of them reported (compare the SLOWEST of each side).
The roofline fraction is 104 B / cell-step against bench.py's HBM_PEAK_GBS = 8000 GB/s (--peak-gbs).
--droplets N: every member carries N droplets (synth.init_rain_drops, seed = member index), enablePrecipitation = 1 and a cloud deck
(synth.add_cloud_deck) so that droplets spawn, grow and fall -- in both modes; the ensemble's record gains `particle_stats`. The default 0
is the droplet-free run.
--statistics FIELD (BASE_CUR or WATER_CUR; --mode ensemble): instead of the stepping time, what ONE wx_ensemble_statistics call over the
whole grid costs (all nine planes, host to host: the call blocks) against the route it replaces -- B read_rect calls of the field and B of
WALL_CUR plus the same arithmetic in numpy, member by member in member order as include/wxsim.h defines it -- after --frame iterations;
--repeats calls of each, the slowest and the median (of the device call also the fastest: slowest - fastest is the run's own noise figure)
reported under the shape's "statistics" key, with the kernel's own time (wx_profile
on member 0) and the bytes it reads per second (members x 20 B per cell and pass, two passes).
--quantiles FIELD (BASE_CUR or WATER_CUR; --mode ensemble): what ONE wx_ensemble_quantiles call over the whole grid costs (p = 0.1, 0.5,
0.9, linear, with count and n_wall; host to host) against the route it replaces -- B read_rect pairs, np.sort along the member axis
and the definition's arithmetic in numpy -- after --frame iterations, --repeats calls of each; under the shape's "quantiles" key with
the kernel's own time (wx_profile on member 0) and, from the same run, the time of the ensemble_statistics kernel with the variance
wanted (two passes over the members). Without --shapes: the two shapes the statistics were measured at and one on the streaming path
(more members than wx_ens_quant_staged_members()): 100x100x64, 2500x300x8, 100x100x96.
--scores FIELD (BASE_CUR or WATER_CUR; --mode ensemble): what ONE wx_ensemble_scores call over the whole grid costs (B members scored
against a truth that is member B of an ensemble of B + 1; no maps: a few hundred bytes come back; host to host) against the route it
replaces -- wx_ensemble_statistics for mean and variance, wx_ensemble_quantiles with rank_of for n_below / n_equal, read_rect of the
truth, and for the CRPS, which no existing call gives, B read_rect calls, np.sort along the member axis and the weighted sums in numpy
-- after --frame iterations, --repeats calls of each; under the shape's "scores" key with the kernel's own time (wx_profile on member 0)
and, from the same run, the quantile kernel's. Without --shapes: 100x100x64 and 2500x300x8.
--spawn (--mode ensemble): B members made from ONE stepped state (a lone handle after --frame x 5 iterations), timed two ways, host to
host, --repeats times each: route A = wx_copy_state into member 0 + wx_ensemble_broadcast + ONE wx_ensemble_perturb (temperature, lattice
pitch 8); route B = what a host did before -- B wx_upload calls of host arrays (the state read back once, untimed; per member numpy noise
on the temperature of the air cells, timed). Route B does NOT make the same ensemble: an upload cannot carry the light textures, curl,
feedback textures, lightning state and `even`, so its members are not the stepped simulation (the record says so: "route_b_carries_the_
state": false). The shape's "spawn" key also holds the perturbation kernel's own time (wx_profile on member 0) against its 36 B per
member-cell at --peak-gbs.
--assimilate FIELD (BASE_CUR: temperature observations; WATER_CUR: channel 0; --mode ensemble): what ONE wx_ensemble_assimilate call
with --observations N point observations over the whole grid costs (localization half-widths 20 x 10 cells, all four channels of FIELD
updated; host to host: the call blocks), against N calls of one observation each, and against the only host route that exists -- B
read_rect triples (base, water, wall), wx_ens_assim_cells on the host, B wx_upload calls. THE UPLOADS LOSE THE STEPPED STATE (light, curl,
the feedback textures, the lightning state): the record says so. The shape's "assimilate" key also holds the two kernels' own times
(wx_profile on member 0) next to the bytes the update kernel moves at most: 3 x 20 B read + 16 B written per member-cell and observation
whose weight there is not 0.
--inflate FIELD (BASE_CUR or WATER_CUR; --mode ensemble): what ONE wx_ensemble_inflate call over the whole grid costs per mode (CONST
lambda 1.1; RTPS alpha 0.5; RTPP alpha 0.5; all four channels; host to host: the call blocks), and one wx_ensemble_prior_save, against
the only host route that exists -- B read_rect pairs (field, wall) and wx_ens_inflate_cells on the host; THE WAY BACK WOULD BE B
wx_upload CALLS, which lose the stepped state (light, curl, the feedback textures, the lightning state) and are not timed: the record
says so. The shape's "inflate" key also holds the kernels' own times (wx_profile on member 0) against the bytes per member-cell the
walks request when every cell is updated -- CONST 52, RTPS 100, RTPP 84, the snapshot 32 -- and against what crosses the memory interface
if every re-read of a walk is served on the chip -- 36, 52, 52 --, both at --peak-gbs. Without
--shapes: 100x100x64 and 2500x300x8.
--covariance FIELD (BASE_CUR or WATER_CUR; --mode ensemble): what ONE wx_ensemble_covariance call over the whole grid costs with 1 and
with 8 point predictors (all four planes wanted; host to host: the call blocks), 8 calls of one predictor next to the one call of 8,
against B read_rect pairs (field, wall) plus the same arithmetic in numpy (float64, vectorised over the cells), and against the
statistics kernel (mean and variance wanted) of the same run, which reads the same member bytes. The shape's "covariance" key holds
the kernels' own times (wx_profile on member 0) and the fraction of --peak-gbs against 20 B + 16 B per member-cell plus the planes
written. Without --shapes: 100x100x64 and 2500x300x8.
--share K (debug build of the library only): the segment-height sweep -- every member's launch shape as for an ensemble of K members."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["ensemble", "handles"], default="ensemble")
    ap.add_argument("--root", default=ROOT, help="checkout to load the package and the library from (the parent commit for the baseline)")
    ap.add_argument("--shapes", default=None, help="XxYxB,... (default 100x100x64,2500x300x8,16000x500x2; with --quantiles 100x100x64,2500x300x8,100x100x96)")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--frame", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--flow", type=float, default=0.2)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="what the roofline fraction is quoted against [GB/s]: bench.py's HBM_PEAK_GBS")
    ap.add_argument("--droplets", type=int, default=0, help="droplets per member (0: none, precipitation off)")
    ap.add_argument("--statistics", default="", metavar="FIELD", help="time one statistics call over the whole grid against B read_rect calls + numpy (BASE_CUR or WATER_CUR)")
    ap.add_argument("--quantiles", default="", metavar="FIELD", help="time one quantile call over the whole grid against B read_rect calls + np.sort (BASE_CUR or WATER_CUR)")
    ap.add_argument("--scores", default="", metavar="FIELD", help="time one score call (B members against member B of B + 1) against statistics + quantiles + read_rect + numpy (BASE_CUR or WATER_CUR)")
    ap.add_argument("--assimilate", default="", metavar="FIELD", help="time one assimilation call of --observations point observations against N calls of one and against read_rect + host function + uploads (BASE_CUR or WATER_CUR)")
    ap.add_argument("--inflate", default="", metavar="FIELD", help="time one inflation call per mode over the whole grid against read_rect + the host function (BASE_CUR or WATER_CUR)")
    ap.add_argument("--covariance", default="", metavar="FIELD", help="time one covariance call with 1 and with 8 point predictors over the whole grid against read_rect + numpy and the statistics kernel (BASE_CUR or WATER_CUR)")
    ap.add_argument("--neighbourhood", default="", metavar="FIELD", help="time one neighbourhood call (B members against member B of B + 1, five scales up to (16, 8), channel 1) against statistics planes + read_rect of the truth + numpy summed-area tables (BASE_CUR or WATER_CUR)")
    ap.add_argument("--gram", default="", metavar="FIELD", help="time one Gram-matrix call over the whole grid against B read_rect calls + numpy and next to the statistics kernel (BASE_CUR or WATER_CUR)")
    ap.add_argument("--observations", type=int, default=40, help="observations per call with --assimilate (1 .. 256)")
    ap.add_argument("--spawn", action="store_true", help="time B members made from one stepped state: device-side broadcast + perturb against B uploads")
    ap.add_argument("--share", type=int, default=0, help="segment-height sweep: the members' launch shapes as for an ensemble of this many members "
                    "(1 = the lone handle's shape; 0 = the shipped rule, B). Needs the debug build: make -C csrc debug, WXSIM_LIB=.../variants/libwxsim_debug.so")
    a = ap.parse_args()
    if a.shapes is None:
        a.shapes = "100x100x64,2500x300x8,2500x300x24" if a.gram else "100x100x64,2500x300x8" if a.scores or a.inflate or a.covariance or a.neighbourhood else "100x100x64,2500x300x8,100x100x96" if a.quantiles else "100x100x8,100x100x64,2500x300x8" if a.assimilate else "100x100x64,2500x300x8,16000x500x2"
    return a


def make_members(pkg, X, Y, B, make, flow=0.2, droplets=0):
    """`make(i)` -> a handle of X x Y (with `droplets` droplets); uploads the scene, sets the parameters, seeds member i's own flow."""
    import numpy as np
    from weather_sandbox_amd import devtools
    P = pkg.params
    hs = []
    if (X, Y) == (100, 100):
        g = np.load(os.path.join(ROOT, "tests", "golden", "save100raw.npz"))
        u = json.loads(str(g["uniforms_json"]))
        u["initial_T"] = g["initial_T"]
        for k in ("userInputValues", "userInputMove", "airplaneValues"):
            u[k] = tuple(u[k])
        u = dict(u, quad_scale=0, enablePrecipitation=0)
        base, water, wall = g["in_base"], g["in_water"].copy(), g["in_wall"]
    else:
        gui = P.merge_settings(None)
        gui["sunAngle"] = 50.0
        u = P.uniforms_from_gui(gui, Y, quad_scale=0)
        u["enablePrecipitation"] = 0
        if droplets:
            base, water, wall = pkg.synth.terrain_grid(X, Y)
        else:
            cols = pkg.synth.terrain_columns(X, Y)
    if droplets:
        u["enablePrecipitation"] = 1
        pkg.synth.add_cloud_deck(water, wall)
    for i in range(B):
        h = make(i)
        if droplets:
            h.upload(base, water, wall, pkg.synth.init_rain_drops(droplets, seed=7 + i))
        elif (X, Y) == (100, 100):
            h.upload(base, water, wall)
        else:
            h.setup_columns(cols)
        h.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
        devtools.seed_flow(h, flow, seed=1 + i)
        hs.append(h)
    return hs


def numpy_statistics(fields, walls, threshold):
    """The per-cell function of include/wxsim.h in numpy: members in member order, vectorised over the cells (what a host does today)."""
    import numpy as np
    shape = fields[0].shape
    thr = np.asarray(threshold, np.float32)
    S, n, above = np.zeros(shape), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    n_wall = np.zeros(shape[:-1], np.int32)
    mn, mx = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    amn, amx = np.full(shape, -1, np.int32), np.full(shape, -1, np.int32)
    takes = []
    with np.errstate(all="ignore"):
        for i, (v, wl) in enumerate(zip(fields, walls)):
            is_wall = wl[..., 1] == 0
            n_wall += is_wall
            take = ~is_wall[..., None] & np.isfinite(v)
            takes.append(take)
            S = np.where(take, S + v.astype(np.float64), S)
            n += take
            lo, hi = take & (v < mn), take & (v > mx)
            mn, amn = np.where(lo, v, mn), np.where(lo, np.int32(i), amn)
            mx, amx = np.where(hi, v, mx), np.where(hi, np.int32(i), amx)
            above += take & (v > thr)
        m = np.where(n > 0, S / n, np.nan)
        Q = np.zeros(shape)
        for v, take in zip(fields, takes):
            d = v.astype(np.float64) - m
            Q = np.where(take, Q + d * d, Q)
        none = n == 0
        return {"mean": m.astype(np.float32), "variance": np.where(none, np.nan, Q / n).astype(np.float32),
                "min": np.where(none, np.float32(np.nan), np.where(mn == 0, np.float32(0), mn)), "max": np.where(none, np.float32(np.nan), np.where(mx == 0, np.float32(0), mx)),
                "argmin": amn, "argmax": amx, "count": n, "n_above": above, "n_wall": n_wall}


def time_statistics(a, ens, X, Y, B):
    import statistics
    import numpy as np
    field, thr = a.statistics, (0.0, 0.0, 0.0, 0.0)

    def device():
        return ens.statistics(field, threshold=thr)

    def reads():
        return [m.read_rect(field) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]

    def host():
        return numpy_statistics(*reads(), thr)

    ens.step(a.frame)
    ens.sync()
    got, want = device(), host()
    differ = [k for k in want if not np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f")]
    if differ:  # two routes that disagree are not two timings of one thing
        sys.exit("--statistics %s %dx%dx%d: wx_ensemble_statistics and the read_rect route disagree in %s" % (field, X, Y, B, ", ".join(differ)))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        device()
    ens[0].profile(True)
    t_dev, t_read, t_host = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        device()
        t_dev.append(time.perf_counter() - t0)
    kernel_ms, launches = ens[0].profile_read().get("ensemble_statistics", (0.0, 0))
    ens[0].profile(False)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = reads()
        t1 = time.perf_counter()
        numpy_statistics(*r, thr)
        t_read.append(t1 - t0)
        t_host.append(time.perf_counter() - t0)
    kernel_us = 1e3 * kernel_ms / max(launches, 1)
    ms = lambda t: round(1e3 * t, 3)
    return {"field": field, "members": B, "calls": a.repeats, "same_numbers": True,
            "statistics_call_ms": {"slowest": ms(max(t_dev)), "median": ms(statistics.median(t_dev)), "fastest": ms(min(t_dev))},
            "read_rect_route_ms": {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_read_rect_median": ms(statistics.median(t_read))},
            "speedup_slowest": round(max(t_host) / max(t_dev), 2),
            "kernel_us": round(kernel_us, 2), "kernel_launches_timed": launches,
            "kernel_gb_read_per_s": round(2 * 20 * X * Y * B / (kernel_us * 1e-6) / 1e9, 1) if kernel_us > 0 else None}


QUANTILES_P = (0.1, 0.5, 0.9)


def numpy_quantiles(fields, walls, p):
    """The per-cell function of include/wxsim.h (WX_QUANT_LINEAR) in numpy: np.sort along the member axis, then the definition's float64
    arithmetic, one operation per rounded operation (what a host does today)."""
    import numpy as np
    v = np.stack(fields)
    is_wall = np.stack([wl[..., 1] == 0 for wl in walls])
    take = ~is_wall[..., None] & np.isfinite(v)
    n = take.sum(0).astype(np.int32)
    with np.errstate(all="ignore"):
        s = np.sort(np.where(take, np.where(v == 0, np.float32(0), v), np.float32(np.inf)), axis=0)
        q = []
        for pj in p:
            h = np.float64(np.float32(pj)) * (n - 1).astype(np.float64)
            k = np.floor(h)
            g = h - k
            ki = np.clip(k.astype(np.int64), 0, None)
            k1 = np.clip(np.minimum(ki + 1, n - 1), 0, None)
            vk, vk1 = np.take_along_axis(s, ki[None], 0)[0].astype(np.float64), np.take_along_axis(s, k1[None], 0)[0].astype(np.float64)
            d = vk1 - vk
            gd = g * d
            q.append(np.where(n > 0, (vk + gd).astype(np.float32), np.float32(np.nan)))
    return {"q": np.stack(q), "count": n, "n_wall": is_wall.sum(0).astype(np.int32)}


def time_quantiles(a, pkg, ens, X, Y, B):
    import statistics
    import numpy as np
    field, p = a.quantiles, QUANTILES_P
    staged = B <= pkg.engine.lib().wx_ens_quant_staged_members()

    def device():
        return ens.quantiles(field, p)

    def reads():
        return [m.read_rect(field) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]

    ens.step(a.frame)
    ens.sync()
    got, want = device(), numpy_quantiles(*reads(), p)
    differ = [k for k in want if not np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f")]
    if differ:  # two routes that disagree are not two timings of one thing
        sys.exit("--quantiles %s %dx%dx%d: wx_ensemble_quantiles and the read_rect route disagree in %s" % (field, X, Y, B, ", ".join(differ)))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        device()
    ens[0].profile(True)
    t_dev, t_read, t_host = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        device()
        t_dev.append(time.perf_counter() - t0)
    kernel_ms, launches = ens[0].profile_read().get("ensemble_quantiles", (0.0, 0))
    for _ in range(a.repeats):  # the comparison: k_ens_stat with the variance wanted reads every member twice
        ens.statistics(field, want=("mean", "variance", "count", "n_wall"))
    stat_ms, stat_launches = ens[0].profile_read().get("ensemble_statistics", (0.0, 0))
    ens[0].profile(False)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = reads()
        t1 = time.perf_counter()
        numpy_quantiles(*r, p)
        t_read.append(t1 - t0)
        t_host.append(time.perf_counter() - t0)
    kernel_us, stat_us = 1e3 * kernel_ms / max(launches, 1), 1e3 * stat_ms / max(stat_launches, 1)
    ms = lambda t: round(1e3 * t, 3)
    return {"field": field, "members": B, "p": list(p), "interp": "linear", "path": "staged (LDS)" if staged else "streaming", "calls": a.repeats, "same_numbers": True,
            "quantiles_call_ms": {"slowest": ms(max(t_dev)), "median": ms(statistics.median(t_dev))},
            "read_rect_route_ms": {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_read_rect_median": ms(statistics.median(t_read))},
            "speedup_slowest": round(max(t_host) / max(t_dev), 2),
            "kernel_us": round(kernel_us, 2), "kernel_launches_timed": launches,
            "kernel_gb_read_per_s": round(20 * X * Y * B / (kernel_us * 1e-6) / 1e9, 1) if kernel_us > 0 and staged else None,
            "statistics_kernel_with_variance_us": round(stat_us, 2), "statistics_kernel_launches_timed": stat_launches,
            "quantiles_kernel_over_statistics_kernel": round(kernel_us / stat_us, 3) if stat_us > 0 else None}


def numpy_scores(stat, rank, truth, truth_wall, fields, walls):
    """What a host reduces the planes to today: the domain sums in plain float64 (np.sum, not exact), the two histograms, and the CRPS
    from the members' sorted values."""
    import numpy as np
    n = stat["count"]
    with np.errstate(all="ignore"):
        ok = (truth_wall[..., 1] != 0)[..., None] & np.isfinite(truth) & (n > 0)
        err = stat["mean"].astype(np.float64) - truth
        v = np.stack(fields)
        take = ~np.stack([wl[..., 1] == 0 for wl in walls])[..., None] & np.isfinite(v)
        s = np.sort(np.where(take, v, np.float32(np.inf)), axis=0).astype(np.float64)
        i = np.arange(len(fields)).reshape(-1, 1, 1, 1)
        inside = i < n
        u = s - truth.astype(np.float64)
        A = np.where(inside, np.abs(u), 0.0).sum(0)
        G = np.where(inside, (2 * i - n + 1) * u, 0.0).sum(0)
        crps = A / n - G / (n.astype(np.float64) ** 2)
    out = {"n_scored": ok.sum((0, 1))}
    for name, x in (("sum_error", err), ("sum_abs_error", np.abs(err)), ("sum_sq_error", err * err), ("sum_variance", stat["variance"].astype(np.float64)), ("sum_crps", crps)):
        out[name] = np.where(ok, x, 0.0).sum((0, 1))
    out["rank_low"] = np.stack([np.bincount(rank["n_below"][..., c][ok[..., c]], minlength=65) for c in range(4)])
    out["rank_high"] = np.stack([np.bincount((rank["n_below"] + rank["n_equal"])[..., c][ok[..., c]], minlength=65) for c in range(4)])
    return out


def time_scores(a, pkg, ens, X, Y, B):
    import statistics
    import numpy as np
    field = a.scores
    sel = list(range(B))

    def device():
        return ens.scores(field, ens[B], members=sel)

    def host():
        t0 = time.perf_counter()
        stat = ens.statistics(field, members=sel, want=("mean", "variance", "count"))
        rank = ens.quantiles(field, (), rank_of=B, want=("n_below", "n_equal"))
        truth, truth_wall = ens[B].read_rect(field), ens[B].read_rect("WALL_CUR")
        fields, walls = [ens[i].read_rect(field) for i in sel], [ens[i].read_rect("WALL_CUR") for i in sel]
        t1 = time.perf_counter()
        return numpy_scores(stat, rank, truth, truth_wall, fields, walls), t1 - t0

    ens.step(a.frame)
    ens.sync()
    got, (want, _) = device(), host()
    scale = 1e-7 * X * Y * max(1.0, float(np.nanmax(np.abs(ens[B].read_rect(field)))))
    for k, v in want.items():  # two routes that disagree are not two timings of one thing (the host's means are float32 and its sums cancel: loose)
        if not (np.array_equal(got[k], v) if v.dtype.kind == "i" else np.allclose(got[k], v, rtol=1e-4, atol=scale)):
            sys.exit("--scores %s %dx%dx%d: wx_ensemble_scores and the host route disagree in %s: %r / %r" % (field, X, Y, B, k, got[k], v))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        device()
    ens[0].profile(True)
    t_dev, t_host, t_calls = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        device()
        t_dev.append(time.perf_counter() - t0)
    kernel_ms, launches = ens[0].profile_read().get("ensemble_scores", (0.0, 0))
    for _ in range(a.repeats):  # the comparison: the quantile kernel reads the same bytes and sorts the same keys
        ens.quantiles(field, (0.1, 0.5, 0.9), members=sel)
    quant_ms, quant_launches = ens[0].profile_read().get("ensemble_quantiles", (0.0, 0))
    ens[0].profile(False)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        _, calls = host()
        t_calls.append(calls)
        t_host.append(time.perf_counter() - t0)
    kernel_us, quant_us = 1e3 * kernel_ms / max(launches, 1), 1e3 * quant_ms / max(quant_launches, 1)
    ms = lambda t: round(1e3 * t, 3)
    return {"field": field, "members": B, "calls": a.repeats, "same_numbers": True, "n_scored": [int(v) for v in got["n_scored"]],
            "scores_call_ms": {"slowest": ms(max(t_dev)), "median": ms(statistics.median(t_dev))},
            "host_route_ms": {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_calls_and_read_rect_median": ms(statistics.median(t_calls))},
            "speedup_slowest": round(max(t_host) / max(t_dev), 2),
            "kernel_us": round(kernel_us, 2), "kernel_launches_timed": launches,
            "kernel_gb_read_per_s": round(20 * X * Y * (B + 1) / (kernel_us * 1e-6) / 1e9, 1) if kernel_us > 0 else None,
            "quantiles_kernel_us": round(quant_us, 2), "quantiles_kernel_launches_timed": quant_launches,
            "scores_kernel_over_quantiles_kernel": round(kernel_us / quant_us, 3) if quant_us > 0 else None}


NBHD_SCALES = [(0, 0), (1, 1), (4, 2), (8, 4), (16, 8)]
NBHD_CHANNEL = 1


def numpy_neighbourhood(count, above, truth, truth_wall, threshold, scales, wrap):
    """What a host does with the statistics planes today: one summed-area table per quantity and scale (windows clipped in y, wrapped
    in x by padding), the fractions, the three sums in plain float64 (np.sum, not exact)."""
    import numpy as np
    Y, X = count.shape
    v = truth[..., NBHD_CHANNEL]
    no = ((truth_wall[..., 1] != 0) & np.isfinite(v)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        eo = no * (v > np.float32(threshold))
    out = {k: [] for k in ("n_scored", "sum_d2", "sum_f2", "sum_o2", "nep")}
    for rx, ry in scales:
        def box(q):
            p = np.pad(np.pad(q.astype(np.int64), ((ry, ry), (0, 0))), ((0, 0), (rx, rx)), mode="wrap" if wrap else "constant")
            sat = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
            sat[1:, 1:] = p.cumsum(0).cumsum(1)
            h, w = 2 * ry + 1, 2 * rx + 1
            return sat[h:h + Y, w:w + X] - sat[:Y, w:w + X] - sat[h:h + Y, :X] + sat[:Y, :X]
        Af, Bf, Ao, Bo = box(above), box(count), box(eo), box(no)
        with np.errstate(all="ignore"):
            pf, po = Af / Bf, Ao / Bo
            d = pf - po
        ok = (Bf > 0) & (Bo > 0)
        out["n_scored"].append(int(ok.sum()))
        for name, t in (("sum_d2", d * d), ("sum_f2", pf * pf), ("sum_o2", po * po)):
            out[name].append(float(t.astype(np.float32)[ok].astype(np.float64).sum()))
        out["nep"].append(pf.astype(np.float32))
    return out


def time_neighbourhood(a, pkg, ens, X, Y, B):
    import statistics
    import numpy as np
    field, sel, wrap = a.neighbourhood, list(range(B)), True
    ens.step(a.frame)
    ens.sync()
    truth_now = ens[B].read_rect(field)[..., NBHD_CHANNEL]
    air = ens[B].read_rect("WALL_CUR")[..., 1] != 0
    pos = truth_now[air & (truth_now > 0)]
    threshold = float(np.median(pos)) if pos.size else float(np.median(truth_now[air]))  # an event in about half of the cells that hold any

    def device(want=()):
        return ens.neighbourhood(field, NBHD_CHANNEL, threshold, NBHD_SCALES, ens[B], members=sel, wrap_x=wrap, want=want)

    def host():
        t0 = time.perf_counter()
        st = ens.statistics(field, members=sel, threshold=(threshold,) * 4, want=("count", "n_above"))
        truth, truth_wall = ens[B].read_rect(field), ens[B].read_rect("WALL_CUR")
        t1 = time.perf_counter()
        return numpy_neighbourhood(st["count"][..., NBHD_CHANNEL], st["n_above"][..., NBHD_CHANNEL], truth, truth_wall, threshold, NBHD_SCALES, wrap), t1 - t0

    got, (want, _) = device(("nep",)), host()
    if got["n_scored"].tolist() != want["n_scored"] or not all(np.array_equal(got["nep"][s], want["nep"][s], equal_nan=True) for s in range(len(NBHD_SCALES))):
        sys.exit("--neighbourhood %s %dx%dx%d: wx_ensemble_neighbourhood and the host route disagree in the counts or in nep" % (field, X, Y, B))
    for k in ("sum_d2", "sum_f2", "sum_o2"):  # (the host's sums are running float64 sums: close, not equal)
        if not np.allclose(got[k], want[k], rtol=1e-9, atol=1e-9):
            sys.exit("--neighbourhood %s %dx%dx%d: the two routes disagree in %s: %r / %r" % (field, X, Y, B, k, got[k], want[k]))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        device()
    ens[0].profile(True)
    t_dev, t_host, t_calls = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        device()
        t_dev.append(time.perf_counter() - t0)
    prof = ens[0].profile_read()
    (points_ms, launches), (windows_ms, _) = prof.get("ensemble_nbhd_points", (0.0, 0)), prof.get("ensemble_nbhd_windows", (0.0, 0))
    for _ in range(a.repeats):  # the comparison OF THE SAME RUN: the statistics kernel reads the same bytes and computes more
        ens.statistics(field, members=sel, threshold=(threshold,) * 4, want=("count", "n_above"))
    stat_ms, stat_launches = ens[0].profile_read().get("ensemble_statistics", (0.0, 0))
    per_scale = []
    for sc in NBHD_SCALES:  # the windows kernel scale by scale
        for _ in range(a.repeats):
            ens.neighbourhood(field, NBHD_CHANNEL, threshold, [sc], ens[B], members=sel, wrap_x=wrap, want=())
        ms_s, n_s = ens[0].profile_read().get("ensemble_nbhd_windows", (0.0, 0))
        per_scale.append(round(1e3 * ms_s / max(n_s, 1), 2))
    ens[0].profile(False)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        _, calls = host()
        t_calls.append(calls)
        t_host.append(time.perf_counter() - t0)
    points_us, windows_us, stat_us = 1e3 * points_ms / max(launches, 1), 1e3 * windows_ms / max(launches, 1), 1e3 * stat_ms / max(stat_launches, 1)
    ms = lambda t: round(1e3 * t, 3)
    den = got["sum_f2"] + got["sum_o2"]
    return {"field": field, "channel": NBHD_CHANNEL, "threshold": threshold, "members": B, "calls": a.repeats, "scales": NBHD_SCALES, "wrap_x": wrap, "same_numbers": True,
            "n_scored": [int(v) for v in got["n_scored"]], "fss": [round(float(1 - d / q), 4) if q > 0 else None for d, q in zip(got["sum_d2"], den)],
            "neighbourhood_call_ms": {"slowest": ms(max(t_dev)), "median": ms(statistics.median(t_dev))},
            "host_route_ms": {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_statistics_and_read_rect_median": ms(statistics.median(t_calls))},
            "speedup_slowest": round(max(t_host) / max(t_dev), 2),
            "points_kernel_us": round(points_us, 2), "windows_kernel_us_all_scales": round(windows_us, 2), "kernel_launches_timed": launches,
            "windows_kernel_us_per_scale_alone": per_scale,
            "points_kernel_gb_read_per_s": round(20 * X * Y * (B + 1) / (points_us * 1e-6) / 1e9, 1) if points_us > 0 else None,
            "statistics_kernel_us": round(stat_us, 2), "statistics_kernel_launches_timed": stat_launches,
            "points_kernel_over_statistics_kernel": round(points_us / stat_us, 3) if stat_us > 0 else None}


def time_spawn(a, pkg, ens, X, Y, B):
    import statistics
    import numpy as np
    E = pkg.engine
    lone = make_members(pkg, X, Y, 1, lambda i: E.Handle(X, Y, a.droplets), a.flow, a.droplets)[0]
    lone.step(5 * a.frame)
    lone.sync()
    amp, scale = (0.0, 0.0, 0.0, 0.5), 8

    def route_a(seed):
        ens[0].copy_from(lone)
        ens.broadcast(0)
        ens.perturb("BASE_CUR", amp, scale=scale, seed=seed)

    base, water, wall = lone.read_rect("BASE_CUR"), lone.read_rect("WATER_CUR"), lone.read_rect("WALL_CUR")
    drops = lone.read_particles() if a.droplets else None
    air = wall[..., 1] != 0
    rng = np.random.default_rng(1)

    def route_b(seed):
        for i in range(B):
            b = base.copy()
            b[..., 3] += np.where(air, rng.uniform(-amp[3], amp[3], air.shape), 0).astype(np.float32)
            ens[i].upload(b, water, wall, drops)

    route_a(0)
    for i in range(B):  # every member shows the stepped state (route B below does not: see the docstring)
        if ens[i].iter != lone.iter or not np.array_equal(ens[i].read_rect("LIGHT_0"), lone.read_rect("LIGHT_0")):
            sys.exit("--spawn %dx%dx%d: member %d is not a clone of the stepped handle" % (X, Y, B, i))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        route_a(0)
    ens[0].profile(True)
    t_a, t_b = [], []
    for k in range(a.repeats):
        t0 = time.perf_counter()
        route_a(1 + k)
        t_a.append(time.perf_counter() - t0)
    kernel_ms, launches = ens[0].profile_read().get("ensemble_perturb", (0.0, 0))
    ens[0].profile(False)
    for k in range(a.repeats):
        t0 = time.perf_counter()
        route_b(1 + k)
        t_b.append(time.perf_counter() - t0)
    lone.close()
    kernel_us = 1e3 * kernel_ms / max(launches, 1)
    gbs = 36 * X * Y * B / (kernel_us * 1e-6) / 1e9 if kernel_us > 0 else None
    ms = lambda t: round(1e3 * t, 3)
    return {"members": B, "calls": a.repeats, "perturbed": "BASE_CUR temperature, amplitude 0.5, scale 8",
            "route_a_broadcast_perturb_ms": {"slowest": ms(max(t_a)), "median": ms(statistics.median(t_a))},
            "route_b_uploads_ms": {"slowest": ms(max(t_b)), "median": ms(statistics.median(t_b))},
            "speedup_slowest": round(max(t_b) / max(t_a), 2), "route_b_carries_the_state": False,
            "route_b_loses": "light textures, curl, feedback textures, lightning state, `even`: its members are fresh uploads, not the stepped simulation",
            "perturb_kernel_us": round(kernel_us, 2), "kernel_launches_timed": launches, "kernel_bytes": 36 * X * Y * B,
            "kernel_gb_per_s": round(gbs, 1) if gbs else None, "kernel_fraction_of_peak": round(gbs / a.peak_gbs, 4) if gbs else None}


def time_assimilate(a, pkg, ens, X, Y, B):
    import statistics
    import numpy as np
    E = pkg.engine
    field, c = a.assimilate, 3 if a.assimilate == "BASE_CUR" else 0
    ens.step(a.frame)
    ens.sync()
    loc = (20.0, 10.0)
    gains = dict(gain_base=1.0 if field == "BASE_CUR" else 0.0, gain_water=1.0 if field == "WATER_CUR" else 0.0, lo_water=0.0)

    def read_all():
        return ([h.read_rect("BASE_CUR") for h in ens.members], [h.read_rect("WATER_CUR") for h in ens.members], [h.read_rect("WALL_CUR") for h in ens.members])

    bases, waters, walls = read_all()
    air = np.all([w[..., 1] != 0 for w in walls], axis=0)
    ys, xs = np.nonzero(air)
    rng = np.random.default_rng(1)

    def observations():
        vals = np.stack([(bases if field == "BASE_CUR" else waters)[i][..., c].astype(np.float64) for i in range(B)])
        out = []
        for k in rng.integers(0, len(xs), a.observations):
            v = vals[:, ys[k], xs[k]]
            sd = max(float(v.std()), 1e-3 * abs(float(v.mean())), 1e-6)
            out.append((field, int(xs[k]), int(ys[k]), c, float(v.mean()) + sd * float(rng.normal()), 0.5 * sd * sd))
        return out

    obs = observations()
    # member-cells x observations the update kernel may touch: weight != 0 where dx < 2 loc_x and dy < 2 loc_y (the members wrap in x)
    yy, xx = np.mgrid[0:Y, 0:X]
    touched = 0
    for o in obs:
        dx = np.abs(xx - o[1])
        touched += int(((np.minimum(dx, X - dx) < 2 * loc[0]) & (np.abs(yy - o[2]) < 2 * loc[1])).sum())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        ens.assimilate(obs, loc=loc, wrap_x=True, **gains)
    ens[0].profile(True)
    t_one, t_n, t_host, t_read, applied = [], [], [], [], 0
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = ens.assimilate(obs, loc=loc, wrap_x=True, **gains)
        t_one.append(time.perf_counter() - t0)
        applied = sum(r["applied"] for r in res)
    prof = ens[0].profile_read()
    ens[0].profile(False)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for o in obs:
            ens.assimilate([o], loc=loc, wrap_x=True, **gains)
        t_n.append(time.perf_counter() - t0)
    drops = [h.read_particles() for h in ens.members] if a.droplets else [None] * B
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        bases, waters, walls = read_all()
        t1 = time.perf_counter()
        nb, nw, _ = E.ens_assim_cells(bases, waters, walls, X, Y, obs, loc=loc, wrap_x=True, **gains)
        for i, h in enumerate(ens.members):
            h.upload(nb[i], nw[i], walls[i], drops[i])
        ens.sync()
        t_read.append(t1 - t0)
        t_host.append(time.perf_counter() - t0)
    obs_ms, obs_n = prof.get("ensemble_assimilate_obs", (0.0, 0))
    upd_ms, upd_n = prof.get("ensemble_assimilate", (0.0, 0))
    obs_us, upd_us = 1e3 * obs_ms / max(obs_n, 1), 1e3 * upd_ms / max(upd_n, 1)
    bytes_most = 76 * touched * B
    ms = lambda t: round(1e3 * t, 3)
    return {"field": field, "members": B, "observations": a.observations, "applied": applied, "loc": list(loc), "calls": a.repeats,
            "one_call_ms": {"slowest": ms(max(t_one)), "median": ms(statistics.median(t_one))},
            "n_calls_of_one_ms": {"slowest": ms(max(t_n)), "median": ms(statistics.median(t_n))},
            "read_host_upload_route_ms": {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_read_rect_median": ms(statistics.median(t_read))},
            "speedup_slowest_over_host_route": round(max(t_host) / max(t_one), 2), "speedup_slowest_over_n_calls": round(max(t_n) / max(t_one), 2),
            "host_route_carries_the_state": False,
            "host_route_loses": "wx_upload resets light, curl, the feedback textures and the lightning state: its members are fresh uploads, not the stepped simulation",
            "obs_kernel_us": round(obs_us, 2), "obs_kernel_launches_timed": obs_n, "update_kernel_us": round(upd_us, 2), "update_kernel_launches_timed": upd_n,
            "update_member_cell_observations": touched * B, "update_kernel_bytes_at_most": bytes_most,
            "update_kernel_gb_per_s_at_most": round(bytes_most / (upd_us * 1e-6) / 1e9, 1) if upd_us > 0 else None,
            "update_kernel_fraction_of_peak_at_most": round(bytes_most / (upd_us * 1e-6) / 1e9 / a.peak_gbs, 4) if upd_us > 0 else None}


INFLATE_BYTES = {"const": 52, "rtps": 100, "rtpp": 84}  # per member-cell, every cell updated: what the walks of csrc/wx_ens_inflate.h request
INFLATE_BYTES_ONCE = {"const": 36, "rtps": 52, "rtpp": 52}  # ... and what crosses the memory interface if every re-read is served on the chip
PRIOR_SAVE_BYTES = 32


def time_inflate(a, pkg, ens, X, Y, B):
    import statistics
    E = pkg.engine
    field = a.inflate
    ens.step(a.frame)
    ens.sync()
    ens.save_prior(field)
    ens.step(a.frame)
    ens.sync()
    calls = {"const": dict(coef=1.1), "rtps": dict(coef=0.5), "rtpp": dict(coef=0.5)}
    clamp = dict(lo=0.0) if field == "WATER_CUR" else {}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        ens.inflate(field, 1.0 + 1e-6, mode="const", **clamp)
    ms = lambda t: round(1e3 * t, 3)  # noqa: E731
    rec = {"field": field, "members": B, "calls": a.repeats, "modes": {}}
    for mode, kw in calls.items():
        ens[0].profile(True)
        t_call = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ens.inflate(field, kw["coef"], mode=mode, **clamp)
            t_call.append(time.perf_counter() - t0)
        prof = ens[0].profile_read()
        ens[0].profile(False)
        k_ms, k_n = prof.get("ensemble_inflate", (0.0, 0))
        k_us = 1e3 * k_ms / max(k_n, 1)
        nbytes = INFLATE_BYTES[mode] * X * Y * B
        gbs = nbytes / (k_us * 1e-6) / 1e9 if k_us > 0 else None
        once = INFLATE_BYTES_ONCE[mode] * X * Y * B / (k_us * 1e-6) / 1e9 if k_us > 0 else None
        rec["modes"][mode] = {"coef": kw["coef"], "one_call_ms": {"slowest": ms(max(t_call)), "median": ms(statistics.median(t_call)), "fastest": ms(min(t_call))},
                              "kernel_us": round(k_us, 2), "kernel_launches_timed": k_n, "bytes_per_member_cell_at_most": INFLATE_BYTES[mode],
                              "kernel_gb_per_s_at_most": round(gbs, 1) if gbs else None, "kernel_fraction_of_peak_at_most": round(gbs / a.peak_gbs, 4) if gbs else None,
                              "bytes_per_member_cell_read_once": INFLATE_BYTES_ONCE[mode], "kernel_gb_per_s_read_once": round(once, 1) if once else None,
                              "kernel_fraction_of_peak_read_once": round(once / a.peak_gbs, 4) if once else None}
    ens[0].profile(True)
    t_save = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ens.save_prior(field)
        t_save.append(time.perf_counter() - t0)
    prof = ens[0].profile_read()
    ens[0].profile(False)
    s_ms, s_n = prof.get("ensemble_prior_save", (0.0, 0))
    s_us = 1e3 * s_ms / max(s_n, 1)
    gbs = PRIOR_SAVE_BYTES * X * Y * B / (s_us * 1e-6) / 1e9 if s_us > 0 else None
    rec["prior_save"] = {"one_call_ms": {"slowest": ms(max(t_save)), "median": ms(statistics.median(t_save))}, "kernel_us": round(s_us, 2), "kernel_launches_timed": s_n,
                         "snapshot_bytes": 16 * X * Y * B, "kernel_gb_per_s": round(gbs, 1) if gbs else None,
                         "kernel_fraction_of_peak": round(gbs / a.peak_gbs, 4) if gbs else None}
    # the host route: B read_rect pairs + the host function (RTPS; the prior read once more, as a host would have kept it); no way back is timed
    prior = [h.read_rect(field) for h in ens.members]
    t_host, t_read = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        fields, walls = [h.read_rect(field) for h in ens.members], [h.read_rect("WALL_CUR") for h in ens.members]
        t1 = time.perf_counter()
        E.ens_inflate_cells(fields, walls, field, 0.5, mode="rtps", priors=prior, **clamp)
        t_read.append(t1 - t0)
        t_host.append(time.perf_counter() - t0)
    rec["read_host_route_rtps_ms"] = {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_read_rect_median": ms(statistics.median(t_read))}
    rec["speedup_slowest_over_host_route_rtps"] = round(max(t_host) / float(rec["modes"]["rtps"]["one_call_ms"]["slowest"]) * 1e3, 2)
    rec["host_route_way_back"] = "not timed: B wx_upload calls, which reset light, curl, the feedback textures and the lightning state"
    return rec


def numpy_covariance(fields, walls, points):
    """The arithmetic of wx_ensemble_covariance in numpy, float64, vectorised over the cells (not bit-exact: numpy's sums are pairwise):
    what a host does with B read_rect results."""
    import numpy as np
    f = np.stack([np.float64(a) for a in fields])
    air = np.all(np.stack([w[..., 1] != 0 for w in walls]), axis=0)
    ok = air[..., None] & np.isfinite(f).all(axis=0)
    n = f.shape[0]
    d = f - f.mean(axis=0)
    qx = (d * d).sum(axis=0)
    out = {"variance": np.where(ok, qx / (n - 1), np.nan).astype(np.float32), "cov": [], "corr": [], "slope": []}
    for x, y, c in points:
        t = f[:, y, x, c]
        e = t - t.mean()
        qj = float((e * e).sum())
        cq = np.tensordot(e, d, axes=(0, 0))
        with np.errstate(invalid="ignore", divide="ignore"):
            out["cov"].append(np.where(ok, cq / (n - 1), np.nan).astype(np.float32))
            out["slope"].append(np.where(ok, cq / qx, np.nan).astype(np.float32))
            out["corr"].append(np.where(ok, np.clip(cq / np.sqrt(qx * qj), -1, 1), np.nan).astype(np.float32))
    return out


COV_READ_BYTES = 36  # per member-cell: walk 1's 16 B + 4 B, walk 2's 16 B (csrc/wx_ens_cov.h)


def time_covariance(a, pkg, ens, X, Y, B):
    import statistics
    field = a.covariance
    ens.step(a.frame)
    ens.sync()
    air = None
    for h in ens.members:
        w = h.read_rect("WALL_CUR")[..., 1] != 0
        air = w if air is None else air & w
    import numpy as np
    ys, xs = np.nonzero(air)
    pick = np.linspace(0, len(xs) - 1, 8).astype(int)
    points = [(field, int(xs[i]), int(ys[i]), 3 if field == "BASE_CUR" else 0) for i in pick]
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed
        ens.covariance(field, points[:1], want=("corr",))
    ms = lambda t: round(1e3 * t, 3)  # noqa: E731
    rec = {"field": field, "members": B, "calls": a.repeats, "predictors": {}}
    for n_pred in (1, 8):
        ens[0].profile(True)
        t_call = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ens.covariance(field, points[:n_pred])
            t_call.append(time.perf_counter() - t0)
        prof = ens[0].profile_read()
        ens[0].profile(False)
        k_ms, k_n = prof.get("ensemble_covariance", (0.0, 0))
        p_ms, p_n = prof.get("ensemble_covariance_pred", (0.0, 0))
        k_us = 1e3 * k_ms / max(k_n, 1)
        nbytes = COV_READ_BYTES * X * Y * B + (3 * n_pred + 1) * 16 * X * Y
        once = (COV_READ_BYTES - 16) * X * Y * B + (3 * n_pred + 1) * 16 * X * Y
        gbs = nbytes / (k_us * 1e-6) / 1e9 if k_us > 0 else None
        gbs_once = once / (k_us * 1e-6) / 1e9 if k_us > 0 else None
        rec["predictors"][str(n_pred)] = {"one_call_ms": {"slowest": ms(max(t_call)), "median": ms(statistics.median(t_call))},
                                          "kernel_us": round(k_us, 2), "prepass_kernel_us": round(1e3 * p_ms / max(p_n, 1), 2), "kernel_launches_timed": k_n,
                                          "bytes_requested": nbytes, "kernel_gb_per_s_requested": round(gbs, 1) if gbs else None,
                                          "kernel_fraction_of_peak_requested": round(gbs / a.peak_gbs, 4) if gbs else None,
                                          "kernel_gb_per_s_second_walk_on_chip": round(gbs_once, 1) if gbs_once else None,
                                          "kernel_fraction_of_peak_second_walk_on_chip": round(gbs_once / a.peak_gbs, 4) if gbs_once else None}
    t_eight = []
    for _ in range(a.repeats):  # 8 calls of one predictor: what taking several predictors at once saves
        t0 = time.perf_counter()
        for p in points:
            ens.covariance(field, [p])
        t_eight.append(time.perf_counter() - t0)
    rec["eight_calls_of_one_ms"] = {"slowest": ms(max(t_eight)), "median": ms(statistics.median(t_eight))}
    rec["eight_calls_over_one_call_of_eight_median"] = round(statistics.median(t_eight) * 1e3 / float(rec["predictors"]["8"]["one_call_ms"]["median"]), 2)
    # the statistics kernel of the same run: the same member bytes, two planes written
    ens[0].profile(True)
    for _ in range(a.repeats):
        ens.statistics(field, want=("mean", "variance"))
    prof = ens[0].profile_read()
    ens[0].profile(False)
    s_ms, s_n = prof.get("ensemble_statistics", (0.0, 0))
    rec["statistics_kernel_us_mean_variance"] = round(1e3 * s_ms / max(s_n, 1), 2)
    # the host route: B read_rect pairs + numpy
    for n_pred in (1, 8):
        t_host, t_read = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fields, walls = [h.read_rect(field) for h in ens.members], [h.read_rect("WALL_CUR") for h in ens.members]
            t1 = time.perf_counter()
            numpy_covariance(fields, walls, [p[1:] for p in points[:n_pred]])
            t_read.append(t1 - t0)
            t_host.append(time.perf_counter() - t0)
        rec["read_numpy_route_%d_ms" % n_pred] = {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_read_rect_median": ms(statistics.median(t_read))}
        rec["speedup_median_over_read_numpy_route_%d" % n_pred] = round(statistics.median(t_host) * 1e3 / float(rec["predictors"][str(n_pred)]["one_call_ms"]["median"]), 2)
    return rec


def _gram_deviations(fields, walls):
    """(4, n, cells) float64, contiguous per channel: the deviations from the members' mean, 0 where a cell-channel does not enter
    (the overflow test of the definition is left out: these fields hold nothing near 2^64)."""
    import numpy as np
    f = np.stack([np.float64(a) for a in fields])
    air = np.all(np.stack([w[..., 1] != 0 for w in walls]), axis=0)
    ok = air[..., None] & np.isfinite(f).all(axis=0)
    d = np.where(ok, f - f.mean(axis=0), 0.0).reshape(f.shape[0], -1, 4)
    return np.ascontiguousarray(np.moveaxis(d, 2, 0))


def numpy_gram(fields, walls):
    """The quick host route: float64, one matrix product per channel on contiguous arrays. Not the device's numbers: the products are
    not rounded to float and BLAS sums in its own order."""
    import numpy as np
    d = _gram_deviations(fields, walls)
    return np.stack([d[c] @ d[c].T for c in range(4)])


def numpy_gram_terms(fields, walls):
    """The numpy restatement of the definition without fsum: per pair a <= b the float32-rounded terms (d_a * d_b).astype(float32),
    summed in float64 by numpy (pairwise, so not the exact sum)."""
    import numpy as np
    d = _gram_deviations(fields, walls)
    n = d.shape[1]
    g = np.zeros((4, n, n))
    for c in range(4):
        for a_ in range(n):
            for b_ in range(a_, n):
                g[c, a_, b_] = g[c, b_, a_] = (d[c, a_] * d[c, b_]).astype(np.float32).sum(dtype=np.float64)
    return g


def time_gram(a, pkg, ens, X, Y, B):
    import statistics
    import numpy as np
    field = a.gram
    ens.step(a.frame)
    ens.sync()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # clock conditioning, untimed (the first call also sizes the ensemble's staging buffers)
        ens.gram(field)
    ms = lambda t: round(1e3 * t, 3)  # noqa: E731
    rec = {"field": field, "members": B, "calls": a.repeats}
    ens[0].profile(True)
    t_call = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        got = ens.gram(field)
        t_call.append(time.perf_counter() - t0)
    prof = ens[0].profile_read()
    ens[0].profile(False)
    k_ms, k_n = prof.get("ensemble_gram", (0.0, 0))
    p_ms, p_n = prof.get("ensemble_gram_centre", (0.0, 0))
    rec["one_call_ms"] = {"slowest": ms(max(t_call)), "median": ms(statistics.median(t_call))}
    rec["kernel_us"] = round(1e3 * k_ms / max(k_n, 1), 2)
    rec["prepass_kernel_us"] = round(1e3 * p_ms / max(p_n, 1), 2)
    rec["kernel_launches_timed"] = k_n
    rec["pairs"] = B * (B + 1) // 2
    rec["entered_fraction"] = [round(float(v) / (X * Y), 4) for v in got["n_entered"]]
    # the statistics kernel of the same run: it reads the same member bytes once
    ens[0].profile(True)
    for _ in range(a.repeats):
        ens.statistics(field, want=("mean", "variance"))
    prof = ens[0].profile_read()
    ens[0].profile(False)
    s_ms, s_n = prof.get("ensemble_statistics", (0.0, 0))
    s_us = 1e3 * s_ms / max(s_n, 1)
    rec["statistics_kernel_us_mean_variance"] = round(s_us, 2)
    rec["gram_kernels_over_statistics_kernel"] = round((rec["kernel_us"] + rec["prepass_kernel_us"]) / s_us, 2) if s_us > 0 else None
    # the host route: B read_rect pairs + numpy
    t_host, t_read = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        fields, walls = [h.read_rect(field) for h in ens.members], [h.read_rect("WALL_CUR") for h in ens.members]
        t1 = time.perf_counter()
        host = numpy_gram(fields, walls)
        t_read.append(t1 - t0)
        t_host.append(time.perf_counter() - t0)
    rec["read_numpy_route_ms"] = {"slowest": ms(max(t_host)), "median": ms(statistics.median(t_host)), "of_which_read_rect_median": ms(statistics.median(t_read))}
    rec["speedup_median_over_read_numpy_route"] = round(statistics.median(t_host) / statistics.median(t_call), 2)
    rec["speedup_median_over_read_rect_alone"] = round(statistics.median(t_read) / statistics.median(t_call), 2)
    # the restatement without fsum (float32 terms per pair), on arrays already read: its arithmetic alone
    t_terms = []
    for _ in range(min(a.repeats, 3)):
        t0 = time.perf_counter()
        terms = numpy_gram_terms(fields, walls)
        t_terms.append(time.perf_counter() - t0)
    rec["numpy_float32_terms_per_pair_ms"] = {"slowest": ms(max(t_terms)), "median": ms(statistics.median(t_terms)), "runs": len(t_terms)}
    rec["speedup_median_over_read_rect_plus_float32_terms"] = round((statistics.median(t_read) + statistics.median(t_terms)) / statistics.median(t_call), 2)
    rec["largest_difference_from_float32_terms_over_sqrt_gaa_gbb"] = float(np.max(np.abs(got["gram"] - terms) / (np.sqrt(np.einsum("cii,cjj->cij", terms, terms)) + 1e-300)))
    scale = np.sqrt(np.einsum("cii,cjj->cij", host, host)) + 1e-300
    rec["largest_difference_from_numpy_over_sqrt_gaa_gbb"] = float(np.max(np.abs(got["gram"] - host) / scale))
    return rec


def main():
    a = parse()
    if a.gram and (a.mode != "ensemble" or a.gram not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--gram BASE_CUR | WATER_CUR needs --mode ensemble")
    if a.covariance and (a.mode != "ensemble" or a.covariance not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--covariance BASE_CUR | WATER_CUR needs --mode ensemble")
    if a.inflate and (a.mode != "ensemble" or a.inflate not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--inflate BASE_CUR | WATER_CUR needs --mode ensemble")
    if a.assimilate and (a.mode != "ensemble" or a.assimilate not in ("BASE_CUR", "WATER_CUR") or not 1 <= a.observations <= 256):
        sys.exit("--assimilate BASE_CUR | WATER_CUR needs --mode ensemble and --observations 1 .. 256")
    if a.spawn and a.mode != "ensemble":
        sys.exit("--spawn needs --mode ensemble")
    if a.statistics and (a.mode != "ensemble" or a.statistics not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--statistics BASE_CUR | WATER_CUR needs --mode ensemble")
    if a.quantiles and (a.mode != "ensemble" or a.quantiles not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--quantiles BASE_CUR | WATER_CUR needs --mode ensemble")
    if a.scores and (a.mode != "ensemble" or a.scores not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--scores BASE_CUR | WATER_CUR needs --mode ensemble")
    if a.neighbourhood and (a.mode != "ensemble" or a.neighbourhood not in ("BASE_CUR", "WATER_CUR")):
        sys.exit("--neighbourhood BASE_CUR | WATER_CUR needs --mode ensemble")
    sys.path.insert(0, a.root)
    if a.share > 0:
        if "debug" not in os.environ.get("WXSIM_LIB", ""):
            sys.exit("--share needs WXSIM_LIB to name the debug build (the shipped library reads no environment variable)")
        os.environ["WX_ENS_SHARE"] = str(a.share)
    import torch
    import wxpkg
    pkg = wxpkg.load_package()
    E = pkg.engine
    E.lib().wx_set_option(None, E.Handle.OPT_PLACEMENT_SEARCH, 0)
    torch.cuda.set_device(0)
    out = {"tool": "ensemble_bench", "mode": a.mode, "root": os.path.relpath(a.root, ROOT), "frame": a.frame, "steps": a.steps, "share": a.share, "droplets": a.droplets,
           "shapes": {}}
    for spec in a.shapes.split(","):
        X, Y, B = (int(v) for v in spec.split("x"))
        if a.spawn:
            ens = E.Ensemble(B, X, Y, a.droplets)
            out["shapes"][spec] = {"members": B, "spawn": time_spawn(a, pkg, ens, X, Y, B)}
            ens.close()
            continue
        if a.scores:  # B members and the truth behind them
            ens = E.Ensemble(B + 1, X, Y)
            make_members(pkg, X, Y, B + 1, lambda i: ens[i], a.flow, 0)
            out["shapes"][spec] = {"members": B, "scores": time_scores(a, pkg, ens, X, Y, B)}
            ens.close()
            continue
        if a.neighbourhood:  # B members and the truth behind them
            ens = E.Ensemble(B + 1, X, Y)
            make_members(pkg, X, Y, B + 1, lambda i: ens[i], a.flow, 0)
            out["shapes"][spec] = {"members": B, "neighbourhood": time_neighbourhood(a, pkg, ens, X, Y, B)}
            ens.close()
            continue
        if a.mode == "ensemble":
            ens = E.Ensemble(B, X, Y, a.droplets) if a.droplets else E.Ensemble(B, X, Y)
            make_members(pkg, X, Y, B, lambda i: ens[i], a.flow, a.droplets)
            step, sync, close = ens.step, ens.sync, ens.close
        else:
            hs = make_members(pkg, X, Y, B, lambda i: E.Handle(X, Y, a.droplets), a.flow, a.droplets)

            def step(n):
                for h in hs:
                    h.step(n)

            def sync():
                for h in hs:
                    h.sync()

            def close():
                for h in hs:
                    h.close()

        if a.statistics:
            out["shapes"][spec] = {"members": B, "statistics": time_statistics(a, ens, X, Y, B)}
            close()
            continue
        if a.quantiles:
            out["shapes"][spec] = {"members": B, "quantiles": time_quantiles(a, pkg, ens, X, Y, B)}
            close()
            continue
        if a.inflate:
            out["shapes"][spec] = {"members": B, "inflate": time_inflate(a, pkg, ens, X, Y, B)}
            close()
            continue
        if a.covariance:
            out["shapes"][spec] = {"members": B, "covariance": time_covariance(a, pkg, ens, X, Y, B)}
            close()
            continue
        if a.gram:
            out["shapes"][spec] = {"members": B, "gram": time_gram(a, pkg, ens, X, Y, B)}
            close()
            continue
        if a.assimilate:
            out["shapes"][spec] = {"members": B, "assimilate": time_assimilate(a, pkg, ens, X, Y, B)}
            close()
            continue

        def frames(n):
            done = 0
            while done < n:
                k = min(a.frame, n - done)
                step(k)
                done += k

        times = []
        for _ in range(a.repeats):
            sync()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.25:  # clock conditioning: a quarter of a second of the same load, untimed
                frames(a.frame)
                sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames(a.steps)
            sync()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        per_iter = [t / a.steps for t in times]  # one iteration of ALL members
        worst = max(per_iter)
        rec = {"members": B, "us_per_iteration_of_all_members": [round(1e6 * t, 2) for t in per_iter],
               "slowest_us": round(1e6 * worst, 2), "slowest_us_per_member_iteration": round(1e6 * worst / B, 3),
               "mcell_steps_per_s_slowest": round(X * Y * B / worst / 1e6, 1),
               "roofline_fraction_slowest": round(X * Y * B * 104 / worst / (a.peak_gbs * 1e9), 4)}
        if a.mode == "ensemble":
            rec["stats"] = ens.stats()
            if a.droplets:
                rec["particle_stats"] = ens.particle_stats()
        out["shapes"][spec] = rec
        close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
