"""GPU box: what one diagnostics call (wx_diagnostics: exact sums, extremes, census in one device pass) costs, next to one wet iteration
of the same handle and to the route it replaces (wx_read_rect of base, water and wall + numpy sums on the host).
Per size: a device-generated terrain with a seeded flow, 20 wet iterations, then -- state parked -- 5 warm-up calls and 20 timed calls.
The call is synchronous (it ends in a stream synchronise), so a host clock around the 20 calls measures memset + both kernels + the
26 KB copy of the table + the synchronise; GB/s = 36 B per cell over that time (the kernel alone: rocprofv3 --kernel-trace --stats).
Usage: diag_cost.py [--out FILE] [XxY ...]      default sizes 2500x300 16384x2048 32768x4096; the readback route at the first two"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import wxpkg  # noqa: E402

pkg = wxpkg.load_package()
from weather_sandbox_amd import devtools  # noqa: E402

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "diag_cost.txt")
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
sizes = [tuple(int(v) for v in a.split("x")) for a in args] or [(2500, 300), (16384, 2048), (32768, 4096)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e3


say("size          cells      wet iteration   diagnostics call   GB/s (36 B/cell)   diag / iteration   readback + numpy   speed-up")
for i, (X, Y) in enumerate(sizes):
    gui = pkg.params.merge_settings(None)
    gui["sunAngle"] = 40.0
    u = pkg.params.uniforms_from_gui(gui, Y, quad_scale=0)
    u["enablePrecipitation"] = 0
    h = pkg.engine.Handle(X, Y, 0)
    h.setup_terrain(pkg.synth.sounding_rows(Y, gui, cloud_deck=True), sim_height=float(gui["simHeight"]))
    h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
    devtools.seed_flow(h, 0.1)
    h.step(20)
    h.sync()
    it_ms = timed(lambda: (h.step(10), h.sync()), 5) / 10
    for _ in range(5):
        d = h.diagnostics()
    diag_ms = timed(h.diagnostics, 20)
    gbs = 36.0 * X * Y / (diag_ms * 1e-3) / 1e9
    rb = "not measured"
    ratio = ""
    if i < 2:
        def route():
            b, w, wl = h.read_rect("BASE_CUR"), h.read_rect("WATER_CUR"), h.read_rect("WALL_CUR")
            air = wl[..., 1] != 0
            return [float(np.sum(f[..., c], dtype=np.float64, where=air)) for f in (b, w) for c in range(4)]
        ref = route()
        rb_ms = timed(route, 2)
        rb, ratio = "%.1f ms" % rb_ms, "%.0fx" % (rb_ms / diag_ms)
        got = d["sum_base"] + d["sum_water"]
        assert all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(got, ref)), (got, ref)
    say("%-13s %-10d %8.3f ms     %8.3f ms        %8.0f           %6.2f             %-18s %s" % ("%dx%d" % (X, Y), X * Y, it_ms, diag_ms, gbs, diag_ms / it_ms, rb, ratio))
    say("              n_air %d  n_wall %d  water %.17g  cloud %.17g  smoke %.17g  non-finite %d / %d" % (
        d["n_air"], d["n_wall"], d["sum_water"][0], d["sum_water"][1], d["sum_water"][3], d["n_nonfinite_base"], d["n_nonfinite_water"]))
    h.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
