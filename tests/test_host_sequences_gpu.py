"""Host call sequences against the CPU oracle, bit for bit: one named test per transition of the handle's lazy / on-demand state
(csrc/wxsim.hip, RunState and Water0) -- reads in an unusual order or left out, options / parameters / the iteration counter changed
between steps, a placement search or a device-side write with a field pending. tools/fuzz_parity.py --mode script draws such
sequences at random (tests/test_fuzz_gpu.py); these are the readable regressions."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_FIELDS = ["BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1", "CURL", "PRECIP_FB", "PRECIP_DEP"]
DRY_FIELDS = ["BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1", "PRECIP_FB", "PRECIP_DEP"]


@pytest.fixture(scope="module")
def E(pkg):
    return pkg.engine


def _scene(pkg, X, Y, seed=3, sigma=0.2, cloud=False):
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    rng = np.random.Generator(np.random.Philox(seed))
    air = wall[..., 1] != 0
    base[..., 0] += np.where(air, rng.normal(0, sigma, (Y, X)), 0).astype(np.float32)
    base[..., 1] += np.where(air, rng.normal(0, sigma / 2, (Y, X)), 0).astype(np.float32)
    if cloud:
        pkg.synth.add_cloud_deck(water, wall)
    return base, water, wall


def _uniforms(pkg, Y, drops=False, **gui_changes):
    mask = gui_changes.pop("pass_mask", pkg.params.PASS_ALL)
    gui = dict(pkg.params.merge_settings(None), **dict({"sunAngle": 35.0}, **gui_changes))
    u = pkg.params.uniforms_from_gui(gui, Y, quad_scale=0, pass_mask=mask)
    u["enablePrecipitation"] = 1 if drops else 0
    if drops:
        u.update(splat_order=1, spawnChanceMult=0.01)
    return u


class Pair:
    """A handle and the oracle, driven alike."""

    def __init__(self, pkg, oracle, E, X, Y, state, u, drops=None, iter0=0, **options):
        self.pkg, self.nd = pkg, 0 if drops is None else len(drops)
        self.h, self.o = E.Handle(X, Y, self.nd), oracle.OracleSim(X, Y, self.nd)
        self.h.upload(*state, drops)
        self.o.upload(*state, drops)
        self.params(u)
        self.h.iter = self.o.iter = iter0
        for k, v in dict(options, **({"SPLAT_ORDER": 1} if self.nd else {})).items():
            self.option(k, v)

    def option(self, name, value):
        self.h.set_option(getattr(self.h, "OPT_" + name), value)

    def params(self, u):
        self.h.set_params(self.pkg.params.fill_struct(self.pkg.params.WxParams(), u), u["initial_T"])
        self.o.set_params(u)

    def step(self, n, flags=0):
        self.h.step(n, flags)
        if not flags & 4:  # (the oracle makes a piece with WX_OVERLAP_MORE_TO_COME up with the next one)
            self.o.step(n + getattr(self, "_owed", 0))
            self._owed = 0
        else:
            self._owed = getattr(self, "_owed", 0) + n

    def same(self, *fields, rect=None, why=""):
        for f in fields:
            x, y, w, hh = rect if rect else (0, 0, self.h.X, self.h.Y)
            if f == "LIGHTNING":  # (a 1 x 1 texture)
                assert np.array_equal(self.h.read_rect(f), self.o.field(f)), why + " LIGHTNING"
                continue
            a, b = self.h.read_rect(f, x, y, w, hh), self.o.field(f)[y:y + hh, x:x + w]
            if f == "EMITTED":
                b = b.astype(np.float16)
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), f"{why} {f}: {np.count_nonzero(a != b)} of {a.size} values differ"
        if self.nd and not fields:
            assert np.array_equal(self.h.read_particles(), self.o.field("DROPS"), equal_nan=True), why + " DROPS"

    def close(self):
        self.h.close()
        self.o.close()


@pytest.mark.parametrize("n", [4, 5], ids=["even", "odd"])
def test_light0_read_before_water0(pkg, oracle, E, n):
    """waterTexture_0 on demand takes lightTexture_0 as the display iteration read it: the planes an odd iteration retired, or light_0's
    own after an even one -- whatever a reader (LIGHT_0, LIGHT_1, EMITTED, a step of no iterations under the other kernel set) did to
    the light textures' representation in between."""
    X, Y = 330, 96
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y), _uniforms(pkg, Y))
    t.step(n)
    t.same("LIGHT_0", "EMITTED", "LIGHT_1", why="before")
    t.same("WATER_0", why="light first")
    t.step(n)
    t.same("LIGHT_1", rect=(7, 3, 100, 20))
    t.option("KERNEL_SET", 0)
    t.h.step(0)  # the per-pass kernels' layout of the light textures, nothing else
    t.option("KERNEL_SET", 1)
    t.same("WATER_0", "LIGHT_0", "WATER_0", why="after a step of no iterations")
    t.same(*ALL_FIELDS)
    t.close()


def test_pending_fields_belong_to_the_parameters_of_their_iteration(pkg, oracle, E):
    """Two steps with nothing read in between, then new parameters (sliders, sun angle, another initial_T row, the iteration counter):
    WATER_0, EMITTED and BASE_DISP asked for afterwards are those of the iteration that ran."""
    X, Y = 300, 80
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y, cloud=True), _uniforms(pkg, Y), iter0=98)
    t.step(3)
    t.step(2)  # (ends on iteration 102: the boundary pass's % 100 / % 20 schedules lie inside)
    u2 = _uniforms(pkg, Y, sunAngle=120.0, dryLapseRate=8.0, IR_rate=4.0, waterTemperature=31.0, greenhouseGases=0.004, sunIntensity=1.7)
    t.params(u2)
    t.h.iter = t.o.iter = 5000
    t.same("EMITTED", "WATER_0", "BASE_DISP", why="old parameters")
    t.params(_uniforms(pkg, Y, sunAngle=200.0, dryLapseRate=6.5))  # (a second initial_T row before the first was ever used)
    t.same("WATER_0", "EMITTED", why="twice")
    t.step(1)
    t.same(*ALL_FIELDS, "EMITTED", why="new parameters")
    assert t.h.iter == 5001
    t.close()


def test_kernel_set_switched_with_display_fields_pending(pkg, oracle, E):
    """marching -> per-pass -> marching: the field mapping, the layout of the light textures and the assembly of BASE_DISP flip with it;
    at every switch WATER_0 / BASE_DISP / EMITTED of the last step are still unread."""
    X, Y = 260, 70
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y, cloud=True), _uniforms(pkg, Y))
    t.step(3)
    t.option("KERNEL_SET", 0)
    t.same("BASE_DISP", "WATER_0", "EMITTED", "WALL_DISP", why="marching step, per-pass selected")
    t.step(2)
    t.option("KERNEL_SET", 1)
    t.same("EMITTED", "WATER_0", "BASE_DISP", "WALL_DISP", "LIGHT_0", why="per-pass step, marching selected")
    a, b = t.h.read_rect("VORT"), t.o.field("VORT")
    assert np.array_equal(a, b)
    t.step(3)
    t.option("KERNEL_SET", 0)
    t.step(1)
    t.option("KERNEL_SET", 1)
    t.step(1, 4)  # a piece that stores no display-side field ...
    t.step(2)     # ... and the one that does
    t.same(*ALL_FIELDS, "EMITTED")
    t.close()


def test_dry_pairs_switched_at_an_odd_count_and_iter_set_between_pairs(pkg, oracle, E):
    X, Y = 420, 64
    state = pkg.synth.dry_grid(X, Y, flow_sigma=0.3)
    u = _uniforms(pkg, Y, pass_mask=pkg.params.PASS_DRY)
    t = Pair(pkg, oracle, E, X, Y, state, u, DRY_PAIRS=1)
    t.h.profile(True)
    t.step(3)  # a pair and a single iteration
    t.option("DRY_PAIRS", 0)
    t.step(3)
    t.same("BASE_DISP", "BASE_CUR")
    t.option("DRY_PAIRS", 1)
    t.h.iter = t.o.iter = 99
    t.step(4)
    t.h.iter = t.o.iter = 18
    t.step(5)
    t.same(*DRY_FIELDS)
    prof = t.h.profile_read()
    assert prof["march_dry2_two_iterations_per_launch"][1] == 1 + 2 + 2, prof
    assert t.h.water_free()
    t.close()


def test_pass_mask_dry_all_dry_on_one_handle(pkg, oracle, E):
    """The water-free shortcut of the dry stencil holds until a step can make water, and does not come back."""
    X, Y = 300, 72
    state = pkg.synth.dry_grid(X, Y, flow_sigma=0.2)
    dry, wet = _uniforms(pkg, Y, pass_mask=pkg.params.PASS_DRY), _uniforms(pkg, Y)
    t = Pair(pkg, oracle, E, X, Y, state, dry)
    t.h.profile(True)
    t.step(4)
    assert t.h.water_free() and "march_dry2_two_iterations_per_launch" in t.h.profile_read()
    t.params(wet)
    t.step(3)
    assert not t.h.water_free()
    t.same(*ALL_FIELDS, "EMITTED", why="all passes")
    t.params(dry)
    t.h.profile(True)
    t.step(4)
    assert not t.h.water_free()
    names = t.h.profile_read()
    assert set(names) == {"fused_dry_vel_advect_pressure"}, names  # (the water-carrying dry kernel: neither marching one)
    t.same(*DRY_FIELDS, why="dry again")
    assert not t.h.read_rect("EMITTED").any()  # (include/wxsim.h: no lighting pass in the last step)
    t.params(wet)
    t.step(2)
    t.same(*ALL_FIELDS, "EMITTED", why="all passes again")
    t.close()


def test_precipitation_switched_off_and_on(pkg, oracle, E):
    X, Y = 256, 96
    drops = pkg.synth.init_rain_drops(800)
    rng = np.random.Generator(np.random.Philox(4))
    drops[:400, 0] = rng.uniform(-1, 1, 400).astype(np.float32)
    drops[:400, 1] = rng.uniform(-0.6, 0.2, 400).astype(np.float32)
    drops[:400, 2] = rng.uniform(0.1, 1.0, 400).astype(np.float32)
    drops[:400, 3] = 0.0
    drops[:400, 4] = 1.0
    on = dict(_uniforms(pkg, Y, drops=True), inactiveDroplets=400.0)
    off = dict(on, enablePrecipitation=0)
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y, cloud=True), on, drops=drops)
    t.step(3)
    assert t.o.field("PRECIP_FB").any()
    t.h.set_lightning([0.3, 0.4, 2.0, 0.7])
    t.o.set_lightning([0.3, 0.4, 2.0, 0.7])
    t.same("PRECIP_FB", "PRECIP_DEP", "LIGHTNING", why="on")
    t.params(off)
    t.step(2)
    assert not t.o.field("PRECIP_FB").any()
    t.same("PRECIP_FB", "PRECIP_DEP", "WATER_0", why="off")
    t.same()
    t.params(on)
    t.step(3)
    t.same(*ALL_FIELDS, "LIGHTNING", why="on again")
    t.same()
    t.close()


def test_row_bands_changed_between_steps(pkg, oracle, E):
    X, Y = 200, 520
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y), _uniforms(pkg, Y), ROW_BANDS=1)
    for bands in (2, 0, 1):
        t.step(2)
        t.option("ROW_BANDS", bands)
        t.same("WATER_0", why=f"before bands {bands}")
        t.step(1)
        t.same(*ALL_FIELDS, why=f"bands {bands}")
    t.close()


def test_tune_placement_with_water0_pending_and_profiling_on(pkg, oracle, E):
    X, Y = 330, 96
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y), _uniforms(pkg, Y))
    t.h.profile(True)
    t.step(5)
    assert t.h.profile_read()["march_wet_full_iteration"][1] == 5
    t.h.tune_placement(2, 2)
    assert t.h.iter == 5
    assert "march_wet_full_iteration" not in t.h.profile_read()  # (the probes' launches are not the caller's)
    t.same("WATER_0", "BASE_DISP", "EMITTED", *ALL_FIELDS, why="after the search")
    t.step(2)
    t.same(*ALL_FIELDS)
    t.close()


def test_tune_placement_in_pair_mode_leaves_the_pair_counters(pkg, oracle, E):
    """The probes of a placement search run the handle's own iteration -- pairs with fast cells here -- and none of it shows in
    wx_pair_stats: the counters equal those of an untuned twin over the same steps."""
    X, Y = 420, 64
    state = pkg.synth.dry_grid(X, Y, flow_sigma=0.35)
    u = _uniforms(pkg, Y, pass_mask=pkg.params.PASS_DRY)
    t, twin = (Pair(pkg, oracle, E, X, Y, state, u, DRY_PAIRS=1) for _ in range(2))
    for p in (t, twin):
        p.step(3)  # an odd count: the next pair starts on iteration 3
    t.h.tune_placement(2, 3)
    for p in (t, twin):
        p.step(4)
    stats, want = t.h.pair_stats(), twin.h.pair_stats()
    assert want[0] > 0, "sigma 0.35 puts second-iteration cells beyond 0.9 cells / iteration"
    assert stats == want
    t.h.tune_placement(1, 2)
    assert t.h.pair_stats() == (0, 0)
    t.same(*DRY_FIELDS)
    for p in (t, twin):
        p.close()


@pytest.mark.parametrize("how", ["eddies", "vortices"])
def test_device_write_then_base_disp(pkg, oracle, E, how):
    """A host that edits velocities in place through wx_device_ptr(BASE_CUR) (devtools.seed_flow / seed_vortices) changes
    baseTexture_0 and nothing else: baseTexture_1 of the last display iteration -- assembled on demand after the marching wet kernel --
    stays what that iteration made (found by tools/fuzz_parity.py --mode script)."""
    devtools = importlib.import_module(pkg.__name__ + ".devtools")
    X, Y = 300, 90
    t = Pair(pkg, oracle, E, X, Y, _scene(pkg, X, Y), _uniforms(pkg, Y))
    t.step(3)
    if how == "eddies":
        devtools.seed_flow(t.h, 0.3, seed=7)
    else:
        devtools.seed_vortices(t.h, 2, peak=1.2, radius=3.0, seed=7)
    written = t.h.read_rect("BASE_CUR")
    assert not np.array_equal(written, t.o.field("BASE_CUR"))
    t.o.view("BASE_CUR")[...] = written
    t.same("BASE_DISP", rect=(10, 5, 200, 60), why="after the write")
    t.same(*ALL_FIELDS, "EMITTED", why="after the write")
    t.step(2)
    t.same(*ALL_FIELDS, "EMITTED")
    t.close()


def test_read_particles_reports_an_overflowed_exact_path(pkg, E):
    """A blocking call that hands out state reports what the iterations left to report: after a step whose exact-path list overflowed
    the droplets belong to a wrong grid, and wx_read_particles says so instead of returning them (found by tools/fuzz_parity.py
    --mode script: a host that read particles first got the pool of a state that the next wx_read_rect refused)."""
    X, Y = 384, 128
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    base[40:110, :, 1] = 1.5
    base[40:110, :, 0] = -1.2
    u = _uniforms(pkg, Y, drops=True)
    h = E.Handle(X, Y, 256)
    h.set_option(h.OPT_FIX_CAP, 1000)
    h.upload(base, water, wall, pkg.synth.init_rain_drops(256))
    h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
    h.step(2)
    with pytest.raises(E.WxError) as ei:
        h.read_particles(10, 20)
    assert ei.value.code == -5 and "exact path holds" in str(ei.value)
    h.close()
