"""Diagnostics on the device (wx_diagnostics / wx_group_diagnostics): every member == the same quantity computed here from plain
readbacks with numpy masks and math.fsum -- sums compared on their bits --, for whole handles and for slabs; planted values; no side
effects on the handle; misuse; one full-size case."""
import ctypes as C
import math

import numpy as np
import pytest

from test_diag_cpu import assert_matches, bits, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(pkg):
    pkg.engine.build()
    return pkg.engine


def expected(h, drops=True):
    want = reference(h.read_rect("BASE_CUR"), h.read_rect("WATER_CUR"), h.read_rect("WALL_CUR"))
    want["iter"] = h.iter
    if drops and h.n_droplets:
        d = h.read_particles()
        act = d[:, 2] >= 0
        want["n_droplets_active"] = int(act.sum())
        want["n_droplets_nonfinite"] = int((act & ~(np.isfinite(d[:, 2]) & np.isfinite(d[:, 3]))).sum())
        want["sum_droplet_mass_x"] = math.fsum(float(t) for t in d[act & np.isfinite(d[:, 2]), 2])
        want["sum_droplet_mass_y"] = math.fsum(float(t) for t in d[act & np.isfinite(d[:, 3]), 3])
    return want


def handle_of(pkg, E, X, Y, base, water, wall, u, drops=None, iter0=0):
    h = E.Handle(X, Y, 0 if drops is None else len(drops))
    h.upload(base, water, wall, drops)
    h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"], u.get("sounding_T"), u.get("sounding_W"), u.get("sounding_Vel"))
    h.iter = iter0
    return h


def terrain_scene(pkg, X, Y, seed=2):
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    rng = np.random.default_rng(seed)
    air = wall[..., 1] != 0
    base[..., 0] += np.where(air, rng.normal(0, 0.2, (Y, X)), 0).astype(np.float32)
    base[..., 1] += np.where(air, rng.normal(0, 0.1, (Y, X)), 0).astype(np.float32)
    water[..., 3] += np.where(air, rng.uniform(0, 2, (Y, X)), 0).astype(np.float32)  # smoke
    gui = pkg.params.merge_settings(None)
    gui["sunAngle"] = 35.0
    u = pkg.params.uniforms_from_gui(gui, Y, quad_scale=0)
    u["enablePrecipitation"] = 0
    return base, water, wall, u


@pytest.mark.parametrize("name,steps", [("synth64", 50), ("randwalls64p", 50), ("precip64", 4), ("save100qa", 300)])
def test_committed_scenes_equal_readback_and_fsum(pkg, golden, E, name, steps):
    g, u = golden(name)
    X, Y = int(g["X"]), int(g["Y"])
    drops = g["in_drops"] if "in_drops" in g.files else None
    if drops is None:
        u = dict(u, enablePrecipitation=0)
    h = handle_of(pkg, E, X, Y, g["in_base"], g["in_water"], g["in_wall"], u, drops, int(g["iter0"]))
    assert_matches(h.diagnostics(), expected(h))  # the uploaded state
    h.step(steps)
    got = h.diagnostics()
    assert_matches(got, expected(h))
    assert got["n_air"] + got["n_wall"] == X * Y and got["iter"] == int(g["iter0"]) + steps
    if drops is not None:
        assert got["n_droplets_active"] > 0 and got["sum_droplet_mass_x"] > 0
    assert E.diag_finish(h.diagnostics_raw()) == got
    h.close()


@pytest.mark.parametrize("X,Y", [(2500, 300), (1000, 77)])
def test_terrain_after_50_iterations(pkg, E, X, Y):
    """A width that is no multiple of the 256-cell chunk (or of 64) and an odd height: partial waves at every row end."""
    base, water, wall, u = terrain_scene(pkg, X, Y)
    h = handle_of(pkg, E, X, Y, base, water, wall, u)
    h.step(50)
    assert_matches(h.diagnostics(), expected(h))
    h.close()


@pytest.mark.parametrize("mixed", [False, True], ids=["uniform_rows", "mixed_exponents_in_a_wave"])
def test_planted_values(pkg, E, mixed):
    """Known values in valid cells, through upload. ``mixed``: exponents 100 apart inside every 64-cell stretch of a row (the waves'
    lane-by-lane path into the LDS bins); otherwise every row holds one value per channel (the waves' register path)."""
    X, Y = 700, 40
    base = np.zeros((Y, X, 4), np.float32)
    water = np.zeros((Y, X, 4), np.float32)
    wall = np.zeros((Y, X, 4), np.int8)
    wall[..., 1] = 1
    wall[0, :, 1], wall[0, :, 3], water[0, :, 0] = 0, 7, 1111.0
    water[0, :, 2], water[0, :, 3] = 0.25, 3.0
    n_air = X * (Y - 1)
    yy = np.arange(Y, dtype=np.float32)[:, None]
    base[..., 3] = 250.0 + yy
    water[1:, :, 0] = 0.5
    if mixed:
        pattern = np.array([2.0 ** -60, 2.0 ** 40, -(2.0 ** 40), 1.5, 2.0 ** -100, -(2.0 ** -100), 3.0, 2.0 ** -140], np.float32)
        base[1:, :, 0] = np.resize(pattern, X)
    tiny = np.array([5], np.uint32).view(np.float32)[0]  # a subnormal
    # the planted cells [y, x]
    base[5, 100:103, 0] = [3e38, -3e38, 1e-30]
    base[7, 650, 1] = np.nan
    base[2, 3, 2] = np.inf                       # the first non-finite base cell: (3, 2)
    base[30, 699, 2] = tiny
    base[9, 9, 3] = -0.0                         # the minimum of T: a zero
    water[12, 345, 0] = -1.25                    # negative water
    water[0, 77, 0] = 3.0                        # a wall cell without its marker
    water[20, 5, 3] = np.float32(1e-42)          # subnormal smoke
    want_vx = math.fsum(float(t) for t in base[1:, :, 0].ravel())
    want_T = float(X) * sum(250.0 + y for y in range(1, Y)) - 259.0
    h = E.Handle(X, Y, 0)
    h.upload(base, water, wall)
    got = h.diagnostics()
    assert got["n_air"] == n_air and got["n_wall"] == X and got["sum_vegetation"] == 7 * X
    assert got["n_marker_mismatch"] == 1 and got["n_negative_water"] == 1
    assert got["n_nonfinite_base"] == 2 and got["first_nonfinite_base"] == (3, 2) and got["n_nonfinite_water"] == 0 and got["first_nonfinite_water"] is None
    assert bits(got["sum_base"][0]) == bits(want_vx) and (mixed or want_vx == float(np.float32(1e-30)))
    assert got["sum_base"][1] == 0.0 and got["sum_base"][3] == want_T
    assert bits(got["sum_base"][2]) == bits(float(tiny))  # (+inf is counted, not added)
    assert got["max_base"][2] == math.inf and got["max_base_at"][2] == (3, 2)
    assert got["min_base"][3] == 0.0 and got["min_base_at"][3] == (9, 9) and got["max_base"][3] == 250.0 + Y - 1 and got["max_base_at"][3] == (0, Y - 1)
    assert got["max_base"][0] == float(np.float32(3e38)) and got["max_base_at"][0] == (100, 5) and got["min_base_at"][0] == (101, 5)
    assert got["min_base"][1] == 0.0 and got["min_base_at"][1] == (0, 1) and got["max_base_at"][1] == (0, 1)  # NaN skipped; ties: the first air cell
    assert got["sum_water"][0] == 0.5 * (n_air - 1) - 1.25 and got["min_water_at"][0] == (345, 12)
    assert bits(got["sum_water"][3]) == bits(float(np.float32(1e-42))) and got["max_water_at"][3] == (5, 20)
    assert got["sum_soil_moisture"] == 0.25 * X and got["sum_snow"] == 3.0 * X
    assert_matches(got, expected(h))  # ... and the whole struct against the readback
    h.close()


@pytest.mark.parametrize("nslab", [2, 3, 8])
def test_slabs_merge_to_the_bits_of_the_whole_domain(pkg, E, nslab):
    """Slab widths 1500, 1000 and 375: none a multiple of 64. Droplets off."""
    X, Y, halo = 3000, 64, 12
    base, water, wall, u = terrain_scene(pkg, X, Y)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
    g.upload(base, water, wall)
    g.set_params(p, u["initial_T"])
    whole = handle_of(pkg, E, X, Y, base, water, wall, u)
    for n in (7, 14):  # inside and at the end of an exchange period
        g.step(n)
        whole.step(n)
        got, want = g.diagnostics(), whole.diagnostics()
        assert got == want
        assert [bits(a) for a in got["sum_base"] + got["sum_water"]] == [bits(a) for a in want["sum_base"] + want["sum_water"]]
    raw = E.diag_empty()
    for h in reversed(g.slabs):  # the hosts' own merge, in another order
        raw = E.diag_merge(raw, h.diagnostics_raw())
    assert raw == whole.diagnostics_raw() and E.diag_finish(raw) == want
    assert_matches(want, expected(whole))
    g.close()
    whole.close()


def test_slabs_with_droplets_at_an_exchange(pkg, E):
    """With droplets the slabs' counts add up to the domain's where an exchange has just been applied: here with WX_OPT_POOL_EXACT and
    the deterministic splat order (bit-identical pools), after whole exchange periods."""
    from test_group_transport import _particle_scene
    X, Y, halo, N, nslab = 512, 128, 64, 6000, 4
    base, water, wall, drops, u = _particle_scene(pkg, X, Y, N)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL, n_droplets=N)
    g.upload(base, water, wall, drops)
    g.set_params(p, u["initial_T"])
    g.set_option(E.Handle.OPT_SPLAT_ORDER, 1)
    g.set_option(E.Handle.OPT_POOL_EXACT, 1)
    whole = handle_of(pkg, E, X, Y, base, water, wall, u, drops)
    whole.set_option(whole.OPT_SPLAT_ORDER, 1)
    per = 1 + (halo - 12) // 9
    for n in (per, 2 * per):
        g.step(n)
        whole.step(n)
        g.exchange()
        got, want = g.diagnostics(), whole.diagnostics()
        assert got == want
        assert want["n_droplets_active"] > 500
    assert_matches(want, expected(whole))
    g.close()
    whole.close()


FIELDS = ("BASE_CUR", "BASE_DISP", "WATER_0", "WATER_CUR", "WALL_CUR", "WALL_DISP", "LIGHT_0", "LIGHT_1", "CURL", "PRECIP_FB", "PRECIP_DEP")


@pytest.mark.parametrize("mode", ["march", "perpass", "dry_pairs"])
def test_diagnostics_change_nothing(pkg, golden, E, mode):
    """Two handles, one call sequence; one of them asks for diagnostics between every two calls: all reads are byte-identical."""
    drops = None
    if mode == "dry_pairs":
        X, Y = 320, 96
        u = pkg.params.uniforms_from_gui(pkg.params.merge_settings(None), Y, quad_scale=0, pass_mask=pkg.params.PASS_DRY)
        u["enablePrecipitation"] = 0
        base, water, wall = pkg.synth.dry_grid(X, Y, flow_sigma=0.2)
    else:
        g, u = golden("precip64")
        X, Y, base, water, wall, drops = int(g["X"]), int(g["Y"]), g["in_base"], g["in_water"], g["in_wall"], g["in_drops"]
    E.set_default_option(E.Handle.OPT_KERNEL_SET, 0 if mode == "perpass" else 1)
    try:
        hs = [handle_of(pkg, E, X, Y, base, water, wall, u, drops) for _ in range(2)]
    finally:
        E.set_default_option(E.Handle.OPT_KERNEL_SET, 1)
    if mode == "dry_pairs":
        for h in hs:
            h.set_option(h.OPT_DRY_PAIRS, 1)
    brush = dict(u, userInputType=3, userInputValues=(0.6, 0.3, 0.05, 6.0), userInputMove=(0.004, -0.002))
    reads = [[], []]

    def run(k, h, probe):
        def rd(f):
            reads[k].append(h.read_rect(f).tobytes())
            probe()

        for call in (lambda: h.step(1), lambda: rd("WATER_0"), lambda: h.step(10), lambda: rd("BASE_DISP"), lambda: rd("LIGHT_0"),
                     lambda: (h.stream_frame(), reads[k].append(h.stream_wait()["WATER_CUR"].tobytes())), lambda: setattr(h, "iter", 1000),
                     lambda: h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), brush), u["initial_T"]), lambda: h.step(1),
                     lambda: h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"]), lambda: h.step(10), lambda: h.step(1)):
            call()
            probe()

    seen = []
    run(0, hs[0], lambda: None)
    run(1, hs[1], lambda: seen.append(hs[1].diagnostics()))
    assert reads[0] == reads[1]
    for f in FIELDS:
        assert hs[0].read_rect(f).tobytes() == hs[1].read_rect(f).tobytes(), f
    if drops is not None:
        assert hs[0].read_particles().tobytes() == hs[1].read_particles().tobytes()
    assert hs[0].iter == hs[1].iter == 1012 and seen[-1]["iter"] == 1012 and len({d["iter"] for d in seen}) > 4
    assert hs[0].diagnostics() == seen[-1]
    for h in hs:
        h.close()


def test_misuse_returns_codes(pkg, E):
    L = E.lib()
    h = E.Handle(64, 32, 0)
    d, raw = E.WxDiag(), E.WxDiagRaw()
    assert L.wx_diagnostics(h._h, C.byref(d)) == -5 and b"before wx_upload" in L.wx_last_error(h._h)  # WX_E_STATE
    assert L.wx_diag_collect(h._h, C.byref(raw)) == -5
    assert L.wx_diagnostics(h._h, None) == -1 and L.wx_diag_collect(h._h, None) == -1
    with pytest.raises(E.WxError) as ei:
        h.diagnostics()
    assert ei.value.code == -5
    h.close()
    g = E.Group(2, 256, 32, halo=12, devices=[0, 0], transport=E.TRANSPORT_LOCAL)
    assert L.wx_group_diagnostics(g._g, None) == -1
    assert L.wx_group_diagnostics(g._g, C.byref(d)) == -5 and b"before wx_upload" in L.wx_group_last_error(g._g)
    g.close()
    with pytest.raises(E.WxError) as ei:  # a destroyed group: the binding passes NULL, the library touches nothing
        g.diagnostics()
    assert ei.value.code == -1


def test_full_size_group_equals_whole_handle(pkg, E):
    """16384 x 2048, 20 iterations: eight slabs == the whole handle, every member; the sums against numpy's float64 sums of a readback."""
    from test_gpu_fullsize import _uniforms, _wet_state
    X, Y, nslab, halo = 16384, 2048, 8, 24
    base, water, wall = _wet_state(pkg, X, Y, seed=21)
    u = _uniforms(pkg, Y)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    whole = handle_of(pkg, E, X, Y, base, water, wall, u)
    whole.step(20)
    want = whole.diagnostics()
    b, w, wl = whole.read_rect("BASE_CUR"), whole.read_rect("WATER_CUR"), whole.read_rect("WALL_CUR")
    whole.close()
    air = wl[..., 1] != 0
    assert want["n_air"] == int(air.sum()) and want["n_wall"] == X * Y - want["n_air"] and want["n_nonfinite_base"] == 0
    for name, f in (("base", b), ("water", w)):
        for c in range(4):
            v = f[..., c]
            ref = float(np.sum(v, dtype=np.float64, where=air))
            scale = float(np.sum(np.abs(v), dtype=np.float64, where=air))
            assert abs(want["sum_" + name][c] - ref) <= 1e-12 * max(scale, 1e-300), (name, c)
            assert want["max_" + name][c] == float(v[air].max()) and want["min_" + name][c] == float(v[air].min())
            y, x = np.unravel_index(np.argmax(np.where(air, v, -np.inf)), v.shape)
            assert want["max_" + name + "_at"][c] == (int(x), int(y))
    del b, w, wl, air
    g = E.Group(nslab, X, Y, halo=halo, devices=[0] * nslab, transport=E.TRANSPORT_LOCAL)
    g.upload(base, water, wall)
    del base, water, wall
    g.set_params(p, u["initial_T"])
    g.step(20)
    assert g.diagnostics() == want
    g.close()
