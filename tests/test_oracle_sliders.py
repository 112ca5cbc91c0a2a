"""CPU oracle vs the reference's own output AWAY FROM THE DEFAULT SETTINGS (tests/golden/sliders64_*.npz, oracle/golden/gen_golden.py).

Every other fixture runs at (nearly) the GUI's defaults, and several defaults are multiplicative identities (IR_rate = 1,
aboveZeroThreshold = 1): a restatement that uses such a uniform in the wrong place agrees with the reference there by arithmetic.
The sliders64 family draws every control the simulation reads over the range the reference's GUI offers (params.GUI_RANGES, a
stratified draw: each control near its low end, near its high end and in between), half of the scenes without horizontal wrap
and with an input at the x edge, three with precipitation and hand-built droplets.

Two things are checked: the oracle reproduces the reference on every scene (tolerances stated per field below, none looser than
what tests/test_oracle_golden.py uses unless the reason stands next to the number), and -- computed by the test itself, every
run -- each uniform MATTERS to a compared field of some scene by at least 100 x the tolerance that field is compared with
(test_every_uniform_moves_a_compared_field_by_100_tolerances; the table it prints is quoted in DESIGN.md section 2).
"""

import numpy as np
import pytest

ULP_T = 3.0518e-05  # fp32 ulp at ~300 K
NAMES = [f"sliders64_{k:02d}" for k in range(8)]
ITS = (1, 5, 20)
EPS = 1.1920929e-07


def _z(shape, dt=np.float32):
    return np.zeros(shape, dt)


def _uniforms(g, u):
    u = dict(u)
    u["varyings"] = g["varyings"]  # fragCoord / texCoord as the reference's rasteriser interpolated them
    u["subpixel_bits"] = 4  # SwiftShader snaps point sprites to 1/16 px
    return u


def tolerances(g, u):
    """key -> tolerance against the reference; 0 = bit for bit. Keys: "it<N>:<field>" of the run, "pp:<pass>_<field>" of iteration 0
    pass by pass on the reference's own intermediate textures."""
    precip = int(g["precip"])
    ir = max(1.0, float(u["IR_rate"]))
    t = {}
    for it in ITS:
        t[f"it{it}:v"] = 5e-7 if it <= 5 else 1e-6  # test_synth64: 5e-7 at 10 iterations; test_sounding64: 1e-6 at 10 (these scenes carry its forcing too)
        t[f"it{it}:P"] = 5e-7 if it <= 5 else 1e-6
        t[f"it{it}:T"] = 4 * ULP_T   # test_synth64
        t[f"it{it}:vapour_cloud"] = 5e-5  # test_synth64: cloud water where it is evaporating, pow() ulps amplified
        # precipitation / smoke in air, soil moisture / snow in walls. test_synth64: 1e-6 at 10 iterations; twice that at twice the
        # iterations. With droplets the precipitation channel takes the particle feedback, a sum of 144-texel splats of cbrt() / pow()
        # results: 2e-5 (measured 1.3e-5).
        t[f"it{it}:precip_smoke"] = 2e-5 if precip else (1e-6 if it <= 5 else 2e-6)
        t[f"it{it}:sunlight"] = 0.02  # test_save100: 0.25 (LINEAR-filter weight precision); here 1e-5 of up to 2600 W/m2
        # test_save100: IR 0.2, net heating 1e-7 -- the latter times IR_rate here, which multiplies the whole term
        # (lightingShader.frag:152). At 20 iterations a trace of evaporating cloud that differs by 2e-5 (inside the bound above)
        # changes its cell's emissivity, 5 x cloud x 300 / Y, by 6e-4: 0.12 W/m2 of IR and 6e-7 of heating in that cell and the
        # two above it (measured in sliders64_05 at (55, 3); 1e-7 x IR_rate everywhere else). IR keeps test_save100's bound there.
        t[f"it{it}:net_heating"] = (1e-7 if it <= 5 else 4e-7) * ir
        t[f"it{it}:IR"] = 0.05 if it <= 5 else 0.2
        if precip:
            # test_precip64: 2.5e-7 after one iteration (cbrt / pow ulps on masses). At 20 iterations positions have integrated
            # 20 velocities that differ by up to 5e-7 each, scaled 2 / X: 5e-6 (measured 2.8e-6)
            t[f"it{it}:drops"] = {1: 2.5e-7, 5: 2e-6, 20: 5e-6}[it]  # (measured 6e-8, 1.1e-6, 2.8e-6)
            t[f"it{it}:precip_fb"] = 1e-8 if it <= 5 else 2e-8  # test_precip64: 1e-8 (fp32 sum order of overlapping splats) at iteration 1
            t[f"it{it}:precip_dep"] = 0.0 if it == 1 else 1e-8  # test_precip64: exact at iteration 1; later the deposited masses carry growth ulps
    t.update({"pp:velocity_base": 0.0, "pp:vort": 0.0, "pp:boundary_vP": 0.0, "pp:boundary_T": ULP_T, "pp:boundary_water": 1e-6,
              "pp:advection_vP": 0.0, "pp:advection_T": 2 * ULP_T, "pp:advection_water": 4e-6,  # test_randwalls64p: 4e-6 (GL_POINT-drawn)
              "pp:pressure_base": 0.0, "pp:lighting_sunlight": 0.0, "pp:lighting_net_heating": 2e-9 * ir, "pp:lighting_IR": 1e-3})
    if precip:
        t.update({"pp:precip_drops": 2.5e-7, "pp:precip_fb": 1e-8, "pp:precip_dep": 0.0})
    return t


def outputs(oracle, g, u):
    """Everything that is compared, as the oracle computes it under the uniforms ``u``: key -> array (walls under "...:wall")."""
    u = _uniforms(g, u)
    X, Y = int(g["X"]), int(g["Y"])
    precip = int(g["precip"])
    nd = len(g["in_drops"]) if precip else 0
    out = {}
    s = oracle.OracleSim(X, Y, nd)
    s.upload(g["in_base"], g["in_water"], g["in_wall"], g["in_drops"] if nd else None)
    s.set_params(u)
    s.iter = int(g["iter0"])
    done = 0
    for it in ITS:
        s.step(it - done)
        done = it
        b, w, l = s.field("BASE_CUR"), s.field("WATER_CUR"), s.field("LIGHT_1")
        out.update({f"it{it}:wall": s.field("WALL_CUR"), f"it{it}:v": b[..., :2], f"it{it}:P": b[..., 2], f"it{it}:T": b[..., 3],
                    f"it{it}:vapour_cloud": w[..., :2], f"it{it}:precip_smoke": w[..., 2:], f"it{it}:sunlight": l[..., 0],
                    f"it{it}:net_heating": l[..., 1], f"it{it}:IR": l[..., 2:]})
        if precip:
            out.update({f"it{it}:drops": s.field("DROPS"), f"it{it}:precip_fb": s.field("PRECIP_FB"), f"it{it}:precip_dep": s.field("PRECIP_DEP")})
    s.close()
    # iteration 0 pass by pass, each pass on the reference's output of the one before (light, feedback, deposition are still zero)
    L, p = oracle.lib(), oracle.make_params(u, X, Y)
    it0 = float(g["iter0"])
    bo, wo = _z((Y, X, 4)), _z((Y, X, 4), np.int8)
    L.wxo_velocity(p, g["in_base"].ravel(), g["in_wall"].ravel(), bo.ravel(), wo.ravel())
    out["pp:velocity_base"] = bo
    cu, vo = _z((Y, X)), _z((Y, X, 2))
    L.wxo_curl(p, g["pp_velocity_base"].ravel(), cu.ravel())
    L.wxo_vorticity(p, cu.ravel(), vo.ravel())
    out["pp:vort"] = vo
    bo, wa, wl = _z((Y, X, 4)), _z((Y, X, 4)), _z((Y, X, 4), np.int8)
    L.wxo_boundary(p, u["initial_T"], it0, g["pp_velocity_base"].ravel(), g["in_water"].ravel(), g["pp_vort"].ravel(),
                   np.ascontiguousarray(g["in_wall"]).ravel(), _z(Y * X * 4), _z(Y * X * 4), _z(Y * X * 2), bo.ravel(), wa.ravel(), wl.ravel())
    out.update({"pp:boundary_wall": wl, "pp:boundary_vP": bo[..., :3], "pp:boundary_T": bo[..., 3], "pp:boundary_water": wa})
    bo, wa, wl = _z((Y, X, 4)), _z((Y, X, 4)), _z((Y, X, 4), np.int8)
    snd = [np.ascontiguousarray(u[k], np.float32) for k in ("sounding_T", "sounding_W", "sounding_Vel")]
    L.wxo_advection(p, u["initial_T"], *[a.ctypes.data for a in snd], g["pp_boundary_base"].ravel(), g["pp_boundary_water"].ravel(),
                    g["pp_boundary_wall"].ravel(), bo.ravel(), wa.ravel(), wl.ravel())
    out.update({"pp:advection_wall": wl, "pp:advection_vP": bo[..., :3], "pp:advection_T": bo[..., 3], "pp:advection_water": wa})
    bo, wl2 = _z((Y, X, 4)), _z((Y, X, 4), np.int8)
    L.wxo_pressure(p, g["pp_advection_base"].ravel(), g["pp_advection_wall"].ravel(), bo.ravel(), wl2.ravel())
    out["pp:pressure_base"] = bo
    lo = _z((Y, X, 4))
    L.wxo_lighting(p, g["pp_advection_base"].ravel(), g["pp_advection_water"].ravel(), g["pp_advection_wall"].ravel(), _z(Y * X * 4), lo.ravel())
    out.update({"pp:lighting_sunlight": lo[..., 0], "pp:lighting_net_heating": lo[..., 1], "pp:lighting_IR": lo[..., 2:]})
    if precip:
        d, fb, dep = _z((nd, 5)), _z((Y, X, 4)), _z((Y, X, 2))
        L.wxo_precipitation(p, it0, nd, g["in_drops"].ravel(), g["pp_advection_base"].ravel(), g["pp_advection_water"].ravel(), _z(4), d.ravel(), fb.ravel(), dep.ravel())
        out.update({"pp:precip_drops": d, "pp:precip_fb": fb, "pp:precip_dep": dep})
    return out


def reference(g):
    """The same keys from the fixture: what the reference's shaders rendered."""
    r = {}
    for it in ITS:
        b, w, l = g[f"it{it}_base_cur"], g[f"it{it}_water_cur"], g[f"it{it}_light_1"]
        r.update({f"it{it}:wall": g[f"it{it}_wall_cur"], f"it{it}:v": b[..., :2], f"it{it}:P": b[..., 2], f"it{it}:T": b[..., 3],
                  f"it{it}:vapour_cloud": w[..., :2], f"it{it}:precip_smoke": w[..., 2:], f"it{it}:sunlight": l[..., 0],
                  f"it{it}:net_heating": l[..., 1], f"it{it}:IR": l[..., 2:]})
        if int(g["precip"]):
            r.update({f"it{it}:drops": g[f"it{it}_drops"], f"it{it}:precip_fb": g[f"it{it}_precip_fb"], f"it{it}:precip_dep": g[f"it{it}_precip_dep"]})
    bb, ab, ll = g["pp_boundary_base"], g["pp_advection_base"], g["pp_lighting_light"]
    r.update({"pp:velocity_base": g["pp_velocity_base"], "pp:vort": g["pp_vort"], "pp:boundary_wall": g["pp_boundary_wall"],
              "pp:boundary_vP": bb[..., :3], "pp:boundary_T": bb[..., 3], "pp:boundary_water": g["pp_boundary_water"],
              "pp:advection_wall": g["pp_advection_wall"], "pp:advection_vP": ab[..., :3], "pp:advection_T": ab[..., 3],
              "pp:advection_water": g["pp_advection_water"], "pp:pressure_base": g["pp_pressure_base"],
              "pp:lighting_sunlight": ll[..., 0], "pp:lighting_net_heating": ll[..., 1], "pp:lighting_IR": ll[..., 2:]})
    if int(g["precip"]):
        r.update({"pp:precip_drops": g["pp_precip_drops"], "pp:precip_fb": g["pp_precip_fb"], "pp:precip_dep": g["pp_precip_dep"]})
    return r


def check_against_reference(out, g, u):
    """Shared with tests/test_gpu_parity.py (there ``out`` comes from the HIP engine): every key within its tolerance."""
    ref, tol = reference(g), tolerances(g, u)
    bad = []
    for k, r in ref.items():
        if k not in out:
            continue
        if k.endswith("wall") or tol[k] == 0.0:
            if not np.array_equal(out[k], r):
                bad.append((k, "not bit-exact", float(np.abs(out[k].astype(np.float64) - r).max())))
        else:
            e = float(np.abs(out[k] - r).max())
            if not e <= tol[k]:
                bad.append((k, e, tol[k]))
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_off_default(oracle, golden, name):
    g, u = golden(name)
    assert int(g["points"]) == 1
    out = outputs(oracle, g, u)
    assert set(reference(g)) == set(out)
    assert check_against_reference(out, g, u) == []
    # the inputs the scenes exist for did act: walls changed (%100 rules, brush), and in the scenes with droplets some spawned,
    # some deposited, one left through the bottom edge
    if int(g["precip"]):
        d0, d20 = g["in_drops"], g["it20_drops"]
        assert ((d0[:, 2] < 0) & (d20[:, 2] >= 0)).sum() >= 5 and np.abs(g["it20_precip_dep"]).max() > 0 or np.abs(g["it5_precip_dep"]).max() > 0
        assert d0[20, 1] < -1.0 and g["it1_drops"][20, 2] < 0 and np.abs(g["pp_precip_dep"]).max() > 0


def test_family_covers_the_gui_ranges(pkg, golden):
    """Every control: a scene in the lowest and one in the highest 6 % of its GUI range, interior ones, never the default; both values
    of the three booleans; sun at noon, low and below the horizon; the runs cross iterNum % 100 == 0 and % 20 == 0."""
    P = pkg.params
    us = [golden(n) for n in NAMES]
    D = P.uniforms_from_gui(dict(P.GUI_DEFAULTS), 48)
    span = {k: P.GUI_RANGES[k] for k in P.GUI_RANGES if k not in ("simHeight", "sunAngle", "spawnChance", "waterTemperature", "sunIntensity")}
    span.update(spawnChanceMult=P.GUI_RANGES["spawnChance"], dryLapse=(50.0, 150.0), waterTemperature=(273.15, 313.15))
    for k, (lo, hi) in span.items():
        f = sorted((float(u[k]) - lo) / (hi - lo) for _, u in us)
        if k.startswith("globalEffects"):  # the GUI keeps start <= end: the pair is sorted after the draw
            assert f[0] < 0.1 or f[-1] > 0.9, k
            continue
        assert f[0] <= 0.0601 and f[-1] >= 0.9399 and sum(0.06 < v < 0.94 for v in f) >= 5, (k, f)
        assert all(abs(float(u[k]) - float(D[k])) > 0.015 * (hi - lo) for _, u in us), k
    for k in ("wrapHorizontally", "enablePrecipitation", "dynamicWaterTemperature"):
        assert {int(u[k]) for _, u in us} == {0, 1}, k
    zen = sorted(float(u["sunAngle"]) for _, u in us)
    assert zen[0] < -np.pi / 2 and zen[-1] > np.pi / 2 and 0.0 in zen  # below the horizon on both sides, exactly overhead
    for g, u in us:
        i0 = int(g["iter0"])
        assert any((i0 + i) % 100 == 0 for i in range(20)) and (u["wrapHorizontally"] or u["userInputType"] >= 0)


# ------------------------------------------------------------------------------------------------
# sensitivity: the pin means something only where the uniform moves what is compared
# ------------------------------------------------------------------------------------------------
# fields of wx_params the reference does not have: this project's own constructs
NOT_REFERENCE_UNIFORMS = {"quad_scale": "fragCoord scale of the quad-drawn goldens, no uniform of the reference (tests/test_gpu_parity.py runs both values)",
                          "pass_mask": "the dry pass mask is this project's own construct; the reference cannot render it"}
# Uniforms no scene of 20 iterations can bring to the margin, with the floor that is asserted instead and why.
BELOW_100 = {"globalDrying": (50.0, "the GUI offers 0 .. 1e-4 per iteration: 20 iterations at the top of the range remove 2e-3 of vapour, against a bound of "
                                    "5e-5 on vapour / cloud (pow() ulps where cloud evaporates) and 2e-6 on the advected fields; sounding64 pins the term too")}
TENTH_IS_DISCRETE = {"aboveZeroThreshold": "enters only the spawn decision of inactive droplets over warm cloud (a few dozen decisions per scene): a tenth of the "
                                           "range flips none of them; the move back to the default does"}
BOOLEANS = ("wrapHorizontally", "enablePrecipitation", "dynamicWaterTemperature")


def _uniform_ranges(P, n_drops=256):
    r = {k: v for k, v in P.GUI_RANGES.items() if k not in ("simHeight", "sunAngle", "spawnChance")}
    r.update(spawnChanceMult=P.GUI_RANGES["spawnChance"], dryLapse=(50.0, 150.0), waterTemperature=(273.15, 313.15),
             sunIntensity=(0.0, 2600.0), sunAngle=(-100.0 * P.DEG2RAD, 100.0 * P.DEG2RAD), inactiveDroplets=(0.0, float(n_drops)))  # (the host's count of the pool, app.js:5957-5966)
    return r


# What the particle pass reads (precipitationShader.vert). Every OTHER uniform is judged on the scenes without droplets and on the
# single passes of iteration 0 only: an inactive droplet spawns on fract(pow(cloud * 10, 2)), so in a run with droplets ANY change of
# the cloud field, however small, flips a spawn decision sooner or later and moves the droplet count by one -- that is chaos, not
# the uniform entering a formula, and it would hand every uniform a margin of 1e8.
PARTICLE_UNIFORMS = ("evapHeat", "meltingHeat", "dryLapse", "aboveZeroThreshold", "subZeroThreshold", "spawnChanceMult", "snowDensity", "fallSpeed",
                     "growthRate0C", "growthRate_30C", "freezingRate", "meltingRate", "evapRate", "inactiveDroplets", "enablePrecipitation")


def _margin(out, alt, tol, particle_uniform, precip_scene):
    """max over compared float fields of (how far the field moved) / (the tolerance it is compared with); fields compared bit for
    bit count with one ulp of their largest value."""
    best = (0.0, None)
    for k, t in tol.items():
        if not particle_uniform and (k.startswith("pp:precip") or (precip_scene and not k.startswith("pp:"))):
            continue
        move = float(np.abs(out[k].astype(np.float64) - alt[k]).max())
        t_eff = t if t > 0 else EPS * max(float(np.abs(out[k]).max()), 1e-30)
        if move / t_eff > best[0]:
            best = (move / t_eff, k)
    return best


def test_every_uniform_moves_a_compared_field_by_100_tolerances(pkg, oracle, golden, capsys):
    P = pkg.params
    D = P.uniforms_from_gui(dict(P.GUI_DEFAULTS), 48)
    fields = [f[0] for f in P.WxParams._fields_]
    assert set(NOT_REFERENCE_UNIFORMS) <= set(fields)
    R = _uniform_ranges(P)
    scenes = []
    for n in NAMES:
        g, u = golden(n)
        scenes.append((n, g, u, outputs(oracle, g, u), tolerances(g, u)))
    rows, failed = [], []
    for U in fields:
        if U in NOT_REFERENCE_UNIFORMS:
            continue
        best_d, best_t = (0.0, None, None), (0.0, None, None)
        for n, g, u, out, tol in scenes:
            same = np.array_equal(np.asarray(u[U], np.float64), np.asarray(D[U], np.float64))
            if U in BOOLEANS:
                alt = dict(u, **{U: 1 - int(u[U])})  # a boolean has no default to return to that every scene leaves: the other value
            elif same:
                alt = None
            else:
                alt = dict(u, **{U: D[U]})
            if alt is not None:
                m, k = _margin(out, outputs(oracle, g, alt), tol, U in PARTICLE_UNIFORMS, int(g["precip"]))
                if m > best_d[0]:
                    best_d = (m, n, k)
            if U in R:  # moved by a tenth of its range: does the VALUE enter rightly, not only whether it does
                lo, hi = R[U]
                v = float(u[U]) + 0.1 * (hi - lo)
                v = v if v <= hi else float(u[U]) - 0.1 * (hi - lo)
                m, k = _margin(out, outputs(oracle, g, dict(u, **{U: v})), tol, U in PARTICLE_UNIFORMS, int(g["precip"]))
                if m > best_t[0]:
                    best_t = (m, n, k)
        rows.append((U, best_d, best_t if U in R else None))
        if best_d[0] < BELOW_100.get(U, (100.0,))[0] or (U in R and U not in TENTH_IS_DISCRETE and best_t[0] < 10.0):
            failed.append(U)
    with capsys.disabled():
        print("\nuniform                   back to default: margin  scene        field                   | a tenth of the range: margin  scene        field")
        for U, d, t in rows:
            tt = f"{t[0]:12.3g}  {str(t[1])[-2:]:>5}  {t[2]}" if t else "           -  (an input, not a slider)"
            print(f"{U:25s} {d[0]:12.3g}  {str(d[1])[-2:]:>5}  {str(d[2]):24s} | {tt}")
        for U, why in NOT_REFERENCE_UNIFORMS.items():
            print(f"{U:25s} not checked: {why}")
        for U, (floor, why) in BELOW_100.items():
            print(f"{U:25s} floor {floor:g} instead of 100: {why}")
        for U, why in TENTH_IS_DISCRETE.items():
            print(f"{U:25s} tenth of the range not asserted: {why}")
    assert not failed, f"no sliders64 scene where these uniforms move a compared field by 100 x its tolerance (10 x for a tenth of the range): {failed}"


# ------------------------------------------------------------------------------------------------
# lightning requests under off-default settings, in both summation orders of the splats
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splat_order", [0, 1])
def test_lightning_requests_off_default_both_splat_orders(oracle, golden, splat_order):
    """precipitationShader.vert:121-140 iteration by iteration on the reference's own inputs (as test_lightning64: the strike decision
    hashes the bits of temperature and water) with snowDensity, meltingHeat, both thresholds and the rates off default. splat_order
    1 is the summation the HIP engine's deterministic mode computes: its 1-px sprite on texel (1,0) takes the request."""
    g, u = golden("sliders64_lightning")
    u = dict(_uniforms(g, u), splat_order=splat_order)
    X, Y, n = int(g["X"]), int(g["Y"]), len(g["in_drops"])
    L, p = oracle.lib(), oracle.make_params(u, X, Y)
    drops, light = g["in_drops"].copy(), np.zeros(4, np.float32)
    requests = 0
    for k in range(1, int(g["niter"]) + 1):
        it = float(int(g["iter0"]) + k - 1)
        d_out, fb, dep = _z((n, 5)), _z((Y, X, 4)), _z((Y, X, 2))
        L.wxo_precipitation(p, it, n, drops.ravel(), g[f"it{k}_base_disp"].ravel(), g[f"it{k}_water_cur"].ravel(), light, d_out.ravel(), fb.ravel(), dep.ravel())
        L.wxo_lightning_location(p, it, fb.ravel(), light)
        rd, rfb, rl = g[f"it{k}_drops"], g[f"it{k}_precip_fb"], g[f"it{k}_lightning"]
        flip = np.abs(d_out - rd).max(1) > 2.5e-7  # a spawn decision within one pow() ulp of its threshold (see test_lightning64)
        assert flip.sum() <= 2, (k, int(flip.sum()))
        assert np.array_equal((d_out[:, 2] >= 0)[~flip], (rd[:, 2] >= 0)[~flip])
        assert abs(fb[0, 0, 0] - rfb[0, 0, 0]) <= flip.sum(), k
        if not flip.any():
            assert np.array_equal(fb[0, 1], rfb[0, 1]), (k, fb[0, 1], rfb[0, 1])  # the request texel: sums of identical terms, exact
            assert np.abs(fb - rfb).max() <= (1e-8 if splat_order == 0 else 2e-7 * max(1.0, float(np.abs(rfb[1:]).max())))
        assert np.array_equal(light, rl), (k, light, rl)
        requests += int(rfb[0, 1, 2] != 0)
        drops, light = rd.copy(), rl.copy()
    assert requests >= 2 and np.abs(g[f"it{int(g['niter'])}_lightning"]).max() > 0
