"""CPU oracle vs the reference's own output on the SURFACE ROW's slow physics (tests/golden/surface*.npz, recipe in
oracle/golden/gen_golden.py): vegetation growth by rate and interval, fire spread / burn-down / rain, the industrial chimneys, dust, the
sea's temperature reset. Wall textures bit for bit at every dump, fields with the tolerances tests/test_oracle_sliders.py states --
and per scene an assertion, computed from the REFERENCE's arrays, that the event the scene exists for is there."""
import numpy as np
import pytest

from test_oracle_sliders import ULP_T

LAND, WATER, FIRE, URBAN, INDUSTRIAL = 1, 2, 3, 4, 6
DUMPS = {"surface64_growth": (70, 71, 75), "surface64_growth10k": (70, 71, 75), "surface64_fire": (1, 5, 6, 7, 11, 12),
         "surface64_spread": (5, 6, 105, 106, 205, 206, 305, 306, 310), "surface112_industry": (1, 10)}


def _oracle_run(oracle, g, u, its):
    X, Y = int(g["X"]), int(g["Y"])
    u = dict(u, varyings=g["varyings"], subpixel_bits=4)
    o = oracle.OracleSim(X, Y, 0)
    o.upload(g["in_base"], g["in_water"], g["in_wall"])
    o.set_params(u)
    o.iter = int(g["iter0"])
    done, out = 0, {}
    for it in its:
        o.step(it - done)
        done = it
        out[it] = (o.field("BASE_CUR"), o.field("WATER_CUR"), o.field("WALL_CUR"), o.field("LIGHT_0"), o.field("LIGHT_1"))
    o.close()
    return out


def check_fields(out, g, its):
    """``out``: dump -> (base, water, wall, light_0, light_1) of the implementation under test: the oracle here, the HIP engine in
    tests/test_gpu_parity.py::test_vs_reference_surface_scenes. Walls always bit for bit; base / water / light where the fixture
    keeps them. Measured: the oracle agrees with four of the five fixtures to 0.0 on every field; in surface112_industry the vapour
    of the AIR cells over the sea uploaded at 600 K (300 g / kg) differs by 10 ulp of its value -- the relative term."""
    bad = []
    for it in its:
        if not np.array_equal(out[it][2], g[f"it{it}_wall_cur"]):
            bad.append((it, "wall", int((out[it][2] != g[f"it{it}_wall_cur"]).sum())))
        if f"it{it}_base_cur" not in g.files:
            continue
        b, w, rb, rw = out[it][0], out[it][1], g[f"it{it}_base_cur"], g[f"it{it}_water_cur"]
        few, long = it <= 5, it > 20  # (long: surface64_spread's dump after 310 iterations, smoke of a fire accumulated: measured 6.1e-5 / 2.5e-5)
        # tests/test_oracle_sliders.py: v, P 5e-7 up to 5 iterations, 1e-6 beyond; T 4 ulp; vapour / cloud 5e-5; the other two water channels 1e-6 / 2e-6
        checks = [("v,P", np.abs(b[..., :3] - rb[..., :3]).max(), 5e-7 if few else 1e-6), ("T", np.abs(b[..., 3] - rb[..., 3]).max(), 4 * ULP_T),
                  ("vapour_cloud", (np.abs(w[..., :2] - rw[..., :2]) - 1.2e-6 * np.abs(rw[..., :2])).max(), 2e-4 if long else 5e-5),
                  ("precip_smoke", np.abs(w[..., 2:] - rw[..., 2:]).max(), 1e-4 if long else (1e-6 if few else 2e-6))]
        for k, li in (("light_0", 3), ("light_1", 4)):
            if f"it{it}_{k}" in g.files:  # sunlight 0.02 W/m2, net heating 4e-7, IR 0.2 (the sliders' bounds at 20 iterations)
                l, rl = out[it][li], g[f"it{it}_{k}"]
                checks += [(k + " sunlight", np.abs(l[..., 0] - rl[..., 0]).max(), 0.02), (k + " net heating", np.abs(l[..., 1] - rl[..., 1]).max(), 4e-7),
                           (k + " IR", np.abs(l[..., 2:] - rl[..., 2:]).max(), 0.2)]
        bad += [(it, name, float(e), tol) for name, e, tol in checks if not e <= tol]
    return bad


@pytest.mark.parametrize("name", sorted(DUMPS))
def test_oracle_reproduces_the_reference_on_the_surface_scenes(oracle, golden, name):
    g, u = golden(name)
    assert int(g["points"]) == 1
    out = _oracle_run(oracle, g, u, DUMPS[name])
    assert check_fields(out, g, DUMPS[name]) == []
    if name == "surface112_industry":  # the boundary pass of iteration 0 on its own: the chimneys' additions before advection moves them
        L, p = oracle.lib(), oracle.make_params(dict(u, varyings=g["varyings"]), int(g["X"]), int(g["Y"]))
        X, Y = int(g["X"]), int(g["Y"])
        z = lambda *s, dt=np.float32: np.zeros(s, dt)
        bo, wo = z(Y, X, 4), z(Y, X, 4, dt=np.int8)
        L.wxo_velocity(p, g["in_base"].ravel(), g["in_wall"].ravel(), bo.ravel(), wo.ravel())
        cu, vo = z(Y, X), z(Y, X, 2)
        L.wxo_curl(p, bo.ravel(), cu.ravel())
        L.wxo_vorticity(p, cu.ravel(), vo.ravel())
        b2, w2, wl2 = z(Y, X, 4), z(Y, X, 4), z(Y, X, 4, dt=np.int8)
        L.wxo_boundary(p, u["initial_T"], float(g["iter0"]), bo.ravel(), g["in_water"].ravel(), vo.ravel(), np.ascontiguousarray(g["in_wall"]).ravel(),
                       z(Y * X * 4), z(Y * X * 4), z(Y * X * 2), b2.ravel(), w2.ravel(), wl2.ravel())
        assert np.array_equal(wl2, g["pp_boundary_wall"])
        assert np.array_equal(b2[..., :3], g["pp_boundary_base"][..., :3]) and np.abs(b2[..., 3] - g["pp_boundary_base"][..., 3]).max() <= ULP_T
        assert (np.abs(w2 - g["pp_boundary_water"]) - 1.2e-6 * np.abs(g["pp_boundary_water"]))[g["in_wall"][..., 1] != 0].max() <= 1e-6


def _surface(g, arr):
    h = (g["in_wall"][..., 1] == 0).sum(0)
    return np.array([arr[h[x] - 1, x] for x in range(int(g["X"]))]), h


def _rates(g):
    """Growth rate per column as the shader computes it, from the reference's dumps after the growth iteration (soil moisture of the
    surface cell; the light the boundary pass read is the texture the iteration before it wrote)."""
    soil, h = _surface(g, g["it71_water_cur"][..., 2])
    light = np.array([max(g["it71_light_0"][h[x], x, 0], g["it71_light_1"][h[x], x, 0]) for x in range(len(h))], np.float32)
    return (soil * np.sqrt(light) * np.float32(0.01)).astype(np.int64), light


def test_growth_happened_in_the_reference_for_every_rate(golden):
    """From the reference's arrays alone. At 9 240 000 (a multiple of every interval) a cell below the temperature cap grows whatever
    its rate 1 .. 10; at 10 000 rates 1, 2, 4, 5, 10 grow and 3, 6 .. 9 do not: `(100 / rate) * 100`."""
    grown = {}
    for name in ("surface64_growth", "surface64_growth10k"):
        g, _ = golden(name)
        v0, _ = _surface(g, g["it70_wall_cur"][..., 3])
        v1, _ = _surface(g, g["it71_wall_cur"][..., 3])
        rate, light = _rates(g)
        assert light.min() > 500.0  # the sun has come down (less beside the steps)
        assert set(np.unique(v1 - v0)) <= {0, 1}
        assert np.array_equal(_surface(g, g["it75_wall_cur"][..., 3])[0], v1)  # (nothing grows off the interval)
        grown[name] = {r: int((v1 - v0)[(rate == r) & (v0 == 20)].sum()) for r in range(0, 12)}, {r: int(((rate == r) & (v0 == 20)).sum()) for r in range(0, 12)}
        assert (v1 - v0)[v0 == 100].sum() == 0  # above the cap: never
        assert (v1 - v0)[rate > 100].sum() == 0  # interval 0: the documented choice (`% 0` is false)
        assert (rate > 100).sum() >= 3
    lcm, candidates = grown["surface64_growth"]
    assert all(candidates[r] >= 1 and lcm[r] == candidates[r] for r in range(1, 11)), (lcm, candidates)
    assert lcm[0] == 0 and sum(lcm.values()) >= 15
    tenk, candidates = grown["surface64_growth10k"]
    assert all(tenk[r] == candidates[r] >= 1 for r in (1, 2, 4, 5, 10)) and all(tenk[r] == 0 and candidates[r] >= 1 for r in (3, 6, 7, 8, 9)), (tenk, candidates)


def test_fire_events_happened_in_the_reference(golden):
    g, _ = golden("surface64_fire")
    t0, t1, t7, t12 = (a[1, :, 0] for a in (g["in_wall"], g["it1_wall_cur"], g["it7_wall_cur"], g["it12_wall_cur"]))
    assert t0[34] == t0[38] == FIRE and t1[34] == t1[38] == LAND  # out by rain (precipitation above it) and by soaked soil
    assert g["in_water"][2, 34, 2] > 1.0 and g["in_water"][1, 38, 2] >= 300.0
    assert g["it6_wall_cur"][1, 30, 0] == FIRE and g["it6_wall_cur"][1, 30, 3] == 10 and t7[30] == LAND and g["it7_wall_cur"][1, 30, 3] == 9  # burnt down at 8696
    assert (t12 == FIRE).sum() == 1 and t12[12] == FIRE and np.array_equal(t12, g["it11_wall_cur"][1, :, 0])  # 8700 smooths, 87 is no multiple of 10: no spread
    assert (g["it12_water_cur"][2:8, 12, 3] > g["in_water"][2:8, 12, 3]).any() and g["it12_base_cur"][2, 12, 3] > g["it1_base_cur"][2, 12, 3]  # smoke and heat above the fire


def _divisor(water_surface):
    return (water_surface[..., 2] * np.float32(0.1) + water_surface[..., 3] * np.float32(0.5)).astype(np.int64) + 10


def test_the_fire_walked_in_the_reference(golden):
    """surface64_spread, from the reference's arrays: one cell each way at 1000, 1100, 1200 and 1300 -- the rings' divisors, computed
    from the reference's own soil moisture and snow at the end, are 10, 11, 12, 13, made of soil alone, snow alone and both --, never
    earlier; vegetation 20 ignites and 19 does not; smoke of 4.86 and 5.24 ignites what lies under it and 4.29 does not."""
    g, _ = golden("surface64_spread")
    assert int(g["iter0"]) == 995 and int(g["Y"]) >= 50
    T = {it: g[f"it{it}_wall_cur"][1, :, 0] for it in DUMPS["surface64_spread"]}
    assert (g["it310_wall_cur"][2:, :, 1] != 0).all()  # the air stayed air
    for ring, (before, after) in enumerate(((5, 6), (105, 106), (205, 206), (305, 306)), start=1):
        for x in (12 - ring, 12 + ring):
            assert T[before][x] == LAND and T[after][x] == FIRE, (ring, x)
        if ring > 1:
            assert np.array_equal(T[before], T[{105: 6, 205: 106, 305: 206}[before]])  # nothing moves between smoothing iterations
    end = g["it310_water_cur"][1]
    assert [int(_divisor(end[12 + r])) for r in (1, 2, 3, 4)] == [10, 11, 12, 13] == [int(_divisor(end[12 - r])) for r in (1, 2, 3, 4)]
    assert end[14, 3] < 0.2 and end[15, 3] > 3.0 and end[16, 2] > 20.0 and end[16, 3] > 2.0  # soil alone, snow alone, both
    assert T[310][7] == T[310][17] == LAND
    assert g["in_wall"][1, 25, 3] == 20 and g["in_wall"][1, 27, 3] == 19 and T[6][25] == FIRE and T[310][27] == LAND and T[310][26] == FIRE
    smoke = g["it5_water_cur"][2, :, 3]
    lit = (T[5] == LAND) & (T[6] == FIRE)
    assert lit[(smoke > 4.5) & (smoke < 5.0)].sum() >= 5 and lit[(smoke > 5.0) & (smoke < 5.5)].sum() >= 5
    assert (smoke[54:61] > 4.0).all() and not lit[54:61].any() and lit[(smoke > 4.5) & (T[5] == LAND)].all()


def test_industry_dust_and_sea_happened_in_the_reference(golden):
    g, _ = golden("surface112_industry")
    X = int(g["X"])
    w0, w1, b1 = g["in_water"], g["pp_boundary_water"], g["pp_boundary_base"]
    ind = g["in_wall"][0, :, 0] == INDUSTRIAL
    vap, smoke = w1[6, :, 0] - w0[6, :, 0], w1[7, :, 3] - w0[7, :, 3]  # air cells at VERT_DISTANCE 5 and 6 (two wall rows)
    assert set(np.nonzero(vap > 0.2)[0].tolist()) == {18, 22, 98, 102} and set(np.nonzero(smoke > 0.005)[0].tolist()) == {29, 109}
    assert ind[[17, 19, 21, 23, 28, 30, 97, 108, 110]].all()  # ... and not next to them, though the surface there is industrial too
    veg = g["it1_wall_cur"][1, :, 3]
    assert (veg[ind] == 15).all() and (veg[g["in_wall"][0, :, 0] == URBAN] == 75).all() and (g["in_wall"][1, :, 3][ind] == 100).all()
    dust = w1[2, :, 3] - w0[2, :, 3]
    wet = np.isin(np.arange(X), (44, 46))  # precipitation of 6 in the first air cell there: the line's `< 5.0`
    bare = np.zeros(X, bool)
    bare[40:56:2] = True
    assert (dust[bare & ~wet] > 0.02).all() and (dust[bare & wet] == 0).all() and (dust[41:56:2] == 0).all()  # vegetation 5 under wind; vegetation 12 none
    assert (w0[2, [44, 46], 2] >= 5.0).all()
    T0, T1 = g["in_base"][1, :, 3], g["it1_base_cur"][1, :, 3]
    assert (T0[62:66] == 600.0).all() and (np.abs(T1[62:66] - 298.15) < 0.1).all()  # above 500 K: reset to 25 C
    assert T0[67] == 499.0 and T1[67] > 300.0  # below 500 K and beside cooler water: clamped to the maximum, not reset
    assert T0[66] == 499.0 and abs(T1[66] - 298.15) < 0.1  # (beside 600 K the neighbour average lifts it above 500 first)
    assert int(g["iter0"]) % 20 == 0 and X > 80 + 29
