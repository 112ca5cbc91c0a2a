"""The accounting of the droplet life-cycle suite (tests/droplet_scenes.py; tests/test_droplet_gpu.py runs the same case list on the
card), computed from the case list and the oracle's own outputs -- nothing here is asserted by hand: the hash restated in numpy equals
the oracle's, every probe lands where its scene says, every case's event HAPPENS at the iteration it is named for, no texel of any
compared iteration of any case receives two order-sensitive deposits (the condition under which the default splat order, fp32 atomics,
may be compared bit for bit), and the case list reaches the tile / strip / edge phases and the tile transitions it is there for. No GPU."""
import ctypes as C

import numpy as np
import pytest

import droplet_scenes as D
import impulse_scenes as I

CASES = D.cases()
F = np.float32


@pytest.fixture(scope="module")
def runs(oracle):
    """Every case through the oracle once: case id -> (case, scene, per-iteration records)."""
    out = {}
    for c in CASES:
        sc = D.build_case(c)
        out[D.case_id(c)] = (c, sc, D.run_oracle(oracle, c, sc))
    return out


# ---- the restatement ----
def test_hash_restated_equals_the_oracle(oracle):
    L = oracle.lib()
    rng = np.random.Generator(np.random.Philox(11))
    xs = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(D.hash_u32(xs), np.array([L.wxo_hash(int(x)) for x in xs], np.uint32))
    a = np.concatenate([rng.random(2000, dtype=F) * F(20) - F(10), F(-2.0) - rng.random(500, dtype=F), rng.random(500, dtype=F) * F(700)])
    b = np.concatenate([rng.random(2000, dtype=F), rng.random(1000, dtype=F) * F(300)])
    mine = D.random2d(a, b)
    theirs = np.array([L.wxo_random2d(float(p), float(q)) for p, q in zip(a, b)], F)
    assert np.array_equal(mine.view(np.uint32), theirs.view(np.uint32))
    assert mine.min() >= 0 and mine.max() < 1


@pytest.mark.parametrize("X,Y", [D.GRIDS["ragged"], D.GRIDS["tiny"], (1100, 523)])
def test_probe_restated_through_the_particle_pass(oracle, X, Y):
    """Random inactive records and iteration numbers through wxo_precipitation over a grid on which EVERY probe spawns (cloud
    everywhere, still air, no fall speed): the droplet comes out at its probe, (tc - 0.5) * 2 -- bit for bit what probe_coords says."""
    rng = np.random.Generator(np.random.Philox(X))
    n = 600
    drops = rng.random((n, 5), dtype=F)
    drops[:, 2] = F(-10.0) + drops[:, 2]
    drops[n // 2:, 2] = F(-2.0) - (drops[n // 2:, 0] * F(2) - F(1))  # the seeds a retired droplet carries: -2 - x, y
    drops[n // 2:, 3] = drops[n // 2:, 1] * F(2) - F(1)
    drops[n // 2:, 0] = drops[n // 2:, 0] * F(2) - F(1)
    base = np.zeros((Y, X, 4), F)
    base[..., 3] = 450.0  # (below 500, and above 0 C at every height)
    water = np.zeros((Y, X, 4), F)
    water[..., 0], water[..., 1] = 20.0, 5.0
    u = D.uniforms(Y, fallSpeed=0.0, evapRate=0.0)
    p = oracle.make_params(u, X, Y)
    for it in (0, 1, 7, 599, 600, 601, 123457, 9_240_000):
        out, fb, dep = np.zeros_like(drops), np.zeros((Y, X, 4), F), np.zeros((Y, X, 2), F)
        oracle.lib().wxo_precipitation(C.byref(p), float(it), n, drops.reshape(-1), base.reshape(-1), water.reshape(-1), np.zeros(4, F),
                                       out.reshape(-1), fb.reshape(-1), dep.reshape(-1))
        tc0, tc1 = D.probe_coords(drops[:, 2], drops[:, 3], drops[:, 0], it)
        assert (out[:, 2] > 0).all(), "every probe spawns rain on this grid"
        x = (tc0 - F(0.5)) * F(2.0)
        t = x + F(1.0)  # (the flight's wrap of x, which a spawn goes through in the same iteration)
        x = (t - F(2.0) * np.floor(t / F(2.0))) - F(1.0)
        assert np.array_equal(out[:, 0].view(np.uint32), x.view(np.uint32)), it
        assert np.array_equal(out[:, 1].view(np.uint32), ((tc1 - F(0.5)) * F(2.0)).view(np.uint32)), it


def test_seed_search_puts_every_probe_where_the_scene_says(runs):
    n = 0
    for c, sc, _ in runs.values():
        X, Y = c["X"], c["Y"]
        d = sc["drops"]
        inactive = [k for k in range(len(d)) if d[k, 2] < 0]
        assert all(-10 <= d[k, 2] < -9 and 0 <= d[k, 3] < 1 for k in inactive), D.case_id(c)
        probes = {k: e for k, e in sc["expect"].items() if d[k, 2] < 0}
        sites = set(sc["sites"])
        for k, e in probes.items():
            for it in [min(e)]:  # (a record that retires and probes again does so with other seeds: the events test follows it)
                cx, cy = D.probe_texel(d[k, 2], d[k, 3], d[k, 0], sc["iter0"] + it, X, Y)
                assert (int(cx[0]), int(cy[0])) in sites, (D.case_id(c), k, it)
                n += 1
    assert n >= 100


# ---- the events ----
def _want(e):
    return {e} if isinstance(e, str) else set(e)


@pytest.mark.parametrize("kind", D.KINDS + D.ORDER1_KINDS)
def test_every_case_s_event_happens_when_it_is_named_for(runs, kind):
    mine = [v for v in runs.values() if v[0]["kind"] == kind]
    assert mine
    for c, sc, rec in mine:
        cid = D.case_id(c)
        n_events = 0
        for it, r in enumerate(rec):
            for k, names in enumerate(r["names"]):
                e = sc["expect"].get(k)
                if e is None:
                    assert names == {"idle"}, (cid, it, k, names)  # a filler record never finds cloud
                elif it in e:
                    assert _want(e[it]) <= names, (cid, it, k, e[it], names, r["before"][k], r["after"][k])
                    n_events += 1
                elif r["before"][k, 2] < 0 and it < max(e):
                    assert names == {"idle"}, (cid, it, k, names)  # a probe before its iteration
        assert n_events >= 1, cid
        assert len(rec) == sc["n_iter"] >= sc["event_at"] + 4, cid  # followed for 3 iterations and more after the event
        # the kind's own observables
        ev = rec[sc["event_at"]]
        if kind.startswith("lightning"):
            mode, req = sc["lightning_mode"], ev["request"]
            if mode == "refused":
                assert not req.any() and np.array_equal(ev["lightning"], ev["lightning_before"]), cid
                assert ev["lightning_before"][2] >= sc["event_iter"] - 30
            else:
                assert req[3] >= F(0.01), (cid, req)  # the request's intensity
                pure = F(sc["event_iter"]) - F(0.15)  # the request's iteration number shares its channel with the spawn's vapour: iterNum - 0.15
                if mode == "covered":
                    assert req[2] != pure and abs(req[2] - pure) < 0.1, (cid, req)  # ... and with the covering sprite's vapour share
                else:
                    assert req[2] == pure, (cid, req)
                granted = not np.array_equal(ev["lightning"], ev["lightning_before"])
                assert granted == (mode != "discarded"), (cid, ev["lightning"])
                if granted:
                    assert np.array_equal(ev["lightning"], req)
        if kind == "spawn_surface" and c["Y"] > 12:
            (px, py), probe = sc["surface_probe"]["peak"], sc["surface_probe"]["probe"]
            h = sc["h"]
            assert h[px] == py and h[px - 1] < py and h[(px + 1) % c["X"]] < py, cid  # a one-cell peak: the only cell of its row directly above a surface cell nearby
            assert probe == (px + c["offset"][0] % 2, py) and "spawn_rain" in ev["names"][0], cid
        if kind == "spawn_wall" and c["Y"] > 12:
            d0 = sc["drops"][0]  # the stale copy of the record (old seeds, old position) would probe elsewhere two iterations on, and find nothing
            ox, oy = D.probe_texel(d0[2], d0[3], d0[0], sc["iter0"] + sc["event_at"] + 2, c["X"], c["Y"])
            assert (int(ox[0]), int(oy[0])) != sc["probes_again_at"] and sc["water"][oy[0], ox[0], 1] == 0, cid
            assert "spawn" in rec[sc["event_at"] + 2]["names"][0], cid
        if kind in ("refresh", "refresh_covered"):
            at = sc["refresh_at"] - sc["iter0"]
            n_inactive = sum(1 for k in range(len(rec[at]["before"])) if rec[at]["before"][k, 2] < 0)
            assert sc["u"]["inactiveDroplets"] == D.HUGE_INACTIVE
            if kind == "refresh":
                assert rec[at]["count"][0] == n_inactive  # the count that becomes inactiveDroplets: far from 1e12
            else:  # the parked sprite's mass share sits on the count that is taken
                assert n_inactive < rec[at]["count"][0] < n_inactive + 0.01, (cid, rec[at]["count"])
        if kind.startswith("ground") or kind == "spawn_wall":
            assert ev["dep_any"], cid  # (ground_bottom too: the texel above the floor's is wall, the retired droplet is moved up by a row into the grid)
        if kind == "edge_top":
            assert rec[0]["before"][0, 1] > 1 and "ground" in rec[0]["names"][0], cid  # above the top: no sprite; the wrapped fetch reads the floor
        if kind == "flag_row":
            b, t = sc["boundary_row"], sc["boundary_row"] // D.TILE[1]
            assert D.anchor_of(rec[1]["after"][0], c["X"], c["Y"])[1] - 6 == b, cid  # in iteration 1 the sprite's lowest row is the tile row's first row ...
            assert rec[0]["fb_tiles"][t - 1].any() and not rec[1]["fb_tiles"][t - 1].any(), cid  # ... over a tile row that was left in iteration 0 ...
            assert D.anchor_of(rec[2]["after"][0], c["X"], c["Y"])[1] - 6 == b - 1, cid  # ... and enters it one iteration later
        if kind == "last_retires":
            for q in sc["quiet"]:
                assert not rec[q]["fb_any"] and not rec[q]["dep_any"] and rec[q]["count"][0] == len(sc["drops"]), (cid, q)
            assert rec[4]["fb_any"]


def test_only_the_refreshed_count_lets_the_probe_spawn(oracle, runs):
    """Probe A is refused in iteration 600, while inactiveDroplets is still 1e12; probe B spawns in iteration 601, after the refresh; the
    two probed cells were planted with the same cloud water, so the count alone made the difference."""
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] in ("refresh", "refresh_covered")]:
        at = sc["refresh_at"] - sc["iter0"]
        a, b = sorted(k for k, e in sc["expect"].items())[:2]
        assert rec[at]["names"][a] == {"idle"} and "spawn_rain" in rec[at + 1]["names"][b], D.case_id(c)
        # probe A's cell holds the same cloud as probe B's: the chance, not the threshold, refused it
        d = rec[at]["before"]
        ax, ay = D.probe_texel(d[a, 2], d[a, 3], d[a, 0], sc["refresh_at"], c["X"], c["Y"])
        bx, by = D.probe_texel(d[b, 2], d[b, 3], d[b, 0], sc["refresh_at"] + 1, c["X"], c["Y"])
        assert sc["water"][ay[0], ax[0], 1] == sc["water"][by[0], bx[0], 1] > 6


def test_ground_deposits_reach_the_surface(oracle, runs):
    """The surface cell under a deposit ends the run with other soil moisture / snow than in the same scene run without particles:
    the boundary pass read the deposition texture."""
    n = 0
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] in ("ground_flat", "ground_peak", "ground_pit", "ground_step", "ground_buried")]:
        quiet = D.run_oracle(oracle, c, sc, enablePrecipitation=0)
        a, b = rec[-1]["water"], quiet[-1]["water"]
        wall = sc["wall"][..., 1] == 0
        changed = (a[..., 2:] != b[..., 2:]).any(-1) & wall
        assert changed.any(), D.case_id(c)
        n += 1
    assert n >= 5 * len(D.CONFIG_CYCLE)


def test_refused_spawns_are_refused_by_the_chance_not_by_luck(runs):
    """spawn_refused / refresh: at the refused probe's cell the pre-test passed (cloud above the threshold) and fract((10 cloud)^2) is
    far above the chance that inactiveDroplets = 1e12 leaves."""
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] == "spawn_refused"]:
        assert sc["u"]["inactiveDroplets"] == D.HUGE_INACTIVE
        assert (sc["water"][..., 1].max() - 1.0) * c["X"] * c["Y"] / D.HUGE_INACTIVE < 1e-6


# ---- disjointness, finiteness ----
def test_no_texel_receives_two_deposits_in_any_compared_iteration(runs):
    """The allowed share of dropped cases is zero: every iteration of every case."""
    assert len(runs) == len(CASES)
    for cid, (c, sc, rec) in runs.items():
        if c["kind"] in D.ORDER1_KINDS:
            # order 1 only: the inactive count is kept in a slot of its own on both sides and added to texel (0,0) once, so the
            # additions of 1.0 are no deposits of the texel; the sprites themselves must still be disjoint
            assert D.CONFIGS[c["config"]].get("splat_order") == 1, cid
            for r in rec:
                m = r["before"][:, 2] >= 0
                assert I.deposits_per_texel(r["before"][m], r["after"][m], c["X"], c["Y"]) <= 1, cid
            continue
        assert [r["deposits"] for r in rec] == [min(1, r["deposits"]) for r in rec], (cid, [r["deposits"] for r in rec])


def test_every_scene_stays_finite_and_slow(runs):
    for cid, (c, sc, rec) in runs.items():
        assert all(r["finite"] for r in rec), cid
        assert max(r["vmax"] for r in rec) < 0.9, (cid, max(r["vmax"] for r in rec))


# ---- the case list ----
def test_every_kind_meets_every_configuration():
    seen = {(c["kind"], c["config"]) for c in CASES if c["grid"] == "ragged" and c["kind"] in D.KINDS}
    assert seen == {(k, g) for k in D.KINDS for g in D.CONFIG_CYCLE}
    assert {c["kind"] for c in CASES if c["grid"] == "aligned"} == set(D.KINDS)
    assert {c["kind"] for c in CASES if c["grid"] == "tiny"} == set(D.TINY_KINDS)
    assert {(c["kind"], c["bands"]) for c in CASES if c["grid"] == "bands"} == {(k, b) for b, k in enumerate(D.BAND_KINDS)} | {("walk", b) for b in (0, 1, 2)}
    assert {(c["kind"], c["config"]) for c in CASES if c["kind"] in D.ORDER1_KINDS} == {(k, g) for k in D.ORDER1_KINDS for g in ("order1", "order1_perpass")}
    assert len({D.case_id(c) for c in CASES}) == len(CASES)
    # no offset is spare: each (kind, configuration) pair is run at ONE offset, so dropping an offset drops pairs
    for off in D.OFFSETS:
        assert any(tuple(c["offset"]) == off for c in CASES if c["grid"] == "ragged")
    # both parities of the work lists meet a probe's event: an even and an odd number of iterations before it, under every configuration
    probes = ("spawn_rain", "spawn_snow", "spawn_wall", "lightning_granted", "spawn_surface")
    for g in D.CONFIG_CYCLE:
        assert {c["lead"] for c in CASES if c["config"] == g and c["kind"] in probes} == {0, 1}, g


EVENT_NAMES = ("spawn_rain", "spawn_snow", "spawn_held", "spawn_retire", "evaporated_rain", "evaporated_snow", "ground_bottom", "ground_wall", "ground_buried",
               "deposit_rain", "deposit_snow", "deposit_mixed", "wrap", "cold", "warm", "freeze", "freeze_all", "melt", "melt_all", "density_up",
               "rime", "grew", "evap_all", "in_cloud")


def test_every_event_happens_under_every_configuration(runs):
    for g in D.CONFIG_CYCLE:
        seen = set()
        for c, sc, rec in runs.values():
            if c["config"] == g:
                for r in rec:
                    for names in r["names"]:
                        seen |= names
        assert not set(EVENT_NAMES) - seen, (g, set(EVENT_NAMES) - seen)


PARITY_NAMES = ("spawn_rain", "spawn_snow", "spawn_retire", "evaporated", "ground", "flight", "freeze", "melt", "grew")


def test_events_meet_both_parities_of_the_work_lists(runs):
    """An upload resets the work-list parity, so the parity an event meets is that of its iteration since the start of the case. Probes
    are placed in iteration 0 or 1 by the case's lead; evaporations happen in iteration 0 (planted below 0.04) and 1 (evap_limited),
    ground hits in 0 (planted in the wall) and 1 (the walk scene's droplet that falls into the surface), flights go on through both.
    Under every configuration each of these names is met at an even and at an odd iteration, and so are the tile transitions that
    follow them (dirty -> zeroed one iteration after an event of either parity)."""
    for g in D.CONFIG_CYCLE:
        seen = set()
        for c, sc, rec in runs.values():
            if c["config"] == g:
                for it, r in enumerate(rec):
                    for names in r["names"]:
                        seen |= {(n, it % 2) for n in names}
        missing = {(n, p) for n in PARITY_NAMES for p in (0, 1)} - seen
        assert not missing, (g, missing)


def _anchors(runs):
    """(case, iteration, anchor q, anchor r) of every sprite the oracle splatted."""
    for cid, (c, sc, rec) in runs.items():
        X, Y = c["X"], c["Y"]
        for it, r in enumerate(rec):
            for k in range(len(r["before"])):
                b, a = r["before"][k], r["after"][k]
                flew = b[2] >= 0 or (a[2] >= 0 and "spawn_held" not in r["names"][k]) or "spawn_retire" in r["names"][k]
                if flew and abs(a[0]) <= 1 and abs(a[1]) <= 1:
                    q, rr = D.anchor_of(a, X, Y)
                    yield c, it, q, rr


def test_tile_and_strip_phases_of_the_sprites(runs):
    """Anchors on both sides of a 64-column and of a 16-row tile boundary and sprites that straddle one by one pixel and by eleven; the
    56-column strip seam crossed inside a tile; sprites in rows 0 and Y - 1 and cut by each edge and by a corner; anchor column X and
    anchor row Y, which on the aligned grid own an extra tile column / row of the accumulation grid."""
    tx, ty = D.TILE
    seen = set()
    for c, it, q, r in _anchors(runs):
        X, Y = c["X"], c["Y"]
        i0, j0 = q - 6, r - 6
        for b in range(tx, X, tx):
            if i0 < b <= i0 + 11:
                seen.add(("x_straddle", b - i0))  # columns of the sprite before the boundary
            if abs(q - b) <= 6:
                seen.add(("x_side", "left" if q < b else "right"))
        for b in range(ty, Y, ty):
            if j0 < b <= j0 + 11:
                seen.add(("y_straddle", b - j0))
            if abs(r - b) <= 6:
                seen.add(("y_side", "below" if r < b else "above"))
        for b in range(D.STRIP, X, D.STRIP):
            if i0 < b <= i0 + 11 and b % tx:
                seen.add("strip_seam_inside_a_tile")
        if j0 <= 0:
            seen.add("row_0")
        if j0 + 11 >= Y - 1:
            seen.add("row_Y-1")
        for name, cut in (("left", i0 < 0), ("right", i0 + 11 >= X), ("bottom", j0 < 0), ("top", j0 + 11 >= Y)):
            if cut:
                seen.add(("cut", name))
        if i0 + 11 >= X and j0 + 11 >= Y:
            seen.add(("cut", "corner"))
        if q == X:
            seen.add(("anchor_column_X", c["grid"]))
        if r == Y:
            seen.add(("anchor_row_Y", c["grid"]))
    need = {("x_straddle", 1), ("x_straddle", 11), ("y_straddle", 1), ("y_straddle", 11), ("x_side", "left"), ("x_side", "right"), ("y_side", "below"),
            ("y_side", "above"), "strip_seam_inside_a_tile", "row_0", "row_Y-1", ("cut", "left"), ("cut", "right"), ("cut", "bottom"), ("cut", "top"),
            ("cut", "corner"), ("anchor_column_X", "ragged"), ("anchor_row_Y", "ragged"), ("anchor_column_X", "aligned"), ("anchor_row_Y", "aligned")}
    assert not need - seen, need - seen


def test_every_tile_transition_is_met_under_every_configuration(runs):
    """Per configuration, separately for the feedback and the deposition texture, some tile goes clean -> dirty, dirty -> dirty, dirty
    -> zeroed, stays skipped for two iterations and more, and is entered again after that."""
    for g in D.CONFIG_CYCLE:
        for tex in ("fb_tiles", "dep_tiles"):
            seen = set()
            for c, sc, rec in runs.values():
                if c["config"] != g:
                    continue
                maps = np.array([r[tex] for r in rec])
                for j in range(maps.shape[1]):
                    for i in range(maps.shape[2]):
                        seen |= D.transitions(list(maps[:, j, i]))
            assert not set(D.TRANSITIONS) - seen, (g, tex, set(D.TRANSITIONS) - seen)
    # the deposition tile's cycle is its own: in the walk scenes some tile's deposition map differs from its feedback map
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] == "walk"]:
        assert any(not np.array_equal(r["fb_tiles"], r["dep_tiles"]) for r in rec), D.case_id(c)


def test_schedules_put_the_event_where_the_configuration_says():
    for config in D.CONFIG_CYCLE:
        for lead in (0, 1, 2):
            calls, compare = D.schedule(config, lead + 5, lead)
            assert sum(n for n, _ in calls) == lead + 5 == compare[-1]
            done = 0
            for n, flag in calls:
                if done <= lead < done + n:
                    last = lead == done + n - 1
                    if D.CONFIGS[config].get("plain"):
                        assert not last and flag == 0
                    elif D.CONFIGS[config].get("pieces"):
                        assert flag == 4 and n == 1
                    else:
                        assert last and n == 1 and flag == 0
                done += n
