"""The slab velocity watch on the card (VxTrack / vx_track_commit / k_vx_scan, vx_seen in the three marching kernels, k_vx_roll,
wx_slab_vx_take / wx_slab_set_vx_bound / wx_slab_period, ring_vx_bootstrap / ring_vx_roll): the VALUE wx_slab_vx_take returns against
the oracle's measured-stage |vx|, float32 bit for bit (A); the watched zone and the two limits on lone slab handles (B); the sizing
arithmetic against a restatement of include/wxsim.h (C); the ring protocol against a model of a dozen lines (D). Scenes and case
lists: tests/watch_scenes.py; tests/test_vx_watch_cpu.py accounts for them on the oracle alone."""
import json

import numpy as np
import pytest

import impulse_scenes as I
import watch_scenes as W

pytestmark = pytest.mark.gpu
WX_E_INVALID, WX_E_STATE = -1, -5


@pytest.fixture(scope="module")
def E(pkg):
    pkg.engine.build()
    return pkg.engine


@pytest.fixture(scope="module")
def backgrounds():
    return {g: W.background(*g) for g in (W.SMALL, W.PHASE)}


def _options(h, f, bands=1):
    """tools/fuzz_parity.py's way of configuring a handle (run_impulse_case: after upload and set_params)."""
    h.set_option(h.OPT_KERNEL_SET, f.get("kernel_set", 1))
    h.set_option(h.OPT_DRY_KERNEL, f.get("dry_kernel", 1))
    h.set_option(h.OPT_DRY_PAIRS, f.get("pairs", 1))
    h.set_option(h.OPT_ROW_BANDS, bands)
    h.set_option(h.OPT_WATER0_ON_DEMAND, 1)


def _load(pkg, h, family, scene, u, bands=1, quiet=None):
    """The scene into the handle, configured as the family says; ``quiet``: the background, for the priming pair of dry_pairs_plain."""
    f = W.FAMILIES[family]
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    slab = h.halo > 0
    if f.get("prime"):  # a quiet pair first: the handle hears of an empty exact-path list, the trigger then meets the PLAIN instantiation
        h.upload(*quiet)
        h.set_params(p, u["initial_T"])
        _options(h, f, bands)
        if slab:
            h.slab_assert_water_free(True)
        h.step(2)
        assert h.pair_stats() == (0, 0)
    h.upload(*scene)
    h.set_params(p, u["initial_T"])
    h.iter = 0
    _options(h, f, bands)
    if slab and f["dry"]:
        h.slab_assert_water_free(True)  # (a lone slab: the host's word that the whole domain is water-free -- the water-free kernels run)
        assert h.water_free()


def _run_calls(h, calls):
    for n, flags in calls:
        h.step(n, flags)


def _take_bits(h):
    return W.bits(h.slab_vx_take())


def _fresh(family):
    return family == "dry_pairs_taint"  # (a fresh handle's hint word starts at 1: its first pair runs TAINT)


def _whole_case(pkg, E, oracle, c, bg, handle=None):
    """One part-A case -> (bits the handle's take returned, bits expected, pair stats or None)."""
    family = c["family"]
    f = W.FAMILIES[family]
    u = W.uniforms(family, c["Y"])
    scene = W.whole_scene(c, bg)
    seen, _ = W.reference(oracle, scene, u, family)
    h = handle if handle is not None else E.Handle(c["X"], c["Y"], 0)
    try:
        _load(pkg, h, family, scene, u, bands=c.get("bands", 1), quiet=bg)
        _run_calls(h, f["calls"])
        got = _take_bits(h)
        stats = h.pair_stats() if f["kernel"] == "dry2" else None
        again = _take_bits(h)
    finally:
        if handle is None:
            h.close()
    assert again == 0, (c, again)  # the take reset the accumulator
    return got, W.bits(W.expected_take(seen)), stats, [float(a.max()) for a in seen]


@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_take_equals_the_oracles_measured_vx_on_169x52(pkg, E, oracle, backgrounds, family):
    """A lone fast cell with quiet neighbours at every lane group, row and sign of the case list (and the cell that is fast in vy alone,
    and the pair straddling 0.5): the take is the oracle's measured-stage maximum, bit for bit, or 0.0 below 0.5.
    [mutations: fabsf dropped from vx_seen; `m >= 0.5f` as `>`; strip relative to the launch has no effect on a whole domain]"""
    cases = [c for c in W.whole_cases() if c["family"] == family and (c["X"], c["Y"]) == W.SMALL]
    assert cases
    bg = backgrounds[W.SMALL]
    shared = None if _fresh(family) else E.Handle(W.SMALL[0], W.SMALL[1], 0)
    bad = []
    try:
        for c in cases:
            got, want, stats, maxima = _whole_case(pkg, E, oracle, c, bg, shared)
            if got != want:
                bad.append({"case": c, "got": float(np.int32(got).view(np.float32)), "want": float(np.int32(want).view(np.float32)), "per_iteration": maxima,
                            "phases": I.site_phases(c["x"], c["y"], c["X"])})
            if stats is not None and c["group"] in W.LANE_GROUPS:  # which instantiation ran: TAINT records a first-iteration cell of 0.9 and more, the plain one takes it inline
                assert (stats[0] > 0) == (family == "dry_pairs_taint"), (c, stats)
    finally:
        if shared is not None:
            shared.close()
    assert not bad, "%d of %d cases: %s" % (len(bad), len(cases), json.dumps(bad[:12]))


@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_take_on_the_phase_grid(pkg, E, oracle, backgrounds, family):
    """One case per kernel on 505 x 77 (X % 56 == 1: the site is the one-column ragged strip of the 56-column kernels)."""
    (c,) = [c for c in W.whole_cases() if c["family"] == family and (c["X"], c["Y"]) == W.PHASE]
    got, want, _, maxima = _whole_case(pkg, E, oracle, c, backgrounds[W.PHASE])
    assert want != 0 and got == want, (c, got, want, maxima)


@pytest.mark.parametrize("family,mode", [(f, m) for f in ("wet_display", "dry_pairs_taint") for m in (0, 1, 2)])
def test_take_under_the_three_row_band_modes(pkg, E, oracle, family, mode):
    """2500 x 300, the smallest grid on which the three ROW_BANDS modes differ. The wet kernel: a lone cell in EVERY row next to a border
    between two row segments of the mode's launch shape (watch_scenes.band_border_rows: 185 rows of the one table of mode 0, 154 of the
    eight bands of modes 1 and 2 -- the 1- and 2-row tail segments of every band, the bands of 37 rows that clip the table), columns and
    signed values going round; the reference is the oracle on the 128 columns around the site. The pair kernel: one site per mode."""
    cases = [c for c in W.whole_cases() if c["family"] == family and c.get("bands") == mode]
    assert len(cases) == (len(W.band_border_rows(mode)) if family == "wet_display" else 1)
    bg = W.background(*W.BANDS)
    shared = None if _fresh(family) else E.Handle(W.BANDS[0], W.BANDS[1], 0)
    u = W.uniforms(family, W.BANDS[1])
    bad = []
    try:
        for c in cases:
            want = W.bits(W.expected_take(W.cropped_reference(oracle, c, bg)))
            h = shared if shared is not None else E.Handle(c["X"], c["Y"], 0)
            try:
                _load(pkg, h, family, W.whole_scene(c, bg), u, bands=mode)
                _run_calls(h, W.FAMILIES[family]["calls"])
                got = _take_bits(h)
                assert _take_bits(h) == 0
            finally:
                if shared is None:
                    h.close()
            assert want != 0, c
            if got != want:
                bad.append({"case": c, "got": float(np.int32(got).view(np.float32)), "want": float(np.int32(want).view(np.float32))})
    finally:
        if shared is not None:
            shared.close()
    assert not bad, "%d of %d cases: %s" % (len(bad), len(cases), json.dumps(bad[:12]))


# ---- semantics, once per kernel family ----
SEMANTIC_FAMILIES = ("wet_display", "dry_single", "dry_pairs_taint", "dry_pairs_plain", "perpass", "dry_tiled")


@pytest.mark.parametrize("family", SEMANTIC_FAMILIES)
def test_take_is_the_maximum_since_the_last_take_and_resets(pkg, E, oracle, backgrounds, family):
    """Three iterations (one call: pairs run a pair and a single one) of a scene whose lone cell is fast in the FIRST iteration only:
    the take is the maximum over all three, not the last one's; a second take with nothing run returns 0.0; the next iterations
    start from 0 again (the quiet flow: 0.0). [mutation: wx_slab_vx_take without its memset]"""
    f = W.FAMILIES[family]
    X, Y = W.SMALL
    scan = f["stage"] is None
    c = {"family": family, "X": X, "Y": Y, "x": 57, "y": 30, "vx": W.SIGNED_SCAN[family][0] if scan else -7.5, "vy": 0.0}
    u = W.uniforms(family, Y)
    scene = W.whole_scene(c, backgrounds[W.SMALL])
    calls = ((1, 0),) if scan else ((3, 0),)  # (kernels that do not track: the scan sees the last state only -- one iteration)
    seen, _ = W.reference(oracle, scene, u, family, calls=calls)
    want = W.expected_take(seen)
    if not scan:
        assert seen[0].max() >= 1.0 and max(a.max() for a in seen[1:]) < W.HALF
    assert want >= W.HALF
    h = E.Handle(X, Y, 0)
    try:
        _load(pkg, h, family, scene, u, quiet=backgrounds[W.SMALL])
        _run_calls(h, calls)
        assert _take_bits(h) == W.bits(want), (family, [float(a.max()) for a in seen])
        assert _take_bits(h) == 0
        assert _take_bits(h) == 0
        if not scan:
            h.step(2)  # the flow is quiet by now
            assert _take_bits(h) == 0
    finally:
        h.close()


@pytest.mark.parametrize("family", ("wet_display", "dry_single", "dry_pairs_taint"))
def test_take_after_an_upload_scans_the_uploaded_state(pkg, E, backgrounds, family):
    """Directly after an upload the take is the planted value itself (k_vx_scan over the whole domain), whichever kernels will step."""
    X, Y = W.SMALL
    h = E.Handle(X, Y, 0)
    try:
        for x, y, v in ((0, 1, 1.3), (X - 1, Y - 2, -7.5), (57, 8, 3.0), (100, 51, -0.75)):
            c = {"X": X, "Y": Y, "x": x, "y": y, "vx": v, "vy": 0.0}
            _load(pkg, h, family, W.whole_scene(c, backgrounds[W.SMALL]), W.uniforms(family, Y), quiet=backgrounds[W.SMALL])
            assert _take_bits(h) == W.bits(abs(v)), (family, c)
            assert _take_bits(h) == 0
    finally:
        h.close()


def test_scan_compares_exactly(pkg, E, backgrounds):
    """The scan path's comparison with 0.5 is exact: an uploaded |vx| of exactly 0.5 is returned as 0.5, its float32 predecessor gives
    0.0, a NaN gives +inf (and so does -inf). [mutation: `m >= 0.5f` as `>`]"""
    X, Y = W.SMALL
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    h = E.Handle(X, Y, 0)
    try:
        for v, want in ((0.5, 0.5), (-0.5, 0.5), (below, 0.0), (-below, 0.0), (float("nan"), float("inf")), (float("-inf"), float("inf"))):
            c = {"X": X, "Y": Y, "x": 168, "y": 30, "vx": v, "vy": 0.0}
            scene = W.whole_scene(c, backgrounds[W.SMALL])
            if v != v:
                scene[0][30, 168, 0] = np.float32("nan")
            _load(pkg, h, "wet_display", scene, W.uniforms("wet_display", Y))
            assert _take_bits(h) == W.bits(want), (v, want)
    finally:
        h.close()


# ---- cases that need more than lone cells: the dry pair kernel's exact paths ----
def _spiked(X, Y):
    base, water, wall, _, sites = I.impulse_scene(X, Y, "fast_vx", offset=W.SPIKED_OFFSET, fast_values=I.DRY_FAST_VALUES)
    return (base, water, wall), sites


def test_pair_kernels_recomputed_cells_are_watched(pkg, E, oracle):
    """The planted 20 / 80 spikes of impulse_scenes.DRY_FAST_VALUES on a fresh handle (TAINT): the first pair's take is the oracle's
    maximum over both iterations; the SECOND pair (iterations 3 and 4, TAINT again: the first left entries) is faster in its second
    iteration than in its first, at a cell whose neighbourhood the taint turned into NaN inside the march -- only k_dry2_fix, which
    recomputes it, can report it. [mutation: the vx_track_commit of k_dry2_fix removed]"""
    X, Y = W.PHASE
    scene, _ = _spiked(X, Y)
    u = W.uniforms("dry_pairs_taint", Y)
    seen, _ = W.reference(oracle, scene, u, "dry_pairs_taint", calls=((4, 0),))
    m = [np.float32(a.max()) for a in seen]
    assert m[3] > m[2] >= np.float32(0.9), m  # (tests/test_vx_watch_cpu.py: ... and the fastest cell of iteration 4 has a fast first-iteration cell in its cone)
    h = E.Handle(X, Y, 0)
    try:
        _load(pkg, h, "dry_pairs_taint", scene, u)
        h.step(2)
        assert _take_bits(h) == W.bits(max(m[0], m[1])), m
        first = h.pair_stats()
        h.step(2)
        got = _take_bits(h)
        second = h.pair_stats()
        assert first[0] > 0 or first[1] > 0, first
        assert second[0] > 0, second
        assert got == W.bits(m[3]), (float(np.int32(got).view(np.float32)), m)
    finally:
        h.close()


def test_pair_repeated_whole_is_watched_once_more_with_the_same_result(pkg, E, oracle):
    """A list of 4 entries (WX_OPT_FIX_CAP, as tests/test_gpu_parity.py provokes it): the pair is repeated whole by
    march_dry_redo_items, which commits its |vx| again -- the take still is the oracle's maximum over both iterations."""
    X, Y = W.PHASE
    scene, _ = _spiked(X, Y)
    u = W.uniforms("dry_pairs_taint", Y)
    seen, _ = W.reference(oracle, scene, u, "dry_pairs_taint", calls=((4, 0),))
    m = [np.float32(a.max()) for a in seen]
    h = E.Handle(X, Y, 0)
    try:
        h.set_option(h.OPT_FIX_CAP, 4)
        _load(pkg, h, "dry_pairs_taint", scene, u)
        h.step(2)
        assert _take_bits(h) == W.bits(max(m[0], m[1])), m
        assert h.pair_stats()[1] > 0
        h.step(2)
        assert _take_bits(h) == W.bits(max(m[2], m[3])), m
        assert h.pair_stats()[1] > 0
    finally:
        h.close()


# ---- B: the zone and the limits, on lone slab handles ----
def _slab(E, x0):
    return E.Handle(W.SLAB["X_owned"], W.SLAB["Y"], 0, X_global=W.SLAB["X_global"], x0=x0, halo=W.SLAB["halo"])


def _local(scene, x0):
    idx = W.slab_window(x0)
    return tuple(np.ascontiguousarray(a[:, idx]) for a in scene)


def _slab_first_iteration(pkg, E, family, scene, x0, bound=None, calls=None):
    """A fresh lone slab: upload the window of ``scene``, take (the scan of the uploaded state, without a check), optionally set a
    bound, run the family's calls -> the handle (the caller syncs, takes and closes)."""
    u = W.uniforms(family, W.SLAB["Y"])
    h = _slab(E, x0)
    quiet = _local(W.background(W.SLAB["X_global"], W.SLAB["Y"]), x0)
    _load(pkg, h, family, _local(scene, x0), u, quiet=quiet)
    h.slab_vx_take()
    if bound is not None:
        h.slab_set_vx_bound(bound)
    _run_calls(h, calls or W.FAMILIES[family]["calls"])
    return h


@pytest.mark.parametrize("family", W.SLAB_FAMILIES)
def test_slab_zone_must_see_and_never_recorded(pkg, E, oracle, family):
    """halo 12, 256 owned columns (x0 = 0 and 256: the wrap of the global column index inside the array): a lone cell at local
    columns 8, 35, 244, 271 is returned with its reference value; one in an unwatched strip (64, 140, 215) is not recorded and --
    below 2 * halo - 8 = 16 -- not reported. Only the first iteration of the period is compared (pairs: the two of the period; the
    cone of 6 leaves the owned columns and the zone's inner part exact). The host never tells the handle about the flow: a must-see
    value of 1.0 and more is also REPORTED by the next sync, a never-recorded one is not. [mutations: zone_r rounded up; strip relative to the launch; fabsf dropped]"""
    f = W.FAMILIES[family]
    for c in [c for c in W.slab_cases() if c["family"] == family]:
        scene = W.slab_scene(c["c"], c["x0"], c["vx"])
        seen, _ = W.reference(oracle, scene, W.uniforms(family, W.SLAB["Y"]), family)
        cols = W.slab_window(c["x0"])
        zone = W.scan_zone_columns() if f["stage"] is None else W.valid_columns(len(seen))
        want = W.expected_take([a[:, cols] for a in seen], zone) if c["class"] == "must_see" else np.float32(0.0)
        h = _slab_first_iteration(pkg, E, family, scene, c["x0"])
        try:
            assert h.slab_cone == 6 and h.slab_period == 2
            got = _take_bits(h)
            assert got == W.bits(want), (c, float(np.int32(got).view(np.float32)), float(want), [float(a[:, cols].max()) for a in seen])
            reported = None
            try:
                h.sync()
            except E.WxError as e:
                reported = e
            over = c["class"] == "must_see" and want >= np.float32(1.0)  # the period limit cone - 5
            assert (reported is not None) == over, (c, float(want), reported)
            if reported is not None:
                assert reported.code == WX_E_STATE and "|vx| reached" in str(reported)
        finally:
            h.close()


@pytest.mark.parametrize("family", ("wet_display", "dry_single", "dry_pairs_taint", "dry_pairs_plain"))
def test_slab_period_limit_straddled(pkg, E, oracle, family):
    """The period limit cone - 5: a must-see site whose measured-stage value is just below 1.0 passes, just above is WX_E_STATE
    with "|vx| reached"; after wx_slab_set_vx_bound(0.7) (cone 7, limit 2.0) the same pair passes and a pair around 2.0 separates.
    [mutation: `m >= t.limit` as `>` -- the upper value of the dry pairs is measured at exactly the limit]"""
    stage = W.FAMILIES[family]["stage"]
    calls = ((1, 0),) if family == "wet_display" or family == "dry_single" else ((2, 0),)
    for name, bound, limit, expect in (("period", None, 1.0, (False, True)), ("period", 0.7, 2.0, (False, False)), ("period7", 0.7, 2.0, (False, True))):
        for side, raises in enumerate(expect):
            vx = W.STRADDLES[(name, stage)][side]
            h = _slab_first_iteration(pkg, E, family, W.straddle_scene(name, vx), 0, bound=bound, calls=calls)
            try:
                assert h.slab_cone == (6 if bound is None else 7)
                if raises:
                    with pytest.raises(E.WxError) as ei:
                        h.sync()
                    assert ei.value.code == WX_E_STATE and "|vx| reached" in str(ei.value), ei.value
                else:
                    h.sync()
                m = W.straddle_measured(oracle, name, stage, vx)
                assert _take_bits(h) == W.bits(m), (family, name, side, float(m))
            finally:
                h.close()


@pytest.mark.parametrize("family", ("wet_display", "dry_single", "dry_pairs_taint", "dry_pairs_plain"))
def test_slab_interior_limit_straddled(pkg, E, oracle, family):
    """A never-recorded column: just below 2 * halo - 8 = 16 silent and the take stays 0.0, at 16 and above reported.
    [mutations: limit_in from 2 * halo; zone_r rounded up does not show here]"""
    stage = W.FAMILIES[family]["stage"]
    calls = ((1, 0),) if family == "wet_display" or family == "dry_single" else ((2, 0),)
    for side, raises in enumerate((False, True)):
        vx = W.STRADDLES[("interior", stage)][side]
        h = _slab_first_iteration(pkg, E, family, W.straddle_scene("interior", vx), 0, calls=calls)
        try:
            if raises:
                with pytest.raises(E.WxError) as ei:
                    h.sync()
                assert ei.value.code == WX_E_STATE and "|vx| reached" in str(ei.value), ei.value
            else:
                h.sync()
            assert _take_bits(h) == 0, (family, side)
        finally:
            h.close()


def test_slab_limits_on_the_scan_path_are_exact(pkg, E):
    """Uploaded values, compared exactly: |vx| = 1.0 in a must-see cell -- the take runs the stale scan WITHOUT a check and returns 1.0;
    wx_device_ptr(BASE_CUR) marks the state untracked, the next take scans WITH the check: WX_E_STATE at the next sync. The float32
    predecessor of 1.0: no error. The same at the interior limit 16.0 in a never-recorded column, where the take stays 0.0.
    [mutations: `m >= t.limit` as `>`; limit_in from 2 * halo]"""
    below1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    below16 = float(np.nextafter(np.float32(16.0), np.float32(0.0)))
    for c_local, v, take, raises in ((W.MUST_SEE[1], 1.0, 1.0, True), (W.MUST_SEE[2], -1.0, 1.0, True), (W.MUST_SEE[1], below1, below1, False),
                                     (W.NEVER_RECORDED[1], 16.0, 0.0, True), (W.NEVER_RECORDED[0], -16.0, 0.0, True), (W.NEVER_RECORDED[2], below16, 0.0, False),
                                     (W.NEVER_RECORDED[1], -below16, 0.0, False)):
        for x0 in W.SLAB["x0s"]:
            h = _slab(E, x0)
            try:
                _load(pkg, h, "wet_display", _local(W.slab_scene(c_local, x0, v), x0), W.uniforms("wet_display", W.SLAB["Y"]))
                assert _take_bits(h) == W.bits(take), (c_local, v)
                h.sync()  # the stale scan ran without a check
                assert h.device_ptr("BASE_CUR") != 0
                assert _take_bits(h) == W.bits(take), (c_local, v)
                if raises:
                    with pytest.raises(E.WxError) as ei:
                        h.sync()
                    assert ei.value.code == WX_E_STATE and "|vx| reached" in str(ei.value), ei.value
                else:
                    h.sync()
            finally:
                h.close()


# ---- C: the sizing arithmetic ----
def _crossings():
    """The float32 neighbours of every v at which 1.25 v + 0.25 crosses an integer up to 8."""
    out = []
    for k in range(1, 9):
        v = np.float32((k - 0.25) / 1.25)
        for _ in range(3):
            v = np.nextafter(v, np.float32(0.0))
        for _ in range(7):
            out.append(float(v))
            v = np.nextafter(v, np.float32(np.inf))
    return out


SIZING_V = [0.0, 0.5, float(np.nextafter(np.float32(0.6), np.float32(0.0))), float(np.float32(0.6)), 0.7, 1.39, 1.4, 2.4, 6.0, 1e6, float("inf")] + _crossings()


@pytest.mark.parametrize("halo", (6, 12, 13, 42, 64))
def test_sizing_without_particles(pkg, E, halo):
    """wx_slab_set_vx_bound / wx_slab_cone / wx_slab_period against the header's text. [mutation: `* 1.25f + 0.25f` as `* 1.25f`]"""
    h = E.Handle(128, 16, 0, X_global=512, x0=0, halo=halo)
    try:
        assert (h.slab_cone, h.slab_period) == (6, halo // 6)
        crossed = set()
        for v in SIZING_V:
            cone, period, refused = W.sizing(v, halo)
            before = (h.slab_cone, h.slab_period)
            if refused:
                with pytest.raises(E.WxError) as ei:
                    h.slab_set_vx_bound(v)
                assert ei.value.code == WX_E_STATE and "wider halo" in str(ei.value), (v, ei.value)
                assert (h.slab_cone, h.slab_period) == before  # a refused bound changes nothing
            else:
                h.slab_set_vx_bound(v)
                assert (h.slab_cone, h.slab_period) == (cone, period), (v, halo)
            crossed.add(W.sizing(v, 10 ** 9)[0])  # (the cone a halo wide enough would get)
        assert crossed >= set(range(6, 15)), crossed  # the list crosses every integer up to 8
        for v in (float("nan"), -0.0001, float("-inf")):
            with pytest.raises(E.WxError) as ei:
                h.slab_set_vx_bound(v)
            assert ei.value.code == WX_E_INVALID, (v, ei.value)
    finally:
        h.close()


@pytest.mark.parametrize("halo,X_owned,X_global", [(64, 128, 512), (128, 256, 1024)])
def test_sizing_with_particles(pkg, E, halo, X_owned, X_global):
    h = E.Handle(X_owned, 16, 8, X_global=X_global, x0=0, halo=halo)
    try:
        assert h.slab_period == min(15, 1 + (halo - 12) // 9)  # WX_SLAB_PERIOD_PARTICLES(halo) for |vx| < 1
        seen = set()
        for v in SIZING_V + [12.0, 20.0, 24.8, 25.0, 50.0]:
            cone, period, refused = W.sizing(v, halo, particles=True)
            if refused:
                with pytest.raises(E.WxError) as ei:
                    h.slab_set_vx_bound(v)
                assert ei.value.code == WX_E_STATE, (v, ei.value)
            else:
                h.slab_set_vx_bound(v)
                assert (h.slab_cone, h.slab_period) == (cone, period), (v, halo)
            seen.add((period, refused))
        assert len({p for p, r in seen if not r}) >= 4 and any(r for _, r in seen), seen  # the list reaches several periods and the refusal
    finally:
        h.close()


# ---- D: the ring protocol ----
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("wet", [True, False])
def test_ring_sizes_every_period_by_the_two_latest_rolls(pkg, E, oracle, wet, overlap):
    """1024 x 64, a group of 2, halo 42, local transport, one iteration per call, the overlapped and the in-order protocol: a jet that
    decays through the cone thresholds. The cones and periods of every slab after every call are the model's (watch_scenes.ring_model);
    no error is reported; the group ends bit for bit as one handle.
    [mutations: k_vx_roll reading without the exchange; ring_vx_roll ignoring the older slot; `* 1.25f + 0.25f` as `* 1.25f`]"""
    X, Y, halo, n = W.RING["X"], W.RING["Y"], W.RING["halo"], W.RING["iterations"]
    scene, u = W.ring_scene(wet)
    family = "wet_display" if wet else "dry_single"
    seen, _ = W.reference(oracle, scene, u, family, calls=((n, 0),))
    model, _ = W.ring_model(np.abs(scene[0][..., 0]).max(), [a.max() for a in seen], halo)
    model = [(m["cone"], m["period"]) for m in model]
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    g = E.Group(2, X, Y, halo=halo, devices=[0, 0], transport=E.TRANSPORT_LOCAL)
    whole = E.Handle(X, Y, 0)
    try:
        g.upload(*scene)
        g.set_params(p, u["initial_T"])
        whole.upload(*scene)
        whole.set_params(p, u["initial_T"])
        g.set_option(E.Handle.OPT_EXCHANGE_OVERLAP, overlap)
        if not wet:
            g.set_option(E.Handle.OPT_DRY_PAIRS, 0)
            whole.set_option(E.Handle.OPT_DRY_PAIRS, 0)
        got = []
        for _ in range(n):
            g.step(1)
            got.append([(s.slab_cone, s.slab_period) for s in g.slabs])
        g.sync()
        whole.step(n)
        assert all(x[0] == x[1] for x in got), got
        assert [x[0] for x in got] == model, (list(zip(model, got)), [float(a.max()) for a in seen])
        from test_group_transport import FIELDS
        for fld in FIELDS if wet else FIELDS[:3]:
            assert np.array_equal(g.read(fld), whole.read_rect(fld)), fld
    finally:
        g.close()
        whole.close()


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("wet", [True, False])
def test_group_reports_a_watched_site_in_its_iteration_and_no_unwatched_one(pkg, E, oracle, wet, overlap):
    """A group of 2 slabs at part B's geometry, one iteration per call, so that the split launches (edge strips first before the
    exchange, edge strips last behind it) run with their two strip ranges and ABSOLUTE strip indices: a pressure spike in the last
    watched strip before the interior of slab 1 accelerates the flow past the period's limit in the second (third) iteration -- the
    call in which the oracle shows it is the one whose sync reports it; the same spike in an unwatched strip is never reported and the
    group stays bit for bit one handle. [mutations: strip relative to the launch's first strip; zone_r rounded up]"""
    family = "wet_display" if wet else "dry_single"
    X, Y, halo = W.SLAB["X_global"], W.SLAB["Y"], W.SLAB["halo"]
    u = W.uniforms(family, Y)
    p = pkg.params.fill_struct(pkg.params.WxParams(), u)
    for name, (_, _, call) in W.GROUP_SITES.items():
        scene = W.group_scene(name)
        seen, _ = W.reference(oracle, scene, u, family, calls=((W.GROUP_CALLS, 0),))
        first = next((k + 1 for k, a in enumerate(seen) if a.max() >= np.float32(1.0)), None)
        assert first is not None and (call is None or first == call), (name, [float(a.max()) for a in seen])  # (tests/test_vx_watch_cpu.py)
        g = E.Group(2, X, Y, halo=halo, devices=[0, 0], transport=E.TRANSPORT_LOCAL)
        whole = E.Handle(X, Y, 0)
        try:
            g.upload(*scene)
            g.set_params(p, u["initial_T"])
            whole.upload(*scene)
            whole.set_params(p, u["initial_T"])
            g.set_option(E.Handle.OPT_EXCHANGE_OVERLAP, overlap)
            if not wet:
                g.set_option(E.Handle.OPT_DRY_PAIRS, 0)
                whole.set_option(E.Handle.OPT_DRY_PAIRS, 0)
            reported = None
            for k in range(1, W.GROUP_CALLS + 1):
                try:
                    g.step(1)
                    g.sync()
                except E.WxError as e:
                    assert e.code == WX_E_STATE and "|vx| reached" in str(e), e
                    reported = k
                    break
            assert reported == call, (name, reported, call, [float(a.max()) for a in seen])
            if call is None:
                assert all(s.slab_cone == 6 for s in g.slabs)
                whole.step(W.GROUP_CALLS)
                for fld in ("BASE_CUR", "WALL_CUR"):
                    assert np.array_equal(g.read(fld), whole.read_rect(fld)), (name, fld)
        finally:
            g.close()
            whole.close()
