"""The velocity-watch cases (tests/watch_scenes.py, run on the card by tests/test_vx_watch_gpu.py) accounted for on the oracle
alone: every item of the lane / row / value / zone lists is met by the case list and none is spare, the straddling pairs straddle,
the backgrounds stay below 0.5 at the measured stage, the ring scenes meet the four conditions their model needs. Removing a kernel
family, a lane group or a zone class from the lists makes a test of this file fail."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import impulse_scenes as I
import watch_scenes as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CASES = W.whole_cases()
SMALL_CASES = [c for c in CASES if (c["X"], c["Y"]) == W.SMALL]


# ---- the lists ----
def test_families_are_the_kernels_that_step():
    """One family per way an iteration can meet the trigger: the marching wet kernel (display iteration, plain iteration, piece), the
    one-iteration dry kernel, the pair kernel fresh (TAINT) and primed (plain), the per-pass set, the tiled dry kernel -- and every one of
    them appears in every part of the case list it can appear in."""
    assert set(W.FAMILIES) == {"wet_display", "wet_plain", "wet_piece", "dry_single", "dry_pairs_taint", "dry_pairs_plain", "perpass", "dry_tiled"}
    assert {f["kernel"] for f in W.FAMILIES.values()} == {"wet", "dry1", "dry2", "scan"}
    for grid in (W.SMALL, W.PHASE):
        assert {c["family"] for c in CASES if (c["X"], c["Y"]) == grid} == set(W.FAMILIES), grid
    assert {(c["family"], c["bands"]) for c in CASES if (c["X"], c["Y"]) == W.BANDS} == {(f, m) for f in ("wet_display", "dry_pairs_taint") for m in (0, 1, 2)}
    assert set(W.SLAB_FAMILIES) == set(W.FAMILIES)  # every family of part A can run on a lone slab
    assert {c["family"] for c in W.slab_cases()} == set(W.SLAB_FAMILIES)
    assert len({json.dumps(c, sort_keys=True) for c in CASES}) == len(CASES)
    # the strip widths are the kernels' (tests/test_impulse_cpu.py compares impulse_scenes' constants with the sources)
    assert (W.FAMILIES["wet_display"]["strip"], W.FAMILIES["dry_single"]["strip"], W.FAMILIES["dry_pairs_taint"]["strip"]) == (56, 60, 56)
    assert W.SMALL[0] == 3 * 56 + 1 == 2 * 60 + 49


def _lane_items(X, strip):
    """What the issue's column list asks of a family: label -> predicate over a column."""
    items = {"column 0": lambda x: x == 0, "column 1": lambda x: x == 1, "column X-2": lambda x: x == X - 2, "column X-1": lambda x: x == X - 1}
    if strip is None:
        items["interior"] = lambda x: 2 < x < X - 3
        return items
    full = (X // strip) * strip
    for lane in (0, 1, 2, strip - 3, strip - 2, strip - 1):
        items["lane %d of a whole strip" % lane] = lambda x, lane=lane: x < full and x % strip == lane
    items["interior lane"] = lambda x: x < full and 3 <= x % strip < strip - 3
    items["first column of the ragged strip"] = lambda x: x == full
    items["last column of the ragged strip"] = lambda x: x == X - 1 and X % strip != 0
    return items


def _row_items(Y, segments):
    firsts, lasts = {lo for lo, _ in segments if lo > 0}, {hi - 1 for _, hi in segments if hi < Y}
    return {"row 1": lambda y: y == 1, "row Y-2": lambda y: y == Y - 2, "first row of a segment": lambda y: y in firsts, "last row of a segment": lambda y: y in lasts}


@pytest.fixture(scope="module")
def wet_segments(tmp_path_factory):
    """The wet kernel's row segments on the grids of part A, from the launch-shape harness of tests/test_launch_shape_cpu.py."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("shape") / "shape_harness")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-DWX_DEBUG", "-Wno-unused-value", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "shape_harness.hip")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("WX_WET_")}
    out = {}
    for sh in json.loads(subprocess.check_output([exe] + [str(v) for g in (W.SMALL, W.PHASE) for v in g], env=env)):
        assert sh["bands"] == 0
        out[(sh["X"], sh["Y"])] = list(zip(sh["start"], sh["start"][1:]))
    # the band grid under the three WX_OPT_ROW_BANDS modes (the harness takes the mode from the debug switch; 1 is the default)
    for mode, e in ((0, {"WX_WET_BANDS": "0"}), (1, {}), (2, {"WX_WET_BANDS": "2"})):
        (sh,) = json.loads(subprocess.check_output([exe] + [str(v) for v in W.BANDS], env=dict(env, **e)))
        out[("bands", mode)] = (bool(sh["bands"]), tuple(sh["start"]))
    return out


def test_dry_segments_are_the_launch_shapes(tmp_path_factory):
    """The 8-row segments watch_scenes.dry_segments states for 169 x 52, from the launch functions. The one-iteration dry kernel:
    march_seg_rows (csrc/wx_march.h) through a host-only harness -- it returns its minimum of 8 rows whenever the device holds at least
    strips x ceil(Y / 8) = 21 waves at once, which every device does (the harness falls back to 8192 without one), and Y % 8 != 0 keeps
    launch_march_dry from cutting row bands. The pair kernel: launch_march_dry2 takes max(8, min(128, (3 (Y / 8) / 16) & ~3)) = 8 rows --
    no device figure enters while Y % 8 != 0 (its fill rule and its bands need Y % 8 == 0)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("shape") / "march_shape_harness")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-DWX_DEBUG", "-Wno-unused-value", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "march_shape_harness.hip")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("WX_MARCH")}
    X, Y = W.SMALL
    (sh,) = json.loads(subprocess.check_output([exe, str(X), str(Y)], env=env))
    assert Y % 8 != 0 and sh["n_strips"] == (X + 59) // 60 and sh["n_strips"] * ((Y + 7) // 8) <= 256 <= sh["capacity"]
    assert W.dry_segments(X, Y, 60) == [(lo, min(lo + sh["seg_rows"], Y)) for lo in range(0, Y, sh["seg_rows"])]
    R = max(8, min(128, ((3 * (Y // 8)) // 16) & ~3))
    assert W.dry_segments(X, Y, 56) == [(lo, min(lo + R, Y)) for lo in range(0, Y, min(R, Y))]
    assert (7, 8) in [(a[1] - 1, b[0]) for a, b in zip(W.dry_segments(X, Y, 60), W.dry_segments(X, Y, 60)[1:])]  # rows 7 | 8 of the case list: a border


def _segments(family, wet_segments):
    f = W.FAMILIES[family]
    if f["strip"] is None:
        return [(0, W.SMALL[1])]
    return wet_segments[W.SMALL] if f["kernel"] == "wet" else W.dry_segments(W.SMALL[0], W.SMALL[1], f["strip"])


def _missing(family, cases, wet_segments):
    X, Y = W.SMALL
    f = W.FAMILIES[family]
    lane_cases = [c for c in cases if c["group"] in W.LANE_GROUPS]
    miss = [k for k, ok in _lane_items(X, f["strip"]).items() if not any(ok(c["x"]) for c in lane_cases)]
    rows = _row_items(Y, _segments(family, wet_segments))
    if f["strip"] is None:
        rows = {k: v for k, v in rows.items() if k.startswith("row ")}
    miss += [k for k, ok in rows.items() if not any(ok(c["y"]) for c in lane_cases)]
    vals = W.SIGNED if f["stage"] is not None else W.SIGNED_SCAN[family]
    miss += ["value %r" % v for v in vals if not any(c["vx"] == v for c in lane_cases)]
    for x in {c["x"] for c in lane_cases}:  # every column meets both signs, and every row
        here = [c for c in lane_cases if c["x"] == x]
        if {np.sign(c["vx"]) for c in here} != {-1.0, 1.0}:
            miss.append("both signs in column %d" % x)
        if f["strip"] is not None and {c["y"] for c in here} != set(W.ROWS[W.SMALL]):
            miss.append("every row in column %d" % x)
    groups = {c["group"] for c in cases}
    miss += [g for g in ("vy_only",) + (("below_half", "above_half") if f["stage"] is not None else ()) + (("second_iteration",) if f["kernel"] == "dry2" else ())
             if g not in groups]
    return miss


@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_lane_row_and_value_accounting(family, wet_segments):
    """Computed from the case list: the 169 x 52 cases of a family meet every column item (in ITS strip width), every row item (in ITS
    row segments), every value with both signs in every column -- and no lane group, row or value is spare: without any one of them
    something is lost."""
    mine = [c for c in SMALL_CASES if c["family"] == family]
    assert not _missing(family, mine, wet_segments)
    f = W.FAMILIES[family]
    for g in {c["group"] for c in mine}:
        assert _missing(family, [c for c in mine if c["group"] != g], wet_segments), "lane group %s of %s covers nothing of its own" % (g, family)
    if f["strip"] is not None:
        for y in W.ROWS[W.SMALL]:
            assert _missing(family, [c for c in mine if c["y"] != y or c["group"] not in W.LANE_GROUPS], wet_segments), "row %d is spare" % y
    for v in {c["vx"] for c in mine if c["group"] in W.LANE_GROUPS}:
        assert _missing(family, [c for c in mine if c["vx"] != v], wet_segments), "value %r is spare" % v
    # the phase grid's site: the one-column ragged strip of the 56-column kernels, a segment boundary of the wet kernel (38 | 39)
    (c,) = [c for c in CASES if c["family"] == family and (c["X"], c["Y"]) == W.PHASE]
    assert c["x"] == W.PHASE[0] - 1 and W.PHASE[0] % 56 == 1
    if f["kernel"] == "wet":
        assert c["y"] + 1 in {lo for lo, _ in wet_segments[W.PHASE]}


def test_band_cases_meet_every_segment_border(oracle, wet_segments):
    """2500 x 300 under the three ROW_BANDS modes: the literal tables of watch_scenes are the launch shape's (the harness); the absolute
    segments -- band start + table start, clipped to the band -- cover every row once; every row that is the last row of a segment or the
    first of the next one carries exactly one lone-cell case of the wet kernel, none is spare, and columns and values all come up in
    every mode. On the oracle: every such cell is measured at 0.5 or more; the window of 128 columns the GPU test takes its reference
    from holds the bits of the whole grid (a sample of cases), and the whole background stays below 0.5."""
    X, Y = W.BANDS
    bg = W.background(X, Y)
    u = W.uniforms("wet_display", Y)
    quiet, _ = W.reference(oracle, bg, u, "wet_display")
    assert quiet[0].max() < W.HALF
    for mode in (0, 1, 2):
        assert wet_segments[("bands", mode)] == W.BAND_TABLES[mode], mode
        segs = W.band_segments(mode)
        assert [r for lo, hi in segs for r in range(lo, hi)] == list(range(Y)), mode
        borders = {lo for lo, _ in segs if lo > 0}
        want_rows = sorted({r for b in borders for r in (b - 1, b) if 1 <= r <= Y - 2})
        mine = [c for c in CASES if c["family"] == "wet_display" and c.get("bands") == mode]
        assert sorted(c["y"] for c in mine) == want_rows == W.band_border_rows(mode), mode  # every border from both sides, one case per row, none spare
        if W.BAND_TABLES[mode][0]:  # the short tail segments of every band and the clipped last segment of the 37-row bands are among them
            heights = {hi - lo for lo, hi in segs}
            assert {1, 2} <= heights and {(k + 1) * Y // 8 - k * Y // 8 for k in range(8)} == {37, 38}
            assert len(segs) == sum(11 if (k + 1) * Y // 8 - k * Y // 8 == 38 else 10 for k in range(8))
        assert {c["x"] for c in mine} == set(W.BAND_COLUMNS) and {c["vx"] for c in mine} == set(W.SIGNED)
        for k, c in enumerate(mine):
            crop = W.cropped_reference(oracle, c, bg)
            want = W.expected_take(crop)
            assert want >= W.HALF, (c, float(crop[0].max()))
            if k % 40 == 0:
                full, _ = W.reference(oracle, W.whole_scene(c, bg), u, "wet_display")
                assert W.bits(W.expected_take(full)) == W.bits(want), c
                y, x = np.unravel_index(full[0].argmax(), full[0].shape)
                assert (int(x), int(y)) == (c["x"], c["y"])
    assert {(c["family"], c["bands"]) for c in CASES if c["family"] == "dry_pairs_taint" and "bands" in c} == {("dry_pairs_taint", m) for m in (0, 1, 2)}


# ---- the scenes on the oracle ----
@pytest.fixture(scope="module")
def references(oracle):
    """(family, x, y, vx, vy) -> per-iteration maxima, expected take and where the first iteration's maximum lies, for every 169 x 52
    and 505 x 77 case (computed once)."""
    bgs = {g: W.background(*g) for g in (W.SMALL, W.PHASE)}
    out = []
    for c in CASES:
        g = (c["X"], c["Y"])
        if g == W.BANDS:
            continue
        seen, _ = W.reference(oracle, W.whole_scene(c, bgs[g]), W.uniforms(c["family"], c["Y"]), c["family"])
        rest = [a.copy() for a in seen]
        for a in rest:  # everything but the 3 x 3 cells around the site
            a[max(0, c["y"] - 1):c["y"] + 2, [(c["x"] + d) % c["X"] for d in (-1, 0, 1)]] = 0
        out.append((c, [np.float32(a.max()) for a in seen], W.expected_take(seen), np.unravel_index(seen[0].argmax(), seen[0].shape), max(float(a.max()) for a in rest)))
    return out


def test_lone_cells_are_seen_and_backgrounds_stay_below_half(references):
    """In every iteration run, everything but the planted cell's 3 x 3 neighbourhood is below 0.5 at the measured stage (marching
    families) -- so the expected take IS the lone cell's value; it is 0.5 or more in every lane / row / phase-grid case of a marching
    family and attained at the site in the first iteration, never later. The scan families look at the state after a whole iteration,
    where a spike has spread: 0.5 or more in four of five of their cases."""
    scan_ok = scan_n = 0
    for c, maxima, want, where, rest in references:
        f = W.FAMILIES[c["family"]]
        lane = c["group"] in W.LANE_GROUPS or c["group"] == "phase_grid"
        if f["stage"] is not None and c["group"] != "second_iteration":
            assert rest < 0.5, (c, rest)
            assert all(m < W.HALF for m in maxima[1:]), (c, maxima)
            if lane:
                assert want >= W.HALF and want == maxima[0] and where == (c["y"], c["x"]), (c, maxima, where)
        elif lane:
            scan_n += 1
            scan_ok += bool(want >= W.HALF)
        if c["group"] == "second_iteration":  # the pair's second iteration is the faster one, next to a strip border on either side
            assert f["kernel"] == "dry2" and W.HALF <= maxima[0] < maxima[1] == want, (c, maxima)
            assert c["x"] % 56 in (0, 1, 2, 3, 52, 53, 54, 55)
            continue
        if c["group"] == "vy_only":
            assert want == 0.0 and c["vy"] == 3.0 and c["vx"] == 0.0, (c, maxima)  # the cone depends on vx alone
    assert scan_ok * 5 >= scan_n * 4 and scan_n >= 20, (scan_ok, scan_n)
    for fam in ("perpass", "dry_tiled"):
        signs = {np.sign(c["vx"]) for c, _, want, _, _ in references if c["family"] == fam and want >= W.HALF}
        assert signs == {-1.0, 1.0}, fam


def test_straddling_pairs_straddle(oracle):
    """The literal pairs of tools/find_watch_straddles.py: float32 neighbours whose measured-stage values lie on either side of the
    threshold, closer together than 2^-10 of it."""
    assert set(W.STRADDLES) == {(n, s) for n in W.STRADDLE_SITES for s in (7, 1)}
    for (name, stage), (a, b) in W.STRADDLES.items():
        thr = np.float32(W.STRADDLE_SITES[name][3])
        assert np.float32(b) == np.nextafter(np.float32(a), np.float32(np.inf))
        ma, mb = W.straddle_measured(oracle, name, stage, a), W.straddle_measured(oracle, name, stage, b)
        gap = float(mb - ma) / float(thr)
        assert ma < thr <= mb and gap < 2.0 ** -10, "%s stage %d: measured %r < %r <= %r, gap %.3g of the threshold" % (name, stage, float(ma), float(thr), float(mb), gap)
    assert W.STRADDLE_SITES["period"][1] in W.MUST_SEE and W.STRADDLE_SITES["interior"][1] in W.NEVER_RECORDED
    assert W.INTERIOR_LIMIT == 16.0


def test_spiked_scene_is_faster_in_the_second_iteration_of_its_second_pair(oracle):
    """What test_pair_kernels_recomputed_cells_are_watched needs: iteration 4 (the second of the second pair) is the faster one of its
    pair, 0.9 or more -- its cell is recorded -- and within the 8 x 8 tile neighbourhood of a first-iteration cell (iteration 3) of 0.9
    or more, which the TAINT instantiation turns into NaN: the march itself cannot have seen it."""
    X, Y = W.PHASE
    base, water, wall, _, _ = I.impulse_scene(X, Y, "fast_vx", offset=W.SPIKED_OFFSET, fast_values=I.DRY_FAST_VALUES)
    u = W.uniforms("dry_pairs_taint", Y)
    seen, _ = W.reference(oracle, (base, water, wall), u, "dry_pairs_taint", calls=((4, 0),))
    m = [float(a.max()) for a in seen]
    assert m[0] > 79.9 and m[3] > m[2] >= 0.9, m
    y, x = np.unravel_index(seen[3].argmax(), seen[3].shape)
    near = seen[2][max(0, y - 2):y + 3, [(x + d) % X for d in range(-2, 3)]]
    assert near.max() >= 0.9, (x, y, near.max())


# ---- part B ----
def test_zone_classes():
    """The contract's zone is local columns c < 36 or c >= 244; the launch functions round it to whole strips: 0 and 4 for 56- and for
    60-column strips alike. Every must-see column is in the zone and outside the outermost cone, every never-recorded one lies in an
    unwatched strip of BOTH widths, out of reach of a watched wave's load columns -- one per unwatched strip; nothing is planted in between."""
    halo, X = W.SLAB["halo"], W.SLAB_LOCAL
    assert X == 280 and 3 * halo == 36 and X - 3 * halo == 244
    for w in (56, 60):
        assert ((3 * halo + w - 1) // w, (X - 3 * halo) // w) == (1, 4)
    classes = [W.zone_class(c) for c in range(X)]
    assert [c for c in range(X) if classes[c] == "must_see"] == list(range(6, 36)) + list(range(244, 274))
    never = [c for c in range(X) if classes[c] == "never"]
    assert never == list(range(64, 216))
    assert all(W.zone_class(c) == "must_see" for c in W.MUST_SEE) and all(c in never for c in W.NEVER_RECORDED)
    assert W.MUST_SEE == (8, 35, 244, 271)  # both ends of both sides of the zone
    for w in (56, 60):
        assert sorted(c // w for c in W.NEVER_RECORDED) == [1, 2, 3]
    for fam in W.SLAB_FAMILIES:
        mine = [c for c in W.slab_cases() if c["family"] == fam]
        assert {c["c"] for c in mine if c["class"] == "must_see"} == set(W.MUST_SEE) and {c["c"] for c in mine if c["class"] == "never"} == set(W.NEVER_RECORDED)
        assert {c["class"] for c in mine} == {"must_see", "never"}
        assert {c["x0"] for c in mine} == set(W.SLAB["x0s"]) and {np.sign(c["vx"]) for c in mine} == {-1.0, 1.0}
    # the wrap of the global column index lies inside either array: between the left ghost columns and the owned ones (x0 = 0), between
    # the owned ones and the right ghost columns (x0 = 256, whose last owned column is the domain's)
    assert [int(np.nonzero(np.diff(W.slab_window(x0)) != 1)[0][0]) for x0 in W.SLAB["x0s"]] == [halo - 1, halo + W.SLAB["X_owned"] - 1]


def test_slab_sites_on_the_oracle(oracle):
    """Per lone-slab case, on the whole-domain oracle in local columns: all cells of 0.5 and more lie in the class of the site (a
    must-see site: in the compared part of the zone; a never-recorded one: in the never-recorded columns, below the interior limit);
    and on the oracle of the LOCAL array (periodic across its 280 columns, as the kernels load it) the columns left out of the
    comparison -- the front of invalid ghost columns -- hold only background, below 0.5."""
    classes = np.array([W.zone_class(c) for c in range(W.SLAB_LOCAL)])
    for c in W.slab_cases():
        f = W.FAMILIES[c["family"]]
        u = W.uniforms(c["family"], W.SLAB["Y"])
        scene = W.slab_scene(c["c"], c["x0"], c["vx"])
        seen, _ = W.reference(oracle, scene, u, c["family"])
        local = [a[:, W.slab_window(c["x0"])] for a in seen]
        cols = W.scan_zone_columns() if f["stage"] is None else W.valid_columns(len(seen))
        for j, a in enumerate(local):
            fast = np.nonzero((a >= W.HALF).any(0))[0]
            if c["class"] == "never":
                assert set(classes[fast]) <= {"never"} and a.max() < W.INTERIOR_LIMIT, (c, fast)
            elif f["stage"] is not None:
                assert set(classes[fast]) <= {"must_see"} and set(fast) <= set(cols[j]), (c, fast)
            else:  # (the scan looks at the state after the iteration: a spike at the zone's inner end has spread into the columns next to it)
                assert set(classes[fast]) <= {"must_see", "either"}, (c, fast)
        if c["class"] == "must_see" and f["stage"] is not None:
            assert W.expected_take(local, cols) == np.float32(local[0][:, c["c"]].max()) >= W.HALF, c
        front = W.slab_local_oracle(oracle, scene, c["x0"], u, c["family"])
        for j, a in enumerate(front):
            out = np.ones(W.SLAB_LOCAL, bool)
            out[cols[j]] = False
            if f["stage"] is None:
                out[36:244] = False  # (not scanned into the accumulator)
            assert a[:, out].max() < W.HALF, (c, j, float(a[:, out].max()))


# ---- part D ----
@pytest.mark.parametrize("wet", [True, False])
def test_ring_scene_meets_the_models_conditions(oracle, wet):
    """From the oracle alone: every cell of 0.5 and more lies at owned offsets [50, 126) of some slab in every iteration (the must-see
    zone of its slab, no neighbour's ghost columns); at every exchange the modelled 1.25 v + 0.25 is at least 0.1 away from an integer;
    the cone takes three different values and at least once the OLDER of the two rolls decides -- and decides differently than the
    newer one alone would; no modelled iteration reaches its period's limit. And for the overlapped protocol, whose roll runs behind
    the EDGE strips only: in the iteration before every exchange the strips launched behind it (owned offsets 70 and more) stay below
    0.5 or below the roll they would be counted in instead."""
    X, halo, n = W.RING["X"], W.RING["halo"], W.RING["iterations"]
    scene, u = W.ring_scene(wet)
    seen, _ = W.reference(oracle, scene, u, "wet_display" if wet else "dry_single", calls=((n, 0),))
    xo = X // W.RING["slabs"]
    lo, hi = W.RING["offsets"]
    for k, a in enumerate(seen):
        offs = np.nonzero((a >= W.HALF).any(0))[0] % xo
        assert len(offs) and offs.min() >= lo and offs.max() < hi, (k, offs.min(), offs.max())
    model, exchanges = W.ring_model(np.abs(scene[0][..., 0]).max(), [a.max() for a in seen], halo)
    assert not any(m["reached_limit"] for m in model)
    assert len({m["cone"] for m in model}) >= 3, [m["cone"] for m in model]
    deciding = 0
    for e in exchanges:
        b = 1.25 * e["sized_by"] + 0.25
        assert abs(b - round(b)) >= 0.1, e
    rolls = [e["roll"] for e in exchanges]
    for i, e in enumerate(exchanges):
        if e["older_decides"]:
            deciding += W.sizing(rolls[i - 2], halo)[0] != W.sizing(rolls[i - 1], halo)[0]
    assert deciding >= 1, exchanges
    edge = min((2 * halo - 1) // w + 1 for w in (56, 60)) * 56 - halo  # owned offset where the strips launched behind the edge group begin
    assert edge == 70
    for i, e in enumerate(exchanges[:-1]):
        a = seen[e["after_iteration"]]
        late = np.float32(a[:, [x for x in range(X) if x % xo >= edge]].max())
        assert late < W.HALF or late <= np.float32(exchanges[i + 1]["roll"]), (e, float(late))


@pytest.mark.parametrize("family", ["wet_display", "dry_single"])
def test_group_sites_on_the_oracle(oracle, family):
    """The pressure spikes of the 2-slab group case: the uploaded flow is below 0.5 (the bootstrap keeps cone 6, limit 1.0); the oracle
    shows |vx| >= 1.0 for the first time in the listed call; all cells of 0.5 and more stay in the site's class of slab 1 -- strip 0 of
    both strip widths for the watched site, the never-recorded columns for the other -- below the interior limit, and out of slab 0's
    local array altogether."""
    u = W.uniforms(family, W.SLAB["Y"])
    win0, win1 = W.slab_window(0), W.slab_window(W.SLAB["X_owned"])
    classes = np.array([W.zone_class(c) for c in range(W.SLAB_LOCAL)])
    assert {v[2] for v in W.GROUP_SITES.values()} == {2, 3, None}
    for name, (c_local, A, call) in W.GROUP_SITES.items():
        scene = W.group_scene(name)
        assert np.abs(scene[0][..., 0]).max() < W.HALF
        seen, _ = W.reference(oracle, scene, u, family, calls=((W.GROUP_CALLS, 0),))
        first = next((k + 1 for k, a in enumerate(seen) if a.max() >= np.float32(1.0)), None)
        assert first is not None and (call is None or first == call), (name, [float(a.max()) for a in seen])
        for a in seen[:first if call is not None else None]:
            assert a.max() < W.INTERIOR_LIMIT
            assert a[:, win0].max() < W.HALF
            fast = np.nonzero((a[:, win1] >= W.HALF).any(0))[0]
            if call is None:
                assert set(classes[fast]) <= {"never"}, (name, fast)
            else:
                # (inside the watched strip of both strip widths: 0, or 4 -- which begins at column 240 for the 60-column kernel)
                inside = fast.max() < 56 - 8 if c_local < 140 else fast.min() >= 240 + 2
                assert len(fast) == 0 or (inside and set(classes[fast]) <= {"must_see", "either"}), (name, fast)
