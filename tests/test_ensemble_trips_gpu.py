"""The second and later trips of the ensemble kernels' chunk loops on the GPU. Every case of tests/ensemble_trip_shapes.py -- shapes
at which the busiest wave or workgroup of k_ens_stat, k_ens_assim, k_ens_score, k_ens_quant_staged, k_ens_quant_stream and
k_ens_perturb goes through its loop two, three or five times (tests/test_ensemble_trips_cpu.py holds the shapes to the kernels' caps
and the host functions to the definition on the same arrays) -- is run on the device and compared with the call's host function over
the WHOLE rectangle, `==` on bits (NaNs compared as positions); a failure names the first differing cell with its chunk and trip.
The members are uploaded, not stepped: smooth fields plus noise, sparse walls per member, and the planted cells of each call's own CPU
test in rows of the first and of the last trip, read back through a clone before anything is computed.

The tests are named for what only a later trip executes (DESIGN.md section 3 lists the hand mutations that fail them and pass every
other ensemble test)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ensemble_trip_shapes as T
from test_ensemble_assimilate_gpu import same_results
from test_ensemble_gpu import same_bits
from test_ensemble_perturb_gpu import pre_values
from test_ensemble_quantiles_cpu import P8
from test_ensemble_scores_cpu import ALL, MAPS
from test_ensemble_statistics_cpu import PLANES, THRESHOLD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = T.caps()
FIELD_KEY = {T.B_: "base", T.W_: "water"}


def ids(call):
    return [c.id for c in T.by_call(call)]


def upload(pkg, grid, reverse=False):
    """The grid's members as an ensemble (`reverse`: member i in slot n - 1 - i) and, on the scores grid, the truth as a lone handle."""
    X, Y, B, _ = T.GRIDS[grid]
    m = T.members(grid)
    n = B - 1 if grid == "scores" else B
    P = pkg.params
    u = P.uniforms_from_gui(P.merge_settings(None), Y)  # (nothing is stepped: wx_copy_state asks for parameters, whatever they are)
    ens = pkg.engine.Ensemble(n, X, Y, 0)
    for i in range(n):
        slot = ens[n - 1 - i if reverse else i]
        slot.upload(m["base"][i], m["water"][i], m["wall"][i])
        slot.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
    truth = None
    if grid == "scores":
        truth = pkg.engine.Handle(X, Y)
        truth.upload(m["base"][n], m["water"][n], m["wall"][n])
        truth.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
    return ens, truth


def assert_the_planted_bits_survived(pkg, grid, ens, truth):
    """What the device holds, read through a clone, is what was built: every bit of every member (NaN payloads too), the planted
    blocks of the first and of the last trip by name."""
    X, Y, B, _ = T.GRIDS[grid]
    m = T.members(grid)
    held = pre_values(pkg, ens)
    if truth is not None:
        held.append({f: truth.read_rect(f) for f in (T.B_, T.W_, "WALL_CUR")})
    assert len(held) == B
    for name, first, last, s in T.planted_blocks(grid):
        f, w = T.planted_cells(name, B)
        for i in range(B):
            for row in (first, last):
                for field in (T.B_, T.W_):
                    assert T.block_view(held[i][field], row, X, s).view(np.uint32).tobytes() == f[i].view(np.uint32).tobytes(), (grid, name, "member", i, "row", row, field)
                assert np.array_equal(T.block_view(held[i]["WALL_CUR"], row, X, s), w[i]), (grid, name, "member", i, "row", row)
    for i in range(B):
        assert held[i][T.B_].view(np.uint32).tobytes() == m["base"][i].view(np.uint32).tobytes(), (grid, i)
        assert held[i][T.W_].view(np.uint32).tobytes() == m["water"][i].view(np.uint32).tobytes(), (grid, i)
        assert np.array_equal(held[i]["WALL_CUR"], m["wall"][i]), (grid, i)


@pytest.fixture(scope="module")
def uploaded(pkg):
    made = {}

    def get(grid, reverse=False):
        if (grid, reverse) not in made:
            made[(grid, reverse)] = upload(pkg, grid, reverse)
            if not reverse:
                assert_the_planted_bits_survived(pkg, grid, *made[(grid, reverse)])
        return made[(grid, reverse)]

    yield get
    for ens, truth in made.values():
        ens.close()
        if truth is not None:
            truth.close()


def cut(arrays, rect):
    x, y, w, h = rect
    return [np.ascontiguousarray(a[y:y + h, x:x + w]) for a in arrays]


def assert_planes(case, geo, got, want):
    assert set(got) == set(want), (case.id, sorted(got), sorted(want))
    for k in want:
        msg = T.first_difference(case, geo, got[k], want[k], k)
        assert msg is None, msg


def score_call(case, ens, truth, sel):
    return ens.scores(case.kw["field"], truth, *case.rect, members=sel, want=MAPS if case.kw["maps"] else ())


def assert_scores(case, geo, got, want, where):
    """Every sum, count and reason and both rank histograms; the maps cell by cell."""
    assert set(got) == set(want) == (set(ALL) if case.kw["maps"] else set(ALL) - set(MAPS)), (case.id, where)
    for k in want:
        if k in MAPS:
            msg = T.first_difference(case, geo, got[k], want[k], "%s, %s" % (where, k))
            assert msg is None, msg
        else:
            assert same_bits(np.asarray(got[k]), np.asarray(want[k])), (case.id, where, k, "of %d chunks in %d trips" % (geo.chunks, geo.trips),
                                                                       np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist())


@pytest.mark.parametrize("case", T.by_call("scores"), ids=ids("scores"))
def test_scores_carry_sums_counts_and_histograms_across_trips(pkg, uploaded, case):
    """k_ens_score: cur[] / acc[], cnt[] and sum_n live across the chunk loop and are flushed once, the LDS histograms are zeroed once,
    the image is staged over on every trip (with the maps: behind the extra barrier), the shard is blockIdx % 8. All three maps, none,
    and a rectangle at an odd offset; 3 and 9 selected members; the same members in reversed slots give the same bits."""
    ens, truth = uploaded("scores")
    geo = T.geometry(case, CAPS)
    assert geo.trips >= 3
    m = T.members("scores")
    f, w = cut(m[FIELD_KEY[case.kw["field"]]], case.rect), cut(m["wall"], case.rect)
    sel = T.selection(case)
    want = pkg.engine.ens_score_cells(f[:-1], w[:-1], f[-1], w[-1], members=sel, want=MAPS if case.kw["maps"] else ())
    got = score_call(case, ens, truth, sel)
    assert_scores(case, geo, got, want, "device against host function")
    assert (want["n_scored"] > 0).all() and (want["rank_low"] > 0).sum() > 4
    rens, _ = uploaded("scores", reverse=True)
    n = len(ens.members)
    assert_scores(case, geo, score_call(case, rens, truth, sorted(n - 1 - i for i in sel)), got, "reversed slots against the first order")


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import ensemble_trip_shapes as S
import test_ensemble_trips_gpu as G
ens, truth = G.upload(pkg, "scores")
out = {}
for case in S.by_call("scores"):
    if case.id in G.FAST_CASES:
        for k, v in G.score_call(case, ens, truth, S.selection(case)).items():
            out[case.id + ":" + k] = v
ens.close(); truth.close()
np.savez(sys.argv[2], **out)
"""
FAST_CASES = ("scores-9-maps", "scores-3-offset")


def test_scores_across_trips_under_the_tolerance_build(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernel gives THIS process's host function's bits."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    dst = str(tmp_path / "fast.npz")
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, ROOT, dst], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(dst)
    m = T.members("scores")
    for case in T.by_call("scores"):
        if case.id not in FAST_CASES:
            continue
        f, w = cut(m[FIELD_KEY[case.kw["field"]]], case.rect), cut(m["wall"], case.rect)
        want = pkg.engine.ens_score_cells(f[:-1], w[:-1], f[-1], w[-1], members=T.selection(case), want=MAPS)
        assert_scores(case, T.geometry(case, CAPS), {k: d[case.id + ":" + k] for k in ALL}, want, "tolerance build against host function")


@pytest.mark.parametrize("case", T.by_call("statistics"), ids=ids("statistics"))
def test_statistics_row_and_output_offset_at_large_chunk_indices(pkg, uploaded, case):
    """k_ens_stat: y = ch / cpr and the output offset o on a later trip. All nine planes, with and without the variance pass, 3
    selected members (the remainder loop alone) and 9 (a load group of 8 and one). The members are what the device holds NOW (the
    perturbation and assimilation cases of this file change them)."""
    ens, _ = uploaded("state")
    geo = T.geometry(case, CAPS)
    pre = pre_values(pkg, ens)
    f, w = [p[case.kw["field"]] for p in pre], [p["WALL_CUR"] for p in pre]
    planes = PLANES if case.kw["variance"] else tuple(p for p in PLANES if p != "variance")
    want = pkg.engine.ens_stat_cells(f, w, members=case.sel, threshold=THRESHOLD, want=planes)
    got = ens.statistics(case.kw["field"], members=case.sel, threshold=THRESHOLD, want=planes)
    assert_planes(case, geo, got, want)
    last = want["count"][-(geo.h - (geo.workers // geo.cpr)):]  # rows of the last trip: values entered there
    assert (last == len(T.selection(case))).any() and (want["n_wall"] > 0).any()


@pytest.mark.parametrize("case", T.by_call("quantiles"), ids=ids("quantiles"))
def test_quantiles_restage_the_image_on_every_trip(pkg, uploaded, case):
    """k_ens_quant_staged: the LDS image holds the keys, the sorted column and the result rows in turn and is staged over for the next
    chunk (3 members on two and on three trips; 64 members: the 64 KiB image); k_ens_quant_stream at 65 members: the 64-bit item split
    into (chunk, channel) on the second trip, with one and with two chunks per row. Eight quantiles, the interpolations going round
    the cases, the rank of a member outside the selection."""
    ens, _ = uploaded(case.grid)
    geo = T.geometry(case, CAPS)
    m = T.members(case.grid)
    f, w = m[FIELD_KEY[case.kw["field"]]], m["wall"]
    want = pkg.engine.ens_quant_cells(f, w, P8, members=case.sel, interp=case.kw["interp"], rank_of=case.kw["rank_of"])
    got = ens.quantiles(case.kw["field"], P8, members=case.sel, interp=case.kw["interp"], rank_of=case.kw["rank_of"])
    assert got["q"].shape == (8, geo.h, geo.w, 4)
    assert_planes(case, geo, got, want)
    assert (want["n_below"] >= 0).any() and (want["count"] == len(case.sel)).any()


@pytest.mark.parametrize("case", T.by_call("perturb"), ids=ids("perturb"))
def test_perturb_splits_the_item_into_member_and_chunk(pkg, uploaded, case):
    """k_ens_perturb: the 64-bit item index is split into (member, chunk) by it / per_member, and one wave's consecutive trips land in
    different members. Both fields, add and mul, wrap_x, every member without a mask, [0, 1, 2] and [0, 2]; unselected members and
    wall cells keep their bits, and so does the other field."""
    ens, _ = uploaded("state")
    X, Y, B, _ = T.GRIDS["state"]
    geo = T.geometry(case, CAPS)
    kw = dict(case.kw)
    field, mode = kw.pop("field"), kw.pop("mode")
    other = T.W_ if field == T.B_ else T.B_
    pre = pre_values(pkg, ens)
    sel = T.selection(case)
    assert geo.workers // geo.chunks != 0  # wave 0's second item lies in another member than its first
    want = pkg.engine.ens_perturb_cells([p[field] for p in pre], [p["WALL_CUR"] for p in pre], X, Y, field, T.PERTURB_AMP[field], mode=mode, members=case.sel, **kw)
    ens.perturb(field, T.PERTURB_AMP[field], mode=mode, members=case.sel, **kw)
    for i, member in enumerate(ens.members):
        got = member.read_rect(field)
        msg = T.first_difference(case, geo, got, want[i], "member %d" % i, sel.index(i) if i in sel else 0)
        assert msg is None, msg
        wall_cells = pre[i]["WALL_CUR"][..., 1] == 0
        assert wall_cells.any() and same_bits(got[wall_cells], pre[i][field][wall_cells]), (case.id, "wall cells of member", i)
        assert same_bits(got, pre[i][field]) == (i not in sel), (case.id, "member", i, "selected" if i in sel else "not selected")
        assert same_bits(member.read_rect(other), pre[i][other]) and same_bits(member.read_rect("WALL_CUR"), pre[i]["WALL_CUR"]), (case.id, i)


@pytest.mark.parametrize("case", T.by_call("assimilate"), ids=ids("assimilate"))
def test_assimilate_rereads_its_own_stores_on_every_trip(pkg, uploaded, case):
    """k_ens_assim: y = ch / cpr on a later trip, and inside each trip the lane reads back, for observation j + 1, what it stored for
    observation j. Eight observations of both fields in rows of the first trip, of the last trip and on both sides of the boundary
    between them; every cell in reach of every observation (loc 0, 0) and localized (9, 300); 3 and 9 selected members."""
    ens, _ = uploaded("state")
    X, Y, B, _ = T.GRIDS["state"]
    geo = T.geometry(case, CAPS)
    pre = pre_values(pkg, ens)
    obs = T.observations()
    sel = T.selection(case)
    bases, waters, walls = [p[T.B_] for p in pre], [p[T.W_] for p in pre], [p["WALL_CUR"] for p in pre]
    want_b, want_w, want_res = pkg.engine.ens_assim_cells(bases, waters, walls, X, Y, obs, members=case.sel, **case.kw)
    res = ens.assimilate(obs, members=case.sel, **case.kw)
    assert same_results(res, want_res), (case.id, [(a, b) for a, b in zip(res, want_res) if not same_results([a], [b])][:2])
    assert all(r["applied"] for r in res)
    for i, member in enumerate(ens.members):
        for field, want, before in ((T.B_, want_b[i], bases[i]), (T.W_, want_w[i], waters[i])):
            got = member.read_rect(field)
            msg = T.first_difference(case, geo, got, want, "%s of member %d" % (field, i))
            assert msg is None, msg
            wall_cells = walls[i][..., 1] == 0
            assert same_bits(got[wall_cells], before[wall_cells]), (case.id, field, "wall cells of member", i)
            assert same_bits(got, before) == (i not in sel), (case.id, field, "member", i)
            if i in sel:  # the update reached rows of the first and of the last trip
                d = T.differs(got, before).any(axis=(1, 2))
                assert d[:geo.workers // geo.cpr].any() and d[geo.workers // geo.cpr:].any(), (case.id, field, i)
        assert same_bits(member.read_rect("WALL_CUR"), walls[i])
