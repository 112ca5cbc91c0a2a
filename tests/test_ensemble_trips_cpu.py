"""The cases of tests/ensemble_trip_shapes.py without a GPU: with the caps that csrc/wx_ens_*.h state today every case makes the
busiest wave or workgroup of its kernel take a second trip through its chunk loop -- a third one where the loop carries registers or
an LDS image from trip to trip --, every kernel has a case with two chunks per row and a ragged last chunk, the planted blocks lie in
rows of the first and of the last trip, and on these very arrays each call's host function equals the numpy (assimilation: plain
Python, on rows the last trip owns) restatement of include/wxsim.h in its own test_ensemble_*_cpu.py. A cap that is raised later fails
here instead of turning tests/test_ensemble_trips_gpu.py into one-trip tests. Every comparison is `==` on bits (NaNs compared as
positions)."""
import numpy as np
import pytest

import ensemble_trip_shapes as T
import test_ensemble_assimilate_cpu as A
import test_ensemble_perturb_cpu as PT
import test_ensemble_quantiles_cpu as Q
import test_ensemble_scores_cpu as SC
import test_ensemble_statistics_cpu as ST

CAPS = T.caps()
IDS = [c.id for c in T.CASES]


def test_the_caps_are_read_from_the_headers():
    assert sorted(CAPS) == ["assim", "perturb", "quant", "score", "stat"]
    for stem, c in CAPS.items():
        assert {"WG", "MAX_WGS"} <= set(c) and c["WG"] % 64 == 0 and c["WG"] > 0 and c["MAX_WGS"] > 0, (stem, c)
    assert CAPS["quant"]["STAGED_MEMBERS"] >= 8


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_every_case_takes_a_second_trip(case):
    X, Y, B, _ = T.GRIDS[case.grid]
    x, y, w, h = case.rect
    sel = T.selection(case)
    assert 2 <= X and Y <= 65535 and 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= X and y + h <= Y  # (what wx_create accepts)
    assert sel == sorted(set(sel)) and 0 <= sel[0] and sel[-1] < B
    geo = T.geometry(case, CAPS)
    assert geo.trips >= 2, (case.id, geo)
    staged = CAPS["quant"]["STAGED_MEMBERS"]
    if case.kernel == "quant_stream":
        assert len(sel) > staged
    if case.kernel in ("quant_staged", "score"):
        assert len(sel) <= staged
    if case.call == "quantiles":
        assert case.kw["rank_of"] not in sel and case.kw["rank_of"] < B


def test_every_kernel_has_its_cases():
    assert {c.kernel for c in T.CASES} == set(T.KERNELS)
    for kernel in T.CARRIES_STATE:  # the registers and the LDS image must survive more than one hand-over
        assert max(T.geometry(c, CAPS).trips for c in T.CASES if c.kernel == kernel) >= 3, kernel
    for kernel in T.KERNELS:  # two chunks per row and a last chunk that is not full
        assert any(T.geometry(c, CAPS).cpr >= 2 and c.rect[2] % 64 != 0 for c in T.CASES if c.kernel == kernel), kernel
    assert any(len(T.selection(c)) == CAPS["quant"]["STAGED_MEMBERS"] for c in T.CASES if c.kernel == "quant_staged")  # the 64 KiB image
    assert any(len(T.selection(c)) == CAPS["quant"]["STAGED_MEMBERS"] + 1 for c in T.CASES if c.kernel == "quant_stream")
    for call in ("statistics", "assimilate", "scores"):  # a full load group of 8 and a remainder; the remainder loop alone
        assert {len(T.selection(c)) for c in T.by_call(call)} == {3, 9}, call


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_the_planted_blocks_lie_in_the_first_and_in_the_last_trip(case):
    X, Y, _, _ = T.GRIDS[case.grid]
    geo = T.geometry(case, CAPS)
    x0, y0, w, h = case.rect
    n_sel = len(T.selection(case))
    nr = T.block_rows(X)
    for name, first, last, s in T.planted_blocks(case.grid):
        cells = [divmod(s + i, X) for i in range(T.N_PLANTED)]  # (row in the block, x)
        assert all(r < nr for r, _ in cells) and first + nr <= last and last + nr <= Y - 1
        inside = [(r, x - x0) for r, x in cells if x0 <= x < x0 + w]
        assert len(inside) == T.N_PLANTED and 0 <= first - y0 and last + nr - 1 - y0 < h, (case.id, name)
        if X >= 67:
            assert {x // 64 for _, x in inside} == {0, 1}  # on both sides of a chunk boundary
        assert {T.trip_of(case, geo, first - y0 + r, x) for r, x in inside} == {0}, (case.id, name)
        assert {T.trip_of(case, geo, last - y0 + r, x, n_sel - 1, 3) for r, x in inside} == {geo.trips - 1}, (case.id, name)


@pytest.mark.parametrize("grid", sorted(T.GRIDS))
def test_the_members_hold_the_planted_cells(grid):
    X, Y, B, names = T.GRIDS[grid]
    m = T.members(grid)
    assert len(m["base"]) == len(m["water"]) == len(m["wall"]) == B and m["base"][0].shape == (Y, X, 4) and not m["base"][0].flags.writeable
    for name, first, last, s in T.planted_blocks(grid):
        f, w = T.planted_cells(name, B)
        for i in range(B):
            for row in (first, last):
                for held in (m["base"][i], m["water"][i]):
                    assert T.block_view(held, row, X, s).view(np.uint32).tobytes() == f[i].view(np.uint32).tobytes(), (grid, name, i, row)
                assert np.array_equal(T.block_view(m["wall"][i], row, X, s), w[i]), (grid, name, i, row)
    special = sum(int((~np.isfinite(a)).sum()) for a in m["base"])
    assert special > 0 and len({a.tobytes() for a in m["wall"]}) == B  # non-finite values; walls that differ per member


def cut(arrays, rect):
    x, y, w, h = rect
    return [np.ascontiguousarray(a[y:y + h, x:x + w]) for a in arrays]


def field_of(m, case):
    return m["base"] if case.kw["field"] == T.B_ else m["water"]


@pytest.mark.parametrize("case", T.by_call("statistics"), ids=[c.id for c in T.by_call("statistics")])
def test_statistics_host_function_equals_the_definition(pkg, case):
    m = T.members(case.grid)
    f, w = cut(field_of(m, case), case.rect), cut(m["wall"], case.rect)
    want = ST.reference(f, w, case.sel, ST.THRESHOLD)
    planes = ST.PLANES if case.kw["variance"] else tuple(p for p in ST.PLANES if p != "variance")
    got = pkg.engine.ens_stat_cells(f, w, members=case.sel, threshold=ST.THRESHOLD, want=planes)
    ST.check(got, {k: want[k] for k in planes}, case.id)
    assert (want["count"] == len(T.selection(case))).any() and (want["n_wall"] > 0).any() and np.isnan(want["mean"]).any()


@pytest.mark.parametrize("case", T.by_call("scores"), ids=[c.id for c in T.by_call("scores")])
def test_scores_host_function_equals_the_definition(pkg, case):
    m = T.members(case.grid)
    f, w = cut(field_of(m, case), case.rect), cut(m["wall"], case.rect)
    sel = T.selection(case)
    want = SC.reference(f[:-1], w[:-1], f[-1], w[-1], sel)
    got = pkg.engine.ens_score_cells(f[:-1], w[:-1], f[-1], w[-1], members=sel, want=SC.MAPS if case.kw["maps"] else ())
    SC.check(got, want if case.kw["maps"] else SC.scalars(want), case.id)
    assert (want["n_scored"] > 0).all() and (want["n_truth_excluded"] > 0).all() and (want["n_empty"] > 0).all() and want["n_overflow"].sum() > 0


@pytest.mark.parametrize("case", T.by_call("quantiles"), ids=[c.id for c in T.by_call("quantiles")])
def test_quantiles_host_function_equals_the_definition(pkg, case):
    m = T.members(case.grid)
    f, w = cut(field_of(m, case), case.rect), cut(m["wall"], case.rect)
    want = Q.reference(f, w, case.sel, Q.P8, case.kw["interp"], case.kw["rank_of"])
    got = pkg.engine.ens_quant_cells(f, w, Q.P8, members=case.sel, interp=case.kw["interp"], rank_of=case.kw["rank_of"])
    Q.check(got, want, case.id)
    assert (want["n_below"] == -1).any() and (want["n_equal"] > 1).any() and (want["count"] == 0).any()


@pytest.mark.parametrize("case", T.by_call("perturb"), ids=[c.id for c in T.by_call("perturb")])
def test_perturb_host_function_equals_the_definition(pkg, case):
    X, Y, B, _ = T.GRIDS[case.grid]
    m = T.members(case.grid)
    kw = dict(case.kw)
    field, mode = kw.pop("field"), kw.pop("mode")
    f = field_of(m, case)
    got = pkg.engine.ens_perturb_cells(f, m["wall"], X, Y, field, T.PERTURB_AMP[field], mode=mode, members=case.sel, **kw)
    want = PT.reference(f, m["wall"], X, Y, amplitude=T.PERTURB_AMP[field], mode=("add", "mul").index(mode), members=case.sel, **kw)
    PT.check(got, want, case.id)
    sel = T.selection(case)
    assert all(ST.same_bits(got[i], f[i]) != (i in sel) for i in range(B))


def last_trip_rows(case, n=3):
    """A sub-rectangle of whole rows that the last trip owns and that holds the planted blocks of the last trip."""
    X, Y, _, _ = T.GRIDS[case.grid]
    geo = T.geometry(case, CAPS)
    rect = (0, Y - 1 - n, X, n)
    assert all(T.trip_of(case, geo, y, x) == geo.trips - 1 for y in range(rect[1], rect[1] + n) for x in (0, X - 1))
    assert all(rect[1] <= last < rect[1] + n for _, _, last, _ in T.planted_blocks(case.grid))
    return rect


@pytest.mark.parametrize("case", T.by_call("assimilate"), ids=[c.id for c in T.by_call("assimilate")])
def test_assimilate_host_function_equals_the_definition_on_rows_of_the_last_trip(pkg, case):
    X, Y, B, _ = T.GRIDS[case.grid]
    m = T.members(case.grid)
    obs = T.observations()
    rect = last_trip_rows(case)
    gb, gw, res = A.check(pkg, m["base"], m["water"], m["wall"], X, Y, obs, case.id, rect=rect, members=case.sel, **case.kw)
    assert all(r["applied"] for r in res)
    sel = T.selection(case)
    moved = [not (ST.same_bits(gb[i], m["base"][i]) and ST.same_bits(gw[i], m["water"][i])) for i in range(B)]
    assert moved == [i in sel for i in range(B)]
    inside = np.zeros((Y, X), bool)
    inside[rect[1]:rect[1] + rect[3]] = True
    assert not any(A.changed(gb[i], m["base"][i])[~inside].any() for i in sel)


def test_the_observations_straddle_the_trips():
    case = T.by_call("assimilate")[0]
    geo = T.geometry(case, CAPS)
    obs = T.observations()
    trips = [T.trip_of(case, geo, o[2], o[1]) for o in obs]
    assert len(obs) == 8 and {o[0] for o in obs} == {T.B_, T.W_} and trips.count(0) >= 3 and trips.count(geo.trips - 1) >= 3
    rows = sorted(o[2] for o in obs)
    edge = [y for y in rows if T.trip_of(case, geo, y, 0) != T.trip_of(case, geo, y - 1, 0)]
    assert len(edge) == 1 and edge[0] - 1 in rows  # the boundary row between two trips, and the row in front of it
    m = T.members("state")
    blocks = [r for _, first, last, _ in T.planted_blocks("state") for r in (first, last)]
    for o in obs:
        assert all(w[o[2], o[1], 1] != 0 for w in m["wall"]) and o[2] not in blocks
