"""Neighbourhood ensemble probabilities and the fractions skill score on the GPU (wx_ensemble_neighbourhood): the device result equals
wx_ens_nbhd_cells on the handles' read-back arrays, bit for bit -- every count, sum, total and both maps --, and with it the numpy
definition `reference` of tests/test_ensemble_neighbourhood_cpu.py: the planted cells, every scale, wrap on and off, whole and interior
rectangles, the seams of the windows kernel's tiles, the later trips of both kernels' persistent loops, more than 64 members, radius 0
against wx_ensemble_statistics, every way of holding the truth; the call changes nothing, is timed under both kernel names, and gives
the same bits in the tolerance build and on stepped states. Every comparison is `==` on bits (NaNs compared as positions)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_ensemble_gpu import FIELDS, same_bits, same_diag
from test_ensemble_neighbourhood_cpu import (ALL, COUNTS, GX, GY, INTERIOR, MAPS, P_SEAM, P_WALL_ALL, SCALES, TOTALS, caps, check, fss_of, members_of,
                                             reference)

pytestmark = pytest.mark.gpu

CH, THR = 1, 0.5


def uploaded(pkg, f, w, tf=None, tw=None, extra=0):
    """An ensemble whose members hold f[i] as BASE and as WATER and w[i] as walls; behind them the truth (if given) and `extra`
    members that are never uploaded. Nothing is stepped."""
    sims = list(zip(f, w)) + ([(tf, tw)] if tf is not None else [])
    Y, X = f[0].shape[:2]
    ens = pkg.engine.Ensemble(len(sims) + extra, X, Y, 0)
    for i, (fi, wi) in enumerate(sims):
        ens[i].upload(fi, fi, wi)
    return ens


def read_back(ens, n, field="WATER_CUR"):
    return [ens[i].read_rect(field) for i in range(n)], [ens[i].read_rect("WALL_CUR") for i in range(n)]


def host(pkg, f, w, X, Y, scales, tf=None, tw=None, field="WATER_CUR", **kw):
    return pkg.engine.ens_nbhd_cells(f, w, X, Y, field, CH, THR, scales, tf, tw, **kw)


@pytest.mark.parametrize("B", [5, 9], ids=["5", "9-a-load-group-and-one"])
def test_device_equals_host_function(pkg, B):
    """70 x 40, the scales and planted cells of the CPU test, wrap on and off, the whole grid and the interior rectangle, both fields,
    both directions of the event; the read-back arrays are the uploaded ones, so the numpy definition is compared as well."""
    assert B % caps()["UNROLL"] == B % 8
    f, w, tf, tw = members_of(B, GX, GY, CH, THR, seed=3, extra=[(20, 40)])
    ens = uploaded(pkg, f, w, tf, tw)
    try:
        for field in ("WATER_CUR", "BASE_CUR"):
            rf, rw = read_back(ens, B + 1, field)
            assert all(same_bits(a, b) for a, b in zip(rf, f + [tf])) and all(same_bits(a, b) for a, b in zip(rw, w + [tw]))
            for wrap in (False, True):
                for rect in (None, INTERIOR):
                    got = ens.neighbourhood(field, CH, THR, SCALES, ens[B], members=range(B), rect=rect, wrap_x=wrap, want=MAPS)
                    want = host(pkg, rf[:B], rw[:B], GX, GY, SCALES, rf[B], rw[B], field=field, rect=rect, wrap_x=wrap)
                    check(got, want, (field, wrap, rect))
                    if field == "WATER_CUR":
                        check(got, reference(f, w, CH, THR, SCALES, tf, tw, rect=rect, wrap_x=wrap), (field, wrap, rect, "definition"))
                    assert (got["n_scored"] > 0).all() and got["n_unscored"][0] >= 2 and np.isnan(got["nep"][0][P_WALL_ALL if rect is None else (0, 0)]) == (rect is None)
        below = ens.neighbourhood("WATER_CUR", CH, THR, SCALES, ens[B], members=range(B), above=False, wrap_x=True, want=MAPS)
        check(below, host(pkg, f, w, GX, GY, SCALES, tf, tw, above=False, wrap_x=True), "below")
        nothing = ens.neighbourhood("WATER_CUR", CH, float("nan"), SCALES[:2], ens[B], members=range(B), want=MAPS)
        check(nothing, pkg.engine.ens_nbhd_cells(f, w, GX, GY, "WATER_CUR", CH, float("nan"), SCALES[:2], tf, tw), "a NaN threshold")
        assert nothing["ev_f"] == 0 == nothing["ev_o"] and nothing["n_f"] > 0
        # without the maps: the same scalars and no map in the answer; a channel of its own
        some = ens.neighbourhood("WATER_CUR", CH, THR, SCALES, ens[B], members=range(B), want=())
        assert set(some) == set(ALL) - set(MAPS)
        check(some, host(pkg, f, w, GX, GY, SCALES, tf, tw, want=()), "scalars only")
        for ch in (0, 3):
            check(ens.neighbourhood("WATER_CUR", ch, THR, [(2, 1)], ens[B], members=range(B), want=MAPS),
                  pkg.engine.ens_nbhd_cells(f, w, GX, GY, "WATER_CUR", ch, THR, [(2, 1)], tf, tw), ("channel", ch))
        # masks: members=None leaves the truth out; a boolean mask; one member
        check(ens.neighbourhood("WATER_CUR", CH, THR, [(1, 1)], ens[B], want=MAPS), host(pkg, f, w, GX, GY, [(1, 1)], tf, tw), "members=None")
        mask = np.arange(B + 1) % 2 == 0
        mask[B] = False
        check(ens.neighbourhood("WATER_CUR", CH, THR, [(1, 1)], ens[B], members=mask, want=MAPS), host(pkg, f, w, GX, GY, [(1, 1)], tf, tw, members=mask[:B]), "a boolean mask")
        check(ens.neighbourhood("WATER_CUR", CH, THR, [(1, 1)], ens[0], members=[2], want=MAPS), host(pkg, f, w, GX, GY, [(1, 1)], f[0], w[0], members=[2]), "one member, truth 0")
    finally:
        ens.close()


def test_tile_seams(pkg):
    """Two tiles of the windows kernel plus a ragged remainder in each direction: windows that straddle a tile seam, halos that leave
    the grid at every edge and cross the x seam, a rectangle that starts inside a tile of the grid."""
    c = caps()
    X, Y = 2 * c["TILE_W"] + 5, 2 * c["TILE_H"] + 3
    scales = [(0, 0), (3, 2), (8, 8), (16, 5), (32, 32)]
    f, w, tf, tw = members_of(3, X, Y, CH, THR, seed=5, extra=[(c["TILE_H"] - 5, c["TILE_W"] - 5), (Y - 12, X - 20)])
    ens = uploaded(pkg, f, w, tf, tw)
    try:
        for wrap in (False, True):
            for rect in (None, (3, 2, X - 4, Y - 3), (c["TILE_W"] - 1, c["TILE_H"] - 1, 2, 2)):
                got = ens.neighbourhood("WATER_CUR", CH, THR, scales, ens[3], rect=rect, wrap_x=wrap, want=MAPS)
                check(got, host(pkg, f, w, X, Y, scales, tf, tw, rect=rect, wrap_x=wrap), (wrap, rect))
        for halo in ([(8, 1)], [(1, 8)], [(9, 0)], [(0, 16)], [(17, 2)]):  # every halo class of the windows kernel, from both axes
            got = ens.neighbourhood("WATER_CUR", CH, THR, halo, ens[3], wrap_x=True, want=MAPS)
            check(got, host(pkg, f, w, X, Y, halo, tf, tw, wrap_x=True), halo)
    finally:
        ens.close()


# the tall grid: one chunk of the points kernel per row, one tile of the windows kernel per TILE_H rows
TALL_X, TALL_SCALES = 24, [(0, 0), (1, 0), (11, 2)]


def tall_grid():
    c = caps()
    return TALL_X, c["POINTS_MAX_WGS"] * c["WG"] // 64 + 16


def test_later_trips_of_both_persistent_loops(pkg):
    """The smallest grid on which the busiest wave of the points kernel and the busiest workgroup of the windows kernel take a second
    trip: planted cells in rows of the first and of the last trip of either, and with wrap_x every halo of the last trip crosses the
    x seam (the widest window is 23 of 24 columns)."""
    c = caps()
    X, Y = tall_grid()
    assert X <= 64 and Y <= 65535
    chunks, waves = ((X + 63) // 64) * Y, c["POINTS_MAX_WGS"] * c["WG"] // 64
    assert waves < chunks <= 2 * waves  # the points kernel: exactly two trips for the busiest waves
    tiles = ((X + c["TILE_W"] - 1) // c["TILE_W"]) * ((Y + c["TILE_H"] - 1) // c["TILE_H"])
    items = tiles * len(TALL_SCALES)
    assert c["WINDOWS_MAX_WGS"] < items <= 2 * c["WINDOWS_MAX_WGS"]  # the windows kernel likewise
    first_row, last_row = P_SEAM[0], Y - 12 + P_SEAM[0]  # the rows of P_SEAM in the two planted patterns
    assert first_row < waves <= last_row  # points: a planted row in the first and in the last trip
    tile_of = lambda s, row: s * tiles + row // c["TILE_H"]  # noqa: E731
    assert tile_of(0, first_row) < c["WINDOWS_MAX_WGS"] <= tile_of(len(TALL_SCALES) - 1, last_row)  # windows: likewise
    assert all(2 * rx + 1 <= X for rx, _ in TALL_SCALES) and 2 * TALL_SCALES[-1][0] + 1 >= X - 1
    f, w, tf, tw = members_of(3, X, Y, CH, THR, seed=7, extra=[(Y - 12, 0)])
    ens = uploaded(pkg, f, w, tf, tw)
    try:
        for wrap in (True, False):
            got = ens.neighbourhood("WATER_CUR", CH, THR, TALL_SCALES, ens[3], wrap_x=wrap, want=MAPS)
            want = host(pkg, f, w, X, Y, TALL_SCALES, tf, tw, wrap_x=wrap)
            check(got, want, ("tall", wrap))
            for row in (first_row, last_row):  # the planted event in column 0 is seen from the last column with wrap only
                assert (got["nep"][1, row, X - 1] > 0) == wrap and got["nep"][0, row, P_SEAM[1]] == 1.0
    finally:
        ens.close()


def test_more_than_64_members(pkg):
    B = 66
    f, w, tf, tw = members_of(B, 20, 12, CH, THR, seed=2)
    ens = uploaded(pkg, f, w, tf, tw)
    try:
        scales = [(0, 0), (2, 1), (9, 32)]
        got = ens.neighbourhood("WATER_CUR", CH, THR, scales, ens[B], wrap_x=True, want=MAPS)
        check(got, host(pkg, f, w, 20, 12, scales, tf, tw, wrap_x=True), "66 members")
        assert got["n_f"] > 64 * 20 * 12 * 0.8 and np.nanmax(got["nep"][0]) == 1.0
    finally:
        ens.close()


def test_radius_0_is_the_statistics_calls_exceedance(pkg):
    """nep at (0, 0) equals (float)((double)n_above / (double)count) of wx_ensemble_statistics for that channel, NaN where count is 0."""
    B = 5
    f, w, _, _ = members_of(B, GX, GY, CH, THR, seed=3, extra=[(20, 40)])
    ens = uploaded(pkg, f, w)
    try:
        for ch in (CH, 2):
            st = ens.statistics("WATER_CUR", threshold=(THR,) * 4, want=("count", "n_above"))
            count, above = st["count"][..., ch], st["n_above"][..., ch]
            with np.errstate(all="ignore"):
                want = np.where(count > 0, (above.astype(np.float64) / count.astype(np.float64)).astype(np.float32), np.float32(np.nan)).astype(np.float32)
            got = ens.neighbourhood("WATER_CUR", ch, THR, [(0, 0)])
            assert same_bits(got["nep"][0], want) and np.isnan(want).any() and got["n_f"] == count.sum() and got["ev_f"] == above.sum(), ch
    finally:
        ens.close()


def test_truth_handles_and_refusals(pkg):
    """A lone handle, an unselected member and a member of another ensemble give the same bits; a selected member as the truth, a
    truth of another size, a slab, a truth or a selected member never uploaded are refused with the header's codes; truth=None gives
    nep alone."""
    E = pkg.engine
    B, X, Y = 3, 20, 12
    f, w, tf, tw = members_of(B, X, Y, CH, THR)
    ens, other = uploaded(pkg, f, w, tf, tw, extra=1), uploaded(pkg, f[:1], w[:1], tf, tw)
    lone, small, never, slab = E.Handle(X, Y), E.Handle(X + 7, Y), E.Handle(X, Y), E.Handle(41, Y, X_global=57, x0=8, halo=8)
    try:
        lone.upload(tf, tf, tw)
        scales, sel = [(0, 0), (2, 1)], list(range(B))
        want = host(pkg, f, w, X, Y, scales, tf, tw, wrap_x=True)
        for name, t in (("an unselected member", ens[B]), ("a lone handle", lone), ("a member of another ensemble", other[1])):
            check(ens.neighbourhood("WATER_CUR", CH, THR, scales, t, members=sel, wrap_x=True, want=MAPS), want, name)
        alone = ens.neighbourhood("WATER_CUR", CH, THR, scales, None, members=sel, wrap_x=True)
        check(alone, host(pkg, f, w, X, Y, scales, wrap_x=True), "no truth")
        assert same_bits(alone["nep"], want["nep"]) and (alone["n_scored"] == 0).all() and alone["n_o"] == 0 and (alone["n_unscored"] == X * Y).all()

        def refused(code, *a, **kw):
            with pytest.raises(E.WxError) as ei:
                ens.neighbourhood(*a, **kw)
            assert ei.value.code == code, (a, kw, str(ei.value))
            return str(ei.value)

        two = dict(members=[0, 1])
        assert "selected" in refused(-1, "WATER_CUR", CH, THR, scales, ens[1], **two)
        assert "cells" in refused(-1, "WATER_CUR", CH, THR, scales, small, **two)
        assert "slab" in refused(-1, "WATER_CUR", CH, THR, scales, slab, **two)
        assert "obs_fraction" in refused(-1, "WATER_CUR", CH, THR, scales, None, want=MAPS, **two)
        assert "WX_FIELD_BASE_CUR" in refused(-1, "CURL", CH, THR, scales, ens[B], **two)
        assert "channel" in refused(-1, "WATER_CUR", 4, THR, scales, ens[B], **two)
        assert "n_scales" in refused(-1, "WATER_CUR", CH, THR, [], ens[B], **two) and "n_scales" in refused(-1, "WATER_CUR", CH, THR, [(1, 1)] * 9, ens[B], **two)
        assert "radius" in refused(-1, "WATER_CUR", CH, THR, [(33, 0)], ens[B], **two) and "radius" in refused(-1, "WATER_CUR", CH, THR, [(0, -1)], ens[B], **two)
        assert "threshold" in refused(-1, "WATER_CUR", CH, float("inf"), scales, ens[B], **two)
        assert "nobody" in refused(-1, "WATER_CUR", CH, THR, scales, ens[B], members=[])
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, 0, 0, 1), (X, 0, 1, 1)):
            assert "outside" in refused(-4, "WATER_CUR", CH, THR, scales, ens[B], rect=rect, **two)
        assert "wider" in refused(-4, "WATER_CUR", CH, THR, [(10, 0)], ens[B], wrap_x=True, **two)
        assert "member 4" in refused(-5, "WATER_CUR", CH, THR, scales, ens[B], members=[0, 4])
        assert "truth" in refused(-5, "WATER_CUR", CH, THR, scales, never, **two) and "truth" in refused(-5, "WATER_CUR", CH, THR, scales, ens[4], **two)
        a, r = E.WxEnsNbhd(), E.WxEnsNbhdResult()
        assert E.lib().wx_ensemble_neighbourhood(ens._e, ens[B]._h, None, None, C.byref(r)) == -1 and E.lib().wx_ensemble_neighbourhood(ens._e, ens[B]._h, C.byref(a), None, None) == -1
        # the ensemble works as before
        check(ens.neighbourhood("WATER_CUR", CH, THR, scales, ens[B], members=sel, wrap_x=True, want=MAPS), want, "after the refusals")
    finally:
        ens.close(), other.close()
        for h in (lone, small, never, slab):
            h.close()


def test_changes_nothing_and_is_profiled(pkg):
    """The members' and the truth's fields and wall bits, the iteration counters, the diagnostics and wx_ensemble_stats are equal
    before and after; wx_profile on member 0 reports one launch of each kernel per call."""
    from test_ensemble_statistics_gpu import make_ensemble, member_specs
    ens = make_ensemble(pkg, member_specs(pkg, 57, 9, 5))
    try:
        ens.step(2)

        def snapshot():
            return ([[m.read_rect(f) for f in FIELDS] for m in ens.members], ens.diagnostics(), [m.iter for m in ens.members], ens.stats())

        a = snapshot()
        ens[0].profile(True)
        for field in ("BASE_CUR", "WATER_CUR"):
            ens.neighbourhood(field, 0, 0.0, [(0, 0), (4, 2)], ens[2], wrap_x=True, want=MAPS)
            ens.neighbourhood(field, 3, 0.0, [(9, 3)], None, rect=(3, 2, 40, 5), members=[1, 3])
        prof = ens[0].profile_read()
        ens[0].profile(False)
        for k in ("ensemble_nbhd_points", "ensemble_nbhd_windows"):
            assert prof[k][1] == 4 and prof[k][0] > 0, (k, prof[k])
        b = snapshot()
        for i in range(5):
            for k, f in enumerate(FIELDS):
                assert same_bits(a[0][i][k], b[0][i][k]), (i, f)
            assert same_diag(a[1][i], b[1][i]) is None, i
        assert a[2] == b[2] and a[3] == b[3]
    finally:
        ens.close()


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_neighbourhood_gpu as T
f, w, tf, tw = T.members_of(5, T.GX, T.GY, T.CH, T.THR, seed=3, extra=[(20, 40)])
ens = T.uploaded(pkg, f, w, tf, tw)
out = {"dev_" + k: v for k, v in ens.neighbourhood("WATER_CUR", T.CH, T.THR, T.SCALES, ens[5], wrap_x=True, want=T.MAPS).items()}
out.update({"host_" + k: v for k, v in T.host(pkg, f, w, T.GX, T.GY, T.SCALES, tf, tw, wrap_x=True).items()})
ens.close()
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernels and its host function give this build's
    host function's bits, and the definition's."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    dst = str(tmp_path / "fast.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, root, dst], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(dst)
    f, w, tf, tw = members_of(5, GX, GY, CH, THR, seed=3, extra=[(20, 40)])
    want = host(pkg, f, w, GX, GY, SCALES, tf, tw, wrap_x=True)
    check(want, reference(f, w, CH, THR, SCALES, tf, tw, wrap_x=True), "exact host vs definition")
    for leg in ("dev_", "host_"):
        check({k: (int(d[leg + k]) if k in TOTALS else d[leg + k]) for k in ALL}, want, leg)


def test_weather_ensemble_on_stepped_states(pkg):
    """WeatherEnsemble.from_sim -> perturb -> step -> neighbourhood against the nature run: the input is a stepped state. The raw
    numbers are the host function's on the read-back arrays; fss, base_rate, frequency_bias and fss_useful are the one-liners of the
    docstring; fss() is the list of them; wrap_x defaults to the members' wrapHorizontally."""
    W = pkg.sim
    X, Y, B = 128, 48, 5
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    sim = W.WeatherSim(X, Y, base, water, wall, None, {"dayNightCycle": False}, sun_angle_deg=30.0)
    sim.verbose = False
    we = None
    try:
        sim.step(6)
        we = W.WeatherEnsemble.from_sim(sim, B)
        we.perturb("BASE_CUR", (0.0, 0.0, 0.0, 0.5), scale=8, seed=3)
        we.step(2)
        sim.step(2)
        f = [m.read_rect("BASE_CUR") for m in we.engine.members] + [sim.handle.read_rect("BASE_CUR")]
        w = [m.read_rect("WALL_CUR") for m in we.engine.members] + [sim.handle.read_rect("WALL_CUR")]
        air = w[B][..., 1] != 0
        thr = float(np.median(f[B][..., 3][air]))  # the truth's median temperature: an event in half of its air cells
        scales = [(0, 0), (2, 2), (8, 4), (16, 8)]
        wrap = bool(we.members[0].gui.get("wrapHorizontally", True))
        out = we.neighbourhood("BASE_CUR", 3, thr, scales, sim, want=MAPS)
        raw = pkg.engine.ens_nbhd_cells(f[:B], w[:B], X, Y, "BASE_CUR", 3, thr, scales, f[B], w[B], wrap_x=wrap)
        check({k: out[k] for k in COUNTS + TOTALS + ("sum_d2", "sum_f2", "sum_o2")}, {k: v for k, v in raw.items() if k not in MAPS}, "stepped: scalars")
        check(out["maps"], {k: raw[k] for k in MAPS}, "stepped: maps")
        check({k: v for k, v in we.engine.neighbourhood("BASE_CUR", 3, thr, scales, sim.handle, wrap_x=not wrap, want=MAPS).items()},
              pkg.engine.ens_nbhd_cells(f[:B], w[:B], X, Y, "BASE_CUR", 3, thr, scales, f[B], w[B], wrap_x=not wrap), "stepped: the other wrap")
        assert 0 < raw["ev_o"] < raw["n_o"] and 0 < raw["ev_f"] < raw["n_f"] and (raw["n_scored"] > 0).all() and (raw["sum_d2"] > 0).all()
        assert same_bits(out["fss"], fss_of(raw)) and ((out["fss"] > 0) & (out["fss"] < 1)).all()
        assert out["base_rate"] == raw["ev_o"] / raw["n_o"] and out["fss_useful"] == 0.5 + out["base_rate"] / 2
        assert out["frequency_bias"] == (raw["ev_f"] / raw["n_f"]) / (raw["ev_o"] / raw["n_o"])
        assert we.fss("BASE_CUR", 3, thr, scales, sim) == [float(v) for v in out["fss"]]
        inside = we.neighbourhood("WATER_CUR", 0, 0.0, [(1, 1)], we[4], rect=(2, 3, 20, 10))  # a member as the truth: the others are counted
        assert inside["n_f"] <= 4 * 200 and inside["n_o"] <= 200 and inside["n_scored"][0] + inside["n_unscored"][0] == 200
        assert np.isnan(we.neighbourhood("WATER_CUR", 0, float("nan"), [(1, 1)], sim)["fss"][0])  # no event anywhere: 0 / 0
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
