"""wx_ensemble_covariance on the GPU: every plane and every result of the device equals wx_ens_cov_cells -- the definition on the CPU,
which tests/test_ensemble_covariance_cpu.py pins to the text of include/wxsim.h -- bit for bit over whole rectangles: uploaded random
members with the planted cells of the CPU test in them, every template bucket of the predictor count, both sources, both fields, masks,
rectangles that start off a multiple of 64 and are 1, 64 and 65 cells wide; the snapshot source behind a step; every refusal of the device call; the chunk loop's second
trip; that the call changes nothing; the pre-pass against wx_ensemble_assimilate's priors; the tolerance build; the profile; and
WeatherEnsemble.sensitivity end to end. Every comparison is `==` on bits (NaNs compared as positions); a failure names predictor,
cell and channel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_ensemble_covariance_cpu as CC
from test_ensemble_covariance_cpu import B_, FLT_MAX, INF, NAN, PLANES, PLANTED, PLANTED_IDS, SEPARATORS, W_, compare, cov_members, f64_bits
from test_ensemble_gpu import same_bits
from test_ensemble_perturb_gpu import pre_values
from test_ensemble_statistics_gpu import make_ensemble, member_specs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def upload_ensemble(pkg, bases, waters, walls):
    """An ensemble whose members hold exactly these arrays (uploaded, not stepped)."""
    E, P = pkg.engine, pkg.params
    Yg, Xg = bases[0].shape[:2]
    u = P.uniforms_from_gui(P.merge_settings(None), Yg)
    ens = E.Ensemble(len(bases), Xg, Yg, 0)
    for m, b, w, wl in zip(ens.members, bases, waters, walls):
        m.upload(b, w, wl)
        m.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
    return ens


def grid_members(B, X, Y, seed=31):
    """Random members (a wall or a non-finite value in one member in one cell of twenty-five) with planted cells of the CPU test in
    them: NaN, +-Inf, FLT_MAX and -0.0 in one member -- once inside the first load group, once in the last member --, a wall in one
    member, equal members. All in rows 1 .. 4, on both sides of the chunk boundary at x = 64."""
    bases, waters, wl = cov_members(B, X, Y, seed=seed, keep=[(2, 1), (X - 1, Y - 1), (0, 0), (5, 2), (X - 2, 3)])
    for member, x0 in ((min(3, B - 1), 6), (B - 1, 61)):
        for f in (bases[member], waters[member]):
            f[3, x0, 0], f[3, x0 + 1, 1], f[3, x0 + 2, 2], f[3, x0 + 3, 3], f[3, x0 + 4, 0] = NAN, INF, -INF, FLT_MAX, -0.0
        wl[member][2, x0 + 1, 1] = 0
    for b, w in zip(bases, waters):
        b[4, 10:14, 3] = bases[0][4, 10:14, 3]
        w[1, 62:67, 0] = waters[0][1, 62:67, 0]
    return bases, waters, wl


def device_equals_host(pkg, ens, bases, waters, walls, field, preds, where, priors=None, **kw):
    Yg, Xg = walls[0].shape[:2]
    got = ens.covariance(field, preds, **kw)
    want = pkg.engine.ens_cov_cells(bases, waters, walls, Xg, Yg, field, preds, priors=priors, **kw)
    compare(got, want, where)
    return got


def predictor_sets(B, X, Y, rng):
    """1, 2, 3 and 8 predictors: every template bucket, and a count inside a bucket; points of both fields, VALUES of several scales."""
    sets, _ = CC.predictor_sets(B, X, Y, rng)
    return [sets[0], [sets[3][1], sets[3][2]], sets[2], sets[3], sets[1]]


@pytest.mark.parametrize("X,Y,B,members", [(70, 9, 2, None), (70, 9, 3, None), (130, 5, 5, [0, 2, 4]), (130, 5, 8, None), (70, 9, 11, [0, 1, 2, 4, 5, 7, 9, 10]),
                                           (130, 5, 9, None), (70, 9, 17, None), (130, 5, 19, [i for i in range(19) if i not in (3, 11)])])
def test_device_equals_host_function(pkg, X, Y, B, members):
    n = B if members is None else len(members)
    assert n in (2, 3, 8, 9, 17)  # a partial load group, a group of 8, 8 + 1, two groups + 1
    rng = np.random.Generator(np.random.Philox(100 + B))
    sets = predictor_sets(B, X, Y, rng)
    if members is not None:  # an unselected member's number is not looked at
        sets = [[p if CC.is_point(p) else np.where(np.isin(np.arange(B), members), p, NAN) for p in s] for s in sets]
    bases, waters, wl = grid_members(B, X, Y)
    rects = [None, (3, 1, 64, Y - 2), (65, 0, 1, Y), (5, 2, 65, 2), (X - 64, 1, 64, 3), (1, Y - 1, X - 1, 1)]
    ens = upload_ensemble(pkg, bases, waters, wl)
    try:
        eligible = valid = 0
        for i, preds in enumerate(sets):  # every bucket, both fields, the whole grid
            for field in (B_, W_):
                got = device_equals_host(pkg, ens, bases, waters, wl, field, preds, (X, Y, B, "set", i, field), members=members)
                eligible += int(np.isfinite(got["variance"]).sum())
                valid += sum(r["valid"] for r in got["results"])
                assert np.isnan(got["variance"]).any() and np.isfinite(got["corr"]).any()
        for i, rect in enumerate(rects):  # points inside and outside the rectangle, and in the other field
            for k in range(2):
                field, preds = (B_, W_)[(i + k) % 2], sets[(i + 2 * k) % len(sets)]
                want = PLANES if (i + k) % 3 else ("corr", "variance")
                device_equals_host(pkg, ens, bases, waters, wl, field, preds, (X, Y, B, "rect", rect, field), rect=rect, members=members, want=want)
        assert eligible > 0.8 * 2 * len(sets) * X * Y * 4 and valid == 2 * sum(len(s) for s in sets)
        for m, b, w in zip(ens.members, bases, waters):  # nothing was written
            assert same_bits(m.read_rect(B_), b) and same_bits(m.read_rect(W_), w)
    finally:
        ens.close()


def device_run(pkg):
    """`run` of the planted cases of tests/test_ensemble_covariance_cpu.py on the device: the arrays are uploaded (nothing is stepped),
    the call is made, and its planes and results equal the host function's bit for bit; the device's answer goes back to the case's
    value-level assertions."""
    def run(bases, waters, walls, X, Y, field, predictors, where, **kw):
        ens = upload_ensemble(pkg, bases, waters, walls)
        try:
            assert all(same_bits(m.read_rect(B_), b) for m, b in zip(ens.members, bases)), where  # the planted bits are on the device
            return device_equals_host(pkg, ens, bases, waters, walls, field, predictors, where, **kw)
        finally:
            ens.close()

    return run


@pytest.mark.parametrize("B", [5, 9])
@pytest.mark.parametrize("case,placements", PLANTED, ids=PLANTED_IDS)
def test_planted_cases_through_the_kernels(pkg, case, placements, B):
    for kw in placements if B == 9 else placements[:1]:
        case(device_run(pkg), B=B, **kw)


def cut(a, rect):
    x, y, w, h = rect
    return np.ascontiguousarray(a[y:y + h, x:x + w])


@pytest.mark.parametrize("members", [None, [0, 1, 2, 3, 5, 6, 7, 8]])
def test_source_prior_behind_a_step(pkg, members):
    """70 x 9, nine members on different terrain: save_prior of both fields, a few iterations, then the covariance of the SNAPSHOT with
    per-member numbers and with points of the CURRENT state; the host function gets the snapshot as read before the step. A rectangle
    strictly inside the snapshot's; the three WX_E_STATE refusals of the snapshot."""
    X, Y, B = 70, 9, 9
    E = pkg.engine
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, B))
    try:
        ens.step(2)
        rng = np.random.Generator(np.random.Philox(7))
        vals = [np.where(np.isin(np.arange(B), range(B) if members is None else members), rng.normal(0, 2, B), NAN), np.arange(B) * 0.5]

        def refused(**kw):
            with pytest.raises(E.WxError) as ei:
                ens.covariance(kw.pop("field", B_), [vals[1]], source="prior", **kw)
            assert ei.value.code == CC.E_STATE, str(ei.value)
            return str(ei.value)

        assert "no snapshot" in refused()
        prior = pre_values(pkg, ens)
        snap = (2, 1, 66, 7)
        ens.save_prior(B_, snap, members), ens.save_prior(W_, snap, members)
        ens.drop_prior(W_)
        assert "no snapshot" in refused(field=W_, rect=snap, members=members)  # one slot per field
        ens.save_prior(W_, snap, members)
        ens.step(3)
        cur = pre_values(pkg, ens)
        assert not same_bits(cur[0][B_], prior[0][B_])
        air = np.all([c["WALL_CUR"][..., 1] != 0 for c in cur], axis=0)
        ys, xs = np.nonzero(air)
        pts = [(B_, int(xs[0]), int(ys[0]), 3), (W_, int(xs[-1]), int(ys[-1]), 0), (B_, int(xs[len(xs) // 2]), int(ys[len(xs) // 2]), 0)]
        bases, waters, wl = [c[B_] for c in cur], [c[W_] for c in cur], [c["WALL_CUR"] for c in cur]
        for field in (B_, W_):
            for rect in (snap, (5, 2, 60, 4)):
                priors = [cut(p[field], rect) for p in prior]
                for preds in ([vals[0]], [pts[0], vals[0], pts[1]], [vals[0], pts[0], pts[1], vals[1], pts[2]]):
                    got = device_equals_host(pkg, ens, bases, waters, wl, field, preds, (field, rect, len(preds)), priors=priors, source="prior", rect=rect,
                                             members=members)
                    assert np.isfinite(got["slope"]).any() and all(r["valid"] for r in got["results"])
                # ... and it is the snapshot that was read, not the current field
                now = ens.covariance(field, [vals[0]], rect=rect, members=members, want=("variance",))["variance"]
                then = ens.covariance(field, [vals[0]], source="prior", rect=rect, members=members, want=("variance",))["variance"]
                assert not same_bits(now, then)
        for rect in (None, (1, 1, 4, 4), (2, 0, 4, 4), (65, 1, 4, 4), (2, 5, 4, 4)):
            assert "not inside" in refused(rect=rect, members=members), rect
        other = [0, 1] if members is None else None
        assert "selection" in refused(rect=snap, members=other)
        assert "selection" in refused(rect=snap, members=[0, 1, 2, 3, 5, 6, 7])
        for i, m in enumerate(ens.members):
            assert same_bits(m.read_rect(B_), cur[i][B_]) and same_bits(m.read_rect(W_), cur[i][W_])
    finally:
        ens.close()


def test_every_refusal_of_the_device_call(pkg):
    """wx_ensemble_covariance's own argument checks (the CPU file refuses through wx_ens_cov_cells): each refusal of include/wxsim.h
    with its code, the never-uploaded member named, the values of an unselected member not looked at; the refused calls write nothing
    and the accepted calls next to them give the host function's bits."""
    E = pkg.engine
    X, Y = 70, 40
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 4)[:3] + [None])  # member 3 is never uploaded
    sel = [0, 1, 2]
    try:
        keep = [ens[i].read_rect(f) for i in sel for f in (B_, W_, "WALL_CUR")]
        ys, xs = np.nonzero(np.all([w[..., 1] != 0 for w in keep[2::3]], axis=0))
        pt = (B_, int(xs[len(xs) // 2]), int(ys[len(ys) // 2]), 3)  # an air cell in all three

        def refused(code, field=B_, preds=(pt,), **kw):
            with pytest.raises(E.WxError) as ei:
                ens.covariance(field, list(preds), **{"members": sel, **kw})
            assert ei.value.code == code, (field, preds, kw, str(ei.value))
            return str(ei.value)

        def raw(code, n_pred=1, **over):
            """The C call with one member of the descriptor or of predictor 0 set to a value the Python layer would not pass."""
            preds, hold = E._cov_predictors([over.pop("pred", pt)], 4)
            c, planes = E._cov_struct(B_, "current", (0, 0, X, Y), n_pred, ("corr",))
            for k, v in over.items():  # kind, channel, values, pfield (the point's field): predictor 0; the rest: the descriptor
                if k in ("kind", "channel", "values", "pfield"):
                    setattr(preds[0], "field" if k == "pfield" else k, v)
                else:
                    setattr(c, k, v)
            mask = np.array([1, 1, 1, 0], np.uint8)
            assert E.lib().wx_ensemble_covariance(ens._e, C.byref(c), preds, None, mask.ctypes.data) == code, over
            assert (planes["corr"] == 0).all()  # (as allocated: nothing was written)

        # WX_E_INVALID
        L = E.lib()
        c0, _ = E._cov_struct(B_, "current", (0, 0, X, Y), 1, ())
        p0, _ = E._cov_predictors([pt], 4)
        assert L.wx_ensemble_covariance(None, C.byref(c0), p0, None, None) == CC.E_INVALID
        assert L.wx_ensemble_covariance(ens._e, None, p0, None, None) == CC.E_INVALID and L.wx_ensemble_covariance(ens._e, C.byref(c0), None, None, None) == CC.E_INVALID
        for f in ("CURL", "BASE_DISP", "WATER_0", "WALL_CUR"):
            refused(CC.E_INVALID, field=f)
            raw(CC.E_INVALID, pfield=E.FIELD_IDS[f])
        raw(CC.E_INVALID, source=2), raw(CC.E_INVALID, source=-1), raw(CC.E_INVALID, kind=2), raw(CC.E_INVALID, kind=-1)
        raw(CC.E_INVALID, channel=4), raw(CC.E_INVALID, channel=-1)
        raw(CC.E_INVALID, n_pred=0), raw(CC.E_INVALID, n_pred=9), raw(CC.E_INVALID, n_pred=-1)
        refused(CC.E_INVALID, preds=[]), refused(CC.E_INVALID, preds=[pt] * 9)
        raw(CC.E_INVALID, pred=np.zeros(4), values=None)
        for v in (NAN, INF, -INF, 3.5e38, -3.5e38):
            for i in sel:
                vals = np.array([1.0, 2.0, 4.0, 8.0])
                vals[i] = v
                refused(CC.E_INVALID, preds=[vals])
                refused(CC.E_INVALID, preds=[pt, vals], source="current")
        refused(CC.E_INVALID, members=[1]), refused(CC.E_INVALID, members=[]), refused(CC.E_INVALID, members=[3])
        # WX_E_RANGE
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (X, 0, 1, 1)):
            refused(CC.E_RANGE, rect=rect)
        for x, y in ((-1, 5), (5, -1), (X, 5), (5, Y)):
            refused(CC.E_RANGE, preds=[(B_, x, y, 0)]), refused(CC.E_RANGE, preds=[np.arange(4.0), (W_, x, y, 1)])
        # WX_E_STATE: a member that was never uploaded, named
        assert "member 3" in refused(CC.E_STATE, members=None) and "member 3" in refused(CC.E_STATE, members=[1, 3])
        assert "member 3" in refused(CC.E_STATE, members=[0, 1, 2, 3], preds=[np.arange(4.0)])
        assert "no snapshot" in refused(CC.E_STATE, source="prior")
        now = [ens[i].read_rect(f) for i in sel for f in (B_, W_, "WALL_CUR")]
        assert all(same_bits(a, b) for a, b in zip(now, keep))  # a refused call writes nothing
        # what is accepted: the same values in an UNSELECTED member, FLT_MAX itself, two members
        bases, waters, wl = keep[0::3], keep[1::3], keep[2::3]
        for v in (NAN, INF, 3.5e38):
            vals = np.array([1.0, 2.0, 4.0, v])
            device_equals_host(pkg, ens, bases + [None], waters + [None], wl + [None], B_, [vals, pt], ("unselected", v), members=sel)
        vals = np.array([float(FLT_MAX), -float(FLT_MAX), 0.0, NAN])
        device_equals_host(pkg, ens, bases + [None], waters + [None], wl + [None], W_, [vals], "FLT_MAX", members=sel)
        got = device_equals_host(pkg, ens, bases + [None], waters + [None], wl + [None], B_, [pt], "two members", members=[0, 2])
        assert np.isfinite(got["corr"]).any()
        ens.sync()  # (no step: member 3 was never uploaded)
    finally:
        ens.close()


def test_chunk_loop_second_trip(pkg):
    """2 columns and just over MAX_WGS * WG / 64 rows, three members: one chunk per row, more rows than the capped grid has waves, so the
    busiest waves take a second trip (tests/test_ensemble_covariance_cpu.py computes that from the header). Planted cells in a row of
    the first and of the last trip; a point predictor in each."""
    X, Y = CC.tall_grid()
    first, last = CC.tall_planted_rows()
    rng = np.random.Generator(np.random.Philox(5))
    mk = lambda: (rng.normal(0, 1, (Y, X, 4)) * np.array([0.1, 0.1, 0.01, 2.0]) + np.array([0, 0, 0, 300.0])).astype(np.float32)  # noqa: E731
    bases, waters = [mk() for _ in range(3)], [np.abs(mk()) for _ in range(3)]
    wl = [np.full((Y, X, 4), 3, np.int8) for _ in range(3)]
    for row in (first, last):
        bases[1][row, 0, 0], bases[2][row, 1, 3], bases[0][row + 1, 0, 1] = NAN, FLT_MAX, -INF
        wl[2][row + 1, 1, 1] = 0
        for b in bases:
            b[row - 1, 1, 2] = np.float32(0.25)
    preds = [(B_, 1, first - 2, 3), np.array([0.5, -1.0, 2.0]), (W_, 0, last - 2, 0)]
    ens = upload_ensemble(pkg, bases, waters, wl)
    try:
        for field in (B_, W_):
            got = device_equals_host(pkg, ens, bases, waters, wl, field, preds, ("tall", field))
            assert all(r["valid"] for r in got["results"])
            for row in (first, last):
                assert np.isfinite(got["variance"][row - 2]).all() and np.isnan(got["variance"][row + 1, 1]).all()
                assert (field == B_) == bool(np.isnan(got["variance"][row, 0, 0])) and (field == B_) == bool(got["variance"][row - 1, 1, 2] == 0)
        ens.save_prior(B_)
        device_equals_host(pkg, ens, bases, waters, wl, B_, preds[:2], "tall, prior", priors=bases, source="prior")
    finally:
        ens.close()


SIDE_FIELDS = ("BASE_CUR", "WATER_CUR", "WALL_CUR", "WATER_0", "BASE_DISP", "CURL", "WALL_DISP", "LIGHT_0", "LIGHT_1")


def test_the_call_changes_nothing(pkg):
    """Directly behind a step whose display side is pending: every readable field of two members, the iteration counters and
    wx_ensemble_stats equal those of a twin ensemble that never made the call, and so does a following step."""
    X, Y = 70, 40
    specs = member_specs(pkg, X, Y, 3)
    ens, twin = make_ensemble(pkg, specs), make_ensemble(pkg, specs)
    try:
        ens.step(4), twin.step(4)
        ens.save_prior(B_), twin.save_prior(B_)
        ens.step(3), twin.step(3)
        stats, iters = ens.stats(), [m.iter for m in ens.members]
        for field, source in ((B_, "current"), (W_, "current"), (B_, "prior")):  # (directly behind the step)
            got = ens.covariance(field, [(B_, 30, 20, 3), np.array([1.0, 2.0, 4.0]), (W_, 11, 30, 0)], source=source)
            assert np.isfinite(got["cov"]).any()
        assert ens.stats() == stats == twin.stats() and [m.iter for m in ens.members] == iters == [m.iter for m in twin.members]
        for i in (0, 2):
            for f in SIDE_FIELDS:
                assert same_bits(ens[i].read_rect(f), twin[i].read_rect(f)), (i, f)
        ens.covariance(B_, [(B_, 30, 20, 3)], members=[0, 2])
        ens.step(3), twin.step(3)
        assert ens.stats() == twin.stats()
        for i in range(3):
            for f in SIDE_FIELDS:
                assert same_bits(ens[i].read_rect(f), twin[i].read_rect(f)), ("after the step", i, f)
    finally:
        ens.close(), twin.close()


def test_the_prepass_gives_the_assimilation_priors(pkg):
    """result.mean / .variance of point predictors on the device have the bits of wx_ensemble_assimilate's prior_mean / prior_var (all
    gains 0: nothing is updated) for the same points on the device."""
    X, Y, B = 70, 9, 9
    bases, waters, wl = grid_members(B, X, Y)
    pts = [(B_, 2, 1, 3), (W_, X - 1, Y - 1, 0), (B_, 0, 0, 0), (W_, 5, 2, 3), (B_, 6, 3, 0), (B_, 7, 2, 1), (W_, 63, 1, 0), (B_, 61, 3, 0)]
    ens = upload_ensemble(pkg, bases, waters, wl)
    try:
        for members in (None, [0, 3, 8], [1, 2, 4, 5, 6, 7, 8]):
            got = ens.covariance(W_, pts, members=members, want=("cov",))["results"]
            res = ens.assimilate([p + (1.0, 1.0) for p in pts], members=members, gain_base=0.0, gain_water=0.0)
            assert sum(r["applied"] for r in res) >= 3 and not all(r["applied"] for r in res)  # (the last point is NaN in the last member)
            for j, (a, b) in enumerate(zip(got, res)):
                assert a["valid"] == b["applied"] and f64_bits(a["mean"]) == f64_bits(b["prior_mean"]) and f64_bits(a["variance"]) == f64_bits(b["prior_var"]), (j, a, b)
        assert all(same_bits(m.read_rect(B_), b) for m, b in zip(ens.members, bases))
    finally:
        ens.close()


def run_separators(pkg):
    """Every separator through both kernels; returns the (variance, cov, slope, corr) bits of its cell."""
    out = []
    for i in range(len(SEPARATORS)):
        bases, waters, wl, point, cell = CC.separator_arrays(i)
        ens = upload_ensemble(pkg, bases, waters, wl)
        try:
            out.append(CC.separator_bits(ens.covariance(B_, [point]), cell))
        finally:
            ens.close()
    return out


def check_separators(bits):
    for i, (_, _, _, defined, fused) in enumerate(SEPARATORS):
        assert tuple(int(v) for v in bits[i]) == defined != fused, (i, bits[i], defined, fused)


def test_planted_separators_on_the_device(pkg):
    """Member values on which a fused d_k*e_k or d_k*d_k changes a float32 result: the device gives the defined bits."""
    check_separators(run_separators(pkg))


FAST_SHAPE = (70, 9, 11)
FAST_MEMBERS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_covariance_gpu as G
X, Y, B = G.FAST_SHAPE
bases, waters, wl = G.grid_members(B, X, Y)
sets = G.predictor_sets(B, X, Y, np.random.Generator(np.random.Philox(9)))
ens = G.upload_ensemble(pkg, bases, waters, wl)
out = {}
for i, preds in enumerate(sets):
    got = ens.covariance((G.B_, G.W_)[i % 2], preds, members=G.FAST_MEMBERS)
    for k in G.PLANES:
        out["%s%d" % (k, i)] = got[k]
    out["res%d" % i] = np.array([[r["valid"], r["mean"], r["variance"]] for r in got["results"]], np.float64)
ens.close()
out["sep"] = np.array(G.run_separators(pkg), np.int64)
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernels give what THIS process's host function gives
    on the same uploaded members -- every template bucket, ten selected members (a load group of 8 and a remainder) --, then the planted
    separators."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    path = str(tmp_path / "fast.npz")
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, ROOT, path], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(path)
    X, Y, B = FAST_SHAPE
    bases, waters, wl = grid_members(B, X, Y)
    sets = predictor_sets(B, X, Y, np.random.Generator(np.random.Philox(9)))
    for i, preds in enumerate(sets):
        want = pkg.engine.ens_cov_cells(bases, waters, wl, X, Y, (B_, W_)[i % 2], preds, members=FAST_MEMBERS)
        got = {k: d["%s%d" % (k, i)] for k in PLANES}
        got["results"] = [dict(valid=bool(r[0]), mean=float(r[1]), variance=float(r[2])) for r in d["res%d" % i]]
        compare(got, want, ("fast", i))
    check_separators(d["sep"])


def test_the_profile_names_both_kernels(pkg):
    ens = make_ensemble(pkg, member_specs(pkg, 70, 40, 3))
    try:
        ens.save_prior(B_, None, [1, 2])
        for source, preds in (("current", [(B_, 30, 20, 3)]), ("prior", [np.array([0.0, 1.0, 3.0])] * 3), ("current", [(W_, 3, 30, 0)] * 8)):
            ens[0].profile(True)
            ens.covariance(B_, preds, source=source, members=[1, 2])  # (member 0 times the launches, whoever is selected)
            prof = ens[0].profile_read()
            assert prof["ensemble_covariance_pred"][1] == 1 and prof["ensemble_covariance"][1] == 1, (source, prof)
            assert prof["ensemble_covariance_pred"][0] > 0 and prof["ensemble_covariance"][0] > 0 and "ensemble_statistics" not in prof
    finally:
        ens.close()


def test_sensitivity_end_to_end(pkg):
    """WeatherEnsemble.sensitivity on 100 x 100 x 8: one spun-up state cloned, temperature perturbed, save_prior, 20 iterations, the
    metric each member's total water vapour (sum_water[0] of wx_ensemble_diagnostics): slope and corr equal the host function on the
    read_rect data of the prior; correlation() is the corr plane of a point predictor."""
    W, E = pkg.sim, pkg.engine
    Xw, Yw, Bw = 100, 100, 8
    base, water, wall = pkg.synth.terrain_grid(Xw, Yw)
    sim = W.WeatherSim(Xw, Yw, base, water, wall, None, {"dayNightCycle": False}, sun_angle_deg=30.0)
    sim.verbose = False
    we = None
    try:
        sim.step(6)
        we = W.WeatherEnsemble.from_sim(sim, Bw)
        with pytest.raises(E.WxError) as ei:
            we.sensitivity(np.arange(Bw), B_)
        assert ei.value.code == CC.E_STATE and "no snapshot" in str(ei.value)
        we.perturb(B_, (0.0, 0.0, 0.0, 0.5), scale=8, seed=3)
        we.save_prior(B_)
        prior = [m.read_rect(B_) for m in we.members]
        walls = [m.read_rect("WALL_CUR") for m in we.members]
        we.step(20)
        metric = lambda diags: [d["sum_water"][0] for d in diags]  # noqa: E731
        J = metric(we.diagnostics())
        assert len(set(J)) == Bw
        got = we.sensitivity(metric, B_)
        want = E.ens_cov_cells(None, None, walls, Xw, Yw, B_, [np.array(J)], source="prior", priors=prior, want=("slope", "corr"))
        compare({"slope": got["slope"][None], "corr": got["corr"][None], "results": [got["result"]]}, want, "sensitivity")
        assert np.isfinite(got["slope"][..., 3]).sum() > Xw * Yw // 2 and np.nanmax(np.abs(got["corr"][..., 3])) > 0.5
        rect = (10, 20, 65, 30)
        part = we.sensitivity(J, B_, rect=rect)
        assert same_bits(part["slope"], cut(got["slope"], rect)) and same_bits(part["corr"], cut(got["corr"], rect))
        air = np.all([w_[..., 1] != 0 for w_ in walls], axis=0)
        ys, xs = np.nonzero(air)
        x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
        cur = [(m.read_rect(B_), m.read_rect(W_)) for m in we.members]
        corr = we.correlation(B_, (B_, x, y, 3))
        want = E.ens_cov_cells([c[0] for c in cur], [c[1] for c in cur], walls, Xw, Yw, B_, [(B_, x, y, 3)], want=("corr",))
        assert same_bits(corr, want["corr"][0]) and corr[y, x, 3] == np.float32(1.0)
        both = we.covariance(B_, [(B_, x, y, 3), np.array(J)], want=("corr",))
        assert same_bits(both["corr"][0], corr)
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
