"""wx_ensemble_gram on the GPU: the matrix and the counts of the device equal wx_ens_gram_cells -- the definition on the CPU, which
tests/test_ensemble_gram_cpu.py pins to an independent restatement -- bit for bit: uploaded random members with the planted cells of
the CPU test in the first and in the last row, n = 2, 5, 9, 17, 33 and 64 selected members (one load group and a remainder, one pair
tile, three and ten, the cap), both centres, both fields, masks, a ragged last chunk and a rectangle strictly inside the grid whose x is
no multiple of 64; the second trip of both chunk loops; that the call changes nothing and repeats its bits; behind a step, on members
with droplets; the tolerance build; and WeatherEnsemble.eofs / distances / medoid end to end against float64 numpy with the derived
bound. Every comparison of the matrix is `==` on bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ensemble_gram_shapes as GS
import test_ensemble_gram_cpu as GC
from test_ensemble_covariance_cpu import cov_members
from test_ensemble_covariance_gpu import upload_ensemble
from test_ensemble_droplets_gpu import _order1, _precip64, pool_of
from test_ensemble_gpu import same_bits, same_diag
from test_ensemble_gram_cpu import B_, CENTERS, COUNTS, SELECTIONS, W_, compare, plant, row_cells, selection
from test_ensemble_statistics_gpu import make_ensemble, member_specs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y = 70, 9
INSIDE = (3, 1, 64, Y - 2)  # strictly inside the grid, x no multiple of 64, one full chunk per row
RAGGED = (61, 0, 9, Y)      # the planted cells of both rows, around the chunk boundary of the GRID but in one chunk of the rectangle


def grid_members(B, members, seed=5):
    """cov_members with the planted cells in the first and in the last row of BOTH fields, x = 60 .. 68."""
    bases, waters, wl = cov_members(B, X, Y, seed=seed)
    sel = selection(B, members)
    for y in (0, Y - 1):
        plant(bases, wl, sel, row_cells(y, 60))
        plant(waters, wl, sel, row_cells(y, 60))
    return bases, waters, wl


def device_equals_host(pkg, ens, fields, walls, field, where, **kw):
    Yg, Xg = walls[0].shape[:2]
    got = ens.gram(field, kw.get("rect"), kw.get("members"), kw.get("center", "mean"))
    compare(got, pkg.engine.ens_gram_cells(fields, walls, Xg, Yg, field, **kw), (where, field, kw))
    return got


@pytest.mark.parametrize("B,members", SELECTIONS, ids=lambda v: None if isinstance(v, list) else str(v))
def test_device_equals_host_function(pkg, B, members):
    n = len(selection(B, members))
    assert n in (2, 5, 9, 17, 33, 64)
    bases, waters, wl = grid_members(B, members)
    ens = upload_ensemble(pkg, bases, waters, wl)
    try:
        for field, fields in ((B_, bases), (W_, waters)):
            for center in CENTERS:
                got = device_equals_host(pkg, ens, fields, wl, field, (B, "whole"), members=members, center=center)
                assert (got["n_entered"] + got["n_excluded"] + got["n_overflow"] == X * Y).all()
                assert (got["n_entered"] > 0.8 * X * Y).all() and (got["n_excluded"] > 0).all() and got["n_overflow"][0] >= 2
                assert (np.diagonal(got["gram"], axis1=1, axis2=2) > 0).all()
                again = ens.gram(field, None, members, center)  # two calls: identical bits
                compare(again, got, (B, "again"))
        device_equals_host(pkg, ens, bases, wl, B_, (B, "inside"), rect=INSIDE, members=members, center="mean")
        device_equals_host(pkg, ens, waters, wl, W_, (B, "inside"), rect=INSIDE, members=members, center="none")
        for center in CENTERS:
            got = device_equals_host(pkg, ens, bases, wl, B_, (B, "ragged"), rect=RAGGED, members=members, center=center)
            if n >= 4:  # the two largest-finite cells: 2 * FLT_MAX off the diagonal, which no float holds
                assert center == "none" or got["gram"][0, 0, 2] > 1.9 * float(GC.FLT_MAX)
        for m, b, w in zip(ens.members, bases, waters):  # nothing was written
            assert same_bits(m.read_rect(B_), b) and same_bits(m.read_rect(W_), w)
    finally:
        ens.close()


@pytest.mark.parametrize("n", [3, 64])
def test_planted_cells_through_the_kernels(pkg, n):
    """The planted row alone, one chunk of nine lanes (row 2 of a grid of four rows: the smallest a handle takes): the value-level
    expectations of the CPU test on the device's answer."""
    for center in CENTERS:
        row, row_walls, _ = GC.planted_row(n, center)
        fields = [np.ascontiguousarray(np.repeat(f, 4, axis=0)) for f in row]
        walls = [np.ascontiguousarray(np.repeat(w, 4, axis=0)) for w in row_walls]
        ens = upload_ensemble(pkg, fields, fields, walls)
        try:
            got = device_equals_host(pkg, ens, fields, walls, W_, ("planted", n), center=center, rect=(0, 2, GC.N_PLANTED, 1))
            GC.planted_expectations(got, n, center)
        finally:
            ens.close()


def test_chunk_loops_second_trip(pkg):
    """2 columns and just over MAX_WGS * WG / 64 rows, three members: one chunk per row, more rows than the pre-pass's capped grid has
    waves and sixteen times the pair kernel's slots (tests/test_ensemble_gram_cpu.py computes that from the header). The planted
    cells in rows of the first and of the last trip."""
    Xt, Yt = GS.tall_grid()
    first, last = GS.tall_planted_rows()
    rng = np.random.Generator(np.random.Philox(5))
    mk = lambda: (rng.normal(0, 1, (Yt, Xt, 4)) * np.array([0.1, 0.1, 0.01, 2.0]) + np.array([0, 0, 0, 300.0])).astype(np.float32)  # noqa: E731
    bases = [mk() for _ in range(GS.TALL_MEMBERS)]
    waters = [np.abs(mk()) for _ in range(GS.TALL_MEMBERS)]
    wl = [np.full((Yt, Xt, 4), 3, np.int8) for _ in range(GS.TALL_MEMBERS)]
    for row in (first, last):
        cells = [(row + j // Xt, j % Xt) for j in range(GC.N_PLANTED)]
        plant(bases, wl, [0, 1, 2], cells)
    ens = upload_ensemble(pkg, bases, waters, wl)
    try:
        for center in CENTERS:
            got = device_equals_host(pkg, ens, bases, wl, B_, "tall", center=center)
            assert got["n_excluded"].tolist() == [4, 4, 4, 2] and got["n_overflow"].tolist() == [2 if center == "mean" else 4, 0, 0, 0]
            # the rows of the last trip alone: what a dropped last flush would lose
            tail = device_equals_host(pkg, ens, bases, wl, B_, "tall, last trip", center=center, rect=(0, last, Xt, Yt - last))
            assert (np.diagonal(tail["gram"], axis1=1, axis2=2) > 0).all()
        device_equals_host(pkg, ens, waters, wl, W_, "tall, water", center="mean", members=[0, 2])
    finally:
        ens.close()


def test_the_call_changes_nothing_behind_a_step(pkg):
    """Directly behind wx_ensemble_step: both fields and the diagnostics of every member are the same before and after the call, two
    calls give the same bits, the device equals the host function on the read-back arrays, and a twin that never made the call steps to
    the same state."""
    Xs, Ys = 70, 40
    specs = member_specs(pkg, Xs, Ys, 3)
    ens, twin = make_ensemble(pkg, specs), make_ensemble(pkg, specs)
    try:
        ens.step(4), twin.step(4)
        first = {(f, c): ens.gram(f, None, None, c) for f in (B_, W_) for c in CENTERS}  # (directly behind the step)
        before = [(m.read_rect(B_), m.read_rect(W_), m.read_rect("WALL_CUR")) for m in ens.members]
        diag = ens.diagnostics()
        iters = [m.iter for m in ens.members]
        for (f, c), got in first.items():
            fields = [b[0] if f == B_ else b[1] for b in before]
            compare(got, pkg.engine.ens_gram_cells(fields, [b[2] for b in before], Xs, Ys, f, center=c), ("behind a step", f, c))
            compare(ens.gram(f, None, None, c), got, ("again", f, c))
            assert (got["n_entered"] > 0).all() and (got["n_excluded"] > 0).all()
        part = device_equals_host(pkg, ens, [b[0] for b in before], [b[2] for b in before], B_, "two members, inside", rect=(5, 3, 60, 30), members=[0, 2])
        assert part["members"] == [0, 2] and part["gram"].shape == (4, 2, 2)
        for m, b in zip(ens.members, before):
            assert same_bits(m.read_rect(B_), b[0]) and same_bits(m.read_rect(W_), b[1]) and same_bits(m.read_rect("WALL_CUR"), b[2])
        after = ens.diagnostics()
        assert all(same_diag(a, b) is None for a, b in zip(after, diag)) and [m.iter for m in ens.members] == iters == [m.iter for m in twin.members]
        assert ens.stats() == twin.stats()
        ens.step(3), twin.step(3)
        for a, b in zip(ens.members, twin.members):
            for f in (B_, W_, "WALL_CUR", "LIGHT_1"):
                assert same_bits(a.read_rect(f), b.read_rect(f)), f
    finally:
        ens.close(), twin.close()


def test_members_with_droplets(pkg, golden):
    """Four members with 400 droplets each, precipitation on: the Gram matrix of WATER_CUR after 16 iterations."""
    g, u = _precip64(golden)
    drops = pool_of(np.ascontiguousarray(g["in_drops"], np.float32), 400)
    specs = []
    for i in range(4):
        water = g["in_water"].copy()
        water[40:44, 8 * i:8 * i + 8, 3] += np.float32(0.5 * (i + 1))
        specs.append(dict(base=g["in_base"], water=water, wall=g["in_wall"], drops=drops, u=dict(u, spawnChanceMult=float(u["spawnChanceMult"]) * (1 + i)),
                          iter0=int(g["iter0"]) + 101 * i, options=_order1(pkg)))
    ens = make_ensemble(pkg, specs, 400)
    try:
        ens.step(16)
        got = ens.gram(W_)
        f, w = [m.read_rect(W_) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        Yd, Xd = w[0].shape[:2]
        compare(got, pkg.engine.ens_gram_cells(f, w, Xd, Yd, W_), "droplets")
        device_equals_host(pkg, ens, f, w, W_, "droplets, rectangle", rect=(5, 7, 50, 41), members=[1, 2, 3], center="none")
        assert (np.diagonal(got["gram"], axis1=1, axis2=2)[3] > 0).all() and ens.particle_stats()["member_iters_particles_batched"] == 4 * 16
    finally:
        ens.close()


FAST_CASES = [(5, None, "mean", B_), (11, [0, 1, 2, 4, 5, 7, 8, 9, 10], "none", W_), (17, None, "mean", W_)]
_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_gram_gpu as G
out = {}
for j, (B, members, center, field) in enumerate(G.FAST_CASES):
    bases, waters, wl = G.grid_members(B, members)
    ens = G.upload_ensemble(pkg, bases, waters, wl)
    got = ens.gram(field, None, members, center)
    ens.close()
    out["gram%d" % j] = got["gram"]
    for k in G.COUNTS:
        out["%s%d" % (k, j)] = got[k]
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernels give what THIS process's host function gives
    on the same uploaded members."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    path = str(tmp_path / "fast.npz")
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, ROOT, path], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(path)
    for j, (B, members, center, field) in enumerate(FAST_CASES):
        bases, waters, wl = grid_members(B, members)
        want = pkg.engine.ens_gram_cells(bases if field == B_ else waters, wl, X, Y, field, members=members, center=center)
        assert same_bits(d["gram%d" % j], want["gram"]) and all(np.array_equal(d["%s%d" % (k, j)], want[k]) for k in COUNTS), (B, center, field)


def test_every_refusal_of_the_device_call(pkg):
    """wx_ensemble_gram's own argument checks on a live ensemble of 66 members whose last was never uploaded: each refusal of
    include/wxsim.h with its code and its message, the never-uploaded member named; every refused call leaves the caller's matrix and
    counts as they were, launches no kernel (the profile of member 0 records none), and the ensemble answers the next valid call with
    the host function's bits."""
    E = pkg.engine
    B = 66
    bases, waters, wl = grid_members(B, None)
    ens = make_ensemble(pkg, [dict(base=b, water=w, wall=l, u=pkg.params.uniforms_from_gui(pkg.params.merge_settings(None), Y))
                              for b, w, l in zip(bases[:B - 1], waters[:B - 1], wl[:B - 1])] + [None])
    L = E.lib()
    out = np.full((4, 66, 66), 7.0)
    try:
        ens[0].profile(True)

        def raw(code, members, field=E.FIELD_IDS[B_], center=0, rect=(0, 0, X, Y), gram=True, desc=True):
            g = E.WxEnsGram()
            g.field, g.center = field, center
            g.x, g.y, g.w, g.h = rect
            g.gram = out.ctypes.data if gram else None
            g.n_selected = -5
            out[...] = 7.0
            mask = np.zeros(B, np.uint8)
            mask[list(members)] = 1
            rc = L.wx_ensemble_gram(ens._e, C.byref(g) if desc else None, mask.ctypes.data)
            assert rc == code, (rc, code, members, field, center, rect)
            assert (out == 7.0).all() and g.n_selected == -5 and not any(g.n_entered[:]) and not any(g.n_overflow[:])  # nothing was written
            return (L.wx_ensemble_last_error(ens._e) or b"").decode()

        some = [0, 1, 2]
        # WX_E_INVALID
        assert L.wx_ensemble_gram(None, C.byref(E.WxEnsGram()), None) == GC.E_INVALID
        raw(GC.E_INVALID, some, desc=False)
        for f in ("CURL", "BASE_DISP", "WATER_0", "WALL_CUR"):
            assert "field" in raw(GC.E_INVALID, some, field=E.FIELD_IDS[f])
        assert "center" in raw(GC.E_INVALID, some, center=2) and "center" in raw(GC.E_INVALID, some, center=-1)
        assert "NULL" in raw(GC.E_INVALID, some, gram=False)
        assert "fewer than two" in raw(GC.E_INVALID, [4]) and "fewer than two" in raw(GC.E_INVALID, [])  # MEAN takes two
        assert "nobody" in raw(GC.E_INVALID, [], center=1)  # NONE takes one
        assert "64" in raw(GC.E_INVALID, range(65)) and "64" in raw(GC.E_INVALID, range(65), center=1)  # 65 uploaded members selected
        assert "64" in raw(GC.E_INVALID, range(B))  # (in front of the look at the members: the 66th was never uploaded)
        # ... and an invalid descriptor is answered in front of the selection, the selection in front of the rectangle
        assert "field" in raw(GC.E_INVALID, [4], field=1, rect=(0, 0, X + 1, 1)) and "fewer" in raw(GC.E_INVALID, [4], rect=(0, 0, X + 1, 1))
        # WX_E_RANGE
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (X, 0, 1, 1)):
            assert "outside" in raw(GC.E_RANGE, some, rect=rect), rect
        assert "outside" in raw(GC.E_RANGE, [1, B - 1], rect=(0, 0, X + 1, 1))  # (the rectangle in front of the look at the members)
        # WX_E_STATE: the member that was never uploaded, named
        assert "member 65" in raw(GC.E_STATE, [0, B - 1]) and "member 65" in raw(GC.E_STATE, [B - 1], center=1)
        assert "member 65" in raw(GC.E_STATE, list(range(2, 65)) + [B - 1])  # 64 selected: the cap itself is taken
        # the Python layer hands the same codes on
        for code, kw in ((GC.E_INVALID, dict(field="CURL", members=some)), (GC.E_INVALID, dict(members=[3])), (GC.E_RANGE, dict(members=some, rect=(0, 0, X, Y + 1))),
                         (GC.E_STATE, dict(members=[0, B - 1])), (GC.E_INVALID, dict(members=None))):
            with pytest.raises(E.WxError) as ei:
                ens.gram(kw.pop("field", B_), kw.get("rect"), kw.get("members"), "mean")
            assert ei.value.code == code, (kw, str(ei.value))
        # no refused call launched anything
        prof = ens[0].profile_read()
        assert not any(k.startswith("ensemble_gram") for k in prof), prof
        # the ensemble is as usable as before: the cap itself, 64 of the 65 uploaded members, and the uploads untouched
        sel = list(range(64))
        for center in CENTERS:
            got = device_equals_host(pkg, ens, bases[:B - 1] + [None], wl[:B - 1] + [None], B_, "after the refusals", members=sel, center=center)
            assert got["gram"].shape == (4, 64, 64)
        device_equals_host(pkg, ens, waters[:B - 1] + [None], wl[:B - 1] + [None], W_, "after the refusals, one member", members=[64], center="none")
        prof = ens[0].profile_read()
        assert prof["ensemble_gram_centre"][1] == 3 and prof["ensemble_gram"][1] == 3
        assert all(same_bits(ens[i].read_rect(B_), bases[i]) for i in (0, 31, 64))
        ens.sync()  # (no step: member 65 was never uploaded)
    finally:
        ens.close()


def test_profile_names_both_kernels(pkg):
    bases, waters, wl = grid_members(5, None)
    ens = upload_ensemble(pkg, bases, waters, wl)
    try:
        ens[0].profile(True)
        ens.gram(B_)
        prof = ens[0].profile_read()
        assert prof["ensemble_gram_centre"][1] == 1 and prof["ensemble_gram"][1] == 1 and prof["ensemble_gram"][0] > 0
    finally:
        ens.close()


def test_eofs_distances_medoid_end_to_end(pkg):
    """Members uploaded as mean + a_k P1 + b_k P2 with two orthogonal sign patterns and dyadic a, b (every member is exact in float32,
    so the centred members have rank 2 exactly). The eigenvalues of WeatherEnsemble.eofs against those of the float64 Gram matrix of
    the read_rect'ed members. THE BOUND, derived: a term (float)(d_a d_b) carries a relative error of at most 2^-24 (no subnormals
    here), so |dG_ab| <= 2^-24 sum |d_a d_b| <= 2^-24 sqrt(G_aa G_bb); the spectral norm of dG is at most n max|dG_ab| <= n 2^-24
    max_a G_aa, and by Weyl's inequality |d lambda| <= n 2^-24 max_a G_aa / (n - 1), G summed over the channels. The eigenvalues from
    the third on are below the same bound."""
    W = pkg.sim
    n = 8
    yy, xx = np.mgrid[0:Y, 0:X]
    P1 = np.where(xx < X // 2, 1.0, -1.0)[..., None] * np.ones(4)
    P2 = np.where(yy % 2 == 0, 1.0, -1.0)[..., None] * np.array([1.0, -1.0, 1.0, 1.0])
    P2[Y - 1] = 0.0  # (an even number of rows carries P2: orthogonal to the constant as well)
    assert (P1 * P2).sum() == 0 and P2.sum(axis=(0, 1)).tolist() == [0, 0, 0, 0]
    a = np.array([-2.0, -1.5, -0.5, 0.0, 0.25, 0.75, 1.0, 2.0])
    b = np.array([0.5, -0.25, 1.0, -1.0, 0.25, -0.5, 0.75, -0.75])
    mean = np.array([0.5, -0.25, 1.0, 300.0]) * np.ones((Y, X, 4))
    members = [(mean + a[k] * 0.5 * P1 + b[k] * 0.25 * P2).astype(np.float32) for k in range(n)]
    assert all((m.astype(np.float64) == mean + a[k] * 0.5 * P1 + b[k] * 0.25 * P2).all() for k, m in enumerate(members))
    wall = np.zeros((Y, X, 4), np.int8)
    wall[..., 1] = 3
    water = np.abs(members[0]) * np.float32(0.001)
    we = W.WeatherEnsemble(n, X, Y, members[0], water, wall, {"dayNightCycle": False}, perturb=lambda i, b_, w_, wl_: (members[i], w_, wl_))
    try:
        read = np.stack([m.read_rect(B_) for m in we.members]).astype(np.float64)
        assert all(same_bits(m.read_rect(B_), members[k]) for k, m in enumerate(we.members))
        D = (read - read.mean(axis=0)).reshape(n, -1)
        G64 = D @ D.T
        lam64 = np.linalg.eigvalsh(G64 / (n - 1))[::-1]
        bound = n * 2.0 ** -24 * np.diag(G64).max() / (n - 1)
        out = we.eofs(B_, k=2)
        lam = out["eigenvalues"]
        print("eigenvalues", lam[:3], "float64", lam64[:3], "bound", bound, "largest difference", np.abs(lam - lam64).max())
        assert lam.shape == (n,) and (np.abs(lam - lam64) <= bound).all()
        assert (np.abs(lam[2:]) <= bound).all() and lam[1] > 100 * bound  # rank 2, and the second is no noise
        # the known answer: N cov(a / 2, b / 4) with N cells x channels carrying P1 (and almost as many P2)
        assert abs(out["explained"][:2].sum() - 1.0) < 1e-5 and out["pcs"].shape == (n, 2) and out["patterns"].shape == (2, Y, X, 4)
        assert np.allclose(out["pcs"].std(axis=0, ddof=1), 1.0, rtol=1e-9) and np.allclose(out["pcs"].mean(axis=0), 0.0, atol=1e-6)
        # a pattern is (float)(Cq / (n - 1)), Cq a float64 sum of n products: the conversion's 2^-24 relative (2^-23 asserted) and
        # float64 rounding of n terms of at most max|d| max|pc| each on either route (2^-45 max|d| max|pc| asserted: n = 8)
        want_patterns = (out["pcs"].T @ D / (n - 1)).reshape(2, Y, X, 4)
        slack = 2.0 ** -45 * np.abs(D).max() * np.abs(out["pcs"]).max()
        assert (np.abs(out["patterns"] - want_patterns) <= 2.0 ** -23 * np.abs(want_patterns) + slack).all()
        # the patterns span the planted ones
        for p in out["patterns"]:
            coef = np.linalg.lstsq(np.stack([P1.ravel(), P2.ravel()], axis=1), p.astype(np.float64).ravel(), rcond=None)
            # (each value within 2^-24 of a combination of P1 and P2, which the least-squares fit then misses by no more)
            assert np.abs(p.astype(np.float64).ravel() - np.stack([P1.ravel(), P2.ravel()], axis=1) @ coef[0]).max() <= 2.0 ** -23 * np.abs(p).max()
        with pytest.raises(ValueError):
            we.eofs(B_, k=9)
        # distances and the medoid against numpy on the same distances
        dist = we.distances(B_)
        want = np.sqrt(((read[:, None] - read[None]) ** 2).sum(axis=(2, 3, 4)))
        # the bound of the docstring on the squares: |dG_ab| <= 2^-24 sqrt(G_aa G_bb) in each of G_aa + G_bb - 2 G_ab, so
        # |d(dist^2)| <= 4 * 2^-24 max G_aa (float64 rounding of either route is eight orders below that)
        d2_bound = 4 * 2.0 ** -24 * np.diag(G64).max()
        print("distances squared: largest difference", np.abs(dist ** 2 - want ** 2).max(), "bound", d2_bound)
        assert dist.shape == (n, n) and (dist == dist.T).all() and (np.diag(dist) == 0).all() and (np.abs(dist ** 2 - want ** 2) <= d2_bound).all()
        assert we.medoid(B_) == int(np.argmin(dist.sum(axis=1)))
        sel = [1, 2, 5, 7]
        sub = we.distances(B_, members=sel)
        assert we.medoid(B_, members=sel) == sel[int(np.argmin(sub.sum(axis=1)))]
        assert (np.abs(sub ** 2 - want[np.ix_(sel, sel)] ** 2) <= d2_bound).all()  # (a sub-selection's mean differs; its G_aa are no larger than 4 max G_aa / 4)
        g = we.gram(W_, rect=(3, 1, 64, 5), center="none")
        assert g["gram"].shape == (4, n, n) and (g["n_entered"] == 64 * 5).all()
    finally:
        we.close()
