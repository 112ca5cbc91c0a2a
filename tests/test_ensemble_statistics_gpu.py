"""Ensemble statistics on the GPU (wx_ensemble_statistics): the device result equals wx_ens_stat_cells on the members' read_rect arrays
and the definition of include/wxsim.h, written down as the explicit member loop `reference` of tests/test_ensemble_statistics_cpu.py --
every plane, both supported fields, whole grids and ragged rectangles, masks, non-finite and wall cells, members with droplets; the call
is ordered behind pending steps, changes nothing, and refuses what the header says it refuses. Every comparison is `==` on bits (NaNs
compared as positions)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import impulse_scenes as I
import surface_scenes as S
from test_ensemble_droplets_gpu import _order1, _precip64, pool_of
from test_ensemble_gpu import FIELDS, Twins, _slider_uniforms, same_bits, same_diag
from test_ensemble_statistics_cpu import CASES, N_SEL_CASES, PLANES, THRESHOLD, check, hand_built, reference, separating_cells_in

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("BASE_CUR", "WATER_CUR")
# vx, vy, pressure, temperature / total water, cloud water, precipitation, smoke: thresholds inside the ranges the scenes hold
THRESHOLDS = {"BASE_CUR": (0.01, 0.0, 0.0, 290.0), "WATER_CUR": (5.0, 0.001, 0.0, 0.5)}
# The boundary pass turns an air cell under a wall cell into wall below 0.99 of the height, and in a grid of at most 50 rows that starts at
# the top row: the wall grows down one row per iteration. A 9-row grid is wall in every cell of every member from the eighth iteration
# on, and its statistics after 12 iterations are the all-wall answer (n_wall = B, count 0, NaN, -1) whatever the members hold. The 9-row
# grids are therefore compared after EARLY iterations as well -- rows 1 .. 4 are still air where the member's terrain leaves them air --
# and what a test says about values that entered, it says about that state.
EARLY = 4


def member_specs(pkg, X, Y, B):
    """B members that differ in terrain (one, three or 2 .. 4 wall rows, planted wall cells: some cells are wall in some members only),
    contents, parameters and iteration counter."""
    specs = []
    for i in range(B):
        k, seed = i % 5, 100 + i
        if k == 0:
            b, w, wl = I.impulse_scene(X, Y, "smoke", offset=(i % 7, 1 + i % 3), seed=seed)[:3]
            u = I.scene_uniforms("smoke", Y)
        elif k == 1:
            b, w, wl = S.surface_scene(X, Y, "snow", offset=i % 5, seed=seed)[:3]
            u = S.scene_uniforms(Y)
        elif k == 2:
            b, w, wl = S.surface_scene(X, Y, "smoke", offset=i % 4, variant="stepped", seed=seed)[:3]
            u = S.scene_uniforms(Y, wrap=False)
        elif k == 3:
            b, w, wl = I.impulse_scene(X, Y, "cloud", offset=(i % 6, 2), seed=seed)[:3]
            u = _slider_uniforms(pkg, Y, 7 + i)
        else:
            b, w, wl = I.impulse_scene(X, Y, "wall", offset=(i % 9, 1 + i % 4), seed=seed)[:3]
            u = I.scene_uniforms("wall", Y)
        specs.append(dict(base=b, water=w, wall=wl, u=u, iter0=37 * i + (9990 if i == 1 else 0)))
    return specs


def make_ensemble(pkg, specs, n_droplets=0):
    E, P = pkg.engine, pkg.params
    Y, X = specs[0]["base"].shape[:2]
    ens = E.Ensemble(len(specs), X, Y, n_droplets)
    for i, s in enumerate(specs):
        if s is None:
            continue
        ens[i].upload(s["base"], s["water"], s["wall"], s.get("drops"))
        for opt, val in s.get("options", {}).items():
            ens[i].set_option(opt, val)
        ens[i].iter = s.get("iter0", 0)
        ens[i].set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
    return ens


class Stepped:
    """An ensemble stepped ``steps`` iterations, its members' fields as read_rect returns them, and the definition evaluated on them -- once."""

    def __init__(self, pkg, X, Y, B, steps=12):
        self.pkg, self.X, self.Y, self.B = pkg, X, Y, B
        self.ens = make_ensemble(pkg, member_specs(pkg, X, Y, B))
        self.ens.step(steps)
        self.walls = [m.read_rect("WALL_CUR") for m in self.ens.members]
        self.fields = {f: [m.read_rect(f) for m in self.ens.members] for f in STAT_FIELDS}
        self._ref = {}

    def ref(self, field, members=None):
        key = (field, None if members is None else tuple(members))
        if key not in self._ref:
            self._ref[key] = reference(self.fields[field], self.walls, members, THRESHOLDS[field])
        return self._ref[key]


@pytest.fixture(scope="module")
def stepped(pkg):
    made = {}

    def get(X, Y, B, steps=12):
        if (X, Y, B, steps) not in made:
            made[(X, Y, B, steps)] = Stepped(pkg, X, Y, B, steps)
        return made[(X, Y, B, steps)]

    yield get
    for s in made.values():
        s.ens.close()


def cut(planes, x, y, w, h):
    return {k: np.ascontiguousarray(v[y:y + h, x:x + w]) for k, v in planes.items()}


def rectangles(X, Y):
    return [(0, 0, X, Y), (3, 2, X - 5, Y - 5),                               # the whole grid, the interior
            (0, Y // 2, X, 1), (X // 3, 0, 1, Y), (X - 1, Y - 1, 1, 1),       # one row, one column, one cell
            (0, 1, 2, Y - 2), (X - 3, 0, 3, Y), (1, 0, X - 2, 2), (0, Y - 2, X, 2),  # touching the left, right, bottom and top edge
            (X - 65, 1, 65, 3) if X > 65 else (X - 33, 1, 33, 3)]             # ragged: a 64-lane chunk and one column, off the row start


@pytest.mark.parametrize("X,Y,B", [(57, 9, 1), (57, 9, 5), (57, 9, 70), (130, 50, 5), (505, 77, 3)])
def test_device_equals_host_equals_definition(pkg, stepped, X, Y, B):
    t = stepped(X, Y, B)
    device_equals_host_equals_definition(pkg, t)
    if Y == 9:  # (see EARLY)
        assert (t.ref("WATER_CUR")["n_wall"] == B).all()
        t = stepped(X, Y, B, EARLY)
        device_equals_host_equals_definition(pkg, t)
    # the members are different simulations on different terrain: the statistics are not trivial
    w = t.ref("WATER_CUR")
    if B > 1:
        assert 0 < w["n_wall"].max() <= B and ((w["n_wall"] > 0) & (w["n_wall"] < B)).any()
        assert (w["variance"][w["count"] > 1] > 0).any() and (w["argmax"] != w["argmin"]).any()
        assert (w["n_above"] > 0).any() and (w["n_above"] < w["count"]).any()


def device_equals_host_equals_definition(pkg, t):
    X, Y = t.X, t.Y
    for field in STAT_FIELDS:
        thr = THRESHOLDS[field]
        want = t.ref(field)
        host = pkg.engine.ens_stat_cells(t.fields[field], t.walls, threshold=thr)
        check(host, want, (field, "host function, whole grid"))
        for (x, y, w, h) in rectangles(X, Y):
            got = t.ens.statistics(field, x, y, w, h, threshold=thr)
            assert got["mean"].shape == (h, w, 4) and got["n_wall"].shape == (h, w) and got["argmax"].dtype == np.int32
            check(got, cut(want, x, y, w, h), (field, (x, y, w, h)))
        x, y, w, h = rectangles(X, Y)[1]  # the host function on the rectangle's own cells, as a host without the device call would
        sub = pkg.engine.ens_stat_cells([a[y:y + h, x:x + w] for a in t.fields[field]], [a[y:y + h, x:x + w] for a in t.walls], threshold=thr)
        check(sub, cut(want, x, y, w, h), (field, "host function, interior"))


def test_nonfinite_and_wall_cells(pkg):
    """Member 2 is uploaded with NaN / +Inf / -Inf in a few BASE_CUR cells, member 3 with a column of wall cells; nothing is stepped."""
    X, Y = 57, 9
    specs = member_specs(pkg, X, Y, 5)
    bad = [(6, 20, 0, np.nan), (6, 21, 3, np.inf), (7, 40, 1, -np.inf), (5, 56, 2, np.nan), (8, 0, 0, np.inf)]  # (y, x, channel, value): rows that are air in every member
    for (y, x, c, v) in bad:
        assert all(s["wall"][y, x, 1] != 0 for s in specs)
        specs[2]["base"][y, x, c] = v
    specs[3]["wall"] = specs[3]["wall"].copy()
    specs[3]["wall"][:, 10, 1] = 0
    ens = make_ensemble(pkg, specs)
    try:
        fields, walls = [m.read_rect("BASE_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        thr = THRESHOLDS["BASE_CUR"]
        want = reference(fields, walls, None, thr)
        got = ens.statistics("BASE_CUR", threshold=thr)
        check(got, want, "non-finite")
        check(pkg.engine.ens_stat_cells(fields, walls, threshold=thr), want, "non-finite, host")
        for (y, x, c, v) in bad:
            assert got["count"][y, x, c] == 4 and got["n_wall"][y, x] == 0 and got["argmin"][y, x, c] != 2 and got["argmax"][y, x, c] != 2, (y, x, c)
            assert np.isfinite(got["mean"][y, x, c]) and np.isfinite(got["max"][y, x, c]) and np.isfinite(got["min"][y, x, c])
            assert all(got["count"][y, x, o] == 5 for o in range(4) if o != c)
        assert (got["n_wall"][:, 10] >= 1).all() and got["n_wall"][Y - 1, 10] == 1 and (got["count"][Y - 1, 10] == 4).all()
        assert (got["argmin"][Y - 1, 10] != 3).all()
        assert (got["count"].sum(-1) + 4 * got["n_wall"] + np.isin(np.arange(X * Y).reshape(Y, X), [y * X + x for (y, x, _, _) in bad]) == 20).all()
    finally:
        ens.close()


PX, PY = 57, 9  # the grid the definition's planted cases are laid out on: cell i of hand_built is (y, x) = divmod(i, PX)


def uploaded_hand_built(pkg, B):
    """hand_built(B, 57 * 9) -- the planted cases and the separating cells in front (row 0), random float bit patterns and random walls
    behind -- uploaded as BASE and as WATER of B members; nothing is stepped, and an upload keeps every bit pattern."""
    f, w = hand_built(B, PX * PY)
    f, w = [a.reshape(PY, PX, 4) for a in f], [a.reshape(PY, PX, 4) for a in w]
    ens = pkg.engine.Ensemble(B, PX, PY, 0)
    for i in range(B):
        ens[i].upload(f[i], f[i], w[i])
    return ens, f, w


@pytest.mark.parametrize("B,members", CASES + N_SEL_CASES, ids=["7", "1", "70-masked", "n_sel=8", "n_sel=9", "n_sel=16"])
def test_planted_cases_on_the_device(pkg, B, members):
    """The cases of the definition that `hand_built` plants -- the fixed-order sum, subnormals with FLT_MAX, zeros of both signs, ties,
    values at / above / below a threshold, a subnormal and a NaN threshold, all-wall and all-non-finite cells -- and the separating
    cells, through k_ens_stat: the float compares of the device and the select-written cell_add meet them here."""
    ens, f, w = uploaded_hand_built(pkg, B)
    try:
        sel = list(range(B)) if members is None else list(members)
        walls = [m.read_rect("WALL_CUR") for m in ens.members]
        assert all(np.array_equal(a, b) for a, b in zip(walls, w))
        for field in STAT_FIELDS:
            fields = [m.read_rect(field) for m in ens.members]
            assert all(a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes() for a, b in zip(fields, f))  # (NaN payloads too)
            want = reference(fields, walls, members, THRESHOLD)
            check(pkg.engine.ens_stat_cells(fields, walls, members=members, threshold=THRESHOLD), want, (field, B, "host function"))
            for (x, y, rw, rh) in rectangles(PX, PY):
                got = ens.statistics(field, x, y, rw, rh, threshold=THRESHOLD, members=members)
                check(got, cut(want, x, y, rw, rh), (field, B, (x, y, rw, rh)))
            got = ens.statistics(field, threshold=THRESHOLD, members=members)
            row = {k: v[0] for k, v in got.items()}  # the planted cells, by value
            n_sel, zero = len(sel), np.float32(0).view(np.uint32)
            S = np.float64(0)
            for i in sel:  # 1: the sum in member order
                S = S + np.float64((list(np.float32([1e30, 1.0, -1e30, 1.0])) + [np.float32(0)] * 3)[i % 7])
            assert row["mean"][1, 0] == np.float32(S / np.float64(n_sel)) and row["count"][1, 0] == n_sel
            if B == 7:
                assert S == 1.0 and row["mean"][1, 0] == np.float32(1.0 / 7.0)  # 1, not the 0 of a sorted or pairwise sum
                assert row["n_above"][9].tolist() == [2, 2, 0, 2] and row["count"][9].tolist() == [7, 7, 7, 7]
                assert np.isfinite(row["mean"][2]).all() and row["max"][2, 0] == np.float32(3.4028234663852886e38)
                assert row["n_wall"][6] == 3 and row["count"][6, 0] == 4 and row["argmin"][6, 0] == 5 and row["argmax"][6, 0] == 2
                assert row["argmin"][7, 0] == 0 and row["argmax"][7, 1] == 0 and row["argmax"][7, 2] == 0 and row["argmin"][7, 3] == 1
            assert (row["variance"][0].view(np.uint32) == zero).all() and (row["mean"][0] == 1.5).all()
            assert (row["count"][4] == 0).all() and row["n_wall"][4] == 0 and np.isnan(row["max"][4]).all() and np.isnan(row["variance"][4]).all()
            assert row["n_wall"][5] == n_sel and (row["count"][5] == 0).all() and np.isnan(row["mean"][5]).all() and (row["argmin"][5] == -1).all()
            assert row["max"][7, 2].view(np.uint32) == zero  # the maximum is a -0.0 (member 0, 3, ...): reported as +0.0
            assert (row["n_above"][:, 2] == 0).all() and row["count"][10, 2] == n_sel  # the NaN threshold
            tied = [i for i in sel if i % 7 in (2, 5)]
            if tied:  # 8: the tie is held by the smaller member index
                assert row["argmin"][8, 0] == tied[0] and row["argmax"][8, 1] == tied[0] and row["min"][8, 0] == -7.0 and row["max"][8, 1] == 9.0
            here = separating_cells_in(B, members)
            assert bool(here) == (B > 1)
            for cell, _, _, defined, _ in here:
                assert (row["variance"][cell].view(np.uint32) == defined).all(), (field, B, cell)
    finally:
        ens.close()


FAST_STEPPED = [(6, None), CASES[2]]
FAST_UPLOADED = [CASES[0], CASES[2], N_SEL_CASES[2]]


def fast_leg_threshold(tag, field):
    return THRESHOLDS[field] if tag[0] == "s" else THRESHOLD


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_statistics_gpu as T
out = {}
def record(tag, ens, members):
    out[tag + "_WALL_CUR"] = np.stack([m.read_rect("WALL_CUR") for m in ens.members])
    for f in T.STAT_FIELDS:
        out[f"{tag}_{f}"] = np.stack([m.read_rect(f) for m in ens.members])
        for k, v in ens.statistics(f, threshold=T.fast_leg_threshold(tag, f), members=members).items():
            out[f"{tag}_{f}_{k}"] = v
    ens.close()
for B, members in T.FAST_STEPPED:
    ens = T.make_ensemble(pkg, T.member_specs(pkg, 57, 9, B))
    ens.step(T.EARLY)
    record(f"s{B}", ens, members)
for B, members in T.FAST_UPLOADED:
    record(f"u{B}", T.uploaded_hand_built(pkg, B)[0], members)
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its k_ens_stat gives what THIS process's host function
    and the definition give on the values the members held. Stepped members (the simulation steps of the two builds differ, the
    statistics of what they hold do not), and uploaded members that hold hand_built's data: among them the separating cells, the only
    data on which a Q += d * d that the code generator fused into an FMA shows in the float32 variance."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    dst = str(tmp_path / "fast.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, root, dst], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(dst)
    for tag, cases in (("s", FAST_STEPPED), ("u", FAST_UPLOADED)):
        for B, members in cases:
            walls = list(d[f"{tag}{B}_WALL_CUR"])
            for f in STAT_FIELDS:
                thr = fast_leg_threshold(tag, f)
                fields = list(d[f"{tag}{B}_{f}"])
                got = {k: d[f"{tag}{B}_{f}_{k}"] for k in PLANES}
                check(got, pkg.engine.ens_stat_cells(fields, walls, members=members, threshold=thr), (tag, B, f, "fast device vs exact host"))
                check(got, reference(fields, walls, members, thr), (tag, B, f, "fast device vs definition"))
                assert (got["variance"][got["count"] > 1] > 0).any()
                if tag == "u":  # the members held hand_built's bits, the separating cells among them
                    want = hand_built(B, PX * PY)[0]
                    assert all(a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes() for a, b in zip(fields, want))
                    here = separating_cells_in(B, members)
                    assert len(here) >= 3
                    for cell, _, _, defined, fused in here:
                        assert (got["variance"][0, cell].view(np.uint32) == defined).all() and defined != fused, (B, f, cell)


def test_masks(pkg, stepped):
    t = stepped(57, 9, 5, EARLY)
    for field in STAT_FIELDS:
        thr = THRESHOLDS[field]
        check(t.ens.statistics(field, threshold=thr, members=[0, 2, 4]), t.ref(field, (0, 2, 4)), (field, "members 0, 2, 4"))
        check(t.ens.statistics(field, 3, 2, 52, 4, threshold=thr, members=np.array([True, False, True, False, True])), cut(t.ref(field, (0, 2, 4)), 3, 2, 52, 4),
              (field, "boolean mask"))
        one = t.ens.statistics(field, threshold=thr, members=[3])
        check(one, t.ref(field, (3,)), (field, "member 3 alone"))
        entered = (t.walls[3][..., 1] != 0)[..., None] & np.isfinite(t.fields[field][3])
        assert same_bits(one["mean"][entered], t.fields[field][3][entered])
        assert (one["variance"][entered].view(np.uint32) == 0).all()  # +0.0
        assert (one["argmin"][entered] == 3).all() and (one["argmax"][entered] == 3).all() and (one["count"][entered] == 1).all()
        assert (one["argmin"][~entered] == -1).all() and np.isnan(one["mean"][~entered]).all() and (one["count"][~entered] == 0).all()
        assert entered.any() and not entered.all()


def test_ordered_behind_a_pending_step(pkg):
    """statistics directly after step(3), no sync in between: the numbers are those of the state AFTER the three iterations (the members'
    pointers are taken at the call: the planes have rotated), i.e. of the read_rects taken afterwards. (Iterations 3 and 6 of a 9-row
    grid: see EARLY.)"""
    ens = make_ensemble(pkg, member_specs(pkg, 57, 9, 5))
    try:
        seen = []
        for field in STAT_FIELDS:
            ens.step(3)
            got = ens.statistics(field, threshold=THRESHOLDS[field])
            want = reference([m.read_rect(field) for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members], None, THRESHOLDS[field])
            check(got, want, (field, "directly behind step(3)"))
            seen.append(ens.statistics("WATER_CUR")["mean"])
            assert np.isfinite(seen[-1]).any()
        assert not same_bits(seen[0][:3], seen[1][:3])  # (the iterations in between change the state: an unordered read would show)
        assert [m.iter for m in ens.members] == [s.get("iter0", 0) + 6 for s in member_specs(pkg, 57, 9, 5)]
    finally:
        ens.close()


def test_changes_nothing(pkg):
    """Every readable field, the diagnostics, the iteration counters and wx_ensemble_stats are the same before and after statistics
    calls, and five further iterations still equal lone handles that never saw the calls."""
    t = Twins(pkg, member_specs(pkg, 57, 9, 5))
    try:
        t.step(EARLY)

        def snapshot():
            return ([[m.read_rect(f) for f in FIELDS] for m in t.ens.members], t.ens.diagnostics(), [m.iter for m in t.ens.members], t.ens.stats())

        a = snapshot()
        for field in STAT_FIELDS:
            t.ens.statistics(field, threshold=THRESHOLDS[field])
            t.ens.statistics(field, 3, 2, 40, 5, members=[1, 3], want=("variance", "n_wall"))
        b = snapshot()
        for i in range(5):
            for k, f in enumerate(FIELDS):
                assert same_bits(a[0][i][k], b[0][i][k]), (i, f)
            assert same_diag(a[1][i], b[1][i]) is None, i
        assert a[2] == b[2] and a[3] == b[3]
        t.ens.statistics("BASE_CUR")  # ... and directly in front of a step
        t.step(5)
        t.compare("after statistics calls")
    finally:
        t.close()


def test_members_with_droplets(pkg, golden):
    """Ensemble(4, 64, 64, 400), deterministic splat order, precipitation on: WATER_CUR after 16 iterations."""
    g, u = _precip64(golden)
    drops = pool_of(np.ascontiguousarray(g["in_drops"], np.float32), 400)
    specs = []
    for i in range(4):
        water = g["in_water"].copy()
        water[40:44, 8 * i:8 * i + 8, 3] += np.float32(0.5 * (i + 1))  # smoke of its own: the members differ from the first iteration on
        specs.append(dict(base=g["in_base"], water=water, wall=g["in_wall"], drops=drops, u=dict(u, spawnChanceMult=float(u["spawnChanceMult"]) * (1 + i)),
                          iter0=int(g["iter0"]) + 101 * i, options=_order1(pkg)))
    ens = make_ensemble(pkg, specs, 400)
    try:
        ens.step(16)
        thr = THRESHOLDS["WATER_CUR"]
        got = ens.statistics("WATER_CUR", threshold=thr)
        fields, walls = [m.read_rect("WATER_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        want = reference(fields, walls, None, thr)
        check(got, want, "droplets")
        check(ens.statistics("WATER_CUR", 5, 7, 50, 41, threshold=thr, members=[1, 2]), cut(reference(fields, walls, (1, 2), thr), 5, 7, 50, 41), "droplets, rectangle")
        assert ens.particle_stats()["member_iters_particles_batched"] == 4 * 16
        assert (want["variance"] > 0).any() and any(np.abs(m.read_rect("PRECIP_FB")).max() > 0 for m in ens.members)
    finally:
        ens.close()


def test_refusals(pkg):
    E = pkg.engine
    X, Y = 57, 9
    specs = member_specs(pkg, X, Y, 3)
    ens = make_ensemble(pkg, specs[:2] + [None])  # member 2 is never uploaded
    try:
        def refused(code, *a, **kw):
            with pytest.raises(E.WxError) as ei:
                ens.statistics(*a, **kw)
            assert ei.value.code == code, (a, kw, str(ei.value))
            return str(ei.value)

        msg = refused(-1, "CURL", members=[0, 1])
        assert "WX_FIELD_BASE_CUR" in msg and "WX_FIELD_WATER_CUR" in msg
        for f in ("WALL_CUR", "BASE_DISP", "WATER_0", "LIGHT_0", "EMITTED"):
            refused(-1, f, members=[0, 1])
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (X, 0, 1, 1)):
            refused(-4, "BASE_CUR", *rect, members=[0, 1])
        assert "member 2" in refused(-5, "BASE_CUR")
        assert "member 2" in refused(-5, "WATER_CUR", members=[0, 2])
        refused(-1, "BASE_CUR", members=[])
        refused(-1, "BASE_CUR", members=np.zeros(3, bool))
        # the ensemble works as before: the uploaded members are served, and with member 2 uploaded all three step and are served
        fields, walls = [ens[i].read_rect("BASE_CUR") for i in (0, 1)], [ens[i].read_rect("WALL_CUR") for i in (0, 1)]
        check(ens.statistics("BASE_CUR", members=[0, 1]), reference(fields, walls), "two of three")
        s, P = specs[2], pkg.params
        ens[2].upload(s["base"], s["water"], s["wall"])
        ens[2].set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
        ens.step(2)
        fields, walls = [m.read_rect("WATER_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]
        check(ens.statistics("WATER_CUR"), reference(fields, walls), "all three")
        assert ens.stats()["member_iters_batched"] == 6
    finally:
        ens.close()


def test_an_overflowed_list_surfaces_here(pkg):
    """WX_OPT_FIX_CAP 2 on a member with fast cells: its report (WX_E_STATE) is what the statistics call returns, naming the member -- once."""
    E = pkg.engine
    X, Y = 505, 77
    fast = I.impulse_scene(X, Y, "fast_vx")
    specs = member_specs(pkg, X, Y, 3)
    specs[1] = dict(base=fast[0], water=fast[1], wall=fast[2], u=I.scene_uniforms("fast_vx", Y), options={E.Handle.OPT_FIX_CAP: 2})
    ens = make_ensemble(pkg, specs)
    try:
        ens.step(2)
        with pytest.raises(E.WxError) as ei:
            ens.statistics("BASE_CUR")
        assert ei.value.code == -5 and "member 1: " in str(ei.value), str(ei.value)
        got = ens.statistics("BASE_CUR")  # the report was consumed
        check(got, reference([m.read_rect("BASE_CUR") for m in ens.members], [m.read_rect("WALL_CUR") for m in ens.members]), "after the report")
    finally:
        ens.close()


def test_weather_ensemble_adds_the_probability(pkg):
    W = pkg.sim
    X, Y = 128, 48
    base, water, wall = pkg.synth.terrain_grid(X, Y)
    over = [{"wind": -0.5 + 0.25 * i, "dayNightCycle": False} for i in range(4)]
    we = W.WeatherEnsemble(4, X, Y, base, water, wall, None, over, sun_angle_deg=30.0)
    try:
        we.step(6)
        st = we.statistics("BASE_CUR", threshold=(0.0, 0.0, 0.0, 288.0))
        assert set(st) == set(PLANES) | {"probability"}
        raw = we.engine.statistics("BASE_CUR", threshold=(0.0, 0.0, 0.0, 288.0))
        check({k: st[k] for k in PLANES}, raw, "pass-through")
        p, n = st["probability"], st["count"]
        assert p.dtype == np.float64 and p.shape == (Y, X, 4)
        assert np.isnan(p[n == 0]).all() and (n == 0).any() and (n == 4).any()  # the terrain's wall cells are wall in every member
        assert np.array_equal(p[n > 0], st["n_above"][n > 0].astype(np.float64) / n[n > 0].astype(np.float64))
        assert ((p[n > 0] > 0) & (p[n > 0] < 1)).any()
        some = we.statistics("WATER_CUR", 2, 3, 20, 10, members=[0, 3], want=("mean",))
        assert set(some) == {"mean", "count", "n_above", "probability"} and some["probability"].shape == (10, 20, 4)
    finally:
        we.close()
