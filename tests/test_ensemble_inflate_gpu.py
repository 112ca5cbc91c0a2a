"""wx_ensemble_inflate, wx_ensemble_prior_save and wx_ensemble_prior_drop on the GPU: after every call the members' BASE_CUR and
WATER_CUR equal wx_ens_inflate_cells -- the definition on the CPU, which tests/test_ensemble_inflate_cpu.py pins to the text of
include/wxsim.h -- of the values they held before (read through a device-side clone) and of the values they held when the snapshot was
taken; the lambda map equals the host's; the planted cells and the separators of the CPU test go through the kernel; the chunk loops
take their second trip; the tolerance build gives the same bits; the snapshot rules, the refusals and the bookkeeping; and the workflow
clone -> perturb -> step -> analysis with relaxation -> statistics. Every comparison is `==` on bits (NaNs compared as positions)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ensemble_trip_shapes as T
import impulse_scenes as I
from test_ensemble_gpu import same_bits
from test_ensemble_inflate_cpu import PLANTED, PLANTED_IDS, SEPARATORS, plant_separators, separator_cell
from test_ensemble_perturb_gpu import pre_values
from test_ensemble_statistics_gpu import make_ensemble, member_specs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
X, Y = 70, 40
B_, W_ = "BASE_CUR", "WATER_CUR"
FIELDS = (B_, W_)
# the minimum, a partial load group, a group of 8 plus one, many groups; the second entry of each: a mask
MASKS = {2: [None, None], 5: [None, [0, 2, 3]], 9: [None, [0, 1, 2, 3, 4, 5, 7, 8]], 70: [None, [i for i in range(70) if i % 7 != 3]]}


def cut(a, rect):
    x, y, w, h = rect
    return np.ascontiguousarray(a[y:y + h, x:x + w])


def host(pkg, cur, prior, field, coef, rect, members, Xg=X, Yg=Y, **kw):
    """wx_ens_inflate_cells on the rectangle's cells of ``cur`` / ``prior`` (one dict per member), pasted back: what the members should
    hold in ``field`` now, and the lambda map of the rectangle (None in RTPP)."""
    rect = (0, 0, Xg, Yg) if rect is None else rect
    x, y, w, h = rect
    sel = range(len(cur)) if members is None else members
    pick = lambda src, f: [cut(src[i][f], rect) if i in sel else None for i in range(len(cur))]  # noqa: E731
    want_lambda = kw.get("mode", "const") != "rtpp"
    got = pkg.engine.ens_inflate_cells(pick(cur, field), pick(cur, "WALL_CUR"), field, coef, priors=None if prior is None else pick(prior, field),
                                       members=members, want_lambda=want_lambda, **kw)
    new, lam = got if want_lambda else (got, None)
    out = []
    for i, p in enumerate(cur):
        f = p[field].copy()
        if new[i] is not None:
            f[y:y + h, x:x + w] = new[i]
        out.append(f)
    return out, lam


# (mode, coef, keywords) of the calls of one round; round 1 adds a rectangle
CALLS = [
    ("const", (1.25, 1.0, 0.5, 1.0625), {}),
    ("rtps", (0.5, 0.0, 1.0, 0.9), dict(lambda_bounds=(0.8, 1.5))),
    ("rtpp", (0.5, 1.0, 0.0, 0.25), {}),
    ("rtps", 1.0, dict(lo=(NAN, NAN, 0.0, NAN))),
    ("const", 3.0, dict(lo=(-0.1, NAN, 0.0, 299.0), hi=(0.4, 0.2, NAN, 301.0))),
    ("rtpp", 0.8, dict(lo=0.0)),
]


@pytest.mark.parametrize("B", [2, 5, 9, 70])
def test_device_equals_host_function(pkg, B):
    """Members on different terrain, stepped; a snapshot of both fields; stepped on (the state now differs from the prior); then all
    three modes on both fields -- round 0: everybody, the whole grid; round 1: a mask, an offset rectangle inside an offset snapshot --
    with the lambda map wanted and not, each compared on every member and both fields against the host function of the values before."""
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, B))
    try:
        ens.step(2)
        changed = {f: 0 for f in FIELDS}
        lam_seen = 0
        for rnd, members in enumerate(MASKS[B]):
            snap_rect, rect = (None, None) if rnd == 0 else ((3, 1, 66, 38), (5, 2, 64, 33))
            prior = pre_values(pkg, ens)
            for f in FIELDS:
                ens.save_prior(f, snap_rect, members)
            for i, m in enumerate(ens.members):  # the members after prior_save: untouched
                assert all(same_bits(m.read_rect(f), prior[i][f]) for f in FIELDS), (rnd, i)
            ens.step(2)
            cur = pre_values(pkg, ens)
            assert not same_bits(cur[0][B_], prior[0][B_])
            for k, (mode, coef, kw) in enumerate(CALLS):
                field = FIELDS[(k + rnd) % 2]
                want_lambda = mode != "rtpp" and (k + rnd) % 3 != 1
                before = cur
                lam = ens.inflate(field, coef, mode=mode, rect=rect, members=members, want_lambda=want_lambda, **kw)
                new, want_lam = host(pkg, before, prior, field, coef, rect, members, mode=mode, **kw)
                cur = [dict(p, **{field: n}) for p, n in zip(before, new)]
                where = (B, rnd, k, mode, field)
                if want_lambda:
                    assert same_bits(lam, want_lam), (where, "lambda", np.argwhere(lam.view(np.uint32) != want_lam.view(np.uint32))[:4].tolist())
                    lam_seen += int(np.isfinite(lam).sum())
                else:
                    assert lam is None
                for i, m in enumerate(ens.members):
                    for f in FIELDS:
                        got = m.read_rect(f)
                        assert same_bits(got, cur[i][f]), (where, f, "member", i, np.argwhere(got.view(np.uint32) != cur[i][f].view(np.uint32))[:4].tolist())
                        if f != field or (members is not None and i not in members):
                            assert same_bits(got, before[i][f]), (where, f, "the other field / an unselected member", i)
                        elif rect is not None:
                            outside = np.ones((Y, X), bool)
                            outside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = False
                            assert same_bits(got[outside], before[i][f][outside]), (where, f, "outside the rectangle", i)
                        changed[f] += int(not same_bits(got, before[i][f]))
            # the snapshot after the inflates: RTPP with alpha = 1 still rebuilds the prior's perturbations
            before = cur
            ens.inflate(B_, 1.0, mode="rtpp", rect=rect, members=members)
            new, _ = host(pkg, before, prior, B_, 1.0, rect, members, mode="rtpp")
            cur = [dict(p, **{B_: n}) for p, n in zip(before, new)]
            assert all(same_bits(m.read_rect(B_), cur[i][B_]) for i, m in enumerate(ens.members)), (B, rnd, "snapshot")
        assert changed[B_] > 0 and changed[W_] > 0 and lam_seen > 0
        for i, m in enumerate(ens.members):
            assert same_bits(m.read_rect("WALL_CUR"), cur[i]["WALL_CUR"])
        ens.step(1)  # ... and the ensemble steps on
        ens.sync()
    finally:
        ens.close()


def device_run(pkg):
    """`run` of the planted cases of tests/test_ensemble_inflate_cpu.py on the device: the snapshot values are uploaded as BASE_CUR and
    saved, the values are uploaded over them (nothing is stepped), the call is made, and what the members hold then and the lambda map
    equal the host function's bit for bit; the device's arrays go back to the case's value-level assertions."""
    E, P = pkg.engine, pkg.params

    def run(fields, walls, priors, coef, where, **kw):
        Yp, Xp = fields[0].shape[:2]
        u = P.uniforms_from_gui(P.merge_settings(None), Yp)
        water = np.zeros((Yp, Xp, 4), np.float32)
        mode = kw.get("mode", "const")
        ens = E.Ensemble(len(fields), Xp, Yp, 0)
        try:
            for src in ((priors, fields) if mode != "const" else (fields,)):
                for m, b, wl in zip(ens.members, src, walls):
                    m.upload(b, water, wl)
                    m.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
                    assert b.view(np.uint32).tobytes() == m.read_rect(B_).view(np.uint32).tobytes(), where  # the planted bits are on the device
                if src is priors:
                    ens.save_prior(B_)
            want_lambda = mode != "rtpp"
            lam = ens.inflate(B_, coef, want_lambda=want_lambda, **kw)
            want = E.ens_inflate_cells(fields, walls, B_, coef, priors=priors, want_lambda=want_lambda, **kw)
            want, want_lam = want if want_lambda else (want, None)
            got = [m.read_rect(B_) for m in ens.members]
            for i in range(len(fields)):
                assert same_bits(got[i], want[i]), (where, "member", i, np.argwhere(got[i].view(np.uint32) != want[i].view(np.uint32))[:4].tolist())
                assert same_bits(ens[i].read_rect(W_), water), (where, "the other field", i)
            if want_lambda:
                assert same_bits(lam, want_lam), (where, "lambda")
            return got, lam
        finally:
            ens.close()

    return run


@pytest.mark.parametrize("B", [5, 9])
@pytest.mark.parametrize("case,placements", PLANTED, ids=PLANTED_IDS)
def test_planted_cases_through_the_member_walks_of_the_kernel(pkg, case, placements, B):
    """The planted cells of the CPU test through k_ens_prior_save and k_ens_inflate on 17 x 7: a wall, NaN / +-Inf / FLT_MAX in one
    member's value and snapshot value (with B = 9 once inside the load group of 8, once in the remainder member behind it; B = 5 walks
    the remainder loop alone), -0.0 with lambda == 1 and a neutral coefficient, sa == 0, lambda at each bound, the overflow in one
    member only, both clamp edges."""
    for kw in placements if B == 9 else placements[:1]:
        case(device_run(pkg), B=B, **kw)


def separator_specs(pkg):
    """Three members (uploaded, not stepped) with tools/find_inflate_separators.py's values planted: the current state, the state that
    holds the snapshot values, and the calls (mode, separator, x, coef)."""
    cur = member_specs(pkg, X, Y, 3)
    for s in cur:
        s["base"], s["wall"] = np.array(s["base"], np.float32), np.array(s["wall"], np.int8)
    prior = [dict(s, base=s["base"].copy()) for s in cur]
    calls = []
    for mode in ("const", "rtps"):
        calls += [(mode,) + c for c in plant_separators([s["base"] for s in cur], [s["wall"] for s in cur], [s["base"] for s in prior], mode)]
    for s, p in zip(cur, prior):
        p["wall"] = s["wall"]
    return cur, prior, calls


def run_separators(pkg, make=make_ensemble):
    """The separator calls on the device, each on the rectangle of its own cell; returns member 0's BASE_CUR afterwards."""
    cur, prior, calls = separator_specs(pkg)
    ens = make(pkg, prior)
    try:
        ens.save_prior(B_)
        for m, s in zip(ens.members, cur):
            m.upload(s["base"], s["water"], s["wall"])
        for mode, i, x, coef in calls:
            ens.inflate(B_, ((1.0 if mode == "const" else 0.0),) * 3 + (coef,), mode=mode, rect=(x, separator_cell(i)[1], 1, 1))
        return ens[0].read_rect(B_)
    finally:
        ens.close()


def check_separators(got_base0):
    for i, (_, _, _, _, _, defined, fused) in enumerate(SEPARATORS):
        x, y = separator_cell(i)
        assert int(got_base0[y, x, 3].view(np.uint32)) == defined != fused, (i, int(got_base0[y, x, 3].view(np.uint32)), defined, fused)


def test_planted_separators_on_the_device(pkg):
    """Member values on which a fused lambda*d_k or d_k*d_k changes a float32 result: the device gives the defined bits."""
    check_separators(run_separators(pkg))


FAST_MEMBERS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 16]
_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_inflate_gpu as G
ens = G.make_ensemble(pkg, G.member_specs(pkg, G.X, G.Y, 17))
ens.step(2)
prior = G.pre_values(pkg, ens)
for f in G.FIELDS:
    ens.save_prior(f, None, G.FAST_MEMBERS)
ens.step(2)
out = {}
for k, (mode, coef, kw) in enumerate(G.CALLS):
    cur = G.pre_values(pkg, ens)
    field = G.FIELDS[k % 2]
    ens.inflate(field, coef, mode=mode, members=G.FAST_MEMBERS, **kw)
    for i, m in enumerate(ens.members):
        out["cur%d_%d" % (k, i)] = cur[i][field]
        out["wall%d_%d" % (k, i)] = cur[i]["WALL_CUR"]
        out["post%d_%d" % (k, i)] = m.read_rect(field)
for i, p in enumerate(prior):
    for f in p:
        out["prior_%s_%d" % (f, i)] = p[f]
ens.close()
out["sep"] = G.run_separators(pkg)
np.savez(sys.argv[2], **out)
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernels give what THIS process's host function gives
    on the values the members held (the simulation steps of the two builds differ, the inflation does not). All three modes on stepped
    members, 11 selected (a load group of 8 and a remainder); then the planted separators."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    path = str(tmp_path / "fast.npz")
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, ROOT, path], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    d = np.load(path)
    prior = [{f: d["prior_%s_%d" % (f, i)] for f in (B_, W_, "WALL_CUR")} for i in range(17)]
    for k, (mode, coef, kw) in enumerate(CALLS):
        field = FIELDS[k % 2]
        cur = [{field: d["cur%d_%d" % (k, i)], "WALL_CUR": d["wall%d_%d" % (k, i)]} for i in range(17)]
        want, _ = host(pkg, cur, prior, field, coef, None, FAST_MEMBERS, mode=mode, **kw)
        for i in range(17):
            assert same_bits(d["post%d_%d" % (k, i)], want[i]), (k, mode, i)
        assert not same_bits(d["post%d_0" % k], d["cur%d_0" % k]) and same_bits(d["post%d_9" % k], d["cur%d_9" % k])
    check_separators(d["sep"])


def inflate_caps():
    text = open(os.path.join(ROOT, "2d-weather-sandbox_amd", "csrc", "wx_ens_inflate.h")).read()
    caps = {}
    for name in ("WG", "MAX_WGS", "SAVE_MAX_WGS"):
        caps[name] = int(re.search(r"^enum \{[^}]*?\b%s = (\d+)\b" % name, text, re.M).group(1))
    return caps


@pytest.mark.parametrize("n_sel", [3, 9])
def test_chunk_loop_second_trip(pkg, n_sel):
    """70 x 4200: 8400 (row, chunk) pairs against the 4 x MAX_WGS waves of the capped grid, so the busiest waves take a second trip
    through the chunk loop; tests/ensemble_trip_shapes.py's members, whose planted blocks (walls in some members, non-finite values)
    lie in rows of the first and of the last trip. The snapshot is the uploaded state, the current state that state perturbed on the
    device; all three modes against the host function on every member."""
    caps = inflate_caps()
    Xg, Yg, Bg, _ = T.GRIDS["state"]
    waves = caps["WG"] // 64 * caps["MAX_WGS"]
    cpr = (Xg + 63) // 64
    assert (Xg, Yg) == (70, 4200) and cpr * Yg > waves  # the shape exceeds the cap
    for _, first, last, _ in T.planted_blocks("state"):
        assert first * cpr < waves <= last * cpr  # the planted blocks lie in rows of the first and of the last trip
    members = None if n_sel == 9 else [0, 4, 8]
    m = T.members("state")
    specs = [dict(base=m["base"][i], water=m["water"][i], wall=m["wall"][i], u=I.scene_uniforms("smoke", Yg)) for i in range(Bg)]
    ens = make_ensemble(pkg, specs)
    try:
        prior = [{B_: m["base"][i], "WALL_CUR": m["wall"][i]} for i in range(Bg)]
        ens.save_prior(B_, None, members)
        ens.perturb(B_, (0.05, 0.05, 0.002, 0.5), scale=5, seed=9)
        cur = [{B_: h.read_rect(B_), "WALL_CUR": m["wall"][i]} for i, h in enumerate(ens.members)]
        assert not same_bits(cur[0][B_], prior[0][B_])
        for mode, coef, kw in (("rtps", (0.5, 0.0, 1.0, 0.9), dict(lambda_bounds=(0.8, 1.5))), ("rtpp", 0.5, {}), ("const", (1.25, 1.0, 0.5, 1.5), {})):
            lam = ens.inflate(B_, coef, mode=mode, members=members, want_lambda=mode != "rtpp", **kw)
            new, want_lam = host(pkg, cur, prior, B_, coef, None, members, Xg, Yg, mode=mode, **kw)
            for i, h in enumerate(ens.members):
                got = h.read_rect(B_)
                assert same_bits(got, new[i]), (mode, "member", i, np.argwhere(got.view(np.uint32) != new[i].view(np.uint32))[:4].tolist())
            if want_lam is not None:
                assert same_bits(lam, want_lam), mode
                assert np.isfinite(lam[1:100]).any() and np.isfinite(lam[-100:-1]).any() and np.isnan(lam).any()
            sel = range(Bg) if members is None else members
            for i in sel:  # rows of both trips moved
                ch = new[i].view(np.uint32) != cur[i][B_].view(np.uint32)
                assert ch[:waves // cpr].any() and ch[waves // cpr:].any(), (mode, i)
            cur = [dict(p, **{B_: n}) for p, n in zip(cur, new)]
    finally:
        ens.close()


def test_prior_save_second_trip(pkg):
    """2 x (cap + 64): with two members twice cap + 64 (member, row, chunk) items against the SAVE_MAX_WGS x 4 waves of
    k_ens_prior_save's capped grid. What the snapshot holds is read back through RTPP with alpha = 1: o_k = m + b_k on every row."""
    caps = inflate_caps()
    cap = caps["WG"] // 64 * caps["SAVE_MAX_WGS"]
    Xg, Yg = 2, cap + 64
    assert 2 * Yg > cap and Yg <= 65535
    rng = np.random.Generator(np.random.Philox(5))
    u = I.scene_uniforms("smoke", Yg)
    wall = np.zeros((Yg, Xg, 4), np.int8)
    wall[1:, :, 1] = 3
    mk = lambda: (rng.normal(0, 1, (Yg, Xg, 4)) * np.array([0.1, 0.1, 0.01, 2.0]) + np.array([0, 0, 0, 300.0])).astype(np.float32)  # noqa: E731
    prior, cur = [mk(), mk()], [mk(), mk()]
    water = np.zeros((Yg, Xg, 4), np.float32)
    ens = make_ensemble(pkg, [dict(base=p, water=water, wall=wall, u=u) for p in prior])
    try:
        ens.save_prior(B_)
        for h, c in zip(ens.members, cur):
            h.upload(c, water, wall)
        ens.inflate(B_, 1.0, mode="rtpp")
        want = pkg.engine.ens_inflate_cells(cur, [wall, wall], B_, 1.0, mode="rtpp", priors=prior)
        for i, h in enumerate(ens.members):
            got = h.read_rect(B_)
            assert same_bits(got, want[i]), (i, np.argwhere(got.view(np.uint32) != want[i].view(np.uint32))[:4].tolist())
            assert not same_bits(got[1:cap // 2], cur[i][1:cap // 2]) and not same_bits(got[cap:], cur[i][cap:]) and same_bits(got[0], cur[i][0])
    finally:
        ens.close()


def test_snapshot_rules_and_refusals(pkg):
    """The refusals of include/wxsim.h answer before anything is written, each with its code and, for the snapshot, a message that says
    which rule it was; a second save replaces the first; the ensemble then works as before."""
    E = pkg.engine
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 4)[:3] + [None])  # member 3 is never uploaded
    sel = [0, 1, 2]
    try:
        keep = [ens[i].read_rect(f) for i in sel for f in FIELDS]

        def refused(code, call=None, **kw):
            with pytest.raises(E.WxError) as ei:
                if call is None:
                    ens.inflate(kw.pop("field", B_), kw.pop("coef", 1.5), **{"members": sel, **kw})
                else:
                    call()
            assert ei.value.code == code, (kw, str(ei.value))
            return str(ei.value)

        # WX_E_INVALID
        refused(-1, field="CURL"), refused(-1, field="BASE_DISP"), refused(-1, mode=3), refused(-1, mode=-1)
        refused(-1, coef=(1, NAN, 1, 1)), refused(-1, coef=float("inf")), refused(-1, coef=(1, 1, -0.5, 1))
        refused(-1, mode="rtpp", coef=1.5), refused(-1, mode="rtpp", coef=0.5, want_lambda=True)
        refused(-1, members=[1]), refused(-1, members=[])
        refused(-1, lambda: ens.save_prior("CURL")), refused(-1, lambda: ens.save_prior(B_, None, [])), refused(-1, lambda: ens.drop_prior("LIGHT_0"))
        # WX_E_RANGE
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, 0, 0, 1), (X, 0, 1, 1)):
            refused(-4, rect=rect)
            refused(-4, lambda: ens.save_prior(B_, rect, sel))
        # WX_E_STATE: a member that was never uploaded
        assert "member 3" in refused(-5, members=None) and "member 3" in refused(-5, members=[1, 3])
        assert "member 3" in refused(-5, lambda: ens.save_prior(B_)) and "member 3" in refused(-5, lambda: ens.save_prior(W_, None, [3]))
        # WX_E_STATE: the snapshot
        for mode in ("rtps", "rtpp"):
            assert "no snapshot" in refused(-5, mode=mode, coef=0.5)
        ens.drop_prior(B_)  # nothing to drop: fine
        ens.save_prior(B_, (10, 5, 40, 20), sel)
        assert "no snapshot" in refused(-5, mode="rtps", coef=0.5, field=W_, rect=(12, 6, 8, 8))  # one slot per field
        for rect in (None, (9, 5, 4, 4), (10, 4, 4, 4), (47, 5, 4, 4), (10, 22, 4, 4)):
            assert "not inside" in refused(-5, mode="rtps", coef=0.5, rect=rect), rect
        assert "selection" in refused(-5, mode="rtpp", coef=0.5, rect=(10, 5, 40, 20), members=[0, 1])
        assert "selection" in refused(-5, mode="rtps", coef=0.5, rect=(10, 5, 40, 20), members=[0, 2])
        now = [ens[i].read_rect(f) for i in sel for f in FIELDS]
        assert all(same_bits(a, b) for a, b in zip(now, keep))  # a refused call writes nothing
        # CONST never looks at a snapshot; the relaxation modes accept the snapshot's rectangle and any rectangle inside it
        walls = [ens[i].read_rect("WALL_CUR") for i in sel]
        prior = [{B_: keep[2 * i], "WALL_CUR": walls[i]} for i in sel]  # (the snapshot was taken of the uploaded state)
        ens.perturb(B_, (0.05, 0.05, 0.002, 0.5), scale=4, seed=2, members=sel)
        cur = [{B_: ens[i].read_rect(B_), "WALL_CUR": walls[i]} for i in sel]
        assert not same_bits(cur[0][B_], prior[0][B_])
        for mode, coef, rect in (("rtps", 0.5, (10, 5, 40, 20)), ("rtpp", 0.5, (49, 24, 1, 1)), ("const", 1.5, None)):
            ens.inflate(B_, coef, mode=mode, rect=rect, members=sel)
            new, _ = host(pkg, cur, prior, B_, coef, rect, None, mode=mode)
            cur = [dict(p, **{B_: n}) for p, n in zip(cur, new)]
            assert all(same_bits(ens[i].read_rect(B_), cur[i][B_]) for i in sel), mode
        # a second save replaces the first: the prior is now the current state, RTPS finds sb == sa and changes nothing
        ens.save_prior(B_, None, sel)
        lam = ens.inflate(B_, 0.5, mode="rtps", members=sel, want_lambda=True)
        assert np.isnan(lam).all() and all(same_bits(ens[i].read_rect(B_), cur[i][B_]) for i in sel)
        ens.drop_prior(B_)
        assert "no snapshot" in refused(-5, mode="rtps", coef=0.5)
        ens.drop_prior(B_), ens.drop_prior(W_)
    finally:
        ens.close()


def test_display_side_fields_survive_and_the_call_is_ordered_behind_a_pending_step(pkg):
    """After a step whose last iteration was a display iteration (WATER_0 pending, BASE_DISP lazy) both fields are inflated, with no sync
    between the step and the calls: the values are those of the stepped state (the host function of the values a twin ensemble holds),
    and WATER_0, BASE_DISP, CURL and the rest of the display side read what an untouched clone of the twin reads."""
    specs = member_specs(pkg, X, Y, 3)
    ens, twin = make_ensemble(pkg, specs), make_ensemble(pkg, specs)
    clone = pkg.engine.Handle(X, Y)
    try:
        twin.step(2)
        prior = pre_values(pkg, twin)
        twin.step(4)
        cur = pre_values(pkg, twin)
        clone.copy_from(twin[1])
        ens.step(2)
        ens.save_prior(B_), ens.save_prior(W_)  # (directly behind the step)
        ens.step(4)
        ens.inflate(B_, 0.7, mode="rtps")  # (directly behind the step)
        ens.inflate(W_, 0.5, mode="rtpp", lo=0.0)
        for field, coef, kw in ((B_, 0.7, dict(mode="rtps")), (W_, 0.5, dict(mode="rtpp", lo=0.0))):
            new, _ = host(pkg, cur, prior, field, coef, None, None, **kw)
            for i, m in enumerate(ens.members):
                assert same_bits(m.read_rect(field), new[i]), (field, i)
        for f in ("WATER_0", "BASE_DISP", "CURL", "WALL_DISP", "LIGHT_0", "LIGHT_1"):
            assert same_bits(ens[1].read_rect(f), clone.read_rect(f)), f
        assert not same_bits(ens[1].read_rect(B_), clone.read_rect(B_)) and not same_bits(ens[1].read_rect(W_), clone.read_rect(W_))
        ens.step(1)
        ens.sync()
    finally:
        ens.close(), twin.close()
        clone.close()


def test_a_water_update_ends_the_water_free_state(pkg):
    specs = []
    for i in range(2):
        b, w, wl = I.impulse_scene(X, Y, "fast_vx", offset=(i, 1 + i), seed=50 + i)[:3]
        specs.append(dict(base=b, water=w, wall=wl, u=I.scene_uniforms("fast_vx", Y, dry=True)))
    ens = make_ensemble(pkg, specs)
    try:
        assert ens[0].water_free() and ens[1].water_free()
        ens.save_prior(B_), ens.save_prior(W_)  # a snapshot changes nothing
        assert ens[0].water_free() and ens[1].water_free()
        ens.inflate(B_, 1.5)  # base only: the water is still known to be trivial
        ens.inflate(B_, 0.5, mode="rtps")
        assert ens[0].water_free() and ens[1].water_free()
        ens.inflate(W_, 1.5)
        assert not ens[0].water_free() and not ens[1].water_free()
        ens.step(2)
        ens.sync()
    finally:
        ens.close()


def test_an_overflowed_list_surfaces_here(pkg):
    """WX_OPT_FIX_CAP 2 on a member with fast cells: its report (WX_E_STATE) is what the call returns, naming the member -- once."""
    E = pkg.engine
    Xb, Yb = 505, 77  # (the shape at which tests/test_ensemble_statistics_gpu.py overflows the list)
    fast = I.impulse_scene(Xb, Yb, "fast_vx")
    specs = member_specs(pkg, Xb, Yb, 3)
    specs[1] = dict(base=fast[0], water=fast[1], wall=fast[2], u=I.scene_uniforms("fast_vx", Yb), options={E.Handle.OPT_FIX_CAP: 2})
    ens = make_ensemble(pkg, specs)
    try:
        ens.step(2)
        with pytest.raises(E.WxError) as ei:
            ens.inflate(B_, 1.25)
        assert ei.value.code == -5 and "member 1: " in str(ei.value), str(ei.value)
        ens.inflate(B_, 1.25)  # the report was consumed
    finally:
        ens.close()


def test_the_profile_names_both_kernels(pkg):
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 3))
    try:
        ens[0].profile(True)
        ens.save_prior(B_, None, [1, 2])  # (member 0 times the launches, whoever is selected)
        prof = ens[0].profile_read()
        assert prof["ensemble_prior_save"][1] == 1 and prof["ensemble_prior_save"][0] > 0 and "ensemble_inflate" not in prof
        for mode, coef in (("const", 1.5), ("rtps", 0.5), ("rtpp", 0.5)):
            ens[0].profile(True)
            ens.inflate(B_, coef, mode=mode, members=[1, 2])
            prof = ens[0].profile_read()
            assert prof["ensemble_inflate"][1] == 1 and prof["ensemble_inflate"][0] > 0 and "ensemble_prior_save" not in prof, (mode, prof)
    finally:
        ens.close()


def test_an_inflated_member_and_its_clone_step_to_the_same_bits(pkg):
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 3))
    lone = pkg.engine.Handle(X, Y)
    try:
        ens.step(3)
        ens.save_prior(B_), ens.save_prior(W_)
        ens.step(2)
        ens.inflate(B_, 0.6, mode="rtps"), ens.inflate(W_, (1.5, 1.5, 1.0, 1.25), lo=0.0)
        lone.copy_from(ens[1])
        ens.step(3)
        lone.step(3)
        for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "LIGHT_1"):
            assert same_bits(ens[1].read_rect(f), lone.read_rect(f)), f
    finally:
        ens.close()
        lone.close()


def test_workflow_from_sim_perturb_step_analysis_statistics(pkg):
    """WeatherEnsemble.from_sim of a stepped WeatherSim, perturb, step, analysis(relax=("rtps", 1)) of the temperatures a lone nature
    run shows at five stations, statistics: with alpha = 1 and no lambda bounds the analysis is handed back the prior's spread, so the
    variance plane after the analysis equals the one taken just before it wherever the prior variance is non-zero and the cell is an air
    cell in all members.

    THE BOUND, derived here from the members' magnitudes. In real numbers the posterior deviations D_k = lambda d_k have sum 0 and
    sum of squares Qb (lambda = sb / sa); the double arithmetic of the definition changes that by a relative u = 64 eps64 at most (a
    handful of operations each). Every member value o_k is ONE double -> float32 rounding of m + D_k: |o_k - (m + D_k)| <= e with
    e = half the largest float32 spacing among the o_k plus u times the largest magnitude. The deviations of the o_k about their own
    mean then differ from D_k by at most 2 e, so |Q_post - Qb| <= sum 2 e (2 |dev_k| + 2 e) + u Qb. Both variance planes are Q / n
    rounded to float32 once: half a float32 spacing each on top."""
    W = pkg.sim
    Xw, Yw, Bw = 128, 48, 6
    base, water, wall = pkg.synth.terrain_grid(Xw, Yw)
    sim = W.WeatherSim(Xw, Yw, base, water, wall, None, {"dayNightCycle": False}, sun_angle_deg=30.0)
    sim.verbose = False
    we = None
    try:
        sim.step(6)
        we = W.WeatherEnsemble.from_sim(sim, Bw)
        we.perturb(B_, (0.0, 0.0, 0.0, 0.5), scale=8, seed=3)
        we.step(2)
        sim.step(2)
        truth, air = sim.read_rect(B_), we[0].read_rect("WALL_CUR")[..., 1] != 0
        cols = (10, 35, 60, 85, 110)
        rows = [y for y in range(12, Yw - 6) if all(air[y, x] for x in cols)]
        assert rows, air.sum(axis=0)[list(cols)].tolist()
        y0 = rows[-1]
        obs = [(B_, x, y0, 3, float(truth[y0, x, 3]), 0.01) for x in cols]
        before = we.statistics(B_, want=("mean", "variance", "n_wall"))
        plain = [m.read_rect(B_) for m in we.members]
        res = we.analysis(obs, relax=("rtps", 1.0), loc=(10.0, 3.0))
        after = we.statistics(B_, want=("mean", "variance"))
        assert all(r["applied"] for r in res)
        post = np.stack([np.float64(m.read_rect(B_)[..., 3]) for m in we.members])
        assert any(not same_bits(m.read_rect(B_), p) for m, p in zip(we.members, plain))
        assert all(same_bits(m.read_rect(B_)[..., :3], p[..., :3]) for m, p in zip(we.members, plain))  # temperature only by default
        vb, va = np.float64(before["variance"][..., 3]), np.float64(after["variance"][..., 3])
        ok = (before["n_wall"] == 0) & (vb > 0) & np.isfinite(post).all(axis=0)
        assert ok.sum() > Xw * Yw // 2
        eps = np.finfo(np.float64).eps
        e = 0.5 * np.max(np.float64(np.spacing(np.float32(np.abs(post)))), axis=0) + 64 * eps * np.max(np.abs(post), axis=0)
        dev = post - post.mean(axis=0)
        bound = (np.sum(2 * e * (2 * np.abs(dev) + 2 * e), axis=0) + 64 * eps * vb * Bw) / Bw
        bound = bound + 0.5 * np.float64(np.spacing(np.float32(vb))) + 0.5 * np.float64(np.spacing(np.float32(va)))
        assert (np.abs(va - vb)[ok] <= bound[ok]).all(), (float(np.max((np.abs(va - vb) / bound)[ok])), np.argwhere(ok & (np.abs(va - vb) > bound))[:4].tolist())
        # ... and the analysis did pull the members: at the stations the mean moved towards the truth
        for x in cols:
            assert abs(float(after["mean"][y0, x, 3]) - float(truth[y0, x, 3])) < abs(float(before["mean"][y0, x, 3]) - float(truth[y0, x, 3])) or abs(res[cols.index(x)]["innovation"]) < 1e-3
        we.step(1)
        we.sync()
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
