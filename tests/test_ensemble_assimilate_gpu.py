"""wx_ensemble_assimilate on the GPU: after every call the members' BASE_CUR and WATER_CUR equal wx_ens_assim_cells -- the serial
definition on the CPU, which tests/test_ensemble_assimilate_cpu.py pins to the text of include/wxsim.h -- of the values they held
before, read through a device-side clone, and the per-observation results (computed on the device: its double division and square root)
equal the host's; one call of 40 observations equals 40 calls of one; the tolerance build gives the same bits; the display-side fields
and the bookkeeping survive; and the workflow clone -> perturb -> step -> assimilate against a nature run -> statistics. Every
comparison is `==` on bits (NaNs compared as positions)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import impulse_scenes as I
from test_ensemble_assimilate_cpu import PLANTED, PLANTED_IDS, SEPARATOR_KW, SEPARATORS, plant_separators, separator_cell
from test_ensemble_gpu import same_bits
from test_ensemble_perturb_gpu import pre_values
from test_ensemble_statistics_gpu import make_ensemble, member_specs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
X, Y = 130, 40
B_, W_ = "BASE_CUR", "WATER_CUR"
# as MASKS of tests/test_ensemble_perturb_gpu.py, with at least two members selected (17: three, and sixteen = two full load groups)
MASKS = {2: [None], 3: [None, [0, 2]], 17: [None, [0, 3, 16], list(range(1, 17))]}
RES_KEYS = ("prior_mean", "prior_var", "innovation", "alpha")


def same_results(a, b):
    return len(a) == len(b) and all(p["applied"] == q["applied"] and all(np.float64(p[k]).view(np.uint64) == np.float64(q[k]).view(np.uint64) or (p[k] != p[k] and q[k] != q[k]) for k in RES_KEYS)
                                    for p, q in zip(a, b))


def air_in_all(pre, members=None):
    sel = range(len(pre)) if members is None else members
    return np.all([pre[i]["WALL_CUR"][..., 1] != 0 for i in sel], axis=0)


def observations(pre, rng, n, *, inside=None, members=None, extra=()):
    """n observations at random cells that are air cells in every selected member (``inside``: of that rectangle), temperature (BASE
    channel 3) and water (WATER channel 0) in turn, each value the members' mean moved by about one spread; then ``extra``."""
    sel = list(range(len(pre))) if members is None else members
    ok = air_in_all(pre, sel)
    if inside is not None:
        x, y, w, h = inside
        m = np.zeros_like(ok)
        m[y:y + h, x:x + w] = True
        ok &= m
    ys, xs = np.nonzero(ok)
    out = []
    for j in range(n):
        k = int(rng.integers(0, len(xs)))
        out.append(obs_at(pre, sel, (B_, 3) if j % 2 == 0 else (W_, 0), int(xs[k]), int(ys[k]), rng))
    return out + list(extra)


def obs_at(pre, sel, what, x, y, rng):
    field, c = what
    v = np.array([float(pre[i][field][y, x, c]) for i in sel])
    v = v[np.isfinite(v)]
    mean, sd = (float(v.mean()), float(v.std())) if len(v) else (0.0, 0.0)
    sd = max(sd, 1e-3 * abs(mean), 1e-6)
    return (field, x, y, c, mean + sd * float(rng.normal()), max(float(np.float32(0.5 * sd * sd)), 1e-30))


def host(pkg, pre, obs, **kw):
    """wx_ens_assim_cells of ``pre`` (one dict per member): what the members should hold now, and the results."""
    nb, nw, res = pkg.engine.ens_assim_cells([p[B_] for p in pre], [p[W_] for p in pre], [p["WALL_CUR"] for p in pre], X, Y, obs, **kw)
    return [{B_: b, W_: w, "WALL_CUR": p["WALL_CUR"]} for b, w, p in zip(nb, nw, pre)], res


def planted_geometry(pre, rng, rect):
    """The planted cases of the CPU test as far as they are geometry: an observation in a cell that is a wall in some member only, at
    x = 0 and x = X - 1 (wrap), twice the same cell and channel, outside the rectangle."""
    sel = list(range(len(pre)))
    walls = np.stack([p["WALL_CUR"][..., 1] == 0 for p in pre])
    some = walls.any(axis=0) & ~walls.all(axis=0)
    ok = air_in_all(pre)
    out = []
    if some.any():
        ys, xs = np.nonzero(some)
        out.append(obs_at(pre, sel, (B_, 3), int(xs[0]), int(ys[0]), rng))
    for x in (0, X - 1):
        ys = np.nonzero(ok[:, x])[0]
        out.append(obs_at(pre, sel, (B_, 3), x, int(ys[len(ys) // 2]), rng))
    ys, xs = np.nonzero(ok[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]])
    x, y = int(xs[len(xs) // 2]) + rect[0], int(ys[len(xs) // 2]) + rect[1]
    out += [obs_at(pre, sel, (B_, 3), x, y, rng), obs_at(pre, sel, (B_, 3), x, y, rng), obs_at(pre, sel, (W_, 0), x, y, rng)]
    m = ok.copy()
    m[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = False
    ys, xs = np.nonzero(m)
    k = np.argmin(np.abs(xs - rect[0]) + np.abs(ys - rect[1]))  # outside the rectangle, next to it
    out.append(obs_at(pre, sel, (B_, 3), int(xs[k]), int(ys[k]), rng))
    return out, bool(some.any())


@pytest.mark.parametrize("B", [2, 3, 17])
def test_device_equals_host_function(pkg, B):
    """Members on different terrain, stepped twice; then a sequence of calls -- observations of both fields updating both fields, the
    whole grid and three rectangles, masks, the planted geometry, 1, 2 and 40 observations -- each compared on every member against the
    host function of the values before, results included."""
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, B))
    try:
        ens.step(2)
        pre = pre_values(pkg, ens)
        assert len({p["WALL_CUR"].tobytes() for p in pre}) > 1  # different terrain
        rng = np.random.Generator(np.random.Philox(40 + B))
        plant_rect = (7, 2, 63, 9)
        planted, has_wall_obs = planted_geometry(pre, rng, plant_rect)
        both = dict(gain_base=(0.5, 0, 0, 1), gain_water=(1, 0.5, 0, 0.25), lo_water=0.0)
        calls = [
            (40, None, dict(loc=(12.0, 6.0), wrap_x=True, **both), ()),
            (1, (3, 5, 1, 7), dict(loc=(0.0, 3.0), gain_base=1.0, gain_water=1.0), ()),
            (2, plant_rect, dict(loc=(20.0, 0.0), wrap_x=False, **both), ()),
            (40, (65, 1, 65, 30), dict(loc=(9.0, 5.0), wrap_x=False, gain_base=(1, 1, 0, 0), gain_water=(1, 0, 0, 1), hi_base=(0.05, NAN, NAN, NAN)), ()),
            (3, plant_rect, dict(loc=(40.0, 4.0), wrap_x=True, **both), planted),
            (2, None, dict(loc=(0.0, 0.0), gain_base=(0, 0, 0, 1)), ()),
            (40, None, dict(loc=(6.0, 3.0), wrap_x=True, gain_base=0.0, gain_water=0.0), ()),  # all gains 0: results only
        ]
        changed = {B_: False, W_: False}
        applied = skipped = 0
        for k, (n, rect, kw, extra) in enumerate(calls):
            members = None if k == 4 else MASKS[B][k % len(MASKS[B])]  # (the planted geometry is planted for all members)
            obs = observations(pre, rng, n, inside=rect if k in (1, 2) else None, members=members, extra=extra)
            before = pre
            got_res = ens.assimilate(obs, rect=rect, members=members, **kw)
            pre, want_res = host(pkg, before, obs, rect=rect, members=members, **kw)
            assert same_results(got_res, want_res), (k, [(a, b) for a, b in zip(got_res, want_res) if not same_results([a], [b])][:2])
            applied, skipped = applied + sum(r["applied"] for r in got_res), skipped + sum(not r["applied"] for r in got_res)
            for i, m in enumerate(ens.members):
                for f in (B_, W_):
                    got = m.read_rect(f)
                    assert same_bits(got, pre[i][f]), (k, f, rect, kw, "member", i, np.argwhere(got.view(np.uint32) != pre[i][f].view(np.uint32))[:4].tolist())
                    if members is not None and i not in members:
                        assert same_bits(got, before[i][f]), (k, f, "unselected member", i)
                    wall_cells = pre[i]["WALL_CUR"][..., 1] == 0
                    assert wall_cells.any() and same_bits(got[wall_cells], before[i][f][wall_cells]), (k, f, "wall cells of member", i)
                    if k == len(calls) - 1:
                        assert same_bits(got, before[i][f]), (k, f, "all gains 0")
                    changed[f] = changed[f] or not same_bits(got, before[i][f])
        assert changed[B_] and changed[W_] and applied > 80 and (skipped > 0 or not has_wall_obs)
        for i, m in enumerate(ens.members):
            assert same_bits(m.read_rect("WALL_CUR"), pre[i]["WALL_CUR"])
        ens.step(1)  # ... and the ensemble steps on
        ens.sync()
    finally:
        ens.close()


def dense_observations(pre, rng, n=40):
    """n observations crowded into a few cells' neighbourhood: overlapping footprints, repeated cells, both fields."""
    ok = air_in_all(pre)
    ys, xs = np.nonzero(ok[10:22, 30:60])
    sel = list(range(len(pre)))
    out = []
    for j in range(n):
        k = int(rng.integers(0, min(len(xs), 25)))
        out.append(obs_at(pre, sel, (B_, 3) if j % 3 else (W_, 0), int(xs[k]) + 30, int(ys[k]) + 10, rng))
    return out


def test_one_call_of_40_observations_equals_40_calls_of_one(pkg):
    """Bit for bit, on the device: the pre-pass's working copies of the observed channels must stay what the state's cells hold."""
    specs = member_specs(pkg, X, Y, 3)
    one, many = make_ensemble(pkg, specs), make_ensemble(pkg, specs)
    try:
        one.step(2), many.step(2)
        pre = pre_values(pkg, one)
        obs = dense_observations(pre, np.random.Generator(np.random.Philox(5)))
        assert len({(o[0], o[1], o[2], o[3]) for o in obs}) < len(obs)  # repeated cells and channels
        kw = dict(loc=(10.0, 5.0), wrap_x=True, gain_base=(0.5, 0, 0, 1), gain_water=(1, 0, 0, 0.5), lo_water=0.0, rect=(5, 1, 120, 38))
        r_one = one.assimilate(obs, **kw)
        r_many = []
        for o in obs:
            r_many += many.assimilate([o], **kw)
        assert same_results(r_one, r_many) and sum(r["applied"] for r in r_one) == len(obs)
        for a, b, p in zip(one.members, many.members, pre):
            for f in (B_, W_):
                assert same_bits(a.read_rect(f), b.read_rect(f)), f
                assert not same_bits(a.read_rect(f), p[f]), f
    finally:
        one.close(), many.close()


@pytest.mark.parametrize("n_obs", [234, 235, 256])
def test_working_copies_in_lds_and_in_the_table(pkg, n_obs):
    """70 members: 234 observations are the most whose working copies fit the pre-pass's 64 KiB of LDS (234 x 70 x 4 B = 65520), from
    235 on they live in the observation table in global memory. Both sides of the threshold and WX_ENS_OBS_MAX, against the host function."""
    B = 70
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, B))
    try:
        ens.step(2)
        pre = pre_values(pkg, ens)
        obs = observations(pre, np.random.Generator(np.random.Philox(n_obs)), n_obs, inside=(20, 8, 40, 12))  # crowded: every cell observed many times
        kw = dict(loc=(3.0, 2.0), gain_base=(0, 0, 0, 1), gain_water=(1, 0, 0, 0), rect=(10, 4, 60, 20))
        res = ens.assimilate(obs, **kw)
        want, want_res = host(pkg, pre, obs, **kw)
        assert same_results(res, want_res) and sum(r["applied"] for r in res) == n_obs
        for i, m in enumerate(ens.members):
            assert same_bits(m.read_rect(B_), want[i][B_]) and same_bits(m.read_rect(W_), want[i][W_]), i
        assert not same_bits(want[0][B_], pre[0][B_]) and not same_bits(want[69][W_], pre[69][W_])
    finally:
        ens.close()


def separator_specs(pkg):
    """Three members (uploaded, not stepped) with tools/find_assimilate_separators.py's values planted, and the observations."""
    specs = member_specs(pkg, X, Y, 3)
    for s in specs:
        s["base"], s["wall"] = np.array(s["base"], np.float32), np.array(s["wall"], np.int8)
    obs = plant_separators([s["base"] for s in specs], [s["wall"] for s in specs])
    return specs, obs


def check_separators(pkg, specs, obs, got_base0, res):
    pre = [{B_: s["base"], W_: np.asarray(s["water"], np.float32), "WALL_CUR": s["wall"]} for s in specs]
    want, want_res = host(pkg, pre, obs, **SEPARATOR_KW)
    assert same_results(res, want_res) and all(r["applied"] for r in res)
    assert same_bits(got_base0, want[0][B_])
    for i, (_, _, _, _, defined, fused) in enumerate(SEPARATORS):
        x, y = separator_cell(i)
        assert int(got_base0[y, x, 3].view(np.uint32)) == defined != fused, i


def test_planted_separators_on_the_device(pkg):
    """Member values on which a fused d_k*e_k or b*e_k changes a float32 result: the device gives the defined bits."""
    specs, obs = separator_specs(pkg)
    ens = make_ensemble(pkg, specs)
    try:
        res = ens.assimilate(obs, **SEPARATOR_KW)
        check_separators(pkg, specs, obs, ens[0].read_rect(B_), res)
    finally:
        ens.close()


def device_run(pkg):
    """`run` of the planted cases of tests/test_ensemble_assimilate_cpu.py on the device: the arrays are uploaded as they are (nothing
    is stepped), the call is made, what the members hold then and the results equal the host function's bit for bit, and the device's
    arrays go back to the case's value-level assertions."""
    E, P = pkg.engine, pkg.params

    def run(bases, waters, walls, Xp, Yp, obs, where, **kw):
        u = P.uniforms_from_gui(P.merge_settings(None), Yp)
        ens = E.Ensemble(len(bases), Xp, Yp, 0)
        try:
            for m, b, w, wl in zip(ens.members, bases, waters, walls):
                m.upload(b, w, wl)
                m.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
                assert b.view(np.uint32).tobytes() == m.read_rect(B_).view(np.uint32).tobytes(), where  # the planted bits are on the device
            res = ens.assimilate(obs, **kw)
            want_b, want_w, want_res = E.ens_assim_cells(bases, waters, walls, Xp, Yp, obs, **kw)
            assert same_results(res, want_res), (where, res, want_res)
            got_b, got_w = [m.read_rect(B_) for m in ens.members], [m.read_rect(W_) for m in ens.members]
            for i in range(len(bases)):
                for f, got, want in ((B_, got_b[i], want_b[i]), (W_, got_w[i], want_w[i])):
                    assert same_bits(got, want), (where, f, "member", i, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
            return got_b, got_w, res
        finally:
            ens.close()

    return run


@pytest.mark.parametrize("B", [5, 9])
@pytest.mark.parametrize("case,placements", PLANTED, ids=PLANTED_IDS)
def test_planted_cases_through_the_entry_test_and_the_member_walks_of_the_kernels(pkg, case, placements, B):
    """The planted cases of the CPU test through k_ens_assim_obs and k_ens_assim on 17 x 7: non-finite and wall observations skipped,
    a NaN and a wall in one member's state cell (the entry test ok[c] of the member walk -- with B = 9 once inside the load group of 8,
    once in the remainder member behind it; B = 5 walks the remainder loop alone), V = 0 and the sign of zero, gain 0, the clamp edges,
    the result beyond FLT_MAX that keeps its bits, localization at exactly dx == loc and dx == 2 loc, the wrap, duplicates."""
    for kw in placements if B == 9 else placements[:1]:
        case(device_run(pkg), B=B, **kw)


_FAST_LEG = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_assimilate_gpu as T
ens = T.make_ensemble(pkg, T.member_specs(pkg, T.X, T.Y, 17))
ens.step(2)
pre = T.pre_values(pkg, ens)
np.savez(sys.argv[2] + "_pre", **{f"{f}{i}": p[f] for i, p in enumerate(pre) for f in p})
obs = T.dense_observations(pre, np.random.Generator(np.random.Philox(6))) + T.observations(pre, np.random.Generator(np.random.Philox(7)), 40)
res = ens.assimilate(obs, **T.FAST_KW)
np.savez(sys.argv[2] + "_post", **{f"{f}{i}": m.read_rect(f) for i, m in enumerate(ens.members) for f in ("BASE_CUR", "WATER_CUR")})
ens.close()
specs, sobs = T.separator_specs(pkg)
ens = T.make_ensemble(pkg, specs)
sres = ens.assimilate(sobs, **T.SEPARATOR_KW)
np.save(sys.argv[2] + "_sep.npy", ens[0].read_rect("BASE_CUR"))
ens.close()
bits = lambda rs: [[r["applied"]] + [np.float64(r[k]).view(np.uint64).item() for k in T.RES_KEYS] for r in rs]
json.dump({"obs": obs, "res": bits(res), "sres": bits(sres)}, open(sys.argv[2] + ".json", "w"))
"""
FAST_KW = dict(loc=(10.0, 5.0), wrap_x=True, gain_base=(0.5, 0, 0, 1), gain_water=(1, 0, 0, 0.5), lo_water=0.0, members=[0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 16])


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernels give what THIS process's host function gives
    on the values the members held (the simulation steps of the two builds differ, the assimilation does not). 80 observations on
    stepped members, 11 selected (a load group of 8 and a remainder); then the planted separators: member values on which a fused
    d_k*e_k or b*e_k changes a float32 result (tools/find_assimilate_separators.py)."""
    import json
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    stem = str(tmp_path / "fast")
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, ROOT, stem], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    a, b, j = np.load(stem + "_pre.npz"), np.load(stem + "_post.npz"), json.load(open(stem + ".json"))
    pre = [{f: a[f"{f}{i}"] for f in (B_, W_, "WALL_CUR")} for i in range(17)]
    obs = [tuple(o) for o in j["obs"]]
    want, want_res = host(pkg, pre, obs, **FAST_KW)
    for i in range(17):
        for f in (B_, W_):
            assert same_bits(b[f"{f}{i}"], want[i][f]), (i, f)
    assert not same_bits(b[f"{B_}0"], a[f"{B_}0"]) and same_bits(b[f"{B_}9"], a[f"{B_}9"])
    got_res = [dict(applied=bool(r[0]), **{k: float(np.uint64(v).view(np.float64)) for k, v in zip(RES_KEYS, r[1:])}) for r in j["res"]]
    assert same_results(got_res, want_res) and sum(r["applied"] for r in got_res) > 60
    unbits = lambda rs: [dict(applied=bool(r[0]), **{k: float(np.uint64(v).view(np.float64)) for k, v in zip(RES_KEYS, r[1:])}) for r in rs]  # noqa: E731
    specs, sobs = separator_specs(pkg)
    check_separators(pkg, specs, sobs, np.load(stem + "_sep.npy"), unbits(j["sres"]))


def test_refusals(pkg):
    """The refusals of include/wxsim.h answer before anything is written; the ensemble then works as before."""
    E = pkg.engine
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 3)[:2] + [None])  # member 2 is never uploaded
    try:
        keep = [ens[i].read_rect(f) for i in (0, 1) for f in (B_, W_)]
        good = [(B_, 20, 20, 3, 300.0, 0.25)]

        def refused(code, obs=good, **kw):
            with pytest.raises(E.WxError) as ei:
                ens.assimilate(obs, **{"members": [0, 1], **kw})
            assert ei.value.code == code, (obs, kw, str(ei.value))
            return str(ei.value)

        refused(-1, obs=[])
        refused(-1, obs=good * 257)
        for bad in (("CURL", 20, 20, 0, 1.0, 0.25), (B_, 20, 20, 4, 1.0, 0.25), (B_, 20, 20, 3, NAN, 0.25), (B_, 20, 20, 3, 1.0, 0.0), (B_, 20, 20, 3, 1.0, float("inf"))):
            refused(-1, obs=good + [bad])
        refused(-1, loc=(-1.0, 0.0)), refused(-1, loc=(0.0, NAN)), refused(-1, gain_base=(0, NAN, 0, 1)), refused(-1, gain_water=float("inf"))
        refused(-1, members=[1]), refused(-1, members=[])
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, 0, 0, 1), (X, 0, 1, 1)):
            refused(-4, rect=rect)
        refused(-4, obs=good + [(B_, X, 20, 3, 300.0, 0.25)]), refused(-4, obs=[(W_, 5, -1, 0, 0.01, 0.25)])
        assert "member 2" in refused(-5, members=None)
        assert "member 2" in refused(-5, members=[1, 2])
        now = [ens[i].read_rect(f) for i in (0, 1) for f in (B_, W_)]
        assert all(same_bits(a, b) for a, b in zip(now, keep))
        pre = [{B_: keep[0], W_: keep[1], "WALL_CUR": ens[0].read_rect("WALL_CUR")}, {B_: keep[2], W_: keep[3], "WALL_CUR": ens[1].read_rect("WALL_CUR")}]
        obs = observations(pre, np.random.Generator(np.random.Philox(1)), 4)
        res = ens.assimilate(obs, members=[0, 1], loc=(8.0, 4.0))
        assert all(r["applied"] for r in res) and not same_bits(ens[0].read_rect(B_), keep[0])
    finally:
        ens.close()


def test_display_side_fields_survive_and_the_call_is_ordered_behind_a_pending_step(pkg):
    """After a step whose last iteration was a display iteration (WATER_0 pending, BASE_DISP lazy) both fields are updated, with no sync
    between the step and the call: the priors are those of the stepped state (the host function of the values an untouched clone of a
    twin ensemble reads), and WATER_0, BASE_DISP, CURL and the rest of the display side read what that clone reads."""
    specs = member_specs(pkg, X, Y, 3)
    ens, twin = make_ensemble(pkg, specs), make_ensemble(pkg, specs)
    clone = pkg.engine.Handle(X, Y)
    try:
        twin.step(4)
        pre = pre_values(pkg, twin)
        clone.copy_from(twin[1])
        obs = observations(pre, np.random.Generator(np.random.Philox(2)), 6)
        kw = dict(loc=(15.0, 6.0), gain_base=(1, 0, 0, 1), gain_water=(1, 0, 0, 1), lo_water=0.0)
        ens.step(4)
        res = ens.assimilate(obs, **kw)  # (directly behind the step)
        want, want_res = host(pkg, pre, obs, **kw)
        assert same_results(res, want_res) and all(r["applied"] for r in res)
        for i, m in enumerate(ens.members):
            assert same_bits(m.read_rect(B_), want[i][B_]) and same_bits(m.read_rect(W_), want[i][W_]), i
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
        ens.assimilate([(B_, 20, 20, 3, 300.0, 0.25)], gain_base=(0, 0, 0, 1))  # base only: the water is still known to be trivial
        assert ens[0].water_free()
        ens.assimilate([(B_, 20, 20, 3, 300.0, 0.25)], gain_base=0.0, gain_water=(0, 0, 0, 1))
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
        obs = [(B_, 100, 40, 3, 300.0, 0.25)]
        with pytest.raises(E.WxError) as ei:
            ens.assimilate(obs, loc=(5.0, 5.0))
        assert ei.value.code == -5 and "member 1: " in str(ei.value), str(ei.value)
        ens.assimilate(obs, loc=(5.0, 5.0))  # the report was consumed
    finally:
        ens.close()


def test_the_profile_names_both_kernels(pkg):
    """One launch of each for one state field, however many observations; one more update launch for the second field."""
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 2))
    try:
        pre = pre_values(pkg, ens)
        obs = observations(pre, np.random.Generator(np.random.Philox(3)), 40)
        for n, kw, launches in ((40, dict(gain_base=(0, 0, 0, 1)), 1), (1, dict(gain_base=(0, 0, 0, 1)), 1), (40, dict(gain_base=1.0, gain_water=1.0), 2),
                                (40, dict(gain_base=0.0), 0)):
            ens[0].profile(True)
            ens.assimilate(obs[:n], loc=(10.0, 5.0), **kw)
            prof = ens[0].profile_read()
            assert prof["ensemble_assimilate_obs"][1] == 1 and prof["ensemble_assimilate_obs"][0] > 0, (n, kw)
            assert prof.get("ensemble_assimilate", (0.0, 0))[1] == launches, (n, kw, prof)
    finally:
        ens.close()


def test_workflow_from_sim_perturb_step_assimilate_statistics(pkg):
    """WeatherEnsemble.from_sim of a stepped WeatherSim, perturb, step, assimilate the temperatures a lone nature run shows at five
    stations, statistics: the variance at the observed cells does not grow. (The stations lie more than 2 loc apart, so each observed
    cell is changed by its own observation only, whose factor on the deviations is sqrt(R / D) < 1.)"""
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
        stations = [(x, y0) for x in cols]
        obs = [(B_, x, y, 3, float(truth[y, x, 3]), 0.01) for x, y in stations]
        before = we.statistics(B_, want=("mean", "variance"))
        res = we.assimilate(obs, loc=(10.0, 3.0))  # wrap_x: the members' wrapHorizontally
        after = we.statistics(B_, want=("mean", "variance"))
        assert all(r["applied"] for r in res)
        for (x, y), r in zip(stations, res):
            assert 0 < after["variance"][y, x, 3] < before["variance"][y, x, 3], (x, y)
            assert abs(float(after["mean"][y, x, 3]) - float(truth[y, x, 3])) < abs(float(before["mean"][y, x, 3]) - float(truth[y, x, 3])) or abs(r["innovation"]) < 1e-3
            assert r["prior_var"] > 0 and abs(r["prior_mean"] - float(before["mean"][y, x, 3])) < 1e-3
        far = (after["variance"].view(np.uint32) == before["variance"].view(np.uint32))
        assert far[:y0 - 6].all() and far[y0 + 6:].all() and not far[y0 - 2:y0 + 3].all()  # localized in height
        assert same_bits(after["variance"][..., :3], before["variance"][..., :3])  # temperature only by default
        we.step(1)
        we.sync()
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
