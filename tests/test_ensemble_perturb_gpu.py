"""wx_ensemble_perturb on the GPU: the members' fields after the launch equal wx_ens_perturb_cells -- the kernel's own per-cell function on
the CPU, which tests/test_ensemble_perturb_cpu.py pins to the definition of include/wxsim.h -- of the values they held before, read through
a device-side clone; the display-side fields survive; a perturbed fresh ensemble steps like lone handles uploaded with the host function's
arrays; and the workflow spin up -> clone -> perturb -> step -> statistics. Every comparison is `==` on bits (NaNs compared as positions)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import impulse_scenes as I
from test_ensemble_gpu import FIELDS, same_bits
from test_ensemble_perturb_cpu import AMP as PLANTED_AMP
from test_ensemble_perturb_cpu import PLANTED_RUNS, PX, PY, planted_run
from test_ensemble_statistics_gpu import make_ensemble, member_specs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
X, Y = 130, 40
AMP = {"BASE_CUR": (0.05, 0.0, 1e-4, 2.0), "WATER_CUR": (0.5, 0.01, 0.0, 0.2)}
CLAMP = {"BASE_CUR": dict(lo=(-0.03, NAN, NAN, NAN), hi=(NAN, NAN, NAN, 300.0)), "WATER_CUR": dict(lo=(0.0, 0.0, NAN, 0.0))}
RECTS = [(0, 0, X, Y), (3, 5, 1, 7), (7, 2, 63, 9), (65, 1, 65, 30), (1, 17, 129, 1), (0, 39, 130, 1)]  # w = 130, 1, 63, 65 at odd x; h = 1; the whole grid
MASKS = {1: [None, [0]], 3: [None, [0, 2], [1]], 17: [None, [0, 3, 16], [5]]}


def pre_values(pkg, ens):
    """Every member's BASE_CUR, WATER_CUR and WALL_CUR, read through a clone (wx_copy_state into a lone handle, read there)."""
    lone = pkg.engine.Handle(ens.X, ens.Y, ens.n_droplets)
    try:
        out = []
        for m in ens.members:
            lone.copy_from(m)
            out.append({f: lone.read_rect(f) for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR")})
        return out
    finally:
        lone.close()


def host_perturb(pkg, pre, field, rect, members, **kw):
    """wx_ens_perturb_cells on the rectangle's cells of ``pre`` (one dict per member), pasted back: what the members should hold now."""
    x, y, w, h = rect
    cut = lambda a: np.ascontiguousarray(a[y:y + h, x:x + w])  # noqa: E731
    new = pkg.engine.ens_perturb_cells([cut(p[field]) for p in pre], [cut(p["WALL_CUR"]) for p in pre], X, Y, field, AMP[field], rect=rect, members=members, **kw)
    for p, n in zip(pre, new):
        p[field] = p[field].copy()
        p[field][y:y + h, x:x + w] = n


@pytest.mark.parametrize("B", [1, 3, 17])
def test_device_equals_host_function(pkg, B):
    """Members on different terrain, stepped twice; then a sequence of perturbations -- both fields, both modes, every rectangle and
    mask -- each compared on every member (the unselected ones keep their bits) against the host function of the values before."""
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, B))
    try:
        ens.step(2)
        pre = pre_values(pkg, ens)
        for i, m in enumerate(ens.members):  # the clone shows what the member shows
            assert same_bits(m.read_rect("BASE_CUR"), pre[i]["BASE_CUR"]) and same_bits(m.read_rect("WATER_CUR"), pre[i]["WATER_CUR"])
        assert B == 1 or len({p["WALL_CUR"].tobytes() for p in pre}) > 1  # different terrain
        k, changed = 0, {"BASE_CUR": False, "WATER_CUR": False}
        for field in ("BASE_CUR", "WATER_CUR"):
            for rect in RECTS:
                mode, members = ("add", "mul")[k % 2], MASKS[B][k % len(MASKS[B])]
                kw = dict(mode=mode, scale=(1, 3, 8, 64)[k % 4], seed=1000 + k, wrap_x=k % 3 == 0, **(CLAMP[field] if k % 5 == 0 else {}))
                before = [p[field] for p in pre]
                ens.perturb(field, AMP[field], rect=rect, members=members, **kw)
                host_perturb(pkg, pre, field, rect, members, **kw)
                for i, m in enumerate(ens.members):
                    got = m.read_rect(field)
                    assert same_bits(got, pre[i][field]), (field, rect, kw, "member", i, np.argwhere(got.view(np.uint32) != pre[i][field].view(np.uint32))[:4].tolist())
                    if members is not None and i not in members:
                        assert same_bits(got, before[i]), (field, rect, "unselected member", i)
                    wall_cells = pre[i]["WALL_CUR"][..., 1] == 0  # (whatever the host function says: a member's wall cells keep their bits)
                    assert wall_cells.any() and same_bits(got[wall_cells], before[i][wall_cells]), (field, rect, "wall cells of member", i)
                    changed[field] = changed[field] or not same_bits(got, before[i])
                k += 1
        assert changed["BASE_CUR"] and changed["WATER_CUR"]
        for i, m in enumerate(ens.members):  # the other field and the walls were never touched by a perturbation of one field
            assert same_bits(m.read_rect("WALL_CUR"), pre[i]["WALL_CUR"])
        ens.step(1)  # ... and the ensemble steps on
        ens.sync()
    finally:
        ens.close()


@pytest.mark.parametrize("B", [3, 17])
def test_planted_special_values_through_the_kernel(pkg, B):
    """The hand-built members of the CPU test through k_ens_perturb (nothing is stepped; every run starts from a fresh upload, whose
    bits the members show before the call): the device holds the host function's bits and what must be left alone is left alone --
    wall cells, the channel of amplitude 0, non-finite values, unselected members, the FLT_MAX whose result would overflow."""
    E, P = pkg.engine, pkg.params
    u = P.uniforms_from_gui(P.merge_settings(None), PY)
    ens = E.Ensemble(B, PX, PY, 0)

    def on_the_device(f, w, field, call):
        for m, a, wl in zip(ens.members, f, w):
            m.upload(a, a, wl)
            m.set_params(P.fill_struct(P.WxParams(), u), u["initial_T"])
            assert m.read_rect(field).view(np.uint32).tobytes() == a.view(np.uint32).tobytes()
        ens.perturb(field, PLANTED_AMP, **call)
        other = "WATER_CUR" if field == "BASE_CUR" else "BASE_CUR"
        assert all(m.read_rect(other).view(np.uint32).tobytes() == a.view(np.uint32).tobytes() for m, a in zip(ens.members, f))
        return [m.read_rect(field) for m in ens.members]

    try:
        for field, kw in PLANTED_RUNS:
            planted_run(pkg, B, field, kw, on_the_device)
    finally:
        ens.close()


def test_the_profile_names_the_kernel(pkg):
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 2))
    try:
        ens[0].profile(True)
        ens.perturb("BASE_CUR", AMP["BASE_CUR"], scale=4)
        prof = ens[0].profile_read()
        assert prof["ensemble_perturb"][1] == 1 and prof["ensemble_perturb"][0] > 0
    finally:
        ens.close()


_FAST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import wxpkg
pkg = wxpkg.load_package()
assert pkg.engine.lib().wx_arith() == 1, "not the tolerance build"
import test_ensemble_perturb_gpu as T
ens = T.make_ensemble(pkg, T.member_specs(pkg, T.X, T.Y, 3))
ens.step(2)
pre = T.pre_values(pkg, ens)
np.savez(sys.argv[2] + "_pre", **{f"{f}{i}": p[f] for i, p in enumerate(pre) for f in p})
ens.perturb("BASE_CUR", T.AMP["BASE_CUR"], mode="mul", scale=8, seed=5, wrap_x=True, rect=(7, 2, 65, 9))
ens.perturb("WATER_CUR", T.AMP["WATER_CUR"], mode="add", scale=3, seed=6, members=[0, 2])
np.savez(sys.argv[2] + "_post", **{f"{f}{i}": m.read_rect(f) for i, m in enumerate(ens.members) for f in ("BASE_CUR", "WATER_CUR")})
ens.close()
"""


def test_the_tolerance_build_on_the_device(pkg, tmp_path):
    """libwxsim_fast.so in a process of its own (a process holds one libwxsim): its kernel gives what THIS process's host function gives
    on the values the members held (the simulation steps of the two builds differ, the perturbation does not)."""
    fast = pkg.engine.FAST_LIB_PATH
    assert os.path.exists(fast), "libwxsim_fast.so is not built"
    stem = str(tmp_path / "fast")
    subprocess.check_call([sys.executable, "-c", _FAST_LEG, ROOT, stem], env=dict(os.environ, WXSIM_LIB=fast), timeout=300)
    a, b = np.load(stem + "_pre.npz"), np.load(stem + "_post.npz")
    pre = [{f: a[f"{f}{i}"] for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR")} for i in range(3)]
    host_perturb(pkg, pre, "BASE_CUR", (7, 2, 65, 9), None, mode="mul", scale=8, seed=5, wrap_x=True)
    host_perturb(pkg, pre, "WATER_CUR", (0, 0, X, Y), [0, 2], mode="add", scale=3, seed=6)
    for i in range(3):
        for f in ("BASE_CUR", "WATER_CUR"):
            assert same_bits(b[f"{f}{i}"], pre[i][f]), (i, f)
        assert not same_bits(b[f"BASE_CUR{i}"], a[f"BASE_CUR{i}"])


def test_refusals(pkg):
    """Every refusal of include/wxsim.h answers before anything is written; the ensemble then works as before."""
    E = pkg.engine
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 3)[:2] + [None])  # member 2 is never uploaded
    try:
        keep = [ens[i].read_rect(f) for i in (0, 1) for f in ("BASE_CUR", "WATER_CUR")]
        amp = AMP["BASE_CUR"]

        def refused(code, field, **kw):
            with pytest.raises(E.WxError) as ei:
                ens.perturb(field, amp, **kw)
            assert ei.value.code == code, (field, kw, str(ei.value))
            return str(ei.value)

        for f in ("CURL", "WALL_CUR", "BASE_DISP", "WATER_0", "LIGHT_0"):
            assert "WX_FIELD_BASE_CUR" in refused(-1, f, members=[0, 1])
        refused(-1, "BASE_CUR", members=[0, 1], mode=2)
        refused(-1, "BASE_CUR", members=[0, 1], scale=0)
        for rect in ((1, 0, X, 1), (0, 1, 1, Y), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (X, 0, 1, 1)):
            refused(-4, "WATER_CUR", members=[0, 1], rect=rect)
        assert "member 2" in refused(-5, "BASE_CUR")
        assert "member 2" in refused(-5, "WATER_CUR", members=[1, 2])
        refused(-1, "BASE_CUR", members=[])
        now = [ens[i].read_rect(f) for i in (0, 1) for f in ("BASE_CUR", "WATER_CUR")]
        assert all(same_bits(a, b) for a, b in zip(now, keep))
        ens.perturb("BASE_CUR", amp, members=[0, 1], scale=4)
        assert not same_bits(ens[0].read_rect("BASE_CUR"), keep[0]) and not same_bits(ens[1].read_rect("BASE_CUR"), keep[2])
    finally:
        ens.close()


def test_display_side_fields_survive(pkg):
    """After a step whose last iteration was a display iteration (WATER_0 pending, BASE_DISP lazy) both fields are perturbed: WATER_0,
    BASE_DISP, CURL and the rest of the display side read what an untouched clone reads."""
    ens = make_ensemble(pkg, member_specs(pkg, X, Y, 2))
    clone = pkg.engine.Handle(X, Y)
    try:
        ens.step(4)
        clone.copy_from(ens[1])
        ens.perturb("BASE_CUR", AMP["BASE_CUR"], scale=3)
        ens.perturb("WATER_CUR", AMP["WATER_CUR"], scale=3)
        for f in ("WATER_0", "BASE_DISP", "CURL", "WALL_DISP", "LIGHT_0", "LIGHT_1"):
            assert same_bits(ens[1].read_rect(f), clone.read_rect(f)), f
        assert not same_bits(ens[1].read_rect("BASE_CUR"), clone.read_rect("BASE_CUR")) and not same_bits(ens[1].read_rect("WATER_CUR"), clone.read_rect("WATER_CUR"))
    finally:
        ens.close()
        clone.close()


def _upload_equivalence(pkg, specs, steps=6):
    """A freshly uploaded ensemble, perturbed in base (vx, T) and water, against lone handles uploaded with the host function's arrays:
    compared from the first iteration on, on every field."""
    E, P = pkg.engine, pkg.params
    B = len(specs)
    ens = make_ensemble(pkg, specs)
    lone = [E.Handle(X, Y) for _ in specs]
    try:
        kb, kw = dict(mode="add", scale=5, seed=31, wrap_x=True), dict(mode="mul", scale=2, seed=32)
        amp_b, amp_w = (0.02, 0.0, 0.0, 0.5), (0.1, 0.0, 0.0, 0.3)
        ens.perturb("BASE_CUR", amp_b, **kb)
        ens.perturb("WATER_CUR", amp_w, lo=(0.0, NAN, NAN, 0.0), **kw)
        walls = [s["wall"] for s in specs]
        base = E.ens_perturb_cells([s["base"] for s in specs], walls, X, Y, "BASE_CUR", amp_b, **kb)
        water = E.ens_perturb_cells([s["water"] for s in specs], walls, X, Y, "WATER_CUR", amp_w, lo=(0.0, NAN, NAN, 0.0), **kw)
        for i, s in enumerate(specs):
            assert not same_bits(base[i], s["base"])
            for opt, val in s.get("options", {}).items():
                lone[i].set_option(opt, val)
            lone[i].upload(base[i], water[i], s["wall"])
            lone[i].iter = s.get("iter0", 0)
            lone[i].set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
            assert same_bits(ens[i].read_rect("BASE_CUR"), base[i]) and same_bits(ens[i].read_rect("WATER_CUR"), water[i]), i
        for it in range(steps):
            ens.step(1)
            for i in range(B):
                lone[i].step(1)
                for f in FIELDS:
                    a, b = ens[i].read_rect(f), lone[i].read_rect(f)
                    assert same_bits(a, b), ("iteration", it + 1, "member", i, f, int((a != b).sum()))
        return ens.stats(), [water[i] for i in range(B)], [m.read_rect("WATER_CUR") for m in ens.members]
    finally:
        ens.close()
        for h in lone:
            h.close()


def test_equals_an_upload_at_iteration_0_wet(pkg):
    stats, _, _ = _upload_equivalence(pkg, member_specs(pkg, X, Y, 3))
    assert stats["member_iters_batched"] == 18


def test_equals_an_upload_at_iteration_0_water_free_dry(pkg):
    """A water-free scene under WX_PASS_DRY whose (trivial) water got perturbed: smoke appears (v + a r with a lower clamp of 0), so the
    member is no longer water-free and must run the water-carrying dry kernel, as the lone handle that was uploaded with that water does."""
    specs = []
    for i in range(2):
        b, w, wl = I.impulse_scene(X, Y, "fast_vx", offset=(i, 1 + i), seed=50 + i)[:3]
        specs.append(dict(base=b, water=w, wall=wl, u=I.scene_uniforms("fast_vx", Y, dry=True)))
    E = pkg.engine
    ens = make_ensemble(pkg, specs)
    try:
        assert ens[0].water_free()
        ens.perturb("WATER_CUR", (0.0, 0.0, 0.0, 0.25), mode="add", scale=2, seed=9, lo=(NAN, NAN, NAN, 0.0))
        assert not ens[0].water_free()
    finally:
        ens.close()
    # the comparison itself, with an additive smoke perturbation (a multiplicative one leaves the zeros of a water-free scene zero)
    ens = make_ensemble(pkg, specs)
    lone = [E.Handle(X, Y) for _ in specs]
    try:
        kw = dict(mode="add", scale=2, seed=9, lo=(NAN, NAN, NAN, 0.0))
        amp = (0.0, 0.0, 0.0, 0.25)
        ens.perturb("WATER_CUR", amp, **kw)
        water = E.ens_perturb_cells([s["water"] for s in specs], [s["wall"] for s in specs], X, Y, "WATER_CUR", amp, **kw)
        assert (water[0][..., 3] > 0).any()
        P = pkg.params
        for i, s in enumerate(specs):
            lone[i].upload(s["base"], water[i], s["wall"])
            lone[i].set_params(P.fill_struct(P.WxParams(), s["u"]), s["u"]["initial_T"])
            assert not lone[i].water_free()
        for it in range(6):
            ens.step(1)
            for i in range(2):
                lone[i].step(1)
                for f in FIELDS:
                    a, b = ens[i].read_rect(f), lone[i].read_rect(f)
                    assert same_bits(a, b), ("iteration", it + 1, "member", i, f, int((a != b).sum()))
        assert not same_bits(ens[0].read_rect("WATER_CUR"), water[0])  # the smoke moved: the water-carrying kernel ran
    finally:
        ens.close()
        for h in lone:
            h.close()


def test_workflow_from_sim_perturb_step_statistics(pkg):
    """WeatherEnsemble.from_sim of a stepped WeatherSim, perturb, step, statistics."""
    W = pkg.sim
    Xw, Yw, B = 128, 48, 4
    base, water, wall = pkg.synth.terrain_grid(Xw, Yw)
    sim = W.WeatherSim(Xw, Yw, base, water, wall, None, {"dayNightCycle": False}, sun_angle_deg=30.0)
    sim.verbose = False
    we = None
    try:
        sim.step(6)
        we = W.WeatherEnsemble.from_sim(sim, B)
        for m in we.members:
            assert m.iter_num == 6 and m.gui == sim.gui
            for f in ("BASE_CUR", "WATER_CUR", "WATER_0", "BASE_DISP", "LIGHT_0", "LIGHT_1", "CURL"):
                assert same_bits(m.read_rect(f), sim.read_rect(f)), f
        st = we.statistics("BASE_CUR")
        air = sim.read_rect("WALL_CUR")[..., 1] != 0
        assert (st["n_wall"] == np.where(air, 0, B)).all() and (st["count"] == np.where(air, B, 0)[..., None]).all()
        assert (st["variance"][air].view(np.uint32) == 0).all()  # clones: the variance is exactly +0.0
        rect = (16, 20, 64, 16)
        we.perturb("BASE_CUR", (0.0, 0.0, 0.0, 0.5), scale=8, seed=3, rect=rect)
        st = we.statistics("BASE_CUR")
        inside = np.zeros((Yw, Xw), bool)
        inside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
        assert (st["variance"][inside & air][:, 3] > 0).all() and (inside & air).any()
        assert (st["variance"][~inside & air].view(np.uint32) == 0).all() and (st["variance"][air][:, :3].view(np.uint32) == 0).all()
        we.step(2)
        st = we.statistics("BASE_CUR")
        air = we[0].read_rect("WALL_CUR")[..., 1] != 0
        assert all(same_bits(m.read_rect("WALL_CUR"), we[0].read_rect("WALL_CUR")) for m in we.members)
        assert (st["count"] == np.where(air, B, 0)[..., None]).all() and (st["n_wall"] == np.where(air, 0, B)).all()
        assert (st["variance"][inside & air] > 0).any() and we[0].iter_num == 8
        # the host-side copy: member 3 takes member 0's state and settings back
        we[3].set_gui(wind=0.3)
        we.broadcast(0, [3])
        assert we[3].gui == we[0].gui and same_bits(we[3].read_rect("BASE_CUR"), we[0].read_rect("BASE_CUR"))
        sim.copy_from(we[1])
        assert sim.iter_num == 8 and same_bits(sim.read_rect("BASE_CUR"), we[1].read_rect("BASE_CUR"))
    finally:
        if we is not None:
            we.close()
        sim.handle.close()
