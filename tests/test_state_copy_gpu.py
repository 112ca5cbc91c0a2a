"""wx_copy_state / wx_ensemble_broadcast on the GPU: after the copy dst shows what src shows -- every readable field (the ones made on demand
included), droplets, iteration counter, diagnostics -- and every later step of dst yields what the same step of src yields, whatever dst
held before, under dst's own options; src is unchanged; the refusals of include/wxsim.h. Every comparison is `==` on bits (NaNs compared
as positions)."""
import numpy as np
import pytest

import impulse_scenes as I
import surface_scenes as S
from test_ensemble_droplets_gpu import _order1, _precip64, pool_of
from test_ensemble_gpu import FIELDS, same_bits, same_diag

pytestmark = pytest.mark.gpu

# VORT is an intermediate: only the per-pass kernel set stores it, and making WATER_0 on demand uses it as scratch -- not comparable
# between handles that differ in those options
NO_VORT = [f for f in FIELDS if f != "VORT"]


def fill(pkg, h, scene, u, iter0=0, options=None, drops=None):
    for opt, val in (options or {}).items():
        h.set_option(opt, val)
    h.upload(scene[0], scene[1], scene[2], drops)
    h.iter = iter0
    h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
    return h


def read_all(h, fields=FIELDS):
    out = {f: h.read_rect(f) for f in fields}
    if h.n_droplets:
        out["droplets"] = h.read_particles()
    return out


def assert_same(dst, src, where, fields=FIELDS, diag=True):
    """dst's fields are read first, then src's."""
    a = read_all(dst, fields)
    b = read_all(src, fields)
    for k in a:
        assert same_bits(a[k], b[k]), (where, k, int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else "shape")
    assert dst.iter == src.iter, where
    if diag:
        assert same_diag(dst.diagnostics(), src.diagnostics()) is None, where


def src_scene(X, Y):
    return S.surface_scene(X, Y, "smoke", offset=1, variant="stepped")[:3], S.scene_uniforms(Y)


def other_scene(X, Y):
    return I.impulse_scene(X, Y, "wall", offset=(2, 3), seed=77)[:3], I.scene_uniforms("wall", Y)


@pytest.mark.parametrize("dst_kind", ["other_scene_stepped_3", "never_uploaded"])
@pytest.mark.parametrize("X,Y", [(130, 40), (70, 24)])
def test_mid_frame_clone(pkg, X, Y, dst_kind):
    """src steps 7 (odd: `even` flipped; the last iteration a display iteration with WATER_0 and BASE_DISP still to be made; nothing read
    since). dst holds another scene on other terrain at another parity, or nothing at all."""
    E = pkg.engine
    src, dst = E.Handle(X, Y), E.Handle(X, Y)
    try:
        fill(pkg, src, *src_scene(X, Y), iter0=9990)
        if dst_kind != "never_uploaded":
            fill(pkg, dst, *other_scene(X, Y))
            dst.step(3)
        src.step(7)
        dst.copy_from(src)
        assert dst.fastest_velocity() == 0.0
        assert_same(dst, src, "after the copy")
        src.step(5)
        dst.step(5)
        assert_same(dst, src, "5 steps later")
        assert dst.iter == 9990 + 12
        # ... and the copy of a state whose on-demand fields HAVE been made, stepped an even number
        dst.step(1)
        dst.copy_from(src)
        assert_same(dst, src, "second copy")
        src.step(2)
        dst.step(2)
        assert_same(dst, src, "2 steps after the second copy")
    finally:
        src.close()
        dst.close()


def test_src_is_unchanged(pkg):
    """A twin of src that is never copied from shows the same fields after the same steps."""
    E, X, Y = pkg.engine, 130, 40
    src, twin, dst = E.Handle(X, Y), E.Handle(X, Y), E.Handle(X, Y)
    try:
        for h in (src, twin):
            fill(pkg, h, *src_scene(X, Y))
            h.step(7)
        dst.copy_from(src)
        assert_same(src, twin, "after being copied from")
        dst.copy_from(src)
        for h in (src, twin):
            h.step(4)
        assert_same(src, twin, "4 steps later")
        assert src.fastest_velocity() == twin.fastest_velocity()
    finally:
        for h in (src, twin, dst):
            h.close()


def test_droplets_across_the_inactive_count_refresh(pkg, golden):
    """WX_OPT_SPLAT_ORDER 1: clone at iteration 598, step 5 (the 600-iteration refresh of the inactive count lies in between): the pool,
    PRECIP_FB, PRECIP_DEP, LIGHTNING and everything else are equal. Default order: the pool after the first iteration."""
    E = pkg.engine
    g, u = _precip64(golden)
    drops = pool_of(np.ascontiguousarray(g["in_drops"], np.float32), 400)
    scene = (g["in_base"], g["in_water"], g["in_wall"])
    src, dst = E.Handle(64, 48, 400), E.Handle(64, 48, 400)
    try:
        fill(pkg, src, scene, u, iter0=591, options=_order1(pkg), drops=drops)
        water = g["in_water"].copy()
        water[30:40, 10:30, 3] += np.float32(1.0)
        fill(pkg, dst, (g["in_base"], water, g["in_wall"]), dict(u, spawnChanceMult=float(u["spawnChanceMult"]) * 3.0), iter0=17, options=_order1(pkg), drops=drops[::-1].copy())
        dst.step(2)
        src.step(7)
        assert src.iter == 598
        dst.copy_from(src)
        assert_same(dst, src, "clone at 598")
        assert np.abs(src.read_rect("PRECIP_FB")).max() > 0
        src.step(5)
        dst.step(5)
        assert_same(dst, src, "at 603")
        assert (src.read_particles()[:, 2] >= 0).any()  # there are active droplets
        # the default order on the clone, the source switched to it as well: one iteration of the same pool on the same grid
        for h in (src, dst):
            h.set_option(E.Handle.OPT_SPLAT_ORDER, 0)
        dst.copy_from(src)
        src.step(1)
        dst.step(1)
        assert same_bits(dst.read_particles(), src.read_particles())
    finally:
        src.close()
        dst.close()


def test_a_clone_without_deposit_records_into_a_handle_with_them(pkg, golden):
    """Options are dst's: src runs the default splat order and owns no deposit records, dst runs WX_OPT_SPLAT_ORDER 1 (its records and
    their constant index table lie behind the storage the two handles share a layout of) -- and the reverse."""
    E = pkg.engine
    g, u = _precip64(golden)
    drops = pool_of(np.ascontiguousarray(g["in_drops"], np.float32), 400)
    scene = (g["in_base"], g["in_water"], g["in_wall"])
    plain, ordered, ref = E.Handle(64, 48, 400), E.Handle(64, 48, 400), E.Handle(64, 48, 400)
    try:
        fill(pkg, plain, scene, u, drops=drops)
        for h in (ordered, ref):
            fill(pkg, h, scene, u, options=_order1(pkg), drops=drops)
        ordered.step(3)
        ref.step(3)
        plain.copy_from(ordered)  # (the pool is bit-identical under either order; the grid under order 1 only)
        ordered.step(2)           # ... ordered moves on, and is then replaced by a state that came through the handle without records
        plain.copy_from(ref)
        ordered.copy_from(plain)
        assert_same(ordered, ref, "through a handle without records")
        ordered.step(4)
        ref.step(4)
        assert_same(ordered, ref, "4 ordered steps later")
    finally:
        for h in (plain, ordered, ref):
            h.close()


def test_the_water_free_dry_state(pkg):
    """128 x 32 under WX_PASS_DRY with one fast cell (the pair kernel's tile path runs): src steps 3 (a pair and a single), the clone
    and src step 4 more; dst's wx_pair_stats start from zero although dst had run pairs of its own."""
    E, X, Y = pkg.engine, 128, 32
    scene = I.impulse_scene(X, Y, "fast_vx", pitch=(1000, 1000), offset=(40, 9), fast_values=(1.3,))
    assert len(scene[4]) == 1
    u = I.scene_uniforms("fast_vx", Y, dry=True)
    src, dst = E.Handle(X, Y), E.Handle(X, Y)
    try:
        fill(pkg, src, scene[:3], u)
        other = I.impulse_scene(X, Y, "fast_vx", pitch=(1000, 1000), offset=(90, 20), fast_values=(2.0,), seed=5)
        fill(pkg, dst, other[:3], u)
        dst.step(2)
        src.step(3)
        assert src.water_free()
        dst.copy_from(src)
        assert dst.pair_stats() == (0, 0) and dst.water_free()
        cells, _ = src.pair_stats()
        assert cells > 0  # src's own counters were not touched by the copy: the tile path ran
        assert_same(dst, src, "dry clone")
        src.step(4)
        dst.step(4)
        assert_same(dst, src, "4 dry steps later")
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("src_opt,dst_opt", [("perpass", "march"), ("march", "perpass"), ("lazy_off", "march"), ("march", "lazy_off")])
def test_options_are_dsts(pkg, src_opt, dst_opt):
    """The clone goes on under its own options: kernel set and WATER_0 on demand differ between the two handles; the results do not
    (the kernel sets are bit-identical to each other), except for the intermediate VORT."""
    E, X, Y = pkg.engine, 130, 40
    opts = {"perpass": {E.Handle.OPT_KERNEL_SET: 0}, "march": {}, "lazy_off": {E.Handle.OPT_WATER0_ON_DEMAND: 0}}
    src, dst = E.Handle(X, Y), E.Handle(X, Y)
    try:
        fill(pkg, src, *src_scene(X, Y), options=opts[src_opt])
        fill(pkg, dst, *other_scene(X, Y), options=opts[dst_opt])
        dst.step(2)
        src.step(7)
        dst.copy_from(src)
        assert_same(dst, src, "after the copy")
        src.step(5)
        dst.step(5)
        assert_same(dst, src, "5 steps later", fields=NO_VORT)
    finally:
        src.close()
        dst.close()


def test_lone_and_member_both_ways_without_a_sync(pkg):
    """A lone handle on the default stream, members on the ensemble's: the copies follow the steps directly."""
    E, X, Y = pkg.engine, 130, 40
    lone, lone2, ens = E.Handle(X, Y), E.Handle(X, Y), E.Ensemble(3, X, Y)
    try:
        fill(pkg, lone, *src_scene(X, Y))
        for i in range(3):
            fill(pkg, ens[i], *other_scene(X, Y), iter0=100 * i)
        lone.step(7)
        ens.step(3)
        ens[1].copy_from(lone)   # lone -> member
        lone2.copy_from(ens[2])  # member -> lone (never uploaded)
        assert_same(ens[1], lone, "lone -> member")
        assert_same(lone2, ens[2], "member -> lone")
        before = ens.stats()
        ens.step(5)
        lone.step(5)
        lone2.step(5)
        assert_same(ens[1], lone, "lone -> member, 5 steps later")
        assert_same(lone2, ens[2], "member -> lone, 5 steps later")
        assert ens.stats()["member_iters_batched"] == before["member_iters_batched"] + 15
    finally:
        ens.close()
        lone.close()
        lone2.close()


def test_broadcast(pkg):
    """Five members, source 2, mask {0, 3}: members 0 and 3 become member 2, members 1 and 4 are untouched bit for bit,
    wx_ensemble_stats is unchanged, and three ensemble steps later 0, 2 and 3 are still equal."""
    E, X, Y = pkg.engine, 130, 40
    ens = E.Ensemble(5, X, Y)
    try:
        scenes = [other_scene(X, Y), (I.impulse_scene(X, Y, "cloud", offset=(1, 4))[:3], I.scene_uniforms("cloud", Y)), src_scene(X, Y),
                  (S.surface_scene(X, Y, "snow")[:3], S.scene_uniforms(Y, wrap=False)), (I.impulse_scene(X, Y, "smoke", offset=(5, 2))[:3], I.scene_uniforms("smoke", Y))]
        for i, (sc, u) in enumerate(scenes):
            fill(pkg, ens[i], sc, u, iter0=10 * i)
        ens.step(3)
        keep = {i: read_all(ens[i]) for i in (1, 4)}
        stats = ens.stats()
        ens.broadcast(2, [0, 3])
        assert ens.stats() == stats
        for i in (0, 3):
            assert_same(ens[i], ens[2], ("broadcast", i))
        for i in (1, 4):
            now = read_all(ens[i])
            assert all(same_bits(now[k], keep[i][k]) for k in now), i
            assert ens[i].iter == 10 * i + 3
        ens.step(3)
        for i in (0, 3):
            assert_same(ens[i], ens[2], ("broadcast, 3 steps later", i))
        assert not same_bits(ens[1].read_rect("WATER_CUR"), ens[2].read_rect("WATER_CUR"))
        ens.broadcast(4)  # NULL mask: all others
        for i in range(4):
            assert_same(ens[i], ens[4], ("broadcast to all", i), diag=False)
        with pytest.raises(E.WxError) as ei:
            ens.broadcast(5)
        assert ei.value.code == -1
        assert E.lib().wx_ensemble_broadcast(ens._e, -1, None) == -1
    finally:
        ens.close()


def test_refusals(pkg):
    E, X, Y = pkg.engine, 70, 24
    L = E.lib()
    a, b = E.Handle(X, Y), E.Handle(X, Y)
    wide, tall, drops, slab = E.Handle(X + 1, Y), E.Handle(X, Y + 1), E.Handle(X, Y, 64), E.Handle(64, Y, X_global=256, x0=0, halo=12)
    try:
        def refused(code, dst, src, text=""):
            with pytest.raises(E.WxError) as ei:
                dst.copy_from(src)
            assert ei.value.code == code and text in str(ei.value), str(ei.value)

        assert L.wx_copy_state(a._h, None) == -1 and L.wx_copy_state(None, a._h) == -1
        refused(-5, b, a, "never uploaded")
        a.upload(*src_scene(X, Y)[0])
        refused(-5, b, a, "no parameters")
        fill(pkg, a, *src_scene(X, Y))
        a.copy_from(a)  # dst == src: nothing to do
        for other in (wide, tall, drops, slab):
            refused(-1, other, a)
            refused(-1, a, other)
        a.step(2)
        b.copy_from(a)
        assert_same(b, a, "after the refusals")
    finally:
        for h in (a, b, wide, tall, drops, slab):
            h.close()


def test_an_overflowed_list_of_src_is_reported_once_and_nothing_is_copied(pkg):
    E, X, Y = pkg.engine, 505, 77
    src, dst = E.Handle(X, Y), E.Handle(X, Y)
    try:
        fast = I.impulse_scene(X, Y, "fast_vx")
        fill(pkg, src, fast[:3], I.scene_uniforms("fast_vx", Y), options={E.Handle.OPT_FIX_CAP: 2})
        fill(pkg, dst, *other_scene(X, Y), iter0=40)
        dst.step(2)
        keep = read_all(dst)
        src.step(2)
        with pytest.raises(E.WxError) as ei:
            dst.copy_from(src)
        assert ei.value.code == -5 and "exact path" in str(ei.value), str(ei.value)
        now = read_all(dst)
        assert all(same_bits(now[k], keep[k]) for k in now) and dst.iter == 42
        dst.copy_from(src)  # the report was consumed
        assert dst.iter == 2
        src.sync()
    finally:
        src.close()
        dst.close()
