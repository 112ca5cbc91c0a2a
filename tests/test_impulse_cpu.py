"""The impulse-lattice scenes (tests/impulse_scenes.py) checked without a GPU: which lane / row / tile phases the case list of
tests/test_impulse_gpu.py reaches with a lone trigger (computed from the list itself -- dropping any offset of a sweep loses something),
that the sites are isolated, that every trigger changes what the oracle computes (a kernel that ignored it would not pass), and that a
scene is a pure function of its arguments."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import impulse_scenes as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "2d-weather-sandbox_amd", "csrc")


def test_strip_geometry_is_the_kernels():
    """The widths the accounting works with are the constants of the kernel sources."""
    def const(fname, name):
        m = re.search(r"constexpr int[^;]*\b%s\s*=\s*(\d+)" % name, open(os.path.join(CSRC, fname)).read())
        assert m, (fname, name)
        return int(m.group(1))
    assert const("wx_wet.h", "WOUT") == I.WET_STRIP
    assert const("wx_march.h", "MOUT") == I.DRY_STRIP
    assert const("wx_march2.h", "M2OUT") == I.PAIR_STRIP
    px, py = I.PITCH
    for m in (I.WET_STRIP, I.DRY_STRIP, I.SPLAT_TILE[0]):
        assert np.gcd(px, m) == 1
    for m in (I.PAIR_TILE, I.SPLAT_TILE[1]):
        assert np.gcd(py, m) == 1 and np.gcd(I.DROPLET_PITCH[1], m) == 1


def _missing(X, Y, sites, requires, strip):
    """What ``sites`` leave uncovered of the requirements; ``strip``: output columns per wave of the kernel the case runs (None: no strips)."""
    sites = set(sites)
    miss = []
    for req in requires:
        if req == "lanes":  # every row x the first three, the last three and an interior output lane of a whole strip; without strips every row
            if strip is None:
                rows = {y for _, y in sites}
                miss += [("rows", y) for y in range(1, Y) if y not in rows]
                continue
            w, full = strip, (X // strip) * strip
            have = {(y, x % w) for x, y in sites if x < full}
            for y in range(1, Y):
                miss += [(req, w, y, ph) for ph in (0, 1, 2, w - 3, w - 2, w - 1) if (y, ph) not in have]
                if not any((y, ph) in have for ph in range(3, w - 3)):
                    miss.append((req, w, y, "interior"))
        elif req == "rows":
            rows = {y for _, y in sites}
            miss += [(req, y) for y in range(1, Y) if y not in rows]
        elif req == "edges":  # columns 0, 1, X-2, X-1 and the first / last two columns of the ragged last strip (56- and 60-column strips)
            cols = {x for x, _ in sites}
            miss += [(req, x) for x in I._edge_columns(X) if x not in cols]
        elif req == "splat_borders":
            have = {(x % 64, y % 16) for x, y in sites}
            miss += [(req, a, b) for a in range(64) for b in range(16) if (a in (0, 63) or b in (0, 15)) and (a, b) not in have]
        elif req == "sprite_straddles":  # the 12 x 12 sprite [x-6, x+5] x [y-6, y+5] over the grid's four edges and over a 64 x 16 tile corner
            tests = {"column 0": lambda x, y: x < 6, "column X-1": lambda x, y: x + 5 >= X, "row 0": lambda x, y: y < 6, "row Y-1": lambda x, y: y + 5 >= Y,
                     "tile corner": lambda x, y: 6 <= x < X - 6 and 6 <= y < Y - 6 and (x - 6) // 64 != (x + 5) // 64 and (y - 6) // 16 != (y + 5) // 16}
            miss += [(req, k) for k, f in tests.items() if not any(f(x, y) for x, y in sites)]
        else:
            raise AssertionError(req)
    return miss


def _group_missing(sw, group, without=None):
    """The requirements of sweep ``sw`` over the cases of one (kind, configuration) -- the sites THOSE cases plant, in the strip width of
    the kernel THAT configuration runs; ``without``: an offset left out."""
    X, Y = sw["grid"]
    sites = [s for c in group if tuple(c["offset"]) != without for s in I.lattice_sites(X, Y, c["pitch"], c["offset"])]
    return _missing(X, Y, sites, sw["requires"], I.config_strip(group[0]["config"]))


@pytest.mark.parametrize("name", [sw["name"] for sw in I.SWEEPS if sw["requires"]])
def test_phase_accounting(name):
    """Computed from the case list the GPU test runs, per (kind, configuration): the sites of the cases that plant THIS kind and run
    THIS configuration cover what the sweep is there for, in the strip width of the kernel that configuration runs (56 columns: wet and
    pair kernel, 60: the one-iteration dry kernel, none: per-pass -- every row). And no offset is spare: without any one of them some
    (kind, configuration) loses something."""
    sw = next(s for s in I.SWEEPS if s["name"] == name)
    groups = {}
    for c in I.cases():
        if c["sweep"] == name:
            groups.setdefault((c["kind"], c["config"]), []).append(c)
    assert set(groups) == {(k, cfg) for k in sw["kinds"] for cfg in sw["configs"]}  # every kind meets every configuration of the sweep
    for key, group in groups.items():
        assert sorted(tuple(c["offset"]) for c in group) == sorted(sw["offsets"]), key  # ... at every offset
        miss = _group_missing(sw, group)
        assert not miss, (key, len(miss), miss[:10])
    one_of_each_geometry = {I.config_strip(cfg): g for (k, cfg), g in groups.items()}.values()  # (sites do not depend on the kind)
    for off in sw["offsets"]:
        assert any(_group_missing(sw, g, without=tuple(off)) for g in one_of_each_geometry), f"offset {off} of {name} covers nothing of its own"


def test_phase_accounting_over_all_cases():
    """Over everything the GPU test runs: every column phase of the 56- and 60-column strips, every position of an 8 x 8 tile (counted
    from the grid's and from the strip's first column); the pair kernel's ragged last strip of one column and of all but one; the case
    list holds no case twice."""
    cs = I.cases()
    assert len({json.dumps(c, sort_keys=True) for c in cs}) == len(cs)
    sites = {(x, y) for c in cs if c["background"] == "air" and c["config"].startswith("dry_pairs") for x, y in I.lattice_sites(c["X"], c["Y"], c["pitch"], c["offset"])}
    assert {((x % 56) % 8, y % 8) for x, y in sites} == {(a, b) for a in range(8) for b in range(8)}
    for strip, prefix in ((56, "wet"), (56, "dry_pairs"), (60, "dry_single")):
        xs = {x for c in cs if c["config"].startswith(prefix) for x, _ in I.lattice_sites(c["X"], c["Y"], c["pitch"], c["offset"])}
        assert {x % strip for x in xs} == set(range(strip)), (strip, prefix)
    assert {c["X"] % 56 for c in cs if c["config"].startswith("dry_pairs")} >= {1, 55}


def test_fast_dry_pair_sites_are_still_fast_in_the_second_iteration(oracle):
    """A lone spike of 7.5 cells / iteration is below 0.9 after the pressure step of its first iteration: the pair kernel's own exact
    path -- second-iteration cells of 0.9 or more, recorded by tile; three cells or more: the pair repeated whole -- would never be
    raised. Every dry-pairs case of a fast kind therefore plants DRY_FAST_VALUES; on the oracle: the velocities the SECOND iteration
    advects with reach 0.9 in nine of ten such scenes and 3 cells in a quarter (how much of a spike survives its first iteration
    varies with where its back-trace lands); the GPU test computes the same from the oracle per case and asserts cells recomputed > 0
    (or the pair repeated) for each case that has such a cell."""
    seen, n1, n3 = set(), 0, 0
    for c in I.cases():
        key = (c["X"], c["Y"], c["kind"], tuple(c["offset"]))
        if not c["config"].startswith("dry_pairs") or c["kind"] not in ("fast_vx", "fast_vy") or key in seen or c["X"] * c["Y"] > 60000:
            continue
        seen.add(key)
        assert c["scene"]["fast_values"] == list(I.DRY_FAST_VALUES)
        u = I.scene_uniforms(c["kind"], c["Y"], dry=True)
        base, water, wall, _, sites = I.build_case(c)
        o = oracle.OracleSim(c["X"], c["Y"], 0)
        o.upload(base, water, wall)
        o.set_params(u)
        o.step(1)
        o.set_params(dict(u, pass_mask=1))  # the velocity pass of iteration 2 alone
        o.step(1)
        v = np.abs(o.field("BASE_CUR")[..., :2]).max(-1)
        o.close()
        n1 += bool(v.max() >= 0.9)
        n3 += bool(v.max() >= 3.0)
    assert len(seen) >= 200 and n1 >= len(seen) * 9 // 10 and n3 >= len(seen) // 4, (len(seen), n1, n3)


def test_sites_are_isolated():
    """No two sites of any case closer than 72 columns (periodic) and 10 rows; the builder plants exactly the lattice on free air."""
    seen = set()
    for c in I.cases():
        key = (c["X"], c["Y"], tuple(c["pitch"]), tuple(c["offset"]))
        if key in seen:
            continue
        seen.add(key)
        sites = I.lattice_sites(c["X"], c["Y"], c["pitch"], c["offset"])
        assert sites and not I.isolation_violations(sites, c["X"]), key
        assert all(0 <= x < c["X"] and 1 <= y < c["Y"] for x, y in sites)
    assert I.isolation_violations([(0, 5), (504, 9)], 505) and not I.isolation_violations([(0, 5), (504, 15)], 505)  # the seam counts


def _oracle(oracle, X, Y, scene, u, n=1, mask=None):
    base, water, wall, drops, _ = scene
    o = oracle.OracleSim(X, Y, 0 if drops is None else len(drops))
    o.upload(base, water, wall, drops)
    o.set_params(u if mask is None else dict(u, pass_mask=mask))
    o.step(n)
    out = {f: o.field(f) for f in ("BASE_CUR", "WATER_CUR", "WALL_CUR", "PRECIP_FB")}
    o.close()
    return out


@pytest.mark.parametrize("kind,dry,background", [(k, False, b) for k in I.KINDS for b in ("air", "terrain")] + [(k, True, "air") for k in I.DRY_KINDS])
def test_every_trigger_changes_what_the_oracle_computes(oracle, kind, dry, background):
    """A floor, not a proof of sensitivity: stepping the oracle with and without the triggers, after one iteration the state differs in
    the 3 x 3 cells around EVERY site (droplets: the feedback texture under the sprite; a wall cell: its own byte at least) and nowhere far from one. For the fast kinds the velocity the advection stage sees at a site planted
    with 2.99 cells / iteration or more really is 0.9 or more, and so at half of all sites: its back-trace leaves the 3 x 3 neighbourhood."""
    X, Y = 505, 133
    u = I.scene_uniforms(kind, Y, dry=dry)
    with_t = I.impulse_scene(X, Y, kind, offset=(3, 5), background=background)
    without = I.impulse_scene(X, Y, kind, offset=(3, 5), background=background, plant=False)
    sites = with_t[4]
    assert len(sites) >= 20 and sites == without[4]
    a, b = _oracle(oracle, X, Y, with_t, u), _oracle(oracle, X, Y, without, u)
    fields = ("PRECIP_FB",) if kind == "droplet" else ("BASE_CUR", "WATER_CUR", "WALL_CUR")
    for x, y in sites:
        ys = slice(max(0, y - 1), y + 2)
        xs = [(x - 1) % X, x, (x + 1) % X]
        assert any(not np.array_equal(a[f][ys][:, xs], b[f][ys][:, xs]) for f in fields), (kind, x, y)
    far = np.ones((Y, X), bool)  # ... and only there: an iteration carries a disturbance a few cells
    for x, y in sites:
        far[max(0, y - 9):y + 10, [(x + d) % X for d in range(-24, 25)]] = False
    if kind not in ("wall", "droplet"):  # (a wall cell re-labels the column above it; a sprite is 12 x 12)
        assert np.array_equal(a["BASE_CUR"][far], b["BASE_CUR"][far])
    if kind in ("fast_vx", "fast_vy"):
        pre = _oracle(oracle, X, Y, with_t, u, mask=1 if dry else 7)["BASE_CUR"]  # what the advection stage reads: after velocity (+ boundary)
        n_fast = 0
        for k, (x, y) in enumerate(sites):
            v = float(np.abs(pre[y, x, :2]).max())
            if 2.99 <= abs(I.site_value(kind, k)):  # (1.3 next to the ground may be braked below 0.9 by the surface layer)
                assert v >= 0.9, (kind, x, y, v)
            n_fast += v >= 0.9
        assert n_fast >= len(sites) // 2, n_fast


DIGESTS = {
    "smoke": "98f026fa7d48fbed1634126051240d510bde6791f7934c5d145eda8290011b97",
    "precip_visual": "27ba1133258c8af9f4fdf52e11a22ad28e4ea9cff88180f2d97dd4fcda828445",
    "cloud": "c87989373e070d0225c0948aee58f8557fcdf305c979a7173a220c1e4dfcd805",
    "wall": "2efbebac38d68eb6b9be7207c37f64da4247ecda659f42656f45b5c30754514a",
    "fast_vx": "a2b7e3d605a9571275d22cfff47928fee10336e3adf6b0b9cd62286b08a566f6",
    "fast_vy": "ca6e8f2f7c2fa6e6098d7b9d06ca2293fb611f9e307e9084cb1e57a2948607c5",
    "droplet": "68daa1a2f65e79737a1a90c8c371b6c5824f7da9300ea2b6eaad54adf3c09c1c",
    "T_spike": "15f925e5d3dca2c556a24a9ee0f01381800f1c672793c75ab2c39391f37648c7",
    "P_spike": "574d8d11e71935882e817c46498d8435626708250dff9d3e6739a5110bd59e30",
}


def _digest(kind):
    X, Y = I.PHASE_GRID
    sc, bg = I.impulse_scene(X, Y, kind, offset=(3, 5)), I.impulse_scene(X, Y, kind, offset=(3, 5), plant=False)
    changed = {n: np.argwhere(np.asarray(p != q).reshape(Y, X, -1)).tolist() for n, p, q in zip(("base", "water", "wall"), sc, bg)}
    rec = {"sites": sc[4], "changed": changed, "values": [I.site_value(kind, k) for k in range(len(sc[4]))],
           "drops": None if sc[3] is None else sc[3].tolist()}
    return hashlib.sha256(json.dumps(rec, sort_keys=True).encode()).hexdigest()


@pytest.mark.parametrize("kind", I.KINDS)
def test_scenes_are_a_pure_function_of_their_arguments(kind):
    """Two builds are identical arrays; the sites, the cells a scene changes and what it plants there are pinned by digest."""
    X, Y = I.PHASE_GRID
    a, b = I.impulse_scene(X, Y, kind, offset=(3, 5)), I.impulse_scene(X, Y, kind, offset=(3, 5))
    for p, q in zip(a[:4], b[:4]):
        assert (p is None and q is None) or np.array_equal(p, q)
    assert a[4] == b[4] and a[4] != I.impulse_scene(X, Y, kind, offset=(4, 5))[4]
    assert _digest(kind) == DIGESTS[kind]
