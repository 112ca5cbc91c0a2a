"""The accounting of the collision suite (tests/collision_scenes.py; tests/test_collision_gpu.py runs the same lists on the card), computed
from the case lists and the oracle's own outputs under its splat audit (wxo_splat_audit: per anchor and channel the number of non-zero
deposits, the exact sums, the derived bound). Nothing is asserted by hand: every exact case has at most two non-zero deposits per anchor
and channel in every iteration -- the condition under which fp32 atomics in any order equal the oracle's order 1 bit for bit --, the
collisions happen where the case says, the membership anchors are isolated and their orderings differ, the dense scene is dense and the
reference alone passes its bound. No GPU."""
import math

import numpy as np
import pytest

import collision_scenes as K
import droplet_scenes as D

CASES = K.cases()
TINY = K.tiny_cases()
F = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def runs(oracle):
    """Every exact case (and the subnormal ones) through the oracle once, in order 1 under the audit and in order 0 beside it."""
    out = {}
    for c in CASES + TINY:
        sc = K.build_case(c)
        out[K.case_id(c)] = (c, sc, K.run_audited(oracle, c, sc, order0=True))
    return out


def _exact(runs):
    return [v for v in runs.values() if v[0]["kind"] in K.EXACT_KINDS]


# ---- the condition of exactness ----
def test_at_most_two_nonzero_deposits_per_anchor_and_channel(runs):
    """Every iteration of every exact case and of the subnormal cases: n_a <= 2 from the audit; at most two lightning requests (their sum
    in the request slot commutes likewise); the inactive count is a sum of ones."""
    assert len(runs) == len(CASES) + len(TINY) == len({K.case_id(c) for c in CASES + TINY})
    for cid, (c, sc, rec) in runs.items():
        for it, r in enumerate(rec):
            assert r["count"].max() <= 2, (cid, it, int(r["count"].max()))
            assert sum("spawn_held" in n for n in r["names"]) <= 2, (cid, it)
            assert r["fb"][0, 0, 3] == 0 and abs(r["exact"][0, 0, 0] - float(r["fb"][0, 0, 0])) < 1e-4, (cid, it)


def test_collisions_happen_where_the_case_says(runs):
    """Iteration 0: every group's droplets do what the variant names and their sprites have the planned anchors; a pair's anchor holds
    TWO deposits (in the channels its variant feeds), an overlap's anchors one each, at the planned distance."""
    for cid, (c, sc, rec) in runs.items():
        r = rec[0]
        for g in sc["groups"]:
            for k, want in zip(g["slots"], g["anchors"]):
                assert set(sc["expect"][k][0]) <= r["names"][k], (cid, k, sc["expect"][k], r["names"][k])
                assert D.anchor_of(r["after"][k], c["X"], c["Y"]) == want, (cid, k, D.anchor_of(r["after"][k], c["X"], c["Y"]), want)
            if g["kind"] == "pair":
                q, rr = g["anchors"][0]
                assert g["anchors"][0] == g["anchors"][1] and r["count"][rr, q].max() == 2, (cid, r["count"][rr, q])
                a, b = (sc["drops"][k] for k in g["slots"])
                assert (a[:2] != b[:2]).all() and a[2] + a[3] != b[2] + b[3], cid  # different positions inside the anchor, different masses
                if g["variant"] == "ground":
                    assert (r["count"][rr, q, 3:] == 2).all() and (r["count"][rr, q, :3] == 0).all(), cid  # rain AND snow, twice
                if g["variant"] in ("flight", "dry", "grow"):
                    assert (r["count"][rr, q, :3] == 2).all(), cid
            if g["kind"] == "overlap":
                (qa, ra), (qb, rb) = g["anchors"]
                if c["placement"] != "wrap":
                    d = (qb - qa, rb - ra)
                    assert d == tuple(c["delta"]) if "delta" in c else d in ((1, 0), (0, 1)), (cid, d)
                assert r["count"][ra, qa].max() == 1 == r["count"][rb, qb].max(), cid
                if g["variant"] == "ground":
                    assert (r["count"][ra, qa, 3:] == 1).all() and (r["count"][rb, qb, 3:] == 1).all(), cid
        # what the droplet life-cycle suite forbids by construction: texels that receive two and more deposits (a sprite and the inactive
        # count on texel (0,0) included); (12, 0) touches without overlapping
        if c["kind"] in ("overlap", "pair", "mailbox"):
            n = K.deposits_per_texel(r["before"], r["after"], c["X"], c["Y"])
            # ... and the overlap carried across the wrap seam ends with one sprite clipped by each rim: the textures do not wrap
            touching = c["kind"] == "overlap" and ((tuple(c.get("delta", ())) == (12, 0) and not c.get("crowd")) or c["placement"] == "wrap")
            assert (n == 1) if touching else (n >= 2), (cid, n)
        # pairs that fly go on colliding: the feedback of a collision is read back by droplets that collide again
        if c["kind"] == "pair" and c["variant"] == "flight":
            assert sum(int(x["count"].max()) == 2 for x in rec) >= 3, cid


def test_every_exact_case_runs_six_coupled_iterations(runs):
    for c, sc, rec in _exact(runs):
        assert len(rec) == K.N_ITER == sc["n_iter"], K.case_id(c)
        calls, compare = D.schedule(c["config"], sc["n_iter"], sc["event_at"])
        assert compare[-1] == K.N_ITER and len(compare) >= 2  # (a plain step of three iterations is compared at its end)


# ---- the case list ----
def _groups(runs, kind):
    for c, sc, rec in runs.values():
        if c["kind"] == kind:
            for g in sc["groups"]:
                if g["kind"] == kind:
                    yield c, sc, rec, g


def _placement_facts(c, sc, rec, g):
    """What the group's anchors and positions of iteration 0 show, as names."""
    X, Y = c["X"], c["Y"]
    out = set()
    qs, rs = [a[0] for a in g["anchors"]], [a[1] for a in g["anchors"]]
    pos = [D.texel_of(rec[0]["after"][k][:2], X, Y) for k in g["slots"]]
    if min(qs) < K.STX <= max(qs):
        out.add("astride_q63|64")
    if min(rs) < K.STY <= max(rs):
        out.add("astride_r15|16")
    for (q, r), (cx, cy, _) in zip(g["anchors"], pos):
        if q == K.STX and int(cx) == K.STX - 1:
            out.add("astride_q63|64")  # the anchor in tile column 1, the droplet's own cell in tile column 0
        if r == K.STY and int(cy) == K.STY - 1:
            out.add("astride_r15|16")
        for name, hit in (("q=0", q == 0), ("q=X", q == X), ("r=0", r == 0), ("r=Y", r == Y)):
            if hit:
                out.add(name)
        if q >= 2 * K.STX and r >= 3 * K.STY and X > 2 * K.STX and Y > 3 * K.STY and X % K.STX and Y % K.STY:
            out.add("ragged_tile")
    for k in g["slots"]:
        if abs(float(rec[0]["after"][k][0]) - float(rec[0]["before"][k][0])) > 1.0:
            out.add("wrapped")
    return out


PLACEMENT_NEEDS = {"interior": set(), "seam": {"astride_q63|64", "astride_r15|16"}, "rim": {"q=0", "q=X", "r=0", "r=Y"}, "wrap": {"wrapped"},
                   "ragged_tile": {"ragged_tile"}}


def test_every_placement_is_met_by_an_overlap_and_a_pair_and_none_is_spare(runs):
    for kind in ("overlap", "pair"):
        seen = {p: set() for p in K.PLACEMENTS}
        for c, sc, rec, g in _groups(runs, kind):
            seen[c["placement"]] |= _placement_facts(c, sc, rec, g)
        for p, need in PLACEMENT_NEEDS.items():
            assert need <= seen[p], (kind, p, need - seen[p])
        assert {c["placement"] for c in CASES if c["kind"] == kind} == set(K.PLACEMENTS), kind
    # none is spare: dropping a placement's cases loses facts no other placement shows
    for p, need in PLACEMENT_NEEDS.items():
        for kind in ("overlap", "pair"):
            other = set()
            for c, sc, rec, g in _groups(runs, kind):
                if c["placement"] != p:
                    other |= _placement_facts(c, sc, rec, g)
            assert not need or need - other, (kind, p)


def test_deltas_variants_and_configurations():
    for p in ("interior", "seam", "ragged_tile"):
        assert {tuple(c["delta"]) for c in CASES if c["kind"] == "overlap" and c["placement"] == p and c["grid"] == "ragged"} == set(K.DELTAS), p
        assert {c["variant"] for c in CASES if c["kind"] == "pair" and c["placement"] == p} == {"flight", "one_evap", "ground"}, p
    assert {c["variant"] for c in CASES if c["kind"] == "overlap"} >= {"grow", "dry", "ground"}
    assert {c["variant"] for c in CASES if c["kind"] == "mailbox"} == {"single", "pair", "single_lightning", "pair_lightning"}
    for kind in ("overlap", "pair"):  # marching and per-pass kernel set; display, plain and MORE_TO_COME iterations
        assert {c["config"] for c in CASES if c["kind"] == kind} == set(K.CONFIGS), kind
    assert set(K.CONFIGS) == {k for k, v in D.CONFIGS.items() if "splat_order" not in v} and len(K.CONFIGS) == 5
    assert {(c["X"], c["Y"]) for c in CASES} == {D.GRIDS["ragged"], D.GRIDS["tiny"]}
    assert all(len(K.build_case(c)["drops"]) == D.POOL for c in CASES[:3])


def test_order_1_and_order_0_differ_on_the_overlap_flights(runs):
    """Why the old comparison (the oracle in order 0) could not be exact: where three sprites overlap, the per-texel sum in droplet-index
    order and the box tree round differently. (Two sprites alone cannot show it: a two-operand sum has one rounding in any tree.)"""
    crowded = [(c, sc, rec) for c, sc, rec in runs.values() if c.get("crowd")]
    assert len(crowded) >= 10 and {c["placement"] for c, _, _ in crowded} == {"interior", "seam", "ragged_tile"}
    for c, sc, rec in crowded:
        assert any(not np.array_equal(r["fb"], r["fb0"]) for r in rec), K.case_id(c)
        assert any(g["kind"] == "crowd" for g in sc["groups"])


def test_mailbox_cases_put_sprites_counts_and_requests_on_the_same_texels(runs):
    n_granted = 0
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] == "mailbox"]:
        cid, r = K.case_id(c), rec[0]
        g = sc["groups"][-1]
        for q, rr in g["anchors"]:
            rows, cols = K.footprint(q, rr, c["X"], c["Y"])
            assert rows.start == 0 and cols.start == 0 and cols.stop >= 2, cid  # the sprite covers (0,0) and (1,0)
        n_inactive = sum(1 for n in r["names"] if n == {"idle"})
        assert n_inactive >= 10 and n_inactive < r["fb"][0, 0, 0] < n_inactive + 0.1, (cid, r["fb"][0, 0])  # the count and the sprite's share
        if "lightning" in c["variant"]:
            assert sum("spawn_held" in n for n in r["names"]) == 1 and r["fb"][0, 1, 3] >= F(0.01), cid
            assert np.array_equal(r["lightning"], r["fb"][0, 1]) and r["fb"][0, 1, 0] != r["fb"][0, 2, 0], cid  # granted: request + sprite share
            n_granted += 1
    assert n_granted == 2
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] == "two_requests"]:
        r = rec[sc["event_at"]]
        assert sum("spawn_held" in n for n in r["names"]) == 2, K.case_id(c)
        assert r["fb"][0, 1, 2] == F(2 * (sc["iter0"] + sc["event_at"])) - F(0.15) - F(0.15) or abs(r["fb"][0, 1, 2] - 2 * (sc["iter0"] + sc["event_at"])) < 0.5


# ---- finiteness, number ranges ----
def test_all_scenes_stay_finite(oracle, runs):
    for cid, (c, sc, rec) in runs.items():
        assert all(r["finite"] and np.isfinite(r["fb"]).all() and np.isfinite(r["dep"]).all() for r in rec), cid
    for c in K.member_cases() + [K.dense_case()]:
        assert all(r["finite"] for r in K.run_audited(oracle, c)), K.case_id(c)


def _smallest(rec):
    vals = [r["least"].min() for r in rec]
    for r in rec:
        for t in (r["fb"], r["dep"]):
            nz = np.abs(t[t != 0])
            if nz.size:
                vals.append(float(nz.min()))
    return min(vals)


def test_only_the_tiny_kind_meets_subnormals(oracle, runs):
    """The guard: every deposit and every non-zero texel of every other case is a normal fp32 number, so a flush of subnormals could be
    excused nowhere else; and the tiny kind does hold subnormal addends AND subnormal sums, in both textures."""
    for cid, (c, sc, rec) in runs.items():
        if c["kind"] != "tiny":
            assert _smallest(rec) >= FLT_MIN, (cid, _smallest(rec))
    for c in K.member_cases() + [K.dense_case()]:
        assert _smallest(K.run_audited(oracle, c)) >= FLT_MIN, K.case_id(c)
    for c, sc, rec in [v for v in runs.values() if v[0]["kind"] == "tiny"]:
        r = rec[0]
        assert (r["least"][[1, 2, 3]] < FLT_MIN).all() and r["least"][4] > FLT_MIN, r["least"]
        for g in sc["groups"]:
            q, rr = g["anchors"][0]
            rows, cols = K.footprint(q, rr, c["X"], c["Y"])
            v = r["dep"][rows, cols, 0] if g["variant"] == "tiny_ground" else r["fb"][rows, cols, 2]
            assert (v != 0).all() and (np.abs(v) < FLT_MIN).all(), (g["variant"], v.flat[0])
            if g["variant"] == "tiny_two":  # 1e-36 / 144 + 3e-37 / 144: a subnormal sum of two subnormal addends
                one = next(x for x in sc["groups"] if x["variant"] == "tiny_one")["anchors"][0]
                assert r["count"][rr, q, 2] == 2 and v.flat[0] > r["fb"][one[1], one[0], 2] > 0


# ---- membership ----
MEMBERS = K.member_cases()


@pytest.mark.parametrize("c", MEMBERS, ids=[K.case_id(c) for c in MEMBERS])
def test_membership_anchor_is_isolated_and_its_orderings_differ(oracle, c):
    sc = K.build_case(c)
    n, X, Y = c["n"], c["X"], c["Y"]
    r = K.run_audited(oracle, c, sc)[0]
    (q, rr), cand, runs_ = K.member_candidates(oracle, c, sc)
    g = sc["groups"][0]
    assert all(D.anchor_of(r["after"][k], X, Y) == (q, rr) for k in g["slots"])
    # isolated: the only anchor of the iteration that holds anything (so no other within 11 columns / rows), with n deposits
    hit = r["count"].max(-1) > 0
    assert hit.sum() == 1 and hit[rr, q] and r["count"][rr, q].max() == n
    nonzero = r["count"][rr, q] > 0
    assert nonzero.any()
    for ch in range(5):
        assert len(cand[ch]) <= math.factorial(n) // 2
        assert len(cand[ch]) >= 2 if nonzero[ch] else cand[ch] == {0}, (K.case_id(c), ch, cand[ch])
    # the droplet arithmetic does not depend on the pool slot: DROPS comes back permuted and otherwise identical
    ident = runs_[tuple(range(n))][0]
    assert len(runs_) == math.factorial(n)
    for perm, (after, fb, dep) in runs_.items():
        want = ident.copy()
        for i, p in enumerate(perm):
            want[g["slots"][i]] = ident[g["slots"][p]]
        assert np.array_equal(after, want), (K.case_id(c), perm)


def test_membership_list():
    assert {(c["placement"], c["n"]) for c in MEMBERS} == {(p, n) for p in ("interior", "seam", "rim") for n in (3, 4)}
    assert {c["variant"] for c in MEMBERS} == {"flight", "ground", "retire"}  # between them every channel


# ---- dense ----
def test_dense_scene_is_dense_and_the_reference_passes_its_bound(oracle):
    c = K.dense_case()
    sc = K.build_case(c)
    assert (c["X"], c["Y"]) == D.GRIDS["ragged"] and (sc["drops"][:, 2] >= 0).sum() == K.DENSE_N == 1500 and sc["n_iter"] == 2
    x0, y0, w, h = K.DENSE_PATCH
    assert (w, h) == (5, 4) and x0 < K.STX < x0 + w
    cx, cy, _ = D.texel_of(sc["drops"][:K.DENSE_N, :2], c["X"], c["Y"])
    assert cx.min() == x0 and cx.max() == x0 + w - 1 and cy.min() == y0 and cy.max() == y0 + h - 1
    rec = K.run_audited(oracle, c, sc)
    r = rec[0]
    n_max = int(r["count"].max())
    assert n_max >= 100, n_max
    assert (r["count"].reshape(-1, 5).max(0) >= 30).all(), r["count"].reshape(-1, 5).max(0)  # every channel, acc2's rain and snow too
    for it, r in enumerate(rec):
        ok, worst = K.within_bound(r["fb"], r["dep"], r["exact"], r["bound"])
        assert ok and 0 < worst < 1, (it, worst)  # the oracle's own order-1 float result: inside, and not identical to the exact planes
        # mass, rain, snow: all addends >= 0, so the bound is relative: at most gamma(max n_a + 7) of the exact value -- a few 1e-5, against
        # the 1 / n_a that one lost or doubled deposit moves
        g = K.gamma(int(r["count"].max()) + 7)
        for ch in (0, 3, 4):
            ex, b = r["exact"][..., ch].copy(), r["bound"][..., ch]
            if ch == 0:
                ex[0, 0] -= r["fb"][0, 0, 0] - 0  # (the count is no deposit)
                ex[0, 0] = max(ex[0, 0], 0.0)
            assert (ex >= 0).all() and (b <= g * ex * (1 + 1e-12)).all(), (it, ch)
        assert g < 2e-5 and 1.0 / int(r["count"].max()) > 100 * g
    assert rec[0]["fb"][0, 0, 0] == K.DENSE_FILL


def test_audit_changes_no_output(oracle):
    """The same case with and without the audit: identical textures and droplets; and the audit's exact planes are what the float
    textures round (within the bound) in every exact case's first iteration."""
    c = next(c for c in CASES if c["kind"] == "pair" and c["variant"] == "flight")
    sc = K.build_case(c)
    a = K.run_audited(oracle, c, sc)
    o = K.oracle_for(oracle, c, sc)
    try:
        for r in a:
            o.step(1)
            assert np.array_equal(o.field("PRECIP_FB"), r["fb"]) and np.array_equal(o.field("PRECIP_DEP"), r["dep"]) and np.array_equal(o.field("DROPS"), r["after"])
            assert K.within_bound(r["fb"], r["dep"], r["exact"], r["bound"])[0]
    finally:
        o.close()
