"""The droplet pool's exchange model (tests/pool_model.py) and the crafted inputs of tests/test_pool_exchange_gpu.py (tests/pool_cases.py),
checked without a GPU: the key orders reports as the documented tuple, the float32 column arithmetic is what local_col() computes, the
buffer layout is the header's, and every crafted input is in the kernels' contract (they index by gid unchecked) before it can reach
a device."""
import itertools
import struct

import numpy as np
import pytest

import pool_cases as PC
import pool_model as M

F = np.float32


def test_key_orders_reports_as_the_documented_tuple():
    """Smallest key == smallest (first flip, -flip count, -last stamp, rank), over every history a period of at most 15 iterations
    allows -- also the combinations no real period produces -- and ranks from 0 to 1023. The key is injective and non-negative."""
    ranks = (0, 1, 2, 63, 64, 1023)
    combos = list(itertools.product(range(15), range(1, 16), range(1, 16), ranks))
    assert len(combos) == 15 * 15 * 15 * len(ranks)
    keys = np.array([M.make_key(*c) for c in combos], np.int64)
    tuples = [(f, -n, -l, r) for f, n, l, r in combos]
    assert (keys >= 0).all() and keys.max() < M.BEST_IDLE and len(set(keys.tolist())) == len(combos)
    by_key = [tuples[k] for k in np.argsort(keys, kind="stable")]
    assert by_key == sorted(tuples)
    for c, k in zip(combos[::97], keys[::97]):
        assert M.key_fields(k) == c
    # the key as k_pool_events_pack builds it from the flip bits and the droplet's meta byte
    assert M.key_of_flips(0b101000, 0x80 | 9, 5) == M.make_key(3, 2, 9, 5)


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _local_col_transcribed(px, Xg, xoff):
    """local_col(g, px / 2.0f + 0.5f) of csrc/wx_kernels.h, statement by statement: every float32 operation is the exactly rounded
    double operation rounded to float32 (innocuous double rounding for +, *, / of float32 operands)."""
    u = _f32(_f32(_f32(px) / 2.0) + 0.5)
    t = int(np.floor(_f32(u * _f32(float(Xg)))))
    r = t % Xg  # wrapmod
    lc = r - xoff
    return lc + Xg if lc < 0 else lc


@pytest.mark.parametrize("geo", list(PC.GEOS))
def test_float32_column_against_float64_and_the_transcription(geo):
    """Off the column boundaries the model's float32 column is the float64 column (the rounding of px / 2 + 0.5 and of the product stays
    below Xg * 2^-24 columns; positions nearer than Xg * 2^-22 to a boundary count as "on" it). On the boundaries -- where, with Xg no power
    of two, float32 and float64 may disagree -- it is what a transcription of local_col() gives."""
    Xg, xo, x0s = PC.GEOS[geo]
    px = PC.zone_pool(geo)[:, 0]
    rng = np.random.Generator(np.random.Philox(3))
    px = np.concatenate([px, rng.uniform(-1, 1, 4000).astype(F), [PC.px_of(c, Xg, 0.0) for c in range(Xg)],
                         [np.nextafter(PC.px_of(c, Xg, 0.0), F(2.0), dtype=F) for c in range(Xg)]]).astype(F)
    t64 = (px.astype(np.float64) / 2.0 + 0.5) * Xg
    off = np.abs(t64 - np.round(t64)) > Xg * 2.0 ** -22
    assert off.sum() > 4000 and (~off).sum() >= 2 * Xg
    got = M.global_col_f32(px, Xg)
    assert np.array_equal(got[off], np.floor(t64[off]).astype(np.int64) % Xg)
    if Xg == 192:
        assert (got[~off] != np.floor(t64[~off]).astype(np.int64) % Xg).any(), "this geometry is there because float32 rounds across a boundary"
    for x0 in x0s:
        m = M.PoolModel(8, Xg, xo, x0, PC.HALO)
        lc = m.local_col(px)
        assert np.array_equal(lc, [_local_col_transcribed(float(p), Xg, m.xoff) for p in px])
        assert lc.min() >= 0 and lc.max() < Xg
    assert M.global_col_f32(F(-1.0), Xg) == 0 and M.global_col_f32(F(1.0), Xg) == 0


def test_layout_constants_match_the_header():
    assert (M.POOL_HDR, M.EVENT_BYTES, M.EDGE_BYTES) == M.header_layout() == (16, 32, 24)
    assert M.EV.itemsize == M.EVENT_BYTES and M.ER.itemsize == M.EDGE_BYTES
    assert M.EV.fields["gid"][1] == 0 and M.EV.fields["key"][1] == 4 and M.EV.fields["rec"][1] == 8 and M.EV.fields["pad"][1] == 28
    assert M.ER.fields["gid"][1] == 0 and M.ER.fields["rec"][1] == 4
    assert M.event_cap(80) == 2 and M.event_cap(16) == 0 and M.event_cap(16 + 32 * 1000 + 31) == 1000
    m = PC.model("seam256", 1)
    assert (m.event_bytes(), m.edge_bytes()) == (16 + 1000 * 32, 16 + 4096 * 24)
    assert PC.model("seam256", 1, n=40000).edge_bytes() == 16 + 5000 * 24
    text = open(M.KERNELS_H).read()
    assert "first flip << 18 | (15 - number of flips) << 14 | (15 - last iteration processed) << 10 | rank" in text


CRAFTED = PC.crafted()


@pytest.mark.parametrize("name,kind,payload", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_every_crafted_input_is_in_contract(name, kind, payload):
    {"pool": PC.check_pool, "events": PC.check_events, "edges": PC.check_edges}[kind](*payload)


def test_the_contract_check_refuses_what_it_must():
    """The check itself: a gid of N, a gid below -1, a key field out of range, a position outside [-1, 1], a negative count."""
    eb = M.POOL_HDR + 4 * M.EVENT_BYTES
    good = (5, M.make_key(2, 1, 4, 0), PC.record(F(0.25), 5))
    PC.check_events(M.events_message([[good]], eb), 1, eb, 10)
    bad = [(10, good[1], good[2]), (-2, good[1], good[2]), (5, M.make_key(2, 1, 4, 0) | (20 << 18), good[2]), (5, good[1], PC.record(F(1.5), 5)),
           (5, M.make_key(2, 1, 4, 3), good[2])]
    for e in bad:
        with pytest.raises(AssertionError):
            PC.check_events(M.events_message([[e]], eb), 1, eb, 10)
    with pytest.raises(AssertionError):
        PC.check_events(M.events_message([[good]], eb, [-1]), 1, eb, 10)
    with pytest.raises(AssertionError):
        PC.check_events(M.events_message([[good]], eb)[:-8], 1, eb, 10)  # shorter than n_ranks * stride
    with pytest.raises(AssertionError):
        PC.check_pool(np.array([[1.25, 0, 1, 0, 0]], F), 1)


def test_crafted_pools_cover_every_zone_and_flag():
    """The planted pools reach what they are planted for: all four flags on every handle, both sides of every zone edge, and across the
    handles of a partition exactly one owner per active droplet."""
    for geo, (Xg, xo, x0s) in PC.GEOS.items():
        drops = PC.zone_pool(geo)
        flags = []
        for k in range(len(x0s)):
            m = PC.model(geo, k)
            m.upload(drops)
            f = m.flags()
            flags.append(f)
            lc = m.local_col(drops[m.active(), 0])
            X, h = m.X, PC.HALO
            for edge in (h, 2 * h, X - 2 * h, X - h):
                assert (lc == edge - 1).any() and (lc == edge % Xg).any(), (geo, k, edge)
            assert set(f.tolist()) == ({1, 2, 3} if X == Xg else {0, 1, 2, 3}), (geo, k)
        if geo != "wide512":
            owners = (np.stack(flags) == 2).sum(0)
            assert np.array_equal(owners, (~(drops[:, 2] < 0)).astype(int)), geo
    assert (PC.zone_pool("seam256")[:, 2] == 0).sum() == 3  # the -0.0 records


def test_arbitration_case_list_has_every_contest():
    """Every kind of contest is there, each with a winner the model takes or keeps as named."""
    per_rank, kinds = PC.arbitration()
    m = PC.model("seam256", 1, rank=1)
    m.upload(PC.zone_pool("seam256"))
    before = m.drops.copy()
    m.events_apply(M.events_message(per_rank, m.event_bytes()), 4)
    sent = {(g, k & M.RANK_MASK): rec for ev in per_rank for g, k, rec in ev if g >= 0}
    seen = set()
    for g, kind in enumerate(kinds):
        kept = np.array_equal(M.bits(m.drops[g]), M.bits(before[g]))
        if kind is None:
            assert kept and not any(gg == g for gg, _ in sent)
            continue
        seen.add(kind)
        assert kept == (kind in ("mine_only", "mine_wins")), (g, kind)
        if not kept:
            winners = [r for (gg, r), rec in sent.items() if gg == g and np.array_equal(M.bits(rec), M.bits(m.drops[g]))]
            assert len(winners) == 1 and winners[0] != 1
            if kind == "lower_rank":
                assert winners[0] == min(r for gg, r in sent if gg == g)
    assert seen == set(PC.KINDS)
    assert (m.best == M.BEST_IDLE).sum() == 800 and m.overflow == 0
    # the second call's key is larger than the first call's winner and is applied all the same
    second = PC.second_call()
    m.events_apply(M.events_message(second, m.event_bytes()), 4)
    for g, k, rec in second[3]:
        assert np.array_equal(M.bits(m.drops[g]), M.bits(rec))


def test_model_clamps_and_reports():
    raw, stride, per_rank = PC.clamped()
    m = PC.model("seam256", 1, rank=1)
    m.upload(PC.zone_pool("seam256"))
    before = m.drops.copy()
    m.events_apply(raw, 4, stride)
    assert m.take_overflow() == 130 and m.take_overflow() == 0 and m.seen_max == 130
    for k, (g, key, rec) in enumerate(per_rank[2]):
        assert np.array_equal(M.bits(m.drops[g]), M.bits(rec if k < 100 else before[g]))


def test_exact_resolve_sums_in_rank_order():
    m = PC.model("seam256", 1, rank=1)
    for name, want in (("sum_order", (0.0, 0.0, 4.0, 0.0)), ("sum_order_low_first", (0.0, 0.0, 4.0, 0.0)), ("accepted", (0.25, -0.5, 4.0, 3.0))):
        per = PC.exact_case(name, 4)
        m.lightning[:] = 0
        m.events_apply(M.events_message([per[0], [], per[1], per[2]], m.event_bytes()), 4, exact=True, it=4)
        assert np.array_equal(m.lightning, np.array(want, F)), name
    # the other orders of the same three records give other sums: the case can tell them apart
    a, b, c = F(1e8), F(1.0), F(-1e8)
    assert F(F(a + c) + b) == 1 and F(F(a + b) + c) == 0 and F(F(b + a) + c) == 0 and F(b + F(a + c)) == 1
    for name in ("two_requests", "stale"):
        per = PC.exact_case(name, 4)
        m.lightning[:] = (9, 9, 9, 9)
        m.events_apply(M.events_message([per[0], [], per[1], per[2]], m.event_bytes()), 4, exact=True, it=4)
        assert (m.lightning == 9).all(), name


def test_period_record_rule():
    state = np.array([7, 7, 7, 7], F)
    want = {"latest": PC.PERIOD_CASES["latest"][1], "equal_times": PC.PERIOD_CASES["equal_times"][1], "not_positive": PC.PERIOD_CASES["not_positive"][2],
            "all_zero": tuple(state)}
    for name, recs in PC.PERIOD_CASES.items():
        assert np.array_equal(M.lightning_latest(recs, state), np.array(want[name], F)), name


def test_pack_scene_has_its_events_where_the_gpu_test_expects_them(oracle):
    """The scripted period of the events-pack test on the CPU oracle: the planted droplets flip in their iterations, nothing else flips,
    no spawn and retirement fall into one iteration, and every active droplet lies where the other rank does not process droplets in that
    iteration (so that "the other rank packs nothing for it" is a property of the scene, not of luck)."""
    import droplet_scenes as D
    sc, who = PC.pack_scene()
    PC.check_pool(sc["drops"], len(sc["drops"]))
    o = oracle.OracleSim(PC.PACK_X, PC.PACK_Y, len(sc["drops"]))
    o.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
    o.set_params(dict(sc["u"], splat_order=1))
    o.iter = sc["iter0"]
    records = [o.field("DROPS")]
    for j in range(PC.PACK_PERIOD):
        o.step(1)
        records.append(o.field("DROPS"))
        names = D.classify(records[-2], records[-1], o.field("BASE_DISP"), o.field("WATER_CUR"), sc["u"])
        assert not any("spawn_retire" in s for s in names)
        for k in np.nonzero((records[-2][:, 2] >= 0) | (records[-1][:, 2] >= 0))[0]:  # active before or after: where it was processed
            rec = records[-2][k] if records[-2][k, 2] >= 0 else records[-1][k]
            col = int(M.global_col_f32(rec[0], PC.PACK_X))
            owner = col // PC.PACK_XO
            assert col in PC.pack_valid_columns(owner, j) and col not in PC.pack_valid_columns(1 - owner, j), (j, k, col)
    o.close()
    flips = PC.flip_history(records)
    assert {k: int(flips[k]) for k in np.nonzero(flips)[0]} == {k: 1 << PC.PACK_EVENTS[name][1] for name, k in who.items()}
    assert PC.PACK_PERIOD == 6 and len(sc["drops"]) == 24
