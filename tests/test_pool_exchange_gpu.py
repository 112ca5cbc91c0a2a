"""The droplet pool's slab exchange kernels against their numpy model (tests/pool_model.py), BIT FOR BIT, on crafted pools and crafted
messages (tests/pool_cases.py; tests/test_pool_exchange_cpu.py holds every one of them to the kernels' contract). The public ABI takes
the exchange buffers as plain device pointers, so a test hands the kernels whatever a peer could legally send: every arbitration rule, the
capacity clamps, the later trips of the grid-stride loops and the column arithmetic at a slab edge and at the periodic seam are reached
on purpose, not when a simulated run happens to. Records are copied, never computed: there is no tolerance in this file."""
import numpy as np
import pytest

import pool_cases as PC
import pool_model as M

pytestmark = pytest.mark.gpu
F = np.float32
WX_E_INVALID, WX_E_STATE = -1, -5
FILL = 0xA5  # sentinel byte (as an int32 gid it is negative: skipped by every reader)


@pytest.fixture(scope="module")
def E(pkg):
    return pkg.engine


@pytest.fixture(scope="module")
def grids(pkg):
    made = {}

    def get(Xg):
        if Xg not in made:
            made[Xg] = pkg.synth.dry_grid(Xg, PC.Y)
            assert made[Xg][1][..., 1].max() == 0  # no cloud water: nothing spawns
        return made[Xg]
    return get


def _handle(E, grids, geo, k, drops, n=PC.N, rank=None):
    Xg, xo, x0s = PC.GEOS[geo]
    h = E.Handle(xo, PC.Y, n, X_global=Xg, x0=x0s[k], halo=PC.HALO)
    h.slab_set_rank(k if rank is None else rank)
    _upload(h, grids, geo, k, drops)
    return h


def _upload(h, grids, geo, k, drops):
    Xg, xo, x0s = PC.GEOS[geo]
    idx = (x0s[k] - PC.HALO + np.arange(xo + 2 * PC.HALO)) % Xg
    base, water, wall = grids(Xg)
    h.upload(np.ascontiguousarray(base[:, idx]), np.ascontiguousarray(water[:, idx]), np.ascontiguousarray(wall[:, idx]), drops)


def _model(geo, k, drops, n=PC.N, rank=None):
    m = PC.model(geo, k, n, rank)
    m.upload(drops)
    return m


def _dev(raw=None, nbytes=None):
    """A device buffer of nbytes (or len(raw)) bytes followed by PC.SENTINEL bytes of FILL."""
    import torch
    nbytes = len(raw) if nbytes is None else nbytes
    host = np.full(nbytes + PC.SENTINEL, FILL, np.uint8)
    host[:nbytes] = 0
    if raw is not None:
        host[:len(raw)] = raw
    return torch.from_numpy(host).to("cuda")


def _host(t, nbytes):
    """(the buffer's first nbytes bytes, "the sentinel behind them is intact")"""
    a = t.cpu().numpy()
    return a[:nbytes], bool((a[nbytes:] == FILL).all()) and len(a) == nbytes + PC.SENTINEL


def _assert_state(h, m, what=""):
    """Records (as bits) and flags of the handle equal the model's."""
    d, f = h.read_particles(), h.pool_flags()
    bad = np.nonzero((M.bits(d) != M.bits(m.drops)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first droplet {bad[0]}: {d[bad[0]]} model {m.drops[bad[0]]}"
    bad = np.nonzero(f != m.flags())[0]
    assert len(bad) == 0, f"{what}: {len(bad)} flags differ, first droplet {bad[0]}: {f[bad[0]]} model {m.flags()[bad[0]]} at px {d[bad[0], 0]!r}"


def _reports_state_error_once(E, h):
    """The next blocking call reports the overflow, the one after it is clean."""
    with pytest.raises(E.WxError) as ei:
        h.sync()
    assert ei.value.code == WX_E_STATE and "droplet-pool exchange buffer" in str(ei.value)
    h.sync()


def _edge_set(raw, cap):
    return sorted((int(e["gid"]), tuple(M.bits(e["rec"]).tolist())) for e in M.read_edges(raw, cap))


def _entry_set(entries):
    return sorted((int(g), tuple(M.bits(rec).tolist())) for g, rec in entries)


# ---- flags and upload-time ownership (pool_reset, k_pool_flags) ----
@pytest.mark.parametrize("geo", ["seam256", "x192"])
def test_flags_and_upload_ownership(E, grids, geo):
    """Droplets on every zone edge of every handle -- at the column's left boundary exactly, one float32 step below it, mid-column --, px =
    -1 and +1, inactive records and m0 = -0.0: the flags after the upload equal the model on every handle, and across the handles of the
    partition every active droplet has exactly one owner."""
    drops = PC.zone_pool(geo)
    flags = []
    for k in range(len(PC.GEOS[geo][2])):
        h = _handle(E, grids, geo, k, drops)
        _assert_state(h, _model(geo, k, drops), f"{geo} handle {k}")
        flags.append(h.pool_flags())
        h.close()
    flags = np.stack(flags)
    active = ~(drops[:, 2] < 0)
    assert np.array_equal((flags == 2).sum(0), active.astype(int)), "every active droplet has exactly one owner"
    assert (flags[:, ~active] == 1).all()
    assert (flags == 0).any() == (geo == "seam256") and (flags == 3).any()


# ---- pool_edges_pack ----
@pytest.mark.parametrize("geo", ["seam256", "x192"])
def test_edges_pack(E, grids, geo):
    """The left and right edge buffers -- count and the set of (gid, record); the order is the atomics' -- equal the model: a droplet
    within `halo` columns of both edges goes into both (every owned column of the 64-column handles), into one or none on the wide
    handle; a droplet outside the owned columns turns to flag 0; refresh_inactive = 1 packs the same; the sentinels stay intact."""
    todo = [(geo, k) for k in range(3)] + ([("wide512", 0)] if geo == "seam256" else [])
    for g, k in todo:
        drops = PC.zone_pool(g)
        h = _handle(E, grids, g, k, drops)
        packed = []
        for refresh in (0, 1):
            if refresh:
                _upload(h, grids, g, k, drops)
            m = _model(g, k, drops)
            nb = h.pool_edge_bytes()
            assert nb == m.edge_bytes()
            left, right = _dev(nbytes=nb), _dev(nbytes=nb)
            h.pool_edges_pack(left.data_ptr(), right.data_ptr(), bool(refresh))
            h.sync()
            want = m.edges_pack()
            got = []
            for side, (t, w) in enumerate(zip((left, right), want)):
                raw, intact = _host(t, nb)
                assert intact, (g, k, side)
                assert M.read_count(raw) == len(w), (g, k, side, refresh)
                assert _edge_set(raw, m.edge_cap) == _entry_set(w), (g, k, side, refresh)
                got.append(_edge_set(raw, m.edge_cap))
            _assert_state(h, m, f"{g} handle {k} refresh {refresh}")
            assert (h.pool_flags() == 0).sum() > (_model(g, k, drops).flags() == 0).sum(), "ghost copies outside the owned columns were demoted"
            packed.append(got)
            L, R = ({e[0] for e in s} for s in got)
            if g == "wide512":
                assert L - R and R - L and not (L & R), "one-sided zones"
                assert ((m.flags() == 2).sum() > len(L | R)), "owned droplets in neither zone"
            else:
                assert L == R and len(L) > 20, "both zones"
        assert packed[0] == packed[1]
        h.close()


def test_edges_pack_overflow_is_reported_by_the_receiver(E, grids):
    """5000 active droplets in one edge zone against the edge capacity of 4096: the header says 5000, exactly 4096 records are valid
    (distinct droplets, their records), nothing is written behind the buffer; the handle that APPLIES the buffer reports WX_E_STATE at
    its next blocking call, and the call after that is clean."""
    n = 5000
    drops = PC.overflow_pool(n)
    packer, taker = _handle(E, grids, "seam256", 1, drops, n), _handle(E, grids, "seam256", 0, drops, n)
    m = _model("seam256", 0, drops, n)
    nb = packer.pool_edge_bytes()
    assert nb == M.POOL_HDR + 4096 * M.EDGE_BYTES == m.edge_bytes()
    left, right = _dev(nbytes=nb), _dev(nbytes=nb)
    packer.pool_edges_pack(left.data_ptr(), right.data_ptr(), False)
    packer.sync()  # (the packer itself has nothing to report)
    for t in (left, right):
        raw, intact = _host(t, nb)
        assert intact and M.read_count(raw) == n
        er = M.read_edges(raw, 4096)
        assert len(er) == 4096 and len(set(er["gid"].tolist())) == 4096
        assert np.array_equal(M.bits(er["rec"]), M.bits(drops[er["gid"]]))
    raw, _ = _host(left, nb)
    taker.pool_edges_apply(left.data_ptr())
    m.edges_apply(raw)
    assert m.take_overflow() == n
    _reports_state_error_once(E, taker)
    _assert_state(taker, m, "receiver of the overflowed buffer")
    packer.close()
    taker.close()


# ---- pool_edges_apply ----
def test_edges_apply_crafted(E, grids):
    """Crafted edge buffers on the middle handle: the records land and `remote` clears -- the flag becomes 2 or 3 by position --; count 0
    changes nothing; the same entries in shuffled order give the same pool."""
    drops = PC.zone_pool("seam256")
    entries = PC.edge_apply_entries()
    gids = [g for g, _ in entries]
    h = _handle(E, grids, "seam256", 1, drops)
    m = _model("seam256", 1, drops)
    before = h.pool_flags()
    assert (before[gids] == 0).any() and (before[gids] == 1).any(), "the entries must clear a remote flag and replace an inactive record"
    nb = h.pool_edge_bytes()
    empty = _dev(M.edges_buffer([], nb))
    h.pool_edges_apply(empty.data_ptr())
    _assert_state(h, m, "count 0")
    results = []
    for order in (np.arange(len(entries)), np.random.Generator(np.random.Philox(2)).permutation(len(entries))):
        _upload(h, grids, "seam256", 1, drops)
        m = _model("seam256", 1, drops)
        raw = M.edges_buffer([entries[k] for k in order], nb)
        buf = _dev(raw)
        h.pool_edges_apply(buf.data_ptr())
        m.edges_apply(raw)
        _assert_state(h, m, "crafted edge buffer")
        f = h.pool_flags()
        assert set(f[gids].tolist()) == {2, 3}
        results.append((h.read_particles(), f))
    assert np.array_equal(M.bits(results[0][0]), M.bits(results[1][0])) and np.array_equal(results[0][1], results[1][1])
    h.sync()
    h.close()


# ---- pool_events_apply: arbitration ----
def test_events_apply_arbitration(E, grids):
    """Crafted buffers of 4 ranks applied on rank 1: one report (taken / kept), first flip against more flips, more flips, later last
    stamp, lower rank, rank 1 the winner (kept) and the loser (taken); entries shuffled, gid -1 records at entry 0 ignored, droplets
    without a report untouched. A second call whose only report for a droplet has a LARGER key than the first call's winner is applied:
    best[] was reset."""
    drops = PC.zone_pool("seam256")
    h = _handle(E, grids, "seam256", 1, drops, rank=1)
    m = _model("seam256", 1, drops, rank=1)
    per_rank, kinds = PC.arbitration()
    raw = M.events_message(per_rank, h.pool_event_bytes())
    assert h.pool_event_bytes() == m.event_bytes()
    buf = _dev(raw)
    h.pool_events_apply(buf.data_ptr(), 4, 0)
    m.events_apply(raw, 4)
    _assert_state(h, m, "first call")
    d = h.read_particles()
    kept = (M.bits(d) == M.bits(drops)).all(1)
    for g, kind in enumerate(kinds):
        assert kept[g] == (kind in (None, "mine_only", "mine_wins")), (g, kind)
    second = PC.second_call()
    raw2 = M.events_message(second, h.pool_event_bytes())
    buf2 = _dev(raw2)
    h.pool_events_apply(buf2.data_ptr(), 4, 0)
    m.events_apply(raw2, 4)
    _assert_state(h, m, "second call")
    d = h.read_particles()
    for g, key, rec in second[3]:
        assert np.array_equal(M.bits(d[g]), M.bits(rec)), f"droplet {g}: the second call's report was not applied"
    assert m.take_overflow() == 0
    h.sync()
    assert _host(buf, len(raw))[1] and _host(buf2, len(raw2))[1]
    h.close()


# ---- stride and clamp ----
def test_events_apply_strides_and_clamp(E, grids):
    """The same messages at stride 0 (whole buffers), at the hosts' 4 KiB-rounded stride and at the exact minimum give the same pool. A
    rank whose count exceeds the stride's capacity has exactly its first `cap` entries read (what follows them in the message is the next
    rank's buffer) and the handle reports WX_E_STATE once. Stride 16 (capacity 0) applies nothing. A stride above pool_event_bytes() or
    below 16 is refused with WX_E_INVALID and changes nothing."""
    drops = PC.zone_pool("seam256")
    h = _handle(E, grids, "seam256", 1, drops, rank=1)
    eb = h.pool_event_bytes()
    per_rank, _ = PC.arbitration()
    strides = PC.strides(per_rank, eb)
    assert strides[0] == 0 and eb > strides[1] > strides[2] > M.POOL_HDR
    results = []
    for stride in strides:
        _upload(h, grids, "seam256", 1, drops)
        m = _model("seam256", 1, drops, rank=1)
        raw = M.events_message(per_rank, stride or eb)
        buf = _dev(raw)
        h.pool_events_apply(buf.data_ptr(), 4, stride)
        m.events_apply(raw, 4, stride)
        _assert_state(h, m, f"stride {stride}")
        results.append(h.read_particles())
    assert all(np.array_equal(M.bits(r), M.bits(results[0])) for r in results)
    # a count above the stride's capacity
    _upload(h, grids, "seam256", 1, drops)
    m = _model("seam256", 1, drops, rank=1)
    raw, stride, sent = PC.clamped()
    buf = _dev(raw)
    h.pool_events_apply(buf.data_ptr(), 4, stride)
    m.events_apply(raw, 4, stride)
    assert m.take_overflow() == len(sent[2]) > M.event_cap(stride)
    _reports_state_error_once(E, h)
    _assert_state(h, m, "clamped")
    d = h.read_particles()
    for k, (g, key, rec) in enumerate(sent[2]):
        assert np.array_equal(M.bits(d[g]), M.bits(rec if k < M.event_cap(stride) else drops[g])), (k, g)
    # capacity 0
    state = h.read_particles(), h.pool_flags()
    raw = M.events_message([[], [], [], []], 16, [3, 0, 1, 0])
    buf0 = _dev(raw)
    h.pool_events_apply(buf0.data_ptr(), 4, 16)
    _reports_state_error_once(E, h)  # (counts of 3 and 1 against a capacity of 0)
    assert np.array_equal(M.bits(h.read_particles()), M.bits(state[0])) and np.array_equal(h.pool_flags(), state[1])
    # strides outside 16 .. pool_event_bytes()
    buf = _dev(M.events_message(per_rank, eb))
    for stride in (eb + 32, eb + 1, 15, 8):
        with pytest.raises(E.WxError) as ei:
            h.pool_events_apply(buf.data_ptr(), 4, stride)
        assert ei.value.code == WX_E_INVALID
    h.sync()
    assert np.array_equal(M.bits(h.read_particles()), M.bits(state[0])) and np.array_equal(h.pool_flags(), state[1])
    h.close()


# ---- later trips of the grid-stride loops ----
def test_events_apply_later_trips(E, grids):
    """20000 droplets, one rank reporting all of them -- more than the 64 x 256 threads of the apply grid -- and another with 300 better
    keys among the last 3000: every record equals the model."""
    n = 20000
    assert n > 64 * 256
    drops = PC.zone_pool("seam256", n)
    h = _handle(E, grids, "seam256", 1, drops, n, rank=1)
    m = _model("seam256", 1, drops, n, rank=1)
    per_rank = PC.later_trips(n)
    raw = M.events_message(per_rank, h.pool_event_bytes())
    buf = _dev(raw)
    h.pool_events_apply(buf.data_ptr(), 3, 0)
    m.events_apply(raw, 3)
    _assert_state(h, m, "later trips")
    d = h.read_particles()
    better = {g: rec for g, key, rec in per_rank[2]}
    assert len(better) == 300 and min(better) >= n - 3000 and max(better) >= 64 * 256
    for g, key, rec in per_rank[0][-4000:]:
        assert np.array_equal(M.bits(d[g]), M.bits(better.get(g, rec)))
    h.sync()
    h.close()


# ---- more ranks than one block of k_pool_check ----
def test_events_apply_checks_every_rank_of_70(E, grids):
    """70 buffers of stride 80 (capacity 2) applied on rank 0: the distinct droplets of ranks 0 .. 69 are all applied (rank 0's own kept).
    On a second handle rank 66's header says 3: its first two entries are applied and the next blocking call raises WX_E_STATE -- the
    header check covers every rank, not the first 64."""
    drops = PC.zone_pool("seam256")
    for over in (None, 66):
        h = _handle(E, grids, "seam256", 0, drops, rank=0)
        m = _model("seam256", 0, drops, rank=0)
        raw, stride, per_rank = PC.many_ranks(70, over)
        buf = _dev(raw)
        h.pool_events_apply(buf.data_ptr(), 70, stride)
        m.events_apply(raw, 70, stride)
        if over is None:
            assert m.take_overflow() == 0
            h.sync()
        else:
            assert m.take_overflow() == 3
            _reports_state_error_once(E, h)
        _assert_state(h, m, f"70 ranks, over {over}")
        d = h.read_particles()
        for r in range(70):
            for g, key, rec in per_rank[r]:
                assert np.array_equal(M.bits(d[g]), M.bits(drops[g] if r == 0 else rec)), (r, g)
        assert _host(buf, len(raw))[1]
        h.close()


# ---- exact mode ----
def _exact_handle(pkg, E, grids):
    drops = PC.exact_pool()
    h = _handle(E, grids, "seam256", 1, drops, rank=1)
    gui = pkg.params.merge_settings(None)
    u = pkg.params.uniforms_from_gui(gui, PC.Y, quad_scale=0)
    u["enablePrecipitation"] = 1
    u["inactiveDroplets"] = float(PC.N - len(PC.EXACT_ACTIVE))
    h.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
    h.set_option(h.OPT_POOL_EXACT, 1)
    return h, _dev(nbytes=h.pool_event_bytes())


def _exact_iteration(h, own, crafted):
    """One iteration, the handle's own buffer packed, the gathered message of 4 ranks (the handle is rank 1) applied -- the documented call
    order --, on the handle and on a model that starts from the handle's state: (model, it, message)."""
    eb = h.pool_event_bytes()
    h.step(1)
    h.pool_events_pack(own.data_ptr())
    h.sync()
    mine, intact = _host(own, eb)
    assert intact
    ev = M.read_events(mine)
    assert len(ev) >= 1 and ev[0]["gid"] == -1 and ev[0]["key"] == 1, "the iteration record sits at entry 0"
    assert (ev["gid"][1:] >= 0).all() and ((ev["key"][1:] & M.RANK_MASK) == 1).all()
    it = h.iter - 1
    m = PC.model("seam256", 1, rank=1)
    m.drops, m.remote, m.lightning = h.read_particles(), h.pool_flags() == 0, h.lightning()
    raw = np.concatenate([M.events_buffer(crafted[0], eb), mine, M.events_buffer(crafted[1], eb), M.events_buffer(crafted[2], eb)])
    buf = _dev(raw)
    h.pool_events_apply(buf.data_ptr(), 4, 0)
    m.events_apply(raw, 4, exact=True, it=it)
    _assert_state(h, m, f"exact mode, iteration {it}")
    assert np.array_equal(M.bits(h.lightning()), M.bits(m.lightning)), (it, h.lightning(), m.lightning)
    return m, it


NO_REQUEST = [[(-1, r, np.zeros(5, F))] for r in (0, 2, 3)]


def test_exact_mode_requests(pkg, E, grids):
    """WX_OPT_POOL_EXACT, one iteration per call, each followed by pack and apply. One request inside the window [max(it - 1, 1), it] is
    accepted and lightning() equals it; two requests in one iteration sum to a time outside the window and are discarded; a stale request
    is discarded; three requests whose channels are 1e8, 1, -1e8 in rank order give the float32 sum taken in that order."""
    h, own = _exact_handle(pkg, E, grids)
    m, it = _exact_iteration(h, own, NO_REQUEST)  # (iteration 0: the window is empty)
    assert it == 0 and (h.lightning() == 0).all()
    m, it = _exact_iteration(h, own, PC.exact_case("accepted", 1))
    assert it == 1 and np.array_equal(h.lightning(), np.array([0.25, -0.5, 1.0, 3.0], F))
    accepted = h.lightning()
    m, it = _exact_iteration(h, own, PC.exact_case("two_requests", 2))
    assert it == 2 and np.array_equal(h.lightning(), accepted)
    m, it = _exact_iteration(h, own, PC.exact_case("stale", 3))
    assert it == 3 and np.array_equal(h.lightning(), accepted)
    m, it = _exact_iteration(h, own, PC.exact_case("sum_order", 4))
    assert it == 4 and np.array_equal(h.lightning(), np.array([0.0, 0.0, 4.0, 0.0], F))
    h.close()


def test_exact_mode_winners_and_sum_order(pkg, E, grids):
    """Exact mode: an active winner whose column is outside the local array becomes flag 0, inside it 2 or 3, an inactive winner 1. And
    the rank-order sum once more with the small term first: (1 + 1e8) - 1e8 = 0, where the reversed order gives 1."""
    h, own = _exact_handle(pkg, E, grids)
    _exact_iteration(h, own, NO_REQUEST)
    winners = PC.exact_winners(1)
    m, it = _exact_iteration(h, own, winners)
    f = h.pool_flags()
    seen = set()
    for ev in winners:
        for g, key, rec in ev:
            if g < 0:
                continue
            col = int(M.global_col_f32(rec[0], 256))
            want = 1 if rec[2] < 0 else (0 if col >= 192 else (2 if 64 <= col < 128 else 3))
            assert f[g] == want, (g, col, f[g], want)
            seen.add(want)
    assert seen == {0, 1, 2, 3}
    m, it = _exact_iteration(h, own, PC.exact_case("sum_order_low_first", 2))
    assert it == 2 and np.array_equal(h.lightning(), np.array([0.0, 0.0, 2.0, 0.0], F))
    h.close()


# ---- period record (the library's own transport) ----
def test_period_record_through_the_local_transport(pkg, E, grids):
    """wx_group_exchange on three slabs of one device: the latest strike is on every slab; equal start times keep the lowest rank's
    record; a slab whose start time is 0 or negative does not count; all zero leaves every slab as it was."""
    Xg = 192
    g = E.Group(3, Xg, PC.Y, halo=PC.HALO, devices=[0] * 3, transport=E.TRANSPORT_LOCAL, n_droplets=64)
    assert g.transport == E.TRANSPORT_LOCAL
    base, water, wall = grids(Xg)
    drops = pkg.synth.init_rain_drops(64)  # (all inactive)
    g.upload(base, water, wall, drops)
    gui = pkg.params.merge_settings(None)
    u = pkg.params.uniforms_from_gui(gui, PC.Y, quad_scale=0)
    u["enablePrecipitation"] = 1
    g.set_params(pkg.params.fill_struct(pkg.params.WxParams(), u), u["initial_T"])
    for name, recs in PC.PERIOD_CASES.items():
        for s, v in zip(g.slabs, recs):
            s.set_lightning(np.array(v, F))
        g.exchange()
        g.sync()
        for k, s in enumerate(g.slabs):
            want = M.lightning_latest(recs, np.array(recs[k], F))
            assert np.array_equal(M.bits(s.lightning()), M.bits(want)), (name, k, s.lightning(), want)
    g.close()


# ---- pool_events_pack: the key's fields ----
def test_events_pack_key_fields(pkg, E):
    """Two slabs of 128 columns driven for one period on a tests/droplet_scenes.py scene in which one droplet spawns in iteration 2 and
    one in iteration 4 of the period and two evaporate in iteration 0 (no spawn-and-retire within one iteration: classify; every event in
    columns the other rank does not process in that iteration: tests/test_pool_exchange_cpu.py holds the scene to it). First flip
    and flip count come from the UNDECOMPOSED handle stepped one iteration at a time; the last stamp is the period's length (the owning
    rank processes a record it holds in every iteration). The owning rank's packed events carry exactly those fields, its rank and its
    final record; the other rank packs nothing for them; the header counts the events; nothing is written behind the buffer; a second
    pack right after yields count 0 (the flips were cleared)."""
    import droplet_scenes as D
    sc, who = PC.pack_scene()
    X, Y, xo, per, n = PC.PACK_X, PC.PACK_Y, PC.PACK_XO, PC.PACK_PERIOD, len(sc["drops"])
    p = pkg.params.fill_struct(pkg.params.WxParams(), sc["u"])

    def prepare(h):
        h.set_params(p, sc["u"]["initial_T"])
        h.set_option(h.OPT_SPLAT_ORDER, 1)
        h.iter = sc["iter0"]
    whole = E.Handle(X, Y, n)
    whole.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
    prepare(whole)
    records = [whole.read_particles()]
    for j in range(per):
        whole.step(1)
        records.append(whole.read_particles())
        names = D.classify(records[-2], records[-1], whole.read_rect("BASE_DISP"), whole.read_rect("WATER_CUR"), sc["u"])
        assert not any("spawn_retire" in s for s in names), f"iteration {j}: a spawn and a retirement in one iteration"
    whole.close()
    flips = PC.flip_history(records)
    for name, k in who.items():
        assert flips[k] == 1 << PC.PACK_EVENTS[name][1], (name, flips[k])
    flipped = np.nonzero(flips)[0]
    assert len(flipped) == len(who), "the scene's four events and no other"
    col0 = M.global_col_f32(sc["drops"][:, 0], X)
    for r in range(2):
        h = E.Handle(xo, Y, n, X_global=X, x0=r * xo, halo=PC.HALO)
        h.slab_set_rank(r)
        idx = (r * xo - PC.HALO + np.arange(xo + 2 * PC.HALO)) % X
        h.upload(np.ascontiguousarray(sc["base"][:, idx]), np.ascontiguousarray(sc["water"][:, idx]), np.ascontiguousarray(sc["wall"][:, idx]), sc["drops"])
        prepare(h)
        h.step(per)
        eb = h.pool_event_bytes()
        assert eb == M.POOL_HDR + n * M.EVENT_BYTES
        buf = _dev(nbytes=eb)
        h.pool_events_pack(buf.data_ptr())
        h.sync()
        raw, intact = _host(buf, eb)
        assert intact
        final = h.read_particles()
        mine = [k for name, k in who.items() if name.endswith(f"rank{r}")]
        ev = M.read_events(raw)
        assert M.read_count(raw) == len(ev) == len(mine), (r, M.read_count(raw))
        assert sorted(ev["gid"].tolist()) == sorted(mine), "the owning rank's droplets and nothing of the other rank's"
        for e in ev:
            k = int(e["gid"])
            f = int(flips[k])
            want = M.make_key((f & -f).bit_length() - 1, bin(f).count("1"), per, r)
            assert int(e["key"]) == want, (r, k, M.key_fields(e["key"]), M.key_fields(want))
            assert np.array_equal(M.bits(e["rec"]), M.bits(final[k])) and e["pad"] == 0
            if sc["drops"][k, 2] >= 0:  # (a droplet that was active at the start lay in this rank's owned columns)
                assert r * xo <= col0[k] < (r + 1) * xo
        h.pool_events_pack(buf.data_ptr())
        h.sync()
        raw, intact = _host(buf, eb)
        assert intact and M.read_count(raw) == 0, "a second pack finds the flips cleared"
        h.close()
