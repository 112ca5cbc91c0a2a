"""Crafted inputs of tests/test_pool_exchange_gpu.py: droplet pools planted on every zone edge of small slab handles, and exchange
messages a peer could legally send. Pure numpy (no GPU): tests/test_pool_exchange_cpu.py asserts over this very list that every input is
in contract -- the kernels trust gid, position, key and count of what they are handed -- before any of it reaches a device.

Every crafted record has a NEGATIVE rec[1] (height), distinct per (droplet, rank): "kept" and "taken" can be told apart, and no read of a
record at a wrong offset could take a float's bits for a droplet index (they are negative as an int32)."""
import numpy as np

import pool_model as M

F = np.float32
Y, N, HALO = 16, 1000, 64
SENTINEL = 4096  # bytes behind every device buffer the tests hand out, checked to be untouched

# name -> (X_global, X_owned, x0 of every handle). "seam256": the left ghost columns of the first and the right ghost columns of the last
# handle wrap through the periodic seam (x0 = 128 only completes the partition for the one-owner check); "x192": Xg is no power of two,
# the float32 product (px / 2 + 0.5) * Xg rounds, and the local array is the whole domain; "wide512": owned columns that are in neither
# edge zone, or in one only
GEOS = {
    "seam256": (256, 64, (0, 64, 192, 128)),
    "x192": (192, 64, (0, 64, 128)),
    "wide512": (512, 192, (128,)),
}


def model(geo, k, n=N, rank=None):
    Xg, xo, x0s = GEOS[geo]
    return M.PoolModel(n, Xg, xo, x0s[k], HALO, k if rank is None else rank)


def px_of(col, Xg, frac=0.5):
    """float32 position of global column col + frac (frac 0: the nearest float32 to the column's left boundary)."""
    return F((np.float64(col) + frac) / Xg * 2.0 - 1.0)


def record(px, gid, active=True, rank=0, m0=None):
    """A droplet record whose channels 1, 3, 4 name (gid, rank): never equal to another crafted record of the same droplet."""
    if m0 is None:
        m0 = 0.5 + gid * 1e-4 if active else -2.5 - gid * 1e-3
    return np.array([px, -0.25 - gid * 1e-4 - rank * 0.03125, m0, 0.125 * (rank + 1), 1.0 + gid], F)


def zone_columns(geo):
    """Global columns of every zone edge of every handle of the geometry, and the first column outside each local array."""
    Xg, xo, x0s = GEOS[geo]
    X, h = xo + 2 * HALO, HALO
    local = [0, h - 1, h, 2 * h - 1, 2 * h, X - 2 * h - 1, X - 2 * h, X - h - 1, X - h, X - 1, -1, X]
    cols = []
    for x0 in x0s:
        cols += [(x0 - h + lc) % Xg for lc in local]
    return sorted(set(cols))


def zone_pool(geo, n=N, seed=5):
    """n droplets: on every zone-edge column its left boundary, one float32 step below it and the middle; px = -1 and +1; inactive records
    on the same columns; m0 = -0.0 (active); the rest random, a third of it active."""
    Xg = GEOS[geo][0]
    rng = np.random.Generator(np.random.Philox(seed))
    px, act = [], []
    for c in zone_columns(geo):
        b = px_of(c, Xg, 0.0)
        below = np.nextafter(b, F(-2.0), dtype=F) if b > -1 else np.nextafter(F(1.0), F(0.0), dtype=F)  # (below -1: the top of the last column)
        px += [b, below, px_of(c, Xg, 0.5)]
        act += [True, True, True]
    px += [F(-1.0), F(1.0)]
    act += [True, True]
    n_planted = len(px)
    assert n_planted + 40 <= n
    for c in zone_columns(geo)[:16]:  # inactive records where an active one would be somebody's
        px.append(px_of(c, Xg, 0.5))
        act.append(False)
    rest = n - len(px)
    px += list(rng.uniform(-1.0, 1.0, rest).astype(F))
    act += list(rng.random(rest) < 0.33)
    drops = np.stack([record(p, g, a) for g, (p, a) in enumerate(zip(px, act))])
    minus_zero = [n_planted - 3, n - 1, n - 2]  # a planted boundary droplet and two random ones: m0 = -0.0 is NOT < 0
    drops[minus_zero, 2] = F(-0.0)
    return drops


def overflow_pool(n=5000):
    """Every droplet active in the owned columns of the handle x0 = 64 of "seam256" (all of them lie in both edge zones)."""
    rng = np.random.Generator(np.random.Philox(17))
    cols = 64 + rng.integers(0, 64, n)
    return np.stack([record(px_of(c, 256, f), g) for g, (c, f) in enumerate(zip(cols, rng.uniform(0.05, 0.95, n)))])


# ---- pool_edges_apply: buffers for the handle x0 = 64 of "seam256" (local array: global columns 0 .. 191) ----
def edge_apply_entries():
    """[(gid, rec)]: droplets the zone pool has anywhere, handed over at owned columns (-> flag 2) and ghost columns (-> flag 3)."""
    cols = [64, 65, 100, 127, 0, 1, 63, 128, 129, 191, 90, 30, 150]
    return [(7 * k + 3, record(px_of(c, 256, 0.25 + 0.05 * (k % 10)), 7 * k + 3, True, rank=2)) for k, c in enumerate(cols * 6)]


# ---- pool_events_apply: 4 ranks, applied on rank 1 ----
KINDS = ("other_only", "mine_only", "first_flip", "more_flips", "later_stamp", "lower_rank", "mine_wins", "mine_loses")


def _event(gid, rank, first, count, last, Xg=256, active=None):
    col = (gid * 37 + rank * 11) % Xg
    active = (gid + rank) % 3 != 0 if active is None else active
    return (gid, M.make_key(first, count, last, rank), record(px_of(col, Xg, 0.3), gid, active, rank))


def arbitration(n=N, n_reported=800, seed=23):
    """per_rank[r] = shuffled [(gid, key, rec)] of 4 ranks, and the kind of every droplet's contest (None: no report)."""
    rng = np.random.Generator(np.random.Philox(seed))
    per_rank, kinds = [[] for _ in range(4)], [None] * n
    for g in range(n_reported):
        kind = KINDS[g % len(KINDS)]
        kinds[g] = kind
        a, b, c = [(0, 2, 3), (2, 3, 0), (3, 0, 2)][(g // len(KINDS)) % 3]  # three ranks that are not rank 1, in turn
        f = g % 9  # first flip 0 .. 8
        if kind == "other_only":
            reports = [(a, f, 1, f + 1)]
        elif kind == "mine_only":
            reports = [(1, f, 1, f + 1)]
        elif kind == "first_flip":    # earlier first flip against more flips
            reports = [(a, f, 1, f + 6), (b, f + 2, 4, f + 6)]
        elif kind == "more_flips":    # equal first flip: more flips wins, although the other saw it later
            reports = [(a, f, 2, f + 6), (b, f, 3, f + 4), (c, f, 1, f + 6)]
        elif kind == "later_stamp":   # equal first flip and count: the later last stamp wins
            reports = [(a, f, 2, f + 3), (b, f, 2, f + 5)]
        elif kind == "lower_rank":    # all equal: the lower rank wins
            reports = [(a, f, 2, f + 3), (b, f, 2, f + 3), (c, f, 2, f + 3)][:2 + (g // len(KINDS)) % 2]
        elif kind == "mine_wins":     # rank 1 the winner against a different record of rank 3: kept
            reports = [(1, f, 1, f + 2), (3, f + 3, 1, f + 4)]
        else:                         # rank 1 the loser: taken
            reports = [(1, f + 4, 1, f + 5), (a, f, 1, f + 5)]
        for r, first, count, last in reports:
            per_rank[r].append(_event(g, r, first, count, last))
    for r in range(4):
        order = rng.permutation(len(per_rank[r]))
        per_rank[r] = [per_rank[r][k] for k in order]
    for r in (0, 2):  # a period / iteration record at entry 0: ignored by best / apply / reset
        per_rank[r].insert(0, (-1, r, np.array([0.5, -0.5, 7.0 + r, 1.0, 0.0], F)))
    return per_rank, kinds


def second_call(n_reported=800):
    """After ``arbitration``: one report per "other_only" droplet, from rank 3, with a LARGER key than the first call's winner."""
    per_rank = [[] for _ in range(4)]
    for g in range(0, n_reported, len(KINDS)):
        gid, key, rec = _event(g, 3, 12, 1, 13)
        rec[3] = F(77.0)
        per_rank[3].append((gid, key, rec))
    return per_rank


def largest_count(per_rank):
    return max(len(e) for e in per_rank)


def strides(per_rank, event_bytes):
    """Whole buffers, the 4 KiB-rounded stride of the hosts, the exact minimum."""
    most = largest_count(per_rank)
    return [0, min(event_bytes, (M.POOL_HDR + most * M.EVENT_BYTES + 4095) // 4096 * 4096), M.POOL_HDR + most * M.EVENT_BYTES]


def clamped(cap=100, excess=30):
    """4 ranks at the stride of ``cap`` entries; rank 2 reports cap + excess: its header says so, its first cap entries are in the message.
    (Rank 3 follows it in the message with retirements only: inactive records.)"""
    per_rank = [[_event(g, r, g % 9, 1, g % 9 + 1, active=False if r == 3 else None) for g in range(200 * r, 200 * r + 60)] for r in range(4)]
    per_rank[2] = [_event(g, 2, g % 9, 1, g % 9 + 1) for g in range(400, 400 + cap + excess)]
    stride = M.POOL_HDR + cap * M.EVENT_BYTES
    counts = [None, None, cap + excess, None]
    return M.events_message([e[:cap] for e in per_rank], stride, counts), stride, per_rank


def later_trips(n=20000):
    """One rank reports every droplet (more entries than the apply grid's 64 x 256 threads), another 300 better keys among the last 3000."""
    rng = np.random.Generator(np.random.Philox(29))
    all_of_them = [_event(int(g), 0, 5, 1, 6) for g in rng.permutation(n)]
    better = [_event(int(g), 2, 2, 1, 6) for g in n - 3000 + rng.permutation(3000)[:300]]
    return [all_of_them, [], better]


def many_ranks(n_ranks=70, over_rank=None):
    """70 buffers of stride 80 (2 entries each), distinct droplets; over_rank's header says 3."""
    per_rank = [[_event(2 * r + k, r, 1, 1, 2) for k in range(2)] for r in range(n_ranks)]
    counts = [3 if r == over_rank else None for r in range(n_ranks)]
    return M.events_message(per_rank, 80, counts), 80, per_rank


# ---- exact mode: the crafted buffers of ranks 0, 2, 3 around the handle's own (rank 1) ----
def exact_case(name, it):
    """per_rank entries of ranks 0, 2, 3 for iteration ``it`` (>= 1; "stale" needs >= 3 for a positive time): iteration records (gid -1 at
    entry 0)."""
    it = float(it)
    rec = lambda x, y, t, w: (-1, 0, np.array([x, y, t, w, 0.0], F))
    none = rec(0, 0, 0, 0)
    if name == "accepted":          # one request inside the window
        r0, r2, r3 = rec(0.25, -0.5, it, 3.0), none, none
    elif name == "two_requests":    # two in one iteration: the start times add up to 2 it > it
        r0, r2, r3 = rec(0.25, -0.5, it, 3.0), rec(-0.5, -0.25, it, 2.0), none
    elif name == "stale":           # older than max(it - 1, 1)
        r0, r2, r3 = none, rec(0.5, -0.5, it - 2.0, 1.0), none
    elif name == "sum_order":       # (1e8 + 1) - 1e8 = 0 in float32, 1e8 + (1 - 1e8) = 1: the order is rank 0, 2, 3
        r0, r2, r3 = rec(1e8, 1e8, it - 1.0, 1e8), rec(1.0, 1.0, 1.0, 1.0), rec(-1e8, -1e8, 0.0, -1e8)
    elif name == "sum_order_low_first":  # (1 + 1e8) - 1e8 = 0, but 1 + (1e8 - 1e8) = 1: told apart from the REVERSED order, too
        r0, r2, r3 = rec(1.0, 1.0, it - 1.0, 1.0), rec(1e8, 1e8, 1.0, 1e8), rec(-1e8, -1e8, 0.0, -1e8)
    else:
        raise KeyError(name)
    out = [[r0], [r2], [r3]]
    for k, e in enumerate(out):  # the record's key is the sender's rank
        e[0] = (-1, (0, 2, 3)[k], e[0][2])
    return out


EXACT_CASES = ("accepted", "two_requests", "stale", "sum_order", "sum_order_low_first")
EXACT_ACTIVE = (3, 250, 501, 777, 998)  # the handful of active droplets of the exact-mode pool


def exact_pool(n=N):
    """All inactive but a handful: heavy drops in the owned columns of the handle x0 = 64 of "seam256"."""
    drops = zone_pool("seam256", n)
    drops[:, 2] = -np.abs(drops[:, 2]) - F(1.0)
    for k, g in enumerate(EXACT_ACTIVE):
        drops[g] = record(px_of(70 + 10 * k, 256), g)
        drops[g, 1] = F(0.5)  # high above the ground
    return drops


def exact_winners(it):
    """Status flips of ranks 0, 2, 3 for the "winners" call: active winners inside and outside the local array of the handle x0 = 64
    (global columns 0 .. 191), inactive winners."""
    spec = [(40, 0, 10, True), (41, 0, 100, True), (42, 0, 170, True), (43, 2, 192, True), (44, 2, 255, True), (45, 3, 220, True),
            (46, 3, 191, True), (47, 0, 200, False), (48, 2, 64, False), (49, 3, 0, True)]
    per_rank = {r: [(-1, r, np.zeros(5, F))] for r in (0, 2, 3)}  # (every rank's iteration record: no request)
    for gid, r, col, active in spec:
        per_rank[r].append((gid, M.make_key(0, 1, 1, r), record(px_of(col, 256, 0.5), gid, active, r)))
    return [per_rank[0], per_rank[2], per_rank[3]]


# ---- period record through the library's transport: 3 slabs ----
PERIOD_CASES = {
    "latest": [(0.1, 0.2, 40.0, 1.0), (0.3, 0.4, 42.0, 2.0), (0.5, 0.6, 41.0, 3.0)],
    "equal_times": [(0.0, 0.0, 0.0, 0.0), (0.3, 0.4, 42.0, 2.0), (0.5, 0.6, 42.0, 3.0)],
    "not_positive": [(0.1, 0.2, -5.0, 1.0), (0.3, 0.4, 0.0, 2.0), (0.5, 0.6, 3.0, 3.0)],
    "all_zero": [(0.1, 0.2, 0.0, 1.0), (0.3, 0.4, 0.0, 2.0), (0.5, 0.6, 0.0, 3.0)],
}


# ---- the contract (tests/test_pool_exchange_cpu.py) ----
def check_pool(drops, n):
    drops = np.asarray(drops)
    assert drops.shape == (n, 5) and drops.dtype == F
    assert np.isfinite(drops).all() and (np.abs(drops[:, 0]) <= 1.0).all()


def check_events(raw, n_ranks, stride, n, record_ok=False):
    """Every header count >= 0; every entry a reader of ANY capacity up to the count could see inside the message has gid in [0, n) or
    exactly -1 (at entry 0 only), a key built from fields in their ranges, the sender's rank in it, a finite position in [-1, 1];
    no droplet twice in one rank's buffer."""
    assert len(raw) >= n_ranks * stride and stride >= M.POOL_HDR
    for r in range(n_ranks):
        cnt = M.read_count(raw, r * stride)
        assert cnt >= 0
        ev = M.read_events(raw, r * stride, M.event_cap(stride))
        gids = [int(g) for g in ev["gid"] if g >= 0]
        assert len(gids) == len(set(gids)), "a droplet twice in one rank's buffer"
        for k, e in enumerate(ev):
            if e["gid"] == -1:
                assert k == 0 and e["key"] == r and np.isfinite(e["rec"]).all()
                continue
            assert 0 <= e["gid"] < n
            first, count, last, rank = M.key_fields(e["key"])
            assert 0 <= first <= 14 and 1 <= count <= 15 and 1 <= last <= 15 and rank == r and e["key"] >= 0
            assert first < last and count <= last - first
            assert M.make_key(first, count, last, rank) == e["key"]
            assert np.isfinite(e["rec"]).all() and abs(e["rec"][0]) <= 1.0
            assert e["rec"][1] < 0, "crafted heights are negative (module docstring)"


def check_edges(raw, n, cap):
    assert len(raw) >= M.POOL_HDR + cap * M.EDGE_BYTES
    assert M.read_count(raw) >= 0
    er = M.read_edges(raw, cap)
    assert len(set(int(g) for g in er["gid"])) == len(er)
    for e in er:
        assert 0 <= e["gid"] < n and np.isfinite(e["rec"]).all() and abs(e["rec"][0]) <= 1.0 and not e["rec"][2] < 0


def crafted():
    """Every crafted input as (name, kind, payload): kind "pool" -> (drops, n); "events" -> (raw, n_ranks, stride, n); "edges" ->
    (raw, n, cap)."""
    out = []
    for geo in GEOS:
        out.append((f"zone_pool[{geo}]", "pool", (zone_pool(geo), N)))
    out.append(("overflow_pool", "pool", (overflow_pool(), 5000)))
    out.append(("exact_pool", "pool", (exact_pool(), N)))
    eb = M.POOL_HDR + N * M.EVENT_BYTES
    per_rank, _ = arbitration()
    for s in strides(per_rank, eb):
        out.append((f"arbitration[stride {s}]", "events", (M.events_message(per_rank, s or eb), 4, s or eb, N)))
    out.append(("second_call", "events", (M.events_message(second_call(), eb), 4, eb, N)))
    raw, stride, _ = clamped()
    out.append(("clamped", "events", (raw, 4, stride, N)))
    out.append(("capacity_zero", "events", (M.events_message([[], [], [], []], 16, [3, 0, 1, 0]), 4, 16, N)))
    out.append(("later_trips", "events", (M.events_message(later_trips(), M.POOL_HDR + 20000 * M.EVENT_BYTES), 3, M.POOL_HDR + 20000 * M.EVENT_BYTES, 20000)))
    for over in (None, 66):
        raw, stride, _ = many_ranks(over_rank=over)
        out.append((f"many_ranks[{over}]", "events", (raw, 70, stride, N)))
    for it in (2, 3, 7):
        for name in EXACT_CASES:
            per = exact_case(name, it)
            out.append((f"exact[{name}, it {it}]", "events", (M.events_message([per[0], [], per[1], per[2]], eb), 4, eb, N)))
        per = exact_winners(it)
        out.append((f"exact[winners, it {it}]", "events", (M.events_message([per[0], [], per[1], per[2]], eb), 4, eb, N)))
    ent = edge_apply_entries()
    gb = M.POOL_HDR + 4096 * M.EDGE_BYTES
    out.append(("edges_apply", "edges", (M.edges_buffer(ent, gb), N, 4096)))
    out.append(("edges_apply[count 0]", "edges", (M.edges_buffer([], gb), N, 4096)))
    return out


# ---- pool_events_pack: a scripted period on two slabs of 128 columns ----
PACK_X, PACK_Y, PACK_XO = 256, 48, 128
PACK_PERIOD = 1 + (HALO - 12) // 9  # WX_SLAB_PERIOD_PARTICLES(64): 6 iterations
PACK_EVENTS = {"spawn_rank0": (60, 2), "spawn_rank1": (200, 4), "retire_rank0": (66, 0), "retire_rank1": (192, 0)}  # name -> (column, iteration)


def pack_valid_columns(rank, j):
    """Global columns in which slab ``rank`` processes droplets in iteration j of the period: its owned columns and, of its 64 ghost columns
    on either side, the 58 - 9 j nearest (6 columns of the cone are used up by the first iteration, 9 by every further one). With two
    slabs of 128 in 256 columns EVERY column of the other slab is a ghost column: an event the other rank must not see -- it would
    report it, too, if a later spawn probe of that record fell into its owned columns -- has to lie in the middle of its rank's columns."""
    m = HALO - 6 - 9 * j
    return {c % PACK_X for c in range(rank * PACK_XO - m, (rank + 1) * PACK_XO + m)}


def pack_scene():
    """A tests/droplet_scenes.py scene on a 256 x 48 domain: one droplet spawns in iteration 2 of the period deep inside rank 0's owned
    columns, one in iteration 4 inside rank 1's, and a droplet of either rank evaporates in iteration 0; every event in columns the OTHER rank
    does not process in that iteration (pack_valid_columns). -> (scene, {name: droplet})."""
    import droplet_scenes as D
    import surface_scenes as S
    sc = D._Scene({"kind": "pool_pack", "X": PACK_X, "Y": PACK_Y, "offset": [0, 0], "lead": 0})
    y = sc.row_of(realT_above=D.ZERO_C)
    who = {}
    for k, name in enumerate(("spawn_rank0", "spawn_rank1")):
        x, it = PACK_EVENTS[name]
        sc.cloud(x, y - k, 8.0 + 0.25 * k)
        who[name] = len(sc.records)
        sc.probe({it: (x, y - k)}, {it: "spawn_rain"})
    for k, name in enumerate(("retire_rank0", "retire_rank1")):
        x, it = PACK_EVENTS[name]
        who[name] = len(sc.records)
        sc.active(x + 0.5, S.GROUND + 10 + k + 0.5, 0.03, 0.0, 1.0, {it: ("evaporated", "evaporated_rain")})
    return sc.finish(PACK_PERIOD, 7), who


def flip_history(records):
    """records[j] = the pool after j iterations (records[0]: before the first): per droplet the flip bits of the period -- bit j set: the
    sign of m0 changed in iteration j."""
    flips = np.zeros(len(records[0]), np.int64)
    for j in range(len(records) - 1):
        flips |= ((records[j][:, 2] < 0) != (records[j + 1][:, 2] < 0)).astype(np.int64) << j
    return flips
