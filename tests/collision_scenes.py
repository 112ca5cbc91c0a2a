"""Colliding deposits in the DEFAULT splat order (fp32 atomics at the sprite's anchor): scenes in which sprites overlap, several droplets
share one anchor and sprites lie over the mailbox texels (0,0) / (1,0) -- what tests/droplet_scenes.py keeps apart by construction.

The oracle's splat_order 1 is the engine's own summation tree (anchors first, then the index-anchored 12 x 12 box sum); the default order
differs from it in ONE place, the order of the additions that land on the same anchor in the same channel. Hence the kinds:

  exact       (overlap, pair, mailbox, two_requests, tiny) every anchor receives at most TWO non-zero deposits per channel and iteration:
              fp32 addition commutes, so the default order equals the oracle's order 1 bit for bit, every field, coupled over 6 iterations;
  membership  n = 3 / 4 droplets on one isolated anchor: the atomics give SOME sequential sum, one of n!/2 values; the candidates come
              from the oracle run once per ordering of the colliding records' pool slots; one iteration is compared;
  dense       1500 droplets over 5 x 4 cells: the bound sum_box gamma(n_a + 7) S_a of oracle/wx_oracle.h (wxo_splat_audit), derived there.

A plain module on top of droplet_scenes (_Scene, background, uniforms, cell_pos, search_seeds, anchor_of) and
impulse_scenes.deposits_per_texel: numpy, no fixture, no GPU. tests/test_collision_cpu.py accounts for the case list on the oracle alone,
tests/test_collision_gpu.py runs it on the card."""
from __future__ import annotations

import itertools

import numpy as np

import droplet_scenes as D
import impulse_scenes as I
import surface_scenes as S
from droplet_scenes import _Scene, anchor_of, background, cell_pos, search_seeds, uniforms  # noqa: F401  (the building blocks, unchanged)

F = np.float32
deposits_per_texel = I.deposits_per_texel
GRIDS = {k: D.GRIDS[k] for k in ("ragged", "tiny")}  # 169 x 52 and 57 x 9: nothing larger
STX, STY = D.TILE
N_ITER = 6       # the feedback of iteration 0 has gone through the grid and back into the droplets
ITER0 = 7
CONFIGS = tuple(k for k in D.CONFIG_CYCLE if "splat_order" not in D.CONFIGS[k])  # the device runs the DEFAULT order under each
DELTAS = ((1, 0), (0, 1), (11, 11), (5, -7), (12, 0))  # anchor B - anchor A of an ``overlap``; (12, 0) touches without overlapping
PLACEMENTS = ("interior", "seam", "rim", "wrap", "ragged_tile")

# (rain, snow, density) of droplet A and droplet B of a group: always different masses
FLY = ((0.5, 0.0, 1.0), (0.3, 0.25, 0.6))
GROUND = ((0.5, 0.2, 0.8), (0.25, 0.35, 0.5))     # rain AND snow: both channels of acc2
RETIRE = ((0.03, 0.0, 1.0), (0.0, 0.02, 0.3))     # total mass < 0.04: evaporates where it is (vapour and heat feedback)
CROWD, CROWD_RECS = ((-5, -2), (-10, -4)), ((0.4, 0.1, 0.9), (0.15, 0.45, 0.4))  # two bystanders of an overlap's flights, relative to anchor A
OFFSETS_IN_ANCHOR = ((0.2, 0.3), (0.35, 0.15))    # positions of A and B relative to their anchor: xw in (q - 0.5, q + 0.5] has anchor q


def _inside(q, r, f, X, Y, neg=False, ground=False):
    """(xw, yw) of a point whose sprite has anchor (q, r), ``f`` from the anchor (mirrored to the low side with ``neg``: the position's
    cell is then (q - 1, r - 1) -- across a tile seam from its anchor when q % 64 == 0 / r % 16 == 0); on the rim the side inside the
    domain; ``ground``: the side that lies in the surface row (anchor rows 2 and 3 both have a half there)."""
    fx, fy = (-f[0], -f[1]) if neg else f
    fx = abs(fx) if q == 0 else (-abs(fx) if q == X else fx)
    fy = abs(fy) if r == 0 else (-abs(fy) if r == Y else fy)
    if ground:
        assert r in (SURFACE_ROW, SURFACE_ROW + 1)
        fy = abs(fy) if r == SURFACE_ROW else -abs(fy)
    return q + fx, r + fy


class _Groups(_Scene):
    """_Scene that remembers its collision groups: {"kind", "slots", "anchors" (of the event iteration), "variant"}."""

    def __init__(self, c, **kw):
        super().__init__(c, **kw)
        self.groups = []

    def plant(self, q, r, f, rec, name, neg=False):
        xw, yw = _inside(q, r, f, self.X, self.Y, neg, name == "ground")
        k = len(self.records)
        self.active(xw, yw, *rec, {0: (name,)}, site=(min(q, self.X - 1), min(r, self.Y - 1)))
        return k

    def group(self, kind, variant, anchors, recs, names, neg=False, cloud=0.0):
        slots = []
        for i, ((q, r), rec, name) in enumerate(zip(anchors, recs, names)):
            if cloud:
                self.cloud(min(q, self.X - 1), min(r, self.Y - 1), cloud)
            slots.append(self.plant(q, r, OFFSETS_IN_ANCHOR[i % 2] if len(anchors) <= 2 else (0.4 - 0.22 * i, 0.1 + 0.1 * i), rec, name, neg))
        self.groups.append({"kind": kind, "variant": variant, "slots": slots, "anchors": [tuple(a) for a in anchors]})

    def finish(self, n_iter=N_ITER, iter0=ITER0, event_at=0):
        out = super().finish(n_iter, iter0, event_at)
        out["groups"] = self.groups
        return out


def _variant_group(sc, kind, variant, a, b):
    """Two droplets with anchors a and b (a == b: a ``pair``) doing what ``variant`` says in iteration 0."""
    if variant in ("grow", "flight"):       # both fly through cloud water: growth (negative vapour feedback), heat
        sc.group(kind, variant, (a, b), FLY, ("flight", "flight"), neg=sc.c.get("neg", False), cloud=1.5)
    elif variant == "dry":                  # both fly through the dry air: evaporation in flight
        sc.group(kind, variant, (a, b), FLY, ("flight", "flight"), neg=sc.c.get("neg", False))
    elif variant == "one_evap":             # one flies, one evaporates for good
        sc.group(kind, variant, (a, b), (FLY[0], RETIRE[1]), ("flight", "evaporated"), neg=sc.c.get("neg", False))
    elif variant == "retire":               # both evaporate for good, where they are: the only life inside the wall rows and on row Y
        sc.group(kind, variant, (a, b), RETIRE, ("evaporated", "evaporated"), neg=sc.c.get("neg", False))
    elif variant == "ground":               # both inside the surface row: two ground hits in one iteration, rain and snow each
        sc.group(kind, variant, (a, b), GROUND, ("ground", "ground"), neg=sc.c.get("neg", False))
    else:
        raise ValueError(variant)


SURFACE_ROW = S.GROUND - 1  # the flat background's surface cells: a droplet inside them hits the ground; its anchor row is 2 or 3


def _anchors_for(c):
    """Anchors (A, B) of the case's group from its placement, its delta (``pair``: (0, 0)) and its variant."""
    X, Y = c["X"], c["Y"]
    dx, dy = c.get("delta", (0, 0))
    place, ground = c["placement"], c["variant"] == "ground"
    if place == "interior":
        qa, ra = (90, 24) if Y > 12 else (30, 6)
    elif place == "seam":      # astride q = 63 | 64 and r = 15 | 16; a pair ON 64 / 16 with its position's cell on the other side
        qa = STX - (dx + 1) // 2 if dx else STX
        ra = (STY - (dy + 1) // 2 if dy > 0 else STY + (-dy) // 2) if dy else STY
    elif place == "ragged_tile":  # the accumulation grid's last tile column (128 ..) and row (48 ..)
        qa, ra = 150, (Y - dy if dy > 1 else (Y - 1 if dy < 0 else 49))  # (11, 11): B on anchor row Y; (5, -7): A on row Y - 1
    else:
        raise ValueError(place)
    if ground:
        assert dy in (0, 1)
        ra = SURFACE_ROW if dy else SURFACE_ROW + c.get("k", 0) % 2
    return (qa, ra), (qa + dx, ra + dy)


def _exact(c):
    kind, place, variant = c["kind"], c["placement"], c["variant"]
    X, Y = c["X"], c["Y"]
    if place == "wrap":  # a wind of 0.4 cells / iteration carries the droplets across x = 1 in iteration 0
        sc = _Groups(c, wind=0.4, fallSpeed=0.0)
        r = Y // 2  # (both start on anchor X, or on X and X - 1; the textures do not wrap, so the overlap ends with a sprite on either rim)
        sc.cloud(X - 1, r, 1.5)
        sc.cloud(0, r, 1.5)
        xb = X - 0.3 if kind == "pair" else X - 1.3  # A: X - 0.15 -> 0.25 (anchor X -> 0); B: -> 0.1 (the pair) or X - 0.9 (anchor X - 1 still)
        slots = []
        for xw, yw, rec in zip((X - 0.15, xb), (r + 0.2, r + 0.35), FLY):
            slots.append(len(sc.records))
            sc.active(xw, yw, *rec, {0: ("flight",)})
        sc.groups.append({"kind": kind, "variant": variant, "slots": slots, "anchors": [(0, r), (0, r) if kind == "pair" else (X - 1, r)]})
        return sc.finish()
    sc = _Groups(c, fallSpeed=0.0)
    if place == "rim":  # q = 0, q = X, r = 0, r = Y: the domain clips the sprites
        d = 0 if kind == "pair" else 1
        if variant == "ground":
            _variant_group(sc, kind, "ground", (0, SURFACE_ROW), (d, SURFACE_ROW))
            _variant_group(sc, kind, "ground", (X - d, SURFACE_ROW + 1), (X, SURFACE_ROW + 1))
        else:
            ra = Y // 2 - 6
            _variant_group(sc, kind, "dry" if kind == "overlap" else "flight", (0, ra), (d, ra))
            _variant_group(sc, kind, "grow" if kind == "overlap" else "one_evap", (X - d, ra + 14), (X, ra + 14))
            _variant_group(sc, kind, "retire", (40, 0), (40, d))
            _variant_group(sc, kind, "retire", (100, Y - d), (100, Y))
        return sc.finish()
    a, b = _anchors_for(c)
    _variant_group(sc, kind, variant, a, b)
    if c.get("crowd"):
        # two more flying sprites over the same texels, five and ten anchors to the left: no deposit shares an anchor with another, yet
        # some texels' 12-windows hold three non-zero anchors, one per quad of tree12 -- where the ASSOCIATION of the box sum decides the
        # last bit (with two sprites alone every texel's sum has two non-zero operands, and any tree gives the same bits)
        sc.group("crowd", "dry", [(a[0] + dx, a[1] + dy) for dx, dy in CROWD], CROWD_RECS, ("flight", "flight"))
    return sc.finish()


def _mailbox(c):
    """A sprite (``single``) or two on one anchor (``pair``) over texels (0,0) and (1,0), into which the inactive records are counted and
    (``lightning``) a granted request is filed in the same iteration."""
    mode = c["variant"]
    sc = _Groups(c, fallSpeed=0.0)
    a = (4, S.GROUND + 2)  # the sprite covers columns -2 .. 9 and rows -1 .. 10
    iter0 = ITER0
    if "lightning" in mode:
        iter0 = 40  # (the gate lightning[2] < iterNum - 30 is open)
        x, y = 30 + (c["X"] - 60) // 2, sc.row_of(realT_below=D.ZERO_C)
        sc.cloud(x, y, 2.0, precip=400.0, r=0)
        sc.probe({0: (x, y)}, {0: "spawn_held"})
    if mode.startswith("single"):
        sc.group("single", mode, (a,), FLY[:1], ("flight",))
    else:
        sc.group("pair", mode, (a, a), FLY, ("flight", "flight"))
    out = sc.finish(N_ITER, iter0)
    out["lightning_mode"] = "covered" if "lightning" in mode else None
    return out


def _two_requests(c):
    """Two snow spawns into cells with 400 units of precipitation in ONE iteration: both file a lightning request; texel (1,0) holds their
    sum, a two-operand sum per channel. (Its iteration channel is then about twice the iteration number: the update discards it.)"""
    sc = _Groups(c)
    y = sc.row_of(realT_below=D.ZERO_C)
    for k, x in enumerate((20 + c["X"] // 8, c["X"] - 20)):
        sc.cloud(x, y - k, 2.0 + 0.5 * k, precip=400.0, r=0)
        sc.probe({c["lead"]: (x, y - k)}, {c["lead"]: "spawn_held"})
    return sc.finish(N_ITER, 40, c["lead"])


TINY_MASSES = (1e-36, 3e-37)  # evaporating: the vapour feedback mass / 144 is subnormal
TINY_RAIN = 5e-39             # a ground hit's rain, itself subnormal (the snow makes it a ground hit: total mass >= 0.04)


def _tiny(c):
    """Subnormal deposits: one evaporating droplet of mass 1e-36, two (1e-36 and 3e-37) on one anchor, one ground hit with rain 5e-39."""
    sc = _Groups(c, fallSpeed=0.0)
    sc.group("single", "tiny_one", ((40, 30),), ((TINY_MASSES[0], 0.0, 1.0),), ("evaporated",))
    sc.group("pair", "tiny_two", ((90, 24), (90, 24)), ((TINY_MASSES[0], 0.0, 1.0), (0.0, TINY_MASSES[1], 0.3)), ("evaporated", "evaporated"))
    sc.group("single", "tiny_ground", ((140, SURFACE_ROW),), ((TINY_RAIN, 0.5, 0.3),), ("ground",))
    return sc.finish(2)


def _member(c):
    """n droplets on ONE isolated anchor; masses drawn from the case's generator (tests/test_collision_cpu.py shows that the draw
    separates the candidates in every non-zero channel)."""
    n, place, variant = c["n"], c["placement"], c["variant"]
    X, Y = c["X"], c["Y"]
    sc = _Groups(c, fallSpeed=0.0)
    a = {"interior": (90, 24), "seam": (STX, STY), "rim": (X, 30)}[place]
    if variant == "ground":
        a = (a[0], SURFACE_ROW + 1)
    if variant == "retire":
        a = (a[0], Y) if place == "rim" else a
    recs = []
    for _ in range(n):
        m = sc.rng.random(3, dtype=F)
        if variant == "retire":
            recs.append((F(0.004) + F(0.014) * m[0], F(0.004) + F(0.014) * m[1], F(0.3) + F(0.7) * m[2]))
        else:
            recs.append((F(0.1) + F(0.8) * m[0], F(0.1) + F(0.8) * m[1], F(0.3) + F(0.7) * m[2]))
    name = {"flight": "flight", "ground": "ground", "retire": "evaporated"}[variant]
    sc.group("member", variant, (a,) * n, recs, (name,) * n, neg=place == "seam", cloud=1.5 if variant == "flight" else 0.0)
    return sc.finish(1)


DENSE_N, DENSE_FILL = 1500, 12
DENSE_PATCH = (62, 1, 5, 4)  # x0, y0, columns, rows: astride the tile seam at q = 64, the surface row and the air above it


def _dense(c):
    """1500 active droplets over 5 x 4 cells astride the tile seam at column 64 -- rows 1 and 2 are land (ground hits: rain and snow),
    rows 3 and 4 the air above it (flights) -- drawn towards the middle of the patch, so that the busiest anchors take a few hundred."""
    sc = _Groups(c)
    x0, y0, w, h = DENSE_PATCH
    rng = sc.rng
    xs = np.clip(x0 + w / 2.0 + rng.standard_normal(DENSE_N) * 1.0, x0 + 0.01, x0 + w - 0.01)
    ys = np.clip(y0 + h / 2.0 + rng.standard_normal(DENSE_N) * 0.9, y0 + 0.01, y0 + h - 0.01)
    m = rng.random((DENSE_N, 3), dtype=F)
    for k in range(DENSE_N):
        px, py = cell_pos(float(xs[k]), float(ys[k]), sc.X, sc.Y)
        sc.records.append((px, py, F(0.05) + F(0.8) * m[k, 0], F(0.05) + F(0.8) * m[k, 1] * F(k % 3 != 0), F(0.3) + F(0.7) * m[k, 2]))
    sc.prepared[:y0 + h + 8, x0 - 8:x0 + w + 8] = True
    for _ in range(DENSE_FILL):
        sc.probe({}, None)
    sc.groups.append({"kind": "dense", "variant": "dense", "slots": list(range(DENSE_N)), "anchors": []})
    return sc.finish(2)


BUILDERS = {"overlap": _exact, "pair": _exact, "mailbox": _mailbox, "two_requests": _two_requests, "tiny": _tiny, "member": _member, "dense": _dense}
EXACT_KINDS = ("overlap", "pair", "mailbox", "two_requests")


def _case(kind, grid, i, **kw):
    X, Y = GRIDS[grid]
    c = {"kind": kind, "grid": grid, "X": X, "Y": Y, "config": CONFIGS[i % len(CONFIGS)], "lead": i % 2}
    c.update(kw)
    return c


def cases():
    """The exact cases: every delta of ``overlap`` and every variant of ``pair`` at the interior, astride the tile seams and on the ragged
    last tile column / row; both kinds on the rim (flights and evaporations; ground hits) and across the wrap seam; the mailbox kinds; two
    requests; a few on the tiny grid. The configuration walks with the running index, as droplet_scenes.CONFIG_CYCLE does."""
    out = []
    i = itertools.count()
    fly = ("grow", "dry", "ground")
    for pi, place in enumerate(("interior", "seam", "ragged_tile")):
        for di, delta in enumerate(DELTAS):
            v = fly[(di + pi) % 3]
            if v == "ground" and delta[1] not in (0, 1):
                v = "grow"
            out.append(_case("overlap", "ragged", next(i), placement=place, delta=delta, variant=v, k=di, crowd=v != "ground"))
        for vi, v in enumerate(("flight", "one_evap", "ground")):
            out.append(_case("pair", "ragged", next(i), placement=place, variant=v, neg=place == "seam", k=vi + pi))
    for kind in ("overlap", "pair"):
        for v in ("mixed", "ground"):
            out.append(_case(kind, "ragged", next(i), placement="rim", variant=v))
        out.append(_case(kind, "ragged", next(i), placement="wrap", variant="grow" if kind == "overlap" else "flight"))
    for v in ("single", "pair", "single_lightning", "pair_lightning"):
        out.append(_case("mailbox", "ragged", next(i), placement="mailbox", variant=v))
    for _ in range(2):
        out.append(_case("two_requests", "ragged", next(i), placement="mailbox", variant="two_requests"))
    out.append(_case("overlap", "tiny", next(i), placement="interior", delta=(1, 0), variant="grow"))
    out.append(_case("overlap", "tiny", next(i), placement="interior", delta=(0, 1), variant="ground"))
    out.append(_case("pair", "tiny", next(i), placement="interior", variant="flight"))
    out.append(_case("pair", "tiny", next(i), placement="interior", variant="ground"))
    out.append(_case("mailbox", "tiny", next(i), placement="mailbox", variant="pair"))
    return out


def tiny_cases():
    return [_case("tiny", "ragged", i, placement="interior", variant="tiny") for i in (0, 4)]  # the marching and the per-pass kernel set


# which draw of the case's generator gives masses whose orderings differ in EVERY non-zero channel (searched once on the oracle, from 0
# upwards; tests/test_collision_cpu.py holds the list to it: a case whose draw stops separating fails there)
MEMBER_DRAWS = {("interior", 3): 173, ("interior", 4): 3, ("seam", 3): 7, ("seam", 4): 1, ("rim", 3): 9, ("rim", 4): 8}


def member_cases():
    """n = 3 (3 candidates) and n = 4 (12) at the interior, on the tile seam (anchor (64, 16), positions in tile (0, 0)) and on the rim."""
    out = []
    for pi, place in enumerate(("interior", "seam", "rim")):
        for ni, n in enumerate((3, 4)):
            out.append(_case("member", "ragged", 2 * pi + ni, placement=place, n=n, variant=("flight", "ground", "retire")[(pi + ni) % 3],
                             draw=MEMBER_DRAWS[place, n]))
    return out


def dense_case():
    return _case("dense", "ragged", 0, placement="seam", variant="dense")


def build_case(c):
    return BUILDERS[c["kind"]](c)


def case_id(c):
    d = c.get("delta")
    return f"{c['kind']}-{c['grid']}-{c['placement']}-{c['variant']}" + (f"-d{d[0]}_{d[1]}" if d else "") + (f"-n{c['n']}" if "n" in c else "") + f"-{c['config']}"


# ---- the oracle's account of a case (no GPU) ----
def oracle_for(wx_oracle, c, sc, drops=None):
    """The oracle in splat_order 1 -- the engine's own summation tree -- whatever the device's configuration."""
    o = wx_oracle.OracleSim(c["X"], c["Y"], len(sc["drops"]))
    o.upload(sc["base"], sc["water"], sc["wall"], sc["drops"] if drops is None else drops)
    o.set_params(dict(sc["u"], splat_order=1))
    o.iter = sc["iter0"]
    if sc["lightning0"]:
        o.set_lightning(sc["lightning0"])
    return o


def run_audited(wx_oracle, c, sc=None, order0=False):
    """The oracle through the case in order 1 under the audit -> per iteration: droplets before / after, classify()'s names, the
    audit's count / least / exact / bound, the float textures, finiteness; with ``order0`` the textures of a second run in order 0."""
    sc = sc or build_case(c)
    X, Y = c["X"], c["Y"]
    o = oracle_for(wx_oracle, c, sc)
    o0 = None
    if order0:
        o0 = oracle_for(wx_oracle, c, sc)
        o0.set_params(dict(sc["u"], splat_order=0))
    rec = []
    try:
        for it in range(sc["n_iter"]):
            b = o.field("DROPS")
            with wx_oracle.SplatAudit(X, Y) as au:
                o.step(1)
            a, base = o.field("DROPS"), o.field("BASE_CUR")
            r = {"before": b, "after": a, "names": D.classify(b, a, o.field("BASE_DISP"), o.field("WATER_CUR"), sc["u"]),
                 "count": au.count.copy(), "least": au.least.copy(), "exact": au.exact.copy(), "bound": au.bound.copy(),
                 "fb": o.field("PRECIP_FB"), "dep": o.field("PRECIP_DEP"), "lightning": o.field("LIGHTNING"),
                 "finite": bool(np.isfinite(base).all() and np.isfinite(o.field("WATER_CUR")).all() and np.isfinite(a).all())}
            if o0 is not None:
                o0.step(1)
                r["fb0"], r["dep0"] = o0.field("PRECIP_FB"), o0.field("PRECIP_DEP")
            rec.append(r)
    finally:
        o.close()
        if o0 is not None:
            o0.close()
    return rec


# ---- membership ----
def footprint(q, r, X, Y):
    """Slices (rows, columns) of the texels an anchor's 12 x 12 sprite covers inside the X x Y textures."""
    return slice(max(0, r - 6), min(Y, r + 6)), slice(max(0, q - 6), min(X, q + 6))


def member_candidates(wx_oracle, c, sc):
    """-> (anchor, candidates, runs): per audit channel the set of footprint values (as float32 bit patterns) the oracle's order 1 gives
    over every ordering of the colliding records' pool slots; ``runs``: ordering -> (DROPS after, fb, dep) for the CPU test."""
    X, Y = c["X"], c["Y"]
    g = sc["groups"][0]
    slots, (q, r) = g["slots"], g["anchors"][0]
    rows, cols = footprint(q, r, X, Y)
    cand = [set() for _ in range(5)]
    runs = {}
    for perm in itertools.permutations(range(len(slots))):
        drops = sc["drops"].copy()
        for i, p in enumerate(perm):
            drops[slots[i]] = sc["drops"][slots[p]]
        o = oracle_for(wx_oracle, c, sc, drops)
        try:
            o.step(1)
            fb, dep, after = o.field("PRECIP_FB"), o.field("PRECIP_DEP"), o.field("DROPS")
        finally:
            o.close()
        planes = [fb[..., 0], fb[..., 1], fb[..., 2], dep[..., 0], dep[..., 1]]
        for ch, pl in enumerate(planes):
            v = pl[rows, cols]
            assert (v == v.flat[0]).all(), (case_id(c), perm, ch)  # an isolated anchor: every texel of the footprint holds the anchor's sum
            cand[ch].add(int(v.reshape(-1)[:1].view(np.uint32)[0]))
        runs[perm] = (after, fb, dep)
    return (q, r), cand, runs


# ---- dense ----
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def planes_of(fb, dep):
    """The five audited channels of a pair of particle textures, [Y, X, 5] in double."""
    return np.concatenate([np.asarray(fb, np.float64)[..., :3], np.asarray(dep, np.float64)], axis=-1)


def within_bound(fb, dep, exact, bound):
    """-> (ok, worst): |out - exact| <= bound texel by texel; the two mailbox texels take one more rounding, u |out|."""
    out = planes_of(fb, dep)
    b = bound.copy()
    b[0, :2, :3] += U * np.abs(out[0, :2, :3])
    err = np.abs(out - exact)
    bad = err > b
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return not bad.any(), float(ratio.max())
