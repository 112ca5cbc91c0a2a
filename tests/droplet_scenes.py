"""Droplet life-cycle scenes: a quiet background (tests/surface_scenes.py: land, flat or stepped, under air at rest on the start
sounding), a pool of two dozen droplet records and grid cells prepared so that a CHOSEN event happens to a CHOSEN droplet at a CHOSEN
iteration -- a spawn, a lightning request, an evaporation, a ground hit with its deposit, the 600-iteration refresh of the inactive
count -- with every 12 x 12 sprite alone on its texels, so that the default splat order (fp32 atomics) may be compared with the oracle
bit for bit (impulse_scenes.deposits_per_texel <= 1 in every compared iteration: tests/test_droplet_cpu.py demands it of every case).

How an event is placed. An inactive droplet probes texel(random2d(m0, x + iter * 0.3754), random2d(m1, x + iter * 0.073162)): the
hash is restated here in numpy uint32 arithmetic (tests/test_droplet_cpu.py pins it to the oracle) and seeds m0 in [-10, -9), m1 in
[0, 1) are SEARCHED so that the probe of iteration k lands on the wanted texel and the probes of the other iterations miss every
prepared cell. Whether the probe spawns is made a property of the scene: the planted cloud water is far above the threshold and the
spawn chance (cloud - threshold) / (inactive + 10) * X * Y * spawnChanceMult is pushed above 1 (spawnChanceMult 1) or to 1e-7 and
below (inactiveDroplets 1e12), so fract((10 cloud)^2) never decides. The lightning branch is made certain the same way: 400 units of
precipitation in the cell put its chance (cloud + precipitation - 2.5) * 0.0033 above 1.

A plain module: numpy on top of surface_scenes / impulse_scenes, no fixture, no GPU. ``cases()`` is what tests/test_droplet_gpu.py
runs and what tests/test_droplet_cpu.py accounts for; ``classify`` names what happened to every droplet in one iteration from its
records before and after and from the grids the particle pass read.
"""
from __future__ import annotations

import zlib

import numpy as np

import impulse_scenes as I
import surface_scenes as S
import wxpkg

F = np.float32
PITCH = (73, 29)  # >= impulse_scenes.DROPLET_PITCH; 73 and 29 are prime: co-prime with the splat tile (64 x 16) and the wet strip (56)
POOL = 24         # records per scene
TILE, STRIP = I.SPLAT_TILE, I.WET_STRIP
GRIDS = {"ragged": (169, 52),   # 3 x 56 + 1: ragged strip, ragged tile column, ragged tile row
         "aligned": (192, 48),  # X % 64 == 0 and Y % 16 == 0: anchor column X / anchor row Y own a tile column / row of the accumulation grid alone
         "tiny": (57, 9),       # less than one tile, less than one strip
         "bands": (1100, 523)}  # the impulse droplet grid, under ROW_BANDS 0 / 1 / 2
ZERO_C = F(273.15)
HUGE_INACTIVE = 1.0e12  # inactiveDroplets that refuses every spawn: the chance is (cloud - threshold) * X * Y / 1e12 < 1e-6 ...
REFUSED_CLOUD = 3.17    # cloud water planted for the refused probes (far above either threshold: the chance, not the pre-test, refuses)


# ---- the hash, restated (csrc/wx_kernels.h hash_u32 / random2d; the oracle's wxo_hash / wxo_random2d) ----
def hash_u32(x):
    x = np.asarray(x, np.uint32).copy()
    x += x << np.uint32(10)
    x ^= x >> np.uint32(6)
    x += x << np.uint32(3)
    x ^= x >> np.uint32(11)
    x += x << np.uint32(15)
    return x


def random2d(sx, sy):
    """float32 in [0, 1): the low 23 bits of hash(bits(sx) + hash(bits(sy))) as the mantissa of a number in [1, 2), minus 1."""
    sx, sy = np.broadcast_arrays(np.atleast_1d(np.asarray(sx, F)), np.atleast_1d(np.asarray(sy, F)))
    h = hash_u32(np.ascontiguousarray(sx).view(np.uint32) + hash_u32(np.ascontiguousarray(sy).view(np.uint32)))
    h = (h & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)
    return h.view(F) - F(1.0)


def probe_coords(m0, m1, x, it):
    """Texture coordinates an inactive droplet (seeds m0, m1, position x) probes in iteration ``it`` (float32 throughout)."""
    x = np.asarray(x, F)
    return random2d(m0, x + F(it) * F(0.3754)), random2d(m1, x + F(it) * F(0.073162))


def probe_texel(m0, m1, x, it, X, Y):
    tc0, tc1 = probe_coords(m0, m1, x, it)
    return np.floor(tc0 * F(X)).astype(np.int64) % X, np.floor(tc1 * F(Y)).astype(np.int64) % Y


def search_seeds(rng, X, Y, want, avoid, iterations, tries=1 << 15):
    """-> (x, m0, m1) of an inactive record whose probe lands on want[it] = (column, row) in those iterations and on no cell of the
    boolean mask ``avoid`` in every other one of ``iterations``. Columns depend on m0 only and rows on m1 only: two vectorised
    searches of ``tries`` candidates each, then the pairs are tried against the mask."""
    others = [it for it in iterations if it not in want]
    for _ in range(64):
        x = F(rng.random(dtype=F))
        m0 = (F(-10.0) + rng.random(tries, dtype=F)).astype(F)
        m0 = m0[(m0 >= F(-10.0)) & (m0 < F(-9.0))]
        m1 = rng.random(tries, dtype=F)
        ok0, ok1 = np.ones(len(m0), bool), np.ones(len(m1), bool)
        for it, (wx, wy) in want.items():
            cx, _ = probe_texel(m0, m0, x, it, X, Y)
            _, cy = probe_texel(m1, m1, x, it, X, Y)
            ok0 &= cx == wx
            ok1 &= cy == wy
        m0, m1 = m0[ok0][:16], m1[ok1][:16]
        for a in m0:
            for b in m1:
                hit = False
                for it in others:
                    cx, cy = probe_texel(a, b, x, it, X, Y)
                    hit = hit or bool(avoid[cy[0], cx[0]])
                if not hit:
                    return x, F(a), F(b)
    raise RuntimeError("no seeds found")


# ---- what happened to a droplet in one iteration ----
def texel_of(pos, X, Y):
    """Texel the particle pass reads for an ACTIVE droplet at ``pos`` (float32, wrapping like the texture fetch)."""
    p = np.asarray(pos, F)
    tcx, tcy = p[..., 0] / F(2.0) + F(0.5), p[..., 1] / F(2.0) + F(0.5)
    return np.floor(tcx * F(X)).astype(np.int64) % X, np.floor(tcy * F(Y)).astype(np.int64) % Y, tcy


def classify(before, after, base_read, water_read, u):
    """Per droplet a set of names for what iteration did to it. ``base_read`` / ``water_read``: the textures the particle pass read
    (the oracle's BASE_DISP / WATER_CUR after that iteration). Status: idle, spawn_rain, spawn_snow, spawn_held (a snow spawn that
    did not fly: the lightning request), spawn_retire (spawned inside a wall cell and retired with new seeds at once), evaporated,
    ground (+ ground_bottom, ground_buried), flight (+ wrap, off_top, off_bottom, cold / warm, freeze, freeze_all, melt, melt_all, density_up, rime,
    grew, evap_all, in_cloud)."""
    b, a = np.asarray(before, F), np.asarray(after, F)
    Y, X = base_read.shape[:2]
    out = []
    for k in range(len(b)):
        s = set()
        was, now = b[k, 2] >= 0, a[k, 2] >= 0
        if not was and not now:
            s.add("idle" if np.array_equal(a[k], b[k]) else "spawn_retire")
        elif not was:
            held = a[k, 2] == 0 and a[k, 3] == F(0.15) and a[k, 4] == F(u["snowDensity"])
            cx, cy, tcy = texel_of(a[k, :2], X, Y)
            s.add("spawn")
            s.add("spawn_rain" if a[k, 2] > 0 else "spawn_snow")
            if held and float(water_read[cy, cx, 1]) > 0:  # (a flying snow spawn inside cloud has grown: its mass is no longer 0.15)
                s.add("spawn_held")
        else:
            cx, cy, tcy = texel_of(b[k, :2], X, Y)
            T = base_read[cy, cx, 3] - tcy * F(u["dryLapse"])
            tot = b[k, 2] + b[k, 3]
            if not now:
                if tot < F(0.04):
                    s.add("evaporated")
                    s.add("evaporated_snow" if b[k, 3] > b[k, 2] else "evaporated_rain")
                else:
                    s.add("ground")
                    s.add("ground_bottom" if b[k, 1] < -1 else "ground_wall")
                    if a[k, 1] != b[k, 1]:
                        s.add("ground_buried")
                    s.add("deposit_mixed" if b[k, 2] > 0 and b[k, 3] > 0 else ("deposit_rain" if b[k, 2] > 0 else "deposit_snow"))
            else:
                s.add("flight")
                s.add("cold" if T < ZERO_C else "warm")
                if abs(float(a[k, 0]) - float(b[k, 0])) > 1.0:
                    s.add("wrap")
                if a[k, 1] > 1:
                    s.add("off_top")
                if a[k, 1] < -1:
                    s.add("off_bottom")
                if water_read[cy, cx, 1] > 0:
                    s.add("in_cloud")
                    if T < ZERO_C and b[k, 4] == 1 and water_read[cy, cx, 2] > 0:
                        s.add("rime")
                area = np.cbrt(tot)
                if T < ZERO_C and b[k, 2] > 0:
                    s.add("freeze")
                    if (ZERO_C - T) * F(u["freezingRate"]) * area > b[k, 2] and a[k, 2] == 0:  # the fminf arm: all the rain there was
                        s.add("freeze_all")
                if T >= ZERO_C and b[k, 3] > 0 and a[k, 2] > 0:
                    s.add("melt")
                    if (T - ZERO_C) * F(u["meltingRate"]) * area > b[k, 3] and a[k, 3] == 0:
                        s.add("melt_all")
                if a[k, 4] > b[k, 4]:
                    s.add("density_up")
                if a[k, 2] + a[k, 3] > tot:
                    s.add("grew")
                if a[k, 2] + a[k, 3] == 0:
                    s.add("evap_all")
        out.append(s)
    return out


# ---- backgrounds ----
def background(X, Y, variant="flat", wind=0.0, sea=()):
    """surface_scenes.background without cloud water; ``wind``: a uniform horizontal wind (cells / iteration) in the air above the
    surface layer; ``sea``: columns turned into sea (water cells are the only wall cells colder than 500 K: the only ones a probe spawns in)."""
    base, water, wall, h = S.background(X, Y, variant)
    air = wall[..., 1] != 0
    water[..., 1] = np.where(air, F(0.0), water[..., 1])
    if wind:
        base[..., 0] = np.where(air & (np.arange(Y)[:, None] >= S.GROUND + 3), base[..., 0] + F(wind), base[..., 0])
    for x in sea:
        w = ~air[:, x]
        base[w, x, 3] = F(288.15)
        water[w, x] = (1002.0, 0.0, 100.0, 0.0)
        wall[:, x, 0] = S.WATER
        wall[w, x, 3] = 0
    return base, water, wall, h


def uniforms(Y, **over):
    u = S.scene_uniforms(Y)
    u["enablePrecipitation"] = 1
    u["spawnChanceMult"] = 1.0  # (cloud - threshold) / (inactive + 10) * X * Y > 1 for a planted cloud on the smallest grid
    u["inactiveDroplets"] = 0.0
    u.update(over)
    return u


def cell_pos(xf, yf, X, Y):
    """Droplet position of the point (xf, yf) in cells."""
    return F((xf / X - 0.5) * 2.0), F((yf / Y - 0.5) * 2.0)


def clear_of_count(x, y):
    """Column ``x`` moved right by 8 where a sprite centred in cell (x, y) would cover texel (0,0): the inactive count is added there
    once per inactive droplet, and a sprite's share on top of it is one deposit too many for an order-free sum."""
    return x + 8 if (x < 7 and y < 7) else x


class _Scene:
    def __init__(self, c, variant="flat", wind=0.0, sea=(), **over):
        self.c, self.X, self.Y = c, c["X"], c["Y"]
        self.base, self.water, self.wall, self.h = background(self.X, self.Y, variant, wind, sea)
        self.u = uniforms(self.Y, **over)
        self.records, self.expect, self.sites, self.probes = [], {}, [], []
        self.prepared = np.zeros((self.Y, self.X), bool)  # cells no stray probe may land on
        self.rng = np.random.Generator(np.random.Philox(zlib.crc32(repr(sorted(c.items())).encode())))
        self.lightning0 = None

    def row_of(self, realT_below=None, realT_above=None):
        """A row of the air whose real temperature is below / above the bound by at least 3 K, nearest to the middle of the air."""
        T = self.base[:, 0, 3] - ((np.arange(self.Y) + F(0.5)) / F(self.Y)) * F(self.u["dryLapse"])
        rows = [y for y in range(S.GROUND + 2, self.Y - 1)
                if (realT_below is None or T[y] < realT_below - 3) and (realT_above is None or T[y] > realT_above + 3)]
        if not rows:
            raise ValueError("no such row on this grid")
        return rows[-1] if realT_above is not None else rows[0]  # (the one nearest to 0 C: the middle of the grid)

    def cloud(self, x, y, v, precip=0.0, r=1):
        """Cloud water ``v`` (and total water with it) in the (2r+1)^2 cells around (x, y), the probe's cell in the middle."""
        for yy in range(max(0, y - r), min(self.Y, y + r + 1)):
            for dx in range(-r, r + 1):
                xx = (x + dx) % self.X
                self.water[yy, xx, 1] += F(v)
                if self.wall[yy, xx, 1] != 0:
                    self.water[yy, xx, 0] += F(v)
                    self.water[yy, xx, 2] += F(precip)
        self.prepared[max(0, y - 8):y + 9, [(x + d) % self.X for d in range(-8, 9)]] = True

    def active(self, xf, yf, rain, snow, density, expect, site=None):
        px, py = cell_pos(xf, yf, self.X, self.Y)
        self.expect[len(self.records)] = expect
        self.records.append((px, py, F(rain), F(snow), F(density)))
        self.sites.append(site or (int(np.floor(xf)) % self.X, int(np.clip(np.floor(yf), 0, self.Y - 1))))

    def probe(self, want, expect):
        """An inactive record whose probe of (relative) iteration k lands on want[k]; placed by finish()."""
        self.expect[len(self.records)] = expect
        self.probes.append((len(self.records), want))
        self.records.append(None)
        self.sites.extend(want.values())

    def finish(self, n_iter, iter0, event_at=0):
        its = list(range(iter0, iter0 + n_iter))
        while len(self.records) < POOL:
            self.probes.append((len(self.records), {}))
            self.records.append(None)
        for k, want in self.probes:
            x, m0, m1 = search_seeds(self.rng, self.X, self.Y, {iter0 + i: t for i, t in want.items()}, self.prepared, its)
            self.records[k] = (x, F(self.rng.random(dtype=F)), m0, m1, F(self.rng.random(dtype=F)))
        return {"base": self.base, "water": self.water, "wall": self.wall, "drops": np.array(self.records, F), "u": self.u, "iter0": iter0,
                "n_iter": n_iter, "event_at": event_at, "expect": self.expect, "sites": self.sites, "lightning0": self.lightning0, "h": self.h}


# ---- kinds ----
# Every kind plants its event at the lattice sites of the case's offset; the event happens in relative iteration c["lead"] (0 or 1: an
# even and an odd number of iterations before it, so both halves of the double-buffered work lists meet it).
def _sites(c, y_min=S.GROUND + 8, y_max=None):
    X, Y = c["X"], c["Y"]
    s = [(x, y) for x, y in I.lattice_sites(X, Y, PITCH, c["offset"], y_min=0)]
    if Y <= 12:  # (the tiny grid: one site in the air; every sprite reaches row 0 there, so none may reach column 0)
        return [(7 + c["offset"][0] % (X - 14), min(Y - 2, S.GROUND + 3))]
    return [(x, min(max(y, y_min), (Y - 8) if y_max is None else y_max)) for x, y in s][:4]


def _spawn(c, cold, refused=False, swapped=False, between=False):
    over = {}
    if swapped:
        over.update(aboveZeroThreshold=0.1, subZeroThreshold=1.0)
    if refused:
        over.update(inactiveDroplets=HUGE_INACTIVE)
    sc = _Scene(c, **over)
    lead = c["lead"]
    y = sc.row_of(realT_below=ZERO_C) if cold else sc.row_of(realT_above=ZERO_C)
    for k, (x, _) in enumerate(_sites(c)[:2]):
        yy = y - (-k if cold else k)
        x = clear_of_count(x, yy)
        # ``between``: cloud water between the two thresholds, below the one that applies: the fminf pre-test passes, the test does not
        v = 0.5 if between else (REFUSED_CLOUD if refused else 2.0 + 0.25 * k)
        sc.cloud(x, yy, v + (0.0 if (cold or between) else 6.0))
        name = "idle" if (refused or between) else ("spawn_snow" if cold else "spawn_rain")
        sc.probe({lead: (x, yy)}, {lead: name})
    # (cold spawns start at iteration 47: the lightning gate lightning[2] < iterNum - 30 is open and the chance, 0 below 2.5 units of
    # cloud + precipitation, is what refuses the request)
    return sc.finish(lead + 5, 47 if cold else 7, lead)


def _spawn_surface(c):
    """A probe into the air cell directly above the surface cell of a one-cell peak -- in the marching kernel's precip_T / t_in row that
    cell is the only one of its kind -- or (odd column offsets) into the neighbouring texel of the same row, which has air below it;
    and a second probe above flat ground 21 columns on, where the two sprites stay apart."""
    sc = _Scene(c, variant="stepped")
    lead, X, h = c["lead"], sc.X, sc.h
    x = clear_of_count(_sites(c)[0][0], 0)
    if c["Y"] > 12:
        while not (h[x] > h[(x - 1) % X] and h[x] > h[(x + 1) % X] and x + 1 < X):
            x = (x + 1) % X
    y = int(h[x])
    first = (x + c["offset"][0] % 2, y) if c["Y"] > 12 else (x, y)
    xx = (x + 21) % X
    while not (h[xx] == h[(xx - 1) % X] == h[(xx + 1) % X]):
        xx = (xx + 1) % X
    for cx, cy in (first, (xx, int(h[xx]))):
        sc.cloud(cx, cy, 6.0, r=0)
        sc.probe({lead: (cx, cy)}, {lead: "spawn_rain"})
    out = sc.finish(lead + 5, 7, lead)
    out["surface_probe"] = {"peak": (x, y), "probe": first}
    return out


def _spawn_wall(c):
    """A probe into a sea surface cell that holds cloud water: water.x > 1000 and T < 500 -- it spawns and retires in the same
    iteration with the seeds -2 - x, y. Two iterations later the retired record probes with those NEW seeds from its new position: a
    cloud is planted where that probe lands, so it spawns again -- a copy of the record that kept the old seeds (a slab that missed
    the flip) probes elsewhere and stays idle. And one probe into a land wall cell (T = 1000 >= 500): no spawn."""
    s = _sites(c)
    X, Y = c["X"], c["Y"]
    xs = clear_of_count(s[0][0], 0)
    xl = clear_of_count((xs + 36) % X, 0)
    sc = _Scene(c, sea=[(xs + d) % X for d in (-1, 0, 1)])
    lead, iter0 = c["lead"], 7
    ys, yl = int(sc.h[xs]) - 1, int(sc.h[xl]) - 1
    sc.cloud(xs, ys, 2.0, r=0)
    sc.cloud(xl, yl, 2.0, r=0)
    again = None
    if Y > 12:
        its = list(range(iter0, iter0 + lead + 5))
        for _ in range(200):
            x, m0, m1 = search_seeds(sc.rng, X, Y, {iter0 + lead: (xs, ys)}, sc.prepared, its)
            tc0, _ = probe_coords(m0, m1, x, iter0 + lead)
            xnew = ((tc0 - F(0.5)) * F(2.0))[0]
            for y in sc.rng.random(64, dtype=F):
                cx, cy = probe_texel(F(-2.0) - x, y, xnew, iter0 + lead + 2, X, Y)
                cx, cy = int(cx[0]), int(cy[0])
                far = min(abs(cx - xs), X - abs(cx - xs)) > 30 and min(abs(cx - xl), X - abs(cx - xl)) > 30 and 12 < cx < X - 12
                ox_, oy_ = probe_texel(m0, m1, x, iter0 + lead + 2, X, Y)  # where the OLD seeds would probe then
                apart = abs(int(ox_[0]) - cx) > 10 or abs(int(oy_[0]) - cy) > 10
                # (the record's other probes with the new seeds must find nothing)
                quiet = all(not sc.prepared[int(b[0]), int(a[0])] for a, b in
                            (probe_texel(F(-2.0) - x, y, xnew, it, X, Y) for it in its if it > iter0 + lead and it != iter0 + lead + 2))
                if far and apart and quiet and S.GROUND + 10 <= cy <= Y - 10:
                    again = (cx, cy)
                    break
            if again:
                break
        if again is None:
            raise RuntimeError("no second probe found")
        k = len(sc.records)
        sc.records.append((x, F(y), m0, m1, F(sc.rng.random(dtype=F))))
        sc.expect[k] = {lead: "spawn_retire", lead + 2: "spawn"}
        sc.sites.extend([(xs, ys), again])
        sc.cloud(again[0], again[1], 9.0)
    else:
        sc.probe({lead: (xs, ys)}, {lead: "spawn_retire"})
    sc.probe({lead: (xl, yl)}, {lead: "idle"})
    out = sc.finish(lead + 5, iter0, lead)
    out["probes_again_at"] = again
    return out


def _lightning(c, mode):
    """A snow spawn in a cell with 400 units of precipitation: the lightning chance is above 1. granted: the request becomes the
    lightning state; refused: a strike 10 iterations ago (lightning[2] >= iterNum - 30), the droplet flies as snow; discarded: the
    request of iteration 0 falls out of lightning_update's window [max(iterNum - 1, 1), iterNum]; covered: a droplet sprite over
    texel (1, 0) adds its mass, heat and vapour share to the request (a two-operand sum per channel: still exact)."""
    sc = _Scene(c)
    lead = c["lead"]
    iter0 = 0 if mode == "discarded" else 40
    if mode == "discarded":
        lead = 0
    x, _ = _sites(c)[0]
    y = sc.row_of(realT_below=ZERO_C)
    if mode == "covered":
        x = 30 + x % (sc.X - 60)  # (away from the sprite over the mailbox)
    sc.cloud(x, y, 2.0, precip=400.0, r=0)
    sc.probe({lead: (x, y)}, {lead: "spawn_snow" if mode == "refused" else "spawn_held"})
    if mode == "discarded":
        sc.lightning0 = (0.0, 0.0, -100.0, 0.0)  # (a fresh state's 0 would refuse every request before iteration 31)
    if mode == "refused":
        sc.lightning0 = (0.25, 0.5, float(iter0 + lead - 10), 1.0)
    if mode == "covered":  # a flying droplet whose sprite covers columns 1 .. 12 of rows 0 .. 10: texel (1,0), not texel (0,0)
        sc.active(7.4, S.GROUND + 1.5, 0.5, 0.0, 1.0, {0: ("flight",), lead: ("flight",)}, site=(1, 0))
    out = sc.finish(lead + 5, iter0, lead)
    out["lightning_mode"], out["event_iter"] = mode, iter0 + lead
    return out


FLIGHT = {
    # kind: (cold row?, cloud, precipitation, [(rain, snow, density)], what the first iteration must show)
    "freeze_down": (True, 0.0, 0.0, [(0.5, 0.0, 1.0), (0.4, 0.2, 0.6)], ("flight", "cold", "freeze")),
    "melt_up": (False, 0.0, 0.0, [(0.0, 0.5, 0.3), (0.2, 0.4, 0.5)], ("flight", "warm", "melt", "density_up")),
    "rime": (True, 1.5, 0.8, [(0.5, 0.0, 1.0), (0.0, 0.5, 1.0)], ("flight", "cold", "rime", "grew")),
    "grow_warm": (False, 9.0, 0.0, [(0.5, 0.0, 1.0), (0.3, 0.3, 0.5)], ("flight", "warm", "in_cloud", "grew")),
    "hail_melt": (False, 0.0, 0.0, [(0.0, 0.5, 0.95), (0.0, 0.6, 0.99)], ("flight", "warm", "melt", "density_up")),
    "freeze_limited": (True, 0.0, 0.0, [(1e-4, 0.5, 0.3), (2e-4, 0.4, 0.3)], ("flight", "cold", "freeze_all")),
    "melt_limited": (False, 0.0, 0.0, [(0.5, 1e-4, 0.9), (0.4, 2e-4, 0.9)], ("flight", "warm", "melt_all")),
    "evap_limited": (False, 0.0, 0.0, [(0.0401, 0.0, 1.0), (0.0, 0.0401, 0.3)], ("flight", "evap_all")),
}


def _flight(c):
    cold, cloud, precip, recs, names = FLIGHT[c["kind"]]
    over = {"evapRate": 1.0} if c["kind"] == "evap_limited" else {}
    sc = _Scene(c, **over)
    y = sc.row_of(realT_below=ZERO_C) if cold else sc.row_of(realT_above=ZERO_C)
    if c["kind"] == "evap_limited" and c["Y"] > 12:
        y = S.GROUND + 14  # (dry air aloft: 20 K below saturation)
    for k, (x, _) in enumerate(_sites(c)[:2]):
        x = clear_of_count(x, y)
        if cloud:
            sc.cloud(x, y, cloud, precip=precip)
        r = recs[k % len(recs)]
        ex = {0: names}
        if c["kind"] == "evap_limited":
            ex[1] = ("evaporated",)
        sc.active(x + 0.5, y + 0.5, *r, ex)
    return sc.finish(5, 7)


def _retire(c):
    """totalMass < 0.04: from the rain side and from the snow side (planted below 0.04: the event is the first iteration)."""
    sc = _Scene(c)
    for k, (x, y) in enumerate(_sites(c)[:4]):
        snow = k % 2 == 1
        sc.active(clear_of_count(x, y) + 0.5, y + 0.5, 0.0 if snow else 0.03, 0.03 if snow else 0.0, 0.3 if snow else 1.0, {0: ("evaporated", "evaporated_snow" if snow else "evaporated_rain")})
    return sc.finish(5, 7)


def _ground(c):
    """Ground hits. wall: droplets planted INSIDE the surface cell of flat ground, of a one-cell peak, of a one-cell pit and of the
    cell beside a step (rain, snow, mixed by site); buried: one row below the surface (the texel above is wall: newPosy += texY);
    bottom: below the grid (newPosy < -1: the deposit's sprite is clipped away). The run goes on for the surface row to read the deposit."""
    kind = c["kind"]
    sc = _Scene(c, variant="stepped")
    X, Y, h = sc.X, sc.Y, sc.h
    x0 = clear_of_count(_sites(c)[0][0], 0)
    masses = [(0.5, 0.0, 1.0), (0.0, 0.5, 0.3), (0.3, 0.25, 0.6)]
    names = ["deposit_rain", "deposit_snow", "deposit_mixed"]

    def column(pred, start):
        for d in range(X):
            x = (start + d) % X
            if pred(x):
                return x
        raise ValueError("no such column")
    flat = lambda x: h[x] == h[(x - 1) % X] == h[(x + 1) % X] == S.GROUND
    peak = lambda x: h[x] > h[(x - 1) % X] and h[x] > h[(x + 1) % X]
    pit = lambda x: h[x] < h[(x - 1) % X] and h[x] < h[(x + 1) % X]
    step = lambda x: h[x] == S.GROUND and h[(x + 1) % X] > h[x]
    if kind == "ground_bottom":
        for k in range(2):
            sc.active((x0 + 40 * k) % X + 0.5, -0.3, *masses[k], {0: ("ground", "ground_bottom", names[k])}, site=((x0 + 40 * k) % X, 0))
        return sc.finish(5, 7)
    preds = {"ground_flat": flat, "ground_peak": peak, "ground_pit": pit, "ground_step": step, "ground_buried": flat}
    pred = preds[kind]
    x = x0
    for k in range(3 if X > 100 else 1):
        x = column(lambda x: x >= 7 and pred(x), x)
        y = int(h[x]) - (2 if kind == "ground_buried" else 1)
        sc.active(x + 0.5, y + 0.5, *masses[(k + c["offset"][0]) % 3],
                  {0: ("ground", "ground_wall", names[(k + c["offset"][0]) % 3]) + (("ground_buried",) if kind == "ground_buried" else ())})
        x = (x + 40) % X
    return sc.finish(5, 7)


def _edges(c):
    """Position edges, with evaporating droplets (a retiring droplet keeps its position: the sprite's centre is exact). exact:
    gposx = +-1 and gposy = +-1 exactly -- anchor column X, anchor row Y; cut: sprites cut by each edge of the grid and by a corner;
    wrap: a flying droplet in the last column whose wind carries it across x = 1; top: one above the top (clipped: no sprite, and
    the texel it reads wraps to the ground row: a ground hit)."""
    kind = c["kind"]
    X, Y = c["X"], c["Y"]
    sc = _Scene(c, wind=0.4 if kind == "edge_wrap" else 0.0)
    ym = Y / 2.0 + c["offset"][1] % 5
    ev = (0.03, 0.0, 1.0)
    if kind == "edge_exact":
        for px, py in ((1.0, 0.1), (-1.0, -0.2)) + (((0.3, 1.0), (-0.4, -1.0)) if Y > 30 else ()):
            sc.expect[len(sc.records)] = {0: ("evaporated",)}
            sc.records.append((F(px), F(py), F(ev[0]), F(ev[1]), F(ev[2])))
            sc.sites.append((int((px + 1) / 2 * X) % X, min(Y - 1, int((py + 1) / 2 * Y))))
    elif kind == "edge_cut":
        pts = [(2.5, ym), (X - 3.5, ym - 14)] + ([(X / 2.0 + c["offset"][0], Y - 2.5), (X / 3.0, 3.5), (X - 2.0, Y - 1.5)] if Y > 30 else [])
        for xf, yf in pts:
            sc.active(xf, yf, *ev, {0: ("evaporated",)})
    elif kind == "edge_wrap":
        sc.active(X - 0.05, ym, 0.5, 0.0, 1.0, {0: ("flight", "wrap")})
        sc.active(X / 2.0, ym, 0.5, 0.0, 1.0, {0: ("flight",)})
    elif kind == "edge_top":
        sc.active(X / 3.0, Y + 0.2, 0.5, 0.0, 1.0, {0: ("ground",)}, site=(X // 3, Y - 1))
        sc.active(X / 3.0 + 40, Y - 2.3, 0.0, 0.5, 0.3, {0: ("flight",)})
        # ... and two whose sprites are clipped away: far enough below the floor to stay there when the ground hit moves it up a row, and
        # left of the grid (no flight ends there -- x wraps -- but an uploaded record may)
        sc.active(X / 3.0 + 80, -3.0, 0.5, 0.0, 1.0, {0: ("ground", "ground_bottom")}, site=(int(X / 3.0 + 80) % X, 0))
        sc.expect[len(sc.records)] = {0: ("evaporated",)}
        sc.records.append((F(-1.2), F(0.1), F(0.03), F(0.0), F(1.0)))
        sc.sites.append((0, Y // 2))
    return sc.finish(5, 7)


def _refresh(c):
    """Starts two iterations before a multiple of 600 with inactiveDroplets = 1e12. The probe of iteration 600 finds cloud and is
    refused (the chance is still computed with 1e12); the iteration's count of inactive droplets -- texel (0,0) -- becomes
    inactiveDroplets, and the probe of iteration 601 into the same kind of cloud spawns."""
    sc = _Scene(c, inactiveDroplets=HUGE_INACTIVE)
    y = sc.row_of(realT_above=ZERO_C)
    s = _sites(c)
    xa = clear_of_count(s[0][0], y)
    xb = clear_of_count((xa + 36) % c["X"], y)
    sc.cloud(xa, y, 6.0 + REFUSED_CLOUD)
    sc.cloud(xb, y, 6.0 + REFUSED_CLOUD)
    sc.probe({2: (xa, y)}, {2: "idle"})
    sc.probe({3: (xb, y)}, {3: "spawn_rain"})
    if c["kind"] == "refresh_covered":  # a flying droplet low over the first columns: its sprite covers texel (0,0) through the crossing
        sc.active(4.0, S.GROUND + 1.5, 0.5, 0.0, 1.0, {k: ("flight",) for k in range(7)}, site=(0, 0))
    out = sc.finish(7, 598, 2)
    out["refresh_at"] = 600
    return out


def _walk(c):
    """Tile state machine. fallSpeed 2.6 / Y and a wind of 0.6 cells / iteration carry a 0.5-unit raindrop a cell down and 0.6 cells along
    per iteration. Walker 1 starts with its sprite's last column up to two columns short of the first 64-column boundary, astride the
    56-column strip seam and astride a 16-row boundary (six rows on either side): it crosses the tile column boundary pixel by pixel and
    leaves the upper tile row after six iterations -- that tile is zeroed once, flagged, and skipped for the rest of the run. Walker 2
    starts one column inside the tile column before the second boundary (eleven beyond it) and leaves it within two iterations. Walker 3
    comes down on the first 16-row boundary from above, in the third strip, over the tile the row-0 droplet left.
    Evaporating droplets in row 0, in row Y - 1 and in the ragged tile column leave tiles that are zeroed, flagged and skipped, and a
    probe re-enters the one of row 0 in iteration 4. The deposition texture goes through its own cycle in the tile of the sea: a ground
    hit in iteration 0 (no feedback: the deposit alone), a second one in iteration 1 (a droplet that fell into the surface), nothing
    for three iterations, then a probe that spawns inside the sea's wall and retires (feedback AND deposition) in iteration 5 or 6."""
    X, Y = c["X"], c["Y"]
    ox = c["offset"][0]
    tall = Y > 30
    sea_x = 24 + ox % 9
    sc = _Scene(c, wind=0.6, sea=[(sea_x + d) % X for d in (-1, 0, 1)], fallSpeed=2.6 / Y)  # (0.05 on 52 rows)
    bx = TILE[0] if X > TILE[0] else STRIP  # the boundary walker 1 crosses: a tile column, or (tiny grid) the strip seam
    by = 2 * TILE[1] if tall else 0
    # the sprite covers columns i0 .. i0 + 11, i0 = ceil(xw - 6.5)
    if tall:
        sc.active(bx - 6.0 - (ox % 3) + 0.25, by + 0.25, 0.5, 0.0, 1.0, {k: ("flight",) for k in range(10)})
        sc.active(2 * bx + 5.25 - (ox % 3), by + 0.25, 0.5, 0.0, 1.0, {k: ("flight",) for k in range(10)})
        # walker 3 comes down on the first 16-row boundary from above, in the third strip, over the tile the row-0 droplet left
        sc.active(2 * STRIP + 6.25, TILE[1] + 8.25, 0.5, 0.0, 1.0, {k: ("flight",) for k in range(10)})
    else:
        sc.active(bx - 6.0 - (ox % 3) + 0.25 - 10, 5.5, 0.5, 0.0, 1.0, {0: ("flight",)})
    ev = (0.03, 0.0, 1.0)
    if tall:
        for xf, yf in [(2 * STRIP + ox % 5 + 0.5, 0.5), (bx + 30 + ox % 7 + 0.5, Y - 0.5), (X - 3.5, Y / 2.0 + 9)]:
            sc.active(xf, yf, *ev, {0: ("evaporated",)})
    ys = int(sc.h[sea_x]) - 1
    sc.active(sea_x + 0.5, ys + 0.5, 0.4, 0.1, 0.8, {0: ("ground", "deposit_mixed")})
    if tall:
        sc.active(sea_x - 15.5, ys + 1.5, 0.5, 0.0, 1.0, {0: ("flight",), 1: ("ground", "deposit_rain")})
    sc.cloud(sea_x, ys, 2.0, r=0)
    again = 6 - c["lead"]  # (the spawn_wall kind of the same configuration retires in iteration 1 - lead: between them both parities)
    sc.probe({again: (sea_x, ys)}, {again: "spawn_retire"})
    if tall:
        xr, yr = 2 * STRIP + ox % 5, S.GROUND + 2
        sc.cloud(xr, yr, 9.0, r=0)
        sc.probe({4: (xr, yr)}, {4: "spawn_rain"})
    return sc.finish(10, 7)


def _last(c):
    """The pool's last active droplet retires (iteration 0: evaporation; the tiny pool's other records are inactive), three quiet
    iterations follow -- every flag at "zero", both textures all zero bar the inactive count -- and then the first spawn."""
    sc = _Scene(c)
    x, y = _sites(c)[0]
    sc.active(x + 0.5, y + 0.5, 0.03, 0.0, 1.0, {0: ("evaporated",)})
    yw = sc.row_of(realT_above=ZERO_C)
    xs = clear_of_count((x + 36) % c["X"], yw)
    sc.cloud(xs, yw, 8.0)
    sc.probe({4: (xs, yw)}, {4: "spawn_rain"})
    out = sc.finish(7, 7)
    out["quiet"] = (1, 2, 3)
    return out


def _flag_row(c):
    """A raindrop comes down on the 16-row boundary at row 32 from above, a cell per iteration: in iteration 1 its sprite's lowest row
    is row 32 itself, the first row of tile row 2, over a tile row that an evaporated droplet left in iteration 0; one iteration later
    it enters tile row 1. The marching kernel loads a row of zeros where the fb_zero flags under its strip say "all zero": this is the
    placement at which the flag of the tile row below and the flag of the row's own tile row could differ. (They do not: the
    classification box-sums the 3 x 3 tile neighbourhood of every tile that holds an anchor, which leaves the tile row below
    unflagged in that iteration -- why a flag read one row off cannot change a result)"""
    X, Y = c["X"], c["Y"]
    sc = _Scene(c, fallSpeed=2.6 / Y)
    x = _sites(c)[0][0]
    x = min(max(x, 8), X - 8)
    by = 2 * TILE[1]
    walker = {k: ("flight",) for k in range(5)}
    sc.active(x + 0.25, by + 8.25, 0.5, 0.0, 1.0, walker)
    sc.active(x + 0.5, by - 8.0, 0.03, 0.0, 1.0, {0: ("evaporated",)})
    out = sc.finish(5, 7)
    out["boundary_row"] = by
    return out


BUILDERS = {
    "spawn_rain": lambda c: _spawn(c, cold=False), "spawn_snow": lambda c: _spawn(c, cold=True),
    "spawn_rain_swapped": lambda c: _spawn(c, cold=False, swapped=True), "spawn_snow_swapped": lambda c: _spawn(c, cold=True, swapped=True),
    "spawn_between": lambda c: _spawn(c, cold=False, between=True), "spawn_between_swapped": lambda c: _spawn(c, cold=True, between=True, swapped=True),
    "spawn_refused": lambda c: _spawn(c, cold=False, refused=True),
    "spawn_surface": _spawn_surface, "spawn_wall": _spawn_wall,
    "lightning_granted": lambda c: _lightning(c, "granted"), "lightning_refused": lambda c: _lightning(c, "refused"),
    "lightning_discarded": lambda c: _lightning(c, "discarded"), "lightning_covered": lambda c: _lightning(c, "covered"),
    **{k: _flight for k in FLIGHT},
    "retire": _retire,
    **{k: _ground for k in ("ground_flat", "ground_peak", "ground_pit", "ground_step", "ground_buried", "ground_bottom")},
    **{k: _edges for k in ("edge_exact", "edge_cut", "edge_wrap", "edge_top")},
    "refresh": _refresh,
    "walk": _walk, "last_retires": _last, "flag_row": _flag_row,
}
# Kinds that run under WX_OPT_SPLAT_ORDER 1 only. refresh_covered: the crossing with a sprite parked over texel (0,0). In order 1 both
# sides keep the inactive count in a slot of its own and add it to the box-summed texel once: a two-operand sum. In the default order
# the texel receives one addition of 1.0 per inactive record besides the sprite's share, and the order of those decides the last bit.
ORDER1_BUILDERS = {
    "refresh_covered": _refresh,
}
KINDS = tuple(BUILDERS)
ORDER1_KINDS = tuple(ORDER1_BUILDERS)

# configuration -> how tools/fuzz_parity.IMPULSE_CONFIGS would say it: kernel set, splat order, waterTexture_0 stored, the schedule
CONFIGS = {
    "wet": {}, "wet_plain": {"plain": True}, "wet_pieces": {"pieces": True}, "wet_stored": {"water0_on_demand": 0}, "perpass": {"kernel_set": 0},
    "order1": {"splat_order": 1}, "order1_perpass": {"splat_order": 1, "kernel_set": 0},
}
CONFIG_CYCLE = tuple(CONFIGS)
OFFSETS = ((0, 14), (57, 3), (120, 22), (5, 9), (63, 27), (110, 1), (1, 17))  # one per configuration of a kind: thinned to the phases test_droplet_cpu.py asks for
BAND_KINDS = ("spawn_snow", "ground_flat", "walk")
# the tiny grid's nine rows span the whole height: no warm air row above the surface layer, and every sprite reaches row 0 (so none may
# reach column 0, and no sprite can be cut by the left edge) -- the kinds that need either are not run there
TINY_KINDS = ("spawn_snow", "spawn_snow_swapped", "spawn_between_swapped", "spawn_wall", "lightning_granted", "lightning_refused", "lightning_discarded",
              "lightning_covered", "freeze_down", "rime", "freeze_limited", "retire", "ground_flat", "ground_peak", "ground_pit", "ground_step",
              "ground_buried", "ground_bottom", "edge_top", "walk")


def schedule(config, n_iter, lead):
    """Handle calls [(iterations, overlap flag)] and the iteration counts after which handle and oracle are compared. display: one
    iteration per step around the event, then 3; plain: the event's iteration is inside a step of three (not its last: no display
    stores); pieces: it is a WX_OVERLAP_MORE_TO_COME piece of its own, the rest of the step follows."""
    cfg = CONFIGS[config]
    if cfg.get("plain"):
        calls = [(1, 0)] * lead + [(3, 0)]
    elif cfg.get("pieces"):
        calls = [(1, 0)] * lead + [(1, 4), (2, 0)]
    else:
        calls = [(1, 0)] * (lead + 2)
    done = sum(n for n, _ in calls)
    while done < n_iter:
        n = min(3, n_iter - done)
        calls.append((n, 0))
        done += n
    compare, done = [], 0
    for n, flag in calls:
        done += n
        if flag == 0:
            compare.append(done)
    return calls, compare


def cases():
    """(kind, grid, offset, lead, configuration): every kind under every configuration on the ragged grid, the offset and the lead
    walking with the product (tool_scenes.CONFIG_CYCLE's way); every kind once on the aligned and on the tiny grid; three kinds on the
    band grid under ROW_BANDS 0 / 1 / 2."""
    out = []
    for ki, kind in enumerate(KINDS):
        for ci, config in enumerate(CONFIG_CYCLE):
            X, Y = GRIDS["ragged"]
            out.append({"kind": kind, "grid": "ragged", "X": X, "Y": Y, "offset": list(OFFSETS[(ki + ci) % len(OFFSETS)]), "lead": (ki + ci) % 2, "config": config})
        for gi, grid in enumerate(("aligned", "tiny")):
            if grid == "tiny" and kind not in TINY_KINDS:
                continue
            X, Y = GRIDS[grid]
            out.append({"kind": kind, "grid": grid, "X": X, "Y": Y, "offset": list(OFFSETS[(ki + gi) % len(OFFSETS)]), "lead": (ki + gi + 1) % 2,
                        "config": CONFIG_CYCLE[(ki + 3 * gi) % len(CONFIG_CYCLE)]})
    for bi, kind in enumerate(BAND_KINDS):
        X, Y = GRIDS["bands"]
        out.append({"kind": kind, "grid": "bands", "X": X, "Y": Y, "offset": [1098 - 500 * bi, 14 + 5 * bi], "lead": bi % 2, "config": "wet", "bands": bi})
    for bi in (0, 1):  # (the tile state machine under every band mode: bands change which segment reads which flag row)
        X, Y = GRIDS["bands"]
        out.append({"kind": "walk", "grid": "bands", "X": X, "Y": Y, "offset": [98 + bi, 24], "lead": bi, "config": "wet", "bands": bi})
    for ki, kind in enumerate(ORDER1_KINDS):
        for ci, config in enumerate(("order1", "order1_perpass")):
            X, Y = GRIDS["ragged"]
            out.append({"kind": kind, "grid": "ragged", "X": X, "Y": Y, "offset": list(OFFSETS[(ki + ci) % len(OFFSETS)]), "lead": ci, "config": config})
    return out


def build_case(c):
    return (BUILDERS.get(c["kind"]) or ORDER1_BUILDERS[c["kind"]])(c)


def case_id(c):
    return f"{c['kind']}-{c['grid']}-{c['config']}-o{c['offset'][0]}_{c['offset'][1]}-l{c['lead']}" + (f"-b{c['bands']}" if "bands" in c else "")


# ---- phases (for messages and the accounting) ----
def anchor_of(rec, X, Y):
    """Anchor (q, r) of a droplet record's sprite in the (X + 1) x (Y + 1) accumulation grid: the sprite covers q - 6 .. q + 5."""
    i0, j0 = I.sprite_windows(np.asarray(rec, F)[None, :], X, Y)
    return int(i0[0]) + 6, int(j0[0]) + 6


def phases(x, y, X):
    return {"tile": (x // TILE[0], y // TILE[1]), "in_tile": (x % TILE[0], y % TILE[1]), "strip": x // STRIP, "strip_lane": x % STRIP}


def describe(field, a, b, sc, X, drops=None):
    """impulse_scenes.describe_difference, plus the droplet nearest to the first differing cell and its anchor's tile / strip phases."""
    ne = a != b
    while ne.ndim > 2:
        ne = ne.any(-1)
    ys, xs = np.nonzero(ne)
    x, y = int(xs[0]), int(ys[0])
    msg = I.describe_difference(field, a, b, sc["sites"], X) + f"; cell phases {phases(x, y, X)}"
    if drops is not None and len(drops):
        Y = a.shape[0]
        anchors = [anchor_of(d, X, Y) if d[2] >= 0 else None for d in drops]
        live = [(abs(q - x) + abs(r - y), k, (q, r)) for k, qr in enumerate(anchors) if qr for q, r in [qr]]
        if live:
            _, k, (q, r) = min(live)
            msg += f"; nearest active droplet {k} {drops[k].tolist()} anchor {(q, r)} phases {phases(q, r, X)}"
    return msg


# ---- the oracle's account of a case (tests/test_droplet_cpu.py; no GPU) ----
def tile_maps(tex, X, Y):
    """Per splat tile: does the texture hold a non-zero value there? The mailbox texels (0,0) and (1,0) are left out."""
    nz = (np.asarray(tex) != 0).any(-1)
    nz[0, :2] = False
    tx, ty = -(-X // TILE[0]), -(-Y // TILE[1])
    out = np.zeros((ty, tx), bool)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = nz[j * TILE[1]:(j + 1) * TILE[1], i * TILE[0]:(i + 1) * TILE[0]].any()
    return out


def run_oracle(wx_oracle, c, sc=None, **over):
    """The oracle through the case, iteration by iteration -> a list of per-iteration records: droplets before / after, classify()'s
    names, deposits_per_texel, the lightning state, texel (0,0) / (1,0) of the feedback texture, the tile maps of both textures, the
    largest velocity, and the fields at the end."""
    sc = sc or build_case(c)
    X, Y = c["X"], c["Y"]
    o = wx_oracle.OracleSim(X, Y, len(sc["drops"]))
    rec = []
    try:
        o.upload(sc["base"], sc["water"], sc["wall"], sc["drops"])
        o.set_params(dict(sc["u"], splat_order=CONFIGS[c["config"]].get("splat_order", 0), **over))
        o.iter = sc["iter0"]
        if sc["lightning0"]:
            o.set_lightning(sc["lightning0"])
        for it in range(sc["n_iter"]):
            b, l0 = o.field("DROPS"), o.field("LIGHTNING")
            o.step(1)
            a, fb, dep, base = o.field("DROPS"), o.field("PRECIP_FB"), o.field("PRECIP_DEP"), o.field("BASE_CUR")
            rec.append({"before": b, "after": a, "names": classify(b, a, o.field("BASE_DISP"), o.field("WATER_CUR"), sc["u"]),
                        "deposits": I.deposits_per_texel(b, a, X, Y), "lightning_before": l0, "lightning": o.field("LIGHTNING"),
                        "count": fb[0, 0].copy(), "request": fb[0, 1].copy(), "fb_tiles": tile_maps(fb, X, Y), "dep_tiles": tile_maps(dep, X, Y),
                        "fb_any": bool(tile_maps(fb, X, Y).any()), "dep_any": bool((dep != 0).any()),
                        "finite": bool(np.isfinite(base).all() and np.isfinite(o.field("WATER_CUR")).all()), "vmax": float(np.abs(base[..., :2]).max()),
                        "water": o.field("WATER_CUR") if it == sc["n_iter"] - 1 else None})
    finally:
        o.close()
    return rec


def transitions(seq):
    """Names of the tile transitions a sequence of per-iteration "holds something" booleans goes through (clean before iteration 0)."""
    out, seen = set(), False
    for i, v in enumerate(seq):
        prev = bool(seq[i - 1]) if i else False
        if v and not seen:
            out.add("clean->dirty")
        if v and prev:
            out.add("dirty->dirty")
        if not v and prev:
            out.add("dirty->zeroed")
            if i + 2 < len(seq) and not seq[i + 1] and not seq[i + 2]:
                out.add("zeroed->skipped x2")
        if v and seen and i >= 2 and not prev and not seq[i - 2]:
            out.add("skipped->dirty")
        seen = seen or bool(v)
    return out


TRANSITIONS = ("clean->dirty", "dirty->dirty", "dirty->zeroed", "zeroed->skipped x2", "skipped->dirty")
