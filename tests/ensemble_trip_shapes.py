"""The shapes at which the chunk loops of the ensemble kernels turn: one list of cases -- (call, X, Y, rectangle, members, selection) --
that tests/test_ensemble_trips_cpu.py checks against the caps it reads from csrc/wx_ens_*.h and tests/test_ensemble_trips_gpu.py runs on
the device; the members' contents (the smooth-plus-noise fields and sparse walls of test_ensemble_assimilate_cpu.members_of with the
planted cells of each call's own CPU test written into rows of the first and of the last trip); the observations of the assimilation
cases; and the arithmetic that names a cell's chunk and trip. No test lives here.

A chunk is one 64-column piece of one row of the rectangle: cpr = ceil(w / 64) chunks per row, cpr * h chunks. Every grid kernel is
persistent: `workers` waves or workgroups stride over `items` work items, so the busiest one makes ceil(items / workers) trips and
item i is met on trip i // workers.

  kernel        items                 workers
  stat, assim   chunks                min(ceil(chunks / 4), MAX_WGS) * 4 waves
  score         chunks                min(chunks, MAX_WGS) workgroups
  quant_staged  chunks                min(chunks, MAX_WGS) workgroups
  quant_stream  4 * chunks            min(chunks, MAX_WGS) * 4 waves       (item = 4 * chunk + channel)
  perturb       chunks * n_selected   min(ceil(items / 4), MAX_WGS) * 4    (item = k * chunks + chunk, k the position in the selection)
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

import test_ensemble_assimilate_cpu as A
import test_ensemble_perturb_cpu as PT
import test_ensemble_quantiles_cpu as Q
import test_ensemble_scores_cpu as SC
import test_ensemble_statistics_cpu as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "2d-weather-sandbox_amd", "csrc")
B_, W_ = "BASE_CUR", "WATER_CUR"
N_PLANTED = 64  # cells per planted block: every planted case of the CPU tests lies in front of cell 64

Case = namedtuple("Case", "id call kernel grid rect sel kw")
Geometry = namedtuple("Geometry", "w h cpr chunks items workers trips")


def caps():
    """{"stat" | "assim" | "score" | "quant" | "perturb": {"WG", "MAX_WGS"[, "STAGED_MEMBERS"]}} as the kernels' headers state them."""
    out = {}
    for stem in ("stat", "assim", "score", "quant", "perturb"):
        text = open(os.path.join(CSRC, "wx_ens_%s.h" % stem)).read()
        found = {}
        for name in ("WG", "MAX_WGS", "STAGED_MEMBERS"):
            m = re.search(r"^enum \{[^}]*?\b%s = (\d+)\b" % name, text, re.M)
            if m:
                found[name] = int(m.group(1))
        out[stem] = found
    if "WG" not in out["score"]:  # (wx_ens_score.h takes the quantile kernel's launch shape: WG = wxq::WG)
        assert re.search(r"^enum \{[^}]*?\bWG = wxq::WG\b", open(os.path.join(CSRC, "wx_ens_score.h")).read(), re.M)
        out["score"]["WG"] = out["quant"]["WG"]
    return out


# grid -> X, Y, members the ensemble holds, the planted blocks in order (block j starts j block heights behind row 1 / in front of row Y - 1)
GRIDS = {
    "scores": (70, 2100, 10, ("scores",)),         # 9 members and the truth (a lone handle on the device)
    "state": (70, 4200, 9, ("statistics", "perturb")),
    "quant3": (70, 8300, 4, ("quantiles",)),       # 3 members and the ranked one
    "quant3tall": (2, 32832, 4, ("quantiles",)),  # 32832 chunks: a third trip of 64 rows, which holds the whole planted block
    "quant66": (2, 16500, 66, ("quantiles",)),     # 65 members and the ranked one
    "quant66wide": (65, 8200, 66, ("quantiles",)),  # ... with two chunks per row, the second of one lane (the streaming kernel's own row split)
}

PERTURB_AMP = {B_: (0.05, 0.0, 1e-4, 2.0), W_: (0.5, 0.01, 0.0, 0.2)}
ASSIM_GAINS = dict(gain_base=(0.5, 0, 0, 1), gain_water=(1, 0.5, 0, 0.25))


def _cases():
    out = []
    whole = lambda g: (0, 0, GRIDS[g][0], GRIDS[g][1])  # noqa: E731
    three, nine = [0, 1, 2], None
    for tag, sel in (("3", three), ("9", nine)):
        out.append(Case("scores-%s-maps" % tag, "scores", "score", "scores", whole("scores"), sel, dict(field=B_, maps=True)))
        out.append(Case("scores-%s-scalars" % tag, "scores", "score", "scores", whole("scores"), sel, dict(field=W_, maps=False)))
        out.append(Case("scores-%s-offset" % tag, "scores", "score", "scores", (1, 1, 69, 2098), sel, dict(field=W_ if sel else B_, maps=True)))
    for tag, sel in (("3", three), ("9", nine)):
        out.append(Case("statistics-%s" % tag, "statistics", "stat", "state", whole("state"), sel, dict(field=B_ if sel else W_, variance=True)))
        out.append(Case("statistics-%s-no-variance" % tag, "statistics", "stat", "state", whole("state"), sel, dict(field=W_ if sel else B_, variance=False)))
    for tag, sel in (("3", three), ("9", nine)):
        out.append(Case("assimilate-%s-everywhere" % tag, "assimilate", "assim", "state", whole("state"), sel, dict(loc=(0.0, 0.0), **ASSIM_GAINS)))
        out.append(Case("assimilate-%s-localized" % tag, "assimilate", "assim", "state", whole("state"), sel, dict(loc=(9.0, 300.0), wrap_x=True, lo_water=0.0, **ASSIM_GAINS)))
    out.append(Case("perturb-base-add", "perturb", "perturb", "state", whole("state"), nine, dict(field=B_, mode="add", scale=3, seed=11)))
    out.append(Case("perturb-water-mul-wrap-0-2", "perturb", "perturb", "state", whole("state"), [0, 2], dict(field=W_, mode="mul", scale=8, seed=12, wrap_x=True)))
    out.append(Case("perturb-base-mul-wrap-3", "perturb", "perturb", "state", whole("state"), three, dict(field=B_, mode="mul", scale=64, seed=13, wrap_x=True)))
    out.append(Case("perturb-water-add-0-2", "perturb", "perturb", "state", whole("state"), [0, 2], dict(field=W_, mode="add", scale=1, seed=14)))
    out.append(Case("quantiles-staged-3", "quantiles", "quant_staged", "quant3", whole("quant3"), three, dict(field=B_, interp="linear", rank_of=3)))
    out.append(Case("quantiles-staged-3-tall", "quantiles", "quant_staged", "quant3tall", whole("quant3tall"), three, dict(field=W_, interp="lower", rank_of=3)))
    out.append(Case("quantiles-staged-64", "quantiles", "quant_staged", "quant66", whole("quant66"), list(range(64)), dict(field=B_, interp="higher", rank_of=65)))
    out.append(Case("quantiles-stream-65", "quantiles", "quant_stream", "quant66", whole("quant66"), list(range(65)), dict(field=W_, interp="linear", rank_of=65)))
    out.append(Case("quantiles-stream-65-wide", "quantiles", "quant_stream", "quant66wide", whole("quant66wide"), list(range(65)), dict(field=B_, interp="lower", rank_of=65)))
    return out


CASES = _cases()
KERNELS = ("stat", "assim", "score", "quant_staged", "quant_stream", "perturb")
CARRIES_STATE = ("score", "quant_staged")  # kernels whose loop hands registers or an LDS image from one trip to the next


def by_call(call):
    return [c for c in CASES if c.call == call]


def selection(case):
    """The selected member indices. None in the case: every member of the calls that change or summarize the members themselves."""
    if case.sel is not None:
        return list(case.sel)
    B = GRIDS[case.grid][2]
    return list(range(B - 1 if case.call == "scores" else B))  # (the scores grid's last member is the truth)


def geometry(case, cap=None):
    cap = caps() if cap is None else cap
    _, _, w, h = case.rect
    cpr = (w + 63) // 64
    chunks = cpr * h
    k = case.kernel
    c = cap["quant" if k.startswith("quant") else k]
    waves = c["WG"] // 64
    if k in ("stat", "assim"):
        items, workers = chunks, min(-(-chunks // waves), c["MAX_WGS"]) * waves
    elif k in ("score", "quant_staged"):
        items, workers = chunks, min(chunks, c["MAX_WGS"])
    elif k == "quant_stream":
        items, workers = 4 * chunks, min(chunks, c["MAX_WGS"]) * waves
    else:
        items = chunks * len(selection(case))
        workers = min(-(-items // waves), c["MAX_WGS"]) * waves
    return Geometry(w, h, cpr, chunks, items, workers, -(-items // workers))


def chunk_of(geo, y, x):
    """The chunk of the rectangle's cell (y, x) (rectangle coordinates)."""
    return y * geo.cpr + x // 64


def trip_of(case, geo, y, x, k=0, channel=0):
    """The trip on which the rectangle's cell (y, x) is met: of position k in the selection (perturb), of that channel (streaming)."""
    ch = chunk_of(geo, y, x)
    item = {"quant_stream": 4 * ch + channel, "perturb": k * geo.chunks + ch}.get(case.kernel, ch)
    return item // geo.workers


def differs(got, want):
    """Where the bits differ, NaNs compared as positions."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        return got != want
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)) & ~(np.isnan(got) & np.isnan(want))


def first_difference(case, geo, got, want, what, k=0):
    """None if ``got`` and ``want`` -- (h, w), (h, w, 4) or (n_q, h, w, 4) over the case's rectangle -- hold the same bits; else the text
    of an assertion message: the first differing cell with its chunk and trip."""
    d = differs(got, want)
    if not d.any():
        return None
    cells = d
    if cells.ndim == 4:
        cells = cells.any(axis=0)
    per_channel = cells if cells.ndim == 3 else cells[..., None]
    y, x, c = (int(v) for v in np.argwhere(per_channel)[0])
    at = tuple(np.argwhere(d)[0])
    return "%s %s: %d differing values, the first in cell x=%d y=%d of the rectangle (channel %d): chunk %d of %d, trip %d of %d; got %r, want %r" % (
        case.id, what, int(d.sum()), x, y, c, chunk_of(geo, y, x), geo.chunks, trip_of(case, geo, y, x, k, c), geo.trips, got[at], want[at])


def block_rows(X):
    return -(-(N_PLANTED + 3) // X)


def planted_blocks(grid):
    """[(name, first row of the block in the first trip, first row of the block in the last trip, flat offset of cell 0 in the block)]:
    a block is block_rows(X) whole rows; on the 70-column grids the 64 cells start at x = 3 and so cross the chunk boundary at x = 64."""
    X, Y, _, names = GRIDS[grid]
    nr, s = block_rows(X), (3 if X >= N_PLANTED + 3 else 0)
    return [(name, 1 + j * nr, Y - 1 - (j + 1) * nr, s) for j, name in enumerate(names)]


def planted_cells(name, B):
    """(fields, walls): per member the N_PLANTED cells of that call's own CPU test, float32 / int8 (N_PLANTED, 4)."""
    if name == "statistics":
        return ST.hand_built(B, N_PLANTED)
    if name == "perturb":  # SPECIALS sprinkled over ordinary values
        f, w = PT.hand_built(B, N_PLANTED, 1)
        return [a[0] for a in f], [a[0] for a in w]
    if name == "quantiles":  # ties, -0.0, non-finite cells; the last member is the ranked one
        return Q.planted(B - 1, N_PLANTED)
    if name == "scores":  # the last member is the truth
        (f, w), (tf, tw) = SC.planted(B - 1, N_PLANTED)
        return list(f) + [tf], list(w) + [tw]
    raise KeyError(name)


def block_view(a, row, X, s):
    """The N_PLANTED cells of the block that starts at ``row`` of the (Y, X, 4) array ``a``, as a view."""
    return a[row:row + block_rows(X)].reshape(-1, 4)[s:s + N_PLANTED]


@functools.lru_cache(maxsize=None)
def members(grid):
    """{"base", "water", "wall"}: per member of the grid the (Y, X, 4) arrays that are uploaded, read-only and shared."""
    X, Y, B, _ = GRIDS[grid]
    if X * Y * B <= 10_000_000:
        bases, waters, walls = A.members_of(B, X, Y, seed=41)
    else:  # many members of a large grid: four of them, member i shifted up by 7 i rows (every member differs in every row)
        four = A.members_of(4, X, Y, seed=41)
        bases, waters, walls = ([np.roll(a[i % 4], 7 * i, axis=0) for i in range(B)] for a in four)
    for name, first, last, s in planted_blocks(grid):
        f, w = planted_cells(name, B)
        for i in range(B):
            for row in (first, last):
                block_view(bases[i], row, X, s)[...] = f[i]
                block_view(waters[i], row, X, s)[...] = f[i]
                block_view(walls[i], row, X, s)[...] = w[i]
    if grid == "state":
        A.clear(walls, [(o[1], o[2]) for o in observations()])
    for a in bases + waters + walls:
        a.setflags(write=False)
    return {"base": bases, "water": waters, "wall": walls}


def observations():
    """Eight observations of both fields on the "state" grid: in rows of the first trip, of the last trip, and on the two rows that the
    boundary between the first and the second trip of k_ens_assim separates. The rows are computed from the caps, the cells are air
    cells in every member (`members` clears them) and lie outside the planted blocks."""
    X, Y, _, _ = GRIDS["state"]
    geo = geometry(by_call("assimilate")[0])
    edge = geo.workers // geo.cpr  # the first row of the second trip
    assert geo.workers % geo.cpr == 0 and 8 < edge < Y - 60
    rows = [5, edge // 2, edge - 1, edge, edge + 1, (edge + Y) // 2, Y - 10, Y - 6]
    out = []
    for j, y in enumerate(rows):
        x = (7 + 9 * j) % X
        out.append((B_, x, y, 3, 300.0 + 0.2 * j, 0.25) if j % 2 == 0 else (W_, x, y, 0, 0.012 + 0.001 * j, 1e-6))
    return out
