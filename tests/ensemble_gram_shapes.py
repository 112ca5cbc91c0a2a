"""The launch shapes of the Gram kernels (csrc/wx_ens_gram.h) as arithmetic a test can check and use: the constants the header states,
the jobs and workers of both kernels, and the narrowest grid on which BOTH chunk loops turn a second time. No test lives here.

A chunk is one 64-column piece of one row of the rectangle. k_ens_gram_centre: `workers` waves stride over the chunks (one wave per
chunk, min(ceil(chunks / 4), MAX_WGS) workgroups of WG / 64 waves). k_ens_gram: the pairs a <= b of the n selected members are cut into
TILE x TILE member blocks, a job is one (tile, channel), and every job has n_slots = max(1, min(chunks, MAX_WGS // n_jobs)) workgroups
that stride over the chunks: chunk i is met by slot i % n_slots on trip i // n_slots."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "2d-weather-sandbox_amd", "csrc", "wx_ens_gram.h")


def caps():
    """{"WG", "MAX_WGS", "TILE", "UNROLL", "ROW"} as the kernels' header states them."""
    text = open(HEADER).read()
    out = {}
    for name in ("WG", "MAX_WGS", "TILE", "UNROLL", "ROW"):
        m = re.search(r"^enum \{[^}]*?\b%s = (\d+)\b" % name, text, re.M)
        assert m, name
        out[name] = int(m.group(1))
    return out


def jobs(n, c=None):
    c = caps() if c is None else c
    nb = -(-n // c["TILE"])
    return nb * (nb + 1) // 2 * 4


def centre_workers(chunks, c=None):
    c = caps() if c is None else c
    waves = c["WG"] // 64
    return min(-(-chunks // waves), c["MAX_WGS"]) * waves


def pair_slots(chunks, n, c=None):
    c = caps() if c is None else c
    return max(1, min(chunks, c["MAX_WGS"] // jobs(n, c)))


TALL_X, TALL_MEMBERS, TALL_ROWS_PAST_ONE_TRIP = 2, 3, 9


def tall_grid():
    """2 columns (one chunk per row) and just more rows than the pre-pass's capped grid has waves: its busiest waves take a second
    trip, and the pair kernel's slots (fewer than the pre-pass's waves) many."""
    c = caps()
    return TALL_X, c["MAX_WGS"] * c["WG"] // 64 + TALL_ROWS_PAST_ONE_TRIP + 1


def tall_planted_block_rows(n_planted=9):
    """Rows a block of planted cells takes on the tall grid: its cells fill whole rows."""
    return -(-n_planted // TALL_X)


def tall_planted_rows():
    """The first row of the planted block in the first trip and of the one in the last trip of both kernels."""
    _, Y = tall_grid()
    return 5, Y - 2 - tall_planted_block_rows()
