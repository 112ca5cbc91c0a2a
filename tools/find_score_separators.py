#!/usr/bin/env python3
"""Find small member sets on which a FUSED multiply-add changes a float32 result of wx_ensemble_scores (include/wxsim.h: wx_ens_score),
although it moves the double behind it by an ulp or two only -- the planted "separating cells" of tests/test_ensemble_scores_cpu.py:

  vr:  Q = Q + d_i * d_i        against  Q = fma(d_i, d_i, Q)             (the population variance, sums in ASCENDING order)
  cr:  G = G + (2i - n + 1) u_i against  G = fma(2i - n + 1, u_i, G)      (the CRPS)
  se:  err * err feeds a conversion to float32 and no sum: there is nothing a build could fuse it with, so no separator exists and
       none is searched for.

The search is tools/find_variance_separators.py's -- coarse, medium and fine value, each moved in steps of its own float32 ulp until
the double lies next to a float32 rounding boundary, both evaluations then done exactly -- on the score call's own arithmetic: the
values are sorted first, and the truth t is part of the cell.

vr separates readily (about one draw in two): every d_i * d_i is inexact. cr needs a cell built for it (find_crps_cells): the product
is exact for most data, and a fused one shows only where the partial sums of G cancel.

Pure numpy + fractions, deterministic from --seed, no library of the project is loaded. The committed literals were printed by

    python tools/find_score_separators.py --seed 1
"""
import argparse
from fractions import Fraction

import numpy as np

from find_variance_separators import directed, draw_cell, f32_bits, to_f32


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding


def scores(values, t, fuse=None):
    """(var, crps) as doubles by the definition; fuse = "Q" or "G": that product contracted into its sum."""
    v = sorted(values)
    n = len(v)
    S = 0.0
    for x in v:
        S = S + x
    m = S / float(n)
    Q = A = G = 0.0
    for i, x in enumerate(v):
        d = x - m
        Q = fma(d, d, Q) if fuse == "Q" else Q + d * d
        u = x - t
        A = A + abs(u)
        k = float(2 * i - n + 1)
        G = fma(k, u, G) if fuse == "G" else G + k * u
    return Q / float(n), A / float(n) - G / (float(n) * float(n))


def scores_scan(values, t, j, steps, which):
    """The defined var (which = 0) or crps (1) with member j moved by `steps` float32 ulps, vectorised over steps."""
    vj = (np.uint32(f32_bits(values[j])) + steps.astype(np.int64)).astype(np.uint32).view(np.float32).astype(np.float64)
    v = np.sort(np.stack([vj if i == j else np.full_like(vj, x) for i, x in enumerate(values)]), axis=0)
    n = len(values)
    S = np.zeros_like(vj)
    for x in v:
        S = S + x
    m = S / np.float64(n)
    Q, A, G = np.zeros_like(vj), np.zeros_like(vj), np.zeros_like(vj)
    for i, x in enumerate(v):
        d = x - m
        dd = d * d
        Q = Q + dd
        u = x - np.float64(t)
        A = A + np.abs(u)
        ku = np.float64(2 * i - n + 1) * u
        G = G + ku
    return (Q / np.float64(n), A / np.float64(n) - G / (np.float64(n) * np.float64(n)))[which]


def find_variance_cells(rng, n, want_above, want_below):
    """Cells of n entered values and a truth (which the variance does not see); the first `want_above` in which the fused float32 vr is
    the larger one and the first `want_below` in which it is the smaller one."""
    above, below = [], []
    while len(above) < want_above or len(below) < want_below:
        values, (coarse, medium, fine) = draw_cell(rng, n - 2)
        t = to_f32(rng.uniform(1.0, 4.0) * (1 if rng.random() < 0.5 else -1))
        scan = lambda vals, j, steps: scores_scan(vals, t, j, steps, 0)  # noqa: E731
        exact = lambda vals, fused: scores(vals, t, "Q" if fused else None)[0]  # noqa: E731
        for vals, a, b in directed(scan, exact, values, [(coarse, 1 << 21), (medium, 64), (fine, 0)]):
            side, wanted = (above, want_above) if b > a else (below, want_below)
            if len(side) < wanted:
                side.append((vals, t, a, b))
                break  # one cell per draw: the cells are different sets of members
    return above + below


def find_crps_cells(rng, want_above, want_below):
    """The same for cr, n = 4. (2i - n + 1) u_i is an exact double unless u_i = v(i) - t fills more than 51 bits and the weight is
    no power of two, and a fused product shows only where the sum it feeds is smaller than the product: where G's partial sums
    CANCEL. So the truth lies far above the members (t about 3: every u_i is about -t and fills its 53 bits), and the members are
    small and graded: v(0) about -2^-19 -- the coarse knob: err = m - t and G / 16 put crps about 2^-23, half a float32 ulp, above t
    --, v(1) about -2^-24, v(2) and v(3) about +2^-28. The walk then ends with -3 u(0) - u(1) + u(2), about +3 t, plus 3 u(3), about
    -3 t: the last step cancels down to 2^-17, the fused G keeps the bits that the separately rounded 3 u(3) lost, and v(3), the
    LARGEST value and the one with the weight 3, is the fine knob whose float32 steps G sees."""
    n = 4
    above, below = [], []
    while len(above) < want_above or len(below) < want_below:
        t = to_f32(rng.uniform(2.0, 4.0))
        cell = [to_f32(-rng.uniform(0.9, 1.1) * 2.0 ** -19), to_f32(-rng.uniform(1.0, 2.0) * 2.0 ** -24), to_f32(rng.uniform(1.0, 1.4) * 2.0 ** -28),
                to_f32(rng.uniform(1.5, 2.0) * 2.0 ** -28)]
        scan = lambda vals, j, steps: scores_scan(vals, t, j, steps, 1)  # noqa: E731
        exact = lambda vals, fused: scores(vals, t, "G" if fused else None)[1]  # noqa: E731
        for vals, a, b in directed(scan, exact, cell, [(0, 1 << 20), (1, 64), (2, 64), (3, 0)], fine_steps=2048):
            side, wanted = (above, want_above) if b > a else (below, want_below)
            if sorted(vals) == vals and len(side) < wanted:
                side.append((vals, t, a, b))
                break  # one cell per draw
    return above + below


def show(name, cells):
    print(f"{name} = [")
    for vals, t, a, b in cells:
        print("    ([%s], 0x%08X, 0x%08X, 0x%08X)," % (", ".join("0x%08X" % f32_bits(v) for v in vals), f32_bits(t), f32_bits(a), f32_bits(b)))
    print("]")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.Philox(a.seed))
    print("# (entered values' float32 bits in member order, the truth's, float32 bits of the defined result, of the fused result)")
    show("VARIANCE_SEPARATORS", find_variance_cells(rng, 5, 1, 1) + find_variance_cells(rng, 7, 1, 0))
    show("CRPS_SEPARATORS", find_crps_cells(rng, 2, 2))


if __name__ == "__main__":
    main()
