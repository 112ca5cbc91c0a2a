#!/usr/bin/env python3
"""Find inputs on which a FUSED multiply-add changes a float32 result of the ensemble calls, although it moves the double behind it
by an ulp or two only -- the planted "separating cells" of tests/test_ensemble_statistics_cpu.py (variance: Q += d * d against
Q = fma(d, d, Q)) and tests/test_ensemble_quantiles_cpu.py (linear interpolation: v(k) + g * d against fma(g, d, v(k)); one fine
scale and a p of its own: find_quantile_cells).

A float32 result (float)(x) of a double x changes only if the two evaluations of x lie on different sides of a float32 rounding
boundary: a double whose low 29 mantissa bits are 1 0000...0. For random data that is a 2^-29 event per ulp of difference, so the search
is directed. The double is a function of the members' values; every value is moved in steps of its own float32 ulp:

  1. COARSE: one value whose step moves the double by about a float32 ulp. Its step lands anywhere between two boundaries, so the best
     of 2^21 consecutive steps lies within some 2^8 double ulps of a boundary.
  2. MEDIUM (variance only): a value about 2^-20 of the others. Its step moves the variance by 2 (v - mean) / n * ulp(v): some 2^7
     double ulps. A few steps bring the double within that of the boundary.
  3. FINE: a value about 2^-30 of the others, a step of which moves the double by a fraction of its ulp. A few thousand steps walk the
     double across the boundary; wherever it lies within 8 double ulps of it, both evaluations are done EXACTLY (the defined one in
     Python floats, one rounded operation at a time; the fused one in rational arithmetic, rounded once) and compared as float32.

Pure numpy + fractions, deterministic from --seed, no library of the project is loaded. Prints Python literals: the members' float32
bit patterns and both results' bit patterns. The committed literals were printed by

    python tools/find_variance_separators.py --seed 1

(a few seconds on one core; about one draw in two yields a cell)."""
import argparse
import struct
from fractions import Fraction

import numpy as np

LOW = (1 << 29) - 1
HALF = 1 << 28


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32_from(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def to_f32(x):
    """Python float (double) -> the nearest float32, as a Python float."""
    return float(np.float32(x))


def boundary_distance(x):
    """Signed distance, in double ulps, of the doubles x from the float32 rounding boundary of their own float32 interval."""
    b = np.abs(np.asarray(x, np.float64)).view(np.uint64)
    return (b & np.uint64(LOW)).astype(np.int64) - HALF


# ---- the two evaluations of the variance of the values that entered, in member order (include/wxsim.h: wx_ens_stat) ----
def variance(values, fused):
    n = len(values)
    S = 0.0
    for v in values:
        S = S + v
    m = S / float(n)
    Q = 0.0
    for v in values:
        d = v - m
        if fused:
            Q = float(Fraction(d) * Fraction(d) + Fraction(Q))  # one rounding
        else:
            dd = d * d
            Q = Q + dd
    return Q / float(n)


def variance_scan(values, j, steps):
    """The defined variance (double) with member j moved by `steps` float32 ulps, vectorised over steps."""
    vj = (np.uint32(f32_bits(values[j])) + steps.astype(np.int64)).astype(np.uint32).view(np.float32).astype(np.float64)
    vs = [vj if i == j else np.float64(v) for i, v in enumerate(values)]
    n = np.float64(len(values))
    S = np.zeros_like(vj)
    for v in vs:
        S = S + v
    m = S / n
    Q = np.zeros_like(vj)
    for v in vs:
        d = v - m
        dd = d * d
        Q = Q + dd
    return Q / n


# ---- the two evaluations of the linear quantile of n ascending values (include/wxsim.h: wx_ens_quant) ----
def quantile(values, p, fused):
    n = len(values)
    h = p * float(n - 1)
    k = int(np.floor(h))
    g = h - float(k)
    k1 = min(k + 1, n - 1)
    d = values[k1] - values[k]
    if fused:
        return float(Fraction(g) * Fraction(d) + Fraction(values[k]))
    gd = g * d
    return values[k] + gd


def quantile_scan(values, p, j, steps):
    vj = (np.uint32(f32_bits(values[j])) + steps.astype(np.int64)).astype(np.uint32).view(np.float32).astype(np.float64)
    vs = [vj if i == j else np.float64(v) for i, v in enumerate(values)]
    n = len(values)
    h = p * float(n - 1)
    k = int(np.floor(h))
    g = np.float64(h - float(k))
    k1 = min(k + 1, n - 1)
    d = vs[k1] - vs[k]
    gd = g * d
    return vs[k] + gd


def move(values, j, step):
    values = list(values)
    values[j] = f32_from(f32_bits(values[j]) + int(step))
    return values


def directed(scan, exact, values, stages, fine_steps=4096, near=8):
    """stages: [(member, half width of the scan)], coarse first; the last member is the fine one. Returns [(values, defined, fused)]
    for every fine step at which the float32 of the two exact evaluations differ."""
    for j, half in stages[:-1]:
        steps = np.arange(-half, half + 1)
        dist = np.abs(boundary_distance(scan(values, j, steps)))
        values = move(values, j, steps[int(np.argmin(dist))])
    j = stages[-1][0]
    steps = np.arange(-fine_steps, fine_steps + 1)
    x = scan(values, j, steps)
    found = []
    for s in steps[np.abs(boundary_distance(x)) <= near]:
        vals = move(values, j, s)
        a, b = exact(vals, False), exact(vals, True)
        if to_f32(a) != to_f32(b):
            found.append((vals, to_f32(a), to_f32(b)))
    return found


def draw_cell(rng, n_big):
    """n_big members of magnitude 1 .. 4 with mixed signs, then a medium (2^-20) and a fine (2^-30) one, shuffled; returns the values
    and the positions of (coarse, medium, fine)."""
    big = [to_f32(rng.uniform(1.0, 4.0) * (1 if rng.random() < 0.6 else -1)) for _ in range(n_big)]
    medium, fine = to_f32(rng.uniform(1.0, 2.0) * 2.0 ** -20), to_f32(rng.uniform(1.0, 1.5) * 2.0 ** -30)
    values = big + [medium, fine]
    order = rng.permutation(len(values))
    values = [values[i] for i in order]
    where = {int(old): new for new, old in enumerate(order)}
    return values, (where[0], where[n_big], where[n_big + 1])


def find_variance_cells(rng, n, want_above, want_below):
    """Cells of n entered values; the first `want_above` in which the fused variance is the larger float32 and the first `want_below`
    in which it is the smaller one."""
    above, below = [], []
    while len(above) < want_above or len(below) < want_below:
        values, (coarse, medium, fine) = draw_cell(rng, n - 2)
        for vals, a, b in directed(variance_scan, variance, values, [(coarse, 1 << 21), (medium, 64), (fine, 0)]):
            side = above if b > a else below
            if len(side) < (want_above if b > a else want_below):
                side.append((vals, a, b))
                break  # one cell per draw: the cells are different sets of members
    return above + below


QUANTILE_P = 0.3141592  # (as float32.) No short fraction: with the tests' 0.1 and 1/3 the result is a coarse lattice that never ties


def find_quantile_cells(rng, p, want_above, want_below):
    """n = 2 (h = p, g = p): two ascending values, lo in (-2, -1] and hi in [2^-24, 2^-23). Two values of like magnitude never
    separate -- g (24 bits) times d (at most 25 bits) is an exact double, fused == defined --; with these d has 48 bits. One fine
    scale is enough: a float32 step of hi moves the result by p * 2^-47, a few double ulps, and the result is linear in it. For each of
    2^16 consecutive lo, solve for the step of hi that brings the result to the next float32 boundary above, keep those whose step
    stays inside hi's binade, and evaluate both definitions exactly at that step and its neighbours. p is a search variable like the
    values: the quantiles the tests ask for otherwise (float32 0.1, 1/3) put lo + g d on a lattice of a few offsets from the boundary,
    on which the two evaluations never differ (tried: 2^20 lo each, no cell)."""
    above, below = [], []
    span = (1 << 23) - 2
    while len(above) < want_above or len(below) < want_below:
        lo, hi = to_f32(-rng.uniform(1.0, 2.0)), 2.0 ** -24
        at = lambda j, k: quantile_scan([lo, hi], p, j, np.asarray(k))  # noqa: E731
        sens = float(at(1, [span])[0] - at(1, [0])[0]) / span
        steps0 = np.arange(1 << 16)
        s0 = at(0, steps0)  # (lo is negative: its bit pattern + 1 is further from zero)
        ulp = np.spacing(np.abs(s0))
        need = boundary_distance(s0).astype(np.float64) * ulp  # to the boundary above: s0 < 0, |s0| shrinks as hi grows
        need = np.where(need < 0, need + ulp * float(1 << 29), need)
        steps1 = np.rint(need / sens).astype(np.int64)
        ok = (steps1 > 2) & (steps1 < span)
        for k0, k1 in zip(steps0[ok], steps1[ok]):
            for dk in (-2, -1, 0, 1, 2):
                vals = move(move([lo, hi], 0, k0), 1, k1 + dk)
                a, b = to_f32(quantile(vals, p, False)), to_f32(quantile(vals, p, True))
                side, wanted = (above, want_above) if b > a else (below, want_below)
                if a != b and len(side) < wanted:
                    side.append((vals, a, b))
                    break
            if len(above) >= want_above and len(below) >= want_below:
                break
    return above + below


def show(name, cells):
    print(f"{name} = [")
    for vals, a, b in cells:
        print("    ([%s], 0x%08X, 0x%08X)," % (", ".join("0x%08X" % f32_bits(v) for v in vals), f32_bits(a), f32_bits(b)))
    print("]")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.Philox(a.seed))
    print("# (entered values' float32 bits in member order, float32 bits of the defined result, of the fused result)")
    show("VARIANCE_SEPARATORS_6", find_variance_cells(rng, 6, 1, 1))
    show("VARIANCE_SEPARATORS_5", find_variance_cells(rng, 5, 1, 0))
    show("VARIANCE_SEPARATORS_9", find_variance_cells(rng, 9, 1, 1))
    print("# (v(0), v(1) as float32 bits, float32 bits of the defined linear quantile at p = float32(%r), n = 2, of the fused one)" % QUANTILE_P)
    show("QUANTILE_SEPARATORS", find_quantile_cells(rng, to_f32(QUANTILE_P), 2, 2))


if __name__ == "__main__":
    main()
