#!/usr/bin/env python3
"""Finds member values on which a FUSED product changes a float32 result of wx_ensemble_covariance (include/wxsim.h), for the tolerance
build's tests: the definition rounds d_k*e_k before it is added to Cq and d_k*d_k before it is added to Qx; a build that contracted
either into an FMA would differ from the definition by an ulp of a DOUBLE, which a float32 result shows about once in 2^29 random
cases. Both searches are therefore directed (tools/find_inflate_separators.py and tools/find_variance_separators.py are the models).

  "cq": n = 3 members and a point predictor whose third value is solved for so that the covariance NEARLY CANCELS: Cq is then about
  2^-24 of its terms (the value has 24 bits), a float32 ulp of cov = Cq / 2 is 2^-47 of them, and one ulp of a double product, 2^-52,
  moves it in about one case of 32. The value is stepped through the floats around the solution.

  "qx": Qx never cancels, so the float32 variance (and with it slope and corr) changes only where Qx / (n - 1) lies within a double ulp
  or two of a float32 rounding boundary. find_variance_separators.directed walks it there: n = 5 members, three of magnitude 1 .. 4,
  one of 2^-20 and one of 2^-30, moved in steps of their own float32 ulp (coarse, medium, fine).

Doubles are Python floats; the fused operation is evaluated in exact rational arithmetic and rounded once. Prints the separators as
Python literals (tests/test_ensemble_covariance_cpu.py: SEPARATORS).

    python tools/find_covariance_separators.py [--want 3] [--seed 1]
"""
import argparse
import math
from fractions import Fraction

import numpy as np

from find_variance_separators import directed, draw_cell, f32_bits, to_f32


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def f32(v):
    with np.errstate(over="ignore"):
        return np.float32(v)


def maps(x, t, fuse=None):
    """(variance, cov, slope, corr) as float32 of one cell-channel x against one point predictor t: the definition, or with ONE product
    fused -- "cq": Cq = fma(d_k, e_k, Cq); "qx": Qx = fma(d_k, d_k, Qx)."""
    n = len(x)
    S = Sj = 0.0
    for v in x:
        S = S + v
    for v in t:
        Sj = Sj + v
    xm, jm = S / n, Sj / n
    d, e = [v - xm for v in x], [v - jm for v in t]
    Qx = Qj = Cq = 0.0
    for ek in e:
        Qj = Qj + ek * ek
    for dk, ek in zip(d, e):
        Qx = fma(dk, dk, Qx) if fuse == "qx" else Qx + dk * dk
        Cq = fma(dk, ek, Cq) if fuse == "cq" else Cq + dk * ek
    den = math.sqrt(Qx * Qj)
    r = Cq / den
    return f32(Qx / (n - 1)), f32(Cq / (n - 1)), f32(Cq / Qx), f32(min(max(r, -1.0), 1.0))


def _variance(values, fused):
    n = len(values)
    S = 0.0
    for v in values:
        S = S + v
    m = S / n
    Q = 0.0
    for v in values:
        d = v - m
        Q = fma(d, d, Q) if fused else Q + d * d
    return Q / (n - 1)


def variance_scan(values, j, steps):
    """The defined sample variance (double) with member j moved by `steps` float32 ulps, vectorised over steps."""
    vj = (np.uint32(f32_bits(values[j])) + steps.astype(np.int64)).astype(np.uint32).view(np.float32).astype(np.float64)
    vs = [vj if i == j else np.float64(v) for i, v in enumerate(values)]
    S = np.zeros_like(vj)
    for v in vs:
        S = S + v
    m = S / np.float64(len(values))
    Q = np.zeros_like(vj)
    for v in vs:
        d = v - m
        Q = Q + d * d
    return Q / np.float64(len(values) - 1)


def find_cq(rng, want, tries):
    found, tried = [], 0
    while tried < tries and len(found) < want:
        tried += 1
        x = [to_f32(rng.uniform(0.25, 2.0)) for _ in range(3)]
        t = [to_f32(rng.uniform(0.25, 2.0)) for _ in range(2)]
        xm = (x[0] + x[1] + x[2]) / 3.0
        d = [v - xm for v in x]
        if abs(d[2]) < 0.05:
            continue
        t2 = np.float32(-(d[0] * t[0] + d[1] * t[1]) / d[2])  # sum d_k t_k == 0 in real numbers
        for step in range(-6, 7):
            v = t2
            for _ in range(abs(step)):
                v = np.nextafter(v, np.float32(np.inf if step > 0 else -np.inf))
            tt = t + [float(v)]
            want_, got = maps(x, tt), maps(x, tt, "cq")
            if np.isfinite(want_[1]) and want_[1] != 0 and got[1].view(np.uint32) != want_[1].view(np.uint32):
                found.append(("cq", tuple(x), tuple(tt), tuple(int(a.view(np.uint32)) for a in want_), tuple(int(a.view(np.uint32)) for a in got)))
                break
    return found, tried


def find_qx(rng, want):
    found = []
    while len(found) < want:
        values, (coarse, medium, fine) = draw_cell(rng, 3)
        for vals, a, b in directed(variance_scan, _variance, values, [(coarse, 1 << 21), (medium, 64), (fine, 0)]):
            want_, got = maps(vals, vals), maps(vals, vals, "qx")
            assert float(want_[0]) == a and float(got[0]) == b
            found.append(("qx", tuple(vals), None, tuple(int(v.view(np.uint32)) for v in want_), tuple(int(v.view(np.uint32)) for v in got)))
            break  # one cell per draw
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--want", type=int, default=3, help="separators per product")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tries", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.Philox(a.seed))
    cq, tried = find_cq(rng, a.want, a.tries)
    qx = find_qx(rng, a.want)
    print("# (product, the members' float32 values of the cell-channel, the point predictor's values (None: the cell-channel itself),")
    print("# (variance, cov, slope, corr) as float32 bits: defined, with that product fused)")
    print("# cq: %d configurations tried" % tried)
    print("SEPARATORS = [")
    for s in cq + qx:
        print("    %r," % (s,))
    print("]")


if __name__ == "__main__":
    main()
