#!/usr/bin/env python3
"""Finds member values on which a FUSED product changes a float32 result of wx_ensemble_assimilate (include/wxsim.h), for the tolerance
build's device test: the definition rounds d_k*e_k before it is added to Cq and b*e_k before it is subtracted from a; a build that
contracted either into an FMA would differ from the definition by an ulp of a DOUBLE, which a float32 result shows about once in 2^29
random cases. The search is therefore directed (tools/find_variance_separators.py is the model): the observed cell itself, n = 3 members,
gain 1, and an observed value chosen so that member 0's posterior value NEARLY CANCELS -- x_0 + increment has a magnitude of about
2^-24 |x_0| (the observed value is a float32: 24 bits), so one float32 ulp of the result is 2^-47 |x_0| and one ulp of the double
increment, 2^-52 |x_0|, moves it in about one case of 32. Doubles are Python floats; the fused operation is evaluated in exact rational
arithmetic and rounded once. Prints the separators as Python literals (tests/test_ensemble_assimilate_cpu.py: SEPARATORS).

    python tools/find_assimilate_separators.py [--want 4] [--seed 1]
"""
import argparse
import math
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def f32(v):
    with np.errstate(over="ignore"):
        return np.float32(v)


def posterior(t, value, R, fuse=None):
    """The observed channel of the observed cell after one observation (gain 1, rho 1, no clamp): the definition, or with ONE product
    fused -- "cov": Cq = fma(d_k, e_k, Cq); "post": x_k + fma(-b, e_k, a)."""
    n = len(t)
    S = 0.0
    for v in t:
        S = S + v
    hm = S / n
    e = [v - hm for v in t]
    Q = 0.0
    for ek in e:
        Q = Q + ek * ek
    V = Q / (n - 1)
    D = V + R
    innovation = value - hm
    alpha = 1.0 / (1.0 + math.sqrt(R / D))
    Cq = 0.0
    for ek in e:  # (x = t: xm = hm, d_k = e_k)
        Cq = fma(ek, ek, Cq) if fuse == "cov" else Cq + ek * ek
    K = (1.0 * (Cq / (n - 1))) / D
    a, b = K * innovation, alpha * K
    return [f32(x + (fma(-b, ek, a) if fuse == "post" else a - b * ek)) for x, ek in zip(t, e)], (hm, K, alpha, e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--want", type=int, default=4, help="separators per product")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tries", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.Philox(a.seed))
    found = {"cov": [], "post": []}
    tried = 0
    while tried < a.tries and min(len(v) for v in found.values()) < a.want:
        tried += 1
        t = [float(np.float32(300.0 + rng.normal())) for _ in range(3)]
        R = float(np.float32(rng.uniform(0.05, 2.0)))
        _, (hm, K, alpha, e) = posterior(t, t[0], R)
        target = hm - (t[0] - alpha * K * e[0]) / K  # member 0's posterior value is 0 here, in real numbers
        v0 = np.float32(target)
        for step in range(-6, 7):
            v = v0
            for _ in range(abs(step)):
                v = np.nextafter(v, np.float32(np.inf if step > 0 else -np.inf))
            value = float(v)
            want, _ = posterior(t, value, R)
            if not np.isfinite(want[0]) or want[0] == 0 or abs(float(want[0])) > 1e-3:
                continue
            for fuse in ("cov", "post"):
                got, _ = posterior(t, value, R, fuse)
                if len(found[fuse]) < a.want and got[0].view(np.uint32) != want[0].view(np.uint32):
                    found[fuse].append((fuse, tuple(t), value, R, int(want[0].view(np.uint32)), int(got[0].view(np.uint32))))
    print("# (product, the three members' float32 values, observed value, error variance, member 0 after: defined bits, fused bits)")
    print("# %d configurations tried" % tried)
    print("SEPARATORS = [")
    for fuse in ("cov", "post"):
        for s in found[fuse]:
            print("    %r," % (s,))
    print("]")


if __name__ == "__main__":
    main()
