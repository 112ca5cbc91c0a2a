#!/usr/bin/env python3
"""Finds member values on which a FUSED product changes a float32 result of wx_ensemble_inflate (include/wxsim.h), for the tolerance
build's device test: the definition rounds lambda*d_k before it is added to m and d_k*d_k before it is added to Qa; a build that
contracted either into an FMA would differ from the definition by an ulp of a DOUBLE, which a float32 result shows about once in 2^29
random cases. The search is therefore directed (tools/find_assimilate_separators.py is the model): n = 3 members with a positive mean
and member 0 between zero and the mean, so that d_0 < 0 and a factor lambda* = m / |d_0| > 1 would carry member 0 to zero; the one
float32 knob of the call -- lambda itself in CONST, alpha in RTPS with a prior of about twice the spread -- is stepped through the
floats around that value. Member 0's result m + lambda*d_0 then NEARLY CANCELS: its magnitude is about 2^-24 m (the knob has 24 bits),
one float32 ulp of it is 2^-47 m, and one ulp of the double product, 2^-52 m, moves it in about one case of 32. Doubles are Python
floats; the fused operation is evaluated in exact rational arithmetic and rounded once. Prints the separators as Python literals
(tests/test_ensemble_inflate_cpu.py: SEPARATORS).

    python tools/find_inflate_separators.py [--want 3] [--seed 1]
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


def posterior(t, p, coef, fuse=None):
    """Member 0's channel after one call without bounds or clamp (p None: CONST with lambda = coef, else RTPS with alpha = coef): the
    definition, or with ONE product fused -- "lam": o_k = fma(lambda, d_k, m); "qa": Qa = fma(d_k, d_k, Qa)."""
    n = len(t)
    S = 0.0
    for v in t:
        S = S + v
    m = S / n
    d = [v - m for v in t]
    if p is None:
        lam = coef
    else:
        Sb = 0.0
        for v in p:
            Sb = Sb + v
        mb = Sb / n
        Qa = Qb = 0.0
        for dk in d:
            Qa = fma(dk, dk, Qa) if fuse == "qa" else Qa + dk * dk
        for v in p:
            bk = v - mb
            Qb = Qb + bk * bk
        sa, sb = math.sqrt(Qa / (n - 1)), math.sqrt(Qb / (n - 1))
        lam = 1.0 + coef * ((sb - sa) / sa)
    return f32(fma(lam, d[0], m) if fuse == "lam" else m + lam * d[0]), (m, d, lam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--want", type=int, default=3, help="separators per product")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tries", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.Philox(a.seed))
    found = {"lam": [], "qa": []}
    tried = 0
    while tried < a.tries and min(len(v) for v in found.values()) < a.want:
        tried += 1
        t = [float(np.float32(rng.uniform(0.25, 2.0))) for _ in range(3)]
        _, (m, d, _) = posterior(t, None, 1.0)
        if not (d[0] < 0.0 and m / -d[0] > 1.25):
            continue
        target = m / -d[0]  # member 0's result is 0 with this factor, in real numbers
        for fuse in ("lam", "qa"):
            if len(found[fuse]) >= a.want:
                continue
            if fuse == "lam":
                p, knob = None, target
            else:  # RTPS: a prior of about twice the spread about another mean; alpha carries lambda to the target
                p = [float(np.float32(m - 0.125 + 2.0 * dk + 0.05 * rng.normal())) for dk in d]
                _, (_, _, lam1) = posterior(t, p, 1.0)
                if not lam1 - 1.0 > 0.25:
                    continue
                knob = (target - 1.0) / (lam1 - 1.0)
            v0 = np.float32(knob)
            for step in range(-6, 7):
                v = v0
                for _ in range(abs(step)):
                    v = np.nextafter(v, np.float32(np.inf if step > 0 else -np.inf))
                coef = float(v)
                want, _ = posterior(t, p, coef)
                if not np.isfinite(want) or want == 0 or abs(float(want)) > 1e-5:
                    continue
                got, _ = posterior(t, p, coef, fuse)
                if len(found[fuse]) < a.want and got.view(np.uint32) != want.view(np.uint32):
                    found[fuse].append((fuse, "const" if p is None else "rtps", tuple(t), None if p is None else tuple(p), coef, int(want.view(np.uint32)),
                                        int(got.view(np.uint32))))
    print("# (product, mode, the three members' float32 values, their snapshot values or None, the float32 coefficient, member 0 after:")
    print("# defined bits, fused bits)")
    print("# %d configurations tried" % tried)
    print("SEPARATORS = [")
    for fuse in ("lam", "qa"):
        for s in found[fuse]:
            print("    %r," % (s,))
    print("]")


if __name__ == "__main__":
    main()
