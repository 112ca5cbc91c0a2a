#!/usr/bin/env python
"""Planted vx values whose measured-stage |vx| straddles a threshold of the velocity watch (tests/watch_scenes.py STRADDLES).

The watch compares an intermediate of the iteration -- the wet kernel's post-boundary velocity (oracle pass mask 7), the dry
kernels' velocity pass output (mask 1) -- with 0.5 (record), cone - 5 (period limit: 1.0, and 2.0 after a bound of 0.7) and
2 * halo - 8 (interior limit: 16). What is planted is the uploaded vx of one cell, so the pair is found by bisection over the
float32 planted values on the CPU oracle: the largest one measured below the threshold and its float32 successor. Prints the
literals and the gap between the two measured values relative to the threshold. No GPU.

  python tools/find_watch_straddles.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def bisect(measure, threshold, lo=0.25, hi=64.0):
    """float32 planted values (a, b), b the successor of a, with measure(a) < threshold <= measure(b)."""
    lo, hi = np.float32(lo), np.float32(hi)
    assert measure(lo) < threshold <= measure(hi), (measure(lo), measure(hi))
    while np.nextafter(lo, np.float32(np.inf)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if measure(mid) < threshold:
            lo = mid
        else:
            hi = mid
    return lo, hi


def main():
    import wx_oracle
    import watch_scenes as W
    wx_oracle.build()
    for name, (_, _, _, thr) in W.STRADDLE_SITES.items():
        for stage in (7, 1):
            thr32 = np.float32(thr)
            a, b = bisect(lambda v: W.straddle_measured(wx_oracle, name, stage, float(v)), thr32)
            ma, mb = W.straddle_measured(wx_oracle, name, stage, float(a)), W.straddle_measured(wx_oracle, name, stage, float(b))
            print(f'    ("{name}", {stage}): ({float(a)!r}, {float(b)!r}),  # measured {float(ma)!r} < {thr} <= {float(mb)!r}: gap {float(mb - ma) / thr:.3g} of the threshold')


if __name__ == "__main__":
    main()
