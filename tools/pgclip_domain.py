#!/usr/bin/env python3
"""The accepted domain of the clipped Poisson-Gaussian curves: a CPU Monte-Carlo table with real Poisson draws.

For every (a, a^2 / b) of the grid the curves of tests/pgclip_model.py are built with the domain check off, then at every true value y
of the list z = clip(lo + a Poisson((y - lo) / a) + sqrt(b) n, lo, hi) is drawn `--draws` times and mapped through the float32 tables.
Printed per row: the largest |inverse(mean forward(z)) - y| and the extremes of std forward(z) / s over the y >= lo + 5.  A row
qualifies when it keeps the bias <= 0.3 grey levels and the deviation within [0.70, 1.15]; the accepted domain is the widest ratio of
the grid at which every row up to a gain a_max qualifies, with a_max the largest gain that has such a ratio above 0.2 (DESIGN 3o
reads the table).  The bias carries the Monte-Carlo error of a mean of `--draws` values, about 0.05 grey levels at the default.  No GPU.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pgclip_model as M  # noqa: E402


def row(a, b, lo, hi, draws, rng):
    cv = M.curves(a, b, lo, hi, domain=False)
    if cv is None:
        return None
    mid = 0.5 * (lo + hi)
    bias = 0.0
    dmin, dmax = np.inf, -np.inf
    for y in (lo + 5, lo + 10, lo + 20, lo + 50, mid, hi - 20, hi - 5, hi):
        z = lo + a * rng.poisson((y - lo) / a, draws) + np.sqrt(b) * rng.standard_normal(draws)
        f = M.forward(np.clip(z, lo, hi).astype(np.float32), cv).astype(np.float64)
        back = float(M.inverse(np.float32(f.mean()), cv))
        bias = max(bias, abs(back - y))
        d = f.std() / cv["s"]
        dmin, dmax = min(dmin, d), max(dmax, d)
    return bias, dmin, dmax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1600000)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    print("a      a^2/b   b         bias    std/s min  std/s max  qualifies")
    for ratio in (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.75, 1.0, 2.0, 4.0):
        for a in (0.5, 1.0, 2.0, 4.0, 5.0, 6.0, 8.0):
            b = a * a / ratio
            r = row(a, b, 0.0, 255.0, args.draws, rng)
            if r is None:
                print(f"{a:<6g} {ratio:<7g} {b:<9.4g} curves refused")
                continue
            ok = r[0] <= 0.3 and r[1] >= 0.70 and r[2] <= 1.15
            print(f"{a:<6g} {ratio:<7g} {b:<9.4g} {r[0]:<7.3f} {r[1]:<10.3f} {r[2]:<10.3f} {'yes' if ok else 'no'}", flush=True)


if __name__ == "__main__":
    main()
