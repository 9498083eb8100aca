#!/usr/bin/env python3
"""Sweep of the view synthesis' parameters on the golden light field (tests/golden/sourceLF_3x3_256_u8.npy, all 9 SAIs, colour,
256 x 256, clean data): max_disparity D, box_radius r, and the loop's step count K and sigma pair, with the centre, a corner and an edge
SAI missing (one at a time).  The hard-thresholding parameters are N=8, nSim=8, nDisp=3, k=8, p=3, dct / sadct / haar, lambda 2.7, opp,
angular window 1.  Prints one line per setting (PSNR of the reconstructed SAI against the source, per position and their mean) and the
best row -- what lfbm5d_view_defaults ships; K = 0 is the synthesis alone.  The loop rows of a (D, r) pair start from that pair's
synthesis.  With a time budget (seconds) the (D, r) pairs get their loop rows in the order of their K = 0 result, best first, and the
pairs that the budget did not reach are named.
usage: python tools/view_sweep.py [out] [budget in seconds]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import core  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS, RS, KS, STARTS, ENDS = (2, 3, 4, 6), (2, 3, 5), (2, 4, 8), (20.0, 30.0, 40.0), (3.0, 5.0, 10.0)
POSITIONS = (("centre", 4), ("corner", 0), ("edge", 1))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    budget = float(sys.argv[2]) if len(sys.argv) > 2 else None
    t0 = time.time()
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)
        if out:
            with open(out, "w") as f:
                f.write("# tools/view_sweep.py (MI355X): golden light field 3x3x256x256x3, clean; PSNR of the reconstructed SAI, dB: "
                        "centre corner edge | mean\n" + "\n".join(lines) + "\n")
    clean = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")).astype(np.float32).reshape(9, -1)).cuda()
    ctx = L.Context(0)
    mask = np.ones(9, np.uint32)
    P = core.make_params(0.0, 2.7, 8, 8, 3, 8, 3, "dct", "sadct", "haar")
    tail = (L.ROWMAJOR, 3, 3, 1, 256, 256, 3)

    def psnr(x, m):
        return float(10.0 * torch.log10(255.0 ** 2 / ((x[m].double() - clean[m].double()) ** 2).mean()))

    def run(D, r, K, s0, s1):
        res = []
        for _, m in POSITIONS:
            missing = np.zeros(9, np.uint32)
            missing[m] = 1
            y = clean.clone()
            y[m] = 0.0
            res.append(psnr(ctx.view_synth(y, mask, missing, P, *tail, max_disparity=D, box_radius=r, ang_radius=1, iterations=K,
                                           sigma_start=s0, sigma_end=s1).out, m))
        return res

    def row(label, v):
        return f"{label}: {v[0]:.3f} {v[1]:.3f} {v[2]:.3f} | {np.mean(v):.3f}"
    say(row("mean of the neighbours (D 0, r 0)", run(0, 0, 0, 30.0, 5.0)))
    res = {}
    for D in DS:
        for r in RS:
            res[(D, r, 0, 0.0, 0.0)] = run(D, r, 0, 30.0, 5.0)
            say(row(f"D {D} r {r} K 0", res[(D, r, 0, 0.0, 0.0)]))
    skipped = []
    for D, r in sorted(((D, r) for D in DS for r in RS), key=lambda k: -np.mean(res[(k[0], k[1], 0, 0.0, 0.0)])):
        if budget is not None and time.time() - t0 > budget:
            skipped.append((D, r))
            continue
        for K in KS:
            for s0 in STARTS:
                for s1 in ENDS:
                    res[(D, r, K, s0, s1)] = run(D, r, K, s0, s1)
                    say(row(f"D {D} r {r} K {K} sigma {s0:4.1f} -> {s1:4.1f}", res[(D, r, K, s0, s1)])
                        + f" ({np.mean(res[(D, r, K, s0, s1)]) - np.mean(res[(D, r, 0, 0.0, 0.0)]):+.3f} over K 0)")
    b = max(res, key=lambda k: np.mean(res[k]))
    b0 = max((k for k in res if k[2] == 0), key=lambda k: np.mean(res[k]))
    say(f"best: D {b[0]} r {b[1]} K {b[2]} sigma {b[3]} -> {b[4]} ({np.mean(res[b]):.3f} dB); best with K = 0: D {b0[0]} r {b0[1]} "
        f"({np.mean(res[b0]):.3f} dB)")
    if skipped:
        say("loop rows not run within the time budget for (D, r) = " + ", ".join(f"({D}, {r})" for D, r in skipped))
    ctx.close()


if __name__ == "__main__":
    main()
