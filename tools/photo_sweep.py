#!/usr/bin/env python3
"""Sweep of the photometric equalisation's admission range and rounds with the numpy model (tests/photo_model.py; needs no GPU -- the GPU
equals the model bit for bit, tests/test_gpu_photo.py).  Two light fields of 3 x 3 views: the golden light field's rows and columns
64..159 (96 x 96 x 3), and the golden centre view's middle 64 x 64 rolled by 2 pixels per view (an exact translation).  Each at
sigma = 0 and with sigma = 10 noise (seed 1) added before the gains, under
  vignette 0.6 / 0.8   synth.vignette_gains(3, 3, edge)
  dim                  view 5 times 0.5
  cast                 channel 1 of view 2 times 1.1
Swept: lo in {4, 16, 32} x hi in {160, 200, 240} x max_rounds in {1, 2, 3}; everything else at the library's defaults.  Per row and input:
the largest relative error of a recovered gain once the free common factor is removed (per channel, the median of recovered / planted).
Rule: the row with the smallest maximum of that error over all inputs; ties go to the wider range, then to fewer rounds.
Writes profiles/photo_defaults.txt with the table, the row the rule picks and the `shipped:` row of the library's defaults.

    python tools/photo_sweep.py
"""
import itertools
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lfbm5d_amd as L                 # noqa: E402
from lfbm5d_amd import synth           # noqa: E402
import photo_model as M                # noqa: E402
import view_model as V                 # noqa: E402

LOS, HIS, ROUNDS = (4.0, 16.0, 32.0), (160.0, 200.0, 240.0), (1, 2, 3)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")


def fields():
    g = np.load(GOLDEN)
    crop = g[:, :, 64:160, 64:160].astype(np.float32)
    base = g[4][:, 96:160, 96:160].astype(np.float32)
    rolled = np.stack([np.roll(base, (2 * (s - 1), 2 * (t - 1)), axis=(1, 2)) for s in range(3) for t in range(3)])
    return (("golden crop", crop), ("translation", rolled))


def plantings():
    one = np.ones((9, 3))
    dim, cast = one.copy(), one.copy()
    dim[5] = 0.5
    cast[2, 1] = 1.1
    return (("vignette 0.6", np.repeat(synth.vignette_gains(3, 3, 0.6)[:, None], 3, axis=1)),
            ("vignette 0.8", np.repeat(synth.vignette_gains(3, 3, 0.8)[:, None], 3, axis=1)), ("dim", dim), ("cast", cast))


def inputs():
    out = []
    for fname, clean in fields():
        for sigma in (0, 10):
            noisy = synth.add_noise_mt19937(clean, float(sigma), seed=1) if sigma else clean
            for pname, g in plantings():
                out.append((f"{fname}, sigma {sigma}, {pname}", synth.apply_gains(noisy, g), g))
    return out


def error(G, planted):
    q = G / planted
    return float(np.abs(q / np.median(q, axis=0) - 1.0).max())


def job(args):
    """The errors after 1, 2 and 3 rounds of one input at one (lo, hi): a run of three rounds passes through the shorter ones."""
    lf, planted, lo, hi = args
    P = L.photo_params()
    A, C, H, W = lf.shape
    res = M.equalise(lf.reshape(A, -1), np.ones(A, np.uint32), V.ROWMAJOR, 3, 3, W, H, C, D=P.max_disparity, r=P.box_radius,
                     ang_radius=P.ang_radius, steps=P.steps, min_sources=P.min_sources, max_rounds=max(ROUNDS), tol=P.tol,
                     min_count=P.min_count, per_channel=P.per_channel, anchor=None, lo=lo, hi=hi)
    gains = res["gains"]
    return [error(gains[min(k, len(gains)) - 1] if gains else np.ones((A, 3)), planted) for k in ROUNDS]


def main():
    ins = inputs()
    grid = list(itertools.product(LOS, HIS))
    work = [(lf, g, lo, hi) for lo, hi in grid for _, lf, g in ins]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        errs = pool.map(job, work)
    table = {}
    for (lo, hi), chunk in zip(grid, [errs[i * len(ins):(i + 1) * len(ins)] for i in range(len(grid))]):
        for ki, k in enumerate(ROUNDS):
            table[(lo, hi, k)] = [e[ki] for e in chunk]
    best = min(table, key=lambda row: (round(max(table[row]), 4), -(row[1] - row[0]), row[2]))
    P = L.photo_params()
    shipped = (P.lo, P.hi, P.max_rounds)
    lines = ["# Photometric equalisation (lfbm5d_photo_*): sweep of lo, hi and max_rounds with the numpy model (tools/photo_sweep.py).",
             "# Per row: the largest relative error of a recovered gain, common factor removed, in per cent, per input; then the row's maximum.",
             "# The golden crop's own views differ by about 1 % with nothing planted: that is the floor of its columns.",
             "# inputs: " + " | ".join(f"{i}: {name}" for i, (name, _, _) in enumerate(ins)),
             "# lo, hi, max_rounds: " + " ".join(f"{i:>5d}" for i in range(len(ins))) + "   max"]
    for row in sorted(table):
        lines.append(f"{row[0]:g}, {row[1]:g}, {row[2]}: " + " ".join(f"{100 * e:5.2f}" for e in table[row]) + f" {100 * max(table[row]):5.2f}")
    lines.append(f"rule (smallest maximum, rounded to 0.01 %; ties: the wider range, then fewer rounds): lo = {best[0]:g}, hi = {best[1]:g}, "
                 f"max_rounds = {best[2]}: {100 * max(table[best]):.2f} %")
    lines.append(f"shipped: lo = {shipped[0]:g}, hi = {shipped[1]:g}, max_rounds = {shipped[2]}: "
                 + (f"{100 * max(table[shipped]):.2f} %" if shipped in table else "not a row of this sweep"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "photo_defaults.txt"), "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
