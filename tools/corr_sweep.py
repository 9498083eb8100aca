"""Sweep of the blind autocorrelation estimate (include/lfbm5d_corr.h) with the numpy model (tests/corr_model.py), no GPU needed.

Data: the golden 3 x 3 x 256^2 light field plus white noise of lfbm5d_amd.synth's generator filtered by 7 x 7 Gaussian taps of width
0.5 or 0.8 pixels (lag-1 correlation 0.26 / 0.67), marginal sigma 10 or 25 (synth.add_correlated_noise, seed 1).  For every block size
and fraction: the root-mean-square log2 error of the variance table of the 8 x 8 DCT made from the estimate against the table of the
true autocorrelation (both clamped at 1 / 64), and the bias of the estimate's sigma.  The all-ones table's error is the yardstick.

Writes profiles/corr_defaults.txt with the `shipped:` row of the library's defaults (LFBM5D_CORR_DEFAULT_FRACTION, block 16), which
tests/test_corr.py reads back.

    python tools/corr_sweep.py
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corr_model as CM  # noqa: E402
from lfbm5d_amd import synth  # noqa: E402

DATA = [(0.5, 10.0), (0.5, 25.0), (0.8, 10.0), (0.8, 25.0)]
BLOCKS = (8, 16, 32)
FRACTIONS = (0.05, 0.1, 0.15, 0.25, 0.5, 1.0)


def shipped():
    src = open(os.path.join(ROOT, "include", "lfbm5d_corr.h")).read()
    return 16, float(re.search(r"#define LFBM5D_CORR_DEFAULT_FRACTION ([0-9.]+)", src).group(1))


def figures(width, sigma, B, fraction, lf=None):
    """(error of the estimate's table, error of the all-ones table, sigma bias in %, lag-1 correlations h and v, true lag-1)."""
    if lf is None:
        lf = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")).astype(np.float32)
    taps = CM.gaussian_taps(width)
    true_acf = CM.from_kernel(taps)
    true = CM.table(true_acf, "dct", 8)[1]
    noisy = synth.add_correlated_noise(lf, sigma, taps, seed=1)
    e = CM.measure(noisy, np.ones(lf.shape[0], np.uint32), B, fraction)
    v = CM.table(e["acf"], "dct", 8)[1]
    return CM.log2_rms(v, true), CM.log2_rms(np.ones(64), true), 100.0 * (e["sigma"] / sigma - 1.0), e["acf"][3, 4], e["acf"][4, 3], true_acf[3, 4]


def main():
    lf = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")).astype(np.float32)
    lines = ["# Blind autocorrelation estimate (lfbm5d_corr_measure_*): sweep of block size and fraction with the numpy model",
             "# (tools/corr_sweep.py), on ONE light field: the golden 3 x 3 x 256^2 views plus Gaussian-filtered white noise (7 x 7 taps).",
             "# Per cell: rms log2 error of the 8 x 8 DCT variance table against the true one (both clamped at 1/64) / bias of sigma in %.",
             "# `white` is the error of the all-ones table, i.e. of not using the feature.  Nothing here was measured on other content.",
             "width sigma block white | " + "  ".join("f=%-12.2f" % f for f in FRACTIONS)]
    B0, f0 = shipped()
    ship = []
    for width, sigma in DATA:
        for B in BLOCKS:
            cells = []
            for fr in FRACTIONS:
                err, white, bias, h, v, t = figures(width, sigma, B, fr, lf)
                cells.append("%.3f / %+6.1f" % (err, bias))
                if B == B0 and fr == f0:
                    ship.append("shipped: block %d fraction %.2f width %.1f sigma %2.0f | error %.3f white %.3f sigma bias %+.1f %% lag-1 %.3f %.3f (true %.3f)"
                                % (B, fr, width, sigma, err, white, bias, h, v, t))
            lines.append("%5.1f %5.0f %5d %5.2f | %s" % (width, sigma, B, white, "  ".join(cells)))
            print(lines[-1], flush=True)
    lines += ["# Choice: block 16, fraction 0.1.  On this smooth light field larger fractions do better at sigma 25 (the best cell of a row is",
              "# at 0.15 to 0.5), but at sigma 10 they let texture into the estimate (block 16, fraction 0.5: 0.72 and 0.90, as bad as white at",
              "# width 0.5), and busier content has more of it; smaller fractions are noisier and more biased.  0.1 keeps the error at or below",
              "# 0.39 on all four data sets.  Block 32 does better still here but leaves too few blocks on small images (a 3 x 3 x 64 x 64",
              "# light field has 4 per plane); block 8 sees lag 3 on few pairs and is the most biased.",
              "# The bias of sigma at the shipped setting is what include/lfbm5d_corr.h quotes."] + ship
    with open(os.path.join(ROOT, "profiles", "corr_defaults.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
