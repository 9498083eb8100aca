#!/usr/bin/env python3
"""The joint repair's default min_valid and the figures its tests cite, from the numpy model on the CPU (tests/repair_model.py on the
golden crops of tests/repair_cases.py).  Writes profiles/repair_defaults.txt.  Needs no GPU.

    python tools/repair_sweep.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import repair_cases as K    # noqa: E402

RULE = ("# Rule, written down before the sweep was run: min_valid is the value of {1, 2, 3, 4} with the largest mean, over the four rows\n"
        "# (two crops, sigma = 0 and 10), of the PSNR of the joint fill over the flagged values; values within 0.05 dB of the best count as\n"
        "# equal, and the smallest of them is taken (it fills the most values from the other views).")


def main():
    lines = ["# Joint repair (lfbm5d_repair_*): the default of min_valid and the figures of tests/test_repair.py, from tests/repair_model.py.",
             "# Golden light field 3 x 3 x 3 x 256 x 256, rows and columns lo..hi - 1, synth.add_defects(seed = 2) written as 0, D = 4, r = 3,",
             "# ang_radius = 1; sigma: white noise from default_rng(1) on every value.", RULE,
             "# crop, sigma: PSNR over the flagged values in dB at min_valid = 1, 2, 3, 4; the rim-inwards fill"]
    mean = [0.0] * 4
    for lo, hi in K.CROPS:
        for sigma in (0.0, 10.0):
            row = [K.fill_gain(lo, hi, min_valid=mv, sigma=sigma) for mv in (1, 2, 3, 4)]
            for i in range(4):
                mean[i] += row[i][0] / 4
            lines.append(f"{lo}..{hi - 1}, sigma {sigma:g}: " + ", ".join(f"{v[0]:.4f}" for v in row) + f"; rim {row[0][1]:.4f}")
            print(lines[-1])
    best = max(mean)
    pick = 1 + min(i for i in range(4) if mean[i] >= best - 0.05)
    lines.append("mean: " + ", ".join(f"{v:.4f}" for v in mean) + f" -> min_valid = {pick}")
    print(lines[-1])
    lines.append("# Gain from the mask: the synthesised SAI of crop 96..159 over all its positions, min_valid = 1 (a missing SAI has no value of")
    lines.append("# its own): mask-aware sweep on the defective light field, today's sweep on it, today's sweep on the clean light field; the")
    lines.append("# gain of the first over the second, and the threshold of the test (half of it)")
    for m, what in ((4, "centre"), (1, "edge"), (0, "corner")):
        a, u, c = K.mask_gain(m)
        lines.append(f"SAI {m} ({what}): {a:.4f}, {u:.4f}, {c:.4f}; gain {a - u:.4f}, threshold {(a - u) / 2:.4f}")
        print(lines[-1])
    lines.append(f"# Cross-view fill against the rim-inwards fill over the flagged values, sigma = 0, min_valid = {pick}: joint, rim; gain, threshold (half)")
    for lo, hi in K.CROPS:
        j, rim = K.fill_gain(lo, hi, min_valid=pick)
        lines.append(f"{lo}..{hi - 1}: {j:.4f}, {rim:.4f}; gain {j - rim:.4f}, threshold {(j - rim) / 2:.4f}")
        print(lines[-1])
    path = os.path.join(ROOT, "profiles", "repair_defaults.txt")
    keep = []
    if os.path.exists(path):                                                 # the loop's record is written by the test's own run
        keep = [l.rstrip("\n") for l in open(path) if l.startswith(("# Loop", "loop"))]
    with open(path, "w") as f:
        f.write("\n".join(lines + keep) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
