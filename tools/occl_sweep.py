#!/usr/bin/env python3
"""The sweep behind lfbm5d_view_occl_default(): PSNR of the synthesised SAI with the exact model (tests/occl_model.py, CPU) for the
ratios 1, 2, 4, 8, 16 and the plain sweep, at steps 1 and 2, clean and with Gaussian noise of sigma 10 on the sources, on the golden
crop (rows and columns 64..191) with the centre and with edge SAI 1 missing and on the two occluder scenes of tests/occl_cases.py at
96 x 96 with the centre missing.  D = 4, r = 3.  Writes profiles/occl_defaults.txt.

    python tools/occl_sweep.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import occl_cases as K        # noqa: E402
import occl_model as O        # noqa: E402
import subpel_model as S      # noqa: E402
import view_model as V        # noqa: E402

RATIOS = (1.0, 2.0, 4.0, 8.0, 16.0)
D, R = 4, 3


def cases():
    crop = np.load(K.K.GOLDEN)[:, :, 64:192, 64:192].astype(np.float32).reshape(9, -1)
    yield "golden crop 64..191, centre missing", crop, 128, 128, 4
    yield "golden crop 64..191, edge SAI 1 missing", crop, 128, 128, 1
    for scene in ("rect", "stripes"):
        yield f"{scene} occluder scene 96 x 96, centre missing", K.occluder_lf(scene, 3, 3, 96, 96, 3), 96, 96, 4


def main():
    mask = np.ones(9, np.uint32)
    head = "case, data, steps: plain sweep | " + " | ".join(f"ratio {r:g}" for r in RATIOS) + "  (PSNR of the synthesised SAI, dB)"
    lines = ["# Occlusion-aware view synthesis (lfbm5d_view_*_occl_*): the sweep behind lfbm5d_view_occl_default().  The exact model",
             "# (tests/occl_model.py) on the CPU; D = 4, r = 3, 3 x 3 views; noisy = Gaussian noise of sigma 10 on the sources (seed 1).",
             "# One sweep on one light field (the golden crop) plus two synthetic occluder scenes (tests/occl_cases.py: a background at",
             "# disparity -1, occluders at +3): it says which ratio to ship, not what to expect on other data.", "# " + head]
    table = []
    for name, clean, H, W, m in cases():
        missing = np.zeros(9, np.uint32)
        missing[m] = 1
        for noisy in (False, True):
            lf = clean.copy()
            if noisy:
                lf = (lf + np.random.default_rng(1).normal(0.0, 10.0, lf.shape)).astype(np.float32)
            x = lf.reshape(9, 3, H, W)
            srcs = V.sources(m, mask, missing, V.ROWMAJOR, 3, 3, 1)
            for Q in (1, 2):
                plain = V.psnr(S.synth_view(x, srcs, D, R, Q)[0], clean[m].reshape(3, H, W))
                swept = O.sweep_errors(x, srcs, D, Q)
                row = [V.psnr(O.decide(swept, r, R)[0], clean[m].reshape(3, H, W)) for r in RATIOS]
                table.append(row)
                line = f"{name}, {'sigma 10' if noisy else 'clean'}, steps {Q}: {plain:.2f} | " + " | ".join(f"{v:.2f}" for v in row)
                print(line, flush=True)
                lines.append(line)
    mean = np.mean(np.array(table), axis=0)
    best = RATIOS[int(np.argmax(mean))]
    lines.append("mean over the rows: " + " | ".join(f"ratio {r:g}: {v:.2f}" for r, v in zip(RATIOS, mean)))
    lines.append(f"best mean: ratio {best:g} -> lfbm5d_view_occl_default()")
    print("\n".join(lines[-2:]))
    with open(os.path.join(ROOT, "profiles", "occl_defaults.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
