#!/usr/bin/env python3
"""Sweep of the super-resolution loop's iteration count K and sigma pair on the golden light field (tests/golden/sourceLF_3x3_256_u8.npy,
all 9 SAIs, colour), scales 2, 3, 4, bicubic D: the low-resolution input is the library's D of the source (scale 3: rows and columns
0..254), the hard-thresholding parameters are N=8, nSim=8, nDisp=3, k=8, p=3, dct / sadct / haar, lambda 2.7, opp, angular window 1.
Prints one line per setting (PSNR of the result against the source, mean over the SAIs), the best setting per scale and the best
setting of the form K, sigma_start = a * scale, sigma_end = b * scale over the three scales -- what lfbm5d_sr_defaults uses.
usage: python tools/superres_sweep.py [out]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import core  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, AS, BS = (4, 8, 12), (5.0, 10.0, 15.0), (0.5, 1.0, 2.0)


def psnr(a, b):
    mse = ((a.double() - b.double()) ** 2).mean(1)
    return float((10.0 * torch.log10(255.0 ** 2 / mse)).mean())


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)
    lf = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")).astype(np.float32)
    ctx = L.Context(0)
    mask = np.ones(9, np.uint32)
    P = core.make_params(0.0, 2.7, 8, 8, 3, 8, 3, "dct", "sadct", "haar")
    gain = {}
    for s in (2, 3, 4):
        n = 256 // s * s
        w = n // s
        hr = torch.from_numpy(np.ascontiguousarray(lf[:, :, :n, :n]).reshape(9, -1)).cuda()
        y = torch.zeros((9, 3 * w * w), dtype=torch.float32, device="cuda")
        res = torch.zeros_like(hr)
        ctx.sr_down(L.sr_defaults(s), hr, mask, y, w, w, 3)
        ctx.sr_up(L.sr_defaults(s), y, mask, res, w, w, 3)
        bic = psnr(res, hr)
        say(f"scale {s}: high resolution {n} x {n}, bicubic interpolation {bic:.3f} dB")
        for K in KS:
            for a in AS:
                for b in BS:
                    sr = L.sr_defaults(s, iterations=K, sigma_start=a * s, sigma_end=b * s)
                    ctx.superres(sr, P, y, mask, res, L.ROWMAJOR, 3, 3, 1, w, w, 3)
                    p = psnr(res, hr)
                    gain[(s, K, a, b)] = p - bic
                    say(f"  scale {s} K {K:2d} sigma {a * s:5.1f} -> {b * s:4.1f}: {p:.3f} dB ({p - bic:+.3f})")
        best = max((k for k in gain if k[0] == s), key=gain.get)
        say(f"  best at scale {s}: K {best[1]}, sigma {best[2] * s} -> {best[3] * s} ({gain[best]:+.3f} dB over bicubic)")
    common = max(((K, a, b) for K in KS for a in AS for b in BS), key=lambda t: sum(gain[(s,) + t] for s in (2, 3, 4)))
    say(f"best common setting: K {common[0]}, sigma_start {common[1]} * scale, sigma_end {common[2]} * scale "
        f"(gains {', '.join(f'{gain[(s,) + common]:+.3f}' for s in (2, 3, 4))} dB at scales 2, 3, 4)")
    d = L.sr_defaults(2)
    say(f"lfbm5d_sr_defaults: K {d.iterations}, sigma_start {d.sigma_start / 2} * scale, sigma_end {d.sigma_end / 2} * scale "
        "(this light field only: not claimed optimal beyond it)")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
