#!/usr/bin/env python3
"""Sweep of the inpainting loop's step count K and sigma pair on the golden light field (tests/golden/sourceLF_3x3_256_u8.npy, all 9
SAIs, colour, 256 x 256): the defect map is synth.add_defects((9, 3, 64, 64), 3) tiled 4 x 4 (6.04 % of the values), the flagged values
are set to 0, the data is clean, the hard-thresholding parameters are N=8, nSim=8, nDisp=3, k=8, p=3, dct / sadct / haar, lambda 2.7,
opp, angular window 1.  Prints one line per setting (PSNR over the flagged values against the source) and the best one -- what
lfbm5d_inpaint_defaults uses; a second block repeats the sweep at sigma = 10 noise with sigma_noise = 10 (whole-field PSNR of the loop's
output against the source is not the figure there: the PSNR over the flagged values is).
usage: python tools/inpaint_sweep.py [out]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import core, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, STARTS, ENDS = (2, 4, 8), (20.0, 30.0, 40.0), (3.0, 5.0, 10.0)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)
    clean = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")).astype(np.float32).reshape(9, -1)).cuda()
    fl = torch.from_numpy(np.tile(synth.add_defects((9, 3, 64, 64), 3), (1, 1, 4, 4)).reshape(9, -1)).cuda()
    f8 = fl.to(torch.uint8)
    ctx = L.Context(0)
    mask = np.ones(9, np.uint32)
    P = core.make_params(0.0, 2.7, 8, 8, 3, 8, 3, "dct", "sadct", "haar")
    tail = (L.ROWMAJOR, 3, 3, 1, 256, 256, 3)

    def psnr(x):
        return float(10.0 * torch.log10(255.0 ** 2 / ((x.double() - clean.double())[fl] ** 2).mean()))
    gen = torch.Generator(device="cuda").manual_seed(1)
    noise = 10.0 * torch.randn(clean.shape, generator=gen, device="cuda")
    best = {}
    for label, data, sn in (("clean data", clean, 0.0), ("sigma 10 noise, sigma_noise 10", clean + noise, 10.0)):
        y = torch.where(fl, 0.0, data).contiguous()
        fill = psnr(ctx.inpaint_fill(y, f8, mask, 256, 256, 3).out)
        say(f"{label}: {100.0 * float(fl.float().mean()):.2f} % flagged, fill alone {fill:.3f} dB over the flagged values")
        res = {}
        for K in KS:
            for s0 in STARTS:
                for s1 in ENDS:
                    r = ctx.inpaint(y, f8, mask, P, *tail, iterations=K, sigma_start=s0, sigma_end=s1, sigma_noise=sn)
                    res[(K, s0, s1)] = psnr(r.out)
                    say(f"  K {K} sigma {s0:4.1f} -> {s1:4.1f}: {res[(K, s0, s1)]:.3f} dB ({res[(K, s0, s1)] - fill:+.3f})")
        b = max(res, key=res.get)
        b4 = max((k for k in res if k[0] == 4), key=res.get)
        best[label] = b
        say(f"  best: K {b[0]}, sigma {b[1]} -> {b[2]} ({res[b]:.3f} dB); best with K = 4: sigma {b4[1]} -> {b4[2]} ({res[b4]:.3f} dB)")
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("# tools/inpaint_sweep.py (MI355X): golden light field 3x3x256x256x3, PSNR over the flagged values\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
