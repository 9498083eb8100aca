#!/usr/bin/env python3
"""Time of the blind noise-level estimate (lfbm5d_noise_level_*): the headline light field (17x17x512x512 colour, sigma 25) and
BASELINE's 15x15x625x434 (sigma 50), device-resident input and the host form, HIP-event time per call.  Prints one JSON line per
light field with the estimate, ms per call (device, device with per-SAI estimates, host), the achieved pixel rate and the share of
HBM bandwidth (one read of the light field; 6.3 TB/s achievable).
usage: python tools/noise_level_time.py [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import synth  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = L.Context(0)
    for ah, aw, H, W, sigma in ((17, 17, 512, 512, 25.0), (15, 15, 434, 625, 50.0)):
        A = ah * aw
        clean = torch.from_numpy(synth.make_lf(ah, aw, H, W).reshape(A, -1)).cuda().float()
        g = torch.Generator(device="cuda").manual_seed(1)
        d = clean + sigma * torch.randn(clean.shape, generator=g, device="cuda")
        del clean
        mask = np.ones(A, np.uint32)
        st = torch.cuda.ExternalStream(ctx.stream())

        def timed(fn):
            fn()                                            # warm-up (buffers, code objects)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(reps):
                e0.record(st)
                r = fn()                                    # returns with the stream synchronised
                e1.record(st)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return r, float(np.median(ms)), float(np.min(ms))

        r, dev_ms, dev_min = timed(lambda: ctx.noise_level(d, mask, W, H, 3))
        _, sai_ms, _ = timed(lambda: ctx.noise_level(d, mask, W, H, 3, per_sai=True))
        h = d.cpu().numpy()
        t0 = time.perf_counter()
        hr = ctx.noise_level(h, mask, W, H, 3)
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ctx.noise_level(h, mask, W, H, 3)
        host_ms2 = (time.perf_counter() - t0) * 1e3
        px = A * 3 * H * W
        print(json.dumps({"lf": f"{ah}x{aw}x{W}x{H}x3", "sigma": sigma, "estimate": r.sigma, "components": r.components,
                          "host_form_identical": hr.sigma == r.sigma and bool(np.array_equal(hr.eigen, r.eigen)),
                          "device_ms_median": round(dev_ms, 3), "device_ms_min": round(dev_min, 3), "device_per_sai_ms": round(sai_ms, 3),
                          "host_ms_first": round(host_ms, 1), "host_ms": round(host_ms2, 1),
                          "gpix_per_s": round(px / dev_ms / 1e6, 1), "hbm_fraction": round(px * 4 / (dev_ms * 1e-3) / 6.3e12, 4)}),
              flush=True)
        del d
    ctx.close()


if __name__ == "__main__":
    main()
