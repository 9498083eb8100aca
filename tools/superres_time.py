#!/usr/bin/env python3
"""Time of the super-resolution operators and loop (lfbm5d_sr_* / lfbm5d_superres_device) at the headline angular size: 17x17 SAIs,
256 x 256 -> 512 x 512 colour, scale 2, bicubic D.  HIP-event time of D, U, one back-projection (two launches), one hard-thresholding
step on the high-resolution light field and the whole loop (the library's defaults), with the byte floor of the back-projection's two
launches -- reads x, y, r; writes r, z (the update launch reads x a second time for its epilogue, counted separately) -- at
6.3 TB/s achievable HBM bandwidth, and the back-projection's share of a step.  Prints one JSON line; `out` also receives it.
usage: python tools/superres_time.py [reps] [out]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import core, synth  # noqa: E402

HBM = 6.3e12


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out = sys.argv[2] if len(sys.argv) > 2 else None
    ah = aw = 17
    w = h = 256
    s = 2
    W, H, A = w * s, h * s, ah * aw
    ctx = L.Context(0)
    sr = L.sr_defaults(s)
    mask = np.ones(A, np.uint32)
    x = torch.from_numpy(synth.make_lf(ah, aw, H, W).reshape(A, -1)).cuda().float()
    y = torch.zeros((A, 3 * w * h), dtype=torch.float32, device="cuda")
    z = torch.zeros_like(x)
    ctx.sr_down(sr, x, mask, y, w, h, 3)
    st = torch.cuda.ExternalStream(ctx.stream())

    def timed(fn, n):
        fn()                                                # warm-up (buffers, tables, code objects)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(n):
            e0.record(st)
            fn()                                            # returns with the stream synchronised
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    down = timed(lambda: ctx.sr_down(sr, x, mask, y, w, h, 3), reps)
    up = timed(lambda: ctx.sr_up(sr, y, mask, z, w, h, 3), reps)
    bp = timed(lambda: ctx.sr_backproject(sr, y, x, mask, z, w, h, 3), reps)
    P = core.make_params(sr.sigma_start, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")
    basic = torch.zeros_like(x)
    step = timed(lambda: ctx.step1(P, z, mask, basic, L.ROWMAJOR, aw, ah, 1, W, H, 3), 1)
    loop = timed(lambda: ctx.superres(sr, P, y, mask, z, L.ROWMAJOR, aw, ah, 1, w, h, 3), 1)
    hi, lo = A * 3 * W * H * 4, A * 3 * w * h * 4
    floor_bytes = 2 * hi + 3 * lo
    floor_ms = floor_bytes / HBM * 1e3
    rec = {"lf": f"{ah}x{aw} {w}x{h}->{W}x{H}x3", "scale": s, "iterations": sr.iterations, "reps": reps,
           "down_ms_median": round(down[0], 3), "down_ms_min": round(down[1], 3), "up_ms_median": round(up[0], 3), "up_ms_min": round(up[1], 3),
           "backproject_ms_median": round(bp[0], 3), "backproject_ms_min": round(bp[1], 3),
           "floor_gb": round(floor_bytes / 1e9, 3), "floor_gb_with_second_read_of_x": round((floor_bytes + hi) / 1e9, 3),
           "floor_ms_at_6.3TBps": round(floor_ms, 3), "backproject_over_floor": round(bp[0] / floor_ms, 2),
           "step1_ms": round(step[0], 1), "backproject_over_step": round(bp[0] / step[0], 5),
           "loop_ms": round(loop[0], 1), "loop_over_steps": round(loop[0] / (sr.iterations * step[0]), 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
