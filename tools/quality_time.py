#!/usr/bin/env python3
"""Time of the quality metrics (lfbm5d_quality_*): the headline light field (17x17x512x512 colour) and 9x9x512x512, device-resident
inputs.  Per light field one JSON line with
  - ms per call without and with SSIM: HIP events on the context's stream around a batch of `batch` whole calls (each the SAI
    list's upload, the kernels, the download of two doubles per SAI and a synchronise), so that a timed window is tens of
    milliseconds and not one call; warm-up first; `reps` windows, alternating between the two forms; median, minimum, maximum and
    standard deviation of the per-call time over the windows,
  - the byte floor (one read of each light field, 2 * asize * C * H * W * 4 bytes) in ms at the 6.3 TB/s the project uses, and the
    ratio of each call to it,
  - the same PSNR on the host: both light fields copied to the host, then the reference's serial float loop per SAI (the oracle's
    compute_psnr), copy and loop timed together and apart,
  - the float64 numpy model (tests/quality_model.py) on `model_sais` SAIs, and that time scaled to the light field.
The lines are printed and written to the output file.
usage: python tools/quality_time.py [reps] [output file, default profiles/quality_time.txt] [batch]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
import quality_model as Q  # noqa: E402

HBM = 6.3e12
MODEL_SAIS = 2


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "quality_time.txt")
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    ctx = L.Context(0)
    lines = []
    for ah, aw, H, W, sigma in ((17, 17, 512, 512, 25.0), (9, 9, 512, 512, 25.0)):
        A = ah * aw
        ref = torch.from_numpy(synth.make_lf(ah, aw, H, W).reshape(A, -1)).cuda().float()
        g = torch.Generator(device="cuda").manual_seed(1)
        test = ref + sigma * torch.randn(ref.shape, generator=g, device="cuda")
        mask = np.ones(A, np.uint32)
        st = torch.cuda.ExternalStream(ctx.stream())

        fns = (lambda: ctx.quality(ref, test, mask, W, H, 3, ssim=False), lambda: ctx.quality(ref, test, mask, W, H, 3, ssim=True))
        q0, q1 = (fn() for fn in fns)                       # warm-up (buffers, code objects)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = ([], [])
        for _ in range(reps):
            for which, fn in enumerate(fns):                # the two forms alternate, window by window
                e0.record(st)
                for _ in range(batch):
                    fn()                                    # returns with the stream synchronised
                e1.record(st)
                e1.synchronize()
                ms[which].append(e0.elapsed_time(e1) / batch)
        stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
                           "std": round(float(np.std(v)), 4)}
        mse_ms, ssim_ms = float(np.median(ms[0])), float(np.median(ms[1]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_ref, h_test = ref.cpu().numpy(), test.cpu().numpy()
        t1 = time.perf_counter()
        host_psnr = float(np.mean([O.psnr(h_ref[i], h_test[i]) for i in range(A)]))
        t2 = time.perf_counter()
        t3 = time.perf_counter()
        m = Q.model(h_ref[:MODEL_SAIS], h_test[:MODEL_SAIS], np.ones(MODEL_SAIS, np.uint32), W, H, 3)
        model_s = time.perf_counter() - t3
        nbytes = 2 * A * 3 * H * W * 4
        floor_ms = nbytes / HBM * 1e3
        lines.append(json.dumps({
            "lf": f"{ah}x{aw}x{W}x{H}x3", "sigma": sigma, "psnr_mean": q1.psnr_mean, "ssim_mean": q1.ssim_mean,
            "mse_bits_equal_with_and_without_ssim": bool(np.array_equal(q0.rmse_sai, q1.rmse_sai)),
            "windows": reps, "calls_per_window": batch, "mse_only_ms_per_call": stats(ms[0]), "mse_ssim_ms_per_call": stats(ms[1]),
            "bytes": nbytes, "floor_ms_at_6.3TBps": round(floor_ms, 4),
            "mse_only_over_floor": round(mse_ms / floor_ms, 2), "mse_ssim_over_floor": round(ssim_ms / floor_ms, 2),
            "host_psnr_mean": host_psnr, "host_d2h_ms": round((t1 - t0) * 1e3, 1), "host_float_loop_ms": round((t2 - t1) * 1e3, 1),
            "host_total_ms": round((t2 - t0) * 1e3, 1),
            "model_sais": MODEL_SAIS, "model_ms_per_sai": round(model_s * 1e3 / MODEL_SAIS, 1),
            "model_ms_scaled_to_lf": round(model_s * 1e3 / MODEL_SAIS * A, 0),
            "model_ssim_difference_on_those_sais": float(np.abs(q1.ssim_sai[:MODEL_SAIS] - m["ssim_sai"]).max())}))
        print(lines[-1], flush=True)
        del ref, test
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/quality_time.py %d <file> %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % (reps, batch))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
