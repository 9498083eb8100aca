#!/usr/bin/env python3
"""Measurements of the Poisson-Gaussian noise routines (lfbm5d_pg_*, lfbm5d_denoise_pg_*) for profiles/pg_noise.txt, one JSON line each:
  - accuracy: the GPU estimate on the whole golden light field (3x3x256x256x3) under synthetic noise (numpy seed 1) for the (a, b) of
    tests/test_pg_noise.py: fitted (a, b) and the relative error of the fitted variance at the light field's mean level 121.4;
  - timings on 17x17x512x512x3, device-resident: the statistics call (lfbm5d_pg_histogram_device: SAI list upload, zero-fill, kernel,
    download of the counts, synchronise), the forward and the inverse transform (out of place); HIP events on the context's stream
    around a batch of whole calls, warm-up first, `reps` windows with the three alternating; median / min / max / std of the per-call
    time, next to the byte floor at the 6.3 TB/s the project uses (statistics: one read of the light field; transforms: one read and
    one write) and the ratio to it;
  - the whole denoise_pg against denoise on that light field (README parameters, model given; median of `job_reps` runs each);
  - benefit: PSNR on the 3x3x64x64 golden crop under a = 8, b = 0 (numpy seed 1): denoise with sigma = sqrt(mean(8 clean)), denoise_pg
    with the true model, denoise_pg with the estimated model.
The lines are printed and written to the output file (the CLI figures at the end of profiles/pg_noise.txt come from
tests/test_gpu_pg_noise.py and are kept by hand).
usage: python tools/pg_time.py [reps] [output file, default profiles/pg_noise.txt] [batch] [job_reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import core, synth  # noqa: E402

HBM = 6.3e12
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
P1 = lambda s: core.make_params(s, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")
P2 = lambda s: core.make_params(s, 2.7, 16, 18, 6, 8, 4, "dct", "sadct", "haar")


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def accuracy(ctx, out):
    lf = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    for a, b in ((1.0, 0.0), (0.5, 4.0), (2.0, 25.0), (0.0, 100.0), (0.25, 1.0)):
        e = ctx.pg_estimate(torch.from_numpy(synth.add_poisson_gaussian(lf, a, b, 1)).cuda(), mask, 256, 256, 3)
        out({"accuracy": "golden 3x3x256x256x3, seed 1", "true_a": a, "true_b": b, "a": round(e.a, 5), "b": round(e.b, 4),
             "a_channel": [round(v, 5) for v in e.a_channel], "b_channel": [round(v, 4) for v in e.b_channel],
             "variance_at_121.4_relative_error": round((e.a * 121.4 + e.b) / (a * 121.4 + b) - 1.0, 4)})
    e = ctx.pg_estimate(torch.from_numpy(lf).cuda(), mask, 256, 256, 3)
    out({"accuracy": "golden 3x3x256x256x3, no noise added", "a": round(e.a, 5), "b": round(e.b, 4)})


def timings(ctx, out, reps, batch, job_reps):
    ah = aw = 17
    H = W = 512
    A = ah * aw
    mask = np.ones(A, np.uint32)
    clean = torch.from_numpy(synth.make_lf(ah, aw, H, W).reshape(A, -1)).cuda().float()
    g = torch.Generator(device="cuda").manual_seed(1)
    model = (2.0, 25.0)
    noisy = clean + torch.sqrt(model[0] * clean + model[1]) * torch.randn(clean.shape, generator=g, device="cuda")
    del clean
    t, back = torch.empty_like(noisy), torch.empty_like(noisy)
    st = torch.cuda.ExternalStream(ctx.stream())
    fns = (lambda: ctx.pg_histogram(noisy, mask, W, H, 3), lambda: ctx.pg_forward(model, noisy, mask, t, W, H, 3),
           lambda: ctx.pg_inverse(model, t, mask, back, W, H, 3))
    for fn in fns:
        fn()                                                # warm-up (buffers, code objects)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = ([], [], [])
    for _ in range(reps):
        for which, fn in enumerate(fns):
            e0.record(st)
            for _ in range(batch):
                fn()                                        # returns with the stream synchronised
            e1.record(st)
            e1.synchronize()
            ms[which].append(e0.elapsed_time(e1) / batch)
    nbytes = A * 3 * H * W * 4
    floors = (nbytes / HBM * 1e3, 2 * nbytes / HBM * 1e3, 2 * nbytes / HBM * 1e3)
    rec = {"lf": f"{ah}x{aw}x{W}x{H}x3", "windows": reps, "calls_per_window": batch}
    for name, v, fl, nb in zip(("statistics", "forward", "inverse"), ms, floors, (nbytes, 2 * nbytes, 2 * nbytes)):
        rec[name] = {"ms_per_call": stats(v), "bytes": nb, "floor_ms_at_6.3TBps": round(fl, 4), "over_floor": round(float(np.median(v)) / fl, 2)}
    out(rec)
    del t, back
    basic, den = torch.empty_like(noisy), torch.empty_like(noisy)
    s = L.pg_scale(model)
    tail = (L.ROWMAJOR, aw, ah, 1, 1, W, H, 3)
    jobs = (lambda: ctx.denoise(P1(s), P2(s), noisy.clone(), mask, basic, den, *tail),
            lambda: ctx.denoise_pg(model, P1(s), P2(s), noisy, mask, basic, den, *tail))
    jm = ([], [])
    for fn in jobs:
        fn()
    for _ in range(job_reps):
        for which, fn in enumerate(jobs):
            arg = noisy.clone() if which == 0 else None     # denoise works on its input in place: the copy stays outside the window
            e0.record(st)
            if which == 0:
                ctx.denoise(P1(s), P2(s), arg, mask, basic, den, *tail)
            else:
                fn()
            e1.record(st)
            e1.synchronize()
            jm[which].append(e0.elapsed_time(e1))
    out({"lf": rec["lf"], "job_runs": job_reps, "denoise_ms": stats(jm[0]), "denoise_pg_ms": stats(jm[1]),
         "denoise_pg_over_denoise": round(float(np.median(jm[1]) / np.median(jm[0])), 4)})


def benefit(ctx, out):
    clean = np.ascontiguousarray(np.load(GOLDEN)[:, :, :64, :64], np.float32).reshape(9, -1)
    noisy = synth.add_poisson_gaussian(clean, 8.0, 0.0, 1)
    mask = np.ones(9, np.uint32)
    tail = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
    psnr = lambda x: float(10.0 * np.log10(255.0 ** 2 / ((x.cpu().numpy().astype(np.float64) - clean) ** 2).mean()))
    d = torch.from_numpy(noisy).cuda()
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    sg = float(np.sqrt((8.0 * clean).mean()))
    ctx.denoise(P1(sg), P2(sg), d.clone(), mask, basic, den, *tail)
    rec = {"benefit": "golden crop 3x3x64x64x3, a = 8, b = 0, seed 1", "global_sigma": round(sg, 4), "psnr_denoise_global_sigma": round(psnr(den), 4)}
    ctx.denoise_pg((8.0, 0.0), P1(sg), P2(sg), d, mask, basic, den, *tail)
    rec["psnr_denoise_pg_true_model"] = round(psnr(den), 4)
    used = ctx.denoise_pg(None, P1(sg), P2(sg), d, mask, basic, den, *tail)
    rec["psnr_denoise_pg_estimated_model"] = round(psnr(den), 4)
    rec["estimated_model"] = [round(used.a[0], 4), round(used.b[0], 4)]
    out(rec)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pg_noise.txt")
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    job_reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    lines = []

    def out(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ctx = L.Context(0)
    accuracy(ctx, out)
    benefit(ctx, out)
    timings(ctx, out, reps, batch, job_reps)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/pg_time.py %d <file> %d %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % (reps, batch, job_reps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
