#!/usr/bin/env python3
"""Measurements of the clipping-aware routines (lfbm5d_clip_*, lfbm5d_declip_*, lfbm5d_denoise_clipped_*) for profiles/clip.txt, one JSON
line each:
  - estimate: noise_level_clipped on the whole golden light field (3x3x256x256x3) under MT19937 noise (seed 1) of sigma 5 .. 75, rounded
    and clipped to 0..255, next to the blind estimate (noise_level) on the same input; and on the float noise at sigma 25;
  - psnr: on the tile rows 192..255, columns 128..191 of the golden light field, rounded and clipped (sigma 25 with the README
    parameters, sigma 50 with those of BASELINE.json configs[4]): denoise, denoise_clipped with the sigma given, denoise_clipped with
    the sigma estimated; PSNR against the clean tile over all values;
  - timings on 17x17x512x512x3, device-resident: the statistics call (lfbm5d_clip_histogram_device: SAI list, zero-fill, kernel, download
    of the counts, synchronise) and the declip call (out of place) at sigma 25; HIP events on the context's stream around a batch of whole
    calls, warm-up first, `reps` windows with the two alternating; median / min / max / std of the per-call time, next to the byte floor
    at the 6.3 TB/s the project uses (statistics: one read of the light field; declip: one read and one write) and the ratio to it;
  - the whole denoise_clipped against denoise on that light field (README parameters, sigma given; median of `job_reps` runs each) and
    the job's overhead.
The lines are printed and written to the output file.
usage: python tools/clip_time.py [reps] [output file, default profiles/clip.txt] [batch] [job_reps]"""
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
README = ((8, 18, 6, 16, 4, "id", "sadct", "haar"), (16, 18, 6, 8, 4, "dct", "sadct", "haar"))
CONFIG5 = ((1, 18, 3, 16, 3, "bior", "sadct", "haar"), (8, 18, 3, 8, 3, "dct", "sadct", "haar"))   # BASELINE.json configs[4]
P = lambda s, pk: core.make_params(s, 2.7, *pk)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def estimate(ctx, out):
    lf = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    for sigma in (5.0, 10.0, 25.0, 50.0, 75.0):
        noisy = synth.add_noise_mt19937(lf, sigma, seed=1)
        d = torch.from_numpy(synth.clip_round(noisy)).cuda()
        e = ctx.noise_level_clipped(d, mask, 256, 256, 3)
        out({"estimate": "golden 3x3x256x256x3, MT19937 seed 1, rounded and clipped to 0..255", "sigma": sigma,
             "clipping_aware": round(e.sigma, 4), "per_channel": [round(v, 4) for v in e.sigma_channel], "levels": e.levels,
             "f_max": e.f_max, "censored_blocks": round(e.censored, 4), "heavily_clipped": e.heavily_clipped,
             "blind": round(ctx.noise_level(d, mask, 256, 256, 3).sigma, 4)})
        if sigma == 25.0:
            e = ctx.noise_level_clipped(torch.from_numpy(noisy).cuda(), mask, 256, 256, 3)
            out({"estimate": "the same, float noise (neither rounded nor clipped)", "sigma": sigma, "clipping_aware": round(e.sigma, 4),
                 "levels": e.levels, "f_max": e.f_max, "quantised": e.quantised})


def psnr_table(ctx, out):
    clean = np.ascontiguousarray(np.load(GOLDEN)[:, :, 192:256, 128:192], np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    tail = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
    psnr = lambda x: round(float(10.0 * np.log10(255.0 ** 2 / ((x.cpu().numpy().astype(np.float64) - clean) ** 2).mean())), 4)
    for sigma, (ht, wi) in ((25.0, README), (50.0, CONFIG5)):
        cl = synth.clip_round(synth.add_noise_mt19937(clean, sigma, seed=1))
        d = torch.from_numpy(cl).cuda()
        basic, den = torch.zeros_like(d), torch.zeros_like(d)
        rec = {"psnr": "golden tile rows 192..255, columns 128..191, 3x3 SAIs x 3 channels, rounded and clipped", "sigma": sigma,
               "noisy": psnr(d)}
        ctx.denoise(P(sigma, ht), P(sigma, wi), d.clone(), mask, basic, den, *tail)
        rec["denoise"] = psnr(den)
        ctx.denoise_clipped(sigma, P(sigma, ht), P(sigma, wi), d.clone(), mask, basic, den, *tail)
        rec["denoise_clipped_sigma_given"] = psnr(den)
        used, e = ctx.denoise_clipped(None, P(sigma, ht), P(sigma, wi), d.clone(), mask, basic, den, *tail)
        rec["denoise_clipped_sigma_estimated"] = psnr(den)
        rec["estimated_sigma"] = round(used, 4)
        rec["estimate_levels_f_max"] = [e.levels, e.f_max]
        out(rec)


def timings(ctx, out, reps, batch, job_reps):
    ah = aw = 17
    H = W = 512
    A = ah * aw
    sigma = 25.0
    mask = np.ones(A, np.uint32)
    clean = torch.from_numpy(synth.make_lf(ah, aw, H, W).reshape(A, -1)).cuda().float()
    g = torch.Generator(device="cuda").manual_seed(1)
    noisy = torch.clamp(torch.round(clean + sigma * torch.randn(clean.shape, generator=g, device="cuda")), 0.0, 255.0)
    del clean
    back = torch.empty_like(noisy)
    st = torch.cuda.ExternalStream(ctx.stream())
    fns = (lambda: ctx.clip_histogram(noisy, mask, W, H, 3), lambda: ctx.declip(sigma, noisy, mask, back, W, H, 3))
    for fn in fns:
        fn()                                                # warm-up (buffers, code objects)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = ([], [])
    for _ in range(reps):
        for which, fn in enumerate(fns):
            e0.record(st)
            for _ in range(batch):
                fn()                                        # returns with the stream synchronised
            e1.record(st)
            e1.synchronize()
            ms[which].append(e0.elapsed_time(e1) / batch)
    nbytes = A * 3 * H * W * 4
    rec = {"lf": f"{ah}x{aw}x{W}x{H}x3", "windows": reps, "calls_per_window": batch}
    for name, v, nb in zip(("statistics", "declip"), ms, (nbytes, 2 * nbytes)):
        fl = nb / HBM * 1e3
        rec[name] = {"ms_per_call": stats(v), "bytes": nb, "floor_ms_at_6.3TBps": round(fl, 4), "over_floor": round(float(np.median(v)) / fl, 2)}
    out(rec)
    del back
    basic, den = torch.empty_like(noisy), torch.empty_like(noisy)
    tail = (L.ROWMAJOR, aw, ah, 1, 1, W, H, 3)
    p1, p2 = P(sigma, README[0]), P(sigma, README[1])
    jobs = (lambda a: ctx.denoise(p1, p2, a, mask, basic, den, *tail), lambda a: ctx.denoise_clipped(sigma, p1, p2, a, mask, basic, den, *tail))
    jm = ([], [])
    for fn in jobs:
        fn(noisy.clone())
    for _ in range(job_reps):
        for which, fn in enumerate(jobs):
            arg = noisy.clone()                             # both work on their input in place: the copy stays outside the window
            torch.cuda.synchronize()
            e0.record(st)
            fn(arg)
            e1.record(st)
            e1.synchronize()
            jm[which].append(e0.elapsed_time(e1))
    out({"lf": rec["lf"], "job_runs": job_reps, "denoise_ms": stats(jm[0]), "denoise_clipped_ms": stats(jm[1]),
         "overhead_ms": round(float(np.median(jm[1]) - np.median(jm[0])), 3),
         "denoise_clipped_over_denoise": round(float(np.median(jm[1]) / np.median(jm[0])), 4)})


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "clip.txt")
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    job_reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    lines = []

    def out(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ctx = L.Context(0)
    estimate(ctx, out)
    psnr_table(ctx, out)
    timings(ctx, out, reps, batch, job_reps)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/clip_time.py %d <file> %d %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % (reps, batch, job_reps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
