#!/usr/bin/env python3
"""What per-view noise levels (include/lfbm5d_views.h) buy and cost.  Workload: synth.make_lf, 9 x 9 SAIs of 128 x 128, colour, under
the noise a devignetted capture carries -- sigma_v = sigma / vignette_gains(edge)[v] (synth.add_view_noise, seed 1) -- at edge 0.5 and
0.3 around sigma = 10 and 25, the README's parameters.  Per case the PSNR (dB, peak 255, mean over the views) per ring of views
(Chebyshev distance from the centre view) and overall of
  (a) denoise with the true pooled (root mean square) sigma,        (b) denoise with the blind pooled estimate (noise_level),
  (c) denoise_views with the true table,                            (d) denoise_views with the estimated table (None),
then the per-SAI estimator's scatter on uniform noise (estimate / sigma over the 81 views), the job time of (c) against (a) -- host
clock around whole calls, which end in a synchronise; a warm-up pair first, then `reps` alternating pairs -- and the figures of the
quality test of tests/test_gpu_views.py (7 x 7 views of 64 x 64 cut from the golden photograph, edge 0.4 around sigma 15, the tests'
small parameters).
usage: python tools/views_time.py [reps, default 5] [output file, default profiles/views.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HT, WIEN = (8, 18, 6, 16, 4, "id", "sadct", "haar"), (16, 18, 6, 8, 4, "dct", "sadct", "haar")          # the README's
SMALL_HT, SMALL_WIEN = (4, 6, 2, 8, 4, "id", "sadct", "haar"), (8, 6, 2, 8, 4, "dct", "sadct", "haar")  # the tests'


def rings(ah, aw):
    s, t = np.mgrid[0:ah, 0:aw]
    return np.maximum(abs(s - ah // 2), abs(t - aw // 2)).reshape(-1)


def psnr_sai(x, clean):
    mse = ((x.astype(np.float64) - clean.astype(np.float64)) ** 2).mean(axis=1)
    return 10.0 * np.log10(255.0 ** 2 / mse)


class Jobs:
    def __init__(self, ctx, ah, aw, H, W, pk):
        import lfbm5d_amd as L
        from lfbm5d_amd import core
        self.L, self.core, self.ctx, self.ah, self.aw, self.H, self.W, self.pk = L, core, ctx, ah, aw, H, W, pk
        self.mask = np.ones(ah * aw, np.uint32)

    def run(self, noisy, sigma=None, table=False):
        """denoise (sigma given) or denoise_views (table: an array, or None for the estimate): (denoised, table used, seconds)."""
        import torch
        P1 = self.core.make_params(sigma or 0.0, 2.7, *self.pk[0])
        P2 = self.core.make_params(sigma or 0.0, 2.7, *self.pk[1])
        d_n = torch.from_numpy(noisy).cuda()
        d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
        torch.cuda.synchronize()
        tail = (self.L.ROWMAJOR, self.aw, self.ah, 1, 1, self.W, self.H, 3)
        t0 = time.perf_counter()
        if table is False:
            self.ctx.denoise(P1, P2, d_n, self.mask, d_b, d_d, *tail)
            used = None
        else:
            used = self.ctx.denoise_views(table, P1, P2, d_n, self.mask, d_b, d_d, *tail)
        dt = time.perf_counter() - t0
        return d_d.cpu().numpy(), used, dt

    def four(self, clean, table, seed=1):
        noisy = self.L.add_view_noise(clean, table, seed=seed)
        pooled = float(np.sqrt((table ** 2).mean()))
        blind = float(self.ctx.noise_level(noisy, self.mask, self.W, self.H, 3).sigma)
        a = psnr_sai(self.run(noisy, sigma=pooled)[0], clean)
        b = psnr_sai(self.run(noisy, sigma=blind)[0], clean)
        c = psnr_sai(self.run(noisy, table=table)[0], clean)
        dd, est, _ = self.run(noisy, table=None)
        d = psnr_sai(dd, clean)
        ring = rings(self.ah, self.aw)
        rec = {"pooled_true": round(pooled, 4), "pooled_blind": round(blind, 4), "sigma_min": round(float(table.min()), 4),
               "sigma_max": round(float(table.max()), 4), "estimate_over_true_min": round(float((est / table).min()), 4),
               "estimate_over_true_max": round(float((est / table).max()), 4), "rings": []}
        for r in range(int(ring.max()) + 1):
            q = ring == r
            rec["rings"].append({"ring": r, "sigma": [round(float(table[q].min()), 3), round(float(table[q].max()), 3)],
                                 "a": round(float(a[q].mean()), 4), "b": round(float(b[q].mean()), 4), "c": round(float(c[q].mean()), 4),
                                 "d": round(float(d[q].mean()), 4), "c_minus_a": round(float((c - a)[q].mean()), 4)})
        rec["overall"] = {"a": round(float(a.mean()), 4), "b": round(float(b.mean()), 4), "c": round(float(c.mean()), 4), "d": round(float(d.mean()), 4),
                          "c_minus_a": round(float((c - a).mean()), 4), "d_minus_b": round(float((d - b).mean()), 4)}
        return rec, noisy, pooled


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv else 5
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "views.txt")
    import torch      # (initialised ahead of the library's context, as in the other tools: the other way round torch found no device)
    import lfbm5d_amd as L
    from lfbm5d_amd import synth
    torch.cuda.init()
    ctx = L.Context(0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ah = aw = 9
    H = W = 128
    clean = np.ascontiguousarray(synth.make_lf(ah, aw, H, W).astype(np.float32)).reshape(ah * aw, -1)
    J = Jobs(ctx, ah, aw, H, W, (HT, WIEN))
    timed = None
    for sigma in (10.0, 25.0):
        for edge in (0.5, 0.3):
            table = sigma / synth.vignette_gains(aw, ah, edge)
            rec, noisy, pooled = J.four(clean, table)
            emit(dict({"lf": f"{ah}x{aw}x{H}x{W}x3 make_lf", "sigma": sigma, "edge": edge}, **rec))
            if sigma == 25.0 and edge == 0.5:
                timed = (noisy, table, pooled)
    # the per-SAI estimator on uniform noise
    for sigma in (10.0, 25.0):
        noisy = synth.add_noise_mt19937(clean, sigma, seed=1)
        est = ctx.noise_level(noisy, J.mask, W, H, 3, per_sai=True)
        r = est.sigma_sai / sigma
        emit({"estimator_on_uniform_noise": sigma, "pooled_over_sigma": round(float(est.sigma) / sigma, 4), "per_sai_over_sigma_min": round(float(r.min()), 4),
              "per_sai_over_sigma_max": round(float(r.max()), 4), "per_sai_over_sigma_std": round(float(r.std()), 4)})
    # job time: (c) against (a), alternating
    noisy, table, pooled = timed
    J.run(noisy, sigma=pooled)
    J.run(noisy, table=table)
    ta, tc = [], []
    for _ in range(reps):
        ta.append(J.run(noisy, sigma=pooled)[2] * 1e3)
        tc.append(J.run(noisy, table=table)[2] * 1e3)
    st = lambda v: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    emit({"job_ms": {"a_denoise": st(ta), "c_denoise_views": st(tc)}, "pairs": reps, "sigma": 25.0, "edge": 0.5,
          "c_over_a": round(float(np.median(tc) / np.median(ta)), 4)})
    # the quality test's workload
    src = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy"))[4]
    ah = aw = 7
    y0 = x0 = (256 - 64 - 6) // 2
    lf = np.stack([src[:, y0 + s:y0 + s + 64, x0 + t:x0 + t + 64] for s in range(ah) for t in range(aw)])
    clean = np.ascontiguousarray(lf.astype(np.float32)).reshape(ah * aw, -1)
    J = Jobs(ctx, ah, aw, 64, 64, (SMALL_HT, SMALL_WIEN))
    rec, _, _ = J.four(clean, 15.0 / synth.vignette_gains(aw, ah, 0.4))
    emit(dict({"lf": "7x7x64x64x3 golden photograph (tests/test_gpu_views.py)", "sigma": 15.0, "edge": 0.4}, **rec))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/views_time.py %d  (MI355X; PSNR in dB, times in ms; a = denoise / true pooled sigma, b = denoise / blind pooled estimate,\n"
                "# c = denoise_views / true table, d = denoise_views / estimated table; see the tool's docstring)\n" % reps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
