#!/usr/bin/env python3
"""Measurements of the correlated-noise feature (include/lfbm5d_corr.h) for profiles/corr.txt, on one MI355X.

  quality   synth.make_lf 3x3x96x96x3 plus synth.add_correlated_noise (Gaussian taps of width 0.8, sigma 25), dct in both steps: mean
            PSNR of the plain job at the true sigma and over a sweep of sigmas (the best single sigma is what a user could reach by
            tuning), of the job with the true autocorrelation and of the job with the blind one (corr_measure at its defaults);
  measure   time per call of lfbm5d_corr_measure_device (both kernels, the two downloads, the host's selection) against a
            device-to-device copy of the light field (one read plus one write of it);
  job       time per two-step job: the plain job (dedicated kernels), the plain job under option group_generic, the job with the true
            autocorrelation.  The last two run the same launches; the table form adds two multiplies per coefficient.
The timed light field is 17x17x512x512x3, device-resident: the golden light field tiled 2 x 2 and repeated over the SAIs, plus seeded
white noise of sigma 25.  A host clock around whole calls that end in a synchronise, warm-up first; median / min / max over `reps` calls.
No counter run is made here: what bounds the kernels is not measured by this tool.
usage: python tools/corr_time.py [reps, default 5] [output file, default profiles/corr.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
AH = AW = 17
H = W = 512
PK1 = (8, 6, 2, 8, 4, "dct", "sadct", "haar")
PK2 = (8, 6, 2, 8, 4, "dct", "sadct", "haar")


def stats(v):
    return "median %.2f ms (min %.2f, max %.2f, %d calls)" % (1e3 * np.median(v), 1e3 * np.min(v), 1e3 * np.max(v), len(v))


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return np.array(out)


def psnr(x, clean):
    x = np.clip(np.rint(x.astype(np.float64)), 0, 255)
    mse = ((x - clean.astype(np.float64)) ** 2).reshape(clean.shape[0], -1).mean(axis=1)
    return float(np.mean(10 * np.log10(255.0 ** 2 / mse)))


def main():
    import torch
    import corr_model as CM
    import lfbm5d_amd as L
    from lfbm5d_amd import core, synth
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "corr.txt")
    ctx = L.Context(0)
    taps = CM.gaussian_taps(0.8)
    acf = L.corr_from_kernel(taps)
    lines = ["# Correlated noise (include/lfbm5d_corr.h): tools/corr_time.py on one MI355X, %s." % torch.cuda.get_device_name(0),
             "# Nothing here was measured on other content, other kernels' widths or other sigmas; what is not listed is unmeasured."]

    def job(noisy, a, sigma, aw, ah, w, h, generic=False):
        P1, P2 = core.make_params(sigma, 2.7, *PK1), core.make_params(sigma, 2.7, *PK2)
        d_b, d_d = torch.zeros_like(noisy), torch.zeros_like(noisy)
        mask = np.ones(aw * ah, np.uint32)
        if generic:
            ctx.set_option("group_generic", 1)
        try:
            if a is None:
                ctx.denoise(P1, P2, noisy.clone(), mask, d_b, d_d, L.ROWMAJOR, aw, ah, 1, 1, w, h, 3)
            else:
                ctx.denoise_corr(a, P1, P2, noisy.clone(), mask, d_b, d_d, L.ROWMAJOR, aw, ah, 1, 1, w, h, 3)
        finally:
            if generic:
                ctx.set_option("group_generic", None)
        return d_d

    # ---- quality ----
    clean = synth.make_lf(3, 3, 96, 96).astype(np.float32)
    noisy = synth.add_correlated_noise(clean, 25.0, taps, seed=1).reshape(9, -1)
    cl = clean.reshape(9, -1)
    d_noisy = torch.from_numpy(noisy).cuda()
    sweep = {s: psnr(job(d_noisy, None, s, 3, 3, 96, 96).cpu().numpy(), cl) for s in (15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 50.0, 60.0, 75.0)}
    est = ctx.corr_measure(d_noisy, np.ones(9, np.uint32), 96, 96, 3)
    p_true = psnr(job(d_noisy, acf, 25.0, 3, 3, 96, 96).cpu().numpy(), cl)
    p_blind = psnr(job(d_noisy, est.acf, 25.0, 3, 3, 96, 96).cpu().numpy(), cl)
    best = max(sweep, key=sweep.get)
    lines += ["quality: synth.make_lf 3x3x96x96x3 + add_correlated_noise(width 0.8, sigma 25, seed 1), dct k 8 N 8 in both steps, mean PSNR over the SAIs",
              "  noisy %.2f dB" % psnr(noisy, cl),
              "  plain job, sigma sweep: " + ", ".join("%.0f: %.2f" % (s, p) for s, p in sweep.items()),
              "  plain job at the true sigma 25: %.2f dB; best single sigma of the sweep (%.0f): %.2f dB" % (sweep[25.0], best, sweep[best]),
              "  true autocorrelation at sigma 25: %.2f dB (%+.2f over the plain job at 25, %+.2f over its best single sigma)" % (p_true, p_true - sweep[25.0], p_true - sweep[best]),
              "  blind autocorrelation at sigma 25: %.2f dB (%+.2f, %+.2f); measured lag-1 %.3f %.3f (true %.3f), its sigma %.2f (%+.1f %%)"
              % (p_blind, p_blind - sweep[25.0], p_blind - sweep[best], est.acf[3, 4], est.acf[4, 3], acf[3, 4], est.sigma, 100 * (est.sigma / 25.0 - 1))]
    print("\n".join(lines), flush=True)

    # ---- times ----
    A = AH * AW
    g9 = torch.from_numpy(np.load(GOLDEN)).cuda().float().repeat(1, 1, 2, 2)
    big = g9.repeat((A + 8) // 9, 1, 1, 1)[:A].reshape(A, -1).contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    big = big + 25.0 * torch.randn(big.shape, device="cuda", generator=gen)
    mask = np.ones(A, np.uint32)
    other = torch.empty_like(big)
    t_copy = timed(lambda: other.copy_(big), reps)
    t_meas = timed(lambda: ctx.corr_measure(big, mask, W, H, 3), reps)
    e = ctx.corr_measure(big, mask, W, H, 3)
    lines += ["measure: 17x17x512x512x3 (%.0f MB), block 16, fraction 0.1: %d blocks, %d selected" % (big.numel() * 4 / 1e6, e.blocks, e.selected),
              "  lfbm5d_corr_measure_device: " + stats(t_meas),
              "  device-to-device copy of the light field (one read plus one write): " + stats(t_copy),
              "  ratio of the medians: %.1f" % (np.median(t_meas) / np.median(t_copy))]
    print("\n".join(lines[-4:]), flush=True)
    t_plain = timed(lambda: job(big, None, 25.0, AW, AH, W, H), reps)
    t_gen = timed(lambda: job(big, None, 25.0, AW, AH, W, H, generic=True), reps)
    t_corr = timed(lambda: job(big, acf, 25.0, AW, AH, W, H), reps)
    lines += ["job: 17x17x512x512x3, both steps (dct k 8 N 8 p 4, 3 x 3 windows), including a copy of the input and two zero-filled outputs",
              "  plain job, dedicated kernels (instruction-identical to the parent commit's: tools/isa_diff.sh): " + stats(t_plain),
              "  plain job under option group_generic: " + stats(t_gen),
              "  job with the true autocorrelation (k_group_corr): " + stats(t_corr),
              "  table form over group_generic: %.3f; over the dedicated kernels: %.2f" % (np.median(t_corr) / np.median(t_gen), np.median(t_corr) / np.median(t_plain))]
    print("\n".join(lines[-5:]), flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
