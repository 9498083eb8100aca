#!/usr/bin/env python3
"""Measurements of the clipped Poisson-Gaussian stage (lfbm5d_pgclip_*, lfbm5d_denoise_pgclip_*) for profiles/pgclip.txt, one JSON line
each.
  cpu   (no GPU) the CPU composition: the numpy maps of tests/pgclip_model.py around the oracle's two steps, next to the oracle at the
        RMS sigma and the oracle between the numpy Poisson-Gaussian transforms with their own estimate on the clipped data.  PSNR on the
        dark tile (rows 192..255, columns 128..191) and on the crop (rows and columns 0..63) of the golden light field, 3x3 SAIs x 3
        channels, README parameters, noise (a, b) of numpy's default_rng(1), rounded and clipped to 0..255.
  gpu   the same table from the GPU: noisy; denoise at the RMS sigma; denoise_pg with its own estimate; denoise_clipped (own estimate);
        denoise_pgclip with the model given and estimated.  Then times on 17x17x512x512x3, device-resident, HIP events on the context's
        stream around windows of `batch` whole calls, `reps` windows, median: pgclip_forward and pgclip_inverse (out of place) against
        pg_forward / pg_inverse (k_pg_transform) and declip (k_declip) in the same run, and against one read plus one write of the light
        field at the 6.3 TB/s the project uses; denoise_pgclip (model given) against denoise.
The lines are printed and appended to the output file.
usage: python tools/pgclip_time.py cpu|gpu [output file, default profiles/pgclip.txt] [reps] [batch] [job_reps]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lfbm5d_amd as L  # noqa: E402
from lfbm5d_amd import core, synth  # noqa: E402

HBM = 6.3e12
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
README = ((8, 18, 6, 16, 4, "id", "sadct", "haar"), (16, 18, 6, 8, 4, "dct", "sadct", "haar"))
MODELS = ((0.0, 625.0), (0.0, 2500.0), (1.0, 100.0), (4.0, 50.0))
REGIONS = {"dark tile rows 192..255, columns 128..191": (slice(192, 256), slice(128, 192)), "crop rows 0..63, columns 0..63": (slice(0, 64), slice(0, 64))}
MASK = np.ones(9, np.uint32)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def region(sl):
    return np.ascontiguousarray(np.load(GOLDEN)[:, :, sl[0], sl[1]], np.float32).reshape(9, -1)


def psnr_of(clean):
    return lambda x: round(float(10.0 * np.log10(255.0 ** 2 / ((np.asarray(x, np.float64) - clean) ** 2).mean())), 4)


def cpu(out):
    from oracle import oracle as O
    import pg_model as PG
    import pgclip_model as M

    def two_steps(x, sigma):
        n1, b, _ = O.run_step1(O.make_params(sigma, 2.7, *README[0]), x.copy(), MASK, O.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        return O.run_step2(O.make_params(sigma, 2.7, *README[1]), n1.copy(), b.copy(), MASK, O.ROWMAJOR, 3, 3, 1, 64, 64, 3)[2]

    for name, sl in REGIONS.items():
        clean = region(sl)
        psnr = psnr_of(clean)
        for a, b in MODELS:
            z = synth.clip_round(synth.add_poisson_gaussian(clean, a, b, 1))
            rec = {"cpu_composition": name, "model": [a, b], "noisy": psnr(z)}
            rms = float(np.sqrt((a * clean + b).mean()))
            rec["rms_sigma"] = round(rms, 4)
            rec["oracle_at_rms_sigma"] = psnr(two_steps(z, rms))
            e = PG.estimate(z, MASK, 64, 64, 3)
            t, s = PG.forward_lf(z, [e["a"]] * 3, [e["b"]] * 3, 3)
            rec["pg_estimate_on_clipped"] = [round(e["a"], 4), round(e["b"], 4)]
            rec["oracle_between_pg_transforms"] = psnr(PG.inverse_lf(two_steps(t.astype(np.float32), s), [e["a"]] * 3, [e["b"]] * 3, 3))
            for label, ab in (("given", (a, b)), ("estimated", None)):
                if ab is None:
                    f = M.estimate(z, MASK, 64, 64, 3)
                    ab = (f["a"], f["b"]) if f else None
                    rec["pgclip_estimate"] = [round(v, 4) for v in ab] if ab else None
                cv = M.curves(*ab) if ab else None
                if cv is None:
                    rec["pgclip_composition_model_" + label] = None
                    continue
                d = two_steps(M.forward(z, cv), float(np.float32(cv["s"])))
                rec["pgclip_composition_model_" + label] = psnr(M.inverse(d, cv))
                rec["s_" + label] = round(cv["s"], 4)
            out(rec)


def gpu(out, reps, batch, job_reps):
    import torch
    P = lambda s, pk: core.make_params(s, 2.7, *pk)
    ctx = L.Context(0)
    tail = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
    for name, sl in REGIONS.items():
        clean = region(sl)
        psnr = lambda t: psnr_of(clean)(t.cpu().numpy())
        for a, b in MODELS:
            z = synth.clip_round(synth.add_poisson_gaussian(clean, a, b, 1))
            d = torch.from_numpy(z).cuda()
            basic, den = torch.zeros_like(d), torch.zeros_like(d)
            rec = {"psnr": name, "model": [a, b], "noisy": psnr(d)}
            rms = float(np.sqrt((a * clean + b).mean()))
            ctx.denoise(P(rms, README[0]), P(rms, README[1]), d.clone(), MASK, basic, den, *tail)
            rec["denoise_at_rms_sigma"] = psnr(den)
            try:
                m = ctx.denoise_pg(None, P(1.0, README[0]), P(1.0, README[1]), d.clone(), MASK, basic, den, *tail)
                rec["denoise_pg_own_estimate"] = psnr(den)
                rec["pg_estimate_on_clipped"] = [round(m.a[0], 4), round(m.b[0], 4)]
            except L.LfBm5dError as e:
                rec["denoise_pg_own_estimate"] = str(e)
            used, _ = ctx.denoise_clipped(None, P(1.0, README[0]), P(1.0, README[1]), d.clone(), MASK, basic, den, *tail)
            rec["denoise_clipped"] = psnr(den)
            rec["clipped_sigma"] = round(used, 4)
            _, s = ctx.denoise_pgclip((a, b), P(1.0, README[0]), P(1.0, README[1]), d, MASK, basic, den, *tail)
            rec["denoise_pgclip_model_given"] = psnr(den)
            rec["s_given"] = round(s, 4)
            try:
                e, s = ctx.denoise_pgclip(None, P(1.0, README[0]), P(1.0, README[1]), d, MASK, basic, den, *tail)
                rec["denoise_pgclip_model_estimated"] = psnr(den)
                rec["pgclip_estimate"] = [round(e.a, 4), round(e.b, 4), e.levels, e.f_max]
            except L.LfBm5dError as err:
                rec["denoise_pgclip_model_estimated"] = str(err)
            out(rec)
    # ---- times ----
    ah = aw = 17
    H = W = 512
    A = ah * aw
    mask = np.ones(A, np.uint32)
    a, b = 1.0, 100.0
    clean = torch.from_numpy(synth.make_lf(ah, aw, H, W).reshape(A, -1)).cuda().float()
    g = torch.Generator(device="cuda").manual_seed(1)
    noisy = torch.clamp(torch.round(clean + torch.sqrt(a * clean + b) * torch.randn(clean.shape, generator=g, device="cuda")), 0.0, 255.0)
    del clean
    back = torch.empty_like(noisy)
    cv = L.pgclip_curves(a, b)
    pgm = core.pg_model(a, b)
    st = torch.cuda.ExternalStream(ctx.stream())
    fns = {"pgclip_forward": lambda: ctx.pgclip_forward(cv, noisy, mask, back, W, H, 3),
           "pgclip_inverse": lambda: ctx.pgclip_inverse(cv, noisy, mask, back, W, H, 3),
           "pg_forward": lambda: ctx.pg_forward(pgm, noisy, mask, back, W, H, 3),
           "pg_inverse": lambda: ctx.pg_inverse(pgm, noisy, mask, back, W, H, 3),
           "declip": lambda: ctx.declip(10.0, noisy, mask, back, W, H, 3)}
    for fn in fns.values():
        fn()                                                # warm-up (buffers, code objects)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0.record(st)
            for _ in range(batch):
                fn()                                        # returns with the stream synchronised
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / batch)
    nb = 2 * A * 3 * H * W * 4
    fl = nb / HBM * 1e3
    rec = {"lf": f"{ah}x{aw}x{W}x{H}x3", "windows": reps, "calls_per_window": batch, "bytes_read_plus_write": nb, "floor_ms_at_6.3TBps": round(fl, 4)}
    for k, v in ms.items():
        rec[k] = {"ms_per_call": stats(v), "over_floor": round(float(np.median(v)) / fl, 2)}
    out(rec)
    del back
    basic, den = torch.empty_like(noisy), torch.empty_like(noisy)
    tail = (L.ROWMAJOR, aw, ah, 1, 1, W, H, 3)
    p1, p2 = P(cv.s, README[0]), P(cv.s, README[1])
    jobs = (lambda x: ctx.denoise(p1, p2, x, mask, basic, den, *tail), lambda x: ctx.denoise_pgclip((a, b), p1, p2, x, mask, basic, den, *tail))
    jm = ([], [])
    for fn in jobs:
        fn(noisy.clone())
    for _ in range(job_reps):
        for which, fn in enumerate(jobs):
            arg = noisy.clone()                             # denoise works on its input in place: the copy stays outside the window
            torch.cuda.synchronize()
            e0.record(st)
            fn(arg)
            e1.record(st)
            e1.synchronize()
            jm[which].append(e0.elapsed_time(e1))
    out({"lf": rec["lf"], "job_runs": job_reps, "denoise_ms": stats(jm[0]), "denoise_pgclip_ms": stats(jm[1]),
         "overhead_ms": round(float(np.median(jm[1]) - np.median(jm[0])), 3),
         "denoise_pgclip_over_denoise": round(float(np.median(jm[1]) / np.median(jm[0])), 4),
         "note": "denoise_pgclip includes building the curves on the host (13 million evaluations of F in double, one core)"})
    ctx.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "gpu"
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pgclip.txt")
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    batch = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    job_reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write("# tools/pgclip_time.py %s <file> %d %d %d  (times in ms; see the tool's docstring for what each figure is)\n"
                % (mode, reps, batch, job_reps))

        def out(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if mode == "cpu":
            cpu(out)
        else:
            gpu(out, reps, batch, job_reps)


if __name__ == "__main__":
    main()
