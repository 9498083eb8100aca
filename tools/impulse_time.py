#!/usr/bin/env python3
"""Measurements of the impulse repair (lfbm5d_impulse_*) for profiles/impulse.txt, one JSON line each.  Every step runs in a child
process of its own under its own time limit; the first step that fails ends the run.
  stats     time per call of lfbm5d_impulse_histogram_device (SAI list upload, zero-fill, kernel, download of the counts, synchronise);
  repair    time per call of lfbm5d_impulse_repair_device: the whole call (statistics, quantile, repair kernel, counts), the call with
            every threshold given (no statistics pass), and the whole call with a flag plane written;
  copy      a device-to-device copy of the same bytes (torch copy_): the floor for one read plus one write of the light field;
            the ratios of stats and repair to it are added by the parent;
  endtoend  the figures of tests/test_gpu_impulse.py::test_repair_ahead_of_the_blind_sigma_and_the_filter: 3x3x64x64 golden crop,
            sigma = 10, 0.5 % salt and pepper; blind sigma + denoise on the damaged light field (A) and behind the repair (B).
The timed light field is 17x17x512x512x3, device-resident: the golden light field tiled 2 x 2 and repeated over the SAIs, Gaussian noise
of sigma 10 and 0.5 % salt and pepper drawn on the GPU (seed 1).  HIP events around a batch of whole calls, warm-up first; median / min
/ max / std over `reps` windows of the per-call time.
usage: python tools/impulse_time.py [reps] [output file, default profiles/impulse.txt] [batch]
       python tools/impulse_time.py --step stats|repair|copy|endtoend reps batch     (what the parent starts)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STEPS = (("stats", 240), ("repair", 240), ("copy", 180), ("endtoend", 240))     # step, time limit in seconds
AH = AW = 17
H = W = 512


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def big_lf():
    import torch
    A = AH * AW
    g9 = torch.from_numpy(np.load(GOLDEN)).cuda().float().repeat(1, 1, 2, 2)                      # [9][3][512][512]
    lf = g9.repeat((A + 8) // 9, 1, 1, 1)[:A].reshape(A, -1).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(1)
    lf += 10.0 * torch.randn(lf.shape, generator=gen, device="cuda")
    hit = torch.rand(lf.shape, generator=gen, device="cuda") < 0.005
    val = torch.where(torch.rand(lf.shape, generator=gen, device="cuda") < 0.5, 0.0, 255.0)
    return torch.where(hit, val, lf).contiguous(), np.ones(A, np.uint32)


def timed(fns, stream, reps, batch):
    import torch
    for fn in fns:
        fn()                                                    # warm-up (buffers, code objects)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = [[] for _ in fns]
    for _ in range(reps):
        for which, fn in enumerate(fns):
            e0.record(stream)
            for _ in range(batch):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms[which].append(e0.elapsed_time(e1) / batch)
    return [stats(v) for v in ms]


def step(name, reps, batch):
    import torch
    import lfbm5d_amd as L
    from lfbm5d_amd import core, synth
    ctx = L.Context(0)
    lfname = f"{AH}x{AW}x{W}x{H}x3"
    if name == "endtoend":
        clean = np.ascontiguousarray(np.load(GOLDEN)[:, :, :64, :64], np.float32).reshape(9, -1)
        mask = np.ones(9, np.uint32)
        z = (clean + np.random.default_rng(7).normal(0.0, 10.0, clean.shape)).astype(np.float32)
        damaged, hit = synth.add_impulse(z, 0.005, seed=7)
        P1 = lambda s: core.make_params(s, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")
        P2 = lambda s: core.make_params(s, 2.7, 16, 18, 6, 8, 4, "dct", "sadct", "haar")
        psnr = lambda x: float(10.0 * np.log10(255.0 ** 2 / ((x.cpu().numpy().astype(np.float64) - clean) ** 2).mean()))

        def run(noisy):
            s = ctx.noise_level(noisy, mask, 64, 64, 3).sigma
            basic, den = torch.zeros_like(noisy), torch.zeros_like(noisy)
            ctx.denoise(P1(s), P2(s), noisy.clone(), mask, basic, den, L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
            return s, psnr(den)

        s0, p0 = run(torch.from_numpy(z).cuda())
        sA, pA = run(torch.from_numpy(damaged).cuda())
        rep = ctx.impulse_repair(torch.from_numpy(damaged).cuda(), mask, 64, 64, 3)
        sB, pB = run(rep.out)
        rec = {"endtoend": "golden crop 3x3x64x64x3, sigma 10 (default_rng(7)), 0.5 % salt and pepper (add_impulse seed 7), README parameters",
               "sigma_undamaged": round(s0, 4), "psnr_undamaged": round(p0, 4), "sigma_A_damaged": round(sA, 4), "psnr_A_damaged": round(pA, 4),
               "sigma_B_repaired": round(sB, 4), "psnr_B_repaired": round(pB, 4), "gain_dB": round(pB - pA, 4), "hits": int(hit.sum()),
               "flagged": int(sum(rep.flagged)), "left": int(sum(rep.left)), "thresholds": [round(t, 4) for t in rep.threshold]}
    else:
        noisy, mask = big_lf()
        nbytes = noisy.numel() * 4
        rec = {"lf": lfname, "step": name, "windows": reps, "calls_per_window": batch, "bytes_of_the_light_field": nbytes}
        if name == "copy":
            out = torch.empty_like(noisy)
            rec["copy_ms"] = timed([lambda: out.copy_(noisy)], torch.cuda.current_stream(), reps, batch)[0]
        elif name == "stats":
            st = torch.cuda.ExternalStream(ctx.stream())
            rec["statistics_ms"] = timed([lambda: ctx.impulse_histogram(noisy, mask, W, H, 3)], st, reps, batch)[0]
        else:
            st = torch.cuda.ExternalStream(ctx.stream())
            out = torch.empty_like(noisy)
            fl = torch.zeros(noisy.shape, dtype=torch.uint8, device="cuda")
            r = ctx.impulse_repair(noisy, mask, W, H, 3, out=out)
            T = list(r.threshold)
            t = timed([lambda: ctx.impulse_repair(noisy, mask, W, H, 3, out=out),
                       lambda: ctx.impulse_repair(noisy, mask, W, H, 3, out=out, threshold=T),
                       lambda: ctx.impulse_repair(noisy, mask, W, H, 3, out=out, flags_out=fl)], st, reps, batch)
            rec.update(repair_ms=t[0], repair_thresholds_given_ms=t[1], repair_with_flag_plane_ms=t[2], thresholds=[round(x, 4) for x in T],
                       flagged_share=round(sum(r.flagged) / r.pixels, 6), left=int(sum(r.left)))
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "impulse.txt")
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    recs = {}
    for name, limit in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(reps), str(batch)], capture_output=True, text=True,
                           timeout=limit)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed with exit status {r.returncode}: nothing further is started")
        recs[name] = json.loads(line[-1][7:])
        print(json.dumps(recs[name]), flush=True)
    floor = recs["copy"]["copy_ms"]["median"]
    ratio = {"lf": recs["copy"]["lf"], "floor": "device-to-device copy of the light field (one read + one write)", "copy_ms": floor,
             "statistics_over_copy": round(recs["stats"]["statistics_ms"]["median"] / floor, 2),
             "repair_over_copy": round(recs["repair"]["repair_ms"]["median"] / floor, 2),
             "repair_thresholds_given_over_copy": round(recs["repair"]["repair_thresholds_given_ms"]["median"] / floor, 2)}
    print(json.dumps(ratio), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/impulse_time.py %d <file> %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % (reps, batch))
        f.write("\n".join(json.dumps(recs[n]) for n, _ in STEPS) + "\n" + json.dumps(ratio) + "\n")


if __name__ == "__main__":
    main()
