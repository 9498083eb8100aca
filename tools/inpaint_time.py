#!/usr/bin/env python3
"""Measurements of the defect inpainting (lfbm5d_inpaint_*) for profiles/inpaint.txt, one JSON line each.  Every step runs in a child
process of its own under its own time limit; the first step that fails ends the run.
  fill      time per call of lfbm5d_inpaint_fill_device (SAI list upload, zero-fill of the counters, kernel, download of the counts,
            synchronise), without and with a caller's flag plane, and on a light field without one defect (every tile a copy);
  project   time per call of lfbm5d_inpaint_project_device;
  copy      a device-to-device copy of the light field (torch copy_): the floor for one read plus one write of it; the ratios of
            the fill and the projection to it are added by the parent;
  loop      lfbm5d_inpaint_device with K steps against K calls of lfbm5d_step1_device at the same sigmas on the filled light field
            (each with the copy of its input that the step mutates).
The timed light field is 17x17x512x512x3, device-resident: the golden light field tiled 2 x 2 and repeated over the SAIs, the defect map
of synth.add_defects((9, 3, 64, 64), 3) tiled 8 x 8 and repeated likewise, the flagged values set to 0.  HIP events around a batch of whole
calls, warm-up first; median / min / max / std over `reps` windows of the per-call time.
usage: python tools/inpaint_time.py [reps] [output file, default profiles/inpaint.txt] [batch]
       python tools/inpaint_time.py --step fill|project|copy|loop reps batch     (what the parent starts)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STEPS = (("fill", 240), ("project", 180), ("copy", 180), ("loop", 420))     # step, time limit in seconds
AH = AW = 17
H = W = 512
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")
K, S0, S1 = 4, 30.0, 5.0


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def big_lf():
    import torch
    from lfbm5d_amd import synth
    A = AH * AW
    g9 = torch.from_numpy(np.load(GOLDEN)).cuda().float().repeat(1, 1, 2, 2)                      # [9][3][512][512]
    lf = g9.repeat((A + 8) // 9, 1, 1, 1)[:A].reshape(A, -1).contiguous()
    f9 = torch.from_numpy(synth.add_defects((9, 3, 64, 64), 3)).cuda().repeat(1, 1, 8, 8)
    fl = f9.repeat((A + 8) // 9, 1, 1, 1)[:A].reshape(A, -1).to(torch.uint8).contiguous()
    return torch.where(fl != 0, 0.0, lf).contiguous(), fl, np.ones(A, np.uint32)


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
    from lfbm5d_amd import core
    ctx = L.Context(0)
    y, fl, mask = big_lf()
    rec = {"lf": f"{AH}x{AW}x{W}x{H}x3", "step": name, "windows": reps, "calls_per_window": batch, "bytes_of_the_light_field": y.numel() * 4}
    out = torch.empty_like(y)
    if name == "copy":
        rec["copy_ms"] = timed([lambda: out.copy_(y)], torch.cuda.current_stream(), reps, batch)[0]
    elif name == "fill":
        st = torch.cuda.ExternalStream(ctx.stream())
        codes = torch.zeros_like(fl)
        none = torch.zeros_like(fl)
        r = ctx.inpaint_fill(y, fl, mask, W, H, 3, out=out)
        t = timed([lambda: ctx.inpaint_fill(y, fl, mask, W, H, 3, out=out),
                   lambda: ctx.inpaint_fill(y, fl, mask, W, H, 3, out=out, flags_out=codes),
                   lambda: ctx.inpaint_fill(y, none, mask, W, H, 3, out=out)], st, reps, batch)
        rec.update(fill_ms=t[0], fill_with_flag_plane_ms=t[1], fill_nothing_flagged_ms=t[2], flagged_share=round(sum(r.flagged) / r.pixels, 6),
                   passes=r.passes, launches=r.launches, left=int(sum(r.left)))
    elif name == "project":
        st = torch.cuda.ExternalStream(ctx.stream())
        x = torch.full_like(y, 7.0)
        rec["project_ms"] = timed([lambda: ctx.inpaint_project(fl, x, y, mask, out, W, H, 3)], st, reps, batch)[0]
    else:
        st = torch.cuda.ExternalStream(ctx.stream())
        P = core.make_params(0.0, 2.7, *HT)
        tail = (L.ROWMAJOR, AW, AH, 1, W, H, 3)
        x0 = ctx.inpaint_fill(y, fl, mask, W, H, 3).out
        basic = torch.empty_like(y)
        sig = [S0 * (S1 / S0) ** (k / (K - 1)) for k in range(K)]

        def steps():
            for s in sig:
                ctx.step1(core.make_params(s, 2.7, *HT), x0.clone(), mask, basic, *tail)

        t = timed([lambda: ctx.inpaint(y, fl, mask, P, *tail, iterations=K, sigma_start=S0, sigma_end=S1, out=out), steps], st, reps, batch)
        rec.update(iterations=K, sigma=[S0, S1], loop_ms=t[0], k_steps_ms=t[1], loop_over_k_steps=round(t[0]["median"] / t[1]["median"], 4))
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "inpaint.txt")
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    recs = {}
    for name, limit in STEPS:
        b = 1 if name == "loop" else batch
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(reps), str(b)], capture_output=True, text=True,
                           timeout=limit)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed with exit status {r.returncode}: nothing further is started")
        recs[name] = json.loads(line[-1][7:])
        print(json.dumps(recs[name]), flush=True)
    floor = recs["copy"]["copy_ms"]["median"]
    ratio = {"lf": recs["copy"]["lf"], "floor": "device-to-device copy of the light field (one read + one write)", "copy_ms": floor,
             "fill_over_copy": round(recs["fill"]["fill_ms"]["median"] / floor, 2),
             "fill_nothing_flagged_over_copy": round(recs["fill"]["fill_nothing_flagged_ms"]["median"] / floor, 2),
             "project_over_copy": round(recs["project"]["project_ms"]["median"] / floor, 2),
             "loop_over_k_steps": recs["loop"]["loop_over_k_steps"]}
    print(json.dumps(ratio), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/inpaint_time.py %d <file> %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % (reps, batch))
        f.write("\n".join(json.dumps(recs[n]) for n, _ in STEPS) + "\n" + json.dumps(ratio) + "\n")


if __name__ == "__main__":
    main()
