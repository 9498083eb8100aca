#!/usr/bin/env python3
"""Measurements of the view synthesis (lfbm5d_view_*) for profiles/view.txt, one JSON line each.  Every step runs in a child process of
its own under its own time limit; the first step that fails ends the run.
  fill_one / fill_odd   time per call of lfbm5d_view_fill_device (source table upload, zero-fill of the histogram, kernel, download of
            the histogram, synchronise) at the library's defaults, with (a) one SAI missing (the centre) and (b) every SAI with an odd
            s or t missing (angular up-sampling 9 x 9 -> 17 x 17: 208 of 289);
  copy      a device-to-device copy of the light field (torch copy_): one read plus one write of it;
  step1     one call of lfbm5d_step1_device at sigma 10 with the copy of its input that the step mutates;
  loop_one / loop_odd   lfbm5d_view_device with K steps against K calls of lfbm5d_step1_device at the same sigmas on the completed light
            field (each with its copy).
The ratios are added by the parent.  The timed light field is 17x17x512x512x3, device-resident: the golden light field tiled 2 x 2 and
repeated over the SAIs.  HIP events around a batch of whole calls, warm-up first; median / min / max / std over `reps` windows of the
per-call time.  No counter run is made here: what bounds the kernel is not measured by this tool.
--steps Q (1, 2 or 4): only fill_one and fill_odd, with Q hypotheses per pixel of disparity (lfbm5d_view_fill_steps_device; Q = 1 calls
lfbm5d_view_fill_device, so that the tool also times a library from before the sub-pixel sweep, loaded through LFBM5D_HIP_LIB); the
records carry the number of hypotheses (2 D Q + 1) and the time per hypothesis; the file defaults to profiles/view_steps<Q>.txt.
usage: python tools/view_time.py [--steps Q] [reps] [output file, default profiles/view.txt] [batch]
       python tools/view_time.py --step <name> reps batch [Q]     (what the parent starts)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STEPS = (("fill_one", 240), ("fill_odd", 240), ("copy", 180), ("step1", 300), ("loop_one", 420), ("loop_odd", 420))   # step, time limit in s
AH = AW = 17
H = W = 512
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")
K, S0, S1 = 2, 30.0, 5.0


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def big_lf():
    import torch
    A = AH * AW
    g9 = torch.from_numpy(np.load(GOLDEN)).cuda().float().repeat(1, 1, 2, 2)                      # [9][3][512][512]
    return g9.repeat((A + 8) // 9, 1, 1, 1)[:A].reshape(A, -1).contiguous(), np.ones(A, np.uint32)


def missing_of(name):
    m = np.zeros(AH * AW, np.uint32)
    if name.endswith("one"):
        m[(AH // 2) * AW + AW // 2] = 1
    else:
        for s in range(AH):
            for t in range(AW):
                m[s * AW + t] = 1 if (s % 2 or t % 2) else 0
    return m


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


def step(name, reps, batch, q=1):
    import torch
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    ctx = L.Context(0)
    y, mask = big_lf()
    rec = {"lf": f"{AH}x{AW}x{W}x{H}x3", "step": name, "windows": reps, "calls_per_window": batch, "bytes_of_the_light_field": y.numel() * 4}
    out = torch.empty_like(y)
    tail = (L.ROWMAJOR, AW, AH, 1, W, H, 3)
    st = torch.cuda.ExternalStream(ctx.stream())
    if name == "copy":
        rec["copy_ms"] = timed([lambda: out.copy_(y)], torch.cuda.current_stream(), reps, batch)[0]
    elif name == "step1":
        basic = torch.empty_like(y)
        rec["step1_ms"] = timed([lambda: ctx.step1(core.make_params(10.0, 2.7, *HT), y.clone(), mask, basic, *tail)], st, reps, batch)[0]
    elif name.startswith("fill"):
        missing = missing_of(name)
        vp = L.view_params()
        kw = dict(disparity_steps=q) if q != 1 else {}
        r = ctx.view_fill(y, mask, missing, L.ROWMAJOR, AW, AH, W, H, 3, out=out, **kw)
        disp = torch.zeros((AH * AW, W * H), dtype=torch.int8, device="cuda")
        t = timed([lambda: ctx.view_fill(y, mask, missing, L.ROWMAJOR, AW, AH, W, H, 3, out=out, **kw),
                   lambda: ctx.view_fill(y, mask, missing, L.ROWMAJOR, AW, AH, W, H, 3, out=out, disparity_out=disp, **kw)], st, reps, batch)
        rec.update(fill_ms=t[0], fill_with_disparity_planes_ms=t[1], missing=r.missing, synthesised=r.synthesised, left=r.left,
                   max_disparity=vp.max_disparity, box_radius=vp.box_radius, ang_radius=vp.ang_radius,
                   fill_ms_per_synthesised_sai=round(t[0]["median"] / max(1, r.synthesised), 4))
        if "--steps" in sys.argv or q != 1:
            hyp = 2 * vp.max_disparity * q + 1
            rec.update(disparity_steps=q, hypotheses=hyp, fill_ms_per_hypothesis=round(t[0]["median"] / hyp, 4),
                       library=os.environ.get("LFBM5D_HIP_LIB") or "the tree's")
    else:
        missing = missing_of(name)
        P = core.make_params(0.0, 2.7, *HT)
        x0 = ctx.view_fill(y, mask, missing, L.ROWMAJOR, AW, AH, W, H, 3).out
        basic = torch.empty_like(y)
        sig = [S0 * (S1 / S0) ** (k / (K - 1)) for k in range(K)]

        def steps():
            for s in sig:
                ctx.step1(core.make_params(s, 2.7, *HT), x0.clone(), mask, basic, *tail)

        t = timed([lambda: ctx.view_synth(y, mask, missing, P, *tail, iterations=K, sigma_start=S0, sigma_end=S1, out=out), steps], st, reps, batch)
        rec.update(iterations=K, sigma=[S0, S1], loop_ms=t[0], k_steps_ms=t[1], loop_over_k_steps=round(t[0]["median"] / t[1]["median"], 4))
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def sweep_steps(q, rest):
    """--steps Q: fill_one and fill_odd at Q hypotheses per pixel, each in a child of its own; the first that fails ends the run."""
    if q not in (1, 2, 4):
        sys.exit("--steps takes 1, 2 or 4")
    reps = int(rest[0]) if rest else 5
    path = rest[1] if len(rest) > 1 else os.path.join(ROOT, "profiles", f"view_steps{q}.txt")
    batch = int(rest[2]) if len(rest) > 2 else 3
    lines = []
    for name, limit in STEPS[:2]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(reps), str(batch), str(q), "--steps"],
                           capture_output=True, text=True, timeout=limit)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed with exit status {r.returncode}: nothing further is started")
        lines.append(line[-1][7:])
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/view_time.py --steps %d %d <file> %d  (MI355X; times in ms; see the tool's docstring)\n" % (q, reps, batch))
        f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else 1)
    if len(sys.argv) > 1 and sys.argv[1] == "--steps":
        return sweep_steps(int(sys.argv[2]), sys.argv[3:])
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "view.txt")
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    recs = {}
    for name, limit in STEPS:
        b = 1 if name.startswith("loop") or name == "step1" else batch
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(reps), str(b)], capture_output=True, text=True,
                           timeout=limit)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed with exit status {r.returncode}: nothing further is started")
        recs[name] = json.loads(line[-1][7:])
        print(json.dumps(recs[name]), flush=True)
    floor, one = recs["copy"]["copy_ms"]["median"], recs["step1"]["step1_ms"]["median"]
    ratio = {"lf": recs["copy"]["lf"], "copy_ms": floor, "step1_ms": one}
    for n in ("one", "odd"):
        f = recs["fill_" + n]["fill_ms"]["median"]
        ratio.update({f"fill_{n}_over_copy": round(f / floor, 2), f"fill_{n}_over_step1": round(f / one, 4),
                      f"loop_{n}_over_k_steps": recs["loop_" + n]["loop_over_k_steps"]})
    print(json.dumps(ratio), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/view_time.py %d <file> %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % (reps, batch))
        f.write("\n".join(json.dumps(recs[n]) for n, _ in STEPS) + "\n" + json.dumps(ratio) + "\n")


if __name__ == "__main__":
    main()
