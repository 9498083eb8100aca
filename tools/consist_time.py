#!/usr/bin/env python3
"""Measurements of the consistency check (lfbm5d_consist_*) for profiles/consist.txt, one JSON line each.  Every step runs in a child
process of its own under its own time limit; the first step that fails ends the run.
  one_round   time per call of lfbm5d_consist_device at the library's defaults with the bad-SAI decision off (sai_factor = 0): table
              upload, one sweep over every SAI (k_view_sweep), k_consist_stats, the histograms' download, k_consist_flag, the counts;
  two_rounds  the same with one SAI replaced by uniform noise and max_rounds = 1: the decision finds a bad SAI, a second sweep runs;
  step1       one call of lfbm5d_step1_device at sigma 10 on the same light field, with the copy of its input that the step mutates.
The ratios are added by the parent.  The timed light field is 17x17x512x512x3, device-resident: the golden light field tiled 2 x 2 and
repeated over the SAIs (its angular structure is that of the 3 x 3 field repeated, which does not matter to the cost: every SAI is swept
over every hypothesis whatever it shows).  HIP events around whole calls, warm-up first; median / min / max / std over `reps` windows.
No counter run is made here: what bounds the kernels is not measured by this tool.
usage: python tools/consist_time.py [reps] [output file, default profiles/consist.txt]
       python tools/consist_time.py --step <name> reps     (what the parent starts)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STEPS = (("one_round", 300), ("two_rounds", 300), ("step1", 300))   # step, time limit in s
AH = AW = 17
H = W = 512
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "std": round(float(np.std(v)), 4)}


def big_lf():
    import torch
    A = AH * AW
    g9 = torch.from_numpy(np.load(GOLDEN)).cuda().float().repeat(1, 1, 2, 2)                      # [9][3][512][512]
    return g9.repeat((A + 8) // 9, 1, 1, 1)[:A].reshape(A, -1).contiguous(), np.ones(A, np.uint32)


def timed(fn, stream, reps):
    import torch
    fn()                                                        # warm-up (buffers, code objects)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def step(name, reps):
    import torch
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    ctx = L.Context(0)
    y, mask = big_lf()
    rec = {"lf": f"{AH}x{AW}x{W}x{H}x3", "step": name, "windows": reps, "bytes_of_the_light_field": y.numel() * 4}
    st = torch.cuda.ExternalStream(ctx.stream())
    geo = (L.ROWMAJOR, AW, AH, W, H, 3)
    if name == "step1":
        basic = torch.empty_like(y)
        tail = (L.ROWMAJOR, AW, AH, 1, W, H, 3)
        rec["step1_ms"] = timed(lambda: ctx.step1(core.make_params(10.0, 2.7, *HT), y.clone(), mask, basic, *tail), st, reps)
    else:
        flags = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
        kw = dict(sai_factor=0.0) if name == "one_round" else dict(max_rounds=1)
        if name == "two_rounds":
            y[(AH // 2) * AW + AW // 2] = torch.rand(y.shape[1], device="cuda") * 255.0
        r = ctx.consist(y, mask, *geo, flags_out=flags, fill_nonfinite=False, **kw)
        P = L.consist_params(**kw)
        rec.update(consist_ms=timed(lambda: ctx.consist(y, mask, *geo, flags_out=flags, fill_nonfinite=False, **kw), st, reps), sweeps=r.rounds,
                   bad=len(r.bad), untested=len(r.untested), tested=AH * AW - len(r.bad) - len(r.untested), flagged=sum(r.flagged),
                   max_disparity=P.max_disparity, box_radius=P.box_radius, ang_radius=P.ang_radius)
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "consist.txt")
    recs = {}
    for name, limit in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(reps)], capture_output=True, text=True, timeout=limit)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed with exit status {r.returncode}: nothing further is started")
        recs[name] = json.loads(line[-1][7:])
        print(json.dumps(recs[name]), flush=True)
    one = recs["step1"]["step1_ms"]["median"]
    ratio = {"lf": recs["step1"]["lf"], "step1_ms": one}
    for n in ("one_round", "two_rounds"):
        c = recs[n]["consist_ms"]["median"]
        ratio.update({f"{n}_ms": c, f"{n}_over_step1": round(c / one, 4), f"{n}_ms_per_sweep": round(c / max(1, recs[n]["sweeps"]), 4)})
    print(json.dumps(ratio), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/consist_time.py %d  (MI355X; times in ms; see the tool's docstring for what each figure is)\n" % reps)
        f.write("\n".join(json.dumps(recs[n]) for n, _ in STEPS) + "\n" + json.dumps(ratio) + "\n")


if __name__ == "__main__":
    main()
