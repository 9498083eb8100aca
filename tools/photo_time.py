#!/usr/bin/env python3
"""Measurements of the photometric equalisation (lfbm5d_photo_*) for profiles/photo.txt, one JSON line each.  Every step runs in a child
process of its own under its own time limit; the first step that fails ends the run.
  one_round     time per call of lfbm5d_photo_device at the library's defaults with max_rounds = 1 and tol = 0 (so that the round is
                not cut short): table upload, one sweep over every SAI (k_view_sweep), k_photo_stats, the histograms' download, the
                ratios and the solve on the host, k_photo_apply;
  three_rounds  the same with max_rounds = 3: three sweeps, three corrections (the second and third in place);
  apply         lfbm5d_photo_apply_device alone, out of place, with the gains of a vignette;
  consist       one call of lfbm5d_consist_device with the bad-SAI decision off (tools/consist_time.py's one_round), in the same session.
The timed light field is tools/consist_time.py's: 17x17x512x512x3, device-resident, the golden light field tiled 2 x 2 and repeated over
the SAIs.  HIP events around whole calls, warm-up first; median / min / max / std over `reps` windows.  No counter run is made here: what
bounds the kernels is not measured by this tool.
usage: python tools/photo_time.py [reps] [output file, default profiles/photo.txt]
       python tools/photo_time.py --step <name> reps     (what the parent starts)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEPS = (("one_round", 300), ("three_rounds", 300), ("apply", 300), ("consist", 300))   # step, time limit in s


def step(name, reps):
    import torch
    import lfbm5d_amd as L
    from lfbm5d_amd import synth
    import consist_time as T
    ctx = L.Context(0)
    y, mask = T.big_lf()
    rec = {"lf": f"{T.AH}x{T.AW}x{T.W}x{T.H}x3", "step": name, "windows": reps, "bytes_of_the_light_field": y.numel() * 4}
    st = torch.cuda.ExternalStream(ctx.stream())
    geo = (L.ROWMAJOR, T.AW, T.AH, T.W, T.H, 3)
    if name == "consist":
        flags = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
        rec["consist_ms"] = T.timed(lambda: ctx.consist(y, mask, *geo, flags_out=flags, fill_nonfinite=False, sai_factor=0.0), st, reps)
    elif name == "apply":
        out = torch.empty_like(y)
        gain = np.repeat(synth.vignette_gains(T.AW, T.AH, 0.6)[:, None], 3, axis=1)
        rec["apply_ms"] = T.timed(lambda: ctx.apply_gains(y, gain, chnls=3, out=out), st, reps)
    else:
        out = torch.empty_like(y)
        kw = dict(max_rounds=1 if name == "one_round" else 3, tol=0.0)
        r = ctx.equalise(y, mask, *geo, out=out, **kw)
        P = L.photo_params(**kw)
        rec.update(photo_ms=T.timed(lambda: ctx.equalise(y, mask, *geo, out=out, **kw), st, reps), sweeps=r.rounds, fitted=r.fitted,
                   untested=r.untested, unfit=r.unfit, admitted=r.admitted, skipped_range=r.skipped_range, gain_min=r.gain_min,
                   gain_max=r.gain_max, max_disparity=P.max_disparity, box_radius=P.box_radius, ang_radius=P.ang_radius, steps=P.steps)
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "photo.txt")
    recs = {}
    for name, limit in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(reps)], capture_output=True, text=True, timeout=limit)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed with exit status {r.returncode}: nothing further is started")
        recs[name] = json.loads(line[-1][7:])
        print(json.dumps(recs[name]), flush=True)
    one, three = recs["one_round"]["photo_ms"]["median"], recs["three_rounds"]["photo_ms"]["median"]
    cons, app = recs["consist"]["consist_ms"]["median"], recs["apply"]["apply_ms"]["median"]
    ratio = {"lf": recs["consist"]["lf"], "consist_one_round_ms": cons, "one_round_ms": one, "one_round_over_consist": round(one / cons, 4),
             "three_rounds_ms": three, "three_rounds_ms_per_sweep": round(three / max(1, recs["three_rounds"]["sweeps"]), 4), "apply_ms": app,
             "apply_GB_per_s": round(2 * recs["apply"]["bytes_of_the_light_field"] / (app * 1e-3) / 1e9, 1)}
    print(json.dumps(ratio), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/photo_time.py %d  (MI355X; times in ms; see the tool's docstring for what each figure is; one session)\n" % reps)
        f.write("\n".join(json.dumps(recs[n]) for n, _ in STEPS) + "\n" + json.dumps(ratio) + "\n")


if __name__ == "__main__":
    main()
