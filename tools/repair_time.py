#!/usr/bin/env python3
"""Time of the joint repair (lfbm5d_repair_*) against the two stages it replaces, on the workload of tools/view_time.py (17x17x512x512x3,
the golden light field tiled) with the 64 x 64 map of synth.add_defects(seed = 2) tiled over every SAI (about 6 % of the values) and the
centre SAI missing, at the
library's defaults (D = 4, r = 3, ang_radius = 1):
  fill      repair_fill                            against   view_fill of the centre SAI + inpaint_fill of the flagged values
  job       repair with its K = 4 steps            against   view_synth (K = 4) followed by inpaint (K = 8): what a LFBM5D_DETECT command
                                                             pays today for a bad SAI and flagged values, "each with its own loop"
Whole calls between HIP events on the context's stream, a warm-up call first, median / min / max over `reps` windows of one call; every
measurement runs in a child process of its own under its own time limit, joint and two-stage alternating, and the first child that fails
ends the run.  The two stages are the parent commit's: tools/isa_diff.sh shows their kernels unchanged; --parent-lib <liblfbm5d_hip.so
of a parent build> makes their children load that library instead (through LFBM5D_HIP_LIB).
usage: python tools/repair_time.py [--parent-lib path] [reps] [output file, default profiles/repair.txt]
       python tools/repair_time.py --step <fill|job> <joint|two> reps     (what the parent starts)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import view_time as T      # noqa: E402

LIMIT = 300


def step(name, which, reps):
    import torch
    import lfbm5d_amd as L
    from lfbm5d_amd import core, synth
    ctx = L.Context(0)
    y, mask = T.big_lf()
    A = T.AH * T.AW
    one = np.tile(synth.add_defects((9, 3, 64, 64), 2), (1, 1, T.H // 64, T.W // 64)).reshape(9, -1)
    flags = torch.from_numpy(np.ascontiguousarray(np.tile(one, ((A + 8) // 9, 1))[:A]).astype(np.uint8)).cuda()
    missing = np.zeros(A, np.uint32)
    missing[A // 2] = 1
    out, mid = torch.empty_like(y), torch.empty_like(y)
    P = core.make_params(0.0, 2.7, *T.HT)
    geo = (L.ROWMAJOR, T.AW, T.AH, T.W, T.H, 3)
    tail = (L.ROWMAJOR, T.AW, T.AH, 1, T.W, T.H, 3)
    st = torch.cuda.ExternalStream(ctx.stream())
    rec = {"lf": f"{T.AH}x{T.AW}x{T.W}x{T.H}x3", "step": name, "form": which, "windows": reps, "flagged_share": round(float(one.mean()), 4),
           "library": "a build of the parent commit (--parent-lib)" if os.environ.get("LFBM5D_HIP_LIB") else "the tree's"}
    if name == "fill" and which == "joint":
        r = ctx.repair_fill(y, flags, missing, mask, *geo, out=out)
        fn = lambda: ctx.repair_fill(y, flags, missing, mask, *geo, out=out)
        rec.update(targets=r.targets, views=sum(r.views), rim=sum(r.rim), left=sum(r.left), min_valid=L.repair_params().min_valid)
    elif name == "fill":
        def fn():
            ctx.view_fill(y, mask, missing, *geo, out=mid)                         # writes the centre SAI alone
            ctx.inpaint_fill(y, flags, mask, T.W, T.H, 3, out=out)
    elif which == "joint":
        rec["iterations"] = L.repair_params().iterations
        fn = lambda: ctx.repair(y, flags, missing, mask, P, *tail, sigma_noise=10.0, out=out)
    else:
        rec["iterations"] = [L.view_params().iterations, L.inpaint_params().iterations]

        def fn():
            ctx.view_synth(y, mask, missing, P, *tail, sigma_noise=10.0, out=mid)
            ctx.inpaint(mid, flags, mask, P, *tail, sigma_noise=10.0, out=out)
    rec["ms"] = T.timed([fn], st, reps, 1)[0]
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--step":
        return step(argv[1], argv[2], int(argv[3]))
    parent = None
    if argv and argv[0] == "--parent-lib":
        parent, argv = os.path.abspath(argv[1]), argv[2:]
    reps = int(argv[0]) if argv else 5
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "repair.txt")
    lines = []
    for name in ("fill", "job"):
        pair = []
        for which in ("joint", "two"):
            env = dict(os.environ)
            if parent and which == "two":
                env["LFBM5D_HIP_LIB"] = parent
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, which, str(reps)], capture_output=True, text=True,
                               timeout=LIMIT, env=env)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"step {name} {which} failed with exit status {r.returncode}: nothing further is started")
            pair.append(json.loads(line[-1][7:]))
            lines.append(line[-1][7:])
            print(lines[-1], flush=True)
        a, b = pair[0]["ms"]["median"], pair[1]["ms"]["median"]
        lines.append(json.dumps({"step": name, "joint_ms": a, "two_stage_ms": b, "joint_over_two_stage": round(a / b, 3)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/repair_time.py %d <file>  (MI355X; times in ms; see the tool's docstring)\n" % reps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
