#!/usr/bin/env python3
"""Time of the occlusion-aware plane sweep (lfbm5d_view_fill_occl_device) against the plain sweep at the same (Q, D, r), on the workload
of tools/view_time.py (17x17x512x512x3, the golden light field tiled, the library's D = 4, r = 3, ang_radius = 1): one SAI missing
(the centre, n = 8) and every SAI with an odd s or t missing (208 of 289, n = 2 or 4), at Q = 1 and 2.  Whole calls of view_fill between
HIP events on the context's stream, a warm-up call first, median / min / max over `reps` windows of `batch` calls; every measurement
runs in a child process of its own under its own time limit, plain and occlusion-aware alternating, and the first child that fails ends
the run.  A call holds the table upload, the counters' zero-fill and download and a synchronise besides the kernel.
The plain sweep is the parent commit's: tools/isa_diff.sh shows its kernels unchanged; --parent-lib <liblfbm5d_hip.so of a parent
build> makes the plain children load that library instead (through LFBM5D_HIP_LIB).
usage: python tools/occl_time.py [--parent-lib path] [reps] [output file, default profiles/occl_time.txt] [batch]
       python tools/occl_time.py --step <fill_one|fill_odd> <Q> <ratio> reps batch     (what the parent starts)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import view_time as T      # noqa: E402

LIMIT = 240


def step(name, q, ratio, reps, batch):
    import torch
    import lfbm5d_amd as L
    ctx = L.Context(0)
    y, mask = T.big_lf()
    missing = T.missing_of(name)
    out = torch.empty_like(y)
    vp = L.view_params()
    kw = {}
    if q != 1:
        kw["disparity_steps"] = q
    if ratio:
        kw["occlusion"] = ratio
    st = torch.cuda.ExternalStream(ctx.stream())
    r = ctx.view_fill(y, mask, missing, L.ROWMAJOR, T.AW, T.AH, T.W, T.H, 3, out=out, **kw)
    t = T.timed([lambda: ctx.view_fill(y, mask, missing, L.ROWMAJOR, T.AW, T.AH, T.W, T.H, 3, out=out, **kw)], st, reps, batch)[0]
    hyp = 2 * vp.max_disparity * q + 1
    rec = {"lf": f"{T.AH}x{T.AW}x{T.W}x{T.H}x3", "step": name, "disparity_steps": q, "occl_ratio": ratio, "hypotheses": hyp,
           "windows": reps, "calls_per_window": batch, "fill_ms": t, "fill_ms_per_hypothesis": round(t["median"] / hyp, 4),
           "synthesised": r.synthesised, "max_disparity": vp.max_disparity, "box_radius": vp.box_radius,
           "set_hist": None if r.set_hist is None else list(r.set_hist), "library": "a build of the parent commit (--parent-lib)" if os.environ.get("LFBM5D_HIP_LIB") else "the tree's"}
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--step":
        return step(argv[1], int(argv[2]), float(argv[3]), int(argv[4]), int(argv[5]))
    parent = None
    if argv and argv[0] == "--parent-lib":
        parent, argv = os.path.abspath(argv[1]), argv[2:]
    reps = int(argv[0]) if argv else 5
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "occl_time.txt")
    batch = int(argv[2]) if len(argv) > 2 else 5
    import lfbm5d_amd as L
    default = L.view_occl_default()
    lines = []
    for name in ("fill_one", "fill_odd"):
        for q in (1, 2):
            pair = []
            for ratio in (0.0, default):
                env = dict(os.environ)
                if parent and not ratio:
                    env["LFBM5D_HIP_LIB"] = parent
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(q), str(ratio), str(reps), str(batch)],
                                   capture_output=True, text=True, timeout=LIMIT, env=env)
                line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit(f"step {name} Q={q} ratio={ratio} failed with exit status {r.returncode}: nothing further is started")
                pair.append(json.loads(line[-1][7:]))
                lines.append(line[-1][7:])
                print(lines[-1], flush=True)
            a, b = pair[0]["fill_ms"]["median"], pair[1]["fill_ms"]["median"]
            lines.append(json.dumps({"step": name, "disparity_steps": q, "plain_ms": a, "occl_ms": b, "occl_over_plain_per_call": round(b / a, 3),
                                     "occl_over_plain_per_hypothesis": round(b / a, 3)}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# tools/occl_time.py %d <file> %d  (MI355X; times in ms; see the tool's docstring)\n" % (reps, batch))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
