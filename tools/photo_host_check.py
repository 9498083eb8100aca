#!/usr/bin/env python3
"""Host check of the photometric equalisation's kernels ahead of any GPU run: builds tools/photo_host_check.cpp (the per-thread code of
k_photo_stats and k_photo_apply, lfbm5d_amd/csrc/lfbm5d_photo_device.h, compiled for the host) with the address and undefined-behaviour
sanitizers, feeds it every case of tests/photo_cases.py at (D, r) = (0, 0), (3, 3) with the first sweep's prediction from the numpy model
(the sweep kernels themselves are unchanged and have their own records, profiles/view_parity.txt and profiles/subpel_parity.txt), and
compares the histograms, the two skip counters and the corrected light field (out of place, in place, and into a buffer 4 bytes off
the input's alignment) with the model bit for bit.  Needs no GPU.  Writes profiles/photo_parity.txt.

    python tools/photo_host_check.py [--cxx clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import photo_cases as K     # noqa: E402
import photo_model as M     # noqa: E402
import view_model as V      # noqa: E402

TAB = 2 + 3 * 24
BLOCKS = 3                   # workgroups per plane of the apply grid: more than one, and fewer than the larger planes would get


def run_case(exe, tmp, c, D, r):
    A, C, H, W = c["aw"] * c["ah"], c["C"], c["H"], c["W"]
    p = c["params"]
    x = c["lf"].reshape(A, C, H, W)
    tested, untested, sources, hist, nonfinite, outside, mus = M.sweep(x, c["mask"], c["ang_major"], c["aw"], c["ah"], D, r, p["ang_radius"],
                                                                        p["steps"], p["min_sources"], p["lo"], p["hi"])
    table = np.zeros((len(tested), TAB), np.int32)
    pred = np.zeros((A, C, H, W), np.float32)
    for i, m in enumerate(tested):
        missing = np.zeros(A, np.uint32)
        missing[m] = 1
        srcs = V.sources(m, c["mask"], missing, c["ang_major"], c["aw"], c["ah"], p["ang_radius"])
        table[i, 0], table[i, 1] = m, len(srcs)
        table[i, 2:2 + 3 * len(srcs)] = np.array(srcs, np.int32).reshape(-1)
        pred[m] = mus[m]
    gain = np.ones((A, 3), np.float64)
    gain[:, :C] = np.random.default_rng(A * 1000 + W).uniform(0.5, 1.5, (A, C))
    live = [m for m in range(A) if c["mask"][m]]
    planes = np.array([m * C + ch for m in live for ch in range(C)], np.int32)
    factors = np.array([M.factor(gain[m, ch]) for m in live for ch in range(C)], np.float32)
    case, out = os.path.join(tmp, "case"), os.path.join(tmp, "out")
    with open(case, "wb") as f:
        f.write(np.array([A, C, H, W, len(tested), len(planes), BLOCKS], np.int32).tobytes())
        f.write(np.array([p["lo"], p["hi"]], np.float32).tobytes())
        f.write(np.ascontiguousarray(x).tobytes())
        f.write(pred.tobytes())
        f.write(table.tobytes())
        f.write(planes.tobytes())
        f.write(factors.tobytes())
    run = subprocess.run([exe, case, out], capture_output=True, text=True)
    if run.returncode:
        print(run.stderr[-3000:])
        return None, len(tested), int(hist.sum()), nonfinite, outside
    raw = np.fromfile(out, np.uint8)
    nh, nv = A * C * M.KEYS * 8, A * C * H * W * 4
    got_hist = raw[:nh].view(np.uint64).reshape(A, C, M.KEYS)
    got_skip = [int(v) for v in raw[nh:nh + 16].view(np.uint64)]
    applied = [raw[nh + 16 + i * nv:nh + 16 + (i + 1) * nv].view(np.uint32).reshape(A, -1) for i in range(3)]
    want = M.apply_gains(c["lf"], c["mask"], gain, C)
    empty = [m for m in range(A) if not c["mask"][m]]
    ok = np.array_equal(got_hist, hist) and got_skip == [nonfinite, outside]
    ok = ok and all(np.array_equal(a[live], want.view(np.uint32)[live]) for a in applied)
    ok = ok and not applied[0][empty].any() and not applied[2][empty].any() and np.array_equal(applied[1][empty], c["lf"].view(np.uint32)[empty])
    return ok, len(tested), int(hist.sum()), nonfinite, outside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "clang++"))
    args = ap.parse_args()
    lines = ["# Photometric equalisation (lfbm5d_photo_*): the per-thread code of k_photo_stats and k_photo_apply compiled for the host",
             "# (tools/photo_host_check.cpp: workgroups of 256 threads, the counters zeroed and flushed per workgroup; address and",
             "# undefined-behaviour sanitizers on) against tests/photo_model.py on the cases of tests/photo_cases.py; the first sweep's",
             "# prediction from the model.  Compared: histograms [SAI][C][1026], the two skip counters, the corrected light field written",
             "# out of place, in place and into a buffer 4 bytes off the input's alignment.",
             "# case, D, r: tested SAIs, values admitted, not finite, out of range, result"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "photo_host_check")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               os.path.join(ROOT, "tools", "photo_host_check.cpp"), "-o", exe]
        subprocess.run(cmd, check=True)
        lines.append("# built with: " + " ".join(os.path.basename(w) if os.sep in w else w for w in cmd[:-2]))
        for name in K.NAMES:
            for D, r in K.DRS:
                ok, nt, admitted, nonfinite, outside = run_case(exe, tmp, K.case(name), D, r)
                bad += not ok
                line = (f"{name}, D = {D}, r = {r}: {nt} tested, {admitted} admitted, {nonfinite} not finite, {outside} out of range: "
                        + ("bit-identical, no sanitizer report" if ok else "SANITIZER REPORT" if ok is None else "MISMATCH"))
                print(line)
                lines.append(line)
    lines.append(f"{'all cases bit-identical to the model, no access out of bounds' if not bad else str(bad) + ' cases failed'}")
    with open(os.path.join(ROOT, "profiles", "photo_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
