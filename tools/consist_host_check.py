#!/usr/bin/env python3
"""Host check of the consistency check's kernels ahead of any GPU run: builds tools/consist_host_check.cpp (the per-thread code of
k_consist_stats and k_consist_flag, lfbm5d_amd/csrc/lfbm5d_consist_device.h, compiled for the host) with the address and
undefined-behaviour sanitizers, feeds it every case of tests/consist_cases.py at (D, r) = (0, 0), (3, 3), (8, 7) with the prediction and
d* of the numpy model (k_view_sweep itself is unchanged and has its own record, profiles/view_parity.txt), and compares histograms,
skipped counts, flag planes and counts with the model bit for bit.  Needs no GPU.  Writes profiles/consist_parity.txt.

    python tools/consist_host_check.py [--cxx clang++]
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

import consist_cases as K     # noqa: E402
import consist_model as M     # noqa: E402

TAB = 2 + 3 * 24


def write_case(path, c, res):
    A, C, H, W = c["aw"] * c["ah"], c["C"], c["H"], c["W"]
    table = np.zeros((len(res["tested"]), TAB), np.int32)
    for i, m in enumerate(res["tested"]):
        srcs = res["sources"][m]
        table[i, 0], table[i, 1] = m, len(srcs)
        table[i, 2:2 + 3 * len(srcs)] = np.array(srcs, np.int32).reshape(-1)
    g = np.float32(float(c["params"]["spread"]) ** 2)
    with open(path, "wb") as f:
        f.write(np.array([A, C, H, W, len(res["tested"])], np.int32).tobytes())
        f.write(np.array(list(res["threshold"]) + [g], np.float32).tobytes())
        f.write(np.ascontiguousarray(c["lf"], np.float32).tobytes())
        f.write(np.ascontiguousarray(res["mu"], np.float32).tobytes())
        disp = np.where(res["disp"] == K.DISP_SENTINEL, 0, res["disp"]).astype(np.int8)
        f.write(disp.tobytes())
        f.write(table.tobytes())


def compare(path, c, res):
    A, C, H, W = c["aw"] * c["ah"], c["C"], c["H"], c["W"]
    raw = np.fromfile(path, np.uint8)
    nh, nv = A * C * M.Q * 8, A * C * H * W
    hist = raw[:nh].view(np.uint64).reshape(A, C, M.Q)
    skipped = int(raw[nh:nh + 8].view(np.uint64)[0])
    flags = raw[nh + 8:nh + 8 + nv].reshape(A, -1)
    counts = raw[nh + 8 + nv:].view(np.uint64).reshape(A, 3, 2).sum(axis=0).astype(np.int64)
    want = np.where(res["flags"] == K.FLAG_SENTINEL, 0, res["flags"])
    tested = res["tested"]
    ok = (np.array_equal(hist, res["hist"]) and skipped == res["skipped"] and np.array_equal(flags[tested], want[tested])
          and not flags[[m for m in range(A) if m not in tested]].any() and np.array_equal(counts, res["counts"]))
    return ok, int(counts[:, 0].sum()), int(counts[:, 1].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "clang++"))
    args = ap.parse_args()
    lines = ["# Consistency check (lfbm5d_consist_*): the per-thread code of k_consist_stats and k_consist_flag compiled for the host",
             "# (tools/consist_host_check.cpp: workgroups of 256 threads, the counters zeroed and flushed per workgroup; address and",
             "# undefined-behaviour sanitizers on) against tests/consist_model.py on the cases of tests/consist_cases.py; prediction and d*",
             "# from the model.  Compared: histograms [SAI][C][386], skipped, flag planes, counts per channel and code.",
             "# case, D, r: tested SAIs, sweeps, bad SAIs, values with code 1, with code 2, result"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "consist_host_check")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               os.path.join(ROOT, "tools", "consist_host_check.cpp"), "-o", exe]
        subprocess.run(cmd, check=True)
        lines.append("# built with: " + " ".join(os.path.basename(w) if os.sep in w else w for w in cmd[:-2]))
        for name in K.NAMES:
            for D, r in K.DRS:
                c, res = K.case(name), K.model(name, D, r)
                write_case(os.path.join(tmp, "case"), c, res)
                run = subprocess.run([exe, os.path.join(tmp, "case"), os.path.join(tmp, "out")], capture_output=True, text=True)
                if run.returncode:
                    ok, n1, n2 = False, -1, -1
                    print(run.stderr[-3000:])
                else:
                    ok, n1, n2 = compare(os.path.join(tmp, "out"), c, res)
                bad += not ok
                line = (f"{name}, D = {D}, r = {r}: {len(res['tested'])} tested, {res['rounds']} sweeps, bad {res['bad']}, {n1} code 1, {n2} code 2: "
                        + ("bit-identical, no sanitizer report" if ok else "MISMATCH" if not run.returncode else "SANITIZER REPORT"))
                print(line)
                lines.append(line)
    lines.append(f"{'all cases bit-identical to the model, no access out of bounds' if not bad else str(bad) + ' cases failed'}")
    with open(os.path.join(ROOT, "profiles", "consist_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
