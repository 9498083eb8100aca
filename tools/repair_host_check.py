#!/usr/bin/env python3
"""Host check of the joint repair's kernels ahead of any GPU run: builds tools/repair_host_check.cpp (the per-thread code of
k_repair_valid and k_repair_sweep, lfbm5d_amd/csrc/lfbm5d_repair_device.h, compiled for the host) with the address and
undefined-behaviour sanitizers, feeds it every case of tests/repair_cases.py at (D, r) = (0, 0), (3, 3) and min_valid = 1, 3, and
compares the validity planes, the light field and the flags after the sweep, the disparities, the unsound positions per tile and the
histogram with the numpy model bit for bit.  Needs no GPU.  Writes profiles/repair_parity.txt.

    python tools/repair_host_check.py [--cxx clang++]
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

import repair_cases as K    # noqa: E402
import repair_model as M    # noqa: E402

TAB, SRC, TW, TH = 2 + 3 * 24, 24, 64, 32


def float_tables(r):
    g = np.zeros(226, np.float32)
    g[:(2 * r + 1) ** 2 + 1] = M.g_table(r)
    return np.concatenate([M.RECIP, M.F.reshape(-1), g]).astype(np.float32)


def run_case(exe, tmp, name, D, r, mv):
    c, want = K.case(name), K.model(name, D, r, mv)
    A, C, H, W = c["aw"] * c["ah"], c["C"], c["H"], c["W"]
    valid = want["valid"].reshape(A, H, W)
    rows = []
    for m in range(A):
        if not c["mask"][m] or valid[m].all():
            continue
        srcs = M.sources(m, c["mask"], c["missing"], c["ang_major"], c["aw"], c["ah"], c["ang_radius"])
        if srcs:
            row = np.zeros(TAB, np.int32)
            row[0], row[1] = m, len(srcs)
            row[2:2 + 3 * len(srcs)] = np.array(srcs, np.int32).reshape(-1)
            rows.append(row)
    sai = np.flatnonzero(c["mask"]).astype(np.int32)
    case, out = os.path.join(tmp, "case"), os.path.join(tmp, "out")
    with open(case, "wb") as f:
        f.write(np.array([A, C, H, W, D, r, mv, len(sai), len(rows), c["flags"] is not None], np.int32).tobytes())
        f.write(sai.tobytes())
        f.write(c["missing"].astype(np.uint32).tobytes())
        f.write(c["lf"].tobytes())
        if c["flags"] is not None:
            f.write(c["flags"].tobytes())
        f.write(np.array(rows, np.int32).tobytes())
        f.write(float_tables(r).tobytes())
    run = subprocess.run([exe, case, out], capture_output=True, text=True)
    if run.returncode:
        print(run.stderr[-3000:])
        return None, want
    raw = np.fromfile(out, np.uint8)
    pos, val = A * H * W, A * C * H * W
    nt = ((W + TW - 1) // TW) * ((H + TH - 1) // TH)
    cuts = np.cumsum([0, pos, 4 * val, val, pos, 4 * A * nt, 8 * 17])
    g_valid, g_mid, g_rem, g_disp, g_tiles, g_hist = (raw[cuts[i]:cuts[i + 1]] for i in range(6))
    live = c["mask"] != 0
    tiles = np.zeros((A, nt), np.int64)
    bad = ~valid.astype(bool) & live[:, None, None]
    for t in range(nt):
        ty, tx = divmod(t, (W + TW - 1) // TW)
        tiles[:, t] = bad[:, ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW].sum(axis=(1, 2))
    ok = np.array_equal(g_valid.reshape(A, -1)[live], want["valid"][live])
    ok = ok and np.array_equal(g_mid.view(np.uint32).reshape(A, -1)[live], want["sweep"].view(np.uint32)[live])
    ok = ok and np.array_equal(g_rem.reshape(A, -1)[live], want["rem"][live])
    ok = ok and np.array_equal(g_disp.view(np.int8).reshape(A, -1), want["disp"])
    ok = ok and np.array_equal(g_tiles.view(np.uint32).reshape(A, nt), tiles)
    ok = ok and np.array_equal(g_hist.view(np.uint64).astype(np.int64), want["hist"])
    return bool(ok), want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "clang++"))
    args = ap.parse_args()
    lines = ["# Joint repair (lfbm5d_repair_*): the per-thread code of k_repair_valid and k_repair_sweep compiled for the host",
             "# (tools/repair_host_check.cpp: workgroups of 256 threads, the phases in the kernel's order on planes of the kernel's LDS",
             "# sizes; address and undefined-behaviour sanitizers on) against tests/repair_model.py on the cases of tests/repair_cases.py.",
             "# Compared: validity planes, the light field and the flags after the sweep, d*, unsound positions per tile, the histogram.",
             "# case, D, r, min_valid: targets, swept, values from other views, positions, result"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "repair_host_check")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               os.path.join(ROOT, "tools", "repair_host_check.cpp"), "-o", exe]
        subprocess.run(cmd, check=True)
        lines.append("# built with: " + " ".join(os.path.basename(w) if os.sep in w else w for w in cmd[:-2]))
        for name in K.NAMES + K.CLEAN:
            for D, r in K.DRS:
                for mv in K.MIN_VALIDS:
                    ok, want = run_case(exe, tmp, name, D, r, mv)
                    bad += not ok
                    line = (f"{name}, D = {D}, r = {r}, min_valid = {mv}: {want['targets']} targets, {want['swept']} swept, "
                            f"{int(want['views'].sum())} from other views, {want['positions']} positions: "
                            + ("bit-identical, no sanitizer report" if ok else "SANITIZER REPORT" if ok is None else "MISMATCH"))
                    print(line)
                    lines.append(line)
    lines.append(f"{'all cases bit-identical to the model, no access out of bounds' if not bad else str(bad) + ' cases failed'}")
    with open(os.path.join(ROOT, "profiles", "repair_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
