#!/usr/bin/env python3
"""Host check of the occlusion-aware plane sweep ahead of any GPU run: builds tools/occl_host_check.cpp (the per-thread code of
k_view_sweep_occl, lfbm5d_amd/csrc/lfbm5d_occl_device.h, compiled for the host as a stand-alone program) with the address and
undefined-behaviour sanitizers, drives it workgroup by workgroup over the narrow, the tile-edge, the 24-source and the occluder shapes
of tests/occl_cases.py at steps 1, 2 and 4, (D, r) = (0, 0), (3, 7), (8, 0), (8, 7), the ratios 1, the shipped default and 8, in both
instantiations where the source count allows, and compares values, j*, k*, the 65-bin histogram and the set histogram with the numpy
model (tests/occl_model.py) bit for bit.  Needs no GPU.  Writes profiles/occl_parity.txt.

    python tools/occl_host_check.py [--cxx clang++] [--ratios 1,4,8]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import occl_cases as K        # noqa: E402
import subpel_model as S      # noqa: E402
import view_model as V        # noqa: E402

TAB = 2 + 3 * 24
SHAPES = ("narrow-1x3", "narrow-3x1", "centre", "corners", "empty-source", "centre-R2", "single-63", "edges-31x65", "rect-31x65-centre",
          "rect-31x65-edge", "rect-31x65-two", "stripes-31x65-centre", "stripes-31x65-two", "stripes-65x127-edge", "rect-5x5", "stripes-5x5")


def shipped_ratio():
    """lfbm5d_view_occl_default() as the library's source states it (no library is loaded here)."""
    src = open(os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_view.hip")).read()
    return float(re.search(r"float lfbm5d_view_occl_default\(void\) \{ return ([0-9.]+)f; \}", src).group(1))


def write_case(path, shape, kind, steps, D, r, ratio, hold):
    ah, aw, H, W, C, miss, empty, R = K.SHAPES[shape]
    lf, mask, missing = K.case(shape, kind)
    rows = []
    for m in miss:
        srcs = V.sources(m, mask, missing, K.ROWMAJOR, aw, ah, R)
        row = np.zeros(TAB, np.int32)
        row[0], row[1] = m, len(srcs)
        row[2:2 + 3 * len(srcs)] = np.array(srcs, np.int32).reshape(-1)
        rows.append(row)
    most = max(int(row[1]) for row in rows)
    if hold and most > 8:
        return False
    A = ah * aw
    with open(path, "wb") as f:
        f.write(np.array([A, C, H, W, len(rows), D, steps, r, int(hold)], np.int32).tobytes())
        f.write(np.array([ratio], np.float32).tobytes())
        f.write(np.ascontiguousarray(lf, np.float32).tobytes())
        f.write(np.full(lf.shape, K.OUT_SENTINEL, np.float32).tobytes())
        f.write(np.full((A, H * W), K.DISP_SENTINEL, np.int8).tobytes())
        f.write(np.full((A, H * W), K.SET_SENTINEL, np.uint8).tobytes())
        f.write(np.array(rows, np.int32).tobytes())
    return True


def compare(path, shape, want):
    ah, aw, H, W, C, miss, empty, R = K.SHAPES[shape]
    A = ah * aw
    raw = np.fromfile(path, np.uint8)
    nv, npl = A * C * H * W * 4, A * H * W
    out = raw[:nv].view(np.uint32).reshape(A, -1)
    disp = raw[nv:nv + npl].view(np.int8).reshape(A, -1)
    sets = raw[nv + npl:nv + 2 * npl].reshape(A, -1)
    cnt = raw[nv + 2 * npl:].copy().view(np.uint64).astype(np.int64)
    return (np.array_equal(out, want["out"].view(np.uint32)) and np.array_equal(disp, want["disp"]) and np.array_equal(sets, want["sets"])
            and np.array_equal(cnt[:S.HIST], want["hist"]) and np.array_equal(cnt[S.HIST:], want["set_hist"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "clang++"))
    ap.add_argument("--ratios", default=None, help="comma-separated; default: 1, the shipped default, 8")
    args = ap.parse_args()
    ratios = [float(v) for v in args.ratios.split(",")] if args.ratios else sorted({1.0, shipped_ratio(), 8.0})
    lines = ["# Occlusion-aware plane sweep (lfbm5d_view_*_occl_*): the per-thread code of k_view_sweep_occl compiled for the host",
             "# (tools/occl_host_check.cpp: workgroups of 256 threads, the kernel's phases with its barriers as the boundaries between the",
             "# loops over the threads; address and undefined-behaviour sanitizers on) against tests/occl_model.py on shapes of",
             "# tests/occl_cases.py.  Compared: the output light field with sentinels in what must not be written, j* (int8), k* (uint8), the",
             "# 65-bin histogram, the set histogram.  hold = the instantiation that keeps a channel's warped values in registers (n <= 8),",
             "# recompute = the other.",
             "# shape, data, steps, D, r, ratio, instantiation: positions per k* (set 0..4), result"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "occl_host_check")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               os.path.join(ROOT, "tools", "occl_host_check.cpp"), "-o", exe]
        subprocess.run(cmd, check=True)
        lines.append("# built with: " + " ".join(os.path.basename(w) if os.sep in w else w for w in cmd[:-2]))
        for shape in SHAPES:
            kinds = K.kinds(shape) if shape.startswith("narrow") else K.kinds(shape)[-1:]
            for kind in kinds:
                for steps in K.STEPS:
                    for D, r in K.DRS:
                        for ratio in ratios:
                            want = None
                            for hold in (True, False):
                                if not write_case(os.path.join(tmp, "case"), shape, kind, steps, D, r, ratio, hold):
                                    continue
                                want = want or K.model(shape, kind, steps, D, r, ratio)
                                run = subprocess.run([exe, os.path.join(tmp, "case"), os.path.join(tmp, "out")], capture_output=True, text=True)
                                if run.returncode:
                                    ok = False
                                    print(run.stderr[-3000:])
                                else:
                                    ok = compare(os.path.join(tmp, "out"), shape, want)
                                bad += not ok
                                line = (f"{shape}, {kind}, steps = {steps}, D = {D}, r = {r}, ratio = {ratio:g}, {'hold' if hold else 'recompute'}: "
                                        f"{' '.join(str(int(v)) for v in want['set_hist'])}: "
                                        + ("bit-identical, no sanitizer report" if ok else "MISMATCH" if not run.returncode else "SANITIZER REPORT"))
                                print(line, flush=True)
                                lines.append(line)
    lines.append(f"{'all cases bit-identical to the model, no access out of bounds' if not bad else str(bad) + ' cases failed'}")
    with open(os.path.join(ROOT, "profiles", "occl_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
