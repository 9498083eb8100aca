#!/usr/bin/env python3
"""Sweep of the consistency check's decision parameters with the numpy model (tests/consist_model.py; needs no GPU -- the GPU equals the
model bit for bit, tests/test_gpu_consist.py).  Golden light field, rows and columns 64..191 (3 x 3 x 128 x 128 x 3), clean and with
sigma = 10 noise (seed 1), at the view synthesis' D and r:
  defects   synth.add_defects(seed=2) written as 0 or 255 (whichever is farther from the value)
  dimmed    the same map, the values times 0.6
  bad SAI   synth.degrade_sai(kind, seed=1) of the centre (4), an edge (1) and a corner (0) SAI, kinds dim, noise and shift
Swept: k in {4, 6, 8, 12} x spread in {1, 2, 3, 4} x min_sources in {2, 3, 4, 5} x sai_factor in {1.5, 2, 3}; min_scale, max_rounds and
min_threshold at the library's defaults.  (min_sources = 3 is the number of sources a corner SAI of a complete field has: it tests the
corners, and stops testing one once a neighbour of it has been excluded and two sources on one side are left to extrapolate from.)  Per row: recall = flagged share of the planted values that changed by at least 16 grey levels,
false = flagged share of the values outside the map, both over all nine SAIs (an untested SAI counts with nothing flagged); bad-SAI cases
(of 18) in which exactly the degraded SAI was found bad; SAIs found bad in the four defect inputs (all of them false).
Writes profiles/consist_defaults.txt, with the row the rule below picks and the `shipped:` row of the library's defaults that
tests/test_consist.py checks.

    python tools/consist_sweep.py
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lfbm5d_amd as L                 # noqa: E402
from lfbm5d_amd import synth           # noqa: E402
import consist_model as M              # noqa: E402
import view_model as V                 # noqa: E402

KS, SPREADS, MIN_SOURCES, SAI_FACTORS = (4.0, 6.0, 8.0, 12.0), (1.0, 2.0, 3.0, 4.0), (2, 3, 4, 5), (1.5, 2.0, 3.0)
FALSE_CAP = 0.005


def far(base, fl):
    return np.where(fl, np.where(base > 127.0, np.float32(0.0), np.float32(255.0)), base).astype(np.float32)


def main():
    P = L.consist_params()
    D, r, R = P.max_disparity, P.box_radius, P.ang_radius
    clean = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy"))[:, :, 64:192, 64:192].astype(np.float32)
    fl = synth.add_defects(clean.shape, seed=2)
    mask = np.ones(9, np.uint32)
    inputs = []                                                                  # (name, light field, map or None, degraded SAI or None)
    for sigma in (0, 10):
        base = synth.add_noise_mt19937(clean, float(sigma), seed=1) if sigma else clean
        tag = f"sigma {sigma}"
        inputs.append((f"{tag} defects", far(base, fl), fl, None))
        inputs.append((f"{tag} dimmed", np.where(fl, base * np.float32(0.6), base).astype(np.float32), fl, None))
        for st, pos in ((4, "centre"), (1, "edge"), (0, "corner")):
            for kind in ("dim", "noise", "shift"):
                inputs.append((f"{tag} {kind} {pos}", synth.degrade_sai(base, st, kind, seed=1), None, st))
    bases = {0: clean, 10: synth.add_noise_mt19937(clean, 10.0, seed=1)}
    caches = [dict() for _ in inputs]

    def run(i, k, spread, ms, sf):
        y = inputs[i][1]
        return M.consist(y.reshape(9, -1), mask, V.ROWMAJOR, 3, 3, 128, 128, 3, D=D, r=r, ang_radius=R, k=k, min_threshold=P.min_threshold,
                         spread=spread, min_sources=ms, sai_factor=sf, min_scale=P.min_scale, max_rounds=P.max_rounds, cache=caches[i])

    rows = []
    for k, spread, ms, sf in itertools.product(KS, SPREADS, MIN_SOURCES, SAI_FACTORS):
        rec, fal, right, false_bad, cells = [], [], 0, 0, []
        for i, (name, y, m, st) in enumerate(inputs):
            res = run(i, k, spread, ms, sf)
            if m is None:
                right += res["bad"] == [st]
                continue
            base = bases[0 if name.startswith("sigma 0") else 10]
            got = res["flags"].reshape(y.shape) != 0
            changed = m & (np.abs(y - base) >= 16.0)
            rec.append(float((got & changed).sum()) / float(changed.sum()))
            fal.append(float((got & ~m).sum()) / float((~m).sum()))
            false_bad += len(res["bad"])
            cells.append(f"{100 * rec[-1]:5.1f} {100 * fal[-1]:5.2f}")
        rows.append(dict(k=k, spread=spread, ms=ms, sf=sf, recall=float(np.mean(rec)), false=float(np.mean(fal)), right=right, false_bad=false_bad,
                         text=f"{k:4.0f} {spread:6.0f} {ms:11d} {sf:10.1f} | " + " | ".join(cells) + f" | {right:2d} of 18 | {false_bad}"))
        print(rows[-1]["text"], flush=True)
    best_right = max(w["right"] for w in rows if w["false_bad"] == 0)
    ok = [w for w in rows if w["false_bad"] == 0 and w["right"] == best_right and w["false"] <= FALSE_CAP]
    pick = max(ok, key=lambda w: (round(w["recall"], 4), w["ms"], w["spread"], w["k"], -w["sf"])) if ok else None

    y = inputs[0][1]
    res = M.consist(y.reshape(9, -1), mask, V.ROWMAJOR, 3, 3, 128, 128, 3, D=D, r=r, ang_radius=R, k=P.k, min_threshold=P.min_threshold,
                    spread=P.spread, min_sources=P.min_sources, sai_factor=P.sai_factor, min_scale=P.min_scale, max_rounds=P.max_rounds,
                    cache=caches[0])
    got = res["flags"].reshape(y.shape) != 0
    lines = ["# Consistency check (lfbm5d_consist_*): sweep of the decision parameters with the numpy model (tools/consist_sweep.py), on ONE light",
             f"# field: golden rows and columns 64..191, 3 x 3 views, D = {D}, r = {r}, ang_radius = {R}, min_scale = {P.min_scale:g}, max_rounds = "
             f"{P.max_rounds}, min_threshold = {P.min_threshold:g}.",
             "# Columns: recall % and false % (see the tool's docstring) for clean defects 0/255, clean dimmed x0.6, sigma 10 defects, sigma 10",
             "# dimmed; bad-SAI cases right (centre / edge / corner x dim / noise / shift x clean / sigma 10); SAIs found bad in the defect inputs.",
             "# With min_sources >= 4 the corner SAIs of a 3 x 3 field (3 sources) are untested: their 6 bad-SAI cases cannot be right and",
             "# their defects count as missed; with min_sources = 2 they are tested on 3 sources.",
             "   k spread min_sources sai_factor | clean 0/255  | clean x0.6   | s10 0/255    | s10 x0.6     | bad SAI  | false bad"]
    lines += [w["text"] for w in rows]
    lines.append(f"# rule: no SAI found bad in the defect inputs, the most bad-SAI cases right ({best_right}), mean false share <= {100 * FALSE_CAP:g} %, then "
                 "the largest mean recall; ties to the larger min_sources, the larger spread, the larger k, the smaller sai_factor")
    lines.append("picked: " + (f"k = {pick['k']:g}, spread = {pick['spread']:g}, min_sources = {pick['ms']}, sai_factor = {pick['sf']:g} "
                               f"(mean recall {100 * pick['recall']:.1f} %, mean false {100 * pick['false']:.2f} %)" if pick else "no row meets the rule"))
    lines.append(f"shipped: k = {P.k:g}, spread = {P.spread:g}, min_sources = {P.min_sources}, sai_factor = {P.sai_factor:g}, min_scale = {P.min_scale:g}; "
                 f"golden crop clean, add_defects(seed=2) as 0 / 255: flagged {int(got.sum())}, true hits {int((got & fl).sum())}, "
                 f"false hits {int((got & ~fl).sum())}, bad SAIs {res['bad']}")
    with open(os.path.join(ROOT, "profiles", "consist_defaults.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
