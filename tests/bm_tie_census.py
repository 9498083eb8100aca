"""The tie census: how often does the tie order of block matching matter?

Oracle and GPU keep candidate scan order on exact ties.  The reference calls std::partial_sort / std::sort
with a comparator that looks at the distance alone, so its order among equal distances is whatever the library leaves.  The
oracle's test switch orc_set_tie_order(1) makes the same library calls on the same scan-ordered candidate vectors; this module runs
both orders and counts, per input:
  refs      reference patches;  set: the selected SET of patches differs;  order: same set, another sequence;
            tie: two of the nSx + 1 best passing scores are equal (exact model; "-" on float data, where the model does not apply)
  positions disparity positions over all non-centre views;  disp: another displacement is chosen;  tie: the minimum is attained
            more than once
`python tests/bm_tie_census.py` writes profiles/bm_tie_census.txt.  The numbers depend on the C++ library's sort; only what
follows from the definition is asserted (tests/test_bm_ties.py): no tie, no difference.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bm_tie_cases as Cs
import bm_tie_model as M
import helpers as Hh
from oracle import oracle as O


def oracle_tables(est, cc, k, N, nSim, nDisp, tau, refs, views=None):
    """orc_bm_self on est[cc] and orc_bm_stereo est[cc] -> est[st]: idx, cnt, {st: (best, shape)} over the compared region."""
    A, Hb, Wb = est.shape
    lib = O.lib()
    refs = np.ascontiguousarray(refs, np.uint32)
    idx = np.zeros((len(refs), max(N, 1)), np.uint32)
    cnt = np.zeros(len(refs), np.uint32)
    centre = np.ascontiguousarray(est[cc].reshape(-1), np.float32)
    assert lib.orc_bm_self(centre, Wb, Hb, k, N, nSim + nDisp, nSim, tau, refs, len(refs), idx.reshape(-1), cnt) == 0
    rows, cols = M.region(Hb, Wb, k, nDisp)
    disp = {}
    for st in (range(A) if views is None else views):
        if st == cc:
            continue
        best, shape = np.zeros(Wb * Hb, np.uint32), np.zeros(Wb * Hb, np.uint8)
        assert lib.orc_bm_stereo(centre, np.ascontiguousarray(est[st].reshape(-1), np.float32), Wb, Hb, k, nDisp, tau, best, shape) == 0
        disp[st] = (best.reshape(Hb, Wb)[rows, cols].copy(), shape.reshape(Hb, Wb)[rows, cols].copy())
    return idx, cnt, disp


def count(est, cc, k, N, nSim, nDisp, p, tau, exact):
    """One census row (dict) and, for exact inputs, the model's tie masks with the per-item differences (for the assertions)."""
    A, Hb, Wb = est.shape
    nHW = nSim + nDisp
    rows, cols = M.ref_grid(Hb, k, nHW, p), M.ref_grid(Wb, k, nHW, p)
    refs = (rows[:, None] * Wb + cols[None, :]).reshape(-1).astype(np.uint32)
    lib = O.lib()
    i0, c0, d0 = oracle_tables(est, cc, k, N, nSim, nDisp, tau, refs)
    lib.orc_set_tie_order(1)
    try:
        i1, c1, d1 = oracle_tables(est, cc, k, N, nSim, nDisp, tau, refs)
    finally:
        lib.orc_set_tie_order(0)
    assert np.array_equal(c0, c1)
    seq = np.array([not np.array_equal(i0[r, :c0[r]], i1[r, :c0[r]]) for r in range(len(refs))])
    sets = np.array([set(i0[r, :c0[r]].tolist()) != set(i1[r, :c0[r]].tolist()) for r in range(len(refs))])
    dd = {st: d0[st][0] != d1[st][0] for st in d0}
    assert all(np.array_equal(d0[st][1], d1[st][1]) for st in d0)        # the minimum's VALUE does not depend on the order
    row = dict(refs=len(refs), set=int(sets.sum()), order=int((seq & ~sets).sum()),
               positions=int(sum(v.size for v in dd.values())), disp=int(sum(v.sum() for v in dd.values())),
               ref_tie=None, cut_tie=None, pos_tie=None)
    masks = None
    if exact:
        for a in range(A):
            M.exact_domain(est[a], k)
        ms = M.self_search(est[cc], k, N, nSim, nDisp, tau, refs)
        md = {st: M.disparity_search(est[cc], est[st], k, nDisp, tau) for st in d0}
        row.update(ref_tie=int(ms["tie_any"].sum()), cut_tie=int(ms["tie_cut"].sum()),
                   pos_tie=int(sum(m["tie_min"].sum() for m in md.values())))
        masks = dict(tie_any=ms["tie_any"], tie_cut=ms["tie_cut"], seq=seq, sets=sets,
                     disp={st: (md[st]["tie_min"], dd[st]) for st in d0})
    return row, masks


BASELINE_SETS = [  # name, step, sigma, parameters (helpers.py)
    ("readme-ht", 1, 25.0, Hh.README_HT), ("readme-wien", 2, 25.0, Hh.README_WIEN), ("config4-ht", 1, 10.0, Hh.C4_HT),
    ("config5-ht", 1, 50.0, Hh.C5_HT), ("config5-wien", 2, 50.0, Hh.C5_WIEN),
]
CROP = 96


def baseline_planes(sigma, pk, as_u8):
    """Channel 0 of the padded window of the golden light field's 96 x 96 crop with the suite's noise (helpers.noisy_lf): the
    opponent transform's first channel in float, or -- as_u8 -- the red channel rounded and clipped to 0..255 like an 8-bit file
    (halved for k = 16, whose exact domain ends at R = 127).  Both steps are counted on this plane (the Wiener step's
    pilot is not reproduced here), with each step's own threshold."""
    N, nSim, nDisp, k, p = pk[:5]
    lf = Hh.source_lf(crop=CROP)
    _, noisy = Hh.noisy_lf(lf, sigma)
    if as_u8:
        red = np.clip(np.rint(noisy.reshape(9, 3, CROP * CROP)[:, 0]), 0, 255) // (2 if k > 8 else 1)
        win, Wb, Hb = Hh.padded_window(np.ascontiguousarray(red, np.float32), CROP, CROP, 1, nSim + nDisp, color=False)
    else:
        win, Wb, Hb = Hh.padded_window(noisy, CROP, CROP, 3, nSim + nDisp)
    return np.ascontiguousarray(win[:, :Wb * Hb]).reshape(9, Hb, Wb)


def rows():
    """[(label, row, masks)] over the BASELINE sets (float and 8-bit) and the quantised / saturated cases."""
    out = []
    for name, step, sigma, pk in BASELINE_SETS:
        N, nSim, nDisp, k, p = pk[:5]
        for as_u8 in (False, True):
            est = baseline_planes(sigma, pk, as_u8)
            row, masks = count(est, 4, k, N, nSim, nDisp, p, Hh.tau_match(sigma, 3, step), exact=as_u8)
            out.append((f"{name} {'u8' if as_u8 else 'float'}", row, masks))
    for c in Cs.CASES:
        if c[1] in Cs.NATURAL:
            N, nSim, nDisp, k, p = c[5][:5]
            b = Cs.build(c[0])
            row, masks = count(b["est"], b["cc"], k, N, nSim, nDisp, p, b["tau"], exact=True)
            out.append((c[0], row, masks))
    return out


def fmt(rws):
    f = lambda v: "-" if v is None else str(v)
    lines = [f"{'input':30s} {'refs':>6s} {'set':>6s} {'order':>6s} {'tie':>6s} {'cut-tie':>7s} {'positions':>10s} {'disp':>8s} {'tie':>8s}"]
    for label, r, _ in rws:
        lines.append(f"{label:30s} {r['refs']:6d} {r['set']:6d} {r['order']:6d} {f(r['ref_tie']):>6s} {f(r['cut_tie']):>7s} "
                     f"{r['positions']:10d} {r['disp']:8d} {f(r['pos_tie']):>8s}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    path = os.path.join(Hh.ROOT, "profiles", "bm_tie_census.txt")
    head = ("Tie census of block matching: scan order (oracle, GPU) against std::partial_sort / std::sort with a first-only comparator\n"
            "(orc_set_tie_order(1)).  Columns: tests/bm_tie_census.py.  BASELINE sets: golden light field, 96 x 96 crop, the suite's noise.\n\n")
    cases = ["\nThe test windows (tests/bm_tie_cases.py) by the int64 model: share of reference patches with a tie at the cut, share of\n"
             "positions with a tied disparity minimum, tested values on the threshold, passing-candidate counts and their classes\n\n"
             f"{'case':28s} {'cut-tie':>8s} {'tied-min':>8s} {'thr-eq':>6s} {'passing':>10s}  classes"]
    for c in Cs.CASES:
        m = Cs.model(c[0])
        s = m["self"]
        tied = np.concatenate([d["tie_min"].reshape(-1) for d in m["disp"].values()])
        cases.append(f"{c[0]:28s} {100 * s['tie_cut'].mean():7.1f}% {100 * tied.mean():7.1f}% {int(s['thr_equal'].sum()):6d} "
                     f"{int(s['n_pass'].min()):4d}..{int(s['n_pass'].max()):<4d}  {', '.join(sorted(Cs.path_classes(s['n_pass'], c[5][0])))}")
    with open(path, "w") as fh:
        fh.write(head + fmt(rows()) + "\n".join(cases) + "\n")
    print(open(path).read())
