"""Inputs on which block matching meets EXACT ties: quantised, saturated, flat and periodic light-field windows, built from
tests/golden/sourceLF_3x3_256_u8.npy and numpy only.  Every case is a mirror-padded window [A][C*Hb*Wb] whose channel 0 (the only
plane block matching reads) is integer-valued inside bm_tie_model.exact_domain, so that model, oracle and GPU can be compared bit
for bit with no excluded position; for step 2 the pilot's channel 0 is such a plane too.  Channels 1 and 2 of colour windows carry
the photograph's other channels (any finite values would do).

A case: (name, kind, step, sigma, Cc, (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D), (rows, cols), aw, sums)
  kind   flat | q16 | q64 | sat | vstripes2 | vstripes4 | hstripes2 | hstripes4 | checker | edge | island | threq
  aw     angular window side (3 or 5)
  sums   True for the "natural" kinds (quantised, saturated): num / den are compared as well; the synthetic kinds stop at the
         tables and the group statistics (their transforms are degenerate).
"""
import functools

import numpy as np

import bm_tie_model as M
import helpers as Hh

ID3, DCT3 = ("id", "sadct", "haar"), ("dct", "sadct", "haar")

CASES = [
    # flat: every candidate ties at 0; 121 candidates (65..128 class) and 169 (> 128)
    ("flat-k8-nsim5", "flat", 1, 25.0, 1, (8, 5, 2, 8, 3) + ID3, (48, 48), 3, False),
    ("flat-k16-nsim6-nd3", "flat", 1, 25.0, 3, (8, 6, 3, 16, 4) + ID3, (64, 64), 3, False),
    # quantised photograph
    ("q16-k8-ht", "q16", 1, 25.0, 3, (4, 6, 2, 8, 3) + ID3, (64, 64), 3, True),
    ("q64-k8-wien", "q64", 2, 25.0, 3, (8, 6, 2, 8, 3) + DCT3, (64, 64), 3, True),
    ("q16-k8-wien-n16-grey", "q16", 2, 25.0, 1, (16, 6, 2, 8, 4) + DCT3, (64, 64), 3, True),
    ("q16-k8-ht-grey-p4", "q16", 1, 20.0, 1, (4, 6, 2, 8, 4) + DCT3, (72, 72), 3, True),             # also the subset pass's window
    ("q16-k16-ht-nd3", "q16", 1, 25.0, 3, (8, 8, 3, 16, 4) + ID3, (96, 96), 3, True),
    ("q16-k16-ht-sigma50", "q16", 1, 50.0, 3, (8, 6, 2, 16, 3, "bior", "sadct", "haar"), (96, 96), 3, True),
    ("q16-k8-wien-nd6-nsim18", "q16", 2, 25.0, 3, (16, 18, 6, 8, 4) + DCT3, (48, 48), 3, True),     # the README's search window
    ("q16-k16-ht-wide-p3", "q16", 1, 25.0, 3, (8, 9, 3, 16, 3) + ID3, (72, 150), 3, True),          # ragged second / third strip
    ("q64-k8-wien-wide-p3", "q64", 2, 25.0, 3, (8, 9, 3, 8, 3) + DCT3, (72, 150), 3, True),
    ("sat-k8-ht-5x5", "sat", 1, 25.0, 1, (4, 5, 2, 8, 4) + ID3, (56, 56), 5, False),                 # 24 slots; tables and stats
    ("q16-k10-ht", "q16", 1, 25.0, 3, (4, 6, 2, 10, 4) + DCT3, (72, 72), 3, True),                   # any-size kernel
    ("q16-k6-ht", "q16", 1, 25.0, 3, (8, 6, 2, 6, 3) + ID3, (64, 64), 3, True),
    ("q64-k4-wien-grey", "q64", 2, 25.0, 1, (4, 5, 2, 4, 2, "bior", "sadct", "haar"), (48, 48), 3, True),
    # saturated: half the plane at the clip value
    ("sat-k8-ht-grey", "sat", 1, 25.0, 1, (8, 6, 2, 8, 3) + ID3, (64, 64), 3, True),
    ("sat-k8-wien", "sat", 2, 25.0, 3, (8, 6, 2, 8, 3) + DCT3, (64, 64), 3, True),
    ("sat-k16-ht-nd6-nsim18", "sat", 1, 25.0, 3, (8, 18, 6, 16, 4) + ID3, (48, 48), 3, True),        # README HT: 169 tables
    # periodic and piecewise-constant planes
    ("vstripes2-k8", "vstripes2", 1, 25.0, 3, (4, 6, 2, 8, 3) + ID3, (48, 48), 3, False),
    ("vstripes4-k16-nd3", "vstripes4", 1, 25.0, 1, (8, 6, 3, 16, 4) + ID3, (64, 80), 3, False),
    ("hstripes2-k16", "hstripes2", 1, 25.0, 3, (8, 6, 2, 16, 3) + ID3, (64, 64), 3, False),
    ("hstripes4-k8-wien-nd6", "hstripes4", 2, 25.0, 3, (8, 6, 6, 8, 3) + DCT3, (48, 48), 3, False),
    ("checker3-k8", "checker", 1, 25.0, 3, (8, 6, 2, 8, 3) + ID3, (48, 48), 3, False),
    ("checker3-k16-wien-grey", "checker", 2, 25.0, 1, (8, 6, 2, 16, 4) + DCT3, (64, 64), 3, False),
    ("edge-k8", "edge", 1, 25.0, 3, (8, 6, 2, 8, 3) + ID3, (48, 48), 3, False),
    ("edge-k16-wien-wide", "edge", 2, 25.0, 3, (8, 6, 2, 16, 4) + DCT3, (64, 150), 3, False),
    ("island-k8", "island", 1, 25.0, 3, (8, 6, 2, 8, 3) + ID3, (48, 48), 3, False),
    # a tested distance equal to tau k^2: colour Wiener pass, tau = 2000
    ("threq-k8-wien", "threq", 2, 25.0, 3, (8, 6, 2, 8, 3) + DCT3, (48, 56), 3, False),
    ("threq-k16-wien", "threq", 2, 25.0, 3, (8, 8, 3, 16, 4) + DCT3, (64, 80), 3, False),
]
IDS = [c[0] for c in CASES]
NATURAL = ("q16", "q64", "sat")


def by_name(name):
    return CASES[IDS.index(name)]


def _photo(A, aw, H, W):
    """[A][3][H][W] uint8: the golden light field's nine views, or a 5x5 grid cut from its centre view."""
    if aw == 3:
        return Hh.source_lf(crop=(H, W))
    return Hh.textured_lf(aw, aw, H, W)


def _scale(k):
    """Grey levels are halved for the patch sizes whose exact domain ends below 255 (k = 16: R <= 127; k = 10: R <= 204)."""
    return 2 if k > 8 else 1


def _plane0(kind, A, aw, H, W, k, p, nHW, matched):
    """Integer channel-0 planes [A][H][W] (float32) of a case.  matched=True: the planes block matching reads (the window of
    step 1, the pilot of step 2), which are the kind as the issue defines it.  matched=False: the window of a step-2 pass, for
    the natural kinds the same photograph with other noise, quantised the same way."""
    sc = _scale(k)
    st = np.arange(A)
    s, t = st // aw, st % aw
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((A, H, W), np.int64)
    if kind == "flat":
        out[:] = 100
    elif kind in ("q16", "q64", "sat"):
        g = _photo(A, aw, H, W)[:, 0].astype(np.float64)
        rng = np.random.default_rng(17 if matched else 18)
        if kind == "sat":
            v = np.clip(np.rint(2.5 * g + rng.normal(0, 10, g.shape)), 0, 255)
            out = (v // sc).astype(np.int64)
        else:
            q = 16 if kind == "q16" else 4
            if not matched:
                g = np.clip(g + rng.normal(0, 4, g.shape), 0, 255)
            out = (np.floor(g / q) * (q // sc)).astype(np.int64)
    elif kind in ("vstripes2", "vstripes4", "hstripes2", "hstripes4"):
        per = int(kind[-1])
        for a in range(A):      # one pixel of shift per view, along the stripes' normal
            c = (x + t[a]) if kind[0] == "v" else (y + s[a])
            out[a] = 40 + 80 * ((c % per) < per // 2)
    elif kind == "checker":
        for a in range(A):
            out[a] = 30 + 90 * ((((x + t[a]) // 3) + ((y + s[a]) // 3)) % 2)
    elif kind == "edge":
        for a in range(A):
            out[a] = 50 + 70 * (x + t[a] >= W // 2)
    elif kind == "island":
        # a flat plane with one 14 x 14 block of random 20 / 220 pixels: patches on the block match nothing but themselves (one
        # candidate passes: the duplicate rule), patches that touch it match a few, and everything else ties at 0
        blk = 20 + 200 * np.random.default_rng(5).integers(0, 2, (14, 14))
        for a in range(A):
            out[a] = 100
            y0, x0 = H // 2 - 7 + (s[a] - aw // 2), W // 2 - 7 + (t[a] - aw // 2)
            out[a, y0:y0 + 14, x0:x0 + 14] = blk
    elif kind == "threq":
        # a staircase 100 | 160 (k/2 columns) | 180: the patch that ends in the middle of the 160 step differs from the one k/2
        # columns to its right by 60 in half of its pixels and by 20 in the other half: (3600 + 400) / 2 * k^2 = 2000 k^2.  The
        # step starts k/2 columns right of a reference column of the centre view (padded column nHW + 3 p); the lower third of
        # the plane carries the staircase transposed, and every view is shifted by one pixel.
        c0 = 3 * p + k // 2
        for a in range(A):
            xx, yy = x + (t[a] - aw // 2), y + (s[a] - aw // 2)
            top = 100 + 60 * (xx >= c0) + 20 * (xx >= c0 + k // 2)
            r0 = 2 * H // 3 + k // 2
            out[a] = np.where(yy < 2 * H // 3, top, 100 + 60 * (yy >= r0) + 20 * (yy >= r0 + k // 2))
    else:
        raise ValueError(kind)
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(win, basic (None for step 1), est [A][Hb][Wb] = the planes block matching reads, Wb, Hb, A, cc, tau)."""
    _, kind, step, sigma, Cc, pk, (H, W), aw, _ = by_name(name)
    N, nSim, nDisp, k, p = pk[:5]
    A, nHW = aw * aw, nSim + nDisp
    photo = _photo(A, aw, H, W).astype(np.float32)

    def window(matched):
        arr = np.zeros((A, Cc, H, W), np.float32)
        arr[:, 0] = _plane0(kind, A, aw, H, W, k, p, nHW, matched)
        if Cc == 3:
            arr[:, 1] = 0.5 * (photo[:, 0] - photo[:, 2])
            arr[:, 2] = 0.25 * (photo[:, 0] - 2 * photo[:, 1] + photo[:, 2])
        win, Wb, Hb = Hh.padded_window(arr.reshape(A, -1), W, H, Cc, nHW, color=False)
        return win, Wb, Hb

    win, Wb, Hb = window(step == 1)
    basic = window(True)[0] if step == 2 else None
    est = (win if step == 1 else basic)[:, :Wb * Hb].reshape(A, Hb, Wb)
    for a in range(A):
        M.exact_domain(est[a], k)
    return dict(win=win, basic=basic, est=est, Wb=Wb, Hb=Hb, A=A, cc=A // 2, tau=Hh.tau_match(sigma, Cc, step))


def refs_of(name):
    c = by_name(name)
    N, nSim, nDisp, k, p = c[5][:5]
    b = build(name)
    rows, cols = M.ref_grid(b["Hb"], k, nSim + nDisp, p), M.ref_grid(b["Wb"], k, nSim + nDisp, p)
    return (rows[:, None] * b["Wb"] + cols[None, :]).reshape(-1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def model(name):
    """The exact model's tables and tie statistics of a case: self (centre view) and disp[st] for every other view."""
    c = by_name(name)
    N, nSim, nDisp, k, p = c[5][:5]
    b = build(name)
    est, cc = b["est"], b["cc"]
    refs = refs_of(name)
    return dict(refs=refs, self=M.self_search(est[cc], k, N, nSim, nDisp, b["tau"], refs),
                disp={st: M.disparity_search(est[cc], est[st], k, nDisp, b["tau"]) for st in range(b["A"]) if st != cc})


def path_classes(n_pass, N):
    """The selection-path classes of the issue the passing-candidate counts of a case reach."""
    n = np.asarray(n_pass)
    out = set()
    if ((n < N) & (n > 0) & ((n & (n - 1)) != 0)).any():
        out.add("<N,not-pow2")
    if (n == 1).any():
        out.add("1")
    if ((n >= 2) & (n <= 64)).any():
        out.add("2..64")
    if ((n >= 65) & (n <= 128)).any():
        out.add("65..128")
    if (n > 128).any():
        out.add(">128")
    return out
