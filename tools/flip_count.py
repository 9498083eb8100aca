#!/usr/bin/env python3
"""Hard-threshold decisions against the oracle, group by group: for the hard-thresholding parity cases (tests/test_gpu_parity.py
PASS_CASES) the number of (group, channel) pairs whose survivor count differs from the oracle's, and by how much.  A/B tool for
changes of the transform arithmetic (LFBM5D_HIP_LIB selects the library).
--referee: instead of the oracle, the same pass again in reference-order arithmetic (ht_reference_order, LFBM5D_HT_REF_ORDER); counts
the (group, channel) pairs whose weight differs between the two (bitwise), and the guard-band pairs of the fast chain.
--sigma / --scale: noise level and data range (x scale) of the headline window.
usage: python tools/flip_count.py [--referee] [--sigma S] [--scale X] [full [seed ...] | case-name-substring ...]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as Hh  # noqa: E402
import test_gpu_parity as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
import lfbm5d_amd as L  # noqa: E402


def referee(ctx, sigma, pk, win, Wb, Hb, Cc):
    """the pass with the fast chain, then in reference order: (group, channel) pairs with different weights, guard-band pairs, all pairs"""
    w = []
    for ref in (False, True):
        if ref:
            os.environ["LFBM5D_HT_REF_ORDER"] = "1"
        T.gpu_pass(ctx, 1, sigma, pk, win, None, Wb, Hb, Cc)
        os.environ.pop("LFBM5D_HT_REF_ORDER", None)
        R = len(ctx.last_bm(pk[0], 9, Wb * Hb)[0])
        w.append(ctx.last_weights(R, Cc))
        if not ref:
            lst = ctx.last_group_list()
            guard = int(((lst >> 29) != 7).sum())
    return int((w[0].view(np.uint32) != w[1].view(np.uint32)).sum()), guard, R * Cc


def full(ctx, seeds, sigma=25.0, scale=1.0, use_referee=False):
    """the headline window (3x3x512x512 -> 560x560, README HT parameters: 864 M coefficients per pass) on the benchmark's synthetic
    light field (x scale), one pass per noise seed"""
    from lfbm5d_amd import synth
    pk, H, W = Hh.README_HT, 512, 512
    lf = synth.make_lf(3, 3, H, W).reshape(9, 3, H, W).astype(np.float32) * np.float32(scale)
    for seed in seeds:
        noisy = lf + sigma * np.random.default_rng(seed).standard_normal(lf.shape).astype(np.float32)
        win, Wb, Hb = Hh.padded_window(np.ascontiguousarray(noisy.reshape(9, -1)), W, H, 3, pk[1] + pk[2])
        if use_referee:
            d, guard, pairs = referee(ctx, sigma, pk, win, Wb, Hb, 3)
            print(f"full 560x560 sigma {sigma:g} scale {scale:g} seed {seed}: groups x channels {pairs}  guard-band {guard} ({100.0 * guard / pairs:.2f} %)  "
                  f"weights differing from the reference order {d}", flush=True)
            continue
        num_o, den_o, st = Hh.oracle_pass(1, sigma, pk, win, None, Wb, Hb, 3)
        num_g, den_g = T.gpu_pass(ctx, 1, sigma, pk, win, None, Wb, Hb, 3)
        R = len(ctx.last_bm(pk[0], 9, Wb * Hb)[0])
        w_o, w_g = O.last_weights(R, 3), ctx.last_weights(R, 3)
        sig = np.zeros(4, np.float32)
        O.lib().orc_sigma_table(sigma, 3, O.OPP, sig)
        cnt_o = np.where(w_o == 1.0, 0.0, 1.0 / (w_o.astype(np.float64) * sig[:3].astype(np.float64) ** 2))
        cnt_g = np.where(w_g == 1.0, 0.0, 1.0 / (w_g.astype(np.float64) * sig[:3].astype(np.float64) ** 2))
        d = np.rint(cnt_g - cnt_o)
        print(f"full 560x560 seed {seed}: groups x channels {R * 3}  coefficients {int(st.stack_patches) * 9 * 256 * 3}  flipped {int((d != 0).sum())} "
              f"(max |delta| {int(np.abs(d).max())})  survivors {int(np.rint(cnt_o).sum())}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--referee", action="store_true")
    ap.add_argument("--sigma", type=float, default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("pats", nargs="*")
    args = ap.parse_args()
    ctx = L.Context(0)
    pats = args.pats
    if pats and pats[0] == "full":
        full(ctx, [int(x) for x in pats[1:]] or [1], 25.0 if args.sigma is None else args.sigma, args.scale, args.referee)
        ctx.close()
        return
    for case in T.PASS_CASES:
        name, step, sigma, pk, crop, useSD = case
        if step != 1 or useSD or pk[7] != "haar" or (pats and not any(p in name for p in pats)):
            continue
        sigma = sigma if args.sigma is None else args.sigma
        win, Wb, Hb, Cc = T.window(sigma, pk, crop)
        if args.scale != 1.0:
            win = np.ascontiguousarray(win * np.float32(args.scale))
        if args.referee:
            d, guard, pairs = referee(ctx, sigma, pk, win, Wb, Hb, Cc)
            print(f"{name:24s} sigma {sigma:g} scale {args.scale:g}: groups x channels {pairs:6d}  guard-band {guard:5d}  weights differing from the reference order {d}", flush=True)
            continue
        num_o, den_o, st = Hh.oracle_pass(step, sigma, pk, win, None, Wb, Hb, Cc)
        num_g, den_g = T.gpu_pass(ctx, step, sigma, pk, win, None, Wb, Hb, Cc)
        refs = ctx.last_bm(pk[0], 9, Wb * Hb)[0]
        R = len(refs)
        w_o, w_g = O.last_weights(R, Cc), ctx.last_weights(R, Cc)
        sig = np.zeros(4, np.float32)
        O.lib().orc_sigma_table(sigma, Cc, O.OPP, sig)
        cnt_o = np.where(w_o == 1.0, 0.0, 1.0 / (w_o.astype(np.float64) * sig[:Cc].astype(np.float64) ** 2))
        cnt_g = np.where(w_g == 1.0, 0.0, 1.0 / (w_g.astype(np.float64) * sig[:Cc].astype(np.float64) ** 2))
        d = np.rint(cnt_g - cnt_o)
        eo, eg = Hh.estimate(num_o, den_o, win), Hh.estimate(num_g, den_g, win)
        print(f"{name:24s} groups x channels {R * Cc:6d}  coefficients {int(st.stack_patches) * 9 * pk[3] ** 2 * Cc:10d}  flipped {int((d != 0).sum()):4d} "
              f"(max |delta| {int(np.abs(d).max())})  survivors {int(np.rint(cnt_o).sum()):9d}  max |est diff| {np.abs(eo - eg).max():.2e}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
