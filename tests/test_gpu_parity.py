"""GPU parity tests (run with -m gpu on an MI355X).  Every test drives the HIP path through the
C-ABI (liblfbm5d_hip.so via lfbm5d_amd.core) and checks it against the CPU oracle on the same
seeded inputs, or against size-independent properties at the benchmark's sizes.

Tolerances (float32 path; BASELINE.json north_star: PSNR within +-0.01 dB of the CPU path):
  * block-matching tables (indices, counts, shape flags): identical -- the kernels evaluate the
    reference's integral-image recurrence in the reference's order;
  * one core pass on identical inputs: coverage identical, estimate num/den within 2e-3 grey levels
    (transforms accumulate in float32 on the GPU, in double in the oracle);
  * whole steps: step 1 within 2e-3 grey levels, mean PSNR of either step within 0.01 dB.
"""
import os
import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc, num=None, den=None, mask=None, proc=None, useSD=0, cst=4, pst=4, aw=3):
    from lfbm5d_amd import core
    A = win.shape[0]
    d_win = torch.from_numpy(win).cuda()
    d_basic = torch.from_numpy(basic).cuda() if basic is not None else None
    d_num = torch.zeros_like(d_win) if num is None else torch.from_numpy(num).cuda()
    d_den = torch.zeros_like(d_win) if den is None else torch.from_numpy(den).cuda()
    mask = np.ones(A, np.uint32) if mask is None else mask
    proc = np.zeros(A, np.uint32) if proc is None else proc
    torch.cuda.synchronize()
    ctx.core_pass(step, core.make_params(sigma, 2.7, *pk, useSD=useSD), aw, aw, Wb, Hb, Cc, d_win, d_basic, d_num, d_den,
                  mask, proc, cst, pst)
    return d_num.cpu().numpy(), d_den.cpu().numpy()


def window(sigma, pk, crop, grey=False):
    lf = Hh.source_lf(crop=crop)
    if grey:
        lf = lf[:, :1]
    clean, noisy = Hh.noisy_lf(lf, sigma)
    Cc = lf.shape[1]
    ch, cw = (crop, crop) if np.isscalar(crop) else crop
    win, Wb, Hb = Hh.padded_window(noisy, cw, ch, Cc, pk[1] + pk[2])
    return win, Wb, Hb, Cc


PASS_CASES = [
    # name, step, sigma, params, crop, useSD
    ("ht-id-sadct-haar", 1, 25.0, (4, 6, 2, 8, 3, "id", "sadct", "haar"), 64, 0),
    ("ht-bior-sadct-haar", 1, 25.0, (4, 6, 2, 8, 3, "bior", "sadct", "haar"), 64, 0),
    ("ht-dct-dct-hw", 1, 25.0, (4, 6, 2, 8, 3, "dct", "dct", "hw"), 64, 0),
    ("ht-id-dct-haar", 1, 25.0, (8, 6, 2, 8, 4, "id", "dct", "haar"), 64, 0),      # lambda /= sqrt2 (core:206)
    ("ht-id-id-haar", 1, 25.0, (4, 6, 2, 8, 3, "id", "id", "haar"), 64, 0),
    ("ht-k16-n8", 1, 25.0, (8, 8, 3, 16, 4, "id", "sadct", "haar"), 96, 0),
    ("ht-k16-bior-n1", 1, 50.0, (1, 6, 2, 16, 3, "bior", "sadct", "haar"), 96, 0),   # sigma >= 35: tauMatch 5000
    ("ht-k12", 1, 25.0, (4, 6, 2, 12, 4, "dct", "sadct", "haar"), 72, 0),
    ("ht-k16-dct-n8", 1, 25.0, (8, 8, 3, 16, 4, "dct", "sadct", "haar"), 96, 0),     # BASELINE configuration 2's HT step
    ("ht-k16-dct-hw", 1, 25.0, (4, 6, 2, 16, 3, "dct", "dct", "hw"), 96, 0),
    ("ht-k16-bior-n8", 1, 10.0, (8, 8, 3, 16, 4, "bior", "sadct", "haar"), 96, 0),    # configuration 4's HT step
    ("wien-bior-n8-hw", 2, 25.0, (8, 6, 2, 8, 3, "bior", "dct", "hw"), 64, 0),
    ("wien-n32", 2, 10.0, (32, 8, 2, 8, 4, "dct", "sadct", "haar"), 64, 0),             # N = 32: generic group kernel
    ("ht-n32-hw", 1, 10.0, (32, 8, 2, 8, 4, "bior", "sadct", "hw"), 64, 0),
    ("ht-n32-dct5", 1, 10.0, (32, 8, 2, 8, 4, "bior", "sadct", "dct"), 64, 0),          # 32-point DCT along the stack
    ("wien-n32-dct5", 2, 10.0, (32, 8, 2, 8, 4, "dct", "sadct", "dct"), 64, 0),
    ("ht-n1-p5-bior", 1, 10.0, (1, 16, 3, 16, 5, "bior", "sadct", "haar"), 104, 0),     # README.md:76 (faster EPFL parameters)
    ("wien-n8-p5", 2, 10.0, (8, 16, 3, 8, 5, "dct", "sadct", "haar"), 104, 0),
    ("ht-usesd", 1, 25.0, (4, 6, 2, 8, 3, "id", "sadct", "haar"), 64, 1),
    ("wien-dct-sadct-haar", 2, 25.0, (8, 6, 2, 8, 3, "dct", "sadct", "haar"), 64, 0),
    ("wien-id-dct-hw", 2, 25.0, (8, 6, 2, 8, 3, "id", "dct", "hw"), 64, 0),
    ("wien-bior-n16", 2, 10.0, (16, 6, 2, 8, 4, "bior", "sadct", "haar"), 64, 0),
    ("wien-usesd", 2, 25.0, (8, 6, 2, 8, 3, "dct", "sadct", "haar"), 64, 1),
    ("ht-dct-sadct-dct5", 1, 25.0, (4, 6, 2, 8, 3, "dct", "sadct", "dct"), 64, 0),
    ("ht-id-dct-dct5", 1, 25.0, (8, 6, 2, 8, 4, "id", "dct", "dct"), 64, 0),
    ("wien-dct-sadct-dct5", 2, 25.0, (8, 6, 2, 8, 3, "dct", "sadct", "dct"), 64, 0),
    # non-square SAIs, step 3, wider than one 64-column strip with a ragged last strip (config-5 style: 625x434)
    ("ht-wide-n1-p3", 1, 50.0, (1, 9, 3, 16, 3, "bior", "sadct", "haar"), (72, 150), 0),
    ("ht-tall-id-p3", 1, 25.0, (8, 8, 3, 16, 3, "id", "sadct", "haar"), (150, 72), 0),
    ("wien-wide-n8-p3", 2, 25.0, (8, 9, 3, 8, 3, "dct", "sadct", "haar"), (72, 150), 0),
    # patch sizes without dedicated kernels (round 5; the reference takes any kHard / kWien, utilities_LF.cpp:1214, :1255, with an
    # all-ones "Kaiser" window, bm3d.cpp:1144-1146): the plain table kernel + the general group kernel
    ("ht-k10-dct", 1, 25.0, (4, 6, 2, 10, 4, "dct", "sadct", "haar"), 72, 0),
    ("ht-k6-id-n8", 1, 25.0, (8, 6, 2, 6, 3, "id", "sadct", "haar"), 64, 0),
    ("wien-k10-dct", 2, 25.0, (8, 6, 2, 10, 4, "dct", "sadct", "haar"), 72, 0),
    ("ht-k32-bior", 1, 25.0, (2, 6, 2, 32, 8, "bior", "sadct", "haar"), 112, 0),
    ("wien-k32-dct", 2, 25.0, (2, 6, 2, 32, 8, "dct", "dct", "hw"), 112, 0),
    ("ht-k4-bior", 1, 25.0, (4, 5, 2, 4, 2, "bior", "sadct", "haar"), 48, 0),
    ("wien-k12-dct-n8-hw", 2, 25.0, (8, 6, 2, 12, 4, "dct", "sadct", "hw"), 72, 0),   # stacks beyond 64 KB: the slab kernel (round 5)
]


@pytest.mark.parametrize("case", PASS_CASES, ids=[c[0] for c in PASS_CASES])
def test_core_pass_matches_oracle(ctx, case):
    _check_pass(ctx, case, strict=True)


def _check_pass(ctx, case, strict):
    name, step, sigma, pk, crop, useSD = case
    win, Wb, Hb, Cc = window(sigma, pk, crop)
    _check_window(ctx, name, step, sigma, pk, useSD, win, Wb, Hb, Cc, strict)


def _check_window(ctx, name, step, sigma, pk, useSD, win, Wb, Hb, Cc, strict, basic=None):
    if step == 2 and basic is None:  # a plausible pilot: the oracle's own HT estimate of this window
        n1, d1, _ = Hh.oracle_pass(1, sigma, (pk[0] // 2 or 1,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc)
        basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    num_o, den_o, st = Hh.oracle_pass(step, sigma, pk, win, basic, Wb, Hb, Cc, useSD=useSD)
    ctx.reset_stats()
    num_g, den_g = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc, useSD=useSD)
    s = ctx.stats()
    assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
    # block matching: identical tables
    N, nSim, nDisp, k = pk[0], pk[1], pk[2], pk[3]
    refs, idx, cnt, best, shape = ctx.last_bm(N, 9, Wb * Hb)
    est = (win if step == 1 else basic)[:, :Wb * Hb]
    tau = Hh.tau_match(sigma, Cc, step)
    o_idx = np.zeros((len(refs), max(N, 1)), np.uint32)
    o_cnt = np.zeros(len(refs), np.uint32)
    O.lib().orc_bm_self(np.ascontiguousarray(est[4]), Wb, Hb, k, N, nSim + nDisp, nSim, tau, refs, len(refs),
                        o_idx.reshape(-1), o_cnt)
    assert np.array_equal(o_cnt, cnt)
    for r in range(len(refs)):
        assert np.array_equal(o_idx[r, :o_cnt[r]], idx[r, :cnt[r]]), (name, r)
    regr, regc = slice(nDisp, Hb - k - nDisp + 1), slice(nDisp, Wb - k - nDisp + 1)
    for st_i in (0, 5, 7):
        ob, osh = np.zeros(Wb * Hb, np.uint32), np.zeros(Wb * Hb, np.uint8)
        O.lib().orc_bm_stereo(np.ascontiguousarray(est[4]), np.ascontiguousarray(est[st_i]), Wb, Hb, k, nDisp, tau, ob, osh)
        assert np.array_equal(ob.reshape(Hb, Wb)[regr, regc], best[st_i].reshape(Hb, Wb)[regr, regc])
        assert np.array_equal(osh.reshape(Hb, Wb)[regr, regc], shape[st_i].reshape(Hb, Wb)[regr, regc])
    # aggregation buffers
    assert np.array_equal(den_o != 0, den_g != 0)
    # A Wiener group whose shrinkage coefficients sum to a denormal (a pilot with values around 1e-20, as a hard-threshold
    # pass leaves them where it kills nearly everything) gets the weight 1 / (sigma^2 * sum) = inf
    # (core:1219, :1544): the reference then carries inf / NaN in num and den.  Same entries here, everything else compared.
    nf = ~(np.isfinite(num_o) & np.isfinite(den_o))
    assert np.array_equal(nf, ~(np.isfinite(num_g) & np.isfinite(den_g)))
    if nf.any():
        assert step == 2 and nf.mean() < 0.01
        num_o, den_o, num_g, den_g = (np.where(nf, 0.0, a).astype(np.float32) for a in (num_o, den_o, num_g, den_g))
    eo, eg = Hh.estimate(num_o, den_o, win), Hh.estimate(num_g, den_g, win)
    if strict:
        np.testing.assert_allclose(den_g, den_o, rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(num_g, num_o, rtol=2e-5, atol=2e-2 * max(1.0, float(np.abs(den_o).max())))
        assert np.abs(eo - eg).max() < 2e-3
    elif step == 1 and not useSD:
        # arbitrary configurations, hard-threshold step: the transforms accumulate in float here and in double in the oracle,
        # so a threshold decision can flip for a coefficient within ~1e-6 of the threshold.  Stated group by group: the
        # weights 1 / (sigma_c^2 count) (core:413-421) give every group's survivor count on both sides; all but a few groups
        # per thousand agree exactly, the rest differ by EXACTLY ONE coefficient, and every `den` entry no such group
        # aggregates into is held to 2e-5.
        R = len(refs)
        w_o, w_g = O.last_weights(R, Cc), ctx.last_weights(R, Cc)
        sig = np.zeros(4, np.float32)
        O.lib().orc_sigma_table(sigma, Cc, O.OPP, sig)
        cnt_o = np.where(w_o == 1.0, 0.0, 1.0 / (w_o.astype(np.float64) * sig[:Cc].astype(np.float64) ** 2))
        cnt_g = np.where(w_g == 1.0, 0.0, 1.0 / (w_g.astype(np.float64) * sig[:Cc].astype(np.float64) ** 2))
        dcnt = np.rint(cnt_g - cnt_o)
        assert np.abs((cnt_g - cnt_o) - dcnt).max() < 1e-2 and np.abs(np.rint(cnt_o) - cnt_o).max() < 1e-2   # counts are integers
        flipped = np.argwhere(dcnt != 0)
        assert np.abs(dcnt).max() <= 1 and len(flipped) <= max(2, int(0.01 * R * Cc)), (len(flipped), R * Cc)
        # the entries a flipped (group, channel) aggregates into: its N matches in each of the 9 SAIs
        plane = Wb * Hb
        touched = np.zeros((9, Cc, Hb, Wb), bool)
        best9 = best.reshape(9, plane)
        for (r, c) in flipped:
            for n in range(int(cnt[r])):
                ip = int(idx[r, n])
                for st in range(9):
                    pos = ip if st == 4 else int(best9[st, ip])
                    touched[st, c, pos // Wb:pos // Wb + k, pos % Wb:pos % Wb + k] = True
        tm = touched.reshape(9, -1)
        np.testing.assert_allclose(np.where(tm, 0, den_g), np.where(tm, 0, den_o), rtol=2e-5, atol=1e-7)
        assert np.abs(eo - eg)[~tm].max() < 2e-3 and np.abs(eo - eg).mean() < 2e-4
    else:
        # Wiener step / SD weights: no threshold; weights are float sums of up to N A k^2 = 36 864 shrinkage coefficients
        # (relative round-off up to ~1.3e-4 measured)
        bad = ~np.isclose(den_g, den_o, rtol=2e-4, atol=1e-7)
        assert bad.mean() < 1e-4, bad.mean()
        assert np.abs(eo - eg).mean() < 2e-4 and np.quantile(np.abs(eo - eg), 0.999) < 5e-2


def test_pass_accumulates_into_existing_buffers_and_skips_processed_sais(ctx):
    pk = (4, 6, 2, 8, 3, "id", "sadct", "haar")
    win, Wb, Hb, Cc = window(25.0, pk, 64)
    rng = np.random.default_rng(5)
    base_n = rng.uniform(0, 50, size=win.shape).astype(np.float32)
    base_d = rng.uniform(0.1, 1, size=win.shape).astype(np.float32)
    proc = np.zeros(9, np.uint32)
    proc[[1, 6]] = 1
    num_o, den_o, _ = Hh.oracle_pass(1, 25.0, pk, win, None, Wb, Hb, Cc, num=base_n.copy(), den=base_d.copy(), proc=proc)
    num_g, den_g = gpu_pass(ctx, 1, 25.0, pk, win, None, Wb, Hb, Cc, num=base_n.copy(), den=base_d.copy(), proc=proc)
    per = Cc * Wb * Hb
    assert np.array_equal(num_g[1], base_n[1]) and np.array_equal(den_g[6], base_d[6])   # core:486
    np.testing.assert_allclose(den_g, den_o, rtol=2e-5)
    np.testing.assert_allclose(num_g, num_o, rtol=2e-5, atol=1e-2)


def test_empty_sai_switches_to_sadct_like_the_reference(ctx, monkeypatch):
    """bm5d.cpp:276-280: an empty SAI in the window forces SADCT; its slot stays untouched."""
    pk_dct = (4, 6, 2, 8, 3, "id", "dct", "haar")
    pk_sa = (4, 6, 2, 8, 3, "id", "sadct", "haar")
    win, Wb, Hb, Cc = window(25.0, pk_dct, 64)
    mask = np.ones(9, np.uint32)
    mask[2] = 0
    win[2] = 0
    proc = (1 - mask).astype(np.uint32)
    num_o, den_o, st = Hh.oracle_pass(1, 25.0, pk_sa, win, None, Wb, Hb, Cc, mask=mask, proc=proc)
    num_g, den_g = gpu_pass(ctx, 1, 25.0, pk_sa, win, None, Wb, Hb, Cc, mask=mask, proc=proc)
    assert st.sadct_groups == st.groups
    assert not den_g[2].any() and not num_g[2].any()
    np.testing.assert_allclose(den_g, den_o, rtol=2e-5)
    assert np.abs(Hh.estimate(num_o, den_o, win) - Hh.estimate(num_g, den_g, win)).max() < 2e-3
    # the kernels of such windows (k_group_id_haar_sa: the transform inline, in registers) against the call form of the others
    monkeypatch.setenv("LFBM5D_NO_SA_KERNELS", "1")
    num_c, den_c = gpu_pass(ctx, 1, 25.0, pk_sa, win, None, Wb, Hb, Cc, mask=mask, proc=proc)
    # same products in the same order, but hipcc's contraction of multiply-adds follows the code's shape: round-off apart (the odd
    # threshold decision with it), both at the oracle's bounds
    np.testing.assert_allclose(den_c, den_o, rtol=2e-5)
    np.testing.assert_allclose(den_c, den_g, rtol=2e-5)
    assert np.abs(Hh.estimate(num_c, den_c, win) - Hh.estimate(num_g, den_g, win)).max() < 2e-3


@pytest.mark.parametrize("pk", [(8, 8, 3, 16, 4, "bior", "sadct", "haar"), (4, 6, 2, 16, 4, "bior", "sadct", "haar"),
                                (2, 6, 2, 16, 4, "bior", "sadct", "haar"), (8, 8, 3, 16, 4, "dct", "sadct", "haar"),
                                (8, 8, 3, 16, 4, "bior", "sadct", "hw"), (1, 6, 2, 16, 3, "bior", "sadct", "haar"),
                                (1, 6, 2, 16, 3, "dct", "sadct", "haar")],
                         ids=["bior-n8", "bior-n4", "bior-n2", "dct-n8", "bior-n8-hadamard", "bior-n1", "dct-n1"])
def test_empty_sai_with_16x16_transform_kernels(ctx, pk):
    """The shape-adaptive angular transform inside the 16x16 kernels (k_group_bior16_haar since round 4: inline on LDS scratch between
    the two rounds of 2-D transforms; the others: the call form): an empty SAI makes every group shape-adaptive."""
    win, Wb, Hb, Cc = window(10.0, pk, 96)
    mask = np.ones(9, np.uint32)
    mask[5] = 0
    win[5] = 0
    proc = (1 - mask).astype(np.uint32)
    num_o, den_o, st = Hh.oracle_pass(1, 10.0, pk, win, None, Wb, Hb, Cc, mask=mask, proc=proc)
    ctx.reset_stats()
    num_g, den_g = gpu_pass(ctx, 1, 10.0, pk, win, None, Wb, Hb, Cc, mask=mask, proc=proc)
    s = ctx.stats()
    assert st.sadct_groups == st.groups and (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
    assert not den_g[5].any() and not num_g[5].any()
    assert np.array_equal(den_o != 0, den_g != 0)
    np.testing.assert_allclose(den_g, den_o, rtol=2e-5)
    assert np.abs(Hh.estimate(num_o, den_o, win) - Hh.estimate(num_g, den_g, win)).max() < 2e-2


@pytest.mark.parametrize("pk", [(16, 6, 2, 8, 3, "dct", "sadct", "haar"), (8, 6, 2, 8, 3, "dct", "sadct", "haar"), (4, 6, 2, 8, 3, "dct", "sadct", "hw")],
                         ids=["n16-haar", "n8-haar", "n4-hadamard"])
def test_empty_sai_wiener_window_matches_oracle(ctx, pk, monkeypatch):
    """A Wiener window with an empty SAI: every group takes the shape-adaptive angular transform -- since round 4 in kernels of
    their own (k_group_dct8w3<true>: the transform inline, in registers; the call form made such a pass 8x slower).  Both forms
    against the oracle, and against each other."""
    win, Wb, Hb, Cc = window(25.0, pk, 64)
    mask = np.ones(9, np.uint32)
    mask[6] = 0
    win[6] = 0
    proc = (1 - mask).astype(np.uint32)
    n1, d1, _ = Hh.oracle_pass(1, 25.0, (4,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc, mask=mask, proc=proc)
    basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    num_o, den_o, st = Hh.oracle_pass(2, 25.0, pk, win, basic, Wb, Hb, Cc, mask=mask, proc=proc)
    assert st.sadct_groups == st.groups
    res = []
    for call_form in (False, True):
        if call_form:
            monkeypatch.setenv("LFBM5D_NO_SA_KERNELS", "1")
        ctx.reset_stats()
        num_g, den_g = gpu_pass(ctx, 2, 25.0, pk, win, basic, Wb, Hb, Cc, mask=mask, proc=proc)
        s = ctx.stats()
        assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
        assert not den_g[6].any() and not num_g[6].any()
        np.testing.assert_allclose(den_g, den_o, rtol=2e-4)
        assert np.abs(Hh.estimate(num_o, den_o, win) - Hh.estimate(num_g, den_g, win)).max() < 2e-2
        res.append((num_g, den_g))
    monkeypatch.delenv("LFBM5D_NO_SA_KERNELS")
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=2e-5)
    assert np.abs(Hh.estimate(res[0][0], res[0][1], win) - Hh.estimate(res[1][0], res[1][1], win)).max() < 2e-3


def test_row_shards_sum_to_full_pass(ctx):
    pk = (8, 6, 2, 8, 3, "dct", "sadct", "haar")
    win, Wb, Hb, Cc = window(25.0, pk, 64)
    basic = np.ascontiguousarray((0.5 * win + 0.5 * np.roll(win, 1, axis=1)).astype(np.float32))
    full_n, full_d = gpu_pass(ctx, 2, 25.0, pk, win, basic, Wb, Hb, Cc)
    parts = []
    for r in range(3):
        ctx.set_shard(r, 3)   # ranks > 0 start from zeroed buffers inside the pass
        parts.append(gpu_pass(ctx, 2, 25.0, pk, win, basic, Wb, Hb, Cc))
    ctx.set_shard(0, 1)
    np.testing.assert_allclose(sum(p[0] for p in parts), full_n, rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(sum(p[1] for p in parts), full_d, rtol=1e-5, atol=1e-6)


def test_subset_pass_matches_oracle(ctx):
    """pst != cst (core:531-821): greyscale window, centre pass first, then a pass for another SAI that
    only takes the reference patches whose footprint still has a zero weight (den-aware list,
    utilities_LF.cpp:1031-1099), matched with the irregular-list block matching (core:3631-3945)."""
    pk = (4, 6, 2, 8, 4, "dct", "sadct", "haar")
    win, Wb, Hb, Cc = window(20.0, pk, 72, grey=True)
    num0, den0, st0 = Hh.oracle_pass(1, 20.0, pk, win, None, Wb, Hb, Cc)
    proc = np.zeros(9, np.uint32)
    proc[4] = 1
    for pst in (8, 1):
        num_o, den_o, st = Hh.oracle_pass(1, 20.0, pk, win, None, Wb, Hb, Cc, num=num0.copy(), den=den0.copy(), proc=proc, pst=pst)
        assert 0 < st.groups < st0.groups
        ctx.reset_stats()
        num_g, den_g = gpu_pass(ctx, 1, 20.0, pk, win, None, Wb, Hb, Cc, num=num0.copy(), den=den0.copy(), proc=proc, pst=pst)
        s = ctx.stats()
        assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
        assert np.array_equal(den_o != 0, den_g != 0)
        np.testing.assert_allclose(den_g, den_o, rtol=2e-5, atol=1e-7)
        assert np.abs(Hh.estimate(num_o, den_o, win) - Hh.estimate(num_g, den_g, win)).max() < 2e-3
        assert np.array_equal(num_g[4], num0[4])   # the processed centre SAI is not aggregated into again


@pytest.mark.parametrize("pk,sigma", [((8, 6, 2, 8, 4, "dct", "sadct", "haar"), 20.0), ((4, 5, 2, 12, 3, "dct", "sadct", "hw"), 50.0),
                                      ((8, 6, 1, 8, 3, "bior", "id", "haar"), 50.0)])
def test_subset_pass_of_the_wiener_step_matches_oracle(ctx, pk, sigma):
    """The same for step 2 (core:1332-1658): the pilot-driven matching on the irregular list, the den-aware list on the
    Wiener weights' den, two subset passes one after the other (the second sees the first one's sums)."""
    win, Wb, Hb, Cc = window(sigma, pk, 72, grey=True)
    n1, d1, _ = Hh.oracle_pass(1, sigma, (4,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc)
    basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    num_o, den_o, st0 = Hh.oracle_pass(2, sigma, pk, win, basic, Wb, Hb, Cc)
    num_g, den_g = gpu_pass(ctx, 2, sigma, pk, win, basic, Wb, Hb, Cc)
    assert np.array_equal(den_o != 0, den_g != 0)
    proc = np.zeros(9, np.uint32)
    proc[4] = 1
    for pst in (8, 1, 6):
        # both sides start from the SAME sums (the oracle's): block matching runs on num / den, and sums that differ in
        # the last bits re-order near-tied candidates now and then
        num_in, den_in = num_o.copy(), den_o.copy()
        num_o, den_o, st = Hh.oracle_pass(2, sigma, pk, win, basic, Wb, Hb, Cc, num=num_o, den=den_o, proc=proc.copy(), pst=pst)
        ctx.reset_stats()
        num_g, den_g = gpu_pass(ctx, 2, sigma, pk, win, basic, Wb, Hb, Cc, num=num_in, den=den_in, proc=proc.copy(), pst=pst)
        s = ctx.stats()
        assert st.groups < st0.groups
        assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups), pst
        assert np.array_equal(den_o != 0, den_g != 0), pst
        np.testing.assert_allclose(den_g, den_o, rtol=1e-4, atol=1e-7)
        assert np.abs(Hh.estimate(num_o, den_o, win) - Hh.estimate(num_g, den_g, win)).max() < 5e-3
        proc[pst] = 1


@pytest.mark.parametrize("tiles,grey", [(4, False), (8, False), (4, True), (8, True), (6, True)])   # 6: floored to 4 on both sides (main.cpp:101-102)
def test_tile_mode_matches_the_oracles_tile_mode(ctx, tiles, grey):
    """lfbm5d_set_tiles: the reference's OpenMP tile mode (bm5d.cpp:411-708; what run_bm5d_* does with nb_threads > 1) --
    tiles with a discarded halo.  Both steps against the oracle in the same mode: same windows and passes, PSNR within
    0.01 dB, and measurably different from the untiled result (the mode is there to reproduce tiled reference runs)."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    ah, aw, Hs, Ws = 3, 5, 112, 96
    lf = Hh.textured_lf(ah, aw, Hs, Ws)
    if grey:
        lf = np.ascontiguousarray(lf[:, :1])
    Cc = lf.shape[1]
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(ah * aw, np.uint32)
    p1, p2 = (4, 6, 2, 8, 4, "id", "sadct", "haar"), (8, 6, 2, 8, 4, "dct", "sadct", "haar")
    cs = "rgb" if grey else "opp"
    lib = O.lib()
    lib.orc_set_tiles(tiles)
    try:
        n1, b_o, st1 = O.run_step1(O.make_params(25.0, 2.7, *p1, cs=cs), noisy.copy(), mask, O.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
        w1 = O.last_windows()
        _, _, d_o, st2 = O.run_step2(O.make_params(25.0, 2.7, *p2, cs=cs), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
    finally:
        lib.orc_set_tiles(1)

    def gpu(nt):
        d_noisy = torch.from_numpy(noisy).cuda()
        d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
        ctx.set_tiles(nt)
        try:
            ctx.reset_stats()
            ctx.step1(core.make_params(25.0, 2.7, *p1, color_space=cs), d_noisy, mask, d_basic, L.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
            s1, wins = ctx.stats(), ctx.last_windows()
            ctx.reset_stats()
            ctx.step2(core.make_params(25.0, 2.7, *p2, color_space=cs), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
            s2 = ctx.stats()
        finally:
            ctx.set_tiles(1)
        return d_basic.cpu().numpy(), d_den.cpu().numpy(), s1, s2, wins

    b_g, d_g, s1, s2, wins = gpu(tiles)
    assert np.array_equal(wins, w1)
    assert (s1.windows, s1.passes) == (st1.windows, st1.passes) and s2.windows == st2.windows
    assert np.isfinite(b_g).all() and np.isfinite(d_g).all()
    assert abs(O.psnr_lf(b_g, clean) - O.psnr_lf(b_o, clean)) < 0.01
    assert abs(O.psnr_lf(d_g, clean) - O.psnr_lf(d_o, clean)) < 0.01
    if not grey:
        b_u, d_u, *_ = gpu(1)
        assert O.psnr_lf(d_u, clean) > O.psnr_lf(d_g, clean) + 0.05      # the halo discard costs quality
        assert np.abs(b_u - b_g).max() > 1.0


def test_greyscale_light_field_whole_steps(ctx):
    """C == 1: windows are not finished by their centre pass, the subset path runs."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    lf = Hh.source_lf(crop=96)[:, :1]
    clean, noisy = Hh.noisy_lf(lf, 20.0)
    mask = np.ones(9, np.uint32)
    p1 = (4, 6, 2, 8, 4, "dct", "sadct", "haar")
    p2 = (8, 6, 2, 8, 4, "dct", "sadct", "haar")
    n1, b_o, st1 = O.run_step1(O.make_params(20.0, 2.7, *p1, cs="rgb"), noisy.copy(), mask, O.ROWMAJOR, 3, 3, 1, 96, 96, 1)
    n2, b2, d_o, st2 = O.run_step2(O.make_params(20.0, 2.7, *p2, cs="rgb"), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, 3, 3, 1, 96, 96, 1)
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
    ctx.reset_stats()
    ctx.step1(core.make_params(20.0, 2.7, *p1, color_space="rgb"), d_noisy, mask, d_basic, L.ROWMAJOR, 3, 3, 1, 96, 96, 1)
    s = ctx.stats()
    assert s.passes == st1.passes and s.passes > 1
    assert abs(O.psnr_lf(d_basic.cpu().numpy(), clean) - O.psnr_lf(b_o, clean)) < 0.01
    ctx.step2(core.make_params(20.0, 2.7, *p2, color_space="rgb"), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 3, 3, 1, 96, 96, 1)
    assert abs(O.psnr_lf(d_den.cpu().numpy(), clean) - O.psnr_lf(d_o, clean)) < 0.01


def test_greyscale_multi_window_steps(ctx):
    """Greyscale 5x5 light field (five windows, every window visits its SAIs through the subset path): window sequence of
    both steps, pass count of step 1 and the basic estimate at the north-star bar; step 2 is allowed to end a window's
    subset passes one or two passes earlier or later than the oracle (the lists depend on exact zeros of running sums
    that differ in the last bits) -- where the counts agree the bar is 0.01 dB, else 0.05 dB."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    lf = np.ascontiguousarray(Hh.textured_lf(5, 5, 64, 64)[:, :1])
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(25, np.uint32)
    p1 = (4, 5, 2, 8, 4, "dct", "sadct", "haar")
    p2 = (8, 5, 2, 8, 4, "dct", "sadct", "haar")
    n1, b_o, st1 = O.run_step1(O.make_params(25.0, 2.7, *p1, cs="rgb"), noisy.copy(), mask, O.ROWMAJOR, 5, 5, 1, 64, 64, 1)
    w1_o = O.last_windows()
    _, _, d_o, st2 = O.run_step2(O.make_params(25.0, 2.7, *p2, cs="rgb"), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, 5, 5, 1, 64, 64, 1)
    w2_o = O.last_windows()
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
    ctx.reset_stats()
    ctx.step1(core.make_params(25.0, 2.7, *p1, color_space="rgb"), d_noisy, mask, d_basic, L.ROWMAJOR, 5, 5, 1, 64, 64, 1)
    s1 = ctx.stats()
    assert np.array_equal(ctx.last_windows(), w1_o) and len(w1_o) == 5
    assert s1.passes == st1.passes and s1.passes > s1.windows
    assert abs(O.psnr_lf(d_basic.cpu().numpy(), clean) - O.psnr_lf(b_o, clean)) < 0.01
    ctx.reset_stats()
    ctx.step2(core.make_params(25.0, 2.7, *p2, color_space="rgb"), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 5, 5, 1, 64, 64, 1)
    s2 = ctx.stats()
    assert np.array_equal(ctx.last_windows(), w2_o)
    assert abs(int(s2.passes) - int(st2.passes)) <= 2 * len(w2_o)
    bar = 0.01 if s2.passes == st2.passes else 0.05
    assert abs(O.psnr_lf(d_den.cpu().numpy(), clean) - O.psnr_lf(d_o, clean)) < bar


def test_greyscale_steps_with_a_5x5_window(ctx):
    """The same light field as ONE 5x5 window (aswSize 2): the centre pass and the subset passes of the other 24 SAIs through the
    wide-window kernel (step 1: tau_2D = id) and the slab kernel (step 2: 2 x 8 x 25 x 64 floats per stack pair)."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    lf = np.ascontiguousarray(Hh.textured_lf(5, 5, 64, 64)[:, :1])
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(25, np.uint32)
    p1 = (4, 5, 2, 8, 4, "id", "sadct", "haar")
    p2 = (8, 5, 2, 8, 4, "dct", "sadct", "haar")
    n1, b_o, st1 = O.run_step1(O.make_params(25.0, 2.7, *p1, cs="rgb"), noisy.copy(), mask, O.ROWMAJOR, 5, 5, 2, 64, 64, 1)
    w1_o = O.last_windows()
    _, _, d_o, st2 = O.run_step2(O.make_params(25.0, 2.7, *p2, cs="rgb"), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, 5, 5, 2, 64, 64, 1)
    w2_o = O.last_windows()
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
    ctx.reset_stats()
    ctx.step1(core.make_params(25.0, 2.7, *p1, color_space="rgb"), d_noisy, mask, d_basic, L.ROWMAJOR, 5, 5, 2, 64, 64, 1)
    s1 = ctx.stats()
    assert np.array_equal(ctx.last_windows(), w1_o)
    assert abs(int(s1.passes) - int(st1.passes)) <= 2 * len(w1_o) and s1.passes > s1.windows
    assert abs(O.psnr_lf(d_basic.cpu().numpy(), clean) - O.psnr_lf(b_o, clean)) < (0.01 if s1.passes == st1.passes else 0.05)
    ctx.reset_stats()
    ctx.step2(core.make_params(25.0, 2.7, *p2, color_space="rgb"), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 5, 5, 2, 64, 64, 1)
    s2 = ctx.stats()
    assert np.array_equal(ctx.last_windows(), w2_o)
    assert abs(int(s2.passes) - int(st2.passes)) <= 2 * len(w2_o)
    assert abs(O.psnr_lf(d_den.cpu().numpy(), clean) - O.psnr_lf(d_o, clean)) < (0.01 if s2.passes == st2.passes else 0.05)


def test_subset_passes_on_the_full_grid_scan_equal_the_position_map_form(ctx, monkeypatch):
    """Round 4: the subset passes of a greyscale light field run the second-generation table kernel on the full regular grid and
    take a reference's scores from its place in it (before: round 2's kernel with a position map, LFBM5D_SUBSET_SCAN_V1=1).  Same
    tables, same selections: both steps bit-identical, pass for pass."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    lf = np.ascontiguousarray(Hh.textured_lf(5, 5, 72, 64)[:, :1])
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(25, np.uint32)
    mask[3] = 0
    P1 = core.make_params(25.0, 2.7, 4, 5, 2, 8, 4, "dct", "sadct", "haar", color_space="rgb")
    P2 = core.make_params(25.0, 2.7, 8, 5, 2, 8, 3, "dct", "sadct", "haar", color_space="rgb")
    res = []
    for v1 in (False, True, None):
        if v1:
            monkeypatch.setenv("LFBM5D_SUBSET_SCAN_V1", "1")
        elif v1 is None:   # ... and the passes' reference lists built on the host (rounds 1-3) instead of on the device
            monkeypatch.delenv("LFBM5D_SUBSET_SCAN_V1")
            monkeypatch.setenv("LFBM5D_SUBSET_LIST_HOST", "1")
        d_noisy = torch.from_numpy(noisy).cuda()
        d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
        ctx.reset_stats()
        ctx.step1(P1, d_noisy, mask, d_basic, L.ROWMAJOR, 5, 5, 1, 64, 72, 1)
        ctx.step2(P2, d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 5, 5, 1, 64, 72, 1)
        s = ctx.stats()
        res.append((d_basic.cpu().numpy(), d_den.cpu().numpy(), int(s.passes), int(s.groups)))
    for r in res[1:]:
        assert res[0][2] == r[2] > 10 and res[0][3] == r[3]
        assert np.array_equal(res[0][0], r[0]) and np.array_equal(res[0][1], r[1])
    assert O.psnr_lf(res[0][1][mask != 0], clean[mask != 0]) > O.psnr_lf(noisy[mask != 0], clean[mask != 0]) + 5


E2E = {
    "readme": (25.0, Hh.README_HT, Hh.README_WIEN),
    "config4": (10.0, Hh.C4_HT, Hh.README_WIEN),
    "config5": (50.0, Hh.C5_HT, Hh.C5_WIEN),
}


@pytest.mark.parametrize("name", sorted(E2E))
def test_whole_steps_match_oracle_psnr(ctx, name):
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    sigma, p1, p2 = E2E[name]
    clean, noisy = Hh.noisy_lf(Hh.source_lf(), sigma)
    mask = np.ones(9, np.uint32)
    n1, b_o, _ = O.run_step1(O.make_params(sigma, 2.7, *p1), noisy.copy(), mask, O.ROWMAJOR, 3, 3, 1, 256, 256, 3)
    n2, b2_o, d_o, _ = O.run_step2(O.make_params(sigma, 2.7, *p2), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, 3, 3, 1, 256, 256, 3)
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic = torch.zeros_like(d_noisy)
    d_den = torch.zeros_like(d_noisy)
    torch.cuda.synchronize()
    ctx.step1(core.make_params(sigma, 2.7, *p1), d_noisy, mask, d_basic, L.ROWMAJOR, 3, 3, 1, 256, 256, 3)
    b_g = d_basic.cpu().numpy()
    n1_g = d_noisy.cpu().numpy()
    assert np.abs(b_g - b_o).max() < 2e-3                       # step 1 on identical inputs
    assert np.abs(n1_g - n1).max() < 1e-4                        # same in-place drift of LF_noisy (quirk 5)
    assert abs(O.psnr_lf(b_g, clean) - O.psnr_lf(b_o, clean)) < 1e-4
    # step 2 fed with the oracle's step-1 outputs: isolates the Wiener path
    d_noisy.copy_(torch.from_numpy(n1))
    d_basic.copy_(torch.from_numpy(b_o))
    torch.cuda.synchronize()
    ctx.step2(core.make_params(sigma, 2.7, *p2), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 3, 3, 1, 256, 256, 3)
    assert np.abs(d_den.cpu().numpy() - d_o).max() < 5e-3
    assert np.abs(d_basic.cpu().numpy() - b2_o).max() < 1e-3   # LF_basic mutated in place like the reference
    # the chained GPU run (its own step-1 output feeds step 2): north-star bar, +-0.01 dB
    d_noisy.copy_(torch.from_numpy(n1_g))
    d_basic.copy_(torch.from_numpy(b_g))
    torch.cuda.synchronize()
    ctx.step2(core.make_params(sigma, 2.7, *p2), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 3, 3, 1, 256, 256, 3)
    assert abs(O.psnr_lf(d_den.cpu().numpy(), clean) - O.psnr_lf(d_o, clean)) < 0.01


def test_reference_named_wrappers_on_host_buffers(ctx):
    """run_bm5d_1st_step / run_bm5d_2nd_step with the reference's argument list, numpy buffers."""
    import lfbm5d_amd as L
    clean, noisy = Hh.noisy_lf(Hh.source_lf(crop=96), 25.0)
    mask = np.ones(9, np.uint32)
    P1 = O.make_params(25.0, 2.7, 4, 8, 3, 8, 4, "bior", "sadct", "haar")
    n1, b_o, _ = O.run_step1(P1, noisy.copy(), mask, O.ROWMAJOR, 3, 3, 1, 96, 96, 3)
    h_noisy, h_basic = noisy.copy(), np.zeros_like(noisy)
    assert L.run_bm5d_1st_step(25.0, 2.7, h_noisy, mask, h_basic, L.ROWMAJOR, 3, 3, 1, 96, 96, 3, 4, 8, 3, 8, 4,
                               False, L.BIOR, L.SADCT, L.HAAR, L.OPP, 1, ctx=ctx) == 0
    assert np.abs(h_basic - b_o).max() < 2e-3 and np.abs(h_noisy - n1).max() < 1e-4
    h_den = np.zeros_like(noisy)
    P2 = O.make_params(25.0, 2.7, 8, 8, 3, 8, 4, "dct", "sadct", "haar")
    n2, b2, d_o, _ = O.run_step2(P2, n1.copy(), b_o.copy(), mask, O.ROWMAJOR, 3, 3, 1, 96, 96, 3)
    h_n, h_b = n1.copy(), b_o.copy()
    assert L.run_bm5d_2nd_step(25.0, h_n, mask, h_b, h_den, L.ROWMAJOR, 3, 3, 1, 96, 96, 3, 8, 8, 3, 8, 4, False,
                               L.DCT, L.SADCT, L.HAAR, L.OPP, 1, ctx=ctx) == 0
    assert np.abs(h_den - d_o).max() < 5e-3


def _steps_vs_oracle(ctx, lf, ah, aw, Hs, Ws, p1, p2, major_o, major_g, sigma=25.0, mask=None):
    """Both whole steps on a multi-window light field, GPU (planned windows on lanes) against the oracle (the
    reference's data-driven window choice): identical window sequences, PSNR of both steps within 0.01 dB."""
    from lfbm5d_amd import core
    clean, noisy = Hh.noisy_lf(lf, sigma)
    mask = np.ones(ah * aw, np.uint32) if mask is None else mask
    n1, b_o, st1 = O.run_step1(O.make_params(sigma, 2.7, *p1), noisy.copy(), mask, major_o, aw, ah, 1, Ws, Hs, 3)
    w1_o = O.last_windows()
    n2, _, d_o, st2 = O.run_step2(O.make_params(sigma, 2.7, *p2), n1.copy(), b_o.copy(), mask, major_o, aw, ah, 1, Ws, Hs, 3)
    w2_o = O.last_windows()
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
    ctx.reset_stats()
    ctx.step1(core.make_params(sigma, 2.7, *p1), d_noisy, mask, d_basic, major_g, aw, ah, 1, Ws, Hs, 3)
    w1_g, s1 = ctx.last_windows(), ctx.stats()
    b_g = d_basic.cpu().numpy()
    ctx.reset_stats()
    ctx.step2(core.make_params(sigma, 2.7, *p2), d_noisy, mask, d_basic, d_den, major_g, aw, ah, 1, Ws, Hs, 3)
    w2_g, s2 = ctx.last_windows(), ctx.stats()
    d_g = d_den.cpu().numpy()
    assert np.array_equal(w1_g, w1_o) and np.array_equal(w2_g, w2_o)
    assert (s1.windows, s1.passes) == (st1.windows, st1.passes) and (s2.windows, s2.passes) == (st2.windows, st2.passes)
    m = mask != 0
    pb_g, pb_o = O.psnr_lf(b_g[m], clean[m]), O.psnr_lf(b_o[m], clean[m])
    pd_g, pd_o = O.psnr_lf(d_g[m], clean[m]), O.psnr_lf(d_o[m], clean[m])
    assert abs(pb_g - pb_o) < 0.01, (pb_g, pb_o)          # north-star bar, multi-window
    assert abs(pd_g - pd_o) < 0.01, (pd_g, pd_o)
    assert pd_g > O.psnr_lf(noisy[m], clean[m]) + 6
    return dict(basic=(pb_g, pb_o), denoised=(pd_g, pd_o), max_basic=float(np.abs(b_g - b_o).max()), windows=len(w1_g))


@pytest.mark.parametrize("major", ["row", "col"])
def test_window_schedule_5x5_matches_oracle(ctx, major):
    """2^2+1 windows on a 5x5 light field, both angular orderings: same windows as the oracle's
    data-driven choice, whole-step PSNR within 0.01 dB (bm5d.cpp:179-402)."""
    import lfbm5d_amd as L
    # 96x96 SAIs: from the second window on, block matching runs on a running estimate that differs from the oracle's
    # by float round-off (1e-4 grey levels), which re-orders near-tied candidates in a few groups per hundred; the
    # PSNR of a light field this small then moves by some 0.001 dB per flipped group
    lf = Hh.textured_lf(5, 5, 96, 96)
    if major == "col":   # column-major: SAI index st = s + t * aheight
        lf = np.ascontiguousarray(lf.reshape(5, 5, 3, 96, 96).transpose(1, 0, 2, 3, 4)).reshape(25, 3, 96, 96)
    r = _steps_vs_oracle(ctx, lf, 5, 5, 96, 96, (4, 6, 2, 8, 4, "id", "sadct", "haar"), (8, 6, 2, 8, 4, "dct", "sadct", "haar"),
                         O.ROWMAJOR if major == "row" else O.COLMAJOR, L.ROWMAJOR if major == "row" else L.COLMAJOR)
    assert r["windows"] == 5


def test_multi_window_steps_5x7_match_oracle(ctx):
    """Non-square angular grid, README-style parameters with 16x16 HT patches: windows and PSNR against the oracle."""
    import lfbm5d_amd as L
    lf = Hh.textured_lf(5, 7, 80, 72)
    _steps_vs_oracle(ctx, lf, 5, 7, 80, 72, (8, 8, 3, 16, 4, "id", "sadct", "haar"), (16, 8, 3, 8, 4, "dct", "sadct", "haar"),
                     O.ROWMAJOR, L.ROWMAJOR)


def test_headline_schedule_17x17_matches_oracle(ctx):
    """The benchmark's angular grid (17x17, 64 windows per step, three lanes) at 96x96 pixels: the planned sequence
    equals the oracle's data-driven one window for window and both steps stay within 0.01 dB of the oracle."""
    import lfbm5d_amd as L
    lf = Hh.textured_lf(17, 17, 96, 96)
    r = _steps_vs_oracle(ctx, lf, 17, 17, 96, 96, (8, 10, 3, 16, 4, "id", "sadct", "haar"), (16, 10, 3, 8, 4, "dct", "sadct", "haar"),
                         O.ROWMAJOR, L.ROWMAJOR)
    assert r["windows"] == 64


def test_multi_window_steps_with_empty_sais_match_oracle(ctx):
    """Empty SAIs: the DCT -> SADCT switch is sticky across windows (bm5d.cpp:276-280) and windows are chosen around
    the holes; against the oracle."""
    import lfbm5d_amd as L
    lf = Hh.textured_lf(5, 5, 64, 64)
    mask = np.ones(25, np.uint32)
    mask[[3, 9, 20]] = 0
    _steps_vs_oracle(ctx, lf, 5, 5, 64, 64, (4, 6, 2, 8, 4, "id", "dct", "haar"), (8, 6, 2, 8, 4, "dct", "dct", "haar"),
                     O.ROWMAJOR, L.ROWMAJOR, mask=mask)


def test_multi_rank_graph_played_on_one_gpu_is_bit_identical(ctx, monkeypatch):
    """The multi-GPU step scheme with all ranks played on this GPU (LFBM5D_EMULATE_WORLD): every rank keeps num / den
    of its own, runs the chains of windows the graph gives it and receives the SAIs it needs from other ranks' windows
    as messages (device copies here, RCCL send / recv between real ranks).  The planned sequence is the reference's
    data-driven one, and 2 / 3 / 4 / 8 ranks reproduce the single-rank result BIT FOR BIT.  The opt-in window blocks
    of round 1 (one all-reduce per step) are checked to be what their documentation says: close, not identical."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    ah, aw, Hh_, Ww = 7, 9, 64, 64
    lf = Hh.textured_lf(ah, aw, Hh_, Ww)
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(ah * aw, np.uint32)
    P1 = core.make_params(25.0, 2.7, 4, 6, 2, 8, 4, "id", "sadct", "haar")
    P2 = core.make_params(25.0, 2.7, 8, 6, 2, 8, 4, "dct", "sadct", "haar")

    def run():
        d_noisy = torch.from_numpy(noisy).cuda()
        d_basic = torch.zeros_like(d_noisy)
        d_den = torch.zeros_like(d_noisy)
        ctx.reset_stats()
        ctx.step1(P1, d_noisy, mask, d_basic, L.ROWMAJOR, aw, ah, 1, Ww, Hh_, 3)
        w = ctx.last_windows()
        ctx.step2(P2, d_noisy, mask, d_basic, d_den, L.ROWMAJOR, aw, ah, 1, Ww, Hh_, 3)
        return d_basic.cpu().numpy(), d_den.cpu().numpy(), w, ctx.stats()

    for k in ("LFBM5D_EMULATE_WORLD", "LFBM5D_DATA_DRIVEN_SCHEDULE", "LFBM5D_STEP_SHARDING", "LFBM5D_LANES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LFBM5D_DATA_DRIVEN_SCHEDULE", "1")     # the reference's selection from zero-weight counts
    b0, d0, w0, _ = run()
    monkeypatch.delenv("LFBM5D_DATA_DRIVEN_SCHEDULE")
    plan = core.plan_windows(aw, ah, 1, L.ROWMAJOR)
    assert np.array_equal(plan, w0) and w0[0] == (ah // 2) * aw + aw // 2
    b1, d1, w1, s1 = run()                                        # default: the planned sequence on three lanes
    assert np.array_equal(w1, w0) and np.array_equal(b1, b0) and np.array_equal(d1, d0) and s1.messages == 0
    for n in (2, 3, 4, 8):
        monkeypatch.setenv("LFBM5D_EMULATE_WORLD", str(n))
        b, d, w, st = run()
        ranks, _, _ = core.plan_graph(aw, ah, n)
        msgs = core.plan_messages(aw, ah, n)
        assert np.array_equal(w, w0) and st.windows == 2 * len(w0) and st.messages == 2 * len(msgs) > 0
        assert len(set(ranks.tolist())) > 1                        # several ranks really own windows
        assert np.array_equal(b, b0) and np.array_equal(d, d0), n
    # round 1's window blocks: one all-reduce per step, a rank's matching only sees its own earlier windows
    monkeypatch.setenv("LFBM5D_STEP_SHARDING", "blocks")
    p0 = O.psnr_lf(d0, clean)
    for n in (2, 4):
        monkeypatch.setenv("LFBM5D_EMULATE_WORLD", str(n))
        b, d, w, _ = run()
        assert sorted(w.tolist()) == sorted(w0.tolist()) and not np.array_equal(d, d0)
        assert abs(O.psnr_lf(d, clean) - p0) < 0.5
    monkeypatch.delenv("LFBM5D_EMULATE_WORLD")
    monkeypatch.delenv("LFBM5D_STEP_SHARDING")


@pytest.mark.parametrize("holes", [False, True], ids=["full", "empty-sais"])
def test_window_lanes_are_bit_identical_to_the_sequential_order(ctx, monkeypatch, holes):
    """Pipelined steps (several windows in flight on lanes, dependencies = shared SAIs) against the window-after-window
    order: same windows, same bits, with and without empty SAIs (sticky DCT -> SADCT switch, bm5d.cpp:276-280)."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    ah, aw, Hs, Ws = 7, 9, 64, 64
    lf = Hh.textured_lf(ah, aw, Hs, Ws)
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(ah * aw, np.uint32)
    if holes:
        mask[[0, 11, 40, 62]] = 0
    P1 = core.make_params(25.0, 2.7, 4, 6, 2, 8, 4, "id", "dct", "haar")
    P2 = core.make_params(25.0, 2.7, 8, 6, 2, 8, 4, "dct", "dct", "haar")

    def run():
        d_noisy = torch.from_numpy(noisy).cuda()
        d_basic = torch.zeros_like(d_noisy)
        d_den = torch.zeros_like(d_noisy)
        ctx.reset_stats()
        ctx.step1(P1, d_noisy, mask, d_basic, L.ROWMAJOR, aw, ah, 1, Ws, Hs, 3)
        w = ctx.last_windows()
        ctx.step2(P2, d_noisy, mask, d_basic, d_den, L.ROWMAJOR, aw, ah, 1, Ws, Hs, 3)
        return d_basic.cpu().numpy(), d_den.cpu().numpy(), w, ctx.stats()

    for k in ("LFBM5D_EMULATE_WORLD", "LFBM5D_DATA_DRIVEN_SCHEDULE", "LFBM5D_STEP_SHARDING"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LFBM5D_LANES", "1")
    b0, d0, w0, s0 = run()
    assert s0.lane_windows == 0 and s0.windows == 2 * len(w0)
    for lanes in ("2", "3", "4"):
        monkeypatch.setenv("LFBM5D_LANES", lanes)
        b1, d1, w1, s1 = run()
        assert np.array_equal(w1, w0) and (s1.windows, s1.passes, s1.groups) == (s0.windows, s0.passes, s0.groups)
        assert s1.lane_windows > 0                                  # other lanes really took windows
        assert np.array_equal(b1, b0) and np.array_equal(d1, d0)
    assert O.psnr_lf(d0[mask != 0], clean[mask != 0]) > O.psnr_lf(noisy[mask != 0], clean[mask != 0]) + 6


# ------------------------------------------------------------------------------------------------
# 5x5 angular windows (aswSize 2; bm5d.cpp:215-218, utilities_LF.cpp:881-901, core:1862-2264 with awidth = aheight = 5)
# ------------------------------------------------------------------------------------------------
ASW2_CASES = [
    # name, step, params, crop, empty SAIs of the window
    ("ht-id-sadct-haar", 1, (4, 6, 2, 8, 4, "id", "sadct", "haar"), 64, ()),
    ("ht-id-dct-haar", 1, (4, 6, 2, 8, 4, "id", "dct", "haar"), 64, ()),
    ("ht-dct-sadct-hw-holes", 1, (8, 6, 2, 8, 4, "dct", "sadct", "hw"), 64, (0, 7, 18)),
    ("wien-dct-sadct-haar", 2, (8, 6, 2, 8, 4, "dct", "sadct", "haar"), 64, ()),
    ("wien-bior-dct-haar-holes", 2, (4, 6, 2, 8, 4, "bior", "dct", "haar"), 64, (3, 24)),
    # 16x16 patches, N = 8: 8 x 25 x 256 floats = 200 KiB per stack -> the HBM-scratch form of the generic kernel
    ("ht-bior-sadct-haar-k16", 1, (8, 6, 2, 16, 4, "bior", "sadct", "haar"), 72, ()),
    ("wien-dct-sadct-haar-n16", 2, (16, 6, 2, 8, 4, "dct", "sadct", "haar"), 64, ()),
    # the README's HT parameters on a wide window: the slab kernel of lfbm5d_group_wide.hip (round 5)
    ("ht-id-sadct-haar-k16-n8", 1, (8, 6, 2, 16, 4, "id", "sadct", "haar"), 72, ()),
    ("ht-id-sadct-hw-k12-holes", 1, (4, 6, 2, 12, 4, "id", "sadct", "hw"), 64, (2, 20)),
    ("ht-id-sadct-haar-k10", 1, (4, 6, 2, 10, 4, "id", "sadct", "haar"), 64, ()),        # a side that is no multiple of four: one pixel per load
    ("ht-id-dct-haar-k6-holes", 1, (8, 6, 2, 6, 3, "id", "sadct", "haar"), 56, (5, 23)),
]


def _wide_window_pass(ctx, case, aw, Cc=3):
    name, step, pk, crop, holes = case
    sigma = 25.0
    A, cc = aw * aw, (aw * aw) // 2
    lf = Hh.textured_lf(aw, aw, crop, crop)[:, :Cc]
    _, noisy = Hh.noisy_lf(lf, sigma)
    N, nSim, nDisp, k = pk[0], pk[1], pk[2], pk[3]
    win, Wb, Hb = Hh.padded_window(noisy, crop, crop, Cc, nSim + nDisp)
    mask = np.ones(A, np.uint32)
    for h in holes:
        mask[h] = 0
        win[h] = 0
    proc = (mask == 0).astype(np.uint32)      # the schedule marks empty SAIs as processed (bm5d.cpp:268-270)
    basic = None
    if step == 2:
        n1, d1, _ = Hh.oracle_pass(1, sigma, (4,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc, mask=mask, proc=proc, cst=cc, pst=cc, aw=aw)
        basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    num_o, den_o, st = Hh.oracle_pass(step, sigma, pk, win, basic, Wb, Hb, Cc, mask=mask, proc=proc, cst=cc, pst=cc, aw=aw)
    ctx.reset_stats()
    num_g, den_g = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc, mask=mask, proc=proc, cst=cc, pst=cc, aw=aw)
    s = ctx.stats()
    assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
    if holes:
        assert st.sadct_groups == st.groups or pk[6] in ("dct", "id")
    refs, idx, cnt, best, shape = ctx.last_bm(N, A, Wb * Hb)
    est = (win if step == 1 else basic)[:, :Wb * Hb]
    tau = Hh.tau_match(sigma, Cc, step)
    regr, regc = slice(nDisp, Hb - k - nDisp + 1), slice(nDisp, Wb - k - nDisp + 1)
    for st_i in (0, aw + 1, cc + 1, A - 1):
        if not mask[st_i]:
            continue
        ob, osh = np.zeros(Wb * Hb, np.uint32), np.zeros(Wb * Hb, np.uint8)
        O.lib().orc_bm_stereo(np.ascontiguousarray(est[cc]), np.ascontiguousarray(est[st_i]), Wb, Hb, k, nDisp, tau, ob, osh)
        assert np.array_equal(ob.reshape(Hb, Wb)[regr, regc], best[st_i].reshape(Hb, Wb)[regr, regc])
        assert np.array_equal(osh.reshape(Hb, Wb)[regr, regc], shape[st_i].reshape(Hb, Wb)[regr, regc])
    assert np.array_equal(den_o != 0, den_g != 0)
    np.testing.assert_allclose(den_g, den_o, rtol=1e-4, atol=1e-6)
    eo, eg = Hh.estimate(num_o, den_o, win), Hh.estimate(num_g, den_g, win)
    assert np.abs(eo - eg).max() < 3e-3


@pytest.mark.parametrize("case", ASW2_CASES, ids=[c[0] for c in ASW2_CASES])
def test_5x5_window_pass_matches_oracle(ctx, case):
    """One core pass on a 5x5 angular window (25 SAIs, 24 disparity searches, general 5x5 angular DCT / SADCT):
    identical block matching, coverage and group statistics, estimate within the float tolerance of a 3x3 pass."""
    _wide_window_pass(ctx, case, 5)


# 7x7 angular windows (aswSize 3): 49 SAIs, 48 disparity searches, 7-point angular DCT / SADCT rows and columns
ASW3_CASES = [
    ("ht-id-sadct-haar-holes", 1, (4, 5, 2, 8, 4, "id", "sadct", "haar"), 56, (0, 10, 30, 48)),
    ("ht-dct-dct-hw", 1, (8, 5, 2, 8, 4, "dct", "dct", "hw"), 56, ()),
    ("wien-dct-sadct-haar", 2, (8, 5, 2, 8, 4, "dct", "sadct", "haar"), 56, ()),
    ("wien-bior-sadct-dct5-holes", 2, (4, 5, 2, 8, 4, "bior", "sadct", "dct"), 56, (8, 40)),
    ("ht-id-dct-haar-k12-n4", 1, (4, 5, 2, 12, 4, "id", "dct", "haar"), 64, ()),
    ("ht-id-sadct-haar-k16-n8", 1, (8, 5, 2, 16, 4, "id", "sadct", "haar"), 64, ()),
]


@pytest.mark.parametrize("case", ASW3_CASES, ids=[c[0] for c in ASW3_CASES])
def test_7x7_window_pass_matches_oracle(ctx, case):
    """aswSize 3: one core pass on a 7x7 angular window against the oracle."""
    _wide_window_pass(ctx, case, 7)


# 9x9 and 11x11 angular windows (aswSize 4, 5; round 5): the general forms -- run-time transform sizes, vectors in scratch memory,
# stacks in HBM -- for every window the reference takes on light fields of up to 17x17 SAIs (bm5d.cpp:119-124, :215-218)
ASW4_CASES = [
    ("ht-id-sadct-haar", 1, (4, 5, 2, 8, 4, "id", "sadct", "haar"), 48, ()),
    ("ht-dct-dct-hw-holes", 1, (4, 5, 2, 8, 4, "dct", "dct", "hw"), 48, (0, 13, 41, 80)),
    ("ht-bior-sadct-haar-holes", 1, (2, 5, 2, 8, 4, "bior", "sadct", "haar"), 48, (5, 44, 77)),
    ("wien-dct-sadct-haar", 2, (4, 5, 2, 8, 4, "dct", "sadct", "haar"), 48, ()),
    # round 6 (advisor): the slab kernel's largest request on a 9x9 window -- 2 x 32 x 81 x 4 pixels = 81 KB of LDS, above the
    # 80 KB its instances of windows up to 9x9 were capped at (the launch failed instead of falling back)
    ("wien-dct-sadct-haar-n32", 2, (32, 5, 2, 8, 4, "dct", "sadct", "haar"), 48, ()),
]


@pytest.mark.parametrize("case", ASW4_CASES, ids=[c[0] for c in ASW4_CASES])
def test_9x9_window_pass_matches_oracle(ctx, case):
    """aswSize 4: one core pass on a 9x9 angular window (81 SAIs, 80 disparity searches) against the oracle."""
    _wide_window_pass(ctx, case, 9)


def test_11x11_window_pass_matches_oracle(ctx):
    _wide_window_pass(ctx, ("ht-id-sadct-haar-holes", 1, (2, 4, 2, 8, 4, "id", "sadct", "haar"), 40, (7, 61, 120)), 11)
    _wide_window_pass(ctx, ("wien-dct-dct-haar", 2, (2, 4, 2, 8, 4, "dct", "dct", "haar"), 40, ()), 11)


def test_greyscale_wide_window_passes_match_oracle(ctx):
    """One channel through the wide-window and slab kernels (their grids and the `filt` layout carry the channel count)."""
    _wide_window_pass(ctx, ("grey-ht-id-sadct-haar-k16-n8", 1, (8, 6, 2, 16, 4, "id", "sadct", "haar"), 72, (3,)), 5, Cc=1)
    _wide_window_pass(ctx, ("grey-wien-dct-sadct-haar-n16", 2, (16, 6, 2, 8, 4, "dct", "sadct", "haar"), 64, ()), 5, Cc=1)
    _wide_window_pass(ctx, ("grey-ht-bior-dct-hw-k16", 1, (4, 5, 2, 16, 4, "bior", "dct", "hw"), 64, ()), 7, Cc=1)


@pytest.mark.parametrize("aw", [13, 17])
def test_largest_window_passes_match_oracle(ctx, aw):
    """aswSize 6 and 8 (13x13, 17x17: the whole light field of the headline as ONE window): the wide-window kernel (HT, tau_2D = id)
    and the slab kernel (2-D transform) at their smallest slabs, with empty SAIs -- shape-adaptive passes on the large shape record."""
    A = aw * aw
    _wide_window_pass(ctx, ("ht-id-sadct-haar-holes", 1, (2, 4, 2, 8, 4, "id", "sadct", "haar"), 40, (3, A // 2 + 1, A - 1)), aw)
    _wide_window_pass(ctx, ("ht-bior-sadct-hw", 1, (4, 4, 2, 8, 4, "bior", "sadct", "hw"), 40, ()), aw)
    _wide_window_pass(ctx, ("wien-dct-sadct-haar-holes", 2, (2, 4, 2, 8, 4, "dct", "sadct", "haar"), 40, (0, A - 2)), aw)
    if aw == 13:   # the README's N = 16 in the Wiener step: 2 x 16 x 169 values per coefficient -- the slab kernel's 112 KB tier (four coefficients per slab)
        _wide_window_pass(ctx, ("wien-dct-sadct-haar-n16", 2, (16, 4, 2, 8, 4, "dct", "sadct", "haar"), 40, ()), aw)
    else:          # round 6: the same on 17 x 17 -- 2 x 16 x 289 values per coefficient, slabs of TWO coefficients (74 KB); rounds 4-5 ran it on the general kernel
        _wide_window_pass(ctx, ("wien-dct-sadct-haar-n16", 2, (16, 4, 2, 8, 4, "dct", "sadct", "haar"), 40, ()), aw)
        _wide_window_pass(ctx, ("wien-id-dct-haar-n16-holes", 2, (16, 4, 2, 8, 4, "id", "dct", "haar"), 40, (1, A - 3)), aw)


def test_filt_layouts_of_wide_windows_agree_bit_for_bit(ctx, monkeypatch):
    """Round 6: windows of 11 x 11 SAIs and more keep their filtered patches SAI-major (lfbm5d_kernels.h filt_patch); option
    filt_group_major = the layout of the 3 x 3 windows.  Same patches, same order of additions: identical num / den, for the
    wide-window kernel (HT, tau_2D = id), the slab kernel (Wiener) and a pass cut into bands of reference rows."""
    aw, crop, sigma, Cc = 11, 40, 25.0, 3
    A, cc = aw * aw, (aw * aw) // 2
    _, noisy = Hh.noisy_lf(Hh.textured_lf(aw, aw, crop, crop), sigma)
    for step, pk, band_mb in ((1, (2, 4, 2, 8, 4, "id", "sadct", "haar"), None), (2, (4, 4, 2, 8, 4, "dct", "sadct", "haar"), None),
                              (1, (4, 4, 2, 8, 4, "id", "dct", "haar"), "2")):
        win, Wb, Hb = Hh.padded_window(noisy, crop, crop, Cc, pk[1] + pk[2])
        mask = np.ones(A, np.uint32)
        mask[5] = 0
        win[5] = 0
        proc = (mask == 0).astype(np.uint32)
        basic = np.ascontiguousarray(0.5 * win + 0.5 * np.roll(win, 1, axis=1)) if step == 2 else None
        out = {}
        for layout in ("sai-major", "group-major"):
            if layout == "group-major":
                monkeypatch.setenv("LFBM5D_FILT_GROUP_MAJOR", "1")
            else:
                monkeypatch.delenv("LFBM5D_FILT_GROUP_MAJOR", raising=False)
            if band_mb:
                monkeypatch.setenv("LFBM5D_BAND_MB", band_mb)
            else:
                monkeypatch.delenv("LFBM5D_BAND_MB", raising=False)
            out[layout] = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc, mask=mask, proc=proc, cst=cc, pst=cc, aw=aw)
        monkeypatch.delenv("LFBM5D_FILT_GROUP_MAJOR", raising=False)
        monkeypatch.delenv("LFBM5D_BAND_MB", raising=False)
        assert np.array_equal(out["sai-major"][0], out["group-major"][0]) and np.array_equal(out["sai-major"][1], out["group-major"][1]), (step, pk)
        assert float(np.abs(out["sai-major"][1]).sum()) > 0


@pytest.mark.parametrize("ah,aw,an", [(5, 5, 2), (7, 6, 2), (8, 7, 3), (9, 10, 4)])
def test_whole_steps_with_5x5_windows_match_oracle(ctx, ah, aw, an):
    """aswSize 2 and 3: the window schedule with 5x5 / 7x7 windows (compute_LF_angular_search_window's clamping at the
    borders), both steps against the oracle: same windows, PSNR within 0.01 dB."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    Hs = Ws = 72 if an == 2 else (64 if an == 3 else 48)
    lf = Hh.textured_lf(ah, aw, Hs, Ws)
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(ah * aw, np.uint32)
    p1, p2 = (4, 6, 2, 8, 4, "id", "sadct", "haar"), (8, 6, 2, 8, 4, "dct", "sadct", "haar")
    n1, b_o, st1 = O.run_step1(O.make_params(25.0, 2.7, *p1), noisy.copy(), mask, O.ROWMAJOR, aw, ah, an, Ws, Hs, 3)
    w1 = O.last_windows()
    _, _, d_o, st2 = O.run_step2(O.make_params(25.0, 2.7, *p2), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, aw, ah, an, Ws, Hs, 3)
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
    ctx.reset_stats()
    ctx.step1(core.make_params(25.0, 2.7, *p1), d_noisy, mask, d_basic, L.ROWMAJOR, aw, ah, an, Ws, Hs, 3)
    assert np.array_equal(ctx.last_windows(), w1) and ctx.stats().windows == st1.windows
    pb = O.psnr_lf(d_basic.cpu().numpy(), clean)
    ctx.step2(core.make_params(25.0, 2.7, *p2), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, aw, ah, an, Ws, Hs, 3)
    pd = O.psnr_lf(d_den.cpu().numpy(), clean)
    assert abs(pb - O.psnr_lf(b_o, clean)) < 0.01 and abs(pd - O.psnr_lf(d_o, clean)) < 0.01
    assert pd > O.psnr_lf(noisy, clean) + 6


def _random_cases():
    # LFBM5D_TEST_SEED / LFBM5D_TEST_CASES: wider sweeps by hand (the committed default keeps the suite short)
    rng = np.random.default_rng(int(os.environ.get("LFBM5D_TEST_SEED", "20261002")))
    cases = []
    while len(cases) < int(os.environ.get("LFBM5D_TEST_CASES", "12")):
        step = int(rng.integers(1, 3))
        k = int(rng.choice([8, 12, 16]))
        N = int(rng.choice([1, 2, 4, 8, 16] if step == 2 else [1, 2, 4, 8]))
        nSim, nDisp, p = int(rng.integers(3, 9)), int(rng.integers(1, 4)), int(rng.integers(1, 6))
        tau2 = str(rng.choice(["id", "dct", "bior"] if k != 12 else ["id", "dct"]))
        tau4 = str(rng.choice(["id", "dct", "sadct"]))
        tau5 = str(rng.choice(["haar", "hw", "dct"]))
        ch, cw = int(rng.integers(k + 2 * (nSim + nDisp) + 6, 110)), int(rng.integers(k + 2 * (nSim + nDisp) + 6, 140))
        sigma = float(rng.choice([10.0, 25.0, 50.0]))
        # (stacks beyond the 160 KiB LDS -- e.g. step 2, N = 16, k = 16 -- run on the HBM-scratch form of the generic kernel)
        # useSD stays 0 here: the reference's sd_weighting_5d (core:3140-3173) subtracts two float sums of k^2 N
        # terms that nearly cancel, so its value depends on the summation order to ~1e-3; the two dedicated
        # useSD cases above pin well-conditioned inputs
        cases.append((f"rnd{len(cases)}-s{step}-k{k}-N{N}-{tau2}-{tau4}-{tau5}-p{p}-{ch}x{cw}", step, sigma,
                      (N, nSim, nDisp, k, p, tau2, tau4, tau5), (ch, cw), 0))
    return cases


# Stacks beyond the LDS (lfbm5d_group_slab.hip, round 5): the Wiener step with 12x12 / 16x16 patches, N = 32 -- weights that are float
# sums of up to 2 x 32 x 9 x 256 terms: the tolerances of the sweep, not the strict ones
SLAB_CASES = [
    ("wien-k16-dct-n16", 2, 25.0, (16, 6, 2, 16, 4, "dct", "sadct", "haar"), 96, 0),
    ("wien-k16-bior-n8", 2, 25.0, (8, 6, 2, 16, 4, "bior", "dct", "haar"), 96, 0),
    ("wien-k16-id-n16-dct5", 2, 25.0, (16, 6, 2, 16, 4, "id", "sadct", "dct"), 96, 0),
    ("wien-k12-id-n16", 2, 10.0, (16, 6, 2, 12, 4, "id", "dct", "haar"), 72, 0),
    ("wien-k16-dct-n32-hw", 2, 10.0, (32, 8, 2, 16, 4, "dct", "sadct", "hw"), 96, 0),
    ("ht-k16-dct-n32", 1, 10.0, (32, 8, 2, 16, 4, "dct", "sadct", "haar"), 96, 0),
    ("ht-k12-dct-n32-hw", 1, 10.0, (32, 8, 2, 12, 4, "dct", "dct", "hw"), 72, 0),
]


@pytest.mark.parametrize("case", SLAB_CASES, ids=[c[0] for c in SLAB_CASES])
def test_large_stack_configurations_match_oracle(ctx, case, monkeypatch):
    """... against the oracle, and against the same pass through round 4's general kernel (stacks in HBM slices,
    LFBM5D_NO_SLAB_KERNEL): the slab kernel runs the same transform routines in the same order; only sums that depend on the
    thread layout (the group weights) and the compiler's choice of fused multiply-adds may differ, far inside the oracle's
    tolerance."""
    _check_pass(ctx, case, strict=False)
    name, step, sigma, pk, crop, useSD = case
    win, Wb, Hb, Cc = window(sigma, pk, crop)
    basic = None
    if step == 2:
        n1, d1 = gpu_pass(ctx, 1, sigma, (pk[0] // 2 or 1,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc)
        basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    num_s, den_s = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc)
    monkeypatch.setenv("LFBM5D_NO_SLAB_KERNEL", "1")
    num_g, den_g = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc)
    monkeypatch.delenv("LFBM5D_NO_SLAB_KERNEL")
    fin = np.isfinite(num_s) & np.isfinite(den_s) & np.isfinite(num_g) & np.isfinite(den_g)
    assert fin.mean() > 0.99 and np.array_equal(den_s != 0, den_g != 0)
    es, eg = Hh.estimate(np.where(fin, num_s, 0), np.where(fin, den_s, 0), win), Hh.estimate(np.where(fin, num_g, 0), np.where(fin, den_g, 0), win)
    assert np.abs(es - eg).mean() < 2e-5 and np.quantile(np.abs(es - eg), 0.999) < 5e-3, (np.abs(es - eg).mean(), np.abs(es - eg).max())


@pytest.mark.parametrize("case", _random_cases(), ids=[c[0] for c in _random_cases()])
def test_random_configurations_match_oracle(ctx, case):
    """Seeded sweep over patch sizes, search ranges, steps, transforms and odd window shapes."""
    _check_pass(ctx, case, strict=False)


def test_aggregation_64bit_gather_path_is_identical(ctx, monkeypatch):
    """filt of 4 GiB and more switches the aggregation gathers from a buffer resource to 64-bit addresses; the
    environment override runs that path on a small window: same bits."""
    pk = (8, 6, 2, 8, 3, "dct", "sadct", "haar")
    win, Wb, Hb, Cc = window(25.0, pk, 64)
    basic = np.ascontiguousarray(0.5 * win + 0.5 * np.roll(win, 1, axis=1))
    monkeypatch.delenv("LFBM5D_AGG_64BIT", raising=False)
    n0, d0 = gpu_pass(ctx, 2, 25.0, pk, win, basic, Wb, Hb, Cc)
    monkeypatch.setenv("LFBM5D_AGG_64BIT", "1")
    n1, d1 = gpu_pass(ctx, 2, 25.0, pk, win, basic, Wb, Hb, Cc)
    assert np.array_equal(n0, n1) and np.array_equal(d0, d1) and np.abs(d0).max() > 0


def test_rccl_all_reduce_on_the_library_stream(ctx):
    """The collective of the multi-GPU schemes, on a one-rank communicator: RCCL loads, takes the library's
    non-blocking stream and returns the right sums (the only part of N > 1 a one-GPU box can run for real)."""
    ctx.comm_selftest(1 << 22)


def test_unsupported_configurations_fail_loudly(ctx):
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    t = torch.zeros((25, 3 * 32 * 32), device="cuda")
    with pytest.raises(L.LfBm5dError, match="angular search window"):   # a 7x7 window on a 5x5 light field: the reference's own refusal (bm5d.cpp:119-124)
        ctx.step1(core.make_params(25, 2.7, 4, 4, 2, 8, 4, "id", "sadct", "haar"), t, np.ones(25, np.uint32), t.clone(),
                  L.ROWMAJOR, 5, 5, 3, 32, 32, 3)
    with pytest.raises(L.LfBm5dError, match="power of two"):
        ctx.step1(core.make_params(25, 2.7, 6, 4, 2, 8, 4, "id", "sadct", "haar"), t, np.ones(25, np.uint32), t.clone(),
                  L.ROWMAJOR, 5, 5, 1, 32, 32, 3)


FULL_SIZE = {
    # the headline workload and BASELINE.json configs[2], [3], [4] at their own light-field sizes
    "lf17x17x512x512_sigma25": (17, 17, 512, 512, 25.0, Hh.README_HT, Hh.README_WIEN),
    "lf9x9x512x512_sigma25": (9, 9, 512, 512, 25.0, Hh.README_HT, Hh.README_WIEN),
    "lf17x17x512x512_sigma10_bior": (17, 17, 512, 512, 10.0, Hh.C4_HT, Hh.README_WIEN),
    "lf15x15x625x434_sigma50_n1": (15, 15, 434, 625, 50.0, Hh.C5_HT, Hh.C5_WIEN),
}


@pytest.mark.parametrize("name", sorted(FULL_SIZE))
def test_full_size_properties(ctx, monkeypatch, name):
    """BASELINE configurations at full size: properties that do not need the oracle -- the pipelined run (three lanes)
    and the window-after-window run are bit-identical (no float atomics, dependencies honoured), the windows are the
    planned sequence with one centre pass each (quirk 1), every value is finite, both steps raise the PSNR."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core, synth
    ah, aw, Hs, Ws, sigma, p1, p2 = FULL_SIZE[name]
    A = ah * aw
    lf = synth.make_lf(ah, aw, Hs, Ws)
    clean = torch.from_numpy(lf.reshape(A, -1)).cuda().float()
    del lf
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    noisy0 = clean + sigma * torch.randn(clean.shape, generator=g, device="cuda")
    mask = np.ones(A, np.uint32)
    plan = core.plan_windows(aw, ah, 1, L.ROWMAJOR)
    outs = []
    for lanes in ("2", "1"):
        monkeypatch.setenv("LFBM5D_LANES", lanes)
        noisy = noisy0.clone()
        basic, den = torch.zeros_like(noisy), torch.zeros_like(noisy)
        ctx.reset_stats()
        ctx.step1(core.make_params(sigma, 2.7, *p1), noisy, mask, basic, L.ROWMAJOR, aw, ah, 1, Ws, Hs, 3)
        assert np.array_equal(ctx.last_windows(), plan)
        b1 = basic.clone()
        ctx.step2(core.make_params(sigma, 2.7, *p2), noisy, mask, basic, den, L.ROWMAJOR, aw, ah, 1, Ws, Hs, 3)
        assert np.array_equal(ctx.last_windows(), plan)
        outs.append((b1, den.clone()))
        s = ctx.stats()
        assert s.windows == s.passes == 2 * len(plan)            # one centre pass per window (quirk 1)
        assert (s.lane_windows > 0) == (lanes == "2")
        del noisy, basic, den

    def psnr(x):
        mse = ((x - clean) ** 2).mean(dim=1)
        return float((20 * torch.log10(255.0 / torch.sqrt(mse))).mean())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert psnr(noisy0) + 8 < psnr(outs[0][0]) < psnr(outs[0][1])
    assert torch.isfinite(outs[0][1]).all() and torch.isfinite(outs[0][0]).all()


def test_headline_workload_on_eight_emulated_ranks_is_bit_identical(ctx, monkeypatch):
    """The headline light field (17x17x512x512, sigma 25) with the multi-GPU window graph played by eight ranks on this GPU
    (LFBM5D_EMULATE_WORLD: every rank its own num / den, lanes and exchange streams, messages as device copies in the
    RCCL issue order): bit-identical to the single-rank run, the planned windows, 127+ messages per step."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core, synth
    ah = aw = 17
    Hs = Ws = 512
    A = ah * aw
    clean = torch.from_numpy(synth.make_lf(ah, aw, Hs, Ws).reshape(A, -1)).cuda().float()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    noisy0 = clean + 25.0 * torch.randn(clean.shape, generator=g, device="cuda")
    mask = np.ones(A, np.uint32)
    plan = core.plan_windows(aw, ah, 1, L.ROWMAJOR)
    P1, P2 = core.make_params(25.0, 2.7, *Hh.README_HT), core.make_params(25.0, 2.7, *Hh.README_WIEN)

    def run():
        noisy = noisy0.clone()
        basic, den = torch.zeros_like(noisy), torch.zeros_like(noisy)
        ctx.reset_stats()
        ctx.step1(P1, noisy, mask, basic, L.ROWMAJOR, aw, ah, 1, Ws, Hs, 3)
        assert np.array_equal(ctx.last_windows(), plan)
        b1 = basic.clone()
        ctx.step2(P2, noisy, mask, basic, den, L.ROWMAJOR, aw, ah, 1, Ws, Hs, 3)
        return b1, den, ctx.stats()
    for k in ("LFBM5D_EMULATE_WORLD", "LFBM5D_STEP_SHARDING", "LFBM5D_LANES"):
        monkeypatch.delenv(k, raising=False)
    b0, d0, s0 = run()
    monkeypatch.setenv("LFBM5D_EMULATE_WORLD", "8")
    b8, d8, s8 = run()
    monkeypatch.delenv("LFBM5D_EMULATE_WORLD")
    ranks, _, start = core.plan_graph(aw, ah, 8)
    assert len(set(ranks.tolist())) >= 4 and s0.messages == 0 and s8.messages == 2 * len(core.plan_messages(aw, ah, 8)) >= 254
    assert torch.equal(b0, b8) and torch.equal(d0, d8)


# ------------------------------------------------------------------------------------------------
# per-SAI BM3D (LFBM3Ddenoising): the same kernels with a one-image window
# ------------------------------------------------------------------------------------------------
BM3D_CASES = [
    # name, sigma, grey, crop, hard (N, n, k, p, tau_2D, useSD), wien
    ("readme", 25.0, False, 80, (16, 16, 8, 3, "bior", 0), (32, 16, 8, 3, "dct", 0)),       # README.md:51
    ("sigma40-dct-bior", 40.0, False, 64, (8, 8, 8, 4, "dct", 0), (16, 8, 8, 4, "bior", 0)),   # tauMatch 5000 / 3500
    ("grey-k12", 25.0, True, 72, (16, 10, 12, 4, "dct", 0), (16, 10, 12, 4, "dct", 0)),
    ("k16-bior", 10.0, False, 96, (4, 6, 16, 5, "bior", 0), (8, 6, 16, 5, "bior", 0)),
]


@pytest.mark.parametrize("case", BM3D_CASES, ids=[c[0] for c in BM3D_CASES])
def test_bm3d_steps_match_oracle(ctx, case):
    """bm3d_1st_step / bm3d_2nd_step through lfbm5d_bm3d_step_device against the oracle's restatement
    (bm3d.cpp:315-690) on the same padded image; step 2 runs on the ORACLE's basic estimate."""
    from lfbm5d_amd import core
    _, sigma, grey, crop, hard, wien = case
    lf = Hh.source_lf(crop=crop)[:1]
    if grey:
        lf = lf[:, :1]
    Cc = lf.shape[1]
    clean, noisy = Hh.noisy_lf(lf, sigma)
    nP = hard[1]
    win, Wb, Hb = Hh.padded_window(noisy, crop, crop, Cc, nP)
    inner = np.zeros((Cc, Hb, Wb), bool)
    inner[:, nP:-nP, nP:-nP] = True
    inner = inner.reshape(-1)
    b_o, st1 = O.bm3d_step(1, sigma, 2.7, win[0], None, Wb, Hb, Cc, hard[1], hard[2], hard[0], hard[3], hard[4], hard[5])
    d_win = torch.from_numpy(win[0]).cuda()
    d_out = torch.zeros_like(d_win)
    ctx.reset_stats()
    ctx.bm3d_step(1, core.make_bm3d_params(sigma, 2.7, hard[0], hard[1], hard[2], hard[3], hard[4], hard[5]), Wb, Hb, Cc, d_win, None, d_out)
    s = ctx.stats()
    assert (s.groups, s.stack_patches) == (st1.groups, st1.stack_patches)      # identical matching
    b_g = d_out.cpu().numpy()
    assert np.isfinite(b_o[inner]).all()
    assert np.abs(b_g - b_o)[inner].max() < 2e-3
    # second step on identical inputs: crop + re-pad the oracle's basic estimate like run_bm3d does (bm3d.cpp:148-158)
    basic = np.zeros((1, Cc * crop * crop), np.float32)
    O.lib().orc_unsymetrize(basic[0], b_o, crop, crop, Cc, nP)
    bwin, _, _ = Hh.padded_window(basic, crop, crop, Cc, nP, color=False)
    d_o, st2 = O.bm3d_step(2, sigma, 2.7, win[0], bwin[0], Wb, Hb, Cc, wien[1], wien[2], wien[0], wien[3], wien[4], wien[5])
    d_b = torch.from_numpy(bwin[0]).cuda()
    ctx.reset_stats()
    ctx.bm3d_step(2, core.make_bm3d_params(sigma, 2.7, wien[0], wien[1], wien[2], wien[3], wien[4], wien[5]), Wb, Hb, Cc, d_win, d_b, d_out)
    s = ctx.stats()
    assert (s.groups, s.stack_patches) == (st2.groups, st2.stack_patches)
    assert np.abs(d_out.cpu().numpy() - d_o)[inner].max() < 2e-3


def test_run_bm3d_lf_matches_oracle(ctx):
    """run_bm3d_LF (bm3d_LF.cpp:75-125) on a 2-SAI light field with one empty SAI in between, host buffers through the
    reference-named wrapper: outputs and the in-place drift of LF_noisy like the oracle."""
    import lfbm5d_amd as L
    crop, sigma = 64, 25.0
    clean, noisy = Hh.noisy_lf(Hh.source_lf(crop=crop)[:3], sigma)
    mask = np.array([1, 0, 1], np.uint32)
    hard, wien = (16, 8, 8, 3, "bior", 0), (32, 8, 8, 3, "dct", 0)
    n_o, b_o, d_o, _ = O.run_bm3d_lf(sigma, 2.7, noisy, mask, crop, crop, 3, hard, wien)
    n_g = noisy.copy(); b_g = np.zeros_like(noisy); d_g = np.zeros_like(noisy)
    rc = L.run_bm3d_LF(sigma, n_g, mask, b_g, d_g, crop, crop, 3, hard[1], wien[1], hard[2], wien[2], hard[0], wien[0],
                       hard[3], wien[3], False, False, L.BIOR, L.DCT, 2.7, L.OPP, ctx=ctx)
    assert rc == 0
    assert np.abs(n_g - n_o).max() < 1e-4 and np.abs(n_g[1] - noisy[1]).max() == 0     # empty SAI untouched
    assert np.abs(b_g - b_o).max() < 2e-3
    assert np.abs(d_g - d_o).max() < 5e-3
    for a, b in ((b_g, b_o), (d_g, d_o)):
        assert abs(O.psnr_lf(a[[0, 2]], clean[[0, 2]]) - O.psnr_lf(b[[0, 2]], clean[[0, 2]])) < 1e-3


def test_bm3d_rejects_what_is_not_built(ctx):
    from lfbm5d_amd import core
    t = torch.zeros(3 * 64 * 64, device="cuda")
    with pytest.raises(core.LfBm5dError, match="power of two"):
        ctx.bm3d_step(1, core.make_bm3d_params(25, 2.7, 1, 8, 8, 3, "bior"), 64, 64, 3, t, None, t.clone())
    with pytest.raises(core.LfBm5dError, match="dct or bior"):
        ctx.bm3d_step(1, core.make_bm3d_params(25, 2.7, 8, 8, 8, 3, "id"), 64, 64, 3, t, None, t.clone())
    z = np.zeros((1, 3 * 32 * 32), np.float32)
    with pytest.raises(core.LfBm5dError, match="nWien > nHard"):      # the reference itself returns 0 / 0 there
        ctx.bm3d_lf(core.make_bm3d_params(25, 2.7, 8, 4, 8, 3, "bior"), core.make_bm3d_params(25, 2.7, 8, 6, 8, 3, "dct"),
                    z.copy(), np.ones(1, np.uint32), z.copy(), z.copy(), 32, 32, 3)


@pytest.mark.parametrize("nHard,nWien", [(12, 8), (16, 6)])
def test_bm3d_lf_with_different_search_windows_matches_oracle(ctx, nHard, nWien):
    """run_bm3d pads both steps by nHard, searches the second within nWien and crops it at offset nWien of the
    nHard-padded image (bm3d.cpp:126-189): a shifted picture unless the two are equal.  Reproduced as it is."""
    from lfbm5d_amd import core
    lf = Hh.source_lf(crop=72)[[0, 4]]
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(2, np.uint32)
    hard, wien = (8, nHard, 8, 3, "bior", 0), (16, nWien, 8, 3, "dct", 0)
    _, b_o, d_o, _ = O.run_bm3d_lf(25.0, 2.7, noisy, mask, 72, 72, 3, hard, wien)
    h_noisy, h_basic, h_den = noisy.copy(), np.zeros_like(noisy), np.zeros_like(noisy)
    ctx.bm3d_lf(core.make_bm3d_params(25.0, 2.7, 8, nHard, 8, 3, "bior"), core.make_bm3d_params(25.0, 2.7, 16, nWien, 8, 3, "dct"),
                h_noisy, mask, h_basic, h_den, 72, 72, 3)
    assert np.abs(h_basic - b_o).max() < 5e-3
    assert np.abs(h_den - d_o).max() < 2e-2 and abs(O.psnr_lf(h_den, clean) - O.psnr_lf(d_o, clean)) < 0.01
    assert O.psnr_lf(h_den, clean) < O.psnr_lf(h_basic, clean)      # the reference's shifted crop: worse than its own first step


def test_bm3d_lf_lanes_do_not_change_the_result(ctx, monkeypatch):
    """LFBM3D's SAIs are independent images: run_bm3d_lf deals them to lanes (streams + work buffers of their own, round 4:
    64 -> 105 SAI-MP/s on 512 x 512 SAIs); one, three or five lanes, with an empty SAI in between: the same bytes."""
    from lfbm5d_amd import core
    lf = Hh.source_lf(crop=64)[[0, 2, 4, 5, 6, 7, 8]]
    clean, noisy = Hh.noisy_lf(lf, 25.0)
    mask = np.ones(7, np.uint32)
    mask[3] = 0
    hard, wien = core.make_bm3d_params(25.0, 2.7, 8, 8, 8, 3, "bior"), core.make_bm3d_params(25.0, 2.7, 16, 8, 8, 3, "dct")
    res = []
    for lanes in ("1", "3", "5"):
        monkeypatch.setenv("LFBM5D_BM3D_LANES", lanes)
        h_noisy, h_basic, h_den = noisy.copy(), np.zeros_like(noisy), np.zeros_like(noisy)
        ctx.reset_stats()
        ctx.bm3d_lf(hard, wien, h_noisy, mask, h_basic, h_den, 64, 64, 3)
        res.append((h_noisy, h_basic, h_den, int(ctx.stats().groups)))
    for r in res[1:]:
        assert r[3] == res[0][3] > 0
        assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1]) and np.array_equal(r[2], res[0][2])
    assert not res[0][2][3].any()
    assert O.psnr_lf(res[0][2][mask != 0], clean[mask != 0]) > O.psnr_lf(noisy[mask != 0], clean[mask != 0]) + 5


# ------------------------------------------------------------------------------------------------
# the headline's window pass at its own size against the oracle
# ------------------------------------------------------------------------------------------------
FULL_WINDOWS = [
    # name, step, parameters, H, W, sigma
    ("ht", 1, Hh.README_HT, 512, 512, 25.0),                 # headline: k_bm_scan2<16>, k_group_id_haar, k_aggregate<16x4>
    ("wiener", 2, Hh.README_WIEN, 512, 512, 25.0),           # headline: k_bm_scan2<8>, k_group_dct8w3, k_aggregate<8x8>
    ("config3-ht-bior", 1, Hh.C4_HT, 512, 512, 10.0),        # BASELINE configs[3]: k_group_bior16_haar
    ("config4-ht-n1", 1, Hh.C5_HT, 434, 625, 50.0),          # BASELINE configs[4]: 49 tables per SAI, no self search, three groups per workgroup
    ("config4-wiener-n8", 2, Hh.C5_WIEN, 434, 625, 50.0),    # BASELINE configs[4]: p = 3 grid, N = 8 Wiener stacks, 667 x 476 window
]


@pytest.mark.parametrize("case", FULL_WINDOWS, ids=[c[0] for c in FULL_WINDOWS])
def test_headline_window_pass_matches_oracle_at_full_size(ctx, case):
    """One 3x3 centre-window pass of the benchmark's synthetic light field at the window sizes of the headline and of BASELINE
    configurations [3] and [4] (560^2 / 667 x 476 padded; 15 625 ... 29 601 groups) against the oracle's pass on the same window
    (OpenMP over reference patches: some tens of seconds of CPU): the block-matching tables identical, survivor counts group
    by group, `den` and the estimate as in the random sweep.  These are the sizes the dedicated kernels (table scan with
    eleven waves per workgroup, register-resident HT kernel, the 16x16 wavelet kernel, its three-groups-per-workgroup N = 1
    form, the one-image-at-a-time Wiener kernel, gather aggregation) are tuned at."""
    from lfbm5d_amd import synth
    name, step, pk, H, W, sigma = case
    lf = synth.make_lf(3, 3, H, W).reshape(9, 3, H, W).astype(np.float32)
    noisy = lf + sigma * np.random.default_rng(1).standard_normal(lf.shape).astype(np.float32)
    win, Wb, Hb = Hh.padded_window(np.ascontiguousarray(noisy.reshape(9, -1)), W, H, 3, pk[1] + pk[2])
    _check_window(ctx, "full-" + name, step, sigma, pk, 0, win, Wb, Hb, 3, strict=False)


# ------------------------------------------------------------------------------------------------
# dedicated group kernels against the generic LDS kernel at the benchmark's window size
# ------------------------------------------------------------------------------------------------
DEDICATED = [
    # name, step, params (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D), exact
    ("ht-id-n8", 1, (8, 18, 6, 16, 4, "id", "sadct", "haar"), False),         # README HT: register-resident kernel, Haar on pairs
    ("ht-bior-n8", 1, (8, 18, 6, 16, 4, "bior", "sadct", "haar"), False),     # configuration 4 (same wavelet taps, other Haar association)
    ("ht-bior-n1", 1, (1, 18, 3, 16, 3, "bior", "sadct", "haar"), False),     # configuration 5: three groups per workgroup, no stack transform
    ("ht-dct16-n8", 1, (8, 18, 6, 16, 4, "dct", "sadct", "haar"), False),     # even/odd 16-point DCT against the cosine-table form
    ("wien-dct-n16", 2, (16, 18, 6, 8, 4, "dct", "sadct", "haar"), False),    # README Wiener: butterfly 8-point DCT, packed pair
    ("wien-bior-n16", 2, (16, 18, 6, 8, 4, "bior", "sadct", "haar"), False),
]


def test_wiener_kernel_generations_agree_at_full_window_size(ctx, monkeypatch):
    """k_group_dct8w3 (one image in LDS at a time, factorised 3x3 DCT) against round 2's k_group_dct8w2 (LFBM5D_DCT8W_V2: still
    the kernel of very large windows and of the Hadamard / DCT fibres) on one 3x3x512x512 Wiener pass: same matching, same
    aggregation; no threshold in this step, so the estimates differ by round-off only."""
    from lfbm5d_amd import core, synth
    pk = (16, 18, 6, 8, 4, "dct", "sadct", "haar")
    H = W = 512
    lf = synth.make_lf(3, 3, H, W).reshape(9, 3, H, W).astype(np.float32)
    lf += 25.0 * np.random.default_rng(1).standard_normal(lf.shape).astype(np.float32)
    nHW = pk[1] + pk[2]
    pad = np.pad(lf, ((0, 0), (0, 0), (nHW, nHW), (nHW, nHW)), mode="symmetric")
    Hb, Wb = pad.shape[2:]
    noisy = torch.from_numpy(np.ascontiguousarray(pad).reshape(9, -1)).cuda()
    basic = 0.5 * noisy + 0.5 * torch.roll(noisy, 1, 1)
    P = core.make_params(25.0, 2.7, *pk)
    mask, proc = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    res = []
    for old in (False, True):
        if old:
            monkeypatch.setenv("LFBM5D_DCT8W_V2", "1")
        else:
            monkeypatch.delenv("LFBM5D_DCT8W_V2", raising=False)
        num = torch.zeros_like(noisy); den = torch.zeros_like(noisy)
        ctx.reset_stats()
        ctx.core_pass(2, P, 3, 3, Wb, Hb, 3, noisy, basic, num, den, mask, proc, 4, 4)
        res.append((num.cpu().numpy(), den.cpu().numpy(), ctx.stats().ms_group))
    (n3, d3, ms3), (n2, d2, ms2) = res
    assert ms3 < ms2
    assert np.array_equal(d3 > 0, d2 > 0)
    both = d3 > 0
    np.testing.assert_allclose(d3[both], d2[both], rtol=2e-5)
    diff = np.abs(n3[both] / d3[both] - n2[both] / d2[both])
    # round 6: k_group_dct8w3_u evaluates the angular and Haar stages unnormalised (additions; the constants folded into the shrinkage
    # and the inverse's input scale), k_group_dct8w2 in the reference's scale: the estimates differ by an ulp and a half of a
    # grey level around 150 on average (measured 2.3e-5; 1.9e-5 between the two normalised kernels) -- the bar against the ORACLE
    # (test_core_pass_matches_oracle, wien-* cases) is unchanged
    assert diff.max() < 2e-3 and diff.mean() < 3e-5


@pytest.mark.parametrize("case", DEDICATED, ids=[c[0] for c in DEDICATED])
def test_dedicated_kernels_agree_with_the_generic_kernel_at_full_window_size(ctx, case, monkeypatch):
    """One 3x3x512x512 centre-window pass (560^2 padded, 15 625 / 16 129 groups -- far beyond what the oracle finishes
    in seconds): the dedicated group kernel of the configuration against the generic LDS kernel (LFBM5D_GROUP_GENERIC),
    same matching, same aggregation.  Identical where the arithmetic is the same operation sequence; where a transform
    is factorised, associated or contracted differently, float round-off moves the estimate by ~1e-4 on average;
    hard-threshold ties account for the tail."""
    from lfbm5d_amd import core, synth
    _, step, pk, exact = case
    H = W = 512
    lf = synth.make_lf(3, 3, H, W).reshape(9, 3, H, W).astype(np.float32)
    lf += 25.0 * np.random.default_rng(1).standard_normal(lf.shape).astype(np.float32)
    nHW = pk[1] + pk[2]
    pad = np.pad(lf, ((0, 0), (0, 0), (nHW, nHW), (nHW, nHW)), mode="symmetric")
    Hb, Wb = pad.shape[2:]
    noisy = torch.from_numpy(np.ascontiguousarray(pad).reshape(9, -1)).cuda()
    basic = (0.5 * noisy + 0.5 * torch.roll(noisy, 1, 1)) if step == 2 else None
    P = core.make_params(25.0, 2.7, *pk)
    mask, proc = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    res = []
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("LFBM5D_GROUP_GENERIC", "1")
        else:
            monkeypatch.delenv("LFBM5D_GROUP_GENERIC", raising=False)
        num = torch.zeros_like(noisy); den = torch.zeros_like(noisy)
        ctx.reset_stats()
        ctx.core_pass(step, P, 3, 3, Wb, Hb, 3, noisy, basic, num, den, mask, proc, 4, 4)
        res.append((num.cpu().numpy(), den.cpu().numpy(), ctx.stats().ms_group))
    (n_d, d_d, ms_d), (n_g, d_g, ms_g) = res
    assert ms_d < ms_g                                                   # the dedicated kernel is the faster one
    if exact:
        assert np.array_equal(d_d, d_g) and np.array_equal(n_d, n_g)
    else:
        assert np.array_equal(d_d > 0, d_g > 0)
        both = d_d > 0
        diff = np.abs(n_d[both] / d_d[both] - n_g[both] / d_g[both])
        # the bounds of the random-configuration sweep; the 16-point DCT (even/odd split against the cosine-table product) has
        # a threshold tie in most groups: coefficients up to 16 x the mean grey level carry ~1e-3 of round-off
        assert diff.mean() < 3e-4 and np.quantile(diff, 0.999) < 5e-2
        if step == 2:
            assert diff.max() < 2e-3                                     # no thresholds in the Wiener step
