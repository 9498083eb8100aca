"""Block matching on EXACT ties (GPU): one core pass per case of tests/bm_tie_cases.py, then the tables of that pass against the
oracle's with full bitwise equality -- refs, idx[:cnt], cnt, and best / shape of EVERY non-centre view over the whole compared
region.  tests/test_bm_ties.py holds the oracle to the int64 model on the same cases, so a kernel that resolves a tie in anything
but candidate scan order fails here: the 64-bit (score, scan index) keys and the three selection paths of k_self_select, the
first-table rule of the table kernel's in-workgroup reduction, the (value, order) minimum over a slot's workgroups and its edge
arrays, and `v == bv && order < bo` of the full-table arg-min kernels -- in every generation of the table kernel.

Natural cases (quantised, saturated) go on to the sums with test_gpu_parity._check_window's criteria; flat, periodic and
piecewise-constant planes stop at the tables and the group statistics (their transforms are degenerate)."""
import functools

import numpy as np
import pytest
import torch

import bm_tie_cases as Cs
import bm_tie_census as Census
import bm_tie_model as M
import helpers as Hh
from oracle import oracle as O
from test_gpu_parity import _check_window, gpu_pass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Oracle tables and group statistics of a case, computed once and shared by the kernel generations."""
    _, _, step, sigma, Cc, pk, _, aw, _ = Cs.by_name(name)
    N, nSim, nDisp, k, p = pk[:5]
    b = Cs.build(name)
    refs = Cs.refs_of(name)
    idx, cnt, disp = Census.oracle_tables(b["est"], b["cc"], k, N, nSim, nDisp, b["tau"], refs)
    _, _, st = Hh.oracle_pass(step, sigma, pk, b["win"], b["basic"], b["Wb"], b["Hb"], Cc, cst=b["cc"], pst=b["cc"], aw=aw)
    return refs, idx, cnt, disp, (st.groups, st.stack_patches, st.sadct_groups)


def _check_tables(ctx, name, want_version=None):
    _, _, step, sigma, Cc, pk, _, aw, _ = Cs.by_name(name)
    N, nSim, nDisp, k, p = pk[:5]
    b = Cs.build(name)
    Wb, Hb, A, cc = b["Wb"], b["Hb"], b["A"], b["cc"]
    o_refs, o_idx, o_cnt, o_disp, o_stats = _oracle(name)
    ctx.reset_stats()
    gpu_pass(ctx, step, sigma, pk, b["win"], b["basic"], Wb, Hb, Cc, cst=cc, pst=cc, aw=aw)
    s = ctx.stats()
    if want_version is not None:
        assert ctx.last_scan_version() == want_version
    refs, idx, cnt, best, shape = ctx.last_bm(N, A, Wb * Hb)
    assert np.array_equal(refs, o_refs)
    assert np.array_equal(cnt, o_cnt)
    used = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    bad = np.argwhere(np.where(used, idx, 0) != np.where(used, o_idx, 0))
    assert len(bad) == 0, (name, len(bad), bad[:4].tolist())
    rows, cols = M.region(Hb, Wb, k, nDisp)
    assert len(o_disp) == A - 1
    for st, (ob, osh) in o_disp.items():
        gb, gs = best[st].reshape(Hb, Wb)[rows, cols], shape[st].reshape(Hb, Wb)[rows, cols]
        assert np.array_equal(gb, ob), (name, st, int((gb != ob).sum()), np.argwhere(gb != ob)[:4].tolist())
        assert np.array_equal(gs, osh), (name, st, int((gs != osh).sum()))
    assert (s.groups, s.stack_patches, s.sadct_groups) == o_stats


@pytest.mark.parametrize("name", Cs.IDS)
def test_tables_on_exact_ties_match_oracle(ctx, name):
    """The default kernels: combined form where the table kernel's plan holds (k = 8 / 16), the any-size kernel for k = 4 / 6 / 10."""
    c = Cs.by_name(name)
    _check_tables(ctx, name, want_version=1 if c[5][3] not in (8, 16) else None)
    if c[8]:   # natural data: the sums by the criteria of the parity tests, on the same window and pilot
        b = Cs.build(name)
        _check_window(ctx, name, c[2], c[3], c[5], 0, b["win"], b["Wb"], b["Hb"], c[4], strict=False, basic=b["basic"])


# every generation of the table kernel on the cases that put ties on its seams: nDisp = 2 (25 tables, three workgroups per slot) and
# nDisp = 6 (169 tables, sixteen), more than one 64-column strip with a ragged last one, p = 3 off the store pattern, both steps
GENERATION_CASES = ["flat-k8-nsim5", "flat-k16-nsim6-nd3", "q16-k8-ht", "q64-k8-wien-wide-p3", "q16-k16-ht-wide-p3",
                    "sat-k8-ht-grey", "hstripes4-k8-wien-nd6", "vstripes4-k16-nd3", "checker3-k8", "island-k8", "threq-k8-wien",
                    "threq-k16-wien"]
GENERATIONS = [("scan_full_tables", 2), ("scan_v1", 1), ("scan_any", 1)]


@pytest.mark.parametrize("name", GENERATION_CASES)
@pytest.mark.parametrize("option,version", GENERATIONS, ids=[g[0] for g in GENERATIONS])
def test_tables_on_exact_ties_in_every_kernel_generation(ctx, option, version, name):
    ctx.set_option(option, 1)
    try:
        _check_tables(ctx, name, want_version=version)
    finally:
        ctx.set_option(option, None)


def test_default_generation_is_the_combined_form(ctx):
    """What the default cases above ran: the combined form (version 3) for k = 16 and k = 8 at the suite's search windows."""
    for name in ("q16-k16-ht-nd3", "q16-k8-ht"):
        _check_tables(ctx, name, want_version=3)


def test_subset_pass_on_exact_ties_matches_oracle(ctx):
    """pst != cst on a quantised greyscale window, both forms of the subset scan (full grid, and the position map of
    subset_scan_v1).  The pass matches on num / den where den != 0 and on the window elsewhere: the sums handed to both sides
    are den = 1, num = the window on the left part of every plane, so the matching planes stay the integer planes, ties
    included, and the den-aware reference list is the right part."""
    name = "q16-k8-ht-grey-p4"
    _, _, step, sigma, Cc, pk, _, aw, _ = Cs.by_name(name)
    N, nSim, nDisp, k, p = pk[:5]
    b = Cs.build(name)
    win, Wb, Hb = b["win"], b["Wb"], b["Hb"]
    est = b["est"]
    den0 = np.zeros((9, Hb, Wb), np.float32)
    den0[:, :, :(3 * Wb) // 5] = 1.0
    den0 = den0.reshape(9, -1)
    num0 = (win * den0).astype(np.float32)
    proc = np.zeros(9, np.uint32)
    proc[4] = 1
    rows, cols = M.region(Hb, Wb, k, nDisp)
    for pst in (8, 1):
        num_o, den_o, st = Hh.oracle_pass(step, sigma, pk, win, None, Wb, Hb, Cc, num=num0.copy(), den=den0.copy(), proc=proc, pst=pst)
        assert st.groups > 0
        for v1 in (None, 1):
            ctx.set_option("subset_scan_v1", v1)
            try:
                ctx.reset_stats()
                num_g, den_g = gpu_pass(ctx, step, sigma, pk, win, None, Wb, Hb, Cc, num=num0.copy(), den=den0.copy(), proc=proc, pst=pst)
                s = ctx.stats()
                refs, idx, cnt, best, shape = ctx.last_bm(N, 9, Wb * Hb)
            finally:
                ctx.set_option("subset_scan_v1", None)
            assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
            o_idx, o_cnt = np.zeros((len(refs), N), np.uint32), np.zeros(len(refs), np.uint32)
            centre = np.ascontiguousarray(est[pst].reshape(-1))
            O.lib().orc_bm_self(centre, Wb, Hb, k, N, nSim + nDisp, nSim, b["tau"], refs, len(refs), o_idx.reshape(-1), o_cnt)
            used = np.arange(N)[None, :] < cnt[:, None]
            assert np.array_equal(cnt, o_cnt) and np.array_equal(np.where(used, idx, 0), np.where(used, o_idx, 0))
            sel = np.unique(idx[used])            # the positions the groups read their disparities at
            for st_i in range(9):
                if st_i == pst:
                    continue
                ob, osh = np.zeros(Wb * Hb, np.uint32), np.zeros(Wb * Hb, np.uint8)
                O.lib().orc_bm_stereo(centre, np.ascontiguousarray(est[st_i].reshape(-1)), Wb, Hb, k, nDisp, b["tau"], ob, osh)
                assert np.array_equal(best[st_i][sel], ob[sel]), (pst, v1, st_i)
                assert np.array_equal(shape[st_i][refs], osh[refs]), (pst, v1, st_i)
            assert np.array_equal(den_o != 0, den_g != 0)
            np.testing.assert_allclose(den_g, den_o, rtol=2e-5, atol=1e-7)
            assert np.abs(Hh.estimate(num_o, den_o, win) - Hh.estimate(num_g, den_g, win)).max() < 2e-3


def test_bm3d_step_on_a_quantised_plane_matches_oracle(ctx):
    """Per-SAI BM3D on a 16-level plane, checked the way test_bm3d_steps_match_oracle checks: identical group statistics, output
    within 2e-3 inside the padding; the second step runs on an integer pilot (the clean quantised plane) so that it ties too."""
    from lfbm5d_amd import core
    sigma, crop, nP = 25.0, 64, 8
    hard, wien = (8, 8, 8, 4, "dct", 0), (16, 8, 8, 4, "dct", 0)
    g = Hh.source_lf(crop=crop)[4:5, :1].astype(np.float64)
    noisy = np.floor(np.clip(g + np.random.default_rng(3).normal(0, 6, g.shape), 0, 255) / 16) * 16
    clean = np.floor(g / 16) * 16
    win, Wb, Hb = Hh.padded_window(noisy.reshape(1, -1).astype(np.float32), crop, crop, 1, nP, color=False)
    bwin, _, _ = Hh.padded_window(clean.reshape(1, -1).astype(np.float32), crop, crop, 1, nP, color=False)
    M.exact_domain(win[0], 8); M.exact_domain(bwin[0], 8)
    inner = np.zeros((1, Hb, Wb), bool)
    inner[:, nP:-nP, nP:-nP] = True
    inner = inner.reshape(-1)
    d_win, d_b = torch.from_numpy(win[0]).cuda(), torch.from_numpy(bwin[0]).cuda()
    d_out = torch.zeros_like(d_win)
    for step, prm, pilot_o, pilot_g in ((1, hard, None, None), (2, wien, bwin[0], d_b)):
        out_o, st = O.bm3d_step(step, sigma, 2.7, win[0], pilot_o, Wb, Hb, 1, prm[1], prm[2], prm[0], prm[3], prm[4], prm[5])
        ctx.reset_stats()
        ctx.bm3d_step(step, core.make_bm3d_params(sigma, 2.7, *prm), Wb, Hb, 1, d_win, pilot_g, d_out)
        s = ctx.stats()
        assert (s.groups, s.stack_patches) == (st.groups, st.stack_patches)
        # On a flat stretch every candidate ties at 0 and scan order fills the group before it reaches the reference patch
        # itself, so a few pixels at the band's edge are covered by no patch of the Wiener step: 0 / 0 in the reference's
        # num / den (bm3d.cpp:678-679), and the step's input (here: the pilot) on the GPU, which keeps the input where no patch
        # reached.  Few such pixels, and only in the Wiener step; everything else at the usual bound.
        out_g = d_out.cpu().numpy()
        hole = ~np.isfinite(out_o)
        assert np.isfinite(out_g).all() and hole[inner].mean() < 0.01
        assert step == 2 or not hole[inner].any()
        assert np.array_equal(out_g[inner & hole], (win[0] if step == 1 else bwin[0])[inner & hole])
        assert np.abs(out_g - out_o)[inner & ~hole].max() < 2e-3
