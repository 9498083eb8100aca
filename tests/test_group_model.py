"""The float64 model of the group stage (tests/group_model.py) against the CPU oracle's process_group, on every case the GPU test runs.

Per case of tests/group_cases.py:
  - model and oracle agree on nSx, on the shape-adaptive flag and on every hard-threshold decision outside the gap (survivor counts
    recovered from the weights; a pair with coefficients inside the gap may differ by at most that many, and each difference must
    show in the filtered values as exactly that coefficient); the oracle's hard-threshold weights are the float32 expression of
    their counts bit for bit;
  - their filtered values and weights differ by float32 round-off only: E_filt and E_w (tests/group_ref.py) of the oracle and of a
    second float32 evaluation -- the model's own code in float32 -- stay below 1e-5 (five transform stages of at most 64 x 9 x 32
    terms, each a few sqrt(n) eps32 ~ 1e-6 of the largest input; the Wiener sum runs over up to 32 x 25 x 64 = 51 200 terms: weights
    within 1e-4, times the condition number of the SD weight's subtraction where that is above 1; the windows of 9 x 9 SAIs and
    more sum up to 16 x 289 x 64 = 295 936 terms, and the worst case of an in-order float32 sum grows with the number of terms:
    1e-4 n / 51 200 for a case with n = max nSx A k^2 above 51 200);
  - at most 5 % of the case's (group, channel) pairs are open, the model alone deciding which, so that the GPU test holds the rest
    to exact decisions; in the hard-threshold cases of the wide windows at least a quarter of the pairs keep more than k^2
    coefficients -- more than a DC per pixel --, in those of the BM3D flavour more than nSx -- more than a DC per patch (a BM3D
    pair of two patches holds 2 k^2 coefficients in all) --, so that the filtered patches have structure.
The case table is complete before a GPU sees it: the dispatch of launch_group restated in Python (group_cases.expected_kernels)
reaches every __global__ of the five group files in every spelling a dispatcher launches, every window side of k_group_idw and
k_group_slab and every slab tier of slab_log2.  The wide hard-threshold cases run lambda 3.5: default-lambda decisions on wide
windows stay with the whole-pass tests (tests/test_gpu_parity.py).
"""
import os
import re

import numpy as np
import pytest

import group_cases as K
import group_model as M
import group_ref as G
from oracle import oracle as O

CASES = K.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transform_matrices_are_what_the_definitions_say():
    for n in (1, 2, 4, 8, 16, 32):
        H, W = M.haar_matrix(n), M.hadamard_matrix(n)
        assert np.allclose(H @ H.T, np.eye(n), atol=1e-14)
        assert np.array_equal(W @ W, n * np.eye(n))          # the reference inverts Hadamard by applying it again, over n
        assert np.allclose(M.dct_ortho(n) @ M.dct_ortho(n).T, np.eye(n), atol=1e-14)
    rng = np.random.default_rng(1)
    L = O.lib()
    for n in (2, 4, 8, 16, 32):      # the leaf routines the oracle pins against the compiled reference
        x = rng.normal(0, 50, n).astype(np.float32)
        y = x.copy(); L.orc_haar_forward(y, n)
        assert np.allclose(y, M.haar_matrix(n) @ x, rtol=0, atol=1e-4)
        y = x.copy(); L.orc_hadamard(y, n)
        assert np.allclose(y, M.hadamard_matrix(n) @ x, rtol=0, atol=1e-3)
    for k in (4, 8, 16):
        x = rng.normal(0, 50, (k, k)).astype(np.float32)
        y = np.zeros((k, k), np.float32)
        L.orc_bior_forward(x.reshape(-1), k, y.reshape(-1), k)
        assert np.allclose(y.reshape(-1), M.bior_2d(k, True) @ x.reshape(-1), rtol=0, atol=2e-4)
        z = y.copy(); L.orc_bior_inverse(z.reshape(-1), k)
        assert np.allclose(z.reshape(-1), M.bior_2d(k, False) @ y.reshape(-1).astype(np.float64), rtol=0, atol=2e-4)
        y = np.zeros((k, k), np.float32)
        L.orc_dct2d_forward(x.reshape(-1), k, y.reshape(-1), k)
        assert np.allclose(y.reshape(-1), M.transform_2d(M.DCT, k, True) @ x.reshape(-1), rtol=0, atol=2e-4)


@pytest.mark.parametrize("aw", (3, 5, 7, 9, 13, 17))
def test_sadct_matrices_on_every_shape(aw):
    """Forward and inverse of every 3 x 3 shape (a sample of the 5 x 5 ones; from 7 x 7 on a seeded sample of random shapes of every
    density and every lone-SAI shape of group_cases.wide_shapes) against the oracle's; inverse o forward is the identity on the
    shape and forward o inverse on mask_dct."""
    A = aw * aw
    rng = np.random.default_rng(aw)
    L = O.lib()
    if aw == 3:
        shapes = range(1, 1 << A)
    elif aw == 5:
        shapes = [int(b) | 1 for b in rng.integers(1, 1 << A, 300)]
    else:
        shapes = K.wide_shapes(rng, aw, A // 2, 60) + K.wide_shapes(rng, aw, 2 * aw + 1, 20)[:60:3]
    for bits in shapes:
        F, Gm, md = M.sadct_matrices(int(bits), aw)
        mask = np.array([(bits >> i) & 1 for i in range(A)], np.uint32)
        x = (rng.normal(0, 50, A) * mask).astype(np.float32)
        y, mo = x.copy(), np.zeros(A, np.uint32)
        L.orc_sadct_forward(y, mask, aw, aw, mo)
        assert np.array_equal(mo != 0, md), bits
        assert np.allclose(y, F @ x, rtol=0, atol=2e-4), bits
        z = y.copy(); L.orc_sadct_inverse(z, mask, aw, aw)
        assert np.allclose(z, Gm @ y.astype(np.float64), rtol=0, atol=2e-4), bits
        assert np.allclose(Gm @ F @ x, x, rtol=0, atol=1e-10), bits
        assert np.allclose((F @ Gm)[md][:, md], np.eye(int(md.sum())), atol=1e-12), bits


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_against_oracle_and_second_float32_sample(case):
    ref = G.reference(case)
    m, ro, rs = ref["model"], ref["oracle"], ref["second"]
    assert np.array_equal(ro["nSx"], m["nSx"]) and np.array_equal(ro["use_sadct"] != 0, m["use_sadct"])
    print("%s: R %d, open %d / %d, E_filt oracle %.3g second %.3g, E_w oracle %.3g second %.3g"
          % (case.name, case.R, ro["open_pairs"], ro["pairs"], ro["E_filt"], rs["E_filt"], ro["E_w"], rs["E_w"]))
    for r, what in ((ro, "oracle"), (rs, "second float32 evaluation")):
        assert not r["count_bad"], (what, "survivor counts (group, channel, got, want)", r["count_bad"][:5])
        assert r["E_filt"] < 1e-5, (what, M.where_wrong(case, r, 1e-5))
    assert not ro["weight_bad"], ("oracle", "weights are not 1 / (sigma^2 count) in float32", ro["weight_bad"][:5])
    if case.step == 2 or case.useSD:
        finite = np.isfinite(m["w"])
        for r, what in ((ro, "oracle"), (rs, "second float32 evaluation")):
            # the SD weight subtracts two sums of nSx A k^2 terms: their round-off comes back times the subtraction's condition number
            n_terms = int(m["nSx"].max()) * case.A * case.k * case.k
            lim = 1e-4 * max(1.0, n_terms / 51200.0) * (np.maximum(1.0, m["sd_cond"]) if case.useSD else 1.0) * np.ones_like(m["w"])
            assert (r["rel_w"][finite] < lim[finite]).all() and np.isfinite(r["E_w"]) and not r["huge_bad"], (what, r["E_w"], r["huge_bad"][:5])
    if case.step == 1:
        assert ro["open_pairs"] <= G.OPEN_CAP * ro["pairs"], "more than 5 % of the (group, channel) pairs are open: another seed or a larger sigma"
        assert int((m["ingap"] > 0).sum()) == ro["open_pairs"]     # (the model alone decides which pairs are open)
        if case.section:   # F, G: the survivors are more than a DC per pixel (per patch: BM3D)
            more = m["count"] > (m["nSx"][:, None] if case.bm3d else case.k * case.k)
            print("%s: %d of %d pairs keep more than %s coefficients, median %d" % (case.name, more.sum(), more.size, "nSx" if case.bm3d else "k^2", np.median(m["count"])))
            assert more.mean() >= 0.25, "too few survivors: a smaller sigma or a smaller N (not a higher lambda)"


def test_aggpos_rule_and_special_values():
    by = {c.name: c for c in CASES}
    m = M.run(by["wien-pilot-zero"])
    assert (m["w"] == 1).all() and not m["filt"].any()             # Wiener sum 0: weight 1
    m = M.run(by["wien-pilot-tiny"])
    assert np.isfinite(m["filt"]).all() and (m["w"] > 1e30).all()  # float32 has it inf or nearly
    m = M.run(by["ht-id-haar-k8-sd"])       # the SD weight's res <= 0 -> 0 occurs, and so does res > 0
    assert (m["res"] <= 0).any() and (m["w"][m["res"] <= 0] == 0).all() and (m["w"] > 0).any()
    m = M.run(by["ht-constant"])
    whole = ~m["use_sadct"]
    assert whole.any() and (m["count"][whole] <= 64).all()         # tau_2D = id, the whole window: only the DC of a pixel's 72 values
    c = by["ht-id-haar-k8-edges"]
    pos, present, zero, in_shape, aggpos = M.positions(c)
    assert zero.any() and (aggpos.transpose(1, 2, 0)[zero & in_shape[:, None, :]] != M.ABSENT).all()   # zero patches are aggregated
    pos, present, zero, _, _ = M.positions(by["ht-id-haar-k8-edges-subset"])
    assert not zero.any() and (pos[present] % c.Wb >= c.Wb - c.k).any()


WANT = {   # what the issue's table says a case reaches (the kernels behind the two pre-pass launches)
    "ht-id-haar-k8": [((), "k_group_id_haar_fast+k_group_id_haar_list"), (("ht_reference_order",), "k_group_id_haar+k_group_id_haar_list")],
    "ht-id-hw-k8": [((), "k_group_id_any+k_group_id_any_list")],
    "ht-dct-haar-k8": [((), "k_group_dct8")],
    "ht-bior-haar-k16": [((), "k_group_bior16_haar")], "ht-bior-hw-k16": [((), "k_group_bior16_any")],
    "ht-dct-haar-k16": [((), "k_group_dct16_haar")], "ht-dct-hw-k16": [((), "k_group_dct16_any")],
    "ht-bior-k16-n1": [((), "k_group_bior16_n1")], "ht-dct-k16-n1": [((), "k_group_dct16_n1")],
    "wien-dct-haar-k8": [((), "k_group_dct8w3_u+k_group_dct8w3_list"), (("dct8w_v2",), "k_group_dct8w2<true>"), (("group_generic",), "k_group<2>")],
    "wien-dct-haar-k8-n16": [((), "k_group_dct8w3_u+k_group_dct8w3_list")],
    "wien-dct-hw-k8": [((), "k_group_dct8w2<false>")], "wien-dct-haar-k8-id4": [((), "k_group_dct8w3<false>")],
    "wien-bior-haar-k8": [((), "k_group_dct8w<true>")], "wien-bior-hw-k8": [((), "k_group_dct8w<false>")],
    "ht-dct-k10": [((), "k_group<1>")], "ht-bior-k4": [((), "k_group<1>")],
    "wien-dct-k8-n32-dct5": [((), "k_group_slab<2, WA, MAXN>"), (("no_slab_kernel",), "k_group_big<2, false>")],
    "ht-id-haar-k8-1empty": [((), "k_group_id_haar_sa"), (("no_sa_kernels",), "k_group_id_haar_fast+k_group_id_haar_list")],
    "ht-id-hw-k8-2empty": [((), "k_group_id_any_sa")],
    "wien-dct-haar-k8-1empty": [((), "k_group_dct8w3<true>"), (("no_sa_kernels",), "k_group_dct8w3_u+k_group_dct8w3_list")],
    "ht-bior-k16-n1-1empty": [((), "k_group_bior16_n1_sa")], "ht-dct-k16-n1-2empty": [((), "k_group_dct16_n1_sa")],
    "ht-id-haar-k8-5x5": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight"), (("wide_nosplit",), "k_group_idw<AW, SLAB, false>")],
    "ht-id-haar-k8-5x5-sd": [((), "k_group_idw<AW, SLAB, false>")],
    "ht-dct-haar-k8-n32-5x5": [((), "k_group_slab<1, WA, MAXN>"), (("no_slab_kernel",), "k_group_big<1, false>")],
    "wien-dct-haar-k8-5x5": [((), "k_group_slab<2, WA, MAXN>"), (("no_slab_kernel",), "k_group<2>")],
    # F. 7 x 7 .. 17 x 17
    "ht-id-haar-k8-n8-7x7": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight")],
    "ht-id-haar-k16-9x9": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight")],
    "ht-id-haar-k6-11x11": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight"), (("filt_group_major",), "k_group_idw<AW, SLAB, true>+k_group_idw_weight")],
    "ht-id-haar-k8-c3-13x13": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight")],
    "ht-id-haar-k10-15x15": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight"), (("wide_nosplit",), "k_group_idw<AW, SLAB, false>")],
    "ht-id-haar-k8-15x15-sd": [((), "k_group_idw<AW, SLAB, false>")],
    "ht-id-haar-k8-17x17": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight")],
    "ht-bior-haar-k8-n8-7x7": [((), "k_group_slab<1, WA, MAXN>")], "wien-id-haar-k8-7x7": [((), "k_group_slab<2, WA, MAXN>")],
    "ht-dct-hw-k8-9x9": [((), "k_group_slab<1, WA, MAXN>"), (("no_slab_kernel",), "k_group_big<1, true>")],
    "ht-dct-haar-k12-n2-9x9": [((), "k_group_slab<1, WA, MAXN>")], "wien-dct-haar-k8-n32-9x9": [((), "k_group_slab<2, WA, MAXN>")],
    "wien-dct-haar-k8-11x11": [((), "k_group_slab<2, WA, MAXN>"), (("filt_group_major",), "k_group_slab<2, WA, MAXN>")],
    "wien-dct-haar-k8-n16-13x13": [((), "k_group_slab<2, WA, MAXN>"), (("no_slab_kernel",), "k_group_big<2, true>")],
    "ht-bior-dct5-k8-15x15": [((), "k_group_slab<1, WA, MAXN>")], "wien-dct-haar-k8-n16-17x17": [((), "k_group_slab<2, WA, MAXN>")],
    "ht-bior-haar-k4-7x7": [((), "k_group<1>")], "wien-dct-haar-k8-n2-7x7": [((), "k_group<2>")],
    "ht-dct-haar-k8-9x9-sd": [((), "k_group_big<1, true>")], "wien-dct-haar-k8-9x9-sd": [((), "k_group_big<2, true>")],
    "ht-dct-haar-k10-9x9": [((), "k_group_big<1, true>")],
    "ht-id-haar-k8-9x9-empty": [((), "k_group_idw<AW, SLAB, true>+k_group_idw_weight")],
    "wien-dct-haar-k8-13x13-empty": [((), "k_group_slab<2, WA, MAXN>")],
    # G. per-SAI BM3D
    "bm3d-ht-bior-n16-c3": [((), "k_group_bm3d8<1, true>"), (("group_generic",), "k_group<1>")],
    "bm3d-ht-dct-n32": [((), "k_group_bm3d8<1, false>")], "bm3d-wien-bior-n32": [((), "k_group_bm3d8<2, true>")],
    "bm3d-wien-dct-n16-c3": [((), "k_group_bm3d8<2, false>"), (("group_generic",), "k_group<2>")],
    "bm3d-ht-dct-k12-n16": [((), "k_group<1>")], "bm3d-wien-dct-k12-n16": [((), "k_group<2>")],
}


def test_every_case_reaches_the_kernel_it_is_meant_for():
    by = {c.name: c for c in CASES}
    for name, runs in WANT.items():
        assert [tuple(o) for o, _ in runs] == [tuple(r) for r in by[name].runs], name
        for opt, text in runs:
            assert "+".join(K.expected_kernels(by[name], opt)[2:]) == text, (name, opt)
    reached = {k for c in CASES for r in c.runs for k in K.expected_kernels(c, r)}
    assert reached == set(K.ALL_KERNELS), (sorted(set(K.ALL_KERNELS) - reached), sorted(reached - set(K.ALL_KERNELS)))
    # the templates the trace text does not tell apart: every window side of k_group_idw (both forms from 9 x 9 on share a case
    # table row or two) and of k_group_slab, both MAXN instances, and every slab tier
    runs = [(c, r, K.expected_kernels(c, r)) for c in CASES for r in c.runs]
    idw = {c.aw for c, r, ks in runs if any(k.startswith("k_group_idw<") for k in ks)}
    assert idw == {5, 7, 9, 11, 13, 15, 17}, idw
    assert any(c.aw > 7 and "k_group_idw<AW, SLAB, false>" in ks for c, r, ks in runs)
    slab = [(c, ks) for c, r, ks in runs if any(k.startswith("k_group_slab<") for k in ks)]
    assert {c.aw for c, ks in slab} == {3, 5, 7, 9, 11, 13, 15, 17}
    assert {c.step for c, ks in slab if c.aw >= 7} == {1, 2}
    assert {(c.aw, c.N > 16) for c, ks in slab} >= {(9, True), (9, False), (5, True), (3, True)}
    # slab_log2: every tier a legal configuration reaches is reached by a window of 7 x 7 SAIs or more (1: 17 x 17, Wiener, N = 16)
    tiers = {K.slab_log2(c) for c, ks in slab if c.aw >= 7}
    assert tiers == {1, 2, 3, 4, 5, 6}, tiers
    assert K.slab_log2(by["wien-dct-haar-k8-n16-17x17"]) == 1 and K.slab_log2(by["wien-dct-haar-k8-n32-9x9"]) == 2
    assert {c.tau5 for c, ks in slab if c.aw >= 7} == {M.HAAR, M.HADAMARD, M.DCT} and {c.tau2 for c, ks in slab if c.aw >= 7} == {M.ID, M.DCT, M.BIOR}
    # filt layout: SAI-major from 11 x 11 SAIs on, as in a pass; two of those cases also run group-major
    wide = [c for c in CASES if c.A >= K.SAI_MAJOR_MIN_A]
    assert wide and all(c.sai_major for c in wide) and sum(("filt_group_major",) in c.runs for c in wide) >= 2
    # BM3D: stacks of 2 .. N in equal shares, never one patch
    for c in CASES:
        if c.bm3d and c.R >= 16:
            sizes, n = np.unique(c.self_cnt, return_counts=True)
            assert list(sizes) == [1 << i for i in range(1, c.N.bit_length())] and n.max() - n.min() <= 1, c.name


def test_kernel_list_is_the_source_files():
    """ALL_KERNELS names every __global__ of the five group files (templates by the text their launch site spells)."""
    names = set()
    for f in ("ht", "wiener", "generic", "wide", "slab"):
        src = open(os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_group_%s.hip" % f)).read()
        names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_group\w*)\s*\(", src))
    listed = {re.sub(r"<.*", "", k) for k in K.ALL_KERNELS}
    assert names == listed, (sorted(names - listed), sorted(listed - names))
    # ... and every spelling a dispatcher launches (template arguments included) is listed
    spelled = set()
    for f in ("ht", "wiener", "generic", "wide", "slab"):
        src = open(os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_group_%s.hip" % f)).read()
        spelled |= {x.strip("()") for x in re.findall(r"LFBM5D_LAUNCH\(trace, (\(k_group[^()]*\)|k_group[\w<>]*),", src)}
        assert "hipLaunchKernelGGL" not in src, f
    assert spelled == set(K.ALL_KERNELS), (sorted(spelled - set(K.ALL_KERNELS)), sorted(set(K.ALL_KERNELS) - spelled))


def test_slab_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_group_slab.hip")).read()
    assert int(re.search(r"kSlabFloats = (\d+);", src).group(1)) == K.SLAB_FLOATS
    assert int(re.search(r"kSlabFloatsMax = (\d+);", src).group(1)) == K.SLAB_FLOATS_MAX
    src = open(os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_kernels.h")).read()
    assert int(re.search(r"kSaiMajorMinA = (\d+);", src).group(1)) == K.SAI_MAJOR_MIN_A


def test_gap_constant_is_the_kernels_guard_table():
    src = open(os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_kernels.h")).read()
    body = re.search(r"kHtGuardAbs\[9\]\[4\] = \{(.*?)\};", src, flags=re.S).group(1)
    vals = [float(v) for v in re.findall(r"([0-9.]+e-?[0-9]+)f", body)]
    assert len(vals) == 36 and max(vals) == M.K_GUARD


def test_the_comparison_notices_small_faults():
    """What test_gpu_group.py would say of a kernel that is wrong in one place: each fault below, planted into the oracle's own result
    of one case, breaks the rule meant for it (and the unmodified result breaks none)."""
    case = K.build("faults", 9, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", n_groups=96)
    ref = G.reference(case)
    m, bound = ref["model"], 4 * ref["E_filt"]
    f, w, _, _ = G.oracle_group(case)
    clean = M.compare(case, m, f, w)
    assert M.where_wrong(case, clean, bound) is None and not clean["count_bad"] and not clean["weight_bad"]
    closed = np.flatnonzero((m["ingap"][:, 0] == 0) & (m["count"][:, 0] > 1))
    g, c = int(closed[len(closed) // 2]), 0
    n = int(m["nSx"][g]) - 1
    st = int(np.flatnonzero(m["aggpos"][:, g, n] != M.ABSENT)[-1])
    # one pixel of the last stack slot of one SAI off by 8 E M
    f1 = f.copy()
    f1[g, n, st, c, 37] += np.float32(8 * ref["E_filt"] * m["M"][g, c])
    bad = M.where_wrong(case, M.compare(case, m, f1, w), bound)
    assert bad and (bad["group"], bad["slot"], bad["sai"], bad["channel"], bad["row"], bad["col"]) == (g, n, st, c, 4, 5)
    # one surviving coefficient far from its threshold dropped: the values move, and with the weight following, the count is off
    keep = (np.abs(m["coef"][g, :, :, c]) > 1.5 * m["T"][g, c]) & m["valid"][g, :, :, 0]
    i = tuple(int(x) for x in np.argwhere(keep)[-1])
    X = np.zeros((1,) + m["coef"].shape[1:])
    X[0, i[0], i[1], c, i[2]] = m["coef"][g, i[0], i[1], c, i[2]]
    f2 = f.copy()
    f2[g] -= m["chain"].inv(X, np.array([g]))[0].astype(np.float32)
    r2 = M.compare(case, m, f2, w)
    assert M.where_wrong(case, r2, bound)["group"] == g
    w2 = w.copy()
    w2[g, c] = M.f32_ht_weight(case.sigma[c], np.array([m["count"][g, c] - 1]))[0]
    assert M.compare(case, m, f, w2)["count_bad"] == [(g, c, int(m["count"][g, c]) - 1, int(m["count"][g, c]))]
    # a weight one ulp off its float32 expression
    w3 = w.copy()
    w3[g, c] = np.nextafter(w3[g, c], np.float32(1))
    assert M.compare(case, m, f, w3)["weight_bad"]
    # a patch taken from the neighbouring position
    f4 = f.copy()
    f4[g, n, st, c] = np.roll(f4[g, n, st, c], 1)
    assert M.where_wrong(case, M.compare(case, m, f4, w), bound)


@pytest.mark.parametrize("name", ("wien-dct-haar-k8-13x13-empty", "ht-bior-dct5-k8-15x15", "bm3d-ht-dct-n32", "bm3d-wien-bior-n32"))
def test_the_comparison_notices_small_faults_in_wide_and_bm3d_cases(name):
    """The same on a 13 x 13 window and on the BM3D flavour: a value off by 8 E_filt M, and a patch taken from the neighbouring SAI
    slot (BM3D has one SAI: from the neighbouring stack slot), each planted into the oracle's own result, break the value rule."""
    case = {c.name: c for c in CASES}[name]
    ref = G.reference(case)
    m, bound = ref["model"], 4 * ref["E_filt"]
    f, w, _, _ = G.oracle_group(case)
    assert M.where_wrong(case, M.compare(case, m, f, w), bound) is None
    closed = np.flatnonzero((m["ingap"][:, 0] == 0) & (m["nSx"] > 1)) if case.step == 1 else np.flatnonzero(m["nSx"] > 1)
    # (the group of most survivors: where the threshold leaves a DC only, two SAIs of a shape hold the same patch)
    g, c = int(closed[np.argmax(m["count"][closed, 0])] if case.step == 1 else closed[len(closed) // 2]), 0
    n = int(m["nSx"][g]) - 1
    sais = np.flatnonzero(m["aggpos"][:, g, n] != M.ABSENT)
    st = int(sais[-1])
    f1 = f.copy()
    f1[g, n, st, c, 37] += np.float32(8 * ref["E_filt"] * m["M"][g, c])
    bad = M.where_wrong(case, M.compare(case, m, f1, w), bound)
    assert bad and (bad["group"], bad["slot"], bad["sai"], bad["channel"], bad["row"], bad["col"]) == (g, n, st, c, 37 // case.k, 37 % case.k)
    f2 = f.copy()
    if case.bm3d:
        f2[g, n, st, c] = f[g, n - 1, st, c]
    else:
        f2[g, n, st, c] = f[g, n, int(sais[-2]), c]
    bad = M.where_wrong(case, M.compare(case, m, f2, w), bound)
    assert bad and bad["group"] == g and bad["slot"] == n and bad["sai"] == st
