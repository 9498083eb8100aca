"""The general group kernels' variance-table forms alone (lfbm5d_debug_group_corr, include/lfbm5d_corr.h) against the numpy model
(tests/corr_model.py: tests/group_model.py extended by per-coefficient thresholds, variances and weights).  Run with -m gpu on an
MI355X.

Every case of corr_model.group_cases() runs with a non-trivial table (Gaussian taps of width 0.8) and with the white one:

  - the kernels launched are the _corr ones;
  - non-trivial table: every filtered value aggpos points at within 4 x the float32 round-off of the same model evaluated in float32
    (the rule of tests/test_gpu_group.py; the bound comes from the model, never from the kernel), a coefficient inside the gap that
    the kernel decided the other way added back first (tests/test_corr.py asserts on the CPU that at least 90 % of the pairs have
    none); weights within 4 max(E_w, sqrt(n) eps32), n = nSx A k^2 terms; aggpos and the counters the model's;
  - white table: filt, wgt, aggpos and the counters bit-identical to lfbm5d_debug_group under option group_generic.
"""
import numpy as np
import pytest
import torch

import corr_model as CM
import group_cases as K
import group_model as M

pytestmark = pytest.mark.gpu

CASES = CM.group_cases()
FACTOR = 4
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def launch(ctx, case, acf=None, opt=()):
    """lfbm5d_debug_group_corr with `acf` (None: lfbm5d_debug_group under the options `opt`) of the whole case; filt [R][N][A][C][k2],
    wgt [R][C], aggpos [A][R][N], the kernel text, the two counters."""
    from lfbm5d_amd import core
    R, N, A, C, k2 = case.R, case.N, case.A, case.C, case.k * case.k
    per = N * C * k2
    stride = R * per + 32 if case.sai_major else 0
    filt = torch.full((A * stride if stride else R * A * per,), float("nan"), device="cuda")
    wgt = torch.full((R * C,), -7.0, device="cuda")
    aggpos = torch.full((A * R * N,), SENTINEL, dtype=torch.int32, device="cuda")
    P = core.make_params(*K.params_tuple(case))
    args = (case.step, P, case.aw, case.aw, case.Wb, case.Hb, C, dev(case.noisy.reshape(-1)),
            None if case.basic is None else dev(case.basic.reshape(-1)), dev(case.refs), dev(case.self_idx.reshape(-1)), dev(case.self_cnt),
            dev(case.best.reshape(-1)), torch.from_numpy(case.shape.reshape(-1)).cuda(), filt, wgt, aggpos, case.mask, case.pst)
    kw = dict(fill_quirk=case.fill_quirk, n_refs_total=R, filt_sai_stride=stride)
    for o in opt:
        ctx.set_option(o, 1)
    try:
        text, n_stack, n_sa = ctx.debug_group(*args, **kw) if acf is None else ctx.debug_group_corr(acf, *args, **kw)
    finally:
        for o in opt:
            ctx.set_option(o, None)
    f = filt.cpu().numpy()
    f = f.reshape(A, stride)[:, :R * per].reshape(A, R, N, C, k2).transpose(1, 2, 0, 3, 4) if stride else f.reshape(R, N, A, C, k2)
    return f, wgt.cpu().numpy().reshape(R, C), aggpos.cpu().numpy().view(np.uint32).reshape(A, R, N), text, n_stack, n_sa


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_table_kernels_against_the_model(ctx, case):
    import lfbm5d_amd as L
    acf = L.corr_from_kernel(CM.gaussian_taps(CM.TABLE_TAPS_WIDTH))
    s, v, _ = L.corr_table(acf, case.tau2, case.k)
    assert v.min() < 0.2 and v.max() > 3                     # a table that matters
    ref = CM.reference(case, s, v)
    m = ref["model"]
    f, w, aggpos, text, n_stack, n_sa = launch(ctx, case, acf)
    tag = dict(case=case.name, kernels=text)
    assert text == "+".join(CM.expected_kernels(case)), tag
    assert np.array_equal(aggpos, m["aggpos"]), (tag, "aggpos")
    assert n_stack == int(m["nSx"].sum()) and n_sa == int(m["use_sadct"].sum()), (tag, "counters", n_stack, n_sa)
    res = CM.compare(case, m, f, w, v)
    bound = FACTOR * ref["E_filt"]
    n_terms = m["nSx"].astype(np.float64) * case.A * case.k * case.k
    w_bound = FACTOR * np.maximum(ref["E_w"], np.sqrt(n_terms) * M.EPS32)[:, None]
    print("%s: E_filt gpu %.3g (float32 model %.3g), E_w gpu %.3g (float32 model %.3g), open %d / %d"
          % (case.name, res["E_filt"], ref["E_filt"], res["E_w"], ref["E_w"], res["open_pairs"], res["pairs"]))
    assert res["open_pairs"] <= 0.1 * res["pairs"], tag
    assert M.where_wrong(case, res, bound) is None, (tag, M.where_wrong(case, res, bound))
    assert not res["huge_bad"], (tag, res["huge_bad"][:5])
    bad = ~(res["rel_w"] <= w_bound)
    g, c = (int(x[0]) for x in np.nonzero(bad)) if bad.any() else (0, 0)
    assert not bad.any(), (tag, "weight", dict(group=g, channel=c, got=float(w[g, c]), want=float(m["w"][g, c]), rel=float(res["rel_w"][g, c]),
                                               bound=float(w_bound[g, 0])))
    # the table changed the result: it is not the plain kernels' (the model's weights differ from the plain model's)
    plain = M.run(case)
    assert not np.allclose(plain["w"], m["w"], rtol=1e-3)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_white_table_is_the_general_kernel_bit_for_bit(ctx, case):
    import lfbm5d_amd as L
    f0, w0, a0, text0, n0, s0 = launch(ctx, case, None, ("group_generic",))
    f1, w1, a1, text1, n1, s1 = launch(ctx, case, L.CORR_WHITE)
    assert text1 == "+".join(CM.expected_kernels(case)) and text0 == text1.replace("_corr", ""), (text0, text1)
    assert f0.tobytes() == f1.tobytes() and w0.tobytes() == w1.tobytes() and np.array_equal(a0, a1) and (n0, s0) == (n1, s1), case.name
    # the seam left no table behind: the plain seam afterwards is the plain seam
    f2, w2, a2, text2, n2, s2 = launch(ctx, case, None, ("group_generic",))
    assert text2 == text0 and f2.tobytes() == f0.tobytes() and w2.tobytes() == w0.tobytes()


def test_seam_refusals(ctx):
    import lfbm5d_amd as L
    case = CASES[0]
    bad = np.array(L.CORR_WHITE)
    bad[3, 4] = 0.3
    with pytest.raises(L.LfBm5dError, match="point-symmetric"):
        launch(ctx, case, bad)
    b3 = K.build("corr-refusal-bm3d", 5, step=2, tau2="dct", tau4="id", tau5="hw", k=8, N=4, C=1, nsx="cycle", n_groups=16, bm3d=True)
    from lfbm5d_amd import core
    R, N, A, C, k2 = b3.R, b3.N, b3.A, b3.C, 64
    filt = torch.full((R * A * N * C * k2,), 3.0, device="cuda")
    with pytest.raises(L.LfBm5dError, match="BM3D flavour is not covered"):
        ctx.debug_group_corr(L.CORR_WHITE, b3.step, core.make_params(*K.params_tuple(b3)), 1, 1, b3.Wb, b3.Hb, C, dev(b3.noisy.reshape(-1)),
                             dev(b3.basic.reshape(-1)), dev(b3.refs), dev(b3.self_idx.reshape(-1)), dev(b3.self_cnt), dev(b3.best.reshape(-1)),
                             torch.from_numpy(b3.shape.reshape(-1)).cuda(), filt, torch.zeros(R * C, device="cuda"),
                             torch.zeros(A * R * N, dtype=torch.int32, device="cuda"), b3.mask, b3.pst, n_refs_total=R, bm3d=1)
    assert bool((filt == 3.0).all())
    # after a refused call the plain seam runs the dedicated kernels again: no table is left in the context
    f, w, a, text, n, s = launch(ctx, case)
    assert "_corr" not in text and "k_group<" not in text, text
