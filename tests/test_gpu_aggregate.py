"""The aggregation kernel alone against its in-order model (run with -m gpu on an MI355X).

Every case of tests/agg_cases.py goes through lfbm5d_debug_aggregate -- the launch of a core pass on buffers the test supplies -- and
num / den must equal tests/agg_model.py's float32 scatter BIT FOR BIT (two NaNs count as equal, agg_model.same_bits), under the
default build options, with 64-bit gather addresses (agg_64bit) and with the one-candidate-per-lane scan (agg_scalar_scan); the
read-only inputs must come back unchanged.  tests/test_agg_model.py proves on the CPU which path of the kernel each case reaches.
Three real core passes tie the model to the pipeline: the pass's own den equals the model's on the pass's own positions and weights."""
import numpy as np
import pytest
import torch

import agg_cases as K
import agg_model as M
import helpers as Hh

pytestmark = pytest.mark.gpu

CASES = K.template_cases() + K.special_cases()
OPTIONS = (None, "agg_64bit", "agg_scalar_scan")
_model = {}
_sparse_dev = {}


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def model(case):
    if case.name not in _model:
        g = case.g
        _model[case.name] = M.aggregate(g, case.num0, case.den0, K.patches_of(case), case.wgt, case.aggpos, M.kaiser_table(g.k))
    return _model[case.name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()


def sparse_filt_on_device(case):
    """The dense filt of a case given by its present patches: K.sparse_value of every element, evaluated on the device in integer
    arithmetic; the present patches are read back and must be the ones the model uses."""
    g = case.g
    n = g.R * g.N * g.A * g.C * g.k * g.k
    filt = torch.empty(n, dtype=torch.float32, device="cuda")
    for b in range(0, n, 1 << 24):
        i = torch.arange(b, min(n, b + (1 << 24)), dtype=torch.int64, device="cuda")
        filt[b:b + (1 << 24)] = (((i * 2654435761 + 40503) % (1 << 32) >> 13) % 511 - 255).to(torch.float32)
    pk = g.C * g.k * g.k
    keys = list(case.sparse)
    base = torch.tensor([((gi * g.N + n_) * g.A + st) * pk for gi, n_, st in keys], dtype=torch.int64, device="cuda")
    got = filt[base[:, None] + torch.arange(pk, device="cuda")[None, :]].cpu().numpy()
    assert np.array_equal(got, np.stack([case.sparse[key].reshape(-1) for key in keys]))
    return filt


def run_case(ctx, case):
    """The case's launches in order; returns num, den.  Asserts that the read-only inputs are unchanged."""
    g = case.g
    d_num, d_den, d_wgt, d_pos = dev(case.num0), dev(case.den0), dev(case.wgt), dev(case.aggpos)
    if case.sparse is not None and case.name not in _sparse_dev:
        _sparse_dev[case.name] = sparse_filt_on_device(case)   # (filled once; every launch below checks that it stays as it was)
    whole = _sparse_dev.get(case.name)
    for rb, nb in case.bands:
        if whole is not None:
            d_filt, stride = whole, 0
        else:
            f, stride = K.band_filt(case, rb, nb)
            d_filt = dev(f)
        keep = [t.clone() for t in (d_wgt, d_pos, d_filt)]
        ctx.debug_aggregate(d_num, d_den, d_filt, d_wgt, d_pos, g.mask, g.proc, n_refs_total=g.R, ref_begin=rb, n_groups=nb,
                            n_ref_rows=g.n_ref_rows, n_ref_cols=g.n_ref_cols, Wb=g.Wb, Hb=g.Hb, C_=g.C, A=g.A, k=g.k, N=g.N, pst=g.pst,
                            p=g.p, nSim=g.nSim, nDisp=g.nDisp, filt_sai_stride=stride, irregular=g.irregular, wchan0=g.wchan0,
                            direct=g.direct, lf_stride=g.lf_stride, sai=g.sai)
        for t, t0 in zip((d_wgt, d_pos, d_filt), keep):
            assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), "the launch wrote to a read-only input"
    return d_num.cpu().numpy(), d_den.cpu().numpy()


def where_wrong(case, got, want):
    """The first mismatch as (slot or SAI, channel, row, column) -- what a failing rewrite needs to see."""
    bad = np.flatnonzero(~M.same_bits(got, want))
    if not len(bad):
        return None
    g = case.g
    i = int(bad[0])
    if g.direct:
        W, H = g.Wb - 2 * g.nHW, g.Hb - 2 * g.nHW
        s, r = divmod(i, g.lf_stride)
    else:
        W, H = g.Wb, g.Hb
        s, r = divmod(i, g.C * W * H)
    c, r = divmod(r, W * H)
    return dict(case=case.name, mismatches=len(bad), sai=s, channel=c, row=r // W, col=r % W, got=float(got[i]), want=float(want[i]))


def check_case(ctx, case):
    num_m, den_m = model(case)
    first = None
    for opt in OPTIONS:
        if opt:
            ctx.set_option(opt, 1)
        try:
            num, den = run_case(ctx, case)
        finally:
            if opt:
                ctx.set_option(opt, None)
        assert where_wrong(case, den, den_m) is None, (opt, "den", where_wrong(case, den, den_m))
        assert where_wrong(case, num, num_m) is None, (opt, "num", where_wrong(case, num, num_m))
        if first is None:
            first = (num, den)
        assert M.same_bits(num, first[0]).all() and M.same_bits(den, first[1]).all()
    return first


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_aggregate_equals_the_model_bit_for_bit(ctx, case):
    num, den = check_case(ctx, case)
    g = case.g
    # what the launch must not touch: masked and processed slots; direct form: SAIs outside the window, the slack between SAIs
    untouched = np.ones(len(num), bool)
    for st in M.live_slots(g):
        if g.direct:
            o = int(g.sai[st]) * g.lf_stride
            untouched[o:o + g.C * (g.Wb - 2 * g.nHW) * (g.Hb - 2 * g.nHW)] = False
        else:
            untouched[st * g.C * g.Wb * g.Hb:(st + 1) * g.C * g.Wb * g.Hb] = False
    assert untouched.any() and not untouched.all()
    assert np.array_equal(num[untouched].view(np.uint32), case.num0[untouched].view(np.uint32))
    assert np.array_equal(den[untouched].view(np.uint32), case.den0[untouched].view(np.uint32))


def test_bands_give_the_single_launch(ctx):
    """The same pass as one launch and as row bands launched in raster order, filt holding one band at a time: the same bits."""
    for case in (c for c in CASES if len(c.bands) > 1):
        banded = run_case(ctx, case)
        bands, case.bands = case.bands, [(0, case.g.R)]
        try:
            single = run_case(ctx, case)
        finally:
            case.bands = bands
        assert M.same_bits(banded[0], single[0]).all() and M.same_bits(banded[1], single[1]).all()


@pytest.mark.xfail(strict=True, reason="k_aggregate adds uncovered pixels as 0 * (nearest covered element): a NaN or inf at a patch's rim "
                   "spreads to the uncovered pixels of the tiles it overlaps; adding exactly nothing cost 8 % of the headline job "
                   "(profiles/aggregate_isolated.txt), so the divergence stays (DESIGN.md)")
def test_nonfinite_filt_stays_on_covered_pixels(ctx):
    """One patch holds a NaN and one an inf, at corner elements -- the ones the kernel's clamped reads of uncovered pixels land on.  In
    the model (and in the reference's scatter) only the pixels those patches cover change."""
    check_case(ctx, K.nonfinite_case())


# ---- the model against the real pipeline: den of three core passes ----
PASSES = [
    ("wien-k8-n8", 2, 25.0, (8, 6, 2, 8, 3, "dct", "sadct", "haar"), None),
    ("ht-k16-n4-empty-sai", 1, 25.0, (4, 6, 2, 16, 3, "bior", "sadct", "haar"), 2),   # an empty SAI: every group is shape-adaptive
    ("ht-k6", 1, 25.0, (8, 6, 2, 6, 3, "id", "sadct", "haar"), None),
]


@pytest.mark.parametrize("name,step,sigma,pk,empty", PASSES, ids=[p[0] for p in PASSES])
def test_den_of_a_real_pass_equals_the_model(ctx, name, step, sigma, pk, empty):
    from test_gpu_parity import gpu_pass, window
    win, Wb, Hb, Cc = window(sigma, pk, 64)
    N, nSim, nDisp, k, p = pk[:5]
    A, pst, plane = 9, 4, Wb * Hb
    mask = np.ones(A, np.uint32)
    if empty is not None:
        mask[empty] = 0
    basic = None
    if step == 2:   # a plausible pilot: the hard-threshold estimate of this window
        n1, d1 = gpu_pass(ctx, 1, sigma, (4,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc)
        basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    _, den = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc, mask=mask)
    refs, idx, cnt, best, shape = ctx.last_bm(N, A, plane)
    R = len(refs)
    wgt = ctx.last_weights(R, Cc)
    # the rule of k_group_pos (lfbm5d_group_generic.hip:37-52); tau_4D is sadct in all three passes
    aggpos = np.full((A, R, N), M.ABSENT, np.uint32)
    used = np.arange(N)[None, :] < cnt[:, None]
    ind = np.where(used, idx, 0).astype(np.int64)
    for st in range(A):
        if not mask[st]:
            continue
        pos = ind if st == pst else best[st][ind].astype(np.int64)
        in_shape = np.ones(R, bool) if st == pst else shape[st][refs] != 0
        ok = used & in_shape[:, None] & (pos != M.ABSENT)
        aggpos[st] = np.where(ok, (pos // Wb) << 16 | pos % Wb, M.ABSENT).astype(np.uint32)
    g = M.Geom(Wb=Wb, Hb=Hb, C=Cc, A=A, k=k, N=N, p=p, nSim=nSim, nDisp=nDisp, pst=pst, mask=mask)
    assert g.R == R
    refs_yx = np.stack([refs // Wb, refs % Wb], -1).astype(np.int64)
    assert M.check_reach(g, aggpos, refs_yx) == 0
    zeros = np.zeros(A * Cc * plane, np.float32)
    patch0 = np.zeros((Cc, k * k), np.float32)
    _, den_m = M.aggregate(g, zeros, zeros, lambda gi, n, st: patch0, wgt, aggpos, M.kaiser_table(k))
    assert den_m.any()
    assert np.array_equal(den.reshape(-1).view(np.uint32), den_m.view(np.uint32))


# ---- the seam refuses what the kernel takes for granted ----
def _valid(**over):
    g = M.Geom(Wb=40, Hb=40, C=1, A=9, k=8, N=4, p=3, nSim=5, nDisp=2)
    a = dict(n_refs_total=g.R, ref_begin=0, n_groups=g.R, n_ref_rows=g.n_ref_rows, n_ref_cols=g.n_ref_cols, Wb=40, Hb=40, C_=1, A=9, k=8,
             N=4, pst=4, p=3, nSim=5, nDisp=2)
    a.update(over)
    return g, a


BAD = [
    ("N-not-pow2", dict(N=3), "power of two"),
    ("N-64", dict(N=64), "power of two"),
    ("k-1", dict(k=1), "patch size"),
    ("k-33", dict(k=33), "patch size"),
    ("C-2", dict(C_=2), "chnls"),
    ("Wb-65536", dict(Wb=65536), "65535"),
    ("Hb-65536", dict(Hb=65536), "65535"),
    ("groups-past-the-list", dict(ref_begin=3), "outside the reference list"),
    ("window-too-small", dict(Wb=22), "smaller than 2 nHW"),
    ("null-num", dict(null="num"), "NULL"),
    ("null-den", dict(null="den"), "NULL"),
    ("null-filt", dict(null="filt"), "NULL"),
    ("null-wgt", dict(null="wgt"), "NULL"),
    ("null-aggpos", dict(null="aggpos"), "NULL"),
    ("null-mask", dict(null="mask"), "NULL"),
    ("null-proc", dict(null="proc"), "NULL"),
    ("null-sai-direct", dict(direct=1, lf_stride=26 * 26), "NULL"),
    ("grid-not-the-windows", dict(n_ref_rows=5), "reference grid"),
    ("filt-too-small", dict(filt_bytes=1024), "filt is smaller"),
]


@pytest.mark.parametrize("name,change,message", BAD, ids=[b[0] for b in BAD])
def test_seam_refuses_invalid_arguments(ctx, name, change, message):
    import lfbm5d_amd as L
    change = dict(change)
    null = change.pop("null", None)
    g, a = _valid(**change)
    t = dict(num=torch.full((9 * 40 * 40,), 3.0, device="cuda"), den=torch.full((9 * 40 * 40,), 5.0, device="cuda"),
             filt=torch.ones(g.R * 4 * 9 * 64, device="cuda"), wgt=torch.ones(g.R, device="cuda"),
             aggpos=torch.full((9 * g.R * 4,), (12 << 16) | 12, dtype=torch.int32, device="cuda"),
             mask=np.ones(9, np.uint32), proc=np.zeros(9, np.uint32))
    before = t["num"].clone(), t["den"].clone()
    if null:
        t[null] = None
    with pytest.raises(L.LfBm5dError, match=message):
        ctx.debug_aggregate(t["num"], t["den"], t["filt"], t["wgt"], t["aggpos"], t["mask"], t["proc"], **a)
    # nothing was launched: the sums are as they were, and the same arguments without the fault run
    for x, x0 in zip((t["num"], t["den"]), before):
        assert x is None or torch.equal(x, x0)
    g, a = _valid()
    ctx.debug_aggregate(before[0], before[1], t["filt"] if t["filt"] is not None else torch.ones(g.R * 4 * 9 * 64, device="cuda"),
                        torch.ones(g.R, device="cuda"), torch.full((9 * g.R * 4,), (12 << 16) | 12, dtype=torch.int32, device="cuda"),
                        np.ones(9, np.uint32), np.zeros(9, np.uint32), **a)
    assert float(before[1].max()) > 5.0
