"""The group kernels alone against a float64 model of the chain (run with -m gpu on an MI355X).

Every case of tests/group_cases.py goes through lfbm5d_debug_group -- launch_group of a core pass on tables and buffers the test
supplies -- under each of its option sets, and is compared with tests/group_model.py:

  - aggpos, the two counters (sum of nSx, shape-adaptive groups) and the whole-group entries (| 7 << 29) of the group list are the
    model's (windows beyond 7 x 7 SAIs list nothing: the list is read by kernels of 3 x 3 windows only); the kernels launched are the ones the dispatch restated in group_cases.expected_kernels names;
  - hard-threshold step: the survivor count recovered from wgt equals the model's for every (group, channel) without a coefficient
    inside the gap (group_model.gap_of), differs by at most the number of such coefficients otherwise, and wgt is the float32
    evaluation of 1 / (sigma_c^2 count) bit for bit;
  - every filtered value aggpos points at: |filt - model| / M <= 4 x the larger of two float32 samples of the chain's round-off,
    the oracle's and the model's own code in float32 (tests/group_ref.py, asserted on the CPU by tests/test_group_model.py); a
    coefficient inside the gap that the kernel decided the other way is added back first;
  - Wiener and SD weights: relative error <= 4 max(E_w, sqrt(n) eps32), n = nSx A k^2 terms; weights beyond float32's range as large;
  - slots no patch belongs to (stack positions beyond nSx, empty SAIs, SAIs outside the shape) are not compared.

The cases cover the 3 x 3 windows' dedicated kernels, windows of 5 x 5 to 17 x 17 SAIs (every window side of k_group_idw and
k_group_slab, the large shape record, the general kernels' HBM form; from 11 x 11 on filt is SAI-major as in a pass) and the per-SAI
BM3D flavour (A = 1, launched with bm3d set).  The hard-threshold cases of the wide windows run lambda 3.5: default-lambda
decisions on wide windows stay with the whole-pass tests (tests/test_gpu_parity.py), low-sigma decisions with
tests/test_gpu_ht_decisions.py.
"""
import numpy as np
import pytest
import torch

import group_cases as K
import group_model as M
import group_ref as G

pytestmark = pytest.mark.gpu

CASES = K.cases()
FACTOR = 4
SENTINEL = 0x5A5A5A5A
_seen = {}      # kernel texts of every run, for the completeness test


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def launch(ctx, case, opt=()):
    """One lfbm5d_debug_group of the case's launch; returns filt [groups][N][A][C][k2], wgt [R][C], aggpos [A][R][N], the kernel text,
    the two counters and the group list."""
    from lfbm5d_amd import core
    R, N, A, C, k2 = case.R, case.N, case.A, case.C, case.k * case.k
    rb, nb = case.ref_begin, case.launch
    per = N * C * k2
    stride = nb * per + 32 if case.sai_major and "filt_group_major" not in opt else 0    # (the option matters to passes only: here the stride is the layout)
    filt = torch.full((A * stride if stride else nb * A * per,), float("nan"), device="cuda")
    wgt = torch.full((R * C,), -7.0, device="cuda")
    aggpos = torch.full((A * R * N,), SENTINEL, dtype=torch.int32, device="cuda")
    P = core.make_params(*K.params_tuple(case))
    for o in opt:
        ctx.set_option(o, 1)
    try:
        text, n_stack, n_sa = ctx.debug_group(case.step, P, case.aw, case.aw, case.Wb, case.Hb, C, dev(case.noisy.reshape(-1)),
                                              None if case.basic is None else dev(case.basic.reshape(-1)), dev(case.refs),
                                              dev(case.self_idx.reshape(-1)), dev(case.self_cnt), dev(case.best.reshape(-1)),
                                              torch.from_numpy(case.shape.reshape(-1)).cuda(), filt, wgt, aggpos, case.mask, case.pst,
                                              fill_quirk=case.fill_quirk, n_refs_total=R, ref_begin=rb, n_groups=nb,
                                              filt_sai_stride=stride, bm3d=int(case.bm3d))
        lst = ctx.last_group_list()
    finally:
        for o in opt:
            ctx.set_option(o, None)
    f = filt.cpu().numpy()
    if stride:
        f = f.reshape(A, stride)[:, :nb * per].reshape(A, nb, N, C, k2).transpose(1, 2, 0, 3, 4)
    else:
        f = f.reshape(nb, N, A, C, k2)
    return f, wgt.cpu().numpy().reshape(R, C), aggpos.cpu().numpy().view(np.uint32).reshape(A, R, N), text, n_stack, n_sa, lst


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_group_kernels_against_the_model(ctx, case):
    ref = G.reference(case)
    m = ref["model"]
    rb, nb = case.ref_begin, case.launch
    sl = slice(rb, rb + nb)
    bound = FACTOR * ref["E_filt"]
    n_terms = m["nSx"][sl].astype(np.float64) * case.A * case.k * case.k
    w_bound = FACTOR * np.maximum(ref["E_w"], np.sqrt(n_terms) * M.EPS32)[:, None]
    for opt in case.runs:
        f, w, aggpos, text, n_stack, n_sa, lst = launch(ctx, case, opt)
        _seen.setdefault(case.name, set()).update(text.split("+"))
        tag = dict(case=case.name, option=opt, kernels=text)
        assert text == "+".join(K.expected_kernels(case, opt)), tag
        # geometry
        assert np.array_equal(aggpos[:, sl], m["aggpos"][:, sl]), (tag, "aggpos")
        rest = np.ones(case.R, bool)
        rest[sl] = False
        assert (aggpos[:, rest] == SENTINEL).all() and (w[rest] == -7.0).all(), (tag, "rows outside the launch were written")
        assert n_stack == int(m["nSx"][sl].sum()) and n_sa == int(m["use_sadct"][sl].sum()), (tag, "counters", n_stack, n_sa)
        whole = sorted(int(e & 0x1FFFFFFF) for e in lst if e >> 29 == 7)
        # (k_group_shape<true>, the large shape record, lists nothing: only kernels of 3 x 3 windows read the list)
        listed = np.flatnonzero(m["use_sadct"]) if case.A <= K.MAX_A else []
        assert whole == sorted(int(g) for g in listed if rb <= g < rb + nb), (tag, "group list")
        # values
        res = M.compare(case, m, f, w[sl], sl)
        print("%s %s: E_filt gpu %.3g (oracle %.3g, second %.3g), E_w gpu %.3g (oracle %.3g, second %.3g), open %d / %d"
              % (case.name, "+".join(opt) or "default", res["E_filt"], ref["oracle"]["E_filt"], ref["second"]["E_filt"], res["E_w"],
                 ref["oracle"]["E_w"], ref["second"]["E_w"], res["open_pairs"], res["pairs"]))
        assert not res["count_bad"], (tag, "survivor counts (group, channel, got, want)", res["count_bad"][:5])
        assert not res["weight_bad"], (tag, "wgt is not the float32 1 / (sigma^2 count) (group, channel, got, want)", res["weight_bad"][:5])
        assert M.where_wrong(case, res, bound, sl) is None, (tag, M.where_wrong(case, res, bound, sl))
        assert not res["huge_bad"], (tag, "weights the model has beyond float32's range (group, channel, got)", res["huge_bad"][:5])
        if case.step == 2 or case.useSD:
            bad = ~(res["rel_w"] <= w_bound)
            g, c = (int(x[0]) for x in np.nonzero(bad)) if bad.any() else (0, 0)
            assert not bad.any(), (tag, "weight", dict(group=g + rb, channel=c, got=float(w[sl][g, c]), want=float(m["w"][sl][g, c]),
                                                       rel=float(res["rel_w"][g, c]), bound=float(w_bound[g, 0])))


def test_every_group_kernel_was_reached(ctx):
    """The union of the kernel texts over all cases holds every __global__ of the five group files in every spelling a dispatcher
    launches (tests/test_group_model.py ties this list to the sources)."""
    for case in CASES:
        if case.name not in _seen:      # run alone: the texts do not depend on the data
            for opt in case.runs:
                _seen.setdefault(case.name, set()).update(launch(ctx, case, opt)[3].split("+"))
    reached = set().union(*_seen.values())
    assert reached == set(K.ALL_KERNELS), (sorted(set(K.ALL_KERNELS) - reached), sorted(reached - set(K.ALL_KERNELS)))


# ---- the seam is the pipeline: group + aggregation seams on a pass's own tables give the pass's sums ----
def _passes():
    from test_gpu_aggregate import PASSES
    return PASSES


# two wide windows behind the three 3 x 3 passes: (name, step, sigma, parameters, empty SAI, window side, crop)
WIDE_PASSES = [
    ("ht-id-n4-9x9", 1, 25.0, (4, 4, 2, 8, 4, "id", "sadct", "haar"), None, 9, 48),             # group-major filt, the large shape record
    ("wien-dct-n2-11x11-empty-sai", 2, 25.0, (2, 4, 2, 8, 4, "dct", "sadct", "haar"), 7, 11, 40),   # SAI-major filt
]


@pytest.mark.parametrize("i", range(5), ids=["wien-k8-n8", "ht-k16-n4-empty-sai", "ht-k6"] + [p[0] for p in WIDE_PASSES])
def test_group_and_aggregate_seams_give_the_pass(ctx, i):
    import agg_model as AM
    import helpers as Hh
    from lfbm5d_amd import core
    from test_gpu_parity import gpu_pass, window
    if i < 3:
        name, step, sigma, pk, empty = _passes()[i]
        aw = 3
        win, Wb, Hb, Cc = window(sigma, pk, 64)
    else:   # as tests/test_gpu_parity.py's wide-window passes: a textured light field with a real disparity
        name, step, sigma, pk, empty, aw, crop = WIDE_PASSES[i - 3]
        Cc = 3
        _, noisy = Hh.noisy_lf(Hh.textured_lf(aw, aw, crop, crop)[:, :Cc], sigma)
        win, Wb, Hb = Hh.padded_window(noisy, crop, crop, Cc, pk[1] + pk[2])
    N, nSim, nDisp, k, p = pk[:5]
    A, plane = aw * aw, Wb * Hb
    pst = A // 2
    mask = np.ones(A, np.uint32)
    if empty is not None:
        mask[empty] = 0
        if aw > 3:
            win[empty] = 0
    proc = (mask == 0).astype(np.uint32) if aw > 3 else None      # (the schedule marks empty SAIs as processed)
    wide = dict(cst=pst, pst=pst, aw=aw)
    basic = None
    if step == 2:
        n1, d1 = gpu_pass(ctx, 1, sigma, (4,) + pk[1:5] + ("id", "sadct", "haar"), win, None, Wb, Hb, Cc,
                          **(dict(mask=mask, proc=proc, **wide) if aw > 3 else {}))
        basic = np.ascontiguousarray(Hh.estimate(n1, d1, win).astype(np.float32))
    num, den = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc, mask=mask, proc=proc, **wide)
    refs, idx, cnt, best, shape = ctx.last_bm(N, A, plane)
    R = len(refs)
    g = AM.Geom(Wb=Wb, Hb=Hb, C=Cc, A=A, k=k, N=N, p=p, nSim=nSim, nDisp=nDisp, pst=pst, mask=mask)
    assert g.R == R
    per = N * Cc * k * k
    stride = R * per if A >= K.SAI_MAJOR_MIN_A else 0       # the layout of the pass
    filt = torch.full((R * A * per,), float("nan"), device="cuda")
    wgt = torch.zeros(R * Cc, device="cuda")
    aggpos = torch.full((A * R * N,), SENTINEL, dtype=torch.int32, device="cuda")
    d_win = torch.from_numpy(win).cuda().reshape(-1)
    text, _, _ = ctx.debug_group(step, core.make_params(sigma, 2.7, *pk), aw, aw, Wb, Hb, Cc, d_win, None if basic is None else dev(basic.reshape(-1)),
                                 dev(refs), dev(idx.reshape(-1)), dev(cnt), dev(best.reshape(-1)), torch.from_numpy(shape.reshape(-1)).cuda(),
                                 filt, wgt, aggpos, mask, pst, fill_quirk=1, n_refs_total=R, filt_sai_stride=stride)
    if aw > 3:
        assert "k_group_shape<true>" in text, text
    d_num, d_den = torch.zeros(A * Cc * plane, device="cuda"), torch.zeros(A * Cc * plane, device="cuda")
    ctx.debug_aggregate(d_num, d_den, filt, wgt, aggpos, mask, np.zeros(A, np.uint32) if proc is None else proc, n_refs_total=R, ref_begin=0,
                        n_groups=R, n_ref_rows=g.n_ref_rows, n_ref_cols=g.n_ref_cols, Wb=Wb, Hb=Hb, C_=Cc, A=A, k=k, N=N, pst=pst, p=p,
                        nSim=nSim, nDisp=nDisp, filt_sai_stride=stride)
    assert AM.same_bits(d_den.cpu().numpy(), den.reshape(-1)).all(), name
    assert AM.same_bits(d_num.cpu().numpy(), num.reshape(-1)).all(), name


# ---- the seam refuses what the kernels take for granted ----
def _small(bm3d=False):
    if bm3d:
        return K.build("refusals-bm3d", 5, step=2, tau2="dct", tau4="id", tau5="hw", k=8, N=4, C=1, nsx="cycle", n_groups=16, bm3d=True)
    return K.build("refusals", 5, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=4, C=1, nsx="cycle", n_groups=16)


def _outside(case, what):
    bad = (case.Hb - case.k + 1) * case.Wb                      # a row past Hb - k
    if what == "refs":
        case.refs[3] = bad
    elif what == "refs-column":
        case.refs[3] = case.Wb - case.k + 1                     # a column past Wb - k
    elif what == "self_idx":
        g = int(np.flatnonzero(case.self_cnt > 1)[0])
        case.self_idx[g, 1] = bad
    elif what == "self_idx-plane":
        g = int(np.flatnonzero(case.self_cnt > 1)[0])
        case.self_idx[g, 1] = case.Wb * case.Hb + 5
    else:
        case.best[2, case.refs[5]] = bad


BAD = [
    ("null-noisy", dict(null="noisy"), "NULL"), ("null-basic-step2", dict(null="basic"), "NULL"), ("null-refs", dict(null="refs"), "NULL"),
    ("null-self_idx", dict(null="self_idx"), "NULL"), ("null-self_cnt", dict(null="self_cnt"), "NULL"),
    ("null-best", dict(null="best"), "NULL"), ("null-shape", dict(null="shape"), "NULL"), ("null-filt", dict(null="filt"), "NULL"),
    ("null-wgt", dict(null="wgt"), "NULL"), ("null-aggpos", dict(null="aggpos"), "NULL"), ("null-mask", dict(null="mask"), "NULL"),
    ("C-2", dict(C=2), "chnls"), ("k-1", dict(k=1), "patch size"), ("k-33", dict(k=33), "patch size"),
    ("N-3", dict(N=3), "power of two"), ("N-64", dict(N=64), "power of two"),
    ("bm3d-cnt-1", dict(bm3d=True, cnt=1), "BM3D stack of one patch"),
    ("cnt-0", dict(cnt=0), "stack size"), ("cnt-3", dict(cnt=3), "stack size"), ("cnt-above-N", dict(cnt=8), "stack size"),
    ("refs-outside", dict(outside="refs"), "reference patch lies outside"),
    ("refs-column-outside", dict(outside="refs-column"), "reference patch lies outside"),
    ("self_idx-outside", dict(outside="self_idx"), "stack entry"), ("self_idx-beyond-plane", dict(outside="self_idx-plane"), "stack entry"),
    ("best-outside", dict(outside="best"), "disparity match"),
    ("pst-not-in-mask", dict(pst_empty=True), "pst is not an SAI of the mask"), ("pst-beyond-window", dict(pst=9), "pst is not"),
    ("groups-past-the-list", dict(ref_begin=3), "outside the reference list"),
    ("filt-too-small", dict(filt_floats=1024), "filt is smaller"), ("wgt-too-small", dict(short="wgt"), "wgt is smaller"),
    ("aggpos-too-small", dict(short="aggpos"), "aggpos is smaller"), ("window-too-small", dict(short="noisy"), "noisy / basic are smaller"),
    ("tables-too-small", dict(short="best"), "best / shape are smaller"),
    ("window-4x4", dict(aw=4), "angular search window"), ("window-19x19", dict(aw=19), "angular search window"),
    ("step-3", dict(step=3), "step must be"),
    ("sai-major-on-3x3", dict(sai_major=True), "SAI-major filt is written by the general kernels only"),
    ("Wb-65536", dict(Wb=65536), "65535"), ("Hb-65536", dict(Hb=65536), "65535"),
    ("window-smaller-than-a-patch", dict(Wb=4), "smaller than a patch"),
    ("offsets-beyond-32-bits", dict(aw=17, N=32, k=32, C=3, R=160), "beyond 32 bits"),
    ("null-params", dict(null_field="params"), "NULL"), ("null-counters", dict(null_field="counters"), "NULL"),
]


def _call(ctx, case, t, change):
    from lfbm5d_amd import core
    pt = list(K.params_tuple(case))
    pt[2], pt[5] = change.get("N", case.N), change.get("k", case.k)
    aw = change.get("aw", case.aw)
    R = change.get("R", case.R)
    stride = R * case.N * case.C * case.k * case.k if change.get("sai_major") else 0
    return ctx.debug_group(change.get("step", case.step), core.make_params(*pt), aw, aw, change.get("Wb", case.Wb),
                           change.get("Hb", case.Hb), change.get("C", case.C),
                           t["noisy"], t["basic"], t["refs"], t["self_idx"], t["self_cnt"], t["best"], t["shape"], t["filt"], t["wgt"],
                           t["aggpos"], t["mask"], change.get("pst", case.pst), fill_quirk=1, n_refs_total=R,
                           ref_begin=change.get("ref_begin", 0), n_groups=R, filt_floats=change.get("filt_floats"),
                           filt_sai_stride=stride, bm3d=int(case.bm3d), null=(change["null_field"],) if "null_field" in change else ())


def _tensors(case):
    per = case.N * case.A * case.C * case.k * case.k
    return dict(noisy=dev(case.noisy.reshape(-1)), basic=dev(case.basic.reshape(-1)), refs=dev(case.refs),
                self_idx=dev(case.self_idx.reshape(-1)), self_cnt=dev(case.self_cnt), best=dev(case.best.reshape(-1)),
                shape=torch.from_numpy(case.shape.reshape(-1)).cuda(), filt=torch.full((case.R * per,), 3.0, device="cuda"),
                wgt=torch.full((case.R * case.C,), 5.0, device="cuda"),
                aggpos=torch.full((case.A * case.R * case.N,), SENTINEL, dtype=torch.int32, device="cuda"), mask=case.mask.copy())


@pytest.mark.parametrize("name,change,message", BAD, ids=[b[0] for b in BAD])
def test_seam_refuses_invalid_arguments(ctx, name, change, message):
    import lfbm5d_amd as L
    change = dict(change)
    bm3d = bool(change.pop("bm3d", False))
    case = _small(bm3d)
    if "cnt" in change:
        case.self_cnt[2] = change["cnt"]
    if "outside" in change:
        _outside(case, change["outside"])
    t = _tensors(case)
    if change.get("pst_empty"):
        t["mask"][case.pst] = 0
    if "aw" in change:      # (the host mask has an entry per SAI of the window asked for)
        t["mask"] = np.ones(change["aw"] ** 2, np.uint32)
    if "R" in change:       # (a longer list: the tables of the list are as long)
        t["refs"] = torch.zeros(change["R"], dtype=torch.int32, device="cuda")
        t["self_cnt"] = torch.ones(change["R"], dtype=torch.int32, device="cuda")
        t["self_idx"] = torch.zeros(change["R"] * change["N"], dtype=torch.int32, device="cuda")
    elif "N" in change:
        t["self_idx"] = torch.zeros(case.R * max(case.N, change["N"]), dtype=torch.int32, device="cuda")
    if "null" in change:
        t[change["null"]] = None
    if "short" in change:
        t[change["short"]] = t[change["short"]][:-1].clone()
    keep = {n: t[n] for n in ("filt", "wgt") if t[n] is not None}
    with pytest.raises(L.LfBm5dError, match=message):
        _call(ctx, case, t, change)
    # nothing was launched: filt and wgt are as they were, and the same call without the fault runs
    for n, x in keep.items():
        assert bool((x == (3.0 if n == "filt" else 5.0)).all()), n
    good = _small(bm3d)
    t = _tensors(good)
    text, n_stack, n_sa = _call(ctx, good, t, {})
    assert text.startswith("k_group_pos+k_group_shape<false>+" + ("k_group_bm3d8<2, false>" if bm3d else "k_group_dct8w3_u")) and n_stack == int(good.self_cnt.sum())
    assert not bool((t["wgt"] == 5.0).any()) and not bool((t["filt"] == 3.0).all())
