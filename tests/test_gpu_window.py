"""The window-schedule kernels alone against their exact float32 model (run with -m gpu on an MI355X).

Every case of tests/window_cases.py goes through lfbm5d_debug_window -- one launcher of lfbm5d_window.hip on buffers the test supplies
-- and every buffer must equal tests/window_model.py's prediction BIT FOR BIT (two NaNs count as equal): what the op writes, what it
must leave alone (SAIs outside the list, masked-out slots, the slack between SAIs, the guard words around every buffer) and its
read-only inputs.  The fused kernels equal the chains of plain kernels the header comments of lfbm5d_kernels.h promise, through the
same seam; the seam refuses what the kernels take for granted; the library refuses images smaller than the search range on every entry
that pads; one real ycbcr pass ties the model's colour space to the pipeline.  tests/test_window_model.py proves on the CPU which edge
each case reaches."""
import numpy as np
import pytest
import torch

import helpers as Hh
import window_cases as K
import window_model as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
CASES = K.all_cases()
GUARD = 64
SENT_BITS = int(np.array([K.SENT], F).view(np.uint32)[0])
u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def launch(ctx, op, bufs, alias=None, lst=None, slot_mask=None, **kw):
    """One lfbm5d_debug_window on device copies of `bufs` (name -> flat float32 / uint32 host array, None: a NULL pointer), each
    between guard words; returns name -> the buffer's contents afterwards.  Asserts that the guards are intact."""
    dev = {}
    for name, v in bufs.items():
        if v is not None:
            full = np.concatenate([np.full(GUARD, SENT_BITS, np.uint32), u32(v), np.full(GUARD, SENT_BITS, np.uint32)])
            dev[name] = torch.from_numpy(full.view(np.int32) if v.dtype == np.uint32 else full.view(F)).cuda()
    args = {name: t[GUARD:len(t) - GUARD] for name, t in dev.items()}
    for name, target in (alias or {}).items():
        args[name] = args[target]
    try:
        ctx.debug_window(op, list=lst, slot_mask=slot_mask, **args, **kw)
    finally:
        after = {name: t.cpu().numpy() for name, t in dev.items()}
        for name, a in after.items():
            g = np.concatenate([u32(a)[:GUARD], u32(a)[-GUARD:]])
            assert (g == SENT_BITS).all(), f"{op}: the launch wrote outside {name}"
    return {name: a[GUARD:len(a) - GUARD] for name, a in after.items()}


def first_wrong(got, want):
    bad = np.flatnonzero(~M.same_bits(got, want))
    return None if not len(bad) else dict(mismatches=len(bad), index=int(bad[0]), got=float(got[bad[0]]), want=float(want[bad[0]]))


def check(case, after, want):
    """every buffer of the case against the model's prediction `want`; whatever the model does not mention stays exactly as it was"""
    for name, v in case.bufs.items():
        if v is None:
            continue
        got = after[name]
        if name == "counters" and case.op == "window_end":   # partial counters: the count is their sum, its spread is free
            assert int(u32(got).astype(np.uint64).sum()) == int(v.astype(np.uint64).sum()) + want["counters"], (case.name, "count")
        elif name == "counters" and case.op in ("count_zeros", "count_denoised"):
            assert np.array_equal(u32(got), v + want["counters"]), (case.name, u32(got) - v, want["counters"])
        elif name in want:
            if v.dtype == np.uint32:
                assert np.array_equal(u32(got), want[name]), (case.name, name)
            else:
                assert first_wrong(got, want[name]) is None, (case.name, name, first_wrong(got, want[name]))
        else:
            assert np.array_equal(u32(got), u32(v)), (case.name, name, "the launch wrote to a read-only input")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_model_bit_for_bit(ctx, case):
    want = K.expected(case)
    after = launch(ctx, case.op, case.bufs, case.alias, case.lst, case.slot_mask, **case.kw)
    check(case, after, want)
    # the case is not vacuous: the op changed something it was meant to write
    assert any(not np.array_equal(u32(after[n]), u32(case.bufs[n])) for n in after if n in want or n == "counters") or case.kw.get("rh") == 0


# ---- the fused kernels equal the chains of plain kernels, through the same seam ----
def _geom(case):
    g = case.kw
    imgb, planeb = g["C"] * (g["W"] + 2 * g["N"]) * (g["H"] + 2 * g["N"]), (g["W"] + 2 * g["N"]) * (g["H"] + 2 * g["N"])
    return g, imgb, planeb


BEGIN = [c for c in CASES if c.op == "window_begin" and "sums-form" in c.edges]
END = [c for c in CASES if c.op == "window_end" and "sums-form" in c.edges]


@pytest.mark.parametrize("case", BEGIN, ids=[c.name for c in BEGIN])
def test_window_begin_equals_symetrize_multi_and_estimate_multi(ctx, case):
    g, imgb, planeb = _geom(case)
    n = len(case.lst)
    fused = launch(ctx, "window_begin", case.bufs, lst=case.lst, **g)
    geo = {**g, "w_stride": imgb}     # (k_estimate_multi takes the slots back to back)
    pads = {}
    for src in ("noisy", "basic", "num", "den"):
        if case.bufs[src] is not None:
            pads[src] = launch(ctx, "symetrize_multi", dict(noisy=case.bufs[src], w_noisy=K.sent(n * imgb)), lst=case.lst, **geo)["w_noisy"]
            for i in range(n):
                a = fused["w_" + src][i * g["w_stride"]:i * g["w_stride"] + imgb]
                assert np.array_equal(u32(a), u32(pads[src][i * imgb:(i + 1) * imgb])), (case.name, src, i)
    live = (case.lst != K.EMPTY).astype(np.uint32)
    est = launch(ctx, "estimate_multi", dict(w_num=pads["num"], w_den=pads["den"], w_noisy=pads["basic" if "basic" in pads else "noisy"],
                                             est=K.sent(n * planeb)), slot_mask=live, n=planeb, C=g["C"])["est"]
    assert M.same_bits(est, fused["est"]).all()


@pytest.mark.parametrize("case", END, ids=[c.name for c in END])
def test_window_end_equals_unsymetrize_multi_and_count_denoised(ctx, case):
    g, imgb, _ = _geom(case)
    fused = launch(ctx, "window_end", case.bufs, lst=case.lst, **g)
    for name in ("num", "den"):
        back = launch(ctx, "unsymetrize_multi", dict(w_noisy=case.bufs["w_" + name], out=case.bufs[name]), lst=case.lst, **g)["out"]
        assert np.array_equal(u32(back), u32(fused[name])), (case.name, name)
    live = (case.lst != K.EMPTY).astype(np.uint32)
    cnt = launch(ctx, "count_denoised", dict(w_den=case.bufs["w_den"], counters=np.zeros(1, np.uint32)), slot_mask=live, **g)["counters"]
    added = int(u32(fused["counters"]).astype(np.uint64).sum()) - int(case.bufs["counters"].astype(np.uint64).sum())
    assert int(u32(cnt)[0]) == added > 0


JOB_ENDS = [c for c in CASES if c.op in ("finalize", "output")]


@pytest.mark.parametrize("case", JOB_ENDS, ids=[c.name for c in JOB_ENDS])
def test_finalize_and_output_equal_estimate_lf_and_the_colour_kernels(ctx, case):
    g = case.kw
    b = {k: case.bufs[case.alias.get(k, k)] for k in list(case.bufs) + list(case.alias)}
    fused = launch(ctx, case.op, case.bufs, case.alias, lst=case.lst, **g)
    n_sai, n, img = K._n_sai_of(case), g["lf_stride"], 3 * g["W"] * g["H"]
    dmask = np.zeros(n_sai, np.uint32)
    dmask[case.lst] = 1
    whole = lambda v: np.concatenate([v, K.sent(n_sai * n - len(v))])
    geo = dict(W=g["W"], H=g["H"], C=3, cs=g["cs"], n_sai=n_sai, lf_stride=n)
    col = lambda v, fwd: launch(ctx, "color", dict(noisy=v, dmask=dmask), forward=fwd, **geo)["noisy"] if g["colour"] else v
    e = launch(ctx, "estimate_lf", dict(num=whole(b["num"]), den=whole(b["den"]), sub=whole(b["sub"]), out=K.sent(n_sai * n), dmask=dmask),
               n=n, n_sai=n_sai)["out"][:len(b["num"])]
    image = (np.arange(len(e)) % n) < img   # (estimate_lf also forms the slack between the SAIs)
    same = lambda got, ref: (M.same_bits(got, ref) | ~image).all()
    if case.op == "finalize":
        assert same(col(col(e, 0), 1), fused["basic"])
    else:
        assert same(col(e, 0), fused["out"])
        noisy_name = case.alias.get("noisy_dst", "noisy_dst")
        assert same(np.where(fused[noisy_name] == K.SENT, K.SENT, col(b["noisy"], 0)), fused[noisy_name])
        if b["basic"] is not None:
            assert same(col(b["basic"], 0), fused["basic"])


# ---- the seam refuses what the kernels take for granted ----
def _base(op):
    return next(c for c in CASES if c.op == op)


def _short(name, by=1):
    return lambda c: {name: c.bufs[name][:len(c.bufs[name]) - by]}


BAD = [   # (id, op, changes: kw / null / bufs (a function of the case) / lst / slot_mask, message)
    ("null-input", "symetrize_multi", dict(null=["noisy"]), "NULL pointer"),
    ("null-output", "symetrize_multi", dict(null=["w_noisy"]), "NULL pointer"),
    ("null-list", "window_end", dict(lst=None), "NULL pointer"),
    ("null-slot-mask", "count_denoised", dict(slot_mask=None), "NULL pointer"),
    ("null-counters", "window_begin", dict(null=["counters"]), "NULL pointer"),
    ("null-est", "estimate", dict(null=["est"]), "NULL pointer"),
    ("null-one-window-sum", "window_end", dict(null=["w_num"]), "NULL pointer"),
    ("null-noisy-dst", "output", dict(null=["noisy_dst"], alias={}), "NULL pointer"),
    ("C-2", "symetrize", dict(kw=dict(C=2)), "chnls must be 1 or 3"),
    ("C-0", "window_end", dict(kw=dict(C=0)), "chnls must be 1 or 3"),
    ("finalize-C-1", "finalize", dict(kw=dict(C=1)), "three channels"),
    ("output-C-1", "output", dict(kw=dict(C=1)), "three channels"),
    ("color-C-1", "color", dict(kw=dict(C=1)), "three channels"),
    ("roundtrip-C-1", "color_roundtrip", dict(kw=dict(C=1)), "three channels"),
    ("color-rgb", "color", dict(kw=dict(cs=3)), "yuv, ycbcr and opp"),
    ("finalize-bad-space", "finalize", dict(kw=dict(cs=7)), "yuv, ycbcr and opp"),
    ("estimate-n-0", "estimate", dict(kw=dict(n=0)), "n must be"),
    ("W-0", "symetrize", dict(kw=dict(W=0)), "must not be 0"),
    ("H-0", "window_begin", dict(kw=dict(H=0)), "must not be 0"),
    ("symetrize-N-above-W", "symetrize", dict(kw=dict(W=15)), "padding N is larger"),
    ("symetrize-N-above-H", "symetrize", dict(kw=dict(H=15)), "padding N is larger"),
    ("symetrize_multi-N-above-W", "symetrize_multi", dict(kw=dict(W=6)), "padding N is larger"),
    ("window_begin-N-above-H", "window_begin", dict(kw=dict(H=6)), "padding N is larger"),
    ("window_end-k-above-W", "window_end", dict(kw=dict(k=65)), "patch size k"),
    ("window_end-k-above-H", "window_end", dict(kw=dict(k=33)), "patch size k"),
    ("count_denoised-k-above-W", "count_denoised", dict(kw=dict(k=201)), "patch size k"),
    ("count_denoised-k-above-H", "count_denoised", dict(kw=dict(k=181)), "patch size k"),
    ("list-290", "symetrize_multi", dict(lst=np.zeros(290, np.uint32)), "more than 289"),
    ("slots-290", "estimate_multi", dict(slot_mask=np.ones(290, np.uint32)), "more than 289"),
    ("list-entry-outside", "symetrize_multi", dict(lst=np.array([3], np.uint32)), "outside the light field"),
    ("list-entry-outside-end", "window_end", dict(lst=np.array([0, 9, 1, 2, 3, 4, 5, 6, 7], np.uint32)), "outside the light field"),
    ("finalize-empty-slot", "finalize", dict(lst=np.array([1, K.EMPTY, 2], np.uint32)), "empty slot"),
    ("output-empty-slot", "output", dict(lst=np.array([K.EMPTY], np.uint32)), "empty slot"),
    ("lf-stride-small", "window_begin", dict(kw=dict(lf_stride=3 * 67 * 37 - 1)), "lf_stride smaller than one image"),
    ("w-stride-small", "window_begin", dict(kw=dict(w_stride=3 * 81 * 51 - 1)), "w_stride smaller than one padded image"),
    ("count_denoised-w-stride-small", "count_denoised", dict(kw=dict(w_stride=202 * 182 - 1)), "w_stride smaller than one padded image"),
    ("copy_rect-stride-small", "copy_rect", dict(kw=dict(w_stride=3 * 40 * 30 - 1)), "stride is smaller than one image"),
    ("symetrize-input-small", "symetrize", dict(bufs=_short("noisy")), "smaller than the geometry"),
    ("symetrize-output-small", "symetrize", dict(bufs=_short("w_noisy")), "smaller than the geometry"),
    ("crop-output-small", "crop", dict(bufs=_short("out")), "smaller than the geometry"),
    ("symetrize_multi-window-small", "symetrize_multi", dict(bufs=_short("w_noisy")), "smaller than the geometry"),
    ("unsymetrize_multi-lf-small", "unsymetrize_multi", dict(bufs=_short("out")), "outside the light field"),
    ("estimate-small", "estimate", dict(bufs=_short("den")), "smaller than the geometry"),
    ("estimate-est-small", "estimate", dict(bufs=_short("est")), "smaller than the geometry"),
    ("estimate_multi-small", "estimate_multi", dict(bufs=_short("w_den")), "smaller than the geometry"),
    ("estimate_lf-small", "estimate_lf", dict(bufs=_short("sub")), "smaller than the geometry"),
    ("window_begin-est-small", "window_begin", dict(bufs=_short("est")), "smaller than the geometry"),
    ("window_begin-window-small", "window_begin", dict(bufs=_short("w_basic")), "smaller than the geometry"),
    ("window_begin-counters-small", "window_begin", dict(bufs=_short("counters", 9)), "smaller than the geometry"),
    ("window_end-window-small", "window_end", dict(bufs=_short("w_den")), "smaller than the geometry"),
    ("window_end-lf-small", "window_end", dict(bufs=_short("den")), "outside the light field"),
    ("finalize-lf-small", "finalize", dict(bufs=_short("basic")), "outside the light field"),
    ("color-lf-small", "color", dict(bufs=_short("noisy")), "smaller than the geometry"),
    ("color-dmask-small", "color", dict(bufs=_short("dmask")), "dmask is smaller"),
    ("count_zeros-small", "count_zeros", dict(bufs=_short("den")), "smaller than the geometry"),
    ("count_zeros-counters-small", "count_zeros", dict(bufs=_short("counters")), "smaller than the geometry"),
    ("count_denoised-small", "count_denoised", dict(bufs=_short("w_den")), "smaller than the geometry"),
    ("copy_rect-dst-small", "copy_rect", dict(bufs=_short("out")), "smaller than the geometry"),
    ("copy_rows-src-small", "copy_rows", dict(bufs=_short("w_noisy")), "smaller than the geometry"),
    ("crop-off-beyond", "crop", dict(kw=dict(off=15)), "leaves the padded image"),
    ("copy_rect-right-of-dst", "copy_rect", dict(kw=dict(dx0=31)), "outside its image"),
    ("copy_rect-below-dst", "copy_rect", dict(kw=dict(dy0=29)), "outside its image"),
    ("copy_rect-right-of-src", "copy_rect", dict(kw=dict(sx0=21)), "outside its image"),
    ("copy_rect-below-src", "copy_rect", dict(kw=dict(sy0=14)), "outside its image"),
    ("copy_rect-wider-than-src", "copy_rect", dict(kw=dict(rw=41, sx0=0, dx0=0)), "outside its image"),
    ("copy_rows-below-src", "copy_rows", dict(kw=dict(sy0=11)), "outside their image"),
    ("copy_rows-below-dst", "copy_rows", dict(kw=dict(dy0=21)), "outside their image"),
]


@pytest.mark.parametrize("name,op,change,message", BAD, ids=[b[0] for b in BAD])
def test_seam_refuses_what_the_kernels_take_for_granted(ctx, name, op, change, message):
    import lfbm5d_amd as L
    c = _base(op)
    # the unchanged case runs: the refusal below is the change's
    check(c, launch(ctx, c.op, c.bufs, c.alias, c.lst, c.slot_mask, **c.kw), K.expected(c))
    bufs = dict(c.bufs)
    for n in change.get("null", ()):
        bufs[n] = None
    if "bufs" in change:
        bufs.update(change["bufs"](c))
    kw = {**c.kw, **change.get("kw", {})}
    dev = {n: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for n, v in bufs.items() if v is not None}
    args = dict(dev)
    for n, target in change.get("alias", c.alias).items():
        args[n] = args[target]
    with pytest.raises(L.LfBm5dError, match=message):
        ctx.debug_window(op, list=change.get("lst", c.lst), slot_mask=change.get("slot_mask", c.slot_mask), **args, **kw)
    for n, t in dev.items():   # nothing was launched
        assert np.array_equal(u32(t.cpu().numpy()), u32(bufs[n])), n


def test_the_refusals_start_from_the_cases_they_name():
    """the geometry the table above changes is the first case's of each op (a refusal must be the change's, not the base's)"""
    g = lambda op: _base(op).kw
    assert (g("symetrize")["W"], g("symetrize")["H"], g("symetrize")["N"]) == (64, 32, 16)
    assert (g("symetrize_multi")["N"], g("window_begin")["N"]) == (7, 7) and len(_base("symetrize_multi").lst) == 1
    assert (g("window_end")["W"], g("window_end")["H"]) == (64, 32) and K._n_sai_of(_base("window_end")) == 9
    assert (g("count_denoised")["W"], g("count_denoised")["H"], g("count_denoised")["N"]) == (200, 180, 1)
    assert (g("window_begin")["W"], g("window_begin")["H"], g("window_begin")["C"]) == (67, 37, 3) and _base("window_begin").bufs["w_basic"] is not None
    assert (g("crop")["N"], g("crop")["off"]) == (7, 7)
    r = g("copy_rect")
    assert (r["sW"], r["sH"], r["W"], r["H"], r["rw"], r["rh"], r["C"]) == (40, 30, 50, 45, 20, 17, 3)
    w = g("copy_rows")
    assert (w["sH"], w["H"], w["rh"]) == (50, 60, 40)
    assert K._n_sai_of(_base("symetrize_multi")) == 3 and _base("finalize").alias == {} and _base("output").alias != {}


# ---- images smaller than the search range are refused on every entry that pads ----
SMALL = [("narrow", 5, 24), ("low", 24, 7)]


@pytest.mark.parametrize("entry", ("step1", "step2", "denoise", "bm3d_lf"))
@pytest.mark.parametrize("name,W,H", SMALL, ids=[s[0] for s in SMALL])
def test_images_smaller_than_the_search_range_are_refused(ctx, entry, name, W, H):
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    A, Cc = 9, 3
    p1, p2 = (4, 6, 2, 4, 3, "id", "sadct", "haar"), (8, 6, 2, 4, 3, "dct", "sadct", "haar")   # nSim + nDisp = 8
    assert min(W, H) < p1[1] + p1[2]
    mask = np.ones(A, np.uint32)
    noisy = torch.from_numpy(np.random.default_rng(W).uniform(0, 255, (A, Cc * W * H)).astype(F)).cuda()
    before = noisy.clone()
    basic = torch.from_numpy(K.sent(A * Cc * W * H)).cuda()
    out = torch.from_numpy(K.sent(A * Cc * W * H)).cuda()
    P1, P2 = core.make_params(25.0, 2.7, *p1, color_space="opp"), core.make_params(25.0, 2.7, *p2, color_space="opp")
    ctx.reset_stats()
    with pytest.raises(L.LfBm5dError, match="smaller than the search range nSim \\+ nDisp"):
        if entry == "step1":
            ctx.step1(P1, noisy, mask, basic, L.ROWMAJOR, 3, 3, 1, W, H, Cc)
        elif entry == "step2":
            ctx.step2(P2, noisy, mask, basic, out, L.ROWMAJOR, 3, 3, 1, W, H, Cc)
        elif entry == "denoise":
            ctx.denoise(P1, P2, noisy, mask, basic, out, L.ROWMAJOR, 3, 3, 1, 1, W, H, Cc)
        else:
            ctx.bm3d_lf(core.make_bm3d_params(25.0, 2.7, 8, 8, 4, 3, "bior"), core.make_bm3d_params(25.0, 2.7, 8, 8, 4, 3, "dct"),
                        noisy, mask, basic, out, W, H, Cc)
    torch.cuda.synchronize()
    assert ctx.stats().passes == 0
    for t in (basic, out):
        assert (u32(t.cpu().numpy()) == SENT_BITS).all()
    assert torch.equal(noisy, before)


# ---- one real pass ties the model's ycbcr to the pipeline ----
def test_a_ycbcr_job_matches_the_oracle(ctx):
    """A 3x3 colour light field of 48 x 48 pixels in ycbcr, one hard-thresholding and one Wiener step, against the oracle at the bars of
    test_tile_mode_matches_the_oracles_tile_mode: equal window lists, equal window and pass counts, PSNR of both steps within 0.01 dB."""
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    aw = ah = 3
    Ws = Hs = 48
    clean, noisy = Hh.noisy_lf(Hh.source_lf(48), 25.0)
    Cc = 3
    mask = np.ones(ah * aw, np.uint32)
    p1, p2 = (4, 6, 2, 8, 4, "id", "sadct", "haar"), (8, 6, 2, 8, 4, "dct", "sadct", "haar")
    n1, b_o, st1 = O.run_step1(O.make_params(25.0, 2.7, *p1, cs="ycbcr"), noisy.copy(), mask, O.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
    w1 = O.last_windows()
    _, _, d_o, st2 = O.run_step2(O.make_params(25.0, 2.7, *p2, cs="ycbcr"), n1.copy(), b_o.copy(), mask, O.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
    w2 = O.last_windows()
    d_noisy = torch.from_numpy(noisy).cuda()
    d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
    ctx.reset_stats()
    ctx.step1(core.make_params(25.0, 2.7, *p1, color_space="ycbcr"), d_noisy, mask, d_basic, L.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
    s1, wins1 = ctx.stats(), ctx.last_windows()
    ctx.reset_stats()
    ctx.step2(core.make_params(25.0, 2.7, *p2, color_space="ycbcr"), d_noisy, mask, d_basic, d_den, L.ROWMAJOR, aw, ah, 1, Ws, Hs, Cc)
    s2, wins2 = ctx.stats(), ctx.last_windows()
    b_g, d_g = d_basic.cpu().numpy(), d_den.cpu().numpy()
    assert np.array_equal(wins1, w1) and np.array_equal(wins2, w2)
    assert (s1.windows, s1.passes) == (st1.windows, st1.passes) and (s2.windows, s2.passes) == (st2.windows, st2.passes)
    assert np.isfinite(b_g).all() and np.isfinite(d_g).all()
    pb_g, pb_o, pd_g, pd_o = O.psnr_lf(b_g, clean), O.psnr_lf(b_o, clean), O.psnr_lf(d_g, clean), O.psnr_lf(d_o, clean)
    print(f"ycbcr job: basic {pb_g:.4f} dB (oracle {pb_o:.4f}), denoised {pd_g:.4f} dB (oracle {pd_o:.4f})")
    assert abs(pb_g - pb_o) < 0.01
    assert abs(pd_g - pd_o) < 0.01
    # the light field the caller gets back went through the model's forward and inverse transforms
    back = M.color(M.color(noisy.reshape(9, 3, -1).transpose(1, 0, 2), M.YCBCR, 1), M.YCBCR, 0).transpose(1, 0, 2).reshape(9, -1)
    after1 = M.color(M.color(back.reshape(9, 3, -1).transpose(1, 0, 2), M.YCBCR, 1), M.YCBCR, 0).transpose(1, 0, 2).reshape(9, -1)
    assert M.same_bits(d_noisy.cpu().numpy(), after1).all()
