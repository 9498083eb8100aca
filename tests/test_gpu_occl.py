"""GPU tests of the occlusion-aware plane sweep (lfbm5d_view_*_occl_*, include/lfbm5d_occl.h): k_view_sweep_occl equals the numpy model
(tests/occl_model.py) bit for bit -- values, int8 j*, uint8 k*, the 65-bin histogram, the set histogram and the counts -- at steps 1, 2
and 4, (D, r) = (0, 0), (3, 7), (8, 0), (8, 7) and the ratios 1, the library's default and 8 on the shapes of tests/occl_cases.py (the
sub-pixel sweep's shapes and two occluder scenes whose edges cross the tile edges; both instantiations), with sentinels in what must not
be written and a second call returning the same bits; ratio 0 through the new entry points is the *_steps_* siblings' bits; the optional
outputs; both angular orders; the loop against the same calls made by hand; the host form and the C++ drop-in."""
import ctypes as C

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import occl_cases as K
import occl_model as O
import subpel_model as S
import view_model as V

HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ratios():
    return tuple(sorted({1.0, K.default_ratio(), 8.0}))


def _assert_equals_model(ctx, shape, kind, steps, D, r, ratio, d):
    """One synthesis against the model, with sentinels in what must not be written; and a second call returns the same bits."""
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES[shape]
    lf, mask, missing = K.case(shape, kind)
    want = K.model(shape, kind, steps, D, r, ratio)
    out = _dev(np.full(lf.shape, K.OUT_SENTINEL, np.float32))
    disp = _dev(np.full((ah * aw, H * W), K.DISP_SENTINEL, np.int8))
    sets = _dev(np.full((ah * aw, H * W), K.SET_SENTINEL, np.uint8))
    kw = dict(max_disparity=D, box_radius=r, ang_radius=R, disparity_steps=steps, occlusion=ratio)
    got = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, out=out, disparity_out=disp, sets_out=sets, **kw)
    tag = f"{shape} {kind} steps={steps} D={D} r={r} ratio={ratio}"
    assert np.array_equal(disp.cpu().numpy(), want["disp"]), tag                 # j*, and the sentinel elsewhere
    assert np.array_equal(sets.cpu().numpy(), want["sets"]), tag                 # k*, and the sentinel elsewhere
    assert np.array_equal(_bits(out), want["out"].view(np.uint32)), tag
    assert (got.missing, got.synthesised, got.left, got.pixels) == (want["missing"], want["synthesised"], want["left"], want["pixels"]), tag
    assert list(got.steps_hist) == list(want["hist"]) and len(got.steps_hist) == S.HIST, tag
    assert list(got.set_hist) == list(want["set_hist"]) and sum(got.set_hist) == got.pixels, tag
    if steps == 1:
        assert list(got.disparity_hist) == list(want["hist"][S.J_MAX - V.D_MAX:S.J_MAX + V.D_MAX + 1]), tag
    else:
        assert not any(got.disparity_hist), tag
    again = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, return_disparity=True, return_sets=True, **kw)
    s = want["sais"]
    assert np.array_equal(_bits(again.out)[s], _bits(out)[s]) and np.array_equal(again.disparity.cpu().numpy()[s], want["disp"][s]), tag
    assert np.array_equal(again.sets.cpu().numpy()[s], want["sets"][s]) and again[2:9] == got[2:9], tag
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_synthesis_equals_the_model(ctx, shape):
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES[shape]
    dev = {kind: _dev(K.case(shape, kind)[0]) for kind in K.kinds(shape)}
    half = 0
    for kind, steps, D, r, ratio in K.combos(shape, _ratios()):
        got, want = _assert_equals_model(ctx, shape, kind, steps, D, r, ratio, dev[kind])
        assert (got.synthesised, got.left) == (len(miss), 0)
        assert np.isfinite(got.out.cpu().numpy()[miss]).all()
        half += sum(got.set_hist[1:])
        if shape.startswith("single"):                                          # one source: E = 0 everywhere, j* = 0, k* = 0, a copy
            lf = K.case(shape, kind)[0]
            assert np.array_equal(_bits(got.out)[miss[0]], lf[1 - miss[0]].view(np.uint32))
            assert got.steps_hist[S.J_MAX] == H * W == got.set_hist[0]
    for kind, d in dev.items():                                                 # the input is only read
        assert np.array_equal(_bits(d), K.case(shape, kind)[0].view(np.uint32))
    lf, mask, missing = K.case(shape, K.kinds(shape)[0])
    n = [len(V.sources(m, mask, missing, K.ROWMAJOR, aw, ah, R)) for m in miss]
    if shape in ("centre-R2", "rect-5x5", "stripes-5x5"):
        assert n == [24]                                                        # more than 8 sources: the instantiation that recomputes ran
    if shape in K.SCENES:
        assert half > 0                                                         # half-planes were chosen
        m = miss[-1]                                                            # (SAI 0 of the pair is a corner: no candidate)
        k = K.model(shape, "scene", 1, 3, 7, K.default_ratio())["sets"][m].reshape(H, W)
        if shape.startswith("stripes") and H > K.K.TILE_H and W > K.K.TILE_W:                    # both kinds of choice on both sides of the tile edges
            assert len(np.unique(k[K.K.TILE_H - 1])) > 1 and len(np.unique(k[K.K.TILE_H])) > 1
            assert len(np.unique(k[:, K.K.TILE_W - 1])) > 1 and len(np.unique(k[:, K.K.TILE_W])) > 1
    if max(n) <= 2 or shape == "corners":                                       # no admissible candidate
        assert half == 0


@pytest.mark.gpu
def test_ratio_zero_is_the_steps_sibling_in_bits(ctx):
    import torch
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES["centre"]
    lf, mask, missing = K.case("centre", "textured")
    d = _dev(lf)
    lib, up, ullp = core.lib(), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)
    mp, sp = mask.ctypes.data_as(up), missing.ctypes.data_as(up)
    P = core.make_params(0.0, 2.7, *HT)
    for steps in K.STEPS:
        for D, r, iters in ((3, 3, 0), (8, 7, 0), (2, 1, 1)):
            vp = L.view_params(D, r, R, iters, 20.0, 10.0)
            o = [torch.full_like(d, K.OUT_SENTINEL) for _ in range(2)]
            dp = [torch.full((ah * aw, H * W), K.DISP_SENTINEL, dtype=torch.int8, device="cuda") for _ in range(2)]
            st = torch.full((ah * aw, H * W), K.SET_SENTINEL, dtype=torch.uint8, device="cuda")
            res, hist = [core.ViewResultStruct() for _ in range(2)], [np.zeros(S.HIST, np.uint64) for _ in range(2)]
            occl = core.ViewOcclResultStruct()
            occl.set_hist[0] = 5
            if iters == 0:
                tail = (K.ROWMAJOR, aw, ah, W, H, C_)
                rc0 = lib.lfbm5d_view_fill_steps_device(ctx._h, C.byref(vp), steps, C.c_void_p(d.data_ptr()), mp, sp, C.c_void_p(o[0].data_ptr()),
                                                        C.c_void_p(dp[0].data_ptr()), *tail, C.byref(res[0]), hist[0].ctypes.data_as(ullp))
                rc1 = lib.lfbm5d_view_fill_occl_device(ctx._h, C.byref(vp), steps, 0.0, C.c_void_p(d.data_ptr()), mp, sp,
                                                       C.c_void_p(o[1].data_ptr()), C.c_void_p(dp[1].data_ptr()), C.c_void_p(st.data_ptr()), *tail,
                                                       C.byref(res[1]), hist[1].ctypes.data_as(ullp), C.byref(occl))
            else:
                tail = (K.ROWMAJOR, aw, ah, 1, W, H, C_)
                rc0 = lib.lfbm5d_view_steps_device(ctx._h, C.byref(vp), steps, C.byref(P), C.c_void_p(d.data_ptr()), mp, sp,
                                                   C.c_void_p(o[0].data_ptr()), C.c_void_p(dp[0].data_ptr()), *tail, C.byref(res[0]),
                                                   hist[0].ctypes.data_as(ullp))
                rc1 = lib.lfbm5d_view_occl_device(ctx._h, C.byref(vp), steps, 0.0, C.byref(P), C.c_void_p(d.data_ptr()), mp, sp,
                                                  C.c_void_p(o[1].data_ptr()), C.c_void_p(dp[1].data_ptr()), C.c_void_p(st.data_ptr()), *tail,
                                                  C.byref(res[1]), hist[1].ctypes.data_as(ullp), C.byref(occl))
            assert rc0 == 0 and rc1 == 0
            assert np.array_equal(_bits(o[0]), _bits(o[1])) and np.array_equal(dp[0].cpu().numpy(), dp[1].cpu().numpy())
            assert bytes(res[0]) == bytes(res[1]) and np.array_equal(hist[0], hist[1])
            assert (st == K.SET_SENTINEL).all().item() and not any(occl.set_hist)   # off: no set is written, the result is zero
    a = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, disparity_steps=2, occlusion=None)
    assert a.set_hist is None and a.sets is None


@pytest.mark.gpu
def test_optional_outputs_and_angular_orders(ctx):
    shape = "rect-31x65-two"
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES[shape]
    lf, mask, missing = K.case(shape, "scene")
    rho = K.default_ratio()
    want = K.model(shape, "scene", 2, 3, 7, rho)
    d = _dev(lf)
    kw = dict(max_disparity=3, box_radius=7, disparity_steps=2, occlusion=rho)
    for rd, rs in ((False, False), (True, False), (False, True)):               # d_disp = NULL, d_set = NULL, both
        got = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, return_disparity=rd, return_sets=rs, **kw)
        assert (got.disparity is None, got.sets is None) == (not rd, not rs)
        assert np.array_equal(_bits(got.out)[miss], want["out"].view(np.uint32)[miss])
        assert list(got.set_hist) == list(want["set_hist"]) and list(got.steps_hist) == list(want["hist"])
    # column-major: the same light field with its SAIs in the other order
    perm = [(st % ah) * aw + st // ah for st in range(ah * aw)]                 # column-major index st holds row-major SAI perm[st]
    got = ctx.view_fill(_dev(lf[perm]), mask[perm], missing[perm], L.COLMAJOR, aw, ah, W, H, C_, return_disparity=True, return_sets=True, **kw)
    w2 = O.fill(lf[perm], mask[perm], missing[perm], V.COLMAJOR, aw, ah, W, H, C_, 3, 7, R, steps=2, ratio=rho)
    ms = [i for i in range(ah * aw) if missing[perm][i]]
    assert np.array_equal(_bits(got.out)[ms], w2["out"].view(np.uint32)[ms]) and np.array_equal(got.sets.cpu().numpy()[ms], w2["sets"][ms])
    assert np.array_equal(got.disparity.cpu().numpy()[ms], w2["disp"][ms]) and list(got.set_hist) == list(w2["set_hist"])
    back = [perm.index(i) for i in miss]
    assert np.array_equal(_bits(got.out)[back], want["out"].view(np.uint32)[miss])   # and the same values as row-major


@pytest.mark.gpu
def test_loop_host_form_and_drop_in(ctx):
    """lfbm5d_view_occl_device with K = 2 equals the same public calls made by hand (the fill with occlusion, step 1, projections) in
    bits; the host form equals the device form; the C++ drop-in's view_synth_LF with occl_ratio equals both."""
    import torch
    Kn, tail = 2, (L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    clean = K.occluder_lf("rect", 3, 3, 64, 64, 3)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[[1, 4]] = 1
    y = clean.copy()
    y[[1, 4]] = np.nan                                                          # never read
    d_y = _dev(y)
    P = core.make_params(0.0, 2.7, *HT)
    rho = K.default_ratio()
    kw = dict(max_disparity=4, box_radius=3, iterations=Kn, sigma_start=30.0, sigma_end=5.0, disparity_steps=2, occlusion=True)
    a = ctx.view_synth(d_y, mask, missing, P, *tail, return_disparity=True, return_sets=True, **kw)
    assert np.array_equal(_bits(d_y), y.view(np.uint32))
    x0 = ctx.view_fill(d_y, mask, missing, L.ROWMAJOR, 3, 3, 64, 64, 3, max_disparity=4, box_radius=3, return_disparity=True, return_sets=True,
                       disparity_steps=2, occlusion=rho)
    want = O.fill(y, mask, missing, V.ROWMAJOR, 3, 3, 64, 64, 3, 4, 3, steps=2, ratio=rho)
    assert np.array_equal(_bits(x0.out)[[1, 4]], want["out"].view(np.uint32)[[1, 4]]) and list(x0.set_hist) == list(want["set_hist"])
    assert sum(want["set_hist"][1:]) > 0
    assert np.array_equal(x0.sets.cpu().numpy()[[1, 4]], a.sets.cpu().numpy()[[1, 4]]) and a.set_hist == x0.set_hist
    assert np.array_equal(x0.disparity.cpu().numpy()[[1, 4]], a.disparity.cpu().numpy()[[1, 4]]) and a.steps_hist == x0.steps_hist
    flags = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
    flags[[1, 4]] = 1
    x = x0.out
    for sig in V.sigma_schedule(Kn, 30.0, 5.0):
        z = x.clone()
        basic = torch.zeros_like(z)
        ctx.step1(core.make_params(sig, 2.7, *HT), z, mask, basic, *tail)
        x = torch.zeros_like(z)
        ctx.inpaint_project(flags, basic, d_y, mask, x, 64, 64, 3)
    assert np.array_equal(_bits(a.out), _bits(x))
    plain = ctx.view_synth(d_y, mask, missing, P, *tail, **dict(kw, occlusion=None))
    assert not np.array_equal(_bits(plain.out), _bits(a.out)) and plain.set_hist is None
    # the host form
    h = ctx.view_synth(y.copy(), mask, missing, P, *tail, return_disparity=True, return_sets=True, **kw)
    assert isinstance(h.out, np.ndarray) and np.array_equal(h.out.view(np.uint32), _bits(a.out))
    assert np.array_equal(h.disparity[[1, 4]], a.disparity.cpu().numpy()[[1, 4]]) and np.array_equal(h.sets[[1, 4]], a.sets.cpu().numpy()[[1, 4]])
    assert h[2:9] == a[2:9]
    # the C++ drop-in's view_synth_LF
    probe = {k: v for k, v in kw.items() if k not in ("disparity_steps", "occlusion")}
    cpp, done, left, jmin, jmax, sets = core.view_synth_probe(y, mask, missing, 3, 3, 64, 64, 3, 2.7, HT, disparity_steps=2, occl_ratio=rho, **probe)
    assert np.array_equal(cpp.view(np.uint32), _bits(a.out)) and sets == a.set_hist
    hist = np.array(a.steps_hist)
    assert (done, left, jmin, jmax) == (2, 0, int(np.nonzero(hist)[0][0]) - S.J_MAX, int(np.nonzero(hist)[0][-1]) - S.J_MAX)
