"""GPU tests of the Poisson-Gaussian noise routines (lfbm5d_pg_*, lfbm5d_denoise_pg_*, include/lfbm5d.h) against the numpy model
(tests/pg_model.py): integer equality of the block statistics, the estimate's forms, the transforms within one float32 ulp of the
float64 model, the job against its three calls made by hand, the benefit over one global sigma, and the CLIs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import pg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _noisy_lf(ang, C_, H, W, a=2.0, b=25.0, masked=1):
    if ang == 3:
        u8 = np.load(GOLDEN)[:, :C_, 40:40 + H, 30:30 + W]
    else:
        u8 = synth.make_lf(ang, ang, H, W)[:, :C_]
    A = ang * ang
    lf = synth.add_poisson_gaussian(np.ascontiguousarray(u8, np.float32).reshape(A, -1), a, b, 3)
    mask = np.ones(A, np.uint32)
    if masked is not None:
        mask[masked] = 0
        lf[masked] = 0.0
    return lf, mask


def _assert_stats(ctx, lf, mask, W, H, C_, d=None):
    hist, sm, blocks, skipped = ctx.pg_histogram(_dev(lf) if d is None else d, mask, W, H, C_)
    rh, rs, rb, rk = M.histogram(lf, mask, W, H, C_)
    assert (blocks, skipped) == (rb, rk)
    assert np.array_equal(hist, rh) and np.array_equal(sm, rs)
    assert int(hist.sum()) == blocks - skipped
    return hist, sm


# one chunk of the statistics kernel is 4 x 1024 blocks, its loads come in four sub-chunks of 1024; a workgroup takes every n-th chunk
@pytest.mark.gpu
@pytest.mark.parametrize("ang,C_,H,W", [(3, 1, 53, 67), (3, 3, 53, 67), (3, 3, 53, 66), (5, 3, 61, 77), (5, 1, 60, 78)])
def test_statistics_equal_the_model(ctx, ang, C_, H, W):
    lf, mask = _noisy_lf(ang, C_, H, W)
    _assert_stats(ctx, lf, mask, W, H, C_)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(2, 2), (2, 3), (3, 2), (3, 3),                      # one block
                                 (62, 66), (64, 64), (82, 50),                        # 1023, 1024, 1025 blocks: a sub-chunk's edge
                                 (130, 126), (130, 127), (128, 128), (482, 34),       # 4095, 4095, 4096, 4097 blocks: a chunk's edge
                                 (128, 130)])                                         # 4160 blocks: the second chunk nearly empty
def test_statistics_at_the_kernel_s_edges(ctx, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    for C_ in (1, 3):
        lf = (rng.uniform(0.0, 255.0, (1, C_ * H * W)) + rng.normal(0.0, 6.0, (1, C_ * H * W))).astype(np.float32)
        _assert_stats(ctx, lf, np.ones(1, np.uint32), W, H, C_)


@pytest.mark.gpu
def test_statistics_on_a_buffer_that_is_not_8_byte_aligned(ctx):
    lf, mask = _noisy_lf(3, 3, 53, 66)
    import torch
    buf = torch.zeros(lf.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(lf.reshape(-1)).cuda()
    d = buf[1:].view(9, -1)
    assert d.data_ptr() % 8 == 4 and d.is_contiguous()
    _assert_stats(ctx, lf, mask, 66, 53, 3, d=d)


@pytest.mark.gpu
def test_statistics_skip_non_finite_blocks_and_clamp_the_range(ctx):
    H, W = 40, 52
    lf, mask = _noisy_lf(3, 3, H, W, masked=None)
    x = lf.reshape(9, 3, H, W)
    x[2, 1, 7, 9] = np.nan
    x[2, 1, 20, 30] = np.inf
    x[4, 0, 11, 3] = -np.inf
    x[5, 2, 39, 51] = np.nan                    # H and W even: the last block
    x[0, 0, :6] = -40.0 + x[0, 0, :6] / 16      # below 0: level 0
    x[0, 0, 6:12] = 300.0 + x[0, 0, 6:12] / 16  # above 255: level 63
    x[8, 2, :, :8] *= 1e-7                      # differences below 2^-12: key 0
    x[7, 1, 0:2, 0:2] = [[1000.0, -1000.0], [-1000.0, 1000.0]]   # |d| = 2000 >= 2^8: key 321
    hist, sm = _assert_stats(ctx, lf, mask, W, H, 3)
    _, _, _, skipped = ctx.pg_histogram(_dev(lf), mask, W, H, 3)
    assert skipped == 4
    assert hist[0, 0].sum() >= 3 * 26 and hist[0, 63].sum() >= 3 * 26
    assert sm[0, 0] == 0 or hist[0, 0].sum() > 3 * 26            # the clamped blocks add mc = 0 to the sum
    assert hist[2, :, 0].sum() >= 20 * 4 and hist[1, :, M.Q - 1].sum() >= 1


def _same_estimate(a, b):
    f = lambda e: np.array([e.a, e.b, *e.a_channel, *e.b_channel], np.float64).view(np.uint64)
    assert np.array_equal(f(a), f(b))
    assert (a.blocks, a.skipped) == (b.blocks, b.skipped)
    assert np.array_equal(a.hist, b.hist) and np.array_equal(a.sum_m, b.sum_m)


@pytest.mark.gpu
def test_estimate_forms_determinism_and_read_only_input(ctx):
    H, W = 61, 77
    lf, mask = _noisy_lf(5, 3, H, W)
    d = _dev(lf)
    before = _bits(d).copy()
    e1 = ctx.pg_estimate(d, mask, W, H, 3)
    e2 = ctx.pg_estimate(d, mask, W, H, 3)
    _same_estimate(e1, e2)
    assert np.array_equal(_bits(d), before)
    _same_estimate(e1, ctx.pg_estimate(lf, mask, W, H, 3))                                                    # host form, flat array
    _same_estimate(e1, ctx.pg_estimate([lf[i].copy() if mask[i] else None for i in range(25)], mask, W, H, 3))  # one array per SAI
    _same_estimate(e1, L.pg_estimate(d, mask, W, H, 3))                                                       # module level
    assert np.array_equal(lf.view(np.uint32), before)
    # the estimate is lfbm5d_pg_fit of the histograms it returns, and the model's
    assert (e1.a, e1.b) == L.pg_fit(e1.hist.sum(axis=0), e1.sum_m.sum(axis=0))
    for c in range(3):
        assert (e1.a_channel[c], e1.b_channel[c]) == L.pg_fit(e1.hist[c], e1.sum_m[c])
    r = M.estimate(lf, mask, W, H, 3)
    assert abs(e1.a - r["a"]) <= 1e-10 * abs(r["a"]) + 1e-12 and abs(e1.b - r["b"]) <= 1e-10 * abs(r["b"]) + 1e-12
    assert e1.blocks == r["blocks"] == 24 * 3 * 30 * 38


@pytest.mark.gpu
def test_rejected_inputs(ctx):
    lf, mask = _noisy_lf(3, 3, 53, 67)
    d = _dev(lf)
    for kw in (dict(chnls=2), dict(width=1), dict(height=1), dict(mask=np.zeros(9, np.uint32))):
        args = dict(mask=mask, width=67, height=53, chnls=3)
        args.update(kw)
        for fn in (ctx.pg_estimate, ctx.pg_histogram):
            with pytest.raises(L.LfBm5dError) as e:
                fn(d, args["mask"], args["width"], args["height"], args["chnls"])
            assert str(e.value), kw
    with pytest.raises(L.LfBm5dError, match="256 blocks"):           # too small for any level to be valid
        ctx.pg_estimate(_dev(lf[:, :3 * 4 * 4]), mask, 4, 4, 3)
    out = _dev(np.zeros_like(lf))
    for model in ((-1.0, 5.0), (1.0, -1.0), (float("nan"), 1.0), ([1.0, 1.0, 0.0], [1.0, 1.0, 0.0])):
        for fn in (ctx.pg_forward, ctx.pg_inverse):
            with pytest.raises(L.LfBm5dError, match="model"):
                fn(model, d, mask, out, 67, 53, 3)
    with pytest.raises(L.LfBm5dError, match="non-empty"):
        ctx.pg_forward((1.0, 1.0), d, np.zeros(9, np.uint32), out, 67, 53, 3)
    lib, h = core.lib(), ctx._h
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint))
    res, mdl = core.PgEstimateStruct(), core.pg_model(1.0, 1.0)
    p = C.c_void_p(d.data_ptr())
    assert lib.lfbm5d_pg_estimate_device(h, None, mp, 9, 67, 53, 3, C.byref(res), None, None) == 1
    assert lib.lfbm5d_pg_estimate_device(h, p, None, 9, 67, 53, 3, C.byref(res), None, None) == 1
    assert lib.lfbm5d_pg_estimate_device(h, p, mp, 9, 67, 53, 3, None, None, None) == 1
    assert lib.lfbm5d_pg_estimate_host_sai(h, None, mp, 9, 67, 53, 3, C.byref(res), None, None) == 1
    assert lib.lfbm5d_pg_estimate_host_sai(h, (C.c_void_p * 9)(), mp, 9, 67, 53, 3, C.byref(res), None, None) == 1
    assert "NULL" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_pg_histogram_device(h, p, mp, 9, 67, 53, 3, None, None, None, None) == 1
    assert lib.lfbm5d_pg_forward_device(h, None, p, mp, p, 9, 67, 53, 3) == 1
    assert lib.lfbm5d_pg_forward_device(h, C.byref(mdl), None, mp, p, 9, 67, 53, 3) == 1
    assert lib.lfbm5d_pg_inverse_device(h, C.byref(mdl), p, mp, None, 9, 67, 53, 3) == 1
    assert lib.lfbm5d_last_error(h).decode()


def _ulps(x, ref64):
    """Distance in float32 ulps between x (float32) and the float64 reference rounded to float32."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(x) - key(ref64.astype(np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize("C_,a,b", [(3, [2.0, 0.5, 8.0], [25.0, 4.0, 0.0]), (1, [1.0], [0.0]), (3, [0.0, 1.0, 0.25], [400.0, 9.0, 1.0])])
def test_transforms_within_one_ulp_of_the_model(ctx, C_, a, b):
    import torch
    H, W = 53, 67
    lf, mask = _noisy_lf(3, C_, H, W, a=2.0, b=25.0, masked=4)
    x = lf.reshape(9, C_, H, W)
    x[0, 0, 0, :8] = [-500.0, -60.0, -14.0, -13.0, -1.0, 0.0, 1e-3, 700.0]    # a z + c < 0 at the left, beyond the range at the right
    mask_on = mask != 0
    d = _dev(lf)
    fwd = torch.full_like(d, -7.0)
    s = ctx.pg_forward((a, b), d, mask, fwd, W, H, C_)
    ref, rs = M.forward_lf(lf, a, b, C_)
    assert s == rs == L.pg_scale((a, b), C_)
    g = fwd.cpu().numpy()
    assert np.isfinite(g[mask_on]).all()
    assert _ulps(g[mask_on], ref[mask_on]).max() <= 1
    assert (g[~mask_on] == -7.0).all()                                        # a masked SAI's plane is untouched
    inv = torch.full_like(d, -7.0)
    ctx.pg_inverse((a, b), fwd, mask, inv, W, H, C_)
    gi = inv.cpu().numpy()
    assert _ulps(gi[mask_on], M.inverse_lf(g, a, b, C_)[mask_on]).max() <= 1
    assert (gi[~mask_on] == -7.0).all() and (gi[mask_on] >= 0.0).all()
    if a[0] > 0.0:                                                            # values with a z + c < 0 are finite and map back to 0
        c0 = 0.375 * a[0] * a[0] + b[0]
        low = x[0, 0, 0, :8] * a[0] + c0 < 0.0
        assert low.any() and (gi.reshape(9, C_, H, W)[0, 0, 0, :8][low] == 0.0).all()
    # in place gives the same bits as out of place
    d2 = d.clone()
    ctx.pg_forward((a, b), d2, mask, d2, W, H, C_)
    assert np.array_equal(_bits(d2)[mask_on], _bits(fwd)[mask_on]) and np.array_equal(_bits(d2)[~mask_on], _bits(d)[~mask_on])
    ctx.pg_inverse((a, b), d2, mask, d2, W, H, C_)
    assert np.array_equal(_bits(d2)[mask_on], _bits(inv)[mask_on])
    # the round trip returns the input up to the inverse's bias correction (small against the noise at these levels)
    ok = mask_on[:, None] & (lf > 20.0) & (lf < 255.0)
    assert np.abs(gi[ok] - lf[ok]).max() < 1.0 + 0.3 * max(a)


@pytest.mark.gpu
def test_forward_is_the_identity_for_pure_gaussian_noise(ctx):
    import torch
    lf, mask = _noisy_lf(3, 3, 53, 67, a=0.0, b=400.0, masked=None)
    lf[0, :4] = [-30.0, 0.0, 300.0, 1e-20]
    d = _dev(lf)
    out = torch.zeros_like(d)
    assert ctx.pg_forward((0.0, 400.0), d, mask, out, 67, 53, 3) == 20.0
    assert np.array_equal(_bits(out), _bits(d))


P1 = lambda sigma: core.make_params(sigma, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")     # the README parameters
P2 = lambda sigma: core.make_params(sigma, 2.7, 16, 18, 6, 8, 4, "dct", "sadct", "haar")
TAIL = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)


def _clean_crop():
    return np.ascontiguousarray(np.load(GOLDEN)[:, :, :64, :64], np.float32).reshape(9, -1)


def _psnr(x, clean):
    return float(10.0 * np.log10(255.0 ** 2 / ((x.astype(np.float64) - clean) ** 2).mean()))


def _denoise(ctx, noisy, sigma):
    import torch
    d = _dev(noisy)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    ctx.denoise(P1(sigma), P2(sigma), d, np.ones(9, np.uint32), basic, den, *TAIL)
    return basic, den


def _denoise_pg(ctx, noisy, model):
    import torch
    d = _dev(noisy)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    used = ctx.denoise_pg(model, P1(1.0), P2(99.0), d, np.ones(9, np.uint32), basic, den, *TAIL)   # the sigmas passed are ignored
    return basic, den, used, d


@pytest.mark.gpu
def test_job_is_the_three_calls_made_by_hand(ctx):
    import torch
    clean, mask = _clean_crop(), np.ones(9, np.uint32)
    noisy = synth.add_poisson_gaussian(clean, 2.0, 25.0, 5)
    model = ([2.0, 1.5, 2.5], [25.0, 30.0, 20.0])
    basic, den, used, d = _denoise_pg(ctx, noisy, model)
    assert np.array_equal(_bits(d), noisy.view(np.uint32))                    # d_noisy is only read
    assert list(used.a) == model[0] and list(used.b) == model[1]
    t = torch.zeros_like(d)
    s = ctx.pg_forward(model, d, mask, t, 64, 64, 3)
    b2, d2 = torch.zeros_like(d), torch.zeros_like(d)
    ctx.denoise(P1(s), P2(s), t, mask, b2, d2, *TAIL)
    ctx.pg_inverse(model, b2, mask, b2, 64, 64, 3)
    ctx.pg_inverse(model, d2, mask, d2, 64, 64, 3)
    assert np.array_equal(_bits(basic), _bits(b2)) and np.array_equal(_bits(den), _bits(d2))
    # host forms: flat array and one array per SAI
    hb, hd = np.zeros_like(noisy), np.zeros_like(noisy)
    ctx.denoise_pg(model, P1(1.0), P2(1.0), noisy.copy(), mask, hb, hd, *TAIL)
    assert np.array_equal(hb.view(np.uint32), _bits(basic)) and np.array_equal(hd.view(np.uint32), _bits(den))
    lb, ld = [np.zeros(noisy.shape[1], np.float32) for _ in range(9)], [np.zeros(noisy.shape[1], np.float32) for _ in range(9)]
    L.denoise_pg(model, P1(1.0), P2(1.0), [noisy[i].copy() for i in range(9)], mask, lb, ld, *TAIL, ctx=ctx)
    assert np.array_equal(np.stack(ld).view(np.uint32), _bits(den))


@pytest.mark.gpu
@pytest.mark.parametrize("C_", [1, 3])
def test_job_host_forms_with_empty_sais(ctx, C_):
    """3 x 3 SAIs, column-major, SAI 0 and the centre empty, 67 x 35 pixels (one 64 x 32 tile plus a remainder, width no multiple of 4):
    the host forms (flat array, one array per SAI with None for the empty ones) return the device form's bits and leave the planes of
    empty SAIs alone.  The model is given: the light field is too small for the estimate, whose host forms
    test_estimate_forms_determinism_and_read_only_input compares under a holed mask."""
    import torch
    H, W = 35, 67
    noisy, mask = _noisy_lf(3, C_, H, W, masked=[0, 4])
    tail = (L.COLMAJOR, 3, 3, 1, 1, W, H, C_)
    live = mask != 0
    d = _dev(noisy)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    model = (2.0, 25.0)
    used = ctx.denoise_pg(model, P1(1.0), P2(1.0), d, mask, basic, den, *tail)
    assert np.array_equal(_bits(d), noisy.view(np.uint32))
    hb, hd = np.full_like(noisy, -7.0), np.full_like(noisy, -7.0)
    hused = ctx.denoise_pg(model, P1(1.0), P2(1.0), noisy.copy(), mask, hb, hd, *tail)
    assert list(hused.a) == list(used.a) and list(hused.b) == list(used.b)
    assert np.array_equal(hb.view(np.uint32)[live], _bits(basic)[live]) and np.array_equal(hd.view(np.uint32)[live], _bits(den)[live])
    assert (hb[~live] == -7.0).all() and (hd[~live] == -7.0).all()
    lb, ld = ([np.zeros(noisy.shape[1], np.float32) if mask[i] else None for i in range(9)] for _ in range(2))
    ctx.denoise_pg(model, P1(1.0), P2(1.0), [noisy[i].copy() if mask[i] else None for i in range(9)], mask, lb, ld, *tail)
    for i in np.nonzero(live)[0]:
        assert np.array_equal(lb[i].view(np.uint32), _bits(basic)[i]) and np.array_equal(ld[i].view(np.uint32), _bits(den)[i])


@pytest.mark.gpu
def test_job_on_pure_gaussian_noise_is_the_plain_job(ctx):
    clean = _clean_crop()
    noisy = synth.add_noise_mt19937(clean, 20.0, seed=1)
    pb, pd = _denoise(ctx, noisy, 20.0)
    gb, gd, used, _ = _denoise_pg(ctx, noisy, (0.0, 400.0))
    for g, p in ((gb, pb), (gd, pd)):
        g, p = g.cpu().numpy(), np.maximum(p.cpu().numpy(), 0.0)
        assert _ulps(g, p.astype(np.float64)).max() <= 1


@pytest.mark.gpu
def test_job_refuses_a_sharded_context():
    import torch
    c = L.Context(0)
    try:
        c.set_shard(0, 2)
        d = _dev(_clean_crop())
        out = torch.zeros_like(d)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            c.denoise_pg((1.0, 1.0), P1(1.0), P2(1.0), d, np.ones(9, np.uint32), out, torch.zeros_like(d), *TAIL)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            c.pg_estimate(d, np.ones(9, np.uint32), 64, 64, 3)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            c.pg_forward((1.0, 1.0), d, np.ones(9, np.uint32), out, 64, 64, 3)
    finally:
        c.close()


@pytest.mark.gpu
def test_benefit_over_one_global_sigma(ctx):
    """a = 8, b = 0 on the 3x3x64x64 golden crop, numpy seed 1.  Measured on an MI355X (profiles/pg_noise.txt): plain 34.857 dB,
    denoise_pg with the true model 35.526 dB (+0.67), with the estimated model (a = 7.862, b = 0) 35.595 dB."""
    clean = _clean_crop()
    noisy = synth.add_poisson_gaussian(clean, 8.0, 0.0, 1)
    _, plain = _denoise(ctx, noisy, float(np.sqrt((8.0 * clean).mean())))
    _, true_, _, _ = _denoise_pg(ctx, noisy, (8.0, 0.0))
    _, est, used, _ = _denoise_pg(ctx, noisy, None)
    p = [_psnr(x.cpu().numpy(), clean) for x in (plain, true_, est)]
    print(f"benefit: plain {p[0]:.3f} dB, VST true model {p[1]:.3f} dB, VST estimated model {p[2]:.3f} dB "
          f"(a = {used.a[0]:.4f}, b = {used.b[0]:.4f})")
    e = ctx.pg_estimate(_dev(noisy), np.ones(9, np.uint32), 64, 64, 3)
    assert (used.a[0], used.b[0]) == (e.a, e.b) and used.a[2] == e.a         # NULL model: the pooled estimate for every channel
    assert p[1] >= p[0] + 0.35
    assert p[2] >= p[1] - 0.15


def _write_source_lf(tmp):
    from PIL import Image
    lf = np.load(GOLDEN)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src


def _readme_args(cli, tmp, src):
    if cli == CLI3:
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


def _model_line(stdout):
    m = re.search(r"(Estimated|Given) noise model: a = ([0-9.eE+-]+), b = ([0-9.eE+-]+) \(sigma after stabilisation = ([0-9.eE+-]+)\)", stdout)
    assert m, stdout[-2000:]
    return m.group(1), float(m.group(2)), float(m.group(3)), float(m.group(4))


def _psnrs(tmp):
    txt = open(f"{tmp}/measures.txt").read()
    return {k: float(txt.split(f"-> Average PSNR {k} = ")[1].split()[0]) for k in ("noisy", "basic", "denoised")}


DENOISED_PSNR_PG = 34.6408   # the README command with LFBM5D_SEED=1 LFBM5D_SIGMA=poisson:8,0, measured on an MI355X


@pytest.mark.gpu
def test_cli_poisson_with_a_given_model(tmp_path):
    tmp = str(tmp_path)
    src = _write_source_lf(tmp)
    env = dict(os.environ, LFBM5D_SEED="1", LFBM5D_SIGMA="poisson:8,0")
    out = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:]
    kind, a, b, s = _model_line(out.stdout)
    assert (kind, a, b) == ("Given", 8.0, 0.0) and abs(s - L.pg_scale((8.0, 0.0))) < 1e-4
    vals = _psnrs(tmp)
    print("LFBM5D_SIGMA=poisson:8,0: PSNR", vals)
    assert vals["denoised"] > vals["basic"] > vals["noisy"]
    assert abs(vals["denoised"] - DENOISED_PSNR_PG) < 0.05
    assert os.path.exists(f"{tmp}/denoised/SAI_02_02.png")
    # LFBM3Ddenoising: forward, run_bm3d_LF, inverse
    tmp3 = os.path.join(tmp, "bm3d")
    os.makedirs(tmp3)
    src3 = _write_source_lf(tmp3)
    out = subprocess.run(_readme_args(CLI3, tmp3, src3), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:]
    assert _model_line(out.stdout)[:3] == ("Given", 8.0, 0.0)
    v3 = _psnrs(tmp3)
    print("LFBM3Ddenoising, LFBM5D_SIGMA=poisson:8,0: PSNR", v3)
    assert v3["denoised"] > v3["noisy"] + 5.0


@pytest.mark.gpu
def test_cli_poisson_estimates_the_model_of_gaussian_noise(tmp_path):
    tmp = str(tmp_path)
    src = _write_source_lf(tmp)
    env = dict(os.environ, LFBM5D_SEED="1", LFBM5D_SIGMA="poisson")
    out = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:]
    kind, a, b, s = _model_line(out.stdout)
    vals = _psnrs(tmp)
    print(f"LFBM5D_SIGMA=poisson on Gaussian sigma = 25: a = {a}, b = {b}, s = {s}, PSNR {vals}")
    assert kind == "Estimated" and a < 0.3
    assert abs(np.sqrt(a * 121.0 + b) - 25.0) <= 2.5
    assert vals["denoised"] > vals["basic"] > vals["noisy"]
