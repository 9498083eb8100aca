"""GPU tests of the quality metrics (lfbm5d_quality_*, include/lfbm5d.h) against the float64 numpy model (tests/quality_model.py) on
the same float32 inputs: parity at the kernel's tile edges, closed forms, determinism, rejected inputs, Python and the CLI.

The kernel (lfbm5d_amd/csrc/lfbm5d_quality.hip) gives a wave 64 window columns, a workgroup 256 window columns x 56 window rows, and
stages input rows 11 at a time; the parity sizes sit on and next to each of these edges.

Bounds.  mse: every term is non-negative, so a double sum of N terms in any order is within (N - 1) 2^-53 relative of the exact sum;
forming d^2 and dividing add two roundings; model plus kernel: 2 (N + 2) 2^-53 relative, N = C H W.  ssim: |delta sigma^2| <= 2 * 123 *
2^-53 * peak^2 ~ 1.8e-9 against C2 = 58.5 is ~3e-11 per factor: 1e-9 absolute (1000 x what the separable double form differs from the
2-D one, 100 x below a float32 implementation).  rmse = sqrt(mse) halves the relative error; psnr = 10 log10(peak^2 / mse) turns a
relative error e of mse into 10 / ln 10 * e dB (plus the roundings of log10 itself, a few 2^-52 of the value)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import quality_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
EPS = 2.0 ** -53
SSIM_TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _pair(ang, C_, H, W, sigma, masked=1):
    """(clean, noisy, mask): the golden 3 x 3 light field (256 x 256 SAIs) cropped, or the synthetic 5 x 5 one; SAI `masked` is empty
    and holds NaN."""
    if ang == 3:
        assert H <= 256 and W <= 256
        y0, x0 = min(40, 256 - H), min(30, 256 - W)
        u8 = np.load(GOLDEN)[:, :C_, y0:y0 + H, x0:x0 + W]
    else:
        u8 = synth.make_lf(ang, ang, H, W)[:, :C_]
    A = ang * ang
    assert u8.shape == (A, C_, H, W)
    clean = np.ascontiguousarray(u8, np.float32).reshape(A, -1)
    noisy = synth.add_noise_mt19937(clean, sigma, seed=3)
    mask = np.ones(A, np.uint32)
    if masked is not None:
        mask[masked] = 0
        clean[masked] = np.nan
        noisy[masked] = np.nan
    return clean, noisy, mask


def _mse_tol(C_, H, W):
    return 2.0 * (C_ * H * W + 2) * EPS


def _assert_parity(g, r, mask, C_, H, W, peak=255.0, ssim=True):
    rel = _mse_tol(C_, H, W)
    on = mask != 0
    for name, a in (("psnr", g.psnr_sai), ("rmse", g.rmse_sai)) + ((("ssim", g.ssim_sai),) if ssim else ()):
        assert np.all(a[~on] == 0.0), name                               # empty SAIs: exactly 0
        assert np.isfinite(a).all(), name
        print(name, "max |gpu - model|", np.abs(a - r[name + "_sai"]).max())
    assert np.all(np.abs(g.rmse_sai - r["rmse_sai"]) <= (rel / 2 + 2 * EPS) * r["rmse_sai"])
    psnr_tol = 10.0 / np.log(10.0) * rel + 8 * EPS * np.abs(r["psnr_sai"])
    assert np.all(np.abs(g.psnr_sai - r["psnr_sai"]) <= psnr_tol)
    assert g.count == r["count"] == int(on.sum())
    assert abs(g.mse - r["mse"]) <= rel * r["mse"]
    assert abs(g.rmse_mean - r["rmse_mean"]) <= (rel / 2 + 2 * EPS) * r["rmse_mean"]
    assert abs(g.psnr_mean - r["psnr_mean"]) <= psnr_tol.max()
    # a standard deviation moves by no more than the largest error of an entry: the per-SAI absolute tolerances
    assert abs(g.rmse_std - r["rmse_std"]) <= (rel / 2 + 2 * EPS) * r["rmse_sai"].max()
    assert abs(g.psnr_std - r["psnr_std"]) <= psnr_tol.max()
    if ssim:
        assert np.all(np.abs(g.ssim_sai - r["ssim_sai"]) <= SSIM_TOL)
        assert abs(g.ssim_mean - r["ssim_mean"]) <= SSIM_TOL and abs(g.ssim_std - r["ssim_std"]) <= SSIM_TOL
    else:
        assert g.ssim_sai is None and g.ssim_mean is None and g.ssim_std is None


def _raw(ctx, d_ref, d_test, mask, W, H, C_, peak=255.0, ssim=1):
    """The C-ABI call itself: (rc, summary struct, mse [asize], ssim [asize])."""
    lib, res = core.lib(), core.QualityStruct()
    mse, ss = np.full(mask.size, -1.0), np.full(mask.size, -1.0)
    dp = C.POINTER(C.c_double)
    rc = lib.lfbm5d_quality_device(ctx._h, C.c_void_p(d_ref.data_ptr()), C.c_void_p(d_test.data_ptr()), mask.ctypes.data_as(C.POINTER(C.c_uint)),
                                   mask.size, W, H, C_, peak, ssim, C.byref(res), mse.ctypes.data_as(dp), ss.ctypes.data_as(dp))
    return rc, res, mse, ss


# (H, W): one window position; one row of 20; exactly 64 window columns (one wave); 65 (the second wave holds one); three waves;
# 256 window columns (one workgroup) and 257; 55 / 56 / 57 window rows around the row tile of 56; two staged chunks of 11 input rows
# exactly, and one row more
SIZES = [(11, 11), (11, 30), (12, 74), (27, 75), (43, 139), (12, 266), (11, 267), (65, 23), (66, 30), (67, 21), (22, 13), (23, 11)]
SIGMAS = [0.5, 2.0, 25.0, 50.0]


@pytest.mark.gpu
@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("i,HW", list(enumerate(SIZES)), ids=["%dx%d" % hw for hw in SIZES])
def test_parity_with_the_model(ctx, i, HW, C_):
    H, W = HW
    ang, sigma = (3, 5)[(i + C_ // 3) % 2] if W <= 256 else 5, SIGMAS[(i // 2 + C_) % 4]     # the golden SAIs are 256 wide
    clean, noisy, mask = _pair(ang, C_, H, W, sigma)
    g = ctx.quality(_dev(clean), _dev(noisy), mask, W, H, C_)
    r = Q.model(clean, noisy, mask, W, H, C_)
    _assert_parity(g, r, mask, C_, H, W)
    rc, res, mse, ss = _raw(ctx, _dev(clean), _dev(noisy), mask, W, H, C_)
    assert rc == 0 and mse[1] == 0.0 and ss[1] == 0.0 and np.isfinite(mse).all() and np.isfinite(ss).all()
    print("mse max relative difference", (np.abs(mse - r["mse_sai"])[mask != 0] / r["mse_sai"][mask != 0]).max(), "bound", _mse_tol(C_, H, W))
    assert np.all(np.abs(mse - r["mse_sai"]) <= _mse_tol(C_, H, W) * r["mse_sai"])
    assert np.all(np.abs(ss - r["ssim_sai"]) <= SSIM_TOL)
    for k in ("psnr_mean", "psnr_std", "rmse_mean", "rmse_std", "ssim_mean", "ssim_std", "mse"):
        assert np.isfinite(getattr(res, k)), k


@pytest.mark.gpu
@pytest.mark.parametrize("HW", [(5, 7), (10, 300), (70, 9), (67, 267)])
def test_mse_alone_parity_also_below_the_window_size(ctx, HW):
    H, W = HW
    clean, noisy, mask = _pair(3 if W <= 256 else 5, 3, H, W, 25.0)
    g = ctx.quality(_dev(clean), _dev(noisy), mask, W, H, 3, ssim=False)
    r = Q.model(clean, noisy, mask, W, H, 3, want_ssim=False)
    _assert_parity(g, r, mask, 3, H, W, ssim=False)
    rc, res, mse, ss = _raw(ctx, _dev(clean), _dev(noisy), mask, W, H, 3, ssim=0)
    assert rc == 0 and np.all(np.abs(mse - r["mse_sai"]) <= _mse_tol(3, H, W) * r["mse_sai"]) and np.all(ss == 0.0)


@pytest.mark.gpu
def test_closed_forms(ctx):
    H, W = 30, 75
    clean, noisy, mask = _pair(3, 3, H, W, 25.0)
    d = _dev(noisy)
    g = ctx.quality(d, d, mask, W, H, 3)                                   # identical inputs
    on = mask != 0
    assert np.all(g.rmse_sai == 0.0) and g.mse == 0.0 and np.all(g.psnr_sai[on] == np.inf) and g.psnr_mean == np.inf
    assert np.all(np.abs(g.ssim_sai[on] - 1.0) <= 1e-12) and abs(g.ssim_mean - 1.0) <= 1e-12 and np.all(g.ssim_sai[~on] == 0.0)
    for c1v, c2v, peak in ((100.0, 140.0, 255.0), (0.0, 255.0, 255.0), (0.25, 0.75, 1.0), (17.0, 17.0, 0.0)):   # constant images
        a, b = np.full((9, 3 * H * W), c1v, np.float32), np.full((9, 3 * H * W), c2v, np.float32)
        g = ctx.quality(_dev(a), _dev(b), np.ones(9, np.uint32), W, H, 3, peak=peak)
        k1 = (0.01 * (peak or 255.0)) ** 2
        want = (2 * c1v * c2v + k1) / (c1v ** 2 + c2v ** 2 + k1)
        assert np.all(np.abs(g.ssim_sai - want) <= 1e-9) and abs(g.ssim_mean - want) <= 1e-9
        assert np.all(g.rmse_sai == abs(c1v - c2v)) and g.mse == (c1v - c2v) ** 2


@pytest.mark.gpu
def test_scale_invariance_with_peak_one(ctx):
    """peak = 1 on the inputs scaled by 1 / 255 gives the psnr and ssim of peak = 255.  For the scaling to be exact in float32 the
    inputs are multiples of 255 / 4096 (the scaled ones multiples of 1 / 4096 in 0..2: 13 bits, times 255: 21 bits); what is left is
    the rounding of two double computations of the same real quantity: the bounds of this file."""
    H, W, C_ = 43, 139, 3
    clean, noisy, mask = _pair(5, C_, H, W, 25.0)
    on = mask != 0
    s_clean, s_noisy = (np.where(np.isnan(x), x, np.round(np.clip(x, -255, 510) / 255.0 * 4096.0) / 4096.0).astype(np.float32) for x in (clean, noisy))
    b_clean, b_noisy = s_clean * np.float32(255.0), s_noisy * np.float32(255.0)
    assert np.array_equal(b_clean[on].astype(np.float64), s_clean[on].astype(np.float64) * 255.0)      # exact
    assert np.array_equal(b_noisy[on].astype(np.float64), s_noisy[on].astype(np.float64) * 255.0)
    g1 = ctx.quality(_dev(s_clean), _dev(s_noisy), mask, W, H, C_, peak=1.0)
    g255 = ctx.quality(_dev(b_clean), _dev(b_noisy), mask, W, H, C_, peak=255.0)
    rel = _mse_tol(C_, H, W)
    assert np.all(np.abs(g1.rmse_sai * 255.0 - g255.rmse_sai) <= (rel / 2 + 3 * EPS) * g255.rmse_sai)
    psnr_tol = 10.0 / np.log(10.0) * rel + 8 * EPS * np.abs(g255.psnr_sai)
    assert np.all(np.abs(g1.psnr_sai - g255.psnr_sai) <= psnr_tol) and abs(g1.psnr_mean - g255.psnr_mean) <= psnr_tol.max()
    assert np.all(np.abs(g1.ssim_sai - g255.ssim_sai) <= SSIM_TOL) and abs(g1.ssim_mean - g255.ssim_mean) <= SSIM_TOL
    _assert_parity(g1, Q.model(s_clean, s_noisy, mask, W, H, C_, peak=1.0), mask, C_, H, W)


def _bits(q):
    parts = [np.array([q.psnr_mean, q.psnr_std, q.rmse_mean, q.rmse_std, q.mse, float(q.count)]), q.psnr_sai, q.rmse_sai]
    if q.ssim_sai is not None:
        parts += [np.array([q.ssim_mean, q.ssim_std]), q.ssim_sai]
    return np.concatenate(parts).view(np.uint64)


@pytest.mark.gpu
def test_determinism_host_form_and_read_only_inputs(ctx):
    H, W, C_ = 70, 300, 3                                                   # two row tiles, two column tiles
    clean, noisy, mask = _pair(5, C_, H, W, 25.0, masked=7)
    d_ref, d_test = _dev(clean), _dev(noisy)
    a = ctx.quality(d_ref, d_test, mask, W, H, C_)
    b = ctx.quality(d_ref, d_test, mask, W, H, C_)
    assert np.array_equal(_bits(a), _bits(b))
    for d, src in ((d_ref, clean), (d_test, noisy)):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), src.view(np.uint32))
    h = ctx.quality(clean, noisy, mask, W, H, C_)                           # host form, flat arrays
    assert np.array_equal(_bits(a), _bits(h))
    per_sai = lambda x: [x[i].copy() if mask[i] else None for i in range(25)]
    h2 = ctx.quality(per_sai(clean), per_sai(noisy), mask, W, H, C_)        # one array per SAI, none for the empty one
    assert np.array_equal(_bits(a), _bits(h2))
    m = ctx.quality(d_ref, d_test, mask, W, H, C_, ssim=False)              # the squared error of the call without SSIM
    assert m.ssim_sai is None
    assert np.array_equal(_bits(m), _bits(a._replace(ssim_mean=None, ssim_std=None, ssim_sai=None)))
    rc, res, mse, ss = _raw(ctx, d_ref, d_test, mask, W, H, C_, ssim=0)
    rc1, res1, mse1, ss1 = _raw(ctx, d_ref, d_test, mask, W, H, C_, ssim=1)
    assert rc == 0 and rc1 == 0 and np.array_equal(mse.view(np.uint64), mse1.view(np.uint64)) and np.all(ss == 0.0) and res.has_ssim == 0


@pytest.mark.gpu
def test_rejected_inputs(ctx):
    H, W = 27, 75
    clean, noisy, mask = _pair(3, 3, H, W, 25.0)
    d_ref, d_test = _dev(clean), _dev(noisy)
    bad = [dict(chnls=2), dict(chnls=0), dict(mask=np.zeros(9, np.uint32)), dict(peak=-1.0), dict(peak=float("nan")), dict(peak=float("inf")),
           dict(width=10, height=27), dict(width=75, height=10)]
    for kw in bad:
        args = dict(mask=mask, width=W, height=H, chnls=3, peak=255.0)
        args.update(kw)
        with pytest.raises(L.LfBm5dError) as e:
            ctx.quality(d_ref, d_test, args["mask"], args["width"], args["height"], args["chnls"], peak=args["peak"])
        assert str(e.value), kw
    lib, h = core.lib(), ctx._h
    res = core.QualityStruct()
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint))
    r, t = C.c_void_p(d_ref.data_ptr()), C.c_void_p(d_test.data_ptr())
    ptrs_r, ptrs_t = core._sai_ptrs(list(clean), mask), core._sai_ptrs(list(noisy), mask)
    cases = [(lib.lfbm5d_quality_device, None, t, mp, C.byref(res)), (lib.lfbm5d_quality_device, r, None, mp, C.byref(res)),
             (lib.lfbm5d_quality_device, r, t, None, C.byref(res)), (lib.lfbm5d_quality_device, r, t, mp, None),
             (lib.lfbm5d_quality_host_sai, None, ptrs_t, mp, C.byref(res)), (lib.lfbm5d_quality_host_sai, ptrs_r, None, mp, C.byref(res)),
             (lib.lfbm5d_quality_host_sai, ptrs_r, ptrs_t, None, C.byref(res)), (lib.lfbm5d_quality_host_sai, ptrs_r, ptrs_t, mp, None)]
    for fn, a, b, m, out in cases:
        assert fn(h, a, b, m, 9, W, H, 3, 255.0, 1, out, None, None) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    for missing in (0, 1):                                                # a non-empty SAI without a pointer, in either light field
        ptrs = [core._sai_ptrs(list(clean), mask), core._sai_ptrs(list(noisy), mask)]
        ptrs[missing][4] = None
        assert lib.lfbm5d_quality_host_sai(h, ptrs[0], ptrs[1], mp, 9, W, H, 3, 255.0, 1, C.byref(res), None, None) == 1
        assert "non-empty SAI" in lib.lfbm5d_last_error(h).decode()
    g = ctx.quality(d_ref, d_test, mask, W, H, 3)                          # the context still works
    _assert_parity(g, Q.model(clean, noisy, mask, W, H, 3), mask, 3, H, W)
    assert ctx.quality(d_ref, d_test, mask, W, H, 3, ssim=False).count == 8


@pytest.mark.gpu
def test_python_forms_agree_with_the_c_abi(ctx):
    H, W, C_ = 43, 139, 3
    clean, noisy, mask = _pair(3, C_, H, W, 2.0)
    d_ref, d_test = _dev(clean), _dev(noisy)
    rc, res, mse, ss = _raw(ctx, d_ref, d_test, mask, W, H, C_)
    assert rc == 0 and res.has_ssim == 1 and res.count == 8
    summ = L.quality_summary(mse, ss, mask)                                 # the device forms call the host-only summary
    for q in (ctx.quality(d_ref, d_test, mask, W, H, C_), ctx.quality(clean, noisy, mask, W, H, C_), L.quality(d_ref, d_test, mask, W, H, C_),
              L.quality(clean, noisy, mask, W, H, C_, ctx=ctx)):
        assert isinstance(q, L.Quality)
        assert np.array_equal(q.rmse_sai.view(np.uint64), np.sqrt(mse).view(np.uint64)) and np.array_equal(q.ssim_sai.view(np.uint64), ss.view(np.uint64))
        for k in ("psnr_mean", "psnr_std", "rmse_mean", "rmse_std", "ssim_mean", "ssim_std", "mse"):
            assert getattr(q, k) == getattr(res, k) == getattr(summ, k), k
        assert np.array_equal(_bits(q), _bits(summ))


def _write_lf(tmp, lf):
    from PIL import Image
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src


def _read_lf(d):
    from PIL import Image
    return np.stack([np.asarray(Image.open(f"{d}/SAI_{s + 1:02d}_{t + 1:02d}.png")).transpose(2, 0, 1)
                     for s in range(3) for t in range(3)]).astype(np.float32).reshape(9, -1)


@pytest.mark.gpu
def test_cli_reports_ssim_on_request_only(tmp_path):
    """The README test command on a 96 x 128 crop of the golden SAIs.  With LFBM5D_REPORT_SSIM=1 the average SSIM printed next to every
    average PSNR is the model's on the PNG files the command wrote (the command computes it on the images as the files hold them),
    to the six digits printed: one unit of the last digit covers the print's half unit and the float the drop-in returns (6e-8
    relative); the results file holds an SSIM block per PSNR block.  Without the variable neither shows the word."""
    H, W = 96, 128
    lf = np.ascontiguousarray(np.load(GOLDEN)[:, :, 80:80 + H, 64:64 + W])
    runs = {}
    for mode in ("ssim", "plain"):
        tmp = os.path.join(str(tmp_path), mode)
        os.makedirs(tmp)
        src = _write_lf(tmp, lf)
        args = [CLI, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic", f"{tmp}/denoised",
                f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4", "dct", "sadct", "haar", "0", "opp",
                "0", f"{tmp}/measures.txt"]
        env = dict(os.environ, LFBM5D_SEED="1")
        env.pop("LFBM5D_REPORT_SSIM", None)
        if mode == "ssim":
            env["LFBM5D_REPORT_SSIM"] = "1"
        out = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:]
        runs[mode] = (tmp, out.stdout, open(f"{tmp}/measures.txt").read())
    tmp, stdout, txt = runs["ssim"]
    clean = np.ascontiguousarray(lf, np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    for what, line in (("noisy", "Noisy"), ("basic", "Basic"), ("denoised", "Denoised")):
        r = Q.model(clean, _read_lf(f"{tmp}/{what}"), mask, W, H, 3)
        shown = re.findall(r"- %s light field: \S+ \(SSIM ([0-9.eE+-]+)\)" % line, stdout)
        assert shown, stdout[-2000:]
        unit = 10.0 ** (np.floor(np.log10(r["ssim_mean"])) - 5)
        print(what, "SSIM printed", shown[-1], "model", r["ssim_mean"], "std", r["ssim_std"])
        assert all(abs(float(v) - r["ssim_mean"]) <= unit for v in shown)
        block = txt.split(f"-> Average SSIM {what} = ")[1]
        assert abs(float(block.split()[0]) - r["ssim_mean"]) <= unit
        assert abs(float(block.split(f"-> Standard deviation SSIM {what} = ")[1].split()[0]) - r["ssim_std"]) <= unit
        grid = block.split(f"SSIM for all {what} SAIs:\n")[1].split("\n")[:3]
        vals = np.array([[float(v) for v in row.split()] for row in grid])
        assert vals.shape == (3, 3) and np.all(np.abs(vals.reshape(-1) - r["ssim_sai"]) <= 10.0 ** (np.floor(np.log10(r["ssim_sai"])) - 5))
    assert txt.index("-> Average PSNR noisy") < txt.index("-> Average SSIM noisy") < txt.index("-> Average PSNR basic")
    tmp0, stdout0, txt0 = runs["plain"]
    assert "SSIM" not in txt0 and "SSIM" not in stdout0
    # the rest of the file is as it was: the same text around the numbers (the filter's sums are float atomics: the last digit of a
    # PSNR may differ between two runs), and the noisy light field's block, which no kernel touches, byte for byte
    rest = "".join(re.split(r"\n\*+\n-> Average SSIM .*?\n\*+\n", txt, flags=re.S))
    blank = lambda t: re.sub(r"[0-9.eE+-]+(?= |\n)", "#", t)
    assert blank(rest) == blank(txt0)
    assert rest.split("-> Average PSNR basic")[0] == txt0.split("-> Average PSNR basic")[0]
