"""CPU tests of the quality metrics (lfbm5d_quality_*, include/lfbm5d.h): the declarations and exports, the host-only summary against
numpy, self-checks of the float64 model (tests/quality_model.py) the GPU tests compare with, and the CLIs' LFBM5D_REPORT_SSIM
parsing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from oracle import oracle as O
import quality_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
ENTRY_POINTS = ("lfbm5d_quality_device", "lfbm5d_quality_host_sai", "lfbm5d_quality_summary")


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    lib = C.CDLL(core.library_path())
    for n in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % n, header), n
        assert hasattr(lib, n), n
    assert "} lfbm5d_quality;" in header
    assert C.sizeof(core.QualityStruct) == 7 * 8 + 2 * 4


def test_package_exports_quality():
    for n in ("Quality", "quality", "quality_summary"):
        assert n in L.__all__ and hasattr(L, n), n
    assert {"psnr_mean", "psnr_std", "rmse_mean", "rmse_std", "ssim_mean", "ssim_std", "mse", "count", "psnr_sai", "rmse_sai",
            "ssim_sai"} <= set(L.Quality._fields)
    assert hasattr(L.Context, "quality")


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("n,peak", [(9, 255.0), (25, 1.0), (289, 0.0), (1, 255.0)])
def test_summary_matches_numpy_and_ignores_empty_sais(n, peak):
    rng = np.random.default_rng(n)
    mse = 10.0 ** rng.uniform(-3, 3, n) * (peak or 255.0) ** 2 / 255.0 ** 2
    ssim = rng.uniform(0.1, 1.0, n)
    mask = (rng.uniform(size=n) < 0.8).astype(np.uint32)
    mask[n // 2] = 1
    mse[mask == 0], ssim[mask == 0] = np.nan, np.inf                 # whatever empty SAIs hold is not looked at
    q = L.quality_summary(mse, ssim, mask, peak)
    r = Q.summary(mse, ssim, mask, peak or 255.0)
    assert q.count == r["count"] == int(mask.sum())
    for k in ("psnr_mean", "rmse_mean", "ssim_mean", "mse"):
        assert _rel(getattr(q, k), r[k]) <= 1e-12, k
    for k in ("psnr_std", "rmse_std", "ssim_std"):
        assert abs(getattr(q, k) - r[k]) <= 1e-12 * r[k], k          # (one SAI: both exactly 0)
    on = mask != 0
    np.testing.assert_allclose(q.psnr_sai[on], Q.psnr_of(mse[on], peak or 255.0), rtol=1e-14)
    np.testing.assert_allclose(q.rmse_sai[on], np.sqrt(mse[on]), rtol=1e-15)
    assert np.array_equal(q.ssim_sai[on], ssim[on])
    for a in (q.psnr_sai, q.rmse_sai, q.ssim_sai):
        assert np.all(a[~on] == 0.0)
    p = L.quality_summary(mse, None, mask, peak)                     # without SSIM
    assert p.ssim_mean is None and p.ssim_std is None and p.ssim_sai is None
    assert (p.psnr_mean, p.psnr_std, p.rmse_mean, p.rmse_std, p.mse) == (q.psnr_mean, q.psnr_std, q.rmse_mean, q.rmse_std, q.mse)


def test_summary_one_exact_sai_makes_the_mean_infinite():
    mse, mask = np.array([4.0, 0.0, 9.0, 1.0]), np.array([1, 1, 1, 0], np.uint32)
    q = L.quality_summary(mse, None, mask)
    assert q.psnr_mean == np.inf and np.isnan(q.psnr_std)
    assert q.psnr_sai[1] == np.inf and q.rmse_sai[1] == 0.0
    assert q.rmse_mean == (2.0 + 0.0 + 3.0) / 3 and q.mse == 13.0 / 3 and q.count == 3


def test_summary_rejects_bad_arguments():
    mse, mask = np.array([4.0, 1.0]), np.ones(2, np.uint32)
    for kw in (dict(mask=np.zeros(2, np.uint32)), dict(peak=-1.0), dict(peak=np.nan), dict(peak=np.inf), dict(mask=np.ones(3, np.uint32))):
        with pytest.raises(L.LfBm5dError):
            L.quality_summary(mse, None, kw.get("mask", mask), kw.get("peak", 255.0))
    lib, res = core.lib(), core.QualityStruct()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint)
    m, k = mse.ctypes.data_as(dp), mask.ctypes.data_as(up)
    assert lib.lfbm5d_quality_summary(m, None, k, 2, 255.0, C.byref(res)) == 0
    assert lib.lfbm5d_quality_summary(None, None, k, 2, 255.0, C.byref(res)) == 1
    assert lib.lfbm5d_quality_summary(m, None, None, 2, 255.0, C.byref(res)) == 1
    assert lib.lfbm5d_quality_summary(m, None, k, 2, 255.0, None) == 1
    assert lib.lfbm5d_quality_summary(m, None, k, 0, 255.0, C.byref(res)) == 1


def _crop(H=40, W=52, C_=3):
    return np.ascontiguousarray(np.load(GOLDEN)[:, :C_, 60:60 + H, 70:70 + W], np.float32).reshape(9, -1)


def test_model_ssim_of_an_image_with_itself_is_one():
    a = synth.add_noise_mt19937(_crop(), 25.0, seed=2)
    for st in (0, 4):
        assert abs(Q.ssim(a[st], a[st], 3, 40, 52) - 1.0) <= 1e-12
    assert Q.mse(a[0], a[0]) == 0.0 and Q.psnr_of(0.0) == np.inf


@pytest.mark.parametrize("c1v,c2v,peak", [(100.0, 140.0, 255.0), (0.0, 255.0, 255.0), (0.25, 0.75, 1.0), (17.0, 17.0, 255.0)])
def test_model_ssim_of_constant_images(c1v, c2v, peak):
    a, b = np.full((1, 13, 17), c1v, np.float32), np.full((1, 13, 17), c2v, np.float32)
    k1 = (0.01 * peak) ** 2
    assert abs(Q.ssim(a, b, 1, 13, 17, peak) - (2 * c1v * c2v + k1) / (c1v ** 2 + c2v ** 2 + k1)) <= 1e-9


def test_model_psnr_matches_the_oracle():
    """The oracle's PSNR is the reference's float-accumulated value (compute_psnr); the model's is the same quantity in double."""
    clean = _crop(64, 64)
    for sigma in (2.0, 25.0):
        noisy = synth.add_noise_mt19937(clean, sigma, seed=1)
        r = Q.model(clean, noisy, np.ones(9, np.uint32), 64, 64, 3, want_ssim=False)
        for st in (0, 8):
            assert abs(r["psnr_sai"][st] - O.psnr(clean[st], noisy[st])) <= 1e-3
        assert abs(r["psnr_mean"] - O.psnr_lf(clean, noisy)) <= 1e-3


def test_model_window():
    w = Q.window()
    assert w.shape == (11, 11) and abs(w.sum() - 1.0) <= 1e-15 and np.array_equal(w, w.T)
    assert abs(w[5, 5] / w[5, 4] - np.exp(1.0 / 4.5)) <= 1e-14


def _denoise_args(cli, tmp):
    if cli == "LFBM3Ddenoising":
        return ["none", "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic", f"{tmp}/denoised",
                f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8", f"{tmp}/measures.txt"]
    if cli == "LFBM5Dsuperres":
        return [f"{tmp}/low", "SAI", "_", "3", "3", "1", "1", "1", "row", "2", "bicubic", "0", "0", "0", "0", f"{tmp}/out", "8", "18", "6", "16",
                "4", "id", "sadct", "haar", "0", "opp"]
    return ["none", "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic", f"{tmp}/denoised",
            f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4", "dct", "sadct", "haar", "0", "opp",
            "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising", "LFBM5Dsuperres"])
def test_cli_rejects_an_unknown_ssim_mode(tmp_path, cli):
    """LFBM5D_REPORT_SSIM accepts "1" only; anything else stops the command before it reads a file or touches a GPU."""
    args = [os.path.join(ROOT, "lfbm5d_amd", cli)] + _denoise_args(cli, str(tmp_path))
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_REPORT_SSIM="yes"), timeout=120)
    assert r.returncode != 0 and "LFBM5D_REPORT_SSIM must be" in r.stdout
