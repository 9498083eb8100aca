"""GPU tests of the blind noise-level estimate (lfbm5d_noise_level_*, include/lfbm5d.h) against the float64 numpy model
(tests/noise_model.py) on the same float32 input: parity, the accuracy table, determinism, rejected inputs, the CLIs and Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from noise_model import model

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


def _assert_parity(g, r, rel=1e-4):
    lam = r["eigen"]
    assert g.components == r["components"]
    assert g.patches == r["patches"]
    assert np.abs(g.eigen - lam).max() <= 1e-7 * lam.max()
    assert abs(g.sigma - r["sigma"]) <= rel * r["sigma"]
    np.testing.assert_allclose(g.sigma_channel, r["sigma_channel"][:len(g.sigma_channel)], rtol=rel)
    if r["sigma_sai"] is not None:
        np.testing.assert_allclose(g.sigma_sai, r["sigma_sai"], rtol=rel)


def _parity_lf(ang, C_, H=53, W=67, sigma=10.0):
    if ang == 3:
        u8 = np.load(GOLDEN)[:, :C_, 40:40 + H, 30:30 + W]
    else:
        u8 = synth.make_lf(ang, ang, H, W)[:, :C_]
    A = ang * ang
    lf = synth.add_noise_mt19937(np.ascontiguousarray(u8, np.float32).reshape(A, -1), sigma, seed=3)
    mask = np.ones(A, np.uint32)
    mask[1] = 0
    lf[1] = 0.0
    return lf, mask


@pytest.mark.gpu
@pytest.mark.parametrize("ang,C_,r", [(3, 1, 4), (3, 3, 6), (3, 3, 8), (5, 1, 6), (5, 3, 8), (5, 3, 4), (3, 1, 8), (5, 1, 5)])
def test_parity_with_the_model(ctx, ang, C_, r):
    H, W = 53, 67
    lf, mask = _parity_lf(ang, C_, H, W)
    g = ctx.noise_level(_dev(lf), mask, W, H, C_, patch=r, per_sai=True)
    _assert_parity(g, model(lf, mask, W, H, C_, r, per_sai=True))
    assert g.sigma_sai[1] == 0.0 and len(g.eigen) == r * r


# (input, sigma) -> the model's estimate; golden rows float and clipped, synthetic 5x5x128x128 rows (noise alone, seed 1)
TABLE = {("golden", 2): 2.648, ("golden", 5): 5.293, ("golden", 10): 10.174, ("golden", 25): 25.119, ("golden", 50): 50.134,
         ("synth", 2): 2.125, ("synth", 10): 10.063, ("synth", 25): 25.084, ("synth", 50): 50.105,
         ("clipped", 2): 2.661, ("clipped", 5): 5.283, ("clipped", 10): 10.097, ("clipped", 25): 24.111, ("clipped", 50): 45.102}
SIGMA0 = {"golden": 1.739, "synth": 0.716}   # the model on the clean light fields (photographic noise / synthetic texture)


@pytest.mark.gpu
def test_accuracy_table(ctx):
    golden = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    syn = synth.make_lf(5, 5, 128, 128).astype(np.float32).reshape(25, -1)
    for (kind, sigma), want in TABLE.items():
        clean, A, H, W = (syn, 25, 128, 128) if kind == "synth" else (golden, 9, 256, 256)
        x = synth.add_noise_mt19937(clean, sigma, seed=1)
        if kind == "clipped":
            x = np.clip(np.round(x), 0, 255).astype(np.float32)
        mask = np.ones(A, np.uint32)
        g = ctx.noise_level(_dev(x), mask, W, H, 3)
        r = model(x, mask, W, H, 3)
        _assert_parity(g, r)
        assert abs(g.sigma - want) <= 5e-4 + 1e-4 * want, (kind, sigma, g.sigma)
        if kind != "clipped":
            assert abs(g.sigma - np.hypot(sigma, SIGMA0[kind])) <= 0.03 * sigma + 0.2, (kind, sigma, g.sigma)


def _same(a, b):
    assert a.sigma == b.sigma and a.sigma_channel == b.sigma_channel and a.components == b.components and a.patches == b.patches
    assert np.array_equal(a.eigen, b.eigen)
    assert (a.sigma_sai is None) == (b.sigma_sai is None)
    if a.sigma_sai is not None:
        assert np.array_equal(a.sigma_sai, b.sigma_sai)


@pytest.mark.gpu
def test_determinism_host_form_and_read_only_input(ctx):
    lf, mask = _parity_lf(5, 3, 61, 77, sigma=25.0)
    d = _dev(lf)
    before = d.cpu().numpy().copy()
    a = ctx.noise_level(d, mask, 77, 61, 3, per_sai=True)
    b = ctx.noise_level(d, mask, 77, 61, 3, per_sai=True)
    _same(a, b)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), before.view(np.uint32))
    h = ctx.noise_level(lf, mask, 77, 61, 3, per_sai=True)                                    # host form, flat array
    _same(a, h)
    h2 = ctx.noise_level([lf[i].copy() if mask[i] else None for i in range(25)], mask, 77, 61, 3, per_sai=True)   # one array per SAI
    _same(a, h2)
    assert np.array_equal(lf.view(np.uint32), before.view(np.uint32))


@pytest.mark.gpu
def test_rejected_inputs(ctx):
    lf, mask = _parity_lf(3, 3, 53, 67)
    d = _dev(lf)
    bad = [dict(chnls=2), dict(patch=3), dict(patch=9), dict(width=15, height=53), dict(width=67, height=13, patch=7),
           dict(mask=np.zeros(9, np.uint32))]
    for kw in bad:
        args = dict(mask=mask, width=67, height=53, chnls=3, patch=8)
        args.update(kw)
        with pytest.raises(L.LfBm5dError) as e:
            ctx.noise_level(d, args["mask"], args["width"], args["height"], args["chnls"], patch=args["patch"])
        assert str(e.value), kw
    lib, h = core.lib(), ctx._h
    res = core.NoiseLevelStruct()
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint))
    cases = [(lib.lfbm5d_noise_level_device, None, mp, C.byref(res)),
             (lib.lfbm5d_noise_level_device, C.c_void_p(d.data_ptr()), None, C.byref(res)),
             (lib.lfbm5d_noise_level_device, C.c_void_p(d.data_ptr()), mp, None),
             (lib.lfbm5d_noise_level_host_sai, None, mp, C.byref(res))]
    for fn, buf, m, out in cases:
        assert fn(h, buf, m, 9, 67, 53, 3, 8, out, None, None) == 1
        assert lib.lfbm5d_last_error(h).decode()
    ptrs = (C.c_void_p * 9)()                       # non-empty SAIs without a pointer
    assert lib.lfbm5d_noise_level_host_sai(h, ptrs, mp, 9, 67, 53, 3, 8, C.byref(res), None, None) == 1
    assert "NULL" in lib.lfbm5d_last_error(h).decode()


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


def _estimate(stdout):
    m = re.search(r"Estimated noise level: sigma = ([0-9.eE+-]+)", stdout)
    assert m, stdout[-2000:]
    return float(m.group(1))


DENOISED_PSNR_AUTO = 35.678   # the README command with LFBM5D_SIGMA=auto (sigma 25.119 instead of 25), measured on an MI355X


@pytest.mark.gpu
def test_cli_sigma_auto(tmp_path):
    """README test command with LFBM5D_SEED=1 LFBM5D_SIGMA=auto: the estimate is the model's on that noise (tests/test_cli.py pins
    the noise); the denoised PSNR stays within 0.1 dB of the known-sigma run's 35.708 dB.  Then LFSourceDir = none on the noisy PNGs
    it wrote (rounded and clipped: the estimate is biased low), and LFBM3Ddenoising with the same variable."""
    tmp = str(tmp_path)
    src = _write_source_lf(tmp)
    env = dict(os.environ, LFBM5D_SEED="1", LFBM5D_SIGMA="auto")
    out = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:]
    est = _estimate(out.stdout)
    assert abs(est - 25.119396) <= 1e-4 * 25.119396, est
    txt = open(f"{tmp}/measures.txt").read()
    vals = {k: float(txt.split(f"-> Average PSNR {k} = ")[1].split()[0]) for k in ("noisy", "basic", "denoised")}
    print("LFBM5D_SIGMA=auto: estimate", est, "PSNR", vals)
    assert abs(vals["noisy"] - 20.1672) < 1e-3
    assert abs(vals["denoised"] - 35.7082) < 0.1
    assert abs(vals["denoised"] - DENOISED_PSNR_AUTO) < 0.01

    tmp2 = os.path.join(tmp, "none")
    for d in ("basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp2, d))
    args = _readme_args(CLI, tmp2, "none")
    args[13] = f"{tmp}/noisy"
    out = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_SIGMA="auto"))
    assert out.returncode == 0, out.stdout[-2000:]
    est2 = _estimate(out.stdout)
    print("LFSourceDir = none: estimate", est2)
    assert abs(est2 - 25.0) < 1.5
    assert os.path.exists(f"{tmp2}/denoised/SAI_02_02.png")

    tmp3 = os.path.join(tmp, "bm3d")
    os.makedirs(tmp3)
    src3 = _write_source_lf(tmp3)
    out = subprocess.run(_readme_args(CLI3, tmp3, src3), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:]
    est3 = _estimate(out.stdout)
    assert 20.0 < est3 < 30.0
    assert os.path.exists(f"{tmp3}/denoised/SAI_02_02.png")


@pytest.mark.gpu
def test_python_forms_and_denoise_with_the_estimate():
    import torch
    u8 = np.load(GOLDEN)[:, :, :64, :64]
    clean = np.ascontiguousarray(u8, np.float32).reshape(9, -1)
    noisy = synth.add_noise_mt19937(clean, 20.0, seed=1)
    mask = np.ones(9, np.uint32)
    a = L.noise_level(_dev(noisy), mask, 64, 64, 3)
    b = L.noise_level(noisy, mask, 64, 64, 3)
    _same(a, b)
    assert a.sigma_sai is None and len(a.sigma_channel) == 3 and a.patches == 9 * 3 * 57 * 57
    assert 15.0 < a.sigma < 25.0
    ctx = L.Context(0)
    try:
        P1 = core.make_params(a.sigma, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")
        P2 = core.make_params(a.sigma, 2.7, 16, 18, 6, 8, 4, "dct", "sadct", "haar")
        d_noisy = _dev(noisy)
        d_basic, d_den = torch.zeros_like(d_noisy), torch.zeros_like(d_noisy)
        ctx.denoise(P1, P2, d_noisy, mask, d_basic, d_den, L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
        den = d_den.cpu().numpy()
        assert np.isfinite(den).all()
        mse = lambda x: float(((x - clean) ** 2).mean())
        assert mse(den) < mse(noisy) / 4
    finally:
        ctx.close()
