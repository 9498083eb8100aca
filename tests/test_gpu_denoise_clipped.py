"""GPU tests of the job on clipped data (lfbm5d_denoise_clipped_*, include/lfbm5d.h) on the tile rows 192..255, columns 128..191 of the
golden light field (dark: a third to a half of its blocks hold a clipped pixel), rounded and clipped: the job against its calls made by
hand, the plain and the declipped result against the checker (oracle.run_step1 / run_step2, then the float64 inverse of
tests/clip_model.py), and the gain over the plain job."""
import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from oracle import oracle as O
import clip_model as M
import helpers as Hh

MASK = np.ones(9, np.uint32)
TAIL = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
# sigma -> (hard-thresholding parameters, Wiener parameters, gain of the CPU composition over the plain result in dB: 32.256 -> 32.987 and
# 26.475 -> 29.037, oracle then model inverse)
CASES = {25.0: (Hh.README_HT, Hh.README_WIEN, 0.73), 50.0: (Hh.C5_HT, Hh.C5_WIEN, 2.56)}


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


def _psnr(x, clean):
    return float(10.0 * np.log10(255.0 ** 2 / ((np.asarray(x, np.float64) - clean) ** 2).mean()))


def _key(e):
    """A ClipNoiseLevel as a tuple that compares bit for bit (NaN equals NaN)."""
    return tuple(float(v).hex() if isinstance(v, float) else v for v in (e.sigma, *e.sigma_channel, *e[2:]))


def _tile(sigma):
    u8 = np.ascontiguousarray(Hh.source_lf()[:, :, 192:256, 128:192])
    clean, noisy = Hh.noisy_lf(u8, sigma)
    return clean, synth.clip_round(noisy)


def _params(sigma, pk):
    return core.make_params(sigma, 2.7, *pk)


@pytest.fixture(scope="module")
def checker():
    """sigma -> (clean, clipped noisy, the checker's denoised result, its declipped form in float64), computed once."""
    out = {}
    for sigma, (ht, wi, _) in CASES.items():
        clean, cl = _tile(sigma)
        n1, b, _ = O.run_step1(O.make_params(sigma, 2.7, *ht), cl.copy(), MASK, O.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        _, _, d, _ = O.run_step2(O.make_params(sigma, 2.7, *wi), n1.copy(), b.copy(), MASK, O.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        out[sigma] = (clean, cl, d, M.declip(d, sigma))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", sorted(CASES))
def test_job_with_a_given_sigma(ctx, checker, sigma):
    """Measured on an MI355X (profiles/clip.txt): sigma 25: plain 32.258, declipped 32.989 dB; sigma 50: plain 26.475, declipped
    29.037 dB."""
    import torch
    ht, wi, cpu_gain = CASES[sigma]
    clean, cl, o_plain, o_declipped = checker[sigma]
    # the job
    d = _dev(cl)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    used, est = ctx.denoise_clipped(sigma, _params(1.0, ht), _params(99.0, wi), d, MASK, basic, den, *TAIL)   # the sigmas passed are ignored
    assert used == sigma and est is None
    # by hand: denoise, declip, declip
    d2 = _dev(cl)
    b2, p2 = torch.zeros_like(d), torch.zeros_like(d)
    ctx.denoise(_params(sigma, ht), _params(sigma, wi), d2, MASK, b2, p2, *TAIL)
    plain = p2.cpu().numpy()
    ctx.declip(sigma, b2, MASK, b2, 64, 64, 3)
    ctx.declip(sigma, p2, MASK, p2, 64, 64, 3)
    assert np.array_equal(_bits(basic), _bits(b2)) and np.array_equal(_bits(den), _bits(p2))
    assert np.array_equal(_bits(d), _bits(d2))                               # d_noisy is left as denoise() leaves it
    # against the checker
    g = den.cpu().numpy()
    p_plain, p_decl = _psnr(plain, clean), _psnr(g, clean)
    po_plain, po_decl = _psnr(o_plain, clean), _psnr(o_declipped, clean)
    print(f"sigma = {sigma}: plain GPU {p_plain:.3f} dB (checker {po_plain:.3f}), declipped GPU {p_decl:.3f} dB (checker and model "
          f"inverse {po_decl:.3f}), gain {p_decl - p_plain:.3f} dB (CPU composition {po_decl - po_plain:.3f})")
    assert abs(po_decl - po_plain - cpu_gain) < 0.01                         # the checker reproduces the composition's figures
    assert abs(p_plain - po_plain) <= 0.01                                   # the project's tolerance, as the baseline
    assert abs(p_decl - po_decl) <= 0.02                                     # twice that: the inverse's slope is at most 2
    assert p_decl - p_plain >= 0.5 * cpu_gain
    assert _psnr(basic.cpu().numpy(), clean) > _psnr(cl, clean) + 3.0
    # host forms: flat arrays, one array per SAI
    hb, hd = np.zeros_like(cl), np.zeros_like(cl)
    noisy_h = cl.copy()
    assert ctx.denoise_clipped(sigma, _params(1.0, ht), _params(1.0, wi), noisy_h, MASK, hb, hd, *TAIL) == (sigma, None)
    assert np.array_equal(hb.view(np.uint32), _bits(basic)) and np.array_equal(hd.view(np.uint32), _bits(den))
    assert np.array_equal(noisy_h, cl)                                       # the host form only reads it
    if sigma == 25.0:
        lb, ld = ([np.zeros(cl.shape[1], np.float32) for _ in range(9)] for _ in range(2))
        L.denoise_clipped(sigma, _params(1.0, ht), _params(1.0, wi), [cl[i].copy() for i in range(9)], MASK, lb, ld, *TAIL, ctx=ctx)
        assert np.array_equal(np.stack(ld).view(np.uint32), _bits(den))


@pytest.mark.gpu
def test_job_estimates_sigma_when_none_is_given(ctx):
    import torch
    ht, wi, _ = CASES[25.0]
    clean, cl = _tile(25.0)
    d = _dev(cl)
    e = ctx.noise_level_clipped(d, MASK, 64, 64, 3)
    assert abs(e.sigma / 25.0 - 1.0) < 0.05
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    used, est = ctx.denoise_clipped(None, _params(1.0, ht), _params(1.0, wi), d, MASK, basic, den, *TAIL)
    assert used == e.sigma and _key(est) == _key(e)
    d2 = _dev(cl)
    b2, p2 = torch.zeros_like(d), torch.zeros_like(d)
    ctx.denoise(_params(e.sigma, ht), _params(e.sigma, wi), d2, MASK, b2, p2, *TAIL)
    ctx.declip(e.sigma, b2, MASK, b2, 64, 64, 3)
    ctx.declip(e.sigma, p2, MASK, p2, 64, 64, 3)
    assert np.array_equal(_bits(basic), _bits(b2)) and np.array_equal(_bits(den), _bits(p2))
    # a negative sigma means the same
    d3 = _dev(cl)
    b3, p3 = torch.zeros_like(d), torch.zeros_like(d)
    used3, est3 = ctx.denoise_clipped(-1.0, _params(1.0, ht), _params(1.0, wi), d3, MASK, b3, p3, *TAIL)
    assert used3 == used and _key(est3) == _key(est)
    assert np.array_equal(_bits(p3), _bits(den))
    print(f"sigma = None: estimated {used:.3f}, declipped {_psnr(den.cpu().numpy(), clean):.3f} dB")
