"""CPU tests of the super-resolution operators' tap tables (lfbm5d_sr_taps / lfbm5d_sr_defaults, include/lfbm5d.h; host only, no
GPU) against the float64 model of tests/sr_model.py."""
import ctypes as C

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import sr_model as M

U24 = 2.0 ** -24
CASES = [(s, k, sb) for s in (2, 3, 4) for k, sbs in ((L.SR_BICUBIC, (0.8,)), (L.SR_GAUSSIAN, (0.8, 1.2, 1.6, 5.0))) for sb in sbs]


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("s,kernel,sb", CASES)
@pytest.mark.parametrize("n_low", [5, 13, 32])
def test_taps_agree_with_the_model(s, kernel, sb, n_low):
    sr = L.sr_defaults(s, kernel=kernel, blur_sigma=sb)
    for op, ref, n_in in (("up", M.taps_up(s, n_low), n_low), ("down", M.taps_down(s, kernel, sb, n_low * s), n_low * s)):
        first, w = L.sr_taps(op, sr, n_in)
        assert w.dtype == np.float32 and first.dtype == np.int32
        assert w.shape == ref[1].shape, (op, w.shape, ref[1].shape)          # n_out and T
        assert np.array_equal(first, ref[0])
        assert _ulps(w, ref[1].astype(np.float32)).max() <= 2.0, op
        T = w.shape[1]
        assert T <= 32
        assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= T * U24, op


@pytest.mark.parametrize("s", [2, 3, 4])
def test_up_reproduces_a_linear_ramp(s):
    n = 16
    taps = L.sr_taps("up", L.sr_defaults(s), n)
    a, b = 1.25, 0.5
    out = M.apply_1d(taps, a + b * np.arange(n), n)
    u = (np.arange(n * s) + 0.5) / s - 0.5
    inner = (taps[0] >= 0) & (taps[0] + 3 <= n - 1)                            # no clamped read
    assert inner.sum() >= (n - 3) * s
    assert np.abs(out - (a + b * u))[inner].max() <= 1e-5
    assert np.abs(out - (a + b * u))[~inner].max() > 1e-3                      # (the clamp does bend the border: the mask matters)


@pytest.mark.parametrize("s,kernel,sb", CASES)
def test_down_of_a_constant_is_that_constant(s, kernel, sb):
    n = 12 * s
    taps = L.sr_taps("down", L.sr_defaults(s, kernel=kernel, blur_sigma=sb), n)
    out = M.apply_1d(taps, np.full(n, 100.0), n)
    assert np.abs(out - 100.0).max() <= 100.0 * taps[1].shape[1] * U24


def test_rejected_parameters_return_1():
    lib = core.lib()
    T = C.c_uint(0)

    def rc(sr, op=L.SR_DOWN, n_in=24, t=T):
        return lib.lfbm5d_sr_taps(op, C.byref(sr), n_in, None, None, C.byref(t) if t is not None else None, 0)

    assert rc(L.sr_defaults(2)) == 0 and T.value == 8
    for bad in (dict(scale=1), dict(scale=5), dict(kernel=7), dict(kernel="gaussian", blur_sigma=0.0), dict(kernel="gaussian", blur_sigma=-1.0),
                dict(kernel="gaussian", blur_sigma=5.5), dict(kernel="gaussian", blur_sigma=float("nan"))):
        assert rc(L.sr_defaults(2, **bad)) == 1, bad
    assert rc(L.sr_defaults(2, blur_sigma=9.0)) == 0                           # the bicubic D ignores blur_sigma
    assert rc(L.sr_defaults(2), n_in=0) == 1
    assert rc(L.sr_defaults(3), n_in=25) == 1                                  # D needs a multiple of the scale
    assert rc(L.sr_defaults(3), op=L.SR_UP, n_in=25) == 0
    assert rc(L.sr_defaults(2), op=2) == 1
    assert rc(L.sr_defaults(2), t=None) == 1
    assert lib.lfbm5d_sr_taps(L.SR_DOWN, None, 24, None, None, C.byref(T), 0) == 1
    first, w = np.zeros(12, np.int32), np.zeros(12 * 8 - 1, np.float32)        # w one float short
    assert lib.lfbm5d_sr_taps(L.SR_DOWN, C.byref(L.sr_defaults(2)), 24, first.ctypes.data, w.ctypes.data, C.byref(T), w.size) == 1
    with pytest.raises(L.LfBm5dError):
        L.sr_taps("down", L.sr_defaults(2, scale=7), 24)


def test_defaults_fill_a_valid_struct():
    assert C.sizeof(core.SrParams) == 8 * 4
    for s in (2, 3, 4):
        sr = L.sr_defaults(s)
        assert sr.scale == s and sr.kernel == L.SR_BICUBIC and sr.iterations >= 1 and sr.close_projection == 1
        assert 0.0 < sr.sigma_end <= sr.sigma_start and 0.0 < sr.beta <= 2.0 and 0.0 < sr.blur_sigma <= 5.0
        sr.kernel = L.SR_GAUSSIAN                                              # the struct stays valid when the caller switches kernels
        L.sr_taps("down", sr, 8 * s)
    lib = core.lib()
    assert lib.lfbm5d_sr_defaults(5, C.byref(core.SrParams())) == 1
    assert lib.lfbm5d_sr_defaults(1, C.byref(core.SrParams())) == 1
    assert lib.lfbm5d_sr_defaults(2, None) == 1
