"""GPU tests of the clipped statistics (lfbm5d_clip_histogram_device, include/lfbm5d.h) against the numpy model (tests/clip_model.py):
integer equality of every count on both load paths, with non-finite values and on another range; equality with the Poisson-Gaussian
statistics at the default range; repeated calls; the host form of the estimate."""
import os

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import synth
import clip_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _lf(ang, C_, H, W, sigma=40.0, lo=0.0, hi=255.0, masked=None, rounded=True):
    """A crop of the golden light field (dark and bright regions) under noise of `sigma`, rounded and clipped to lo..hi."""
    y0, x0 = min(150, 256 - H), min(100, 256 - W)
    u8 = np.load(GOLDEN)[:ang * ang, :C_, y0:y0 + H, x0:x0 + W]
    A = ang * ang
    lf = synth.add_noise_mt19937(np.ascontiguousarray(u8, np.float32).reshape(A, -1), sigma, seed=3)
    lf = synth.clip_round(lf, lo, hi) if rounded else np.clip(lf, np.float32(lo), np.float32(hi))
    mask = np.ones(A, np.uint32)
    if masked is not None:
        mask[masked] = 0
        lf[masked] = -1e30          # never read
    return lf, mask


def _key(e):
    """A ClipNoiseLevel as a tuple that compares bit for bit (NaN equals NaN)."""
    return tuple(float(v).hex() if isinstance(v, float) else v for v in (e.sigma, *e.sigma_channel, *e[2:]))


def _assert_stats(ctx, lf, mask, W, H, C_, lo=0.0, hi=255.0, d=None):
    got = ctx.clip_histogram(_dev(lf) if d is None else d, mask, W, H, C_, lo, hi)
    want = M.histogram(lf, mask, W, H, C_, lo, hi)
    assert got[4:] == want[4:]                                    # blocks, skipped
    for g, w, name in zip(got[:4], want[:4], ("hist", "sum", "cens", "whole")):
        assert g.dtype == np.uint64 and np.array_equal(g, w), name
    assert int(got[0].sum()) == got[4] - got[5]
    assert (got[2] <= got[0].sum(axis=2)).all()                   # censored blocks are among the level's blocks
    return got


# odd W: scalar loads (the second case has one block row and column left over too); even W and an aligned buffer: 8-byte loads
@pytest.mark.gpu
@pytest.mark.parametrize("ang,C_,H,W,masked", [(3, 3, 35, 37, 4), (2, 1, 64, 64, None), (3, 3, 34, 66, 0), (2, 3, 130, 128, None)])
def test_counts_equal_the_model(ctx, ang, C_, H, W, masked):
    lf, mask = _lf(ang, C_, H, W, masked=masked)
    hist, sm, cens, whole, blocks, skipped = _assert_stats(ctx, lf, mask, W, H, C_)
    assert skipped == 0 and int(whole.sum()) == blocks            # rounded data: every block is whole
    assert 0 < int(cens.sum()) < blocks                           # and some, not all, hold a 0 or a 255
    lf, mask = _lf(ang, C_, H, W, masked=masked, rounded=False)   # clipped but not rounded: few whole blocks
    _, _, cens2, whole2, _, _ = _assert_stats(ctx, lf, mask, W, H, C_)
    assert int(whole2.sum()) < blocks // 4 and int(cens2.sum()) > 0


@pytest.mark.gpu
def test_counts_on_a_buffer_that_is_not_8_byte_aligned(ctx):
    import torch
    lf, mask = _lf(2, 3, 40, 66)
    buf = torch.zeros(lf.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(lf.reshape(-1)).cuda()
    d = buf[1:].view(4, -1)
    assert d.data_ptr() % 8 == 4 and d.is_contiguous()
    _assert_stats(ctx, lf, mask, 66, 40, 3, d=d)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [52, 53])
def test_counts_skip_non_finite_blocks(ctx, W):
    H = 40
    lf, mask = _lf(3, 3, H, W)
    x = lf.reshape(9, 3, H, W)
    x[2, 1, 7, 9] = np.nan
    x[2, 1, 20, 30] = np.inf
    x[4, 0, 11, 3] = -np.inf
    x[5, 2, 39, 51] = np.nan                    # W = 52: the last block; W = 53: as well (the last column is left over)
    x[6, 0, 3, 3] = 1e38                        # finite, but (p - lo) s sums to inf: skipped like the others
    x[6, 0, 3, 2] = 3e38
    x[0, 0, :6] = -40.0 + x[0, 0, :6] / 16      # below the range: level 0, censored, not whole
    x[0, 0, 6:12] = 300.0 + x[0, 0, 6:12] / 16  # above: level 63
    got = _assert_stats(ctx, lf, mask, W, H, 3)
    assert got[5] == 5
    assert got[2][0, 0] >= 3 * 26 and got[2][0, 63] >= 3 * 26
    assert int(got[3].sum()) < got[4] - got[5]


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(16.0, 235.0), (0.0, 1023.0), (-0.5, 0.5)])
def test_counts_on_another_range(ctx, lo, hi):
    H, W = 44, 50
    lf, mask = _lf(3, 3, H, W, masked=8)
    lf = lf * np.float32((hi - lo) / 255.0) + np.float32(lo)      # the 0..255 data moved onto lo..hi: not whole any more ...
    if hi - lo > 100:
        lf = synth.clip_round(lf, lo, hi)                         # ... unless rounded there
    got = _assert_stats(ctx, lf, mask, W, H, 3, lo, hi)
    assert int(got[2].sum()) > 0
    # the levels fill as they do at 0..255: the rescaling is applied
    assert got[0].sum(axis=(0, 2))[8:56].min() > 0


@pytest.mark.gpu
def test_default_range_equals_the_poisson_gaussian_statistics_and_repeats(ctx):
    for ang, C_, H, W in ((3, 3, 35, 37), (2, 1, 64, 64)):
        lf, mask = _lf(ang, C_, H, W)
        d = _dev(lf)
        a = ctx.clip_histogram(d, mask, W, H, C_)
        b = ctx.clip_histogram(d, mask, W, H, C_)
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y)
        assert a[4:] == b[4:]
        hist, sm, blocks, skipped = ctx.pg_histogram(d, mask, W, H, C_)
        assert np.array_equal(hist, a[0]) and np.array_equal(sm, a[1]) and (blocks, skipped) == a[4:]
        assert np.array_equal(d.cpu().numpy().view(np.uint32), lf.view(np.uint32))      # read only


@pytest.mark.gpu
def test_estimate_host_forms_equal_the_device_form(ctx):
    H = W = 128
    lf, mask = _lf(3, 3, H, W, masked=4)
    d = _dev(lf)
    e1 = ctx.noise_level_clipped(d, mask, W, H, 3)
    k1 = _key(e1)
    assert k1 == _key(ctx.noise_level_clipped(d, mask, W, H, 3))
    assert k1 == _key(ctx.noise_level_clipped(lf, mask, W, H, 3))                                                    # host form, flat array
    assert k1 == _key(ctx.noise_level_clipped([lf[i].copy() if mask[i] else None for i in range(9)], mask, W, H, 3))   # one array per SAI
    assert k1 == _key(L.noise_level_clipped(d, mask, W, H, 3, ctx=ctx))
    hist, sm, cens, whole, blocks, skipped = ctx.clip_histogram(d, mask, W, H, 3)
    f = L.clip_fit(hist, sm, cens, whole)
    assert k1 == _key(f._replace(blocks=blocks, skipped=skipped)) and e1.blocks == 8 * 3 * 64 * 64
    r = M.estimate(lf, mask, W, H, 3)
    assert abs(e1.sigma - r["sigma"]) <= 1e-9 * r["sigma"] and (e1.levels, e1.f_max) == (r["levels"], r["f_max"])
    assert abs(e1.sigma / 40.0 - 1.0) < 0.1 and e1.quantised
