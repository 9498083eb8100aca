"""lfbm5d_corr_measure_* against the numpy model (tests/corr_model.py) bit for bit (run with -m gpu on an MI355X): autocorrelation,
sigma, counts and cut; device and host forms and repeated calls identical; the refusals."""
import numpy as np
import pytest
import torch

import corr_model as CM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def light_field(A, C, H, W, seed, taps_width=0.8, sigma=12.0):
    """A smooth ramp with texture in one corner plus correlated noise: scores differ from block to block."""
    from lfbm5d_amd import synth
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    clean = np.empty((A, C, H, W), np.float32)
    for a in range(A):
        for c in range(C):
            clean[a, c] = 60 + 2.0 * x + 1.0 * y + 10 * c + 40 * ((x > W // 2) & (y > H // 2)) * np.sin(0.9 * x + 0.4 * a)
    clean += (rng.random(clean.shape) * 0.25).astype(np.float32)
    return synth.add_correlated_noise(clean, sigma, CM.gaussian_taps(taps_width), seed=seed)


def same(est, model):
    assert est.blocks == model["blocks"] and est.selected == model["selected"], (est.blocks, est.selected, model["blocks"], model["selected"])
    assert np.float64(est.cut).tobytes() == np.float64(model["cut"]).tobytes(), (est.cut, model["cut"])
    assert np.float64(est.sigma).tobytes() == np.float64(model["sigma"]).tobytes(), (est.sigma, model["sigma"])
    assert est.acf.tobytes() == np.ascontiguousarray(model["acf"], np.float64).tobytes(), np.abs(est.acf - model["acf"]).max()


def both_forms(ctx, lf, mask, W, H, C, B, fraction):
    flat = np.ascontiguousarray(lf.reshape(lf.shape[0], -1))
    dev = ctx.corr_measure(torch.from_numpy(flat).cuda(), mask, W, H, C, block=B, fraction=fraction)
    again = ctx.corr_measure(torch.from_numpy(flat).cuda(), mask, W, H, C, block=B, fraction=fraction)
    host = ctx.corr_measure([None if not m else flat[i] for i, m in enumerate(mask)], mask, W, H, C, block=B, fraction=fraction)
    for other in (again, host):
        assert other.acf.tobytes() == dev.acf.tobytes() and (other.sigma, other.blocks, other.selected, other.cut) == (dev.sigma, dev.blocks, dev.selected, dev.cut)
    return dev


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("fraction", [1.0, 0.25])
def test_measure_is_the_model(ctx, B, fraction):
    """2 x 2 SAIs of 32 x 48 (W x H), three channels, one SAI empty."""
    W, H, C = 32, 48, 3
    lf = light_field(4, C, H, W, seed=3)
    mask = np.array([1, 1, 0, 1], np.uint32)
    lf[2] = np.nan                                        # an empty SAI is never read
    est = both_forms(ctx, lf, mask, W, H, C, B, fraction)
    model = CM.measure(lf, mask, B, fraction)
    assert est.block == B and est.blocks == 3 * C * (W // B) * (H // B)
    same(est, model)
    assert CM.check(est.acf) is None and est.sigma > 0
    if fraction == 1.0:
        assert est.selected == est.blocks
    else:
        assert est.selected == int(np.ceil(0.25 * est.blocks))     # (no ties in this light field)


@pytest.mark.parametrize("B", [8, 16, 32])
def test_one_block(ctx, B):
    """One SAI of exactly B x B, one channel: one block, whatever the fraction."""
    lf = light_field(1, 1, B, B, seed=10 + B)
    for fraction in (1.0, 0.01):
        est = both_forms(ctx, lf, [1], B, B, 1, B, fraction)
        same(est, CM.measure(lf, [1], B, fraction))
        assert est.blocks == est.selected == 1


def test_remainder_is_ignored_and_default_block(ctx):
    """W and H not divisible by the block: the remainder is ignored; block 0 is 16, fraction None the default 0.1; more than one chunk
    of 256 blocks, the last one short."""
    W, H, C = 16 * 9 + 7, 16 * 10 + 15, 3
    lf = light_field(1, C, H, W, seed=21)
    flat = torch.from_numpy(np.ascontiguousarray(lf.reshape(1, -1))).cuda()
    est = ctx.corr_measure(flat, [1], W, H, C, block=0)
    assert est.block == 16 and est.blocks == 3 * 90 and est.selected == 27
    same(est, CM.measure(lf, [1], 16, 0.1))
    lf2 = lf.copy()
    lf2[:, :, 16 * 10:, :] = 1e6                           # the remainder rows and columns take no part
    lf2[:, :, :, 16 * 9:] = -1e6
    est2 = ctx.corr_measure(torch.from_numpy(np.ascontiguousarray(lf2.reshape(1, -1))).cuda(), [1], W, H, C, block=16, fraction=0.1)
    assert est2.acf.tobytes() == est.acf.tobytes() and est2.sigma == est.sigma
    same(ctx.corr_measure(flat, [1], W, H, C, block=32, fraction=0.5), CM.measure(lf, [1], 32, 0.5))


def test_ties_at_the_cut(ctx):
    """A constant light field: every score is 0, the cut is 0, every block is selected whatever the fraction, the result is the white
    autocorrelation with sigma 0.  A light field of two kinds of identical blocks: the ties at the cut are all selected."""
    W, H, C = 32, 32, 1
    const = np.full((2, C, H, W), 37.5, np.float32)
    est = both_forms(ctx, const, [1, 1], W, H, C, 8, 0.25)
    same(est, CM.measure(const, [1, 1], 8, 0.25))
    assert est.selected == est.blocks == 32 and est.cut == 0 and est.sigma == 0 and np.array_equal(est.acf, CM.WHITE)
    y, x = np.mgrid[0:8, 0:8]
    tile_a = ((x + 2 * y) % 5).astype(np.float32)
    tile_b = 3 * tile_a
    lf = np.empty((1, 1, 32, 32), np.float32)
    for by in range(4):
        for bx in range(4):
            lf[0, 0, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = tile_a if (by + bx) % 2 else tile_b
    est = both_forms(ctx, lf, [1], 32, 32, 1, 8, 0.25)     # kth = 4, but all 8 blocks of the lower score tie
    same(est, CM.measure(lf, [1], 8, 0.25))
    assert est.blocks == 16 and est.selected == 8


def test_refusals(ctx):
    import lfbm5d_amd as L
    lf = torch.zeros(2 * 3 * 32 * 32, device="cuda")
    ok = dict(LF=lf, mask=[1, 1], W=32, H=32, C=3, block=16, fraction=0.5)
    for change, message in ((dict(block=12), "block must be 8, 16 or 32"), (dict(block=64), "block must be"), (dict(C=2), "chnls"),
                            (dict(W=15), "at least the block size"), (dict(H=8), "at least the block size"),
                            (dict(fraction=1.5), r"fraction must be in \(0, 1\]"), (dict(fraction=-0.1), "fraction must be"),
                            (dict(fraction=float("nan")), "fraction must be"), (dict(mask=[0, 0]), "no non-empty SAI")):
        a = dict(ok, **change)
        with pytest.raises(L.LfBm5dError, match=message):
            ctx.corr_measure(a["LF"], a["mask"], a["W"], a["H"], a["C"], block=a["block"], fraction=a["fraction"])
    bad = torch.zeros(2 * 3 * 32 * 32, device="cuda")
    bad[5] = float("inf")
    with pytest.raises(L.LfBm5dError, match="not finite"):
        ctx.corr_measure(bad, [1, 1], 32, 32, 3, block=16, fraction=0.5)
    with pytest.raises(L.LfBm5dError, match="NULL pointer for a non-empty SAI"):
        ctx.corr_measure([np.zeros(3 * 32 * 32, np.float32), None], [1, 1], 32, 32, 3)
    c2 = L.Context(0)
    try:
        c2.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            c2.corr_measure(lf, [1, 1], 32, 32, 3)
    finally:
        c2.close()
    # and the same call without a fault runs
    est = ctx.corr_measure(lf, [1, 1], 32, 32, 3, block=16, fraction=0.5)
    assert est.blocks == 2 * 3 * 4 and est.sigma == 0
