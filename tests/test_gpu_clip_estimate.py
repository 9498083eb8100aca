"""GPU tests of the clipping-aware noise level (lfbm5d_noise_level_clipped_*, include/lfbm5d.h) on the whole golden light field: the
accuracy cases of tests/test_clip.py through the library, and equality with the numpy model (tests/clip_model.py)."""
import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import synth
import clip_model as M
from helpers import noisy_lf, source_lf

MASK = np.ones(9, np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _both(ctx, lf):
    e = ctx.noise_level_clipped(_dev(lf), MASK, 256, 256, 3)
    r = M.estimate(lf, MASK, 256, 256, 3)
    assert abs(e.sigma - r["sigma"]) <= 1e-9 * r["sigma"]
    for c in range(3):
        assert abs(e.sigma_channel[c] - r["sigma_channel"][c]) <= 1e-9 * r["sigma_channel"][c]
    assert (e.levels, e.f_max, e.heavily_clipped, e.quantised, e.blocks, e.skipped) == \
        (r["levels"], r["f_max"], r["heavily_clipped"], r["quantised"], r["blocks"], r["skipped"])
    assert abs(e.censored - r["censored"]) <= 1e-12
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [10.0, 25.0, 50.0])
def test_estimate_on_the_clipped_golden_light_field(ctx, sigma):
    """Noise of helpers.noisy_lf (MT19937 seed 1), then rint and clip.  Measured on an MI355X (profiles/clip.txt): 10.263, 25.202,
    50.285; the blind estimate on the same input 24.111 at 25 and 45.102 at 50."""
    _, noisy = noisy_lf(source_lf(), sigma)
    lf = synth.clip_round(noisy)
    e = _both(ctx, lf)
    print(f"sigma = {sigma}: clipping-aware {e.sigma:.3f} ({e.levels} levels, f_max = {e.f_max}, censored blocks {100 * e.censored:.1f} %)")
    assert abs(e.sigma / sigma - 1.0) <= 0.03 and not e.heavily_clipped and e.quantised
    if sigma >= 25.0:
        blind = ctx.noise_level(_dev(lf), MASK, 256, 256, 3).sigma
        print(f"sigma = {sigma}: blind estimate on the same input {blind:.3f}")
        assert abs(e.sigma - sigma) <= 0.5 * abs(blind - sigma)


@pytest.mark.gpu
def test_estimate_under_heavy_clipping_and_on_float_noise(ctx):
    _, noisy = noisy_lf(source_lf(), 75.0)
    e = _both(ctx, synth.clip_round(noisy))
    print(f"sigma = 75: clipping-aware {e.sigma:.3f} ({e.levels} levels, f_max = {e.f_max})")
    assert np.isfinite(e.sigma) and e.heavily_clipped and e.f_max > 0.1
    _, noisy = noisy_lf(source_lf(), 25.0)
    e = _both(ctx, noisy)
    print(f"sigma = 25, float noise: {e.sigma:.3f}")
    assert abs(e.sigma / 25.0 - 1.0) <= 0.03 and not e.quantised and not e.heavily_clipped


@pytest.mark.gpu
def test_estimate_fails_on_a_light_field_without_four_levels(ctx):
    lf = np.full((9, 3 * 64 * 64), 100.0, np.float32) + synth.add_noise_mt19937(np.zeros((9, 3 * 64 * 64), np.float32), 2.0, seed=2)
    with pytest.raises(L.LfBm5dError, match="fewer than 4 intensity levels"):
        ctx.noise_level_clipped(_dev(lf), MASK, 64, 64, 3)
    assert M.estimate(lf, MASK, 64, 64, 3) is None
