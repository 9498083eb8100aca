"""GPU tests of the declipping kernel (lfbm5d_declip_*, include/lfbm5d.h) against the float64 model (tests/clip_model.py): a ramp from
lo - 50 to hi + 50 in steps of 1/64 over sigma x range, on a shape that takes the scalar path and on one that takes the 16-byte path."""
import numpy as np
import pytest

import lfbm5d_amd as L
import clip_model as M

# |GPU - model| in grey levels: an error of 1e-3 at 40 dB moves the PSNR by < 0.004 dB, under the project's 0.01 dB
TOL = 1e-3
SHAPES = [(33, 31), (32, 32)]            # plane of 1023 values: scalar loads and stores; 1024 values, aligned: 16-byte ones
MASK = np.array([1, 0, 1], np.uint32)    # 2 SAIs x 3 channels, and an empty one between them


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


def _ramp(lo, hi):
    n = int((hi - lo + 100.0) * 64.0) + 1
    return (lo - 50.0 + np.arange(n) / 64.0).astype(np.float32)


def _through(ctx, ramp, sigma, lo, hi, H, W):
    """The ramp through the kernel, a light field's worth (the two non-empty SAIs) at a time; the empty SAI's plane holds -7."""
    import torch
    per = 3 * H * W
    out = np.empty_like(ramp)
    for i in range(0, ramp.size, 2 * per):
        piece = np.full(2 * per, ramp[-1], np.float32)
        n = min(2 * per, ramp.size - i)
        piece[:n] = ramp[i:i + n]
        lf = np.full((3, per), -7.0, np.float32)
        lf[0], lf[2] = piece[:per], piece[per:]
        d = _dev(lf)
        o = torch.full_like(d, -9.0)
        ctx.declip(sigma, d, MASK, o, W, H, 3, lo, hi)
        g = o.cpu().numpy()
        assert (g[1] == -9.0).all()                                        # the plane of the empty SAI is not written
        assert np.array_equal(_bits(d), lf.view(np.uint32))                # the input is only read
        out[i:i + n] = np.concatenate([g[0], g[2]])[:n]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("lo,hi", [(0.0, 255.0), (16.0, 235.0)])
@pytest.mark.parametrize("sigma", [1.0, 5.0, 25.0, 50.0, 100.0])
def test_ramp_against_the_model(ctx, sigma, lo, hi, H, W):
    ramp = _ramp(lo, hi)
    assert ramp[0] == lo - 50.0 and ramp[-1] == hi + 50.0
    got = _through(ctx, ramp, sigma, lo, hi, H, W)
    want = M.declip(ramp.astype(np.float64), sigma, lo, hi)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"sigma = {sigma}, range {lo}..{hi}, {H} x {W}: max |GPU - model| = {err:.3g}")
    assert err <= TOL
    assert (np.diff(got) >= 0).all()                                       # non-decreasing
    assert got[0] == lo and got[-1] == hi and got.min() == lo and got.max() == hi
    e_lo = float(M.clipped_mean(lo, sigma, lo, hi))
    assert (got[ramp <= e_lo] == lo).all() and (got[ramp > e_lo + 0.1] > lo).all()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_non_finite_values_in_place_repeats_and_host_forms(ctx, H, W):
    import torch
    sigma, per = 25.0, 3 * H * W
    rng = np.random.default_rng(H)
    lf = rng.uniform(-30.0, 290.0, (3, per)).astype(np.float32)
    lf[0, :6] = [np.nan, np.inf, -np.inf, 0.0, 255.0, -0.0]
    lf[2, -3:] = [np.nan, 1e30, -1e30]                                      # the last values of the last plane
    lf[1] = np.nan                                                          # the empty SAI: never read
    d = _dev(lf)
    out = torch.full_like(d, -9.0)
    ctx.declip(sigma, d, MASK, out, W, H, 3)
    g = out.cpu().numpy()
    assert np.isnan(g[0, 0]) and g[0, 1] == np.inf and g[0, 2] == -np.inf and np.isnan(g[2, -3])
    assert np.array_equal(g[0, :3].view(np.uint32), lf[0, :3].view(np.uint32))    # passed through bit for bit
    assert g[0, 3] == 0.0 and g[0, 4] == 255.0 and g[2, -2] == 255.0 and g[2, -1] == 0.0
    live = np.array([0, 2])
    fin = np.isfinite(lf[live])
    assert np.abs(g[live][fin].astype(np.float64) - M.declip(lf[live][fin].astype(np.float64), sigma)).max() <= TOL
    assert (g[1] == -9.0).all()
    # repeated calls give the same bits; in place equals out of place
    out2 = torch.full_like(d, -9.0)
    ctx.declip(sigma, d, MASK, out2, W, H, 3)
    assert np.array_equal(_bits(out), _bits(out2))
    d2 = d.clone()
    ctx.declip(sigma, d2, MASK, d2, W, H, 3)
    assert np.array_equal(_bits(d2)[live], _bits(out)[live]) and np.array_equal(_bits(d2)[1], lf[1].view(np.uint32))
    # host forms: flat array, one array per SAI (None for the empty one), in place
    h = np.full_like(lf, -9.0)
    ctx.declip(sigma, lf.copy(), MASK, h, W, H, 3)
    assert np.array_equal(h.view(np.uint32), _bits(out))
    hl = [np.zeros(per, np.float32), None, np.zeros(per, np.float32)]
    ctx.declip(sigma, [lf[0].copy(), None, lf[2].copy()], MASK, hl, W, H, 3)
    assert np.array_equal(hl[0].view(np.uint32), _bits(out)[0]) and np.array_equal(hl[2].view(np.uint32), _bits(out)[2])
    hi_ = lf.copy()
    ctx.declip(sigma, hi_, MASK, hi_, W, H, 3)
    assert np.array_equal(hi_.view(np.uint32)[live], _bits(out)[live])


@pytest.mark.gpu
def test_unaligned_buffers_take_the_scalar_path(ctx):
    """A 16-byte-aligned shape on buffers that start 4 bytes past such an address."""
    import torch
    H = W = 32
    per = 3 * H * W
    lf = np.random.default_rng(5).uniform(-30.0, 290.0, (3, per)).astype(np.float32)
    want = torch.zeros(3, per, device="cuda")
    ctx.declip(25.0, _dev(lf), MASK, want, W, H, 3)
    buf = torch.zeros(3 * per + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(lf.reshape(-1)).cuda()
    d = buf[1:].view(3, per)
    assert d.data_ptr() % 16 == 4
    ctx.declip(25.0, d, MASK, d, W, H, 3)
    live = np.array([0, 2])
    assert np.array_equal(_bits(d)[live], _bits(want)[live])
    assert float(buf[0]) == 0.0
