"""GPU tests of the clipped Poisson-Gaussian stage (lfbm5d_pgclip_*, lfbm5d_denoise_pgclip_*, include/lfbm5d_pgclip.h): k_curve_map
against the float32 numpy model bit for bit on every path it has, the estimate against the model, the job against its calls made by hand
and against the CPU composition (numpy maps around the oracle's two steps)."""
import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from oracle import oracle as O
import pgclip_model as M
import helpers as Hh

MASK = np.ones(9, np.uint32)
TAIL = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
SENTINEL = np.float32(12345.0)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t, np.float32)).view(np.uint32)


def _psnr(x, clean):
    return float(10.0 * np.log10(255.0 ** 2 / ((np.asarray(x, np.float64) - clean) ** 2).mean()))


def _params(sigma, pk):
    return core.make_params(sigma, 2.7, *pk)


def _ramp(lo, hi):
    r = (lo - 50.0 + np.arange(int((hi - lo + 100.0) * 64.0) + 1, dtype=np.float64) / 64.0).astype(np.float32)
    return np.concatenate([r, np.array([np.nan, np.inf, -np.inf], np.float32)])


def _through(ctx, fn, cv, values, W, H, C_, offset=False, in_place=False):
    """`values` through the map in light fields of 3 SAIs (the middle one empty, its planes filled with a sentinel) of C_ planes of
    W x H, as many calls as it takes; returns the mapped values.  offset: both buffers start one float past an allocation (4-byte
    aligned only)."""
    import torch
    mask = np.array([1, 0, 1], np.uint32)
    img = C_ * W * H
    out = np.empty_like(values)
    for at in range(0, values.size, 2 * img):
        part = values[at:at + 2 * img]
        lf = np.full((3, img), SENTINEL, np.float32)
        lf.reshape(-1)[np.r_[0:img, 2 * img:3 * img][:part.size]] = part
        lf.reshape(-1)[np.r_[0:img, 2 * img:3 * img][part.size:]] = part[-1] if np.isfinite(part[-1]) else 0.0
        if offset:
            a, b = torch.empty(3 * img + 1, device="cuda"), torch.full((3 * img + 1,), float(SENTINEL), device="cuda")
            d_in, d_out = a[1:].view(3, img), b[1:].view(3, img)
            d_in.copy_(torch.from_numpy(lf))
            assert d_in.data_ptr() % 16 == 4 and d_out.data_ptr() % 16 == 4
        else:
            d_in = _dev(lf)
            d_out = d_in if in_place else torch.full_like(d_in, float(SENTINEL))
        fn(cv, d_in, mask, d_out, W, H, C_)
        res = d_out.cpu().numpy()
        assert np.array_equal(res[1].view(np.uint32), lf[1].view(np.uint32)), "the empty SAI's planes were touched"
        if not in_place:
            assert np.array_equal(_bits(d_in), lf.view(np.uint32)), "the input was written"
        out[at:at + part.size] = res.reshape(-1)[np.r_[0:img, 2 * img:3 * img][:part.size]]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2.0, 25.0, 0.0, 255.0), (0.0, 625.0, 16.0, 235.0)])
def test_curve_map_equals_the_float32_model_bit_for_bit(ctx, case):
    a, b, lo, hi = case
    cv = L.pgclip_curves(*case)
    x = _ramp(lo, hi)
    for name, fn, inverse in (("forward", ctx.pgclip_forward, False), ("inverse", ctx.pgclip_inverse, True)):
        want = M.curve_map(x, cv.inv if inverse else cv.fwd, cv.inv_x0 if inverse else cv.fwd_x0, cv.inv_dx if inverse else cv.fwd_dx,
                           inverse)
        assert np.array_equal(want[-3:].view(np.uint32), x[-3:].view(np.uint32))          # NaN and the infinities pass through
        shapes = {"16x8x3, 16-byte path": (16, 8, 3, {}), "17x5x3, value by value": (17, 5, 3, {}), "16x8x1": (16, 8, 1, {}),
                  "17x5x1": (17, 5, 1, {}), "16x8x3, one float past alignment": (16, 8, 3, dict(offset=True)),
                  "16x8x3, in place": (16, 8, 3, dict(in_place=True)), "17x5x3, in place": (17, 5, 3, dict(in_place=True))}
        for label, (W, H, C_, kw) in shapes.items():
            got = _through(ctx, fn, cv, x, W, H, C_, **kw)
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (name, label, bad[:5], x[bad[:5]], got[bad[:5]], want[bad[:5]])
            if label.startswith("16x8x3, 16"):
                again = _through(ctx, fn, cv, x, W, H, C_)
                assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "two calls differ"
        fin = want[:-3]
        assert (np.diff(fin) >= 0).all(), name
        if inverse:
            assert fin.min() >= np.float32(lo) and fin.max() <= np.float32(hi)
            assert fin[0] == np.float32(lo) and fin[-1] == np.float32(hi)
        else:
            assert (np.diff(fin) > 0).all()                                              # the end segments extend the map


@pytest.mark.gpu
def test_map_host_form_and_refusals(ctx):
    import torch
    cv = L.pgclip_curves(1.0, 100.0)
    x = np.linspace(-20.0, 280.0, 2 * 3 * 64, dtype=np.float32).reshape(2, -1)
    d = _dev(x)
    out = torch.zeros_like(d)
    ctx.pgclip_forward(cv, d, [1, 1], out, 8, 8, 3)
    h = np.zeros_like(x)
    ctx.pgclip_forward(cv, x, [1, 1], h, 8, 8, 3)
    assert np.array_equal(h.view(np.uint32), _bits(out))
    assert np.array_equal(_bits(out), M.forward(x, cv._asdict()).view(np.uint32))
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_forward_device: .*chnls"):
        ctx.pgclip_forward(cv, d, [1, 1], out, 8, 8, 2)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_inverse_device: .*no non-empty SAI"):
        ctx.pgclip_inverse(cv, d, [0, 0], out, 8, 8, 3)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_forward_device: .*overlap"):
        ctx.pgclip_forward(cv, d.view(-1)[:192], [1], d.view(-1)[64:256], 8, 8, 3)
    bad = core.PgclipCurvesStruct()
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_forward_device: bad curves"):
        ctx.pgclip_forward(bad, d, [1, 1], out, 8, 8, 3)


def _noisy_crop(a, b):
    clean = np.ascontiguousarray(Hh.source_lf(64).astype(np.float32)).reshape(9, -1)
    return clean, synth.clip_round(synth.add_poisson_gaussian(clean, a, b, 1))


def _same_estimate(got, want, C_=3):
    close = lambda x, y: abs(x - y) <= 1e-9 * abs(y) or (np.isnan(x) and np.isnan(y))
    assert close(got.a, want["a"]) and close(got.b, want["b"]), (got, want["a"], want["b"])
    for c in range(C_):
        assert close(got.a_channel[c], want["a_channel"][c]) and close(got.b_channel[c], want["b_channel"][c]), c
    assert (got.levels, got.f_max, got.heavily_clipped, got.quantised, got.blocks, got.skipped) == \
        (want["levels"], want["f_max"], want["heavily_clipped"], want["quantised"], want["blocks"], want["skipped"])
    assert close(got.censored, want["censored"])


@pytest.mark.gpu
def test_estimate_matches_the_model(ctx):
    _, z = _noisy_crop(2.0, 25.0)
    d = _dev(z)
    for mask in (MASK, np.array([1, 1, 1, 1, 0, 1, 1, 1, 1], np.uint32)):
        want = M.estimate(z, mask, 64, 64, 3)
        got = ctx.pgclip_estimate(d, mask, 64, 64, 3)
        _same_estimate(got, want)
        assert (got.lo, got.hi) == (0.0, 255.0)
        _same_estimate(L.pgclip_estimate(z, mask, 64, 64, 3, ctx=ctx), want)              # host form
        hist, sm, cens, whole, _, _ = ctx.clip_histogram(d, mask, 64, 64, 3)             # the counts are the clipped stage's
        f = L.pgclip_fit(hist, sm, cens, whole)
        assert (f.a, f.b, f.levels) == (got.a, got.b, got.levels)
    print(f"(2, 25) on the 64 x 64 crop: a = {got.a:.4f}, b = {got.b:.4f} ({got.levels} levels, f_max {got.f_max})")
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_estimate_device: fewer than 4"):
        ctx.pgclip_estimate(_dev(np.zeros((9, 3 * 64 * 64), np.float32)), MASK, 64, 64, 3)


@pytest.fixture(scope="module")
def job_inputs():
    """(clean, clipped noisy) of the 3 x 3 x 64 x 64 golden crop under (1, 100), and the CPU composition of the job with the model
    given: numpy forward map, the oracle's two steps at sigma = (float)s, numpy inverse map."""
    clean, z = _noisy_crop(1.0, 100.0)
    cv = L.pgclip_curves(1.0, 100.0)
    s = float(np.float32(cv.s))
    t = M.forward(z, cv._asdict())
    n1, bs, _ = O.run_step1(O.make_params(s, 2.7, *Hh.README_HT), t.copy(), MASK, O.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    _, _, dn, _ = O.run_step2(O.make_params(s, 2.7, *Hh.README_WIEN), n1.copy(), bs.copy(), MASK, O.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    return clean, z, cv, M.inverse(dn, cv._asdict())


def _by_hand(ctx, cv, z):
    import torch
    d = _dev(z)
    t, b2, p2 = torch.zeros_like(d), torch.zeros_like(d), torch.zeros_like(d)
    ctx.pgclip_forward(cv, d, MASK, t, 64, 64, 3)
    ctx.denoise(_params(cv.s, Hh.README_HT), _params(cv.s, Hh.README_WIEN), t, MASK, b2, p2, *TAIL)
    ctx.pgclip_inverse(cv, b2, MASK, b2, 64, 64, 3)
    ctx.pgclip_inverse(cv, p2, MASK, p2, 64, 64, 3)
    return b2, p2


@pytest.mark.gpu
def test_job_with_a_given_model(ctx, job_inputs):
    """Measured on an MI355X (profiles/pgclip.txt has the table)."""
    import torch
    clean, z, cv, composition = job_inputs
    d = _dev(z)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    est, s = ctx.denoise_pgclip((1.0, 100.0), _params(1.0, Hh.README_HT), _params(99.0, Hh.README_WIEN), d, MASK, basic, den, *TAIL)
    assert (est.a, est.b, est.lo, est.hi) == (1.0, 100.0, 0.0, 255.0) and s == cv.s      # the model used is returned
    assert np.array_equal(_bits(d), z.view(np.uint32))                                   # the noisy light field is only read
    b2, p2 = _by_hand(ctx, cv, z)
    assert np.array_equal(_bits(basic), _bits(b2)) and np.array_equal(_bits(den), _bits(p2))
    g = den.cpu().numpy()
    assert g.min() >= 0.0 and g.max() <= 255.0
    p_gpu, p_cpu = _psnr(g, clean), _psnr(composition, clean)
    print(f"(1, 100) on the crop: noisy {_psnr(z, clean):.3f} dB, denoise_pgclip {p_gpu:.3f} dB, CPU composition {p_cpu:.3f} dB")
    assert abs(p_gpu - p_cpu) <= 0.02                        # the bound of test_gpu_denoise_clipped.py between job and composition
    assert _psnr(basic.cpu().numpy(), clean) > _psnr(z, clean) + 3.0
    # host forms: flat arrays, one array per SAI
    hb, hd = np.zeros_like(z), np.zeros_like(z)
    zh = z.copy()
    L.denoise_pgclip((1.0, 100.0), _params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN), zh, MASK, hb, hd, *TAIL, ctx=ctx)
    assert np.array_equal(hb.view(np.uint32), _bits(basic)) and np.array_equal(hd.view(np.uint32), _bits(den)) and np.array_equal(zh, z)
    lb, ld = ([np.zeros(z.shape[1], np.float32) for _ in range(9)] for _ in range(2))
    ctx.denoise_pgclip((1.0, 100.0), _params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN), [z[i].copy() for i in range(9)], MASK, lb, ld,
                       *TAIL)
    assert np.array_equal(np.stack(ld).view(np.uint32), _bits(den))


@pytest.mark.gpu
def test_job_estimates_the_model_when_none_is_given(ctx, job_inputs):
    import torch
    clean, z, _, _ = job_inputs
    d = _dev(z)
    e = ctx.pgclip_estimate(d, MASK, 64, 64, 3)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    est, s = ctx.denoise_pgclip(None, _params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN), d, MASK, basic, den, *TAIL)
    assert est == e                                                                     # the model used is the estimate, returned
    cv = L.pgclip_curves(e.a, e.b)
    assert s == cv.s
    b2, p2 = _by_hand(ctx, cv, z)
    assert np.array_equal(_bits(basic), _bits(b2)) and np.array_equal(_bits(den), _bits(p2))
    print(f"model estimated: a = {e.a:.4f}, b = {e.b:.4f}, s = {s:.4f}, denoise_pgclip {_psnr(den.cpu().numpy(), clean):.3f} dB")


@pytest.mark.gpu
def test_job_refusals(ctx, job_inputs):
    import torch
    _, z, _, _ = job_inputs
    d = _dev(z)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    p = (_params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN))
    with pytest.raises(L.LfBm5dError, match="lfbm5d_denoise_pgclip_device: .*accepted domain.*denoise_pg"):
        ctx.denoise_pgclip((8.0, 0.0), *p, d, MASK, basic, den, *TAIL)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_denoise_pgclip_device: bad model"):
        ctx.denoise_pgclip((-1.0, 5.0), *p, d, MASK, basic, den, *TAIL)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_denoise_pgclip_device: the range"):
        ctx.denoise_pgclip(None, *p, d, MASK, basic, den, *TAIL, lo=255.0, hi=0.0)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.denoise_pgclip((1.0, 100.0), *p, d, MASK, basic, den, *TAIL[:-1], 2)
    assert float(basic.abs().max()) == 0.0 and float(den.abs().max()) == 0.0


@pytest.mark.gpu
def test_job_beats_the_unclipped_alternatives_on_the_dark_tile(ctx):
    """Rows 192..255, columns 128..191 of the golden light field under (1, 100), rounded and clipped: what a user had before this stage
    is denoise at the RMS sigma or denoise_pg with its own estimate on the clipped data.  The CPU composition (tools/pgclip_time.py cpu)
    gains 0.44 dB over the better of the two there (35.775 against 35.338 and 35.308 dB), so the job must beat both."""
    import torch
    clean = np.ascontiguousarray(Hh.source_lf()[:, :, 192:256, 128:192].astype(np.float32)).reshape(9, -1)
    z = synth.clip_round(synth.add_poisson_gaussian(clean, 1.0, 100.0, 1))
    d = _dev(z)
    basic, den = torch.zeros_like(d), torch.zeros_like(d)
    rms = float(np.sqrt((1.0 * clean + 100.0).mean()))
    ctx.denoise(_params(rms, Hh.README_HT), _params(rms, Hh.README_WIEN), d.clone(), MASK, basic, den, *TAIL)
    p_plain = _psnr(den.cpu().numpy(), clean)
    ctx.denoise_pg(None, _params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN), d.clone(), MASK, basic, den, *TAIL)
    p_pg = _psnr(den.cpu().numpy(), clean)
    ctx.denoise_pgclip((1.0, 100.0), _params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN), d, MASK, basic, den, *TAIL)
    p_given = _psnr(den.cpu().numpy(), clean)
    ctx.denoise_pgclip(None, _params(1.0, Hh.README_HT), _params(1.0, Hh.README_WIEN), d, MASK, basic, den, *TAIL)
    p_est = _psnr(den.cpu().numpy(), clean)
    print(f"dark tile, (1, 100): denoise at the RMS sigma {p_plain:.3f} dB, denoise_pg {p_pg:.3f} dB, denoise_pgclip {p_given:.3f} dB "
          f"(model estimated: {p_est:.3f} dB)")
    assert p_given > max(p_plain, p_pg)
    assert p_est > max(p_plain, p_pg)
