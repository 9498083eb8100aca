"""GPU tests of the defect inpainting (lfbm5d_inpaint_*, include/lfbm5d.h): the fill and the projection equal the numpy model
(tests/inpaint_model.py) bit for bit at every tile edge, in narrow planes and across launches; the loop against the same public calls made
by hand (bits) and against the CPU composition of the model with the checker's run_step1 (PSNR); what the refinement is worth in front of
the denoiser; the host forms, the C++ drop-in, rejected calls and the CLIs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from oracle import oracle as O
import inpaint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
OUT_SENTINEL, FLAG_SENTINEL = -7.0, 9
R = core.INPAINT_PASSES_PER_LAUNCH
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")       # N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D: the super-resolution tests' parameters
WIEN = (16, 8, 3, 8, 3, "dct", "sadct", "haar")
TAIL = (L.ROWMAJOR, 3, 3, 1, 64, 64, 3)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(A, C_, H, W, masked=None, seed=0):
    """Uniform values, a defect map of rectangles (sides up to 7, and up to half the plane) and single values, and non-finite values the map names and does not."""
    rng = np.random.default_rng(seed)
    lf = rng.uniform(0.0, 255.0, (A, C_, H, W)).astype(np.float32)
    fl = rng.random((A, C_, H, W)) < 0.02
    for st in range(A):
        for c in range(C_):
            for _ in range(3):
                h, w = rng.integers(1, min(7, max(1, H // 2)) + 1), rng.integers(1, min(7, max(1, W // 2)) + 1)
                i, j = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
                fl[st, c, i:i + h, j:j + w] = True
    if H * W > 8:
        fl[0, 0, 1, 1] = True
        lf[0, 0, 1, 1] = np.nan                      # named by the map
        fl[0, 0, H - 1, W - 2] = False
        lf[0, 0, H - 1, W - 2] = np.nan              # not named
        fl[A - 1, C_ - 1, 0, W - 1] = False
        lf[A - 1, C_ - 1, 0, W - 1] = np.inf
        fl[A - 1, C_ - 1, H - 2, 0] = True
        lf[A - 1, C_ - 1, H - 2, 0] = -np.inf
    else:                                            # 2 x 2: one value named, one not finite, two sound ones per plane
        fl[:] = False
        fl[:, :, 0, 1] = True
        lf[-1, :, 1, 0] = np.nan
    mask = np.ones(A, np.uint32)
    if masked is not None:
        mask[masked] = 0
        lf[masked] = np.nan                          # never read
    return lf.reshape(A, -1), (fl.reshape(A, -1) * 3).astype(np.uint8), mask


def _assert_fill_equals_model(ctx, lf, fl, mask, W, H, C_):
    """One fill against the model: values, codes, counts and the pass count, with sentinels in what must not be written."""
    out0 = np.full(lf.shape, OUT_SENTINEL, np.float32)
    code0 = np.full(lf.shape, FLAG_SENTINEL, np.uint8)
    want = M.fill(lf, fl, mask, W, H, C_, out=out0, codes=code0)
    d, df = _dev(lf), _dev(fl)
    out, codes = _dev(out0), _dev(code0)
    got = ctx.inpaint_fill(d, df, mask, W, H, C_, out=out, flags_out=codes)
    assert np.array_equal(_bits(d), lf.view(np.uint32)) and np.array_equal(df.cpu().numpy(), fl)   # the inputs are only read
    assert np.array_equal(codes.cpu().numpy(), want["flags"])
    assert np.array_equal(_bits(out), want["out"].view(np.uint32))
    for name in ("flagged", "filled", "left"):
        assert list(getattr(got, name)) == list(want[name]), name
    assert (got.pixels, got.passes) == (want["pixels"], want["passes"])
    assert got.launches >= max(1, -(-want["passes"] // R))
    assert got.out is out and got.flags is codes
    again = ctx.inpaint_fill(d, df, mask, W, H, C_, return_flags=True)                         # the same bits on a second call
    live = mask != 0
    assert np.array_equal(_bits(again.out)[live], _bits(out)[live]) and np.array_equal(again.flags.cpu().numpy()[live], want["flags"][live])
    assert again[2:7] == got[2:7]
    return got, want


# tiles are 64 x 32 with a halo of 8: widths on both sides of a tile edge, several tiles, the smallest plane, a plane narrower than the
# halo, an empty SAI
@pytest.mark.gpu
@pytest.mark.parametrize("A,C_,H,W,masked", [(9, 3, 37, 70, 4), (2, 1, 2, 2, None), (1, 1, 5, 3, None), (4, 1, 65, 63, None),
                                             (4, 1, 65, 64, None), (4, 1, 65, 65, None), (4, 1, 65, 257, None)])
def test_fill_equals_the_model(ctx, A, C_, H, W, masked):
    lf, fl, mask = _case(A, C_, H, W, masked, seed=H * 1000 + W)
    got, want = _assert_fill_equals_model(ctx, lf, fl, mask, W, H, C_)
    print(f"{A} x {C_} x {H} x {W}: flagged {got.flagged}, left {got.left}, {got.passes} passes, {got.launches} launches")
    assert sum(got.flagged) > int((fl[mask != 0] != 0).sum()) - 1 and sum(got.left) == 0 and got.passes >= 1
    assert np.isfinite(got.out.cpu().numpy()[mask != 0]).all()
    if masked is not None:                                                     # empty SAI: out and codes keep their sentinels
        assert (got.out[masked] == OUT_SENTINEL).all() and (got.flags[masked] == FLAG_SENTINEL).all()


def _planted():
    """One 70 x 140 plane (3 x 3 tiles of 64 x 32) with regions where the code can go wrong; returns (plane, boolean map)."""
    H, W = 70, 140
    I = np.random.default_rng(11).uniform(0.0, 255.0, (H, W)).astype(np.float32)
    f = np.zeros((H, W), bool)
    for y in (32, 64):                                                         # across every tile corner and edge
        for x in (64, 128):
            f[y - 2:y + 3, x - 2:x + 3] = True                                 # 5 x 5 on a corner
        f[y - 1:y + 2, 20:25] = True                                           # across a tile row edge
        f[y, 40] = f[y - 1, 44] = True                                         # single values on both sides of it
    for x in (64, 128):
        f[10:15, x - 1:x + 2] = True                                           # across a tile column edge
        f[50, x] = f[52, x - 1] = True
    f[0:3, 0:3] = f[0:4, W - 3:W] = f[H - 3:H, 0:2] = f[H - 2:H, W - 4:W] = True   # the image corners
    f[0:2, 30:36] = f[H - 2:H, 90:96] = f[20:26, 0:2] = f[40:46, W - 2:W] = True   # the image edges
    s = 2 * R + 3
    f[36:36 + s, 76:76 + s] = True                                             # depth R + 2: a second launch
    f[:, 110:112] = True                                                       # a full-height column pair
    I[5, 100] = np.nan; f[5, 100] = True                                       # non-finite values the map names ...
    I[6, 104] = np.inf; f[6, 104] = True
    I[18, 100] = np.nan                                                        # ... and does not
    I[18, 104] = -np.inf
    I[60, 5:8] = np.nan                                                        # a run of them, at a tile row edge
    return I, f


@pytest.mark.gpu
def test_planted_regions(ctx):
    I, f = _planted()
    H, W = I.shape
    J = np.random.default_rng(12).uniform(0.0, 255.0, (H, W)).astype(np.float32)
    lf = np.stack([I.reshape(-1), I[::-1, ::-1].reshape(-1), J.reshape(-1)])   # the plane, the plane turned round, a fully flagged plane
    fl = np.stack([f.reshape(-1), f[::-1, ::-1].reshape(-1), np.ones(H * W, bool)]).astype(np.uint8)
    mask = np.ones(3, np.uint32)
    got, want = _assert_fill_equals_model(ctx, lf, fl, mask, W, H, 1)
    print(f"planted: flagged {got.flagged}, left {got.left}, {got.passes} passes, {got.launches} launches")
    assert got.passes == R + 2 == M.chebyshev_depth(f | ~np.isfinite(I)) and got.launches >= 2
    codes = got.flags.cpu().numpy().reshape(3, H, W)
    out = got.out.cpu().numpy().reshape(3, H, W)
    named = f | ~np.isfinite(I)
    assert np.array_equal(codes[0] == 1, named) and np.array_equal(codes[1] == 1, named[::-1, ::-1])
    assert (codes[2] == 2).all() and np.array_equal(out[2].view(np.uint32), J.view(np.uint32))   # left as it is
    assert got.left == (H * W,) and got.filled == (2 * int(named.sum()),)
    assert np.isfinite(out).all()
    # the fill alone through the loop's entry point (K = 0) is the same call; K >= 1 refuses the plane that is left
    P = core.make_params(0.0, 2.7, *HT)
    z = ctx.inpaint(_dev(lf), _dev(fl), mask, P, L.ROWMAJOR, 3, 1, 1, W, H, 1, iterations=0, return_flags=True)
    assert np.array_equal(_bits(z.out), _bits(got.out)) and np.array_equal(z.flags.cpu().numpy(), got.flags.cpu().numpy())
    with pytest.raises(L.LfBm5dError, match="without one sound value"):
        ctx.inpaint(_dev(lf), _dev(fl), mask, P, L.ROWMAJOR, 3, 1, 1, W, H, 1, iterations=1)


@pytest.mark.gpu
def test_deep_regions_do_not_depend_on_the_launches(ctx):
    """A region of depth 2R + 1 in a plane of several tiles (three launches) and one corner region of depth 3R in a small plane."""
    for H, W, box in ((80, 150, (20, 20 + 4 * R + 1, 60, 60 + 4 * R + 1)), (40, 40, (0, 3 * R, 0, 3 * R))):
        I = np.random.default_rng(H).uniform(0.0, 255.0, (H, W)).astype(np.float32)
        f = np.zeros((H, W), np.uint8)
        f[box[0]:box[1], box[2]:box[3]] = 1
        got, want = _assert_fill_equals_model(ctx, I.reshape(1, -1), f.reshape(1, -1), np.ones(1, np.uint32), W, H, 1)
        print(f"{H} x {W}: {got.passes} passes, {got.launches} launches")
        assert got.passes == M.chebyshev_depth(f != 0) > 2 * R and got.launches >= 3 and got.left == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("A,C_,H,W,masked", [(3, 3, 5, 3, 1), (2, 1, 64, 64, None), (2, 3, 37, 70, None)])
def test_projection_equals_the_model(ctx, A, C_, H, W, masked):
    import torch
    rng = np.random.default_rng(W)
    x = rng.uniform(0.0, 255.0, (A, C_ * H * W)).astype(np.float32)
    y = rng.uniform(0.0, 255.0, (A, C_ * H * W)).astype(np.float32)
    f = ((rng.random(x.shape) < 0.3) * rng.integers(1, 256, x.shape)).astype(np.uint8)
    y[0, 3] = np.nan
    f[0, 3] = 1
    x[0, 5] = np.nan                                                           # selected or not, a value is moved, never computed with
    mask = np.ones(A, np.uint32)
    if masked is not None:
        mask[masked] = 0
    live = mask != 0
    dx, dy, df = _dev(x), _dev(y), _dev(f)
    out = torch.full_like(dx, OUT_SENTINEL)
    ctx.inpaint_project(df, dx, dy, mask, out, W, H, C_)
    want = M.project(f, x, y)
    assert np.array_equal(_bits(out)[live], want.view(np.uint32)[live]) and (out.cpu().numpy()[~live] == OUT_SENTINEL).all()
    assert np.array_equal(_bits(dx), x.view(np.uint32)) and np.array_equal(_bits(dy), y.view(np.uint32))
    off = torch.full((A * C_ * H * W + 1,), OUT_SENTINEL, dtype=torch.float32, device="cuda")    # an output that is not 16-byte aligned
    ctx.inpaint_project(df, dx, dy, mask, off[1:].view(A, -1), W, H, C_)
    assert np.array_equal(_bits(off[1:].view(A, -1))[live], want.view(np.uint32)[live]) and off[0].item() == OUT_SENTINEL
    ctx.inpaint_project(df, dx, dy, mask, dx, W, H, C_)                         # in place
    assert np.array_equal(_bits(dx)[live], want.view(np.uint32)[live])


def _golden_case():
    """Golden light field, rows and columns 80..143, all 9 SAIs, 3 channels; add_defects(seed=3)."""
    clean = np.load(GOLDEN)[:, :, 80:144, 80:144].astype(np.float32).reshape(9, -1)
    fl = synth.add_defects((9, 3, 64, 64), 3).reshape(9, -1)
    return clean, fl, np.ones(9, np.uint32)


@pytest.mark.gpu
def test_loop_is_bit_identical_to_the_same_calls_made_by_hand(ctx):
    import torch
    K = 2
    clean, fl, mask = _golden_case()
    y = np.where(fl, np.float32(np.nan), clean)                                 # the defects are holes of NaN
    d_y, d_f = _dev(y), _dev(fl.astype(np.uint8))
    P = core.make_params(0.0, 2.7, *HT)
    a = ctx.inpaint(d_y, d_f, mask, P, *TAIL, iterations=K, sigma_start=30.0, sigma_end=5.0, return_flags=True)
    assert np.array_equal(_bits(d_y), y.view(np.uint32)) and np.array_equal(d_f.cpu().numpy(), fl.astype(np.uint8))
    b = ctx.inpaint(d_y, d_f, mask, P, *TAIL, iterations=K, sigma_start=30.0, sigma_end=5.0)
    assert np.array_equal(_bits(a.out), _bits(b.out)) and a[2:] == b[2:]

    x0 = ctx.inpaint_fill(d_y, d_f, mask, 64, 64, 3, return_flags=True)
    assert np.array_equal(x0.flags.cpu().numpy(), a.flags.cpu().numpy())
    x = x0.out
    for sig in M.sigma_schedule(K, 30.0, 5.0):
        z = x.clone()
        basic = torch.zeros_like(z)
        ctx.step1(core.make_params(sig, 2.7, *HT), z, mask, basic, *TAIL)
        x = torch.zeros_like(z)
        ctx.inpaint_project(x0.flags, basic, d_y, mask, x, 64, 64, 3)
    assert np.array_equal(_bits(a.out), _bits(x))
    assert np.isfinite(a.out.cpu().numpy()).all()
    assert np.array_equal(_bits(a.out)[~fl], clean.view(np.uint32)[~fl])         # the sound data, bit for bit
    one = ctx.inpaint(d_y, d_f, mask, P, *TAIL, iterations=1, sigma_start=30.0, sigma_end=5.0)
    assert not np.array_equal(_bits(one.out), _bits(a.out))
    # sigma_noise is a floor under the schedule: above sigma_start every step runs at it
    fl10 = ctx.inpaint(d_y, d_f, mask, P, *TAIL, iterations=K, sigma_start=30.0, sigma_end=5.0, sigma_noise=35.0)
    same = ctx.inpaint(d_y, d_f, mask, P, *TAIL, iterations=K, sigma_start=35.0, sigma_end=35.0)
    assert np.array_equal(_bits(fl10.out), _bits(same.out))


@pytest.fixture(scope="module")
def cpu_composition():
    """The CPU composition of tests/test_inpaint.py (K = 4, sigma 30 -> 5, clean data, flagged values zeroed), once."""
    clean, fl, mask = _golden_case()
    y = np.where(fl, np.float32(0.0), clean)

    def step(z, sig):
        _, basic, _ = O.run_step1(O.make_params(sig, 2.7, *HT), z.reshape(9, -1), mask, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        return basic
    x, x0, r = M.loop(y, fl, mask, 64, 64, 3, 4, 30.0, 5.0, step)
    return clean, fl, mask, y, x, x0


@pytest.mark.gpu
def test_loop_against_the_cpu_composition(ctx, cpu_composition):
    """|PSNR_gpu - PSNR_cpu| over the flagged values <= 0.01 K dB (the project's +-0.01 dB per step, summed over the loop's K steps), and
    the loop gains >= 5 dB over the GPU's fill (half of the gain of the CPU composition).  Measured on an MI355X:
    profiles/inpaint_parity.txt."""
    K = 4
    clean, fl, mask, y, x_cpu, x0_cpu = cpu_composition
    cpu, cpu_fill = M.psnr_on(x_cpu, clean, fl), M.psnr_on(x0_cpu, clean, fl)
    got = ctx.inpaint(_dev(y), _dev(fl.astype(np.uint8)), mask, core.make_params(0.0, 2.7, *HT), *TAIL, iterations=K, sigma_start=30.0,
                      sigma_end=5.0)
    fill = ctx.inpaint_fill(_dev(y), _dev(fl.astype(np.uint8)), mask, 64, 64, 3)
    assert np.array_equal(_bits(fill.out), x0_cpu.view(np.uint32))              # the fill is the model's, bit for bit
    gpu, gpu_fill = M.psnr_on(got.out.cpu().numpy(), clean, fl), M.psnr_on(fill.out.cpu().numpy(), clean, fl)
    print(f"K={K} 30 -> 5: fill {gpu_fill:.4f} dB, loop gpu {gpu:.4f} dB, loop cpu {cpu:.4f} dB, gpu-cpu {gpu - cpu:+.4f} dB "
          f"(allowed {0.01 * K:.2f}), gain over the fill {gpu - gpu_fill:.4f} dB; {got.passes} passes, flagged {got.flagged}")
    assert abs(gpu - cpu) <= 0.01 * K
    assert gpu - gpu_fill >= 5.0


def _psnr(x, clean):
    return float(10.0 * np.log10(255.0 ** 2 / ((np.asarray(x, np.float64) - clean) ** 2).mean()))


@pytest.mark.gpu
def test_refinement_ahead_of_the_denoiser(ctx):
    """3x3x64x64 golden crop, sigma = 10 (the checker's seeded noise, seed 1), add_defects(seed=3) with the flagged values zeroed; HT and
    Wiener parameters of the CPU study; whole-field PSNR of `denoise` behind the fill alone and behind the loop (K = 4, sigma 40 -> 10,
    sigma_noise = 10).  The CPU composition gave: undamaged 37.99, damaged 18.76, fill 35.81, fill + loop 37.57 dB: the floor is half of
    its gain of 1.76 dB.  Measured on an MI355X: profiles/inpaint_parity.txt."""
    import torch
    clean, fl, mask = _golden_case()
    noisy = O.add_noise_lf(clean.copy(), 10.0, seed=1)
    damaged = np.where(fl, np.float32(0.0), noisy)
    d_f = _dev(fl.astype(np.uint8))
    P1, P2 = core.make_params(10.0, 2.7, *HT), core.make_params(10.0, 2.7, *WIEN)

    def denoised(x):
        basic, den = torch.zeros_like(x), torch.zeros_like(x)
        ctx.denoise(P1, P2, x.clone(), mask, basic, den, L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
        return _psnr(den.cpu().numpy(), clean)

    p_clean, p_damaged = denoised(_dev(noisy)), denoised(_dev(damaged))
    fill = ctx.inpaint(_dev(damaged), d_f, mask, P1, *TAIL, iterations=0)
    loop = ctx.inpaint(_dev(damaged), d_f, mask, P1, *TAIL, iterations=4, sigma_start=40.0, sigma_end=10.0, sigma_noise=10.0)
    p_fill, p_loop = denoised(fill.out), denoised(loop.out)
    print(f"end to end at sigma 10: undamaged {p_clean:.4f} dB, damaged {p_damaged:.4f} dB, fill {p_fill:.4f} dB, fill + loop {p_loop:.4f} dB, "
          f"gain of the loop {p_loop - p_fill:.4f} dB (CPU composition: 37.99, 18.76, 35.81, 37.57, 1.76)")
    assert p_loop - p_fill >= 0.88
    assert p_clean > p_loop > p_fill > p_damaged


@pytest.mark.gpu
def test_host_forms_return_the_device_forms_bits(ctx):
    clean, fl, mask = _golden_case()
    mask = mask.copy()
    mask[5] = 0
    live = mask != 0
    y = np.where(fl, np.float32(0.0), clean)
    f8 = fl.astype(np.uint8)
    P = core.make_params(0.0, 2.7, *HT)
    kw = dict(iterations=2, sigma_start=30.0, sigma_end=5.0)
    dev = ctx.inpaint(_dev(y), _dev(f8), mask, P, *TAIL, return_flags=True, **kw)
    d_out, d_codes = dev.out.cpu().numpy(), dev.flags.cpu().numpy()
    assert np.array_equal(d_out.view(np.uint32)[5], y.view(np.uint32)[5])        # a fresh device result carries the empty SAI's input
    h = ctx.inpaint(y.copy(), f8, mask, P, *TAIL, return_flags=True, **kw)       # flat host arrays
    assert isinstance(h.out, np.ndarray) and h.out.shape == y.shape
    assert np.array_equal(h.out.view(np.uint32)[live], d_out.view(np.uint32)[live]) and np.array_equal(h.flags[live], d_codes[live])
    assert h[2:] == dev[2:]
    sais = [y[i].copy() if mask[i] else None for i in range(9)]                  # one array per SAI, NULL for the empty one
    fls = [f8[i].copy() if mask[i] else None for i in range(9)]
    outs = [np.zeros(y.shape[1], np.float32) if mask[i] else None for i in range(9)]
    l = L.inpaint(sais, fls, mask, P, *TAIL, ctx=ctx, out=outs, **kw)
    assert all(np.array_equal(outs[i].view(np.uint32), d_out.view(np.uint32)[i]) for i in range(9) if mask[i])
    assert l[2:] == dev[2:] and l.flags is None
    cpp, flagged, left, passes = core.inpaint_probe(y, f8, mask, 3, 3, 64, 64, 3, 2.7, HT, **kw)     # the C++ drop-in's inpaint_LF
    assert np.array_equal(cpp.view(np.uint32)[live], d_out.view(np.uint32)[live])
    assert (flagged, left, passes) == (sum(dev.flagged), 0, dev.passes)
    cpp0, _, _, _ = core.inpaint_probe(y, f8, mask, 3, 3, 64, 64, 3, 2.7, HT, iterations=0)
    fill = ctx.inpaint_fill(_dev(y), _dev(f8), mask, 64, 64, 3)
    assert np.array_equal(cpp0.view(np.uint32)[live], _bits(fill.out)[live])


@pytest.mark.gpu
def test_rejected_calls(ctx):
    import torch
    lf, fl, mask = _case(4, 3, 40, 66)
    d, df = _dev(lf), _dev(fl)
    out = torch.zeros_like(d)
    codes = torch.zeros_like(df)
    P = core.make_params(0.0, 2.7, *HT)
    loop = (P, L.ROWMAJOR, 2, 2, 1, 66, 40, 3)
    with pytest.raises(L.LfBm5dError, match="overlap"):
        ctx.inpaint_fill(d, df, mask, 66, 40, 3, out=d)
    with pytest.raises(L.LfBm5dError, match="overlap"):
        ctx.inpaint(d, df, mask, *loop, out=d)
    with pytest.raises(L.LfBm5dError, match="overlap"):
        ctx.inpaint_fill(d, df, mask, 66, 40, 3, out=out, flags_out=df)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.inpaint_fill(d, df, mask, 66 * 3 // 2, 40, 2, out=out)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.inpaint(d, df, mask, P, L.ROWMAJOR, 2, 2, 1, 99, 40, 2, out=out)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.inpaint_fill(d, df, mask, 1, 40 * 66, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.inpaint_project(df, d, d, mask, out, 40 * 66, 1, 3)
    with pytest.raises(L.LfBm5dError, match="non-empty"):
        ctx.inpaint_fill(d, df, np.zeros(4, np.uint32), 66, 40, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="non-empty"):
        ctx.inpaint(d, df, np.zeros(4, np.uint32), *loop, out=out)
    for kw, word in ((dict(sigma_start=3.0, sigma_end=4.0), "sigma_end"), (dict(sigma_end=0.0), "positive"), (dict(sigma_start=-1.0), "positive"),
                     (dict(sigma_noise=-1.0), "sigma_noise"), (dict(sigma_noise=float("nan")), "sigma_noise")):
        with pytest.raises(L.LfBm5dError, match=word):
            ctx.inpaint(d, df, mask, *loop, out=out, **kw)
    whole = torch.ones_like(df)                                                  # K >= 1 with values left
    with pytest.raises(L.LfBm5dError, match="without one sound value"):
        ctx.inpaint(d, whole, mask, *loop, out=out.clone(), iterations=1)
    assert sum(ctx.inpaint(d, whole, mask, *loop, iterations=0).left) == lf.size   # ... the fill alone reports them
    assert not out.any().item() and not codes.any().item()                       # nothing was written by a rejected call
    lib, h = core.lib(), ctx._h
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint))
    ip, res = L.inpaint_params(), core.InpaintResultStruct()
    p, q, f = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(df.data_ptr())
    tail = (4, 66, 40, 3)
    for args in ((None, f, mp, q), (p, None, mp, q), (p, f, None, q), (p, f, mp, None)):
        assert lib.lfbm5d_inpaint_fill_device(h, *args, None, *tail, C.byref(res)) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    ltail = (L.ROWMAJOR, 2, 2, 1, 66, 40, 3)
    for args in ((None, C.byref(P), p, f, mp, q), (C.byref(ip), None, p, f, mp, q), (C.byref(ip), C.byref(P), None, f, mp, q),
                 (C.byref(ip), C.byref(P), p, None, mp, q), (C.byref(ip), C.byref(P), p, f, None, q), (C.byref(ip), C.byref(P), p, f, mp, None)):
        assert lib.lfbm5d_inpaint_device(h, *args, None, *ltail, C.byref(res)) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    for args in ((None, p, p, mp, q), (f, None, p, mp, q), (f, p, None, mp, q), (f, p, p, None, q), (f, p, p, mp, None)):
        assert lib.lfbm5d_inpaint_project_device(h, *args, *tail) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    ptrs = (C.c_void_p * 4)()                                                    # non-empty SAIs without a pointer
    assert lib.lfbm5d_inpaint_host_sai(h, C.byref(ip), C.byref(P), ptrs, ptrs, mp, ptrs, None, *ltail, C.byref(res)) == 1
    assert "NULL" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_inpaint_fill_device(h, p, f, mp, q, None, *tail, None) == 0  # codes and result are optional
    sharded = L.Context(0)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.inpaint_fill(d, df, mask, 66, 40, 3, out=out)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.inpaint(d, df, mask, *loop, out=out)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.inpaint_project(df, d, d, mask, out, 66, 40, 3)
    finally:
        sharded.close()


def _write_source_lf(tmp):
    from PIL import Image
    lf = np.load(GOLDEN)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff", "defects"):
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


def _defect_line(stdout):
    m = re.search(r"Defect inpainting: (\d+) of (\d+) values flagged \(([0-9.eE+-]+) %\), (\d+) left; (\d+) fill passes, (\d+) refinement steps", stdout)
    assert m, stdout[-2000:]
    return int(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))


def _shape_of(stdout):
    """stdout with every number and progress line taken out: what stays the same from run to run."""
    lines = [l for l in stdout.replace("\r", "\n").split("\n") if "Defect inpainting" not in l]
    return re.sub(r"\n+", "\n", re.sub(r"[0-9.eE+-]+", "#", "\n".join(lines)))


@pytest.mark.gpu
def test_cli_fills_and_refines_under_a_defect_directory(tmp_path):
    """The golden 3 x 3 files at sigma 25 with a directory of defect maps: grey files (every channel), one colour file (one channel),
    one SAI without a file."""
    from PIL import Image
    tmp = str(tmp_path)
    src = _write_source_lf(tmp)
    maps = synth.add_defects((9, 1, 256, 256), 3)[:, 0]
    want = 0
    for i in range(9):
        name = f"{tmp}/defects/SAI_{i // 3 + 1:02d}_{i % 3 + 1:02d}.png"
        if i == 4:
            continue                                                           # no file: no defects in this SAI
        if i == 7:                                                             # a colour file: the green channel alone
            rgb = np.zeros((256, 256, 3), np.uint8)
            rgb[..., 1] = maps[i] * 200
            Image.fromarray(rgb).save(name)
            want += int(maps[i].sum())
        else:
            Image.fromarray((maps[i] * 255).astype(np.uint8)).save(name)
            want += 3 * int(maps[i].sum())
    depth = max(M.chebyshev_depth(maps[i]) for i in range(9) if i != 4)
    env = dict(os.environ, LFBM5D_SEED="1")
    plain = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=env)
    assert plain.returncode == 0 and "Defect" not in plain.stdout
    noisy_plain = open(f"{tmp}/noisy/SAI_01_01.png", "rb").read()
    out = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_DEFECTS=f"{tmp}/defects", LFBM5D_DEFECTS_ITER="1"))
    assert out.returncode == 0, out.stdout[-2000:]
    n, N, pct, left, passes, K = _defect_line(out.stdout)
    print(f"LFBM5D_DEFECTS LFBM5D_DEFECTS_ITER=1: {n} of {N} flagged ({pct} %), {left} left, {passes} passes, {K} steps")
    assert (n, N, left, passes, K) == (want, 9 * 3 * 256 * 256, 0, depth, 1) and abs(pct - 100.0 * n / N) < 1e-3
    assert open(f"{tmp}/noisy/SAI_01_01.png", "rb").read() == noisy_plain        # the noisy files are saved before the fill
    assert _shape_of(out.stdout) == _shape_of(plain.stdout)                      # nothing else is printed
    txt = open(f"{tmp}/measures.txt").read()
    assert float(txt.split("-> Average PSNR denoised = ")[-1].split()[0]) > 30.0
    # the library's number of steps without LFBM5D_DEFECTS_ITER; LFBM5D_SIGMA=poisson and LFBM3Ddenoising run the fill alone and say so
    pois = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_DEFECTS=f"{tmp}/defects", LFBM5D_SIGMA="poisson"))
    assert pois.returncode == 0, pois.stdout[-2000:]
    assert _defect_line(pois.stdout)[5] == 0 and "the fill alone" in pois.stdout
    tmp3 = os.path.join(tmp, "bm3d")
    os.makedirs(tmp3)
    src3 = _write_source_lf(tmp3)
    out3 = subprocess.run(_readme_args(CLI3, tmp3, src3), capture_output=True, text=True, env=dict(env, LFBM5D_DEFECTS=f"{tmp}/defects", LFBM5D_SIGMA="auto"))
    assert out3.returncode == 0, out3.stdout[-2000:]
    n3, N3, _, left3, _, K3 = _defect_line(out3.stdout)
    assert (n3, N3, left3, K3) == (3 * int(maps[[0, 1, 3]].sum()), 4 * 3 * 256 * 256, 0, 0) and "the fill alone" in out3.stdout
    assert out3.stdout.index("Defect inpainting:") < out3.stdout.index("Estimated noise level:")
    for bad in ("x", "-1", "", "1.5"):
        r = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_DEFECTS=f"{tmp}/defects", LFBM5D_DEFECTS_ITER=bad))
        assert r.returncode != 0 and "LFBM5D_DEFECTS_ITER must be" in r.stdout, bad
