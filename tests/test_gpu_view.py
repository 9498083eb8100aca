"""GPU tests of the view synthesis (lfbm5d_view_*, include/lfbm5d.h): the plane sweep equals the numpy model (tests/view_model.py) bit for
bit -- values, disparities, counts, histogram -- at every tile edge, in planes narrower than shift plus halo, with degenerate angular axes,
empty SAIs among the sources and SAIs without a source; the loop against the same public calls made by hand (bits) and against the CPU
composition of the model with the checker's run_step1 (PSNR); what the defaults gain over the mean of the neighbours; the host forms, the
C++ drop-in, rejected calls and the CLIs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
from oracle import oracle as O
import helpers
import view_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
OUT_SENTINEL, DISP_SENTINEL = -7.0, 99
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")       # N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D: the super-resolution tests' parameters
WIEN = (16, 8, 3, 8, 3, "dct", "sadct", "haar")
TAIL = (L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
TILE_W, TILE_H = 64, 32                             # k_view_sweep's tile
DS, RS = (0, 1, 3, 8), (0, 3, 7)


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


def _data(kind, ah, aw, H, W, C_, seed):
    """[ah*aw][C*H*W] float32: uniform random values, or the photograph moving 2 pixels per view."""
    if kind == "uniform":
        return np.random.default_rng(seed).uniform(0.0, 255.0, (ah * aw, C_ * H * W)).astype(np.float32)
    return helpers.textured_lf(ah, aw, H, W, 2)[:, :C_].astype(np.float32).reshape(ah * aw, -1)


def _assert_equals_model(ctx, lf, mask, missing, ang_major, aw, ah, W, H, C_, D, r, R=1):
    """One synthesis against the model: values, disparities, counts and histogram, with sentinels in what must not be written; and a
    second call returns the same bits."""
    A = aw * ah
    x = lf.copy()
    x[(missing != 0) | (mask == 0)] = np.nan                                    # never read
    out0 = np.full(lf.shape, OUT_SENTINEL, np.float32)
    disp0 = np.full((A, H * W), DISP_SENTINEL, np.int8)
    want = M.fill(x, mask, missing, ang_major, aw, ah, W, H, C_, D, r, R, out=out0, disp=disp0)
    d = _dev(x)
    out, disp = _dev(out0), _dev(disp0)
    got = ctx.view_fill(d, mask, missing, ang_major, aw, ah, W, H, C_, max_disparity=D, box_radius=r, ang_radius=R, out=out, disparity_out=disp)
    tag = f"D={D} r={r} R={R}"
    assert np.array_equal(_bits(d), x.view(np.uint32)), tag                     # the input is only read
    assert np.array_equal(disp.cpu().numpy(), want["disp"]), tag
    assert np.array_equal(_bits(out), want["out"].view(np.uint32)), tag
    assert (got.missing, got.synthesised, got.left, got.pixels) == (want["missing"], want["synthesised"], want["left"], want["pixels"]), tag
    assert list(got.disparity_hist) == list(want["hist"]), tag
    assert got.out is out and got.disparity is disp
    again = ctx.view_fill(d, mask, missing, ang_major, aw, ah, W, H, C_, max_disparity=D, box_radius=r, ang_radius=R, return_disparity=True)
    s = want["sais"]
    assert np.array_equal(_bits(again.out)[s], _bits(out)[s]) and np.array_equal(again.disparity.cpu().numpy()[s], want["disp"][s]), tag
    assert again[2:] == got[2:], tag
    return got, want


def _missing(A, sais):
    m = np.zeros(A, np.uint32)
    m[list(sais)] = 1
    return m


ODD_5X5 = [s * 5 + t for s in range(5) for t in range(5) if s % 2 or t % 2]
# ah, aw, H, W, C, missing, empty, ang_radius
SHAPES = {
    "centre": (3, 3, 37, 70, 3, [4], [], 1),
    "corners": (3, 3, 37, 70, 3, [0, 2, 6, 8], [], 1),
    "empty-source": (3, 3, 37, 70, 3, [4], [1], 1),
    "upsample-R1": (5, 5, 33, 34, 1, ODD_5X5, [], 1),
    "upsample-R2": (5, 5, 33, 34, 1, ODD_5X5, [], 2),
    "narrow-1x3": (1, 3, 5, 3, 1, [1], [], 1),                                  # planes narrower than shift plus halo: several reflections
    "narrow-3x1": (3, 1, 2, 2, 1, [0], [], 2),
    "single-63": (2, 1, 65, 63, 1, [1], [], 1),                                 # one source: a copy, d = 0
    "single-64": (2, 1, 65, 64, 1, [1], [], 1),
    "single-65": (2, 1, 65, 65, 1, [0], [], 1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "textured"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_synthesis_equals_the_model(ctx, shape, kind):
    ah, aw, H, W, C_, miss, empty, R = SHAPES[shape]
    lf = _data(kind, ah, aw, H, W, C_, seed=H * 1000 + W)
    mask = np.ones(ah * aw, np.uint32)
    mask[empty] = 0
    missing = _missing(ah * aw, miss)
    for D in DS:
        for r in RS:
            got, want = _assert_equals_model(ctx, lf, mask, missing, L.ROWMAJOR, aw, ah, W, H, C_, D, r, R)
            assert (got.missing, got.synthesised, got.left) == (len(miss), len(miss), 0)
            o = got.out.cpu().numpy()
            assert np.isfinite(o[miss]).all()
            untouched = [i for i in range(ah * aw) if i not in miss]
            assert (o[untouched] == OUT_SENTINEL).all() and (got.disparity.cpu().numpy()[untouched] == DISP_SENTINEL).all()
            if shape.startswith("single"):
                src = 1 - miss[0]
                assert np.array_equal(o[miss[0]].view(np.uint32), lf[src].view(np.uint32)) and got.disparity_hist[8] == H * W
    if kind == "textured" and shape == "centre":                                # the photograph moves 2 pixels per view: found at D >= 2
        b = 8 + 7
        d = got.disparity.cpu().numpy()[4].reshape(H, W)[b:-b, b:-b]
        assert (np.abs(d) == 2).all()


def _step_edge_lf(H, W):
    """3 x 3 views of a scene with a background at disparity 0 and diagonal foreground stripes at disparity 2: the step edges cross every
    tile edge and corner of the plane."""
    src = np.load(GOLDEN)[4].astype(np.float32)                                 # [3][256][256]
    ys, xs = np.mgrid[0:H, 0:W]
    lf = np.zeros((9, 3, H, W), np.float32)
    for s in range(3):
        for t in range(3):
            Y, X = ys + 2 * s, xs + 2 * t                                       # scene coordinates of the foreground
            fg = ((X + Y) % 48) < 24
            lf[s * 3 + t] = np.where(fg[None], src[:, Y + 100, X + 20], src[:, ys, xs])
    return lf.reshape(9, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(2 * TILE_H + 1, 2 * TILE_W - 1), (TILE_H - 1, TILE_W + 1)])
def test_step_edges_across_the_tile_edges(ctx, H, W):
    lf = _step_edge_lf(H, W)
    mask = np.ones(9, np.uint32)
    for miss in ([4], [0, 5]):
        for D, r in ((3, 3), (8, 7), (2, 0)):
            got, want = _assert_equals_model(ctx, lf, mask, _missing(9, miss), L.ROWMAJOR, 3, 3, W, H, 3, D, r)
    got, want = _assert_equals_model(ctx, lf, mask, _missing(9, [4]), L.ROWMAJOR, 3, 3, W, H, 3, 3, 3)
    h = got.disparity_hist
    print(f"{H} x {W}: histogram {dict((d - 8, n) for d, n in enumerate(h) if n)}")
    assert h[8] > H * W // 10 and h[8 + 2] + h[8 - 2] > H * W // 10              # both planes of the scene are found
    d = got.disparity.cpu().numpy()[4].reshape(H, W)
    for y in range(TILE_H - 1, H - 1, TILE_H):                                  # both disparities on both sides of every tile edge
        assert len(np.unique(d[y])) > 1 and len(np.unique(d[y + 1])) > 1
    for x in range(TILE_W - 1, W - 1, TILE_W):
        assert len(np.unique(d[:, x])) > 1 and len(np.unique(d[:, x + 1])) > 1


@pytest.mark.gpu
def test_an_sai_without_a_source_is_left(ctx):
    import torch
    H, W = 20, 30
    lf = _data("uniform", 3, 3, H, W, 3, seed=3)
    mask = np.ones(9, np.uint32)
    mask[[1, 3, 4]] = 0                                                         # the neighbours of SAI 0 are empty
    missing = _missing(9, [0, 8])
    got, want = _assert_equals_model(ctx, lf, mask, missing, L.ROWMAJOR, 3, 3, W, H, 3, 3, 3)
    assert (got.missing, got.synthesised, got.left, got.pixels) == (2, 1, 1, H * W)
    assert (got.out[0] == OUT_SENTINEL).all() and (got.disparity[0] == DISP_SENTINEL).all()
    got, want = _assert_equals_model(ctx, lf, mask, missing, L.ROWMAJOR, 3, 3, W, H, 3, 3, 3, R=2)   # within 2 views it has sources
    assert (got.synthesised, got.left) == (2, 0)
    only = _missing(9, [0])                                                     # nothing to synthesise: no launch, nothing written
    got, want = _assert_equals_model(ctx, lf, mask, only, L.ROWMAJOR, 3, 3, W, H, 3, 3, 3)
    assert (got.missing, got.synthesised, got.left, got.pixels, sum(got.disparity_hist)) == (1, 0, 1, 0, 0)
    assert (got.out == OUT_SENTINEL).all().item()
    # the loop's entry: K = 0 reports it, K >= 1 refuses it after the result is filled in
    P = core.make_params(0.0, 2.7, *HT)
    d = _dev(lf)
    z = ctx.view_synth(d, mask, missing, P, L.ROWMAJOR, 3, 3, 1, W, H, 3, max_disparity=3, box_radius=3, iterations=0)
    assert (z.synthesised, z.left) == (1, 1)
    with pytest.raises(L.LfBm5dError, match="without a source"):
        ctx.view_synth(d, mask, missing, P, L.ROWMAJOR, 3, 3, 1, W, H, 3, max_disparity=3, box_radius=3, iterations=1, out=torch.zeros_like(d))
    res = core.ViewResultStruct()
    vp = L.view_params(3, 3, 1, 1)
    up = C.POINTER(C.c_uint)
    o = torch.zeros_like(d)
    rc = core.lib().lfbm5d_view_device(ctx._h, C.byref(vp), C.byref(P), C.c_void_p(d.data_ptr()), mask.ctypes.data_as(up),
                                       missing.ctypes.data_as(up), C.c_void_p(o.data_ptr()), None, L.ROWMAJOR, 3, 3, 1, W, H, 3, C.byref(res))
    assert rc == 1 and (res.missing, res.synthesised, res.left) == (2, 1, 1)


@pytest.mark.gpu
def test_both_angular_orders(ctx):
    """2 x 3 views (aheight 2, awidth 3), both orders against the model; the column-major call on the permuted light field returns the
    row-major call's planes."""
    ah, aw, H, W = 2, 3, 21, 40
    lf = _data("textured", ah, aw, H, W, 3, 0)
    mask = np.ones(6, np.uint32)
    row, _ = _assert_equals_model(ctx, lf, mask, _missing(6, [1, 5]), L.ROWMAJOR, aw, ah, W, H, 3, 3, 3)
    perm = [(st % ah) * aw + st // ah for st in range(6)]                       # column-major index -> row-major index
    col, _ = _assert_equals_model(ctx, lf[perm], mask, _missing(6, [perm.index(1), perm.index(5)]), L.COLMAJOR, aw, ah, W, H, 3, 3, 3)
    for m in (1, 5):
        assert np.array_equal(_bits(col.out)[perm.index(m)], _bits(row.out)[m])
        assert np.array_equal(col.disparity.cpu().numpy()[perm.index(m)], row.disparity.cpu().numpy()[m])
    assert col.disparity_hist == row.disparity_hist


def _golden_crop(lo, hi):
    return np.load(GOLDEN)[:, :, lo:hi, lo:hi].astype(np.float32).reshape(9, -1)


@pytest.mark.gpu
def test_loop_is_bit_identical_to_the_same_calls_made_by_hand(ctx):
    import torch
    K = 2
    clean = _golden_crop(80, 144)
    mask, missing = np.ones(9, np.uint32), _missing(9, [4])
    y = clean.copy()
    y[4] = np.nan                                                               # never read
    d_y = _dev(y)
    P = core.make_params(0.0, 2.7, *HT)
    kw = dict(max_disparity=3, box_radius=3, iterations=K, sigma_start=30.0, sigma_end=5.0)
    a = ctx.view_synth(d_y, mask, missing, P, *TAIL, return_disparity=True, **kw)
    assert np.array_equal(_bits(d_y), y.view(np.uint32))
    b = ctx.view_synth(d_y, mask, missing, P, *TAIL, **kw)
    assert np.array_equal(_bits(a.out), _bits(b.out)) and a[2:] == b[2:]

    x0 = ctx.view_fill(d_y, mask, missing, L.ROWMAJOR, 3, 3, 64, 64, 3, max_disparity=3, box_radius=3, return_disparity=True)
    assert np.array_equal(x0.disparity.cpu().numpy(), a.disparity.cpu().numpy())
    flags = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
    flags[4] = 1
    x = x0.out
    for sig in M.sigma_schedule(K, 30.0, 5.0):
        z = x.clone()
        basic = torch.zeros_like(z)
        ctx.step1(core.make_params(sig, 2.7, *HT), z, mask, basic, *TAIL)
        x = torch.zeros_like(z)
        ctx.inpaint_project(flags, basic, d_y, mask, x, 64, 64, 3)
    assert np.array_equal(_bits(a.out), _bits(x))
    assert np.isfinite(a.out.cpu().numpy()).all()
    sound = missing == 0
    assert np.array_equal(_bits(a.out)[sound], clean.view(np.uint32)[sound])    # the sound SAIs, bit for bit
    zero = ctx.view_synth(d_y, mask, missing, P, *TAIL, max_disparity=3, box_radius=3, iterations=0)
    assert np.array_equal(_bits(zero.out), _bits(x0.out))                       # K = 0 is the synthesis alone
    one = ctx.view_synth(d_y, mask, missing, P, *TAIL, max_disparity=3, box_radius=3, iterations=1, sigma_start=30.0, sigma_end=5.0)
    assert not np.array_equal(_bits(one.out), _bits(a.out))
    # sigma_noise is a floor under the schedule: above sigma_start every step runs at it
    floor = ctx.view_synth(d_y, mask, missing, P, *TAIL, sigma_noise=35.0, **kw)
    same = ctx.view_synth(d_y, mask, missing, P, *TAIL, **dict(kw, sigma_start=35.0, sigma_end=35.0))
    assert np.array_equal(_bits(floor.out), _bits(same.out))


@pytest.mark.gpu
def test_defaults_beat_the_mean_of_the_neighbours(ctx):
    """Golden rows and columns 64..191, centre missing: the GPU at the shipped defaults gains over the D = 0 result (the mean of the
    neighbours) at least half of what the model gains with the same parameters.  The GPU equals the model bit for bit, so this guards
    the defaults."""
    clean = _golden_crop(64, 192)
    mask, missing = np.ones(9, np.uint32), _missing(9, [4])
    vp = L.view_params()
    D, r, R = vp.max_disparity, vp.box_radius, vp.ang_radius
    y = clean.copy()
    y[4] = 0.0
    m0 = M.psnr(M.fill(y, mask, missing, L.ROWMAJOR, 3, 3, 128, 128, 3, 0, r, R)["out"][4], clean[4])
    m1 = M.psnr(M.fill(y, mask, missing, L.ROWMAJOR, 3, 3, 128, 128, 3, D, r, R)["out"][4], clean[4])
    g0 = ctx.view_fill(_dev(y), mask, missing, L.ROWMAJOR, 3, 3, 128, 128, 3, max_disparity=0)
    g1 = ctx.view_fill(_dev(y), mask, missing, L.ROWMAJOR, 3, 3, 128, 128, 3)
    p0, p1 = M.psnr(g0.out.cpu().numpy()[4], clean[4]), M.psnr(g1.out.cpu().numpy()[4], clean[4])
    print(f"defaults D={D} r={r} R={R}: model mean {m0:.4f} dB, model {m1:.4f} dB (gain {m1 - m0:.4f}); gpu mean {p0:.4f} dB, gpu {p1:.4f} dB "
          f"(gain {p1 - p0:.4f}, floor {(m1 - m0) / 2:.4f})")
    assert m1 - m0 > 0.0
    assert p1 - p0 >= (m1 - m0) / 2


def _composition(y, mask, missing, K, s0, s1, sn):
    def step(z, sig):
        _, basic, _ = O.run_step1(O.make_params(sig, 2.7, *HT), z.reshape(9, -1), mask, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        return basic
    return M.loop(y, mask, missing, L.ROWMAJOR, 3, 3, 64, 64, 3, 3, 3, K, s0, s1, step, sigma_noise=sn)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [0.0, 10.0])
def test_loop_against_the_cpu_composition(ctx, noise):
    """3 x 3 x 64 x 64 golden crop, centre missing, D = 3, r = 3, K = 4.  Clean data: sigma 30 -> 5.  Sigma = 10 noise (the checker's
    seeded noise, seed 1): sigma 40 -> 10 with sigma_noise = 10, then HT + Wiener at sigma 10.  |PSNR_gpu - PSNR_cpu| over the missing SAI
    <= 0.01 K dB (the project's +-0.01 dB per step, summed over the loop's K steps); where the CPU composition gains over the synthesis
    alone the GPU loop must gain half of that.  The CPU composition's figures: profiles/view_parity.txt."""
    import torch
    K = 4
    clean = _golden_crop(80, 144)
    mask, missing = np.ones(9, np.uint32), _missing(9, [4])
    y = O.add_noise_lf(clean.copy(), noise, seed=1) if noise else clean.copy()
    y[4] = 0.0
    s0, s1 = (40.0, 10.0) if noise else (30.0, 5.0)
    x_cpu, x0_cpu, _ = _composition(y, mask, missing, K, s0, s1, noise)
    cpu, cpu0 = M.psnr(x_cpu[4], clean[4]), M.psnr(x0_cpu[4], clean[4])
    P = core.make_params(0.0, 2.7, *HT)
    kw = dict(max_disparity=3, box_radius=3)
    fill = ctx.view_synth(_dev(y), mask, missing, P, *TAIL, iterations=0, **kw)
    got = ctx.view_synth(_dev(y), mask, missing, P, *TAIL, iterations=K, sigma_start=s0, sigma_end=s1, sigma_noise=noise, **kw)
    assert np.array_equal(_bits(fill.out), x0_cpu.view(np.uint32))              # the synthesis is the model's, bit for bit
    gpu, gpu0 = M.psnr(got.out.cpu().numpy()[4], clean[4]), M.psnr(fill.out.cpu().numpy()[4], clean[4])
    print(f"sigma {noise:g}, K={K} {s0:g} -> {s1:g}: synthesis {gpu0:.4f} dB, loop gpu {gpu:.4f} dB, loop cpu {cpu:.4f} dB, gpu-cpu {gpu - cpu:+.4f} dB "
          f"(allowed {0.01 * K:.2f}), gain over the synthesis gpu {gpu - gpu0:+.4f} dB, cpu {cpu - cpu0:+.4f} dB")
    assert abs(gpu - cpu) <= 0.01 * K
    if cpu - cpu0 > 0.0:
        assert gpu - gpu0 >= (cpu - cpu0) / 2
    if noise:                                                                   # what it is worth in front of the denoiser
        P1, P2 = core.make_params(noise, 2.7, *HT), core.make_params(noise, 2.7, *WIEN)

        def denoised(x):
            basic, den = torch.zeros_like(x), torch.zeros_like(x)
            ctx.denoise(P1, P2, x.clone(), mask, basic, den, L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
            return M.psnr(den.cpu().numpy()[4], clean[4]), M.psnr(den.cpu().numpy(), clean)
        whole = denoised(_dev(O.add_noise_lf(clean.copy(), noise, seed=1)))
        p_fill, p_loop = denoised(fill.out), denoised(got.out)
        print(f"denoised at sigma {noise:g} (missing SAI, whole field): all SAIs present {whole[0]:.4f} {whole[1]:.4f} dB, behind the synthesis "
              f"{p_fill[0]:.4f} {p_fill[1]:.4f} dB, behind the loop {p_loop[0]:.4f} {p_loop[1]:.4f} dB")
        assert whole[0] > max(p_fill[0], p_loop[0])                             # a reconstruction does not beat the SAI itself


@pytest.mark.gpu
def test_host_forms_return_the_device_forms_bits(ctx):
    clean = _golden_crop(80, 144)
    mask, missing = np.ones(9, np.uint32), _missing(9, [4, 2])
    mask[5] = 0
    live = mask != 0
    y = clean.copy()
    y[[2, 4]] = np.nan
    P = core.make_params(0.0, 2.7, *HT)
    kw = dict(max_disparity=3, box_radius=2, iterations=2, sigma_start=30.0, sigma_end=5.0)
    dev = ctx.view_synth(_dev(y), mask, missing, P, *TAIL, return_disparity=True, **kw)
    d_out, d_disp = dev.out.cpu().numpy(), dev.disparity.cpu().numpy()
    assert np.array_equal(d_out.view(np.uint32)[5], y.view(np.uint32)[5])        # a fresh device result carries the empty SAI's input
    h = ctx.view_synth(y.copy(), mask, missing, P, *TAIL, return_disparity=True, **kw)   # flat host arrays
    assert isinstance(h.out, np.ndarray) and h.out.shape == y.shape
    assert np.array_equal(h.out.view(np.uint32)[live], d_out.view(np.uint32)[live]) and np.array_equal(h.disparity[[2, 4]], d_disp[[2, 4]])
    assert h[2:] == dev[2:]
    sais = [y[i].copy() if mask[i] and not missing[i] else None for i in range(9)]   # one array per SAI, NULL for empty and missing ones
    outs = [np.zeros(y.shape[1], np.float32) if mask[i] else None for i in range(9)]
    l = L.view_synth(sais, mask, missing, P, *TAIL, ctx=ctx, out=outs, **kw)
    assert all(np.array_equal(outs[i].view(np.uint32), d_out.view(np.uint32)[i]) for i in range(9) if mask[i])
    assert l[2:] == dev[2:] and l.disparity is None
    cpp, done, left, dmin, dmax = core.view_synth_probe(y, mask, missing, 3, 3, 64, 64, 3, 2.7, HT, **kw)   # the C++ drop-in's view_synth_LF
    assert np.array_equal(cpp.view(np.uint32)[live], d_out.view(np.uint32)[live])
    hist = np.array(dev.disparity_hist)
    assert (done, left, dmin, dmax) == (2, 0, int(np.nonzero(hist)[0][0]) - 8, int(np.nonzero(hist)[0][-1]) - 8)
    cpp0, _, _, _, _ = core.view_synth_probe(y, mask, missing, 3, 3, 64, 64, 3, 2.7, HT, max_disparity=3, box_radius=2, iterations=0)
    fill = ctx.view_fill(_dev(y), mask, missing, L.ROWMAJOR, 3, 3, 64, 64, 3, max_disparity=3, box_radius=2)
    assert np.array_equal(cpp0.view(np.uint32)[live], _bits(fill.out)[live])


@pytest.mark.gpu
def test_rejected_calls(ctx):
    import torch
    lf = _data("uniform", 2, 2, 40, 66, 3, seed=1)
    mask, missing = np.ones(4, np.uint32), _missing(4, [3])
    d = _dev(lf)
    out = torch.zeros_like(d)
    disp = torch.zeros((4, 40 * 66), dtype=torch.int8, device="cuda")
    P = core.make_params(0.0, 2.7, *HT)
    fill = (L.ROWMAJOR, 2, 2, 66, 40, 3)
    loop = (P, L.ROWMAJOR, 2, 2, 1, 66, 40, 3)
    with pytest.raises(L.LfBm5dError, match="overlap"):
        ctx.view_fill(d, mask, missing, *fill, out=d)
    with pytest.raises(L.LfBm5dError, match="overlap"):
        ctx.view_synth(d, mask, missing, *loop, out=d)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.view_fill(d, mask, missing, L.ROWMAJOR, 2, 2, 99, 40, 2, out=out, disparity_out=disp)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.view_synth(d, mask, missing, P, L.ROWMAJOR, 2, 2, 1, 99, 40, 2, out=out)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.view_fill(d, mask, missing, L.ROWMAJOR, 2, 2, 1, 40 * 66, 3, out=out, disparity_out=disp)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.view_synth(d, mask, missing, P, L.ROWMAJOR, 2, 2, 1, 40 * 66, 1, 3, out=out)
    for kw, word in ((dict(max_disparity=9), "max_disparity"), (dict(box_radius=8), "box_radius"), (dict(ang_radius=0), "ang_radius"),
                     (dict(ang_radius=3), "ang_radius")):
        with pytest.raises(L.LfBm5dError, match=word):
            ctx.view_fill(d, mask, missing, *fill, out=out, disparity_out=disp, **kw)
        with pytest.raises(L.LfBm5dError, match=word):
            ctx.view_synth(d, mask, missing, *loop, out=out, disparity_out=disp, **kw)
    with pytest.raises(L.LfBm5dError, match="ang_major"):
        ctx.view_fill(d, mask, missing, 0, 2, 2, 66, 40, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="masked empty"):
        ctx.view_fill(d, np.array([1, 1, 1, 0], np.uint32), missing, *fill, out=out, disparity_out=disp)
    with pytest.raises(L.LfBm5dError, match="no SAI is marked missing"):
        ctx.view_fill(d, mask, np.zeros(4, np.uint32), *fill, out=out, disparity_out=disp)
    with pytest.raises(L.LfBm5dError, match="no SAI is marked missing"):
        ctx.view_synth(d, mask, np.zeros(4, np.uint32), *loop, out=out, disparity_out=disp)
    for kw, word in ((dict(sigma_start=3.0, sigma_end=4.0), "sigma_end"), (dict(sigma_end=0.0), "positive"), (dict(sigma_start=-1.0), "positive"),
                     (dict(sigma_noise=-1.0), "sigma_noise"), (dict(sigma_noise=float("nan")), "sigma_noise"), (dict(iterations=1001), "iterations")):
        with pytest.raises(L.LfBm5dError, match=word):
            ctx.view_synth(d, mask, missing, *loop, out=out, **dict(dict(iterations=2), **kw))
    assert not out.any().item() and not disp.any().item()                        # nothing was written by a rejected call
    lib, h = core.lib(), ctx._h
    up = C.POINTER(C.c_uint)
    mp, sp = mask.ctypes.data_as(up), missing.ctypes.data_as(up)
    vp, res = L.view_params(), core.ViewResultStruct()
    p, q = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    for args in ((None, p, mp, sp, q), (C.byref(vp), None, mp, sp, q), (C.byref(vp), p, None, sp, q), (C.byref(vp), p, mp, None, q),
                 (C.byref(vp), p, mp, sp, None)):
        assert lib.lfbm5d_view_fill_device(h, *args, None, *fill, C.byref(res)) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    ltail = (L.ROWMAJOR, 2, 2, 1, 66, 40, 3)
    for args in ((None, C.byref(P), p, mp, sp, q), (C.byref(vp), None, p, mp, sp, q), (C.byref(vp), C.byref(P), None, mp, sp, q),
                 (C.byref(vp), C.byref(P), p, None, sp, q), (C.byref(vp), C.byref(P), p, mp, None, q), (C.byref(vp), C.byref(P), p, mp, sp, None)):
        assert lib.lfbm5d_view_device(h, *args, None, *ltail, C.byref(res)) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    ptrs = (C.c_void_p * 4)()                                                    # non-empty SAIs without a pointer
    assert lib.lfbm5d_view_host_sai(h, C.byref(vp), C.byref(P), ptrs, mp, sp, ptrs, None, *ltail, C.byref(res)) == 1
    assert "NULL" in lib.lfbm5d_last_error(h).decode()
    assert not out.any().item()
    assert lib.lfbm5d_view_fill_device(h, C.byref(vp), p, mp, sp, q, None, *fill, None) == 0   # disparities and result are optional
    assert out[3].any().item() and not out[:3].any().item()
    sharded = L.Context(0)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.view_fill(d, mask, missing, *fill, out=torch.zeros_like(d))
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.view_synth(d, mask, missing, *loop, out=torch.zeros_like(d))
    finally:
        sharded.close()


def _write_crop(tmp):
    """The golden light field's rows and columns 96..159 as 3 x 3 files of 64 x 64."""
    from PIL import Image
    lf = np.load(GOLDEN)[:, :, 96:160, 96:160]
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src


def _args(cli, tmp, src, aw=3, ah=3):
    if cli == CLI3:
        return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "16", "8", "3", "8", "3",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


def _view_line(stdout):
    m = re.search(r"View synthesis: (\d+) of (\d+) SAIs missing, (\d+) left; disparities (-?\d+)\.\.(-?\d+), (\d+) refinement steps", stdout)
    assert m, stdout[-2000:]
    return tuple(int(g) for g in m.groups())


def _shape_of(stdout):
    """stdout with every number and progress line taken out: what stays the same from run to run."""
    lines = [l for l in stdout.replace("\r", "\n").split("\n") if "View synthesis" not in l]
    return re.sub(r"\n+", "\n", re.sub(r"[0-9.eE+-]+", "#", "\n".join(lines)))


@pytest.mark.gpu
def test_cli_reconstructs_the_missing_sais(tmp_path):
    from PIL import Image
    tmp = str(tmp_path)
    src = _write_crop(tmp)
    env = dict(os.environ, LFBM5D_SEED="1")
    plain = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=env)
    assert plain.returncode == 0 and "View synthesis" not in plain.stdout
    files = sorted(os.listdir(f"{tmp}/denoised"))
    before = {d: {f: open(f"{tmp}/{d}/{f}", "rb").read() for f in files} for d in ("noisy",)}
    out = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING="2_2,1_3", LFBM5D_MISSING_ITER="1"))
    assert out.returncode == 0, out.stdout[-2000:]
    n, A, left, dmin, dmax, K = _view_line(out.stdout)
    print(f"LFBM5D_MISSING=2_2,1_3 LFBM5D_MISSING_ITER=1: {n} of {A} missing, {left} left, disparities {dmin}..{dmax}, {K} steps")
    assert (n, A, left, K) == (2, 9, 0, 1) and -8 <= dmin <= 0 <= dmax <= 8
    assert _shape_of(out.stdout) == _shape_of(plain.stdout)                      # nothing else is printed
    for f in files:                                                             # the noisy files of the sound SAIs are the plain run's
        same = open(f"{tmp}/noisy/{f}", "rb").read() == before["noisy"][f]
        assert same == (f not in ("SAI_02_02.png", "SAI_01_03.png")), f
    assert not np.asarray(Image.open(f"{tmp}/noisy/SAI_02_02.png")).any()        # dropped
    rec = np.asarray(Image.open(f"{tmp}/denoised/SAI_02_02.png")).astype(np.float64)
    true = np.asarray(Image.open(f"{src}/SAI_02_02.png")).astype(np.float64)
    psnr = 10.0 * np.log10(255.0 ** 2 / ((rec - true) ** 2).mean())
    print(f"reconstructed and denoised SAI_02_02: {psnr:.2f} dB")
    assert psnr > 20.0                                                          # a black or noisy SAI is below 15 dB
    txt = open(f"{tmp}/measures.txt").read()
    assert "No SAI" not in txt.split("PSNR for all denoised SAIs:")[-1].split("RMSE")[0]   # the PSNR block shows the reconstructed SAIs
    # without a ground truth the files of the missing SAIs need not exist
    tmp2 = os.path.join(tmp, "loaded")
    os.makedirs(tmp2)
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp2, d))
    for f in files:                                                             # the plain run's noisy files, without SAI_02_02
        if f != "SAI_02_02.png":
            open(f"{tmp2}/noisy/{f}", "wb").write(before["noisy"][f])
    r = subprocess.run(_args(CLI, tmp2, "none"), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING="2_2", LFBM5D_SIGMA="auto"))
    assert r.returncode == 0, r.stdout[-2000:]
    assert _view_line(r.stdout)[:3] == (1, 9, 0) and os.path.exists(f"{tmp2}/denoised/SAI_02_02.png")
    assert r.stdout.index("View synthesis:") < r.stdout.index("Estimated noise level:")
    r = subprocess.run(_args(CLI, tmp2, "none"), capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "SAI_02_02.png not found" in r.stdout
    # LFBM5D_SIGMA=poisson and LFBM3Ddenoising run the synthesis alone and say so
    pois = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING="2_2", LFBM5D_MISSING_ITER="2", LFBM5D_SIGMA="poisson"))
    assert pois.returncode == 0, pois.stdout[-2000:]
    assert _view_line(pois.stdout)[5] == 0 and "the synthesis alone" in pois.stdout
    out3 = subprocess.run(_args(CLI3, tmp, src, 2, 2), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING="1_2"))
    assert out3.returncode == 0, out3.stdout[-2000:]
    assert _view_line(out3.stdout)[:3] == (1, 4, 0) and _view_line(out3.stdout)[5] == 0 and "the synthesis alone" in out3.stdout
    # rejected: together with LFBM5D_DEFECTS, malformed lists, SAIs outside the light field
    r = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING="2_2", LFBM5D_DEFECTS=tmp))
    assert r.returncode != 0 and "cannot be combined with LFBM5D_DEFECTS" in r.stdout and "Read input image" not in r.stdout
    for bad in ("", "2", "2_2,", "4_1", "0_1", "a_b", "2-2", " 2_2"):
        r = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING=bad))
        assert r.returncode != 0 and "LFBM5D_MISSING must be" in r.stdout and "Read input image" not in r.stdout, bad
    for bad in ("x", "-1", "", "1.5"):
        r = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_MISSING="2_2", LFBM5D_MISSING_ITER=bad))
        assert r.returncode != 0 and "LFBM5D_MISSING_ITER must be" in r.stdout, bad
