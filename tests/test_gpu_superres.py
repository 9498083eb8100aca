"""GPU tests of the light-field super-resolution (lfbm5d_sr_* / lfbm5d_superres_*, include/lfbm5d.h): the resampling kernels against
the float64 model (tests/sr_model.py), the fused back-projection, the loop against the same loop written out by hand (bits) and
against the CPU composition of the model with the checker's run_step1 (PSNR), the host forms, the C++ drop-in and the CLI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
from oracle import oracle as O
import sr_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Dsuperres")
U24 = 2.0 ** -24
SENTINEL = -777.0
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")      # N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D of the CPU model's table (profiles/sr_parity.txt)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lib_ops(sr, w, h):
    """The model with the library's own float32 tables: only the accumulation differs from the kernels."""
    taps = dict(ux=L.sr_taps("up", sr, w), uy=L.sr_taps("up", sr, h), dx=L.sr_taps("down", sr, w * sr.scale), dy=L.sr_taps("down", sr, h * sr.scale))
    return M.Ops(sr.scale, sr.kernel, sr.blur_sigma, w, h, taps=taps), taps


def _bound(tabs, peak):
    """2 (T+1) 2^-24 (sum |w|)^2 max |in|: two passes of T fused multiply-adds each, T and sum |w| the larger of the two tables'."""
    T = max(t[1].shape[1] for t in tabs)
    S = max(float(np.abs(t[1].astype(np.float64)).sum(1).max()) for t in tabs)
    return 2.0 * (T + 1) * U24 * S * S * peak


# (angular size, mask, C, low w, low h): 1x2 SAIs odd sizes; 3x3 with SAI 1 empty, high-resolution width 140 / 210 / 280 across workgroup
# tiles of 64 columns; 32 x 32 (high-resolution heights across tiles of 16 rows)
SHAPES = {"1x2_c3_13x9": (2, None, 3, 13, 9), "3x3_hole_c1_70x5": (9, 1, 1, 70, 5), "1x1_c1_32x32": (1, None, 1, 32, 32)}


def _shape(name, seed=0):
    A, hole, Cc, w, h = SHAPES[name]
    mask = np.ones(A, np.uint32)
    if hole is not None:
        mask[hole] = 0
    return A, mask, Cc, w, h, np.random.default_rng(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["bicubic", "gaussian"])
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_operators_against_the_model(ctx, shape, s, kernel):
    import torch
    A, mask, Cc, w, h, rng = _shape(shape)
    W, H = w * s, h * s
    sr = L.sr_defaults(s, kernel=kernel, blur_sigma=0.4 * s)
    ops, taps = _lib_ops(sr, w, h)
    low = rng.uniform(0.0, 255.0, (A, Cc, h, w)).astype(np.float32)
    high = rng.uniform(0.0, 255.0, (A, Cc, H, W)).astype(np.float32)
    low[mask == 0] = np.nan
    high[mask == 0] = np.nan                      # planes of empty SAIs are not read ...
    live = mask != 0
    for name, src, shp, model, tabs in (("up", low, (A, Cc, H, W), ops.up, (taps["ux"], taps["uy"])),
                                        ("down", high, (A, Cc, h, w), ops.down, (taps["dx"], taps["dy"]))):
        out = torch.full((A, int(np.prod(shp[1:]))), SENTINEL, dtype=torch.float32, device="cuda")
        d_src = _dev(src.reshape(A, -1))
        if name == "up":
            ctx.sr_up(sr, d_src, mask, out, w, h, Cc)
        else:
            ctx.sr_down(sr, d_src, mask, out, w, h, Cc)
        g = out.cpu().numpy().reshape(shp)
        assert (g[~live] == SENTINEL).all(), name  # ... nor written
        err = float(np.abs(g[live] - model(src[live])).max())
        bound = _bound(tabs, 255.0)
        print(f"{shape} s={s} {kernel} {name}: max |gpu - model| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
        assert np.array_equal(_bits(d_src)[live], _bits(src.reshape(A, -1))[live])   # inputs are only read


@pytest.mark.gpu
@pytest.mark.parametrize("shape,s,kernel,beta", [("1x2_c3_13x9", 2, "bicubic", 1.0), ("3x3_hole_c1_70x5", 3, "gaussian", 0.5),
                                                 ("3x3_hole_c1_70x5", 4, "bicubic", 0.5), ("1x2_c3_13x9", 4, "gaussian", 1.0),
                                                 ("1x1_c1_32x32", 3, "bicubic", 1.0)])
def test_backproject_equals_the_model_composition(ctx, shape, s, kernel, beta):
    import torch
    A, mask, Cc, w, h, rng = _shape(shape, seed=1)
    W, H = w * s, h * s
    sr = L.sr_defaults(s, kernel=kernel, blur_sigma=0.4 * s, beta=beta)
    ops, taps = _lib_ops(sr, w, h)
    y = rng.uniform(0.0, 255.0, (A, Cc, h, w)).astype(np.float32)
    x = rng.uniform(0.0, 255.0, (A, Cc, H, W)).astype(np.float32)
    live = mask != 0
    d_y, d_x = _dev(y.reshape(A, -1)), _dev(x.reshape(A, -1))
    d_z = torch.full_like(d_x, SENTINEL)
    ctx.sr_backproject(sr, d_y, d_x, mask, d_z, w, h, Cc)
    z = d_z.cpu().numpy().reshape(x.shape)
    assert (z[~live] == SENTINEL).all()
    err = float(np.abs(z[live] - ops.backproject(y[live], x[live], beta)).max())
    bound = 3.0 * _bound(list(taps.values()), 255.0)
    print(f"{shape} s={s} {kernel} beta={beta}: max |gpu - model| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    again = torch.full_like(d_x, SENTINEL)
    ctx.sr_backproject(sr, d_y, d_x, mask, again, w, h, Cc)
    assert np.array_equal(_bits(again), _bits(d_z))                # same bits on a second call
    ctx.sr_backproject(sr, d_y, d_x, mask, d_x, w, h, Cc)          # in place
    assert np.array_equal(_bits(d_x)[live], _bits(d_z)[live])


def _golden_case(s, kernel, sb, n):
    """The table's cases: golden light field, all 9 SAIs, 3 channels, rows and columns 80..80+n; y = the model's D, rounded to float32."""
    hr = np.load(GOLDEN)[:, :, 80:80 + n, 80:80 + n].astype(np.float64)
    ops = M.Ops(s, M.GAUSSIAN if kernel == "gaussian" else M.BICUBIC, sb, n // s, n // s)
    return hr, ops, ops.down(hr).astype(np.float32)


@pytest.mark.gpu
def test_loop_is_bit_identical_to_the_hand_written_loop(ctx):
    import torch
    n, s, K = 64, 2, 2
    _, _, y = _golden_case(s, "bicubic", 0.8, n)
    w = h = n // s
    mask = np.ones(9, np.uint32)
    sr = L.sr_defaults(s, iterations=K, sigma_start=20.0, sigma_end=3.0)
    P = core.make_params(0.0, 2.7, *HT)
    d_y = _dev(y.reshape(9, -1))
    out = torch.zeros((9, 3 * n * n), dtype=torch.float32, device="cuda")
    ctx.superres(sr, P, d_y, mask, out, L.ROWMAJOR, 3, 3, 1, w, h, 3)
    assert np.array_equal(_bits(d_y), _bits(y.reshape(9, -1)))     # the input is only read
    out2 = torch.zeros_like(out)
    ctx.superres(sr, P, d_y, mask, out2, L.ROWMAJOR, 3, 3, 1, w, h, 3)
    assert np.array_equal(_bits(out), _bits(out2))

    x = torch.zeros_like(out)
    ctx.sr_up(sr, d_y, mask, x, w, h, 3)
    for sig in M.sigma_schedule(K, 20.0, 3.0):
        z = torch.zeros_like(out)
        ctx.sr_backproject(sr, d_y, x, mask, z, w, h, 3)
        x = torch.zeros_like(out)
        ctx.step1(core.make_params(sig, 2.7, *HT), z, mask, x, L.ROWMAJOR, 3, 3, 1, n, n, 3)
    ctx.sr_backproject(sr, d_y, x, mask, x, w, h, 3)
    assert np.array_equal(_bits(out), _bits(x))
    sr.close_projection = 0
    ctx.superres(sr, P, d_y, mask, out2, L.ROWMAJOR, 3, 3, 1, w, h, 3)
    assert not np.array_equal(_bits(out), _bits(out2))


# the first three rows of the CPU model's table (profiles/sr_parity.txt): (s, kernel, blur sigma, high-resolution size, K, sigma_start, sigma_end) -> the CPU
# composition's PSNR there (bicubic, back-projection only, loop)
TABLE = {(2, "bicubic", 0.8, 64, 4, 20.0, 3.0): (33.549, 34.473, 35.212),
         (3, "gaussian", 1.2, 66, 4, 24.0, 4.0): (29.077, 31.468, 32.239),
         (4, "gaussian", 1.6, 64, 4, 30.0, 5.0): (26.193, 28.951, 29.843)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TABLE))
def test_loop_against_the_cpu_composition(ctx, case):
    """|PSNR_gpu - PSNR_cpu| <= 0.01 (K+1) dB (the project's +-0.01 dB per step, summed over the loop's K steps), and the loop beats
    K+1 plain back-projections of the same operators by >= 0.5 dB.  Measured on an MI355X: profiles/sr_parity.txt."""
    import torch
    s, kernel, sb, n, K, s0, s1 = case
    hr, ops, y = _golden_case(s, kernel, sb, n)
    w = h = n // s
    mask = np.ones(9, np.uint32)

    def cpu_step(z, sig):
        _, basic, _ = O.run_step1(O.make_params(sig, 2.7, *HT), z.astype(np.float32).reshape(9, -1), mask, L.ROWMAJOR, 3, 3, 1, n, n, 3)
        return basic.reshape(z.shape)
    cpu = M.psnr(M.loop(ops, y, K, s0, s1, cpu_step), hr)
    assert abs(cpu - TABLE[case][2]) < 2e-3, cpu                   # the CPU composition is the one of the table

    sr = L.sr_defaults(s, kernel=kernel, blur_sigma=sb, iterations=K, sigma_start=s0, sigma_end=s1)
    d_y = _dev(y.reshape(9, -1))
    out = torch.zeros((9, 3 * n * n), dtype=torch.float32, device="cuda")
    ctx.superres(sr, core.make_params(0.0, 2.7, *HT), d_y, mask, out, L.ROWMAJOR, 3, 3, 1, w, h, 3)
    gpu = M.psnr(out.cpu().numpy().reshape(hr.shape), hr)
    bp = torch.zeros_like(out)
    ctx.sr_up(sr, d_y, mask, bp, w, h, 3)
    bic = M.psnr(bp.cpu().numpy().reshape(hr.shape), hr)
    for _ in range(K + 1):
        ctx.sr_backproject(sr, d_y, bp, mask, bp, w, h, 3)
    plain = M.psnr(bp.cpu().numpy().reshape(hr.shape), hr)
    print(f"s={s} {kernel} HR {n} K={K}: bicubic {bic:.4f}  back-projection {plain:.4f}  loop gpu {gpu:.4f}  loop cpu {cpu:.4f}  "
          f"gpu-cpu {gpu - cpu:+.4f} (allowed {0.01 * (K + 1):.2f})  gain over back-projection {gpu - plain:.4f}")
    assert abs(bic - TABLE[case][0]) < 2e-3 and abs(plain - TABLE[case][1]) < 2e-3
    assert abs(gpu - cpu) <= 0.01 * (K + 1)
    assert gpu - plain >= 0.5


@pytest.mark.gpu
def test_host_forms_return_the_device_forms_bits(ctx):
    import torch
    n, s, K = 64, 2, 2
    _, _, y = _golden_case(s, "bicubic", 0.8, n)
    w = h = n // s
    y = np.ascontiguousarray(y.reshape(9, -1))
    mask = np.ones(9, np.uint32)
    mask[5] = 0
    sr = L.sr_defaults(s, iterations=K, sigma_start=20.0, sigma_end=3.0)
    P = core.make_params(0.0, 2.7, *HT)
    out = torch.full((9, 3 * n * n), SENTINEL, dtype=torch.float32, device="cuda")
    ctx.superres(sr, P, _dev(y), mask, out, L.ROWMAJOR, 3, 3, 1, w, h, 3)
    dev = out.cpu().numpy()
    live = mask != 0
    assert (dev[5] == SENTINEL).all() and np.isfinite(dev[live]).all()
    flat = np.full_like(dev, SENTINEL)
    ctx.superres(sr, P, y, mask, flat, L.ROWMAJOR, 3, 3, 1, w, h, 3)                               # lfbm5d_superres_host_sai, rows of one array
    assert np.array_equal(flat.view(np.uint32), dev.view(np.uint32))
    per_sai = [np.zeros(3 * n * n, np.float32) if mask[i] else None for i in range(9)]
    L.superres(sr, P, [y[i].copy() if mask[i] else None for i in range(9)], mask, per_sai, L.ROWMAJOR, 3, 3, 1, w, h, 3, ctx=ctx)
    assert all(np.array_equal(per_sai[i].view(np.uint32), dev[i].view(np.uint32)) for i in range(9) if mask[i])
    cpp = core.superres_probe(y, mask, 3, 3, w, h, 3, sr, 2.7, HT)                                 # the C++ drop-in's superres_LF
    assert np.array_equal(cpp[live].view(np.uint32), dev[live].view(np.uint32))


@pytest.mark.gpu
def test_rejected_inputs(ctx):
    import torch
    w = h = 16
    mask = np.ones(9, np.uint32)
    P = core.make_params(0.0, 2.7, *HT)
    d_y = torch.zeros((9, 3 * w * h), dtype=torch.float32, device="cuda")
    d_x = torch.zeros((9, 3 * 16 * w * h), dtype=torch.float32, device="cuda")
    bad = [(dict(scale=5), "scale"), (dict(scale=1), "scale"), (dict(iterations=0), "iterations"), (dict(kernel="gaussian", blur_sigma=6.0), "blur_sigma"),
           (dict(kernel="gaussian", blur_sigma=0.0), "blur_sigma"), (dict(sigma_start=3.0, sigma_end=4.0), "sigma_end"),
           (dict(sigma_end=0.0), "positive"), (dict(sigma_start=-1.0, sigma_end=-2.0), "positive"), (dict(kernel=9), "kernel"), (dict(beta=0.0), "beta")]
    for kw, word in bad:
        with pytest.raises(L.LfBm5dError, match=word):
            ctx.superres(L.sr_defaults(2, **kw), P, d_y, mask, d_x, L.ROWMAJOR, 3, 3, 1, w, h, 3)
    with pytest.raises(L.LfBm5dError, match="scale"):
        ctx.sr_up(L.sr_defaults(2, scale=7), d_y, mask, d_x, w, h, 3)
    with pytest.raises(L.LfBm5dError, match="non-empty"):
        ctx.sr_down(L.sr_defaults(2), d_x, np.zeros(9, np.uint32), d_y, w, h, 3)
    lib, hdl, sr = core.lib(), ctx._h, L.sr_defaults(2)
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint))
    py, px = C.c_void_p(d_y.data_ptr()), C.c_void_p(d_x.data_ptr())
    tail = (L.ROWMAJOR, 3, 3, 1, w, h, 3)
    for args in ((None, C.byref(P), py, mp, px), (C.byref(sr), None, py, mp, px), (C.byref(sr), C.byref(P), None, mp, px),
                 (C.byref(sr), C.byref(P), py, None, px), (C.byref(sr), C.byref(P), py, mp, None)):
        assert lib.lfbm5d_superres_device(hdl, *args, *tail) == 1
        assert "NULL" in lib.lfbm5d_last_error(hdl).decode()
    assert lib.lfbm5d_sr_up_device(hdl, C.byref(sr), None, mp, px, 9, w, h, 3) == 1 and "NULL" in lib.lfbm5d_last_error(hdl).decode()
    assert lib.lfbm5d_sr_down_device(hdl, C.byref(sr), px, mp, None, 9, w, h, 3) == 1 and "NULL" in lib.lfbm5d_last_error(hdl).decode()
    assert lib.lfbm5d_sr_backproject_device(hdl, C.byref(sr), py, None, mp, px, 9, w, h, 3) == 1 and "NULL" in lib.lfbm5d_last_error(hdl).decode()
    ptrs = (C.c_void_p * 9)()                                      # non-empty SAIs without a pointer
    assert lib.lfbm5d_superres_host_sai(hdl, C.byref(sr), C.byref(P), ptrs, mp, ptrs, *tail) == 1
    assert "NULL" in lib.lfbm5d_last_error(hdl).decode()


@pytest.mark.gpu
def test_cli(tmp_path):
    """LFBM5Dsuperres on the model's D of the golden 3x3 crop, rounded to 8 bits: nine PNGs of twice the size, exit status 0, and a
    mean PSNR above plain bicubic interpolation's, on stdout and in the results file."""
    from PIL import Image
    n, s = 64, 2
    hr, _, y = _golden_case(s, "bicubic", 0.8, n)
    low8 = np.clip(np.round(y), 0, 255).astype(np.uint8)
    tmp = str(tmp_path)
    for d in ("low", "src", "out"):
        os.makedirs(os.path.join(tmp, d))
    for i in range(9):
        name = f"SAI_{i // 3 + 1:02d}_{i % 3 + 1:02d}.png"
        Image.fromarray(low8[i].transpose(1, 2, 0)).save(f"{tmp}/low/{name}")
        Image.fromarray(hr[i].astype(np.uint8).transpose(1, 2, 0)).save(f"{tmp}/src/{name}")
    args = [CLI, f"{tmp}/low", "SAI", "_", "3", "3", "1", "1", "1", "row", str(s), "bicubic", "0", "0", "0", "0", f"{tmp}/out",
            "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "opp", f"{tmp}/src", f"{tmp}/measures.txt"]
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    for i in range(9):
        im = Image.open(f"{tmp}/out/SAI_{i // 3 + 1:02d}_{i % 3 + 1:02d}.png")
        assert im.size == (n, n) and im.mode == "RGB"
    bic = float(re.search(r"- Bicubic light field: ([0-9.]+)", out.stdout).group(1))
    res = float(re.search(r"- Super-resolved light field: ([0-9.]+)", out.stdout).group(1))
    print("LFBM5Dsuperres: bicubic", bic, "super-resolved", res)
    assert res > bic
    txt = open(f"{tmp}/measures.txt").read()
    assert abs(float(txt.split("-> Average PSNR bicubic = ")[1].split()[0]) - bic) < 1e-3
    assert abs(float(txt.split("-> Average PSNR super-resolved = ")[1].split()[0]) - res) < 1e-3
    assert subprocess.run(args[:10], capture_output=True, text=True).returncode != 0     # too few arguments
