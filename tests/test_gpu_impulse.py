"""GPU tests of the impulse repair (lfbm5d_impulse_*, include/lfbm5d.h): histogram, scale, thresholds, output, flag plane and counts equal
the numpy model (tests/impulse_model.py) bit for bit at every tile edge; planted impulses; empty SAIs; given flags; rejected calls;
determinism of the device and host forms; what the repair is worth in front of the blind sigma and the filter; the CLIs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import impulse_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
OUT_SENTINEL, FLAG_SENTINEL = -7.0, 9


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _damaged_lf(A, C_, H, W, masked=None, sigma=10.0, p=0.02):
    """Golden crop (or the synthetic light field where it does not fit) + Gaussian noise + impulses, a NaN and an inf."""
    if A <= 9 and H <= 200 and W <= 200:
        u8 = np.load(GOLDEN)[:A, :C_, 40:40 + H, 30:30 + W]
    else:
        u8 = synth.make_lf(2, (A + 1) // 2, H, W)[:A, :C_]
    lf = np.ascontiguousarray(u8, np.float32).reshape(A, -1)
    lf = (lf + np.random.default_rng(3).normal(0.0, sigma, lf.shape)).astype(np.float32)
    lf, _ = synth.add_impulse(lf, p, seed=5)
    lf[0, 0] = 255.0
    lf[-1, -1] = np.nan
    if lf.shape[1] > 8:
        lf[0, lf.shape[1] // 2] = np.inf
    mask = np.ones(A, np.uint32)
    if masked is not None:
        mask[masked] = 0
        lf[masked] = np.nan                          # never read
    return lf, mask


def _assert_equals_model(ctx, lf, mask, W, H, C_, **kw):
    """One detect-and-repair call against the model: every output, with sentinels in what must not be written."""
    import torch
    A = len(mask)
    out0 = np.full(lf.shape, OUT_SENTINEL, np.float32)
    code0 = np.full(lf.shape, FLAG_SENTINEL, np.uint8)
    want = M.repair(lf, mask, W, H, C_, out=out0, codes=code0, **kw)
    d = _dev(lf)
    out, fl = _dev(out0), _dev(code0)
    got = ctx.impulse_repair(d, mask, W, H, C_, out=out, flags_out=fl, **kw)
    assert np.array_equal(_bits(d), lf.view(np.uint32))                         # the input is only read
    if want["hist"] is not None:
        hist, pixels, skipped = ctx.impulse_histogram(d, mask, W, H, C_)
        assert np.array_equal(hist, want["hist"]) and (pixels, skipped) == (want["pixels"], want["skipped"])
        assert int(hist.sum()) == pixels - skipped
    assert (got.pixels, got.skipped) == (want["pixels"], want["skipped"])
    assert got.scale == want["scale"] and list(got.scale_channel) == list(want["scale_channel"])
    assert np.array_equal(np.array(got.threshold, np.float32), want["threshold"])
    assert np.array_equal(fl.cpu().numpy(), want["flags"])
    assert np.array_equal(_bits(out), want["out"].view(np.uint32))
    assert np.array_equal(got.counts_sai, want["counts_sai"])
    for name in ("flagged", "repaired", "left"):
        assert list(getattr(got, name)) == list(want[name]), name
    assert got.out is out and got.flags is fl
    return got, want


# tiles are 64 x 32: widths and heights on both sides of a tile edge, several tiles, the smallest plane, an empty SAI
@pytest.mark.gpu
@pytest.mark.parametrize("A,C_,H,W,masked", [(9, 3, 37, 70, 4), (2, 1, 2, 2, None), (4, 1, 65, 63, None), (4, 1, 65, 64, None),
                                             (4, 1, 65, 65, None), (4, 1, 65, 257, None)])
def test_equals_the_model(ctx, A, C_, H, W, masked):
    lf, mask = _damaged_lf(A, C_, H, W, masked)
    got, want = _assert_equals_model(ctx, lf, mask, W, H, C_)
    print(f"{A} x {C_} x {H} x {W}: thresholds {got.threshold}, flagged {got.flagged}, left {got.left}, skipped {got.skipped}")
    assert sum(got.flagged) > 0 and got.skipped > 0
    if masked is not None:                                                     # empty SAI: out and flags keep their sentinels
        assert (got.out[masked] == OUT_SENTINEL).all() and (got.flags[masked] == FLAG_SENTINEL).all()
        assert (got.counts_sai[masked] == 0).all()


@pytest.mark.gpu
def test_other_parameters_equal_the_model(ctx):
    lf, mask = _damaged_lf(4, 3, 40, 66)
    _assert_equals_model(ctx, lf, mask, 66, 40, 3, k=4.0)
    _assert_equals_model(ctx, lf, mask, 66, 40, 3, k=0.5, min_threshold=90.0)
    _assert_equals_model(ctx, lf, mask, 66, 40, 3, threshold=[60.0, 0.0, 80.0])     # one channel still takes k x scale
    got, want = _assert_equals_model(ctx, lf, mask, 66, 40, 3, threshold=[60.0, 70.0, 80.0])
    assert want["hist"] is None and got.scale == 0.0 and got.skipped == 0            # every threshold given: no statistics pass


def _planted():
    """One 70 x 130 plane (3 x 3 tiles of 64 x 32), low noise, with impulses where the code can go wrong; returns (plane, planted mask)."""
    H, W = 70, 130
    I = (120.0 + np.random.default_rng(11).normal(0.0, 2.0, (H, W))).astype(np.float32)
    hit = np.zeros((H, W), bool)

    def put(y, x, v):
        I[y, x] = v
        hit[y, x] = True

    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):               # corners
        put(y, x, 255.0)
    for y, x in ((0, 40), (H - 1, 50), (20, 0), (45, W - 1)):                    # edges
        put(y, x, 0.0)
    for x in (63, 64):                                                           # same-valued pairs across the tile columns 63|64, 64|65
        put(10, x, 255.0); put(10, x + 1, 255.0)                                 # horizontal (10, 63..65 in all)
        put(14 + x - 63, x, 0.0); put(15 + x - 63, x + 1, 0.0)                   # diagonal
    for i, x in enumerate((63, 64, 65)):
        put(50 + 4 * i, x, 0.0); put(51 + 4 * i, x, 0.0)                         # vertical pairs on the columns next to the edges
    for i, y in enumerate((31, 32, 63, 64)):                                     # ... and across the tile rows 31|32, 32|33, 63|64, 64|65
        put(y, 20, 255.0); put(y + 1, 20, 255.0)                                 # vertical (runs of three in all)
        put(y, 100 + 4 * i, 0.0); put(y + 1, 101 + 4 * i, 0.0)                   # diagonal
        put(y, 40 + 4 * i, 255.0); put(y, 41 + 4 * i, 255.0)                     # horizontal, on the rows next to the edges
    put(25, 30, np.nan)                                                          # a NaN centre
    put(25, 90, np.inf)                                                          # an inf centre
    put(40, 10, np.nan)                                                          # a NaN next to a sound pixel (40, 11) ...
    put(5, 110, np.nan); put(5, 111, 255.0)                                      # ... and next to an impulse
    return I, hit


@pytest.mark.gpu
def test_planted_cases(ctx):
    I, hit = _planted()
    H, W = I.shape
    lf = np.stack([I.reshape(-1), I[::-1].reshape(-1)])                          # two SAIs: the plane and its vertical flip
    mask = np.ones(2, np.uint32)
    got, want = _assert_equals_model(ctx, lf, mask, W, H, 1)
    flags = got.flags.cpu().numpy().reshape(2, H, W)
    out = got.out.cpu().numpy().reshape(2, H, W)
    assert (flags[0][hit] == 1).all() and (flags[1][hit[::-1]] == 1).all()       # every planted value is found and repaired
    assert np.isfinite(out).all()
    assert (np.abs(out[0][hit] - 120.0) < 10.0).all()                            # ... by a sound neighbour's value
    assert flags[0][40, 11] == 0 and out[0][40, 11] == I[40, 11]                 # the sound pixel next to a NaN stays
    false_pos = int((flags[0] != 0).sum()) - int(hit.sum())
    assert 0 <= false_pos <= 0.01 * hit.size
    assert got.left == (0,) and got.skipped == 2 * 4                             # R is infinite at the four non-finite centres only


@pytest.mark.gpu
def test_given_flags(ctx):
    lf, mask = _damaged_lf(4, 3, 40, 66, masked=2, p=0.0)
    given = (np.random.default_rng(2).random(lf.shape) < 0.05).astype(np.uint8) * 3   # non-zero = defective
    g = given.reshape(4, 3, 40, 66)
    g[1, 1, 9:12, 62:65] = 1                                                     # a fully flagged 3 x 3 over the tile column 63|64
    g[1, 1, 7:14, 60:67][g[1, 1, 7:14, 60:67] == 3] = 0                          # ... whose surroundings are sound
    g[3, 0, 0:2, 0:2] = 1                                                        # ... and one in a corner: (0, 0)'s neighbours are all flagged
    g[3, 0, 0:3, 0:3][g[3, 0, 0:3, 0:3] == 3] = 0
    out0 = np.full(lf.shape, OUT_SENTINEL, np.float32)
    code0 = np.full(lf.shape, FLAG_SENTINEL, np.uint8)
    want = M.repair(lf, mask, 66, 40, 3, flags=given, out=out0, codes=code0)
    out, fl = _dev(out0), _dev(code0)
    got = ctx.impulse_repair(_dev(lf), mask, 66, 40, 3, flags=_dev(given), out=out, flags_out=fl)
    assert np.array_equal(_bits(out), want["out"].view(np.uint32)) and np.array_equal(fl.cpu().numpy(), want["flags"])
    assert np.array_equal(got.counts_sai, want["counts_sai"]) and got.threshold == (0.0, 0.0, 0.0) and got.scale == 0.0
    codes = fl.cpu().numpy().reshape(4, 3, 40, 66)
    o, x = out.cpu().numpy().reshape(4, 3, 40, 66), lf.reshape(4, 3, 40, 66)
    assert codes[1, 1, 10, 63] == 2 and o[1, 1, 10, 63] == x[1, 1, 10, 63]       # the centre has no sound neighbour: left
    ring = np.ones((3, 3), bool)
    ring[1, 1] = False
    assert (codes[1, 1, 9:12, 62:65][ring] == 1).all()                           # the ring is repaired from outside
    assert codes[3, 0, 0, 0] == 2 and (codes[3, 0, 0:2, 0:2].reshape(-1)[1:] == 1).all()
    assert np.array_equal(codes[mask != 0] != 0, g[mask != 0] != 0)               # exactly the given flags, and nothing detected
    assert sum(got.left) == 2
    # the host form with given flags
    h = ctx.impulse_repair(lf.copy(), mask, 66, 40, 3, flags=given, return_flags=True)
    live = mask != 0
    assert np.array_equal(h.out.view(np.uint32)[live], want["out"].view(np.uint32)[live]) and np.array_equal(h.flags[live], want["flags"][live])
    assert np.array_equal(h.out.view(np.uint32)[2], lf.view(np.uint32)[2])       # a fresh host result carries the empty SAI's input


@pytest.mark.gpu
def test_a_huge_threshold_detects_nothing(ctx):
    lf, mask = _damaged_lf(4, 3, 40, 66)
    lf[~np.isfinite(lf)] = 0.0
    got = ctx.impulse_repair(_dev(lf), mask, 66, 40, 3, threshold=1e9, return_flags=True)
    assert np.array_equal(_bits(got.out), lf.view(np.uint32))
    assert not got.flags.any().item() and got.flagged == (0, 0, 0) and not got.counts_sai.any()
    assert got.threshold == (1e9, 1e9, 1e9)


@pytest.mark.gpu
def test_rejected_calls(ctx):
    import torch
    lf, mask = _damaged_lf(4, 3, 40, 66)
    d = _dev(lf)
    out = torch.zeros_like(d)
    with pytest.raises(L.LfBm5dError, match="alias"):
        ctx.impulse_repair(d, mask, 66, 40, 3, out=d)
    fl = torch.zeros(d.shape, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.LfBm5dError, match="alias"):
        ctx.impulse_repair(d, mask, 66, 40, 3, flags=fl, out=out, flags_out=fl)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.impulse_repair(d, mask, 66 * 3 // 2, 40, 2, out=out)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.impulse_repair(d, mask, 1, 40 * 66, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.impulse_histogram(d, mask, 40 * 66, 1, 3)
    with pytest.raises(L.LfBm5dError, match="non-empty"):
        ctx.impulse_repair(d, np.zeros(4, np.uint32), 66, 40, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="non-empty"):
        ctx.impulse_histogram(d, np.zeros(4, np.uint32), 66, 40, 3)
    for kw in (dict(k=-1.0), dict(k=float("nan")), dict(min_threshold=-1.0), dict(threshold=float("inf"))):
        with pytest.raises(L.LfBm5dError, match="finite"):
            ctx.impulse_repair(d, mask, 66, 40, 3, out=out, **kw)
    assert not out.any().item()                                                  # nothing was written by a rejected call
    lib, h = core.lib(), ctx._h
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint))
    P, res = L.impulse_params(), core.ImpulseResultStruct()
    p, q = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.lfbm5d_impulse_repair_device(h, C.byref(P), p, mp, p, None, 4, 66, 40, 3, C.byref(res), None) == 1
    assert "alias" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_impulse_repair_device(h, None, p, mp, q, None, 4, 66, 40, 3, C.byref(res), None) == 1
    assert lib.lfbm5d_impulse_repair_device(h, C.byref(P), None, mp, q, None, 4, 66, 40, 3, C.byref(res), None) == 1
    assert lib.lfbm5d_impulse_repair_device(h, C.byref(P), p, None, q, None, 4, 66, 40, 3, C.byref(res), None) == 1
    assert lib.lfbm5d_impulse_repair_flags_device(h, p, None, mp, q, None, 4, 66, 40, 3, C.byref(res), None) == 1
    assert lib.lfbm5d_impulse_repair_host_sai(h, C.byref(P), (C.c_void_p * 4)(), None, mp, (C.c_void_p * 4)(), None, 4, 66, 40, 3, C.byref(res), None) == 1
    assert "NULL" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_impulse_histogram_device(h, p, mp, 4, 66, 40, 3, None, None, None) == 1
    assert lib.lfbm5d_impulse_repair_device(h, C.byref(P), p, mp, q, None, 4, 66, 40, 3, None, None) == 0   # result and counts are optional
    sharded = L.Context(0)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.impulse_repair(d, mask, 66, 40, 3, out=out)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.impulse_histogram(d, mask, 66, 40, 3)
    finally:
        sharded.close()


@pytest.mark.gpu
def test_determinism_and_the_host_forms(ctx):
    lf, mask = _damaged_lf(9, 3, 37, 70, masked=4)
    d = _dev(lf)
    a = ctx.impulse_repair(d, mask, 70, 37, 3, return_flags=True)
    b = ctx.impulse_repair(d, mask, 70, 37, 3, return_flags=True)
    live = mask != 0
    for x, y in ((a, b),):
        assert np.array_equal(_bits(x.out), _bits(y.out)) and torch_equal(x.flags, y.flags)
        assert x[2:10] == y[2:10] and np.array_equal(x.counts_sai, y.counts_sai)
    assert np.array_equal(_bits(a.out)[4], lf.view(np.uint32)[4])                # a fresh device result carries the empty SAI's input
    h = ctx.impulse_repair(lf.copy(), mask, 70, 37, 3, return_flags=True)        # flat host array
    assert isinstance(h.out, np.ndarray) and h.out.shape == lf.shape
    assert np.array_equal(h.out.view(np.uint32)[live], _bits(a.out)[live]) and np.array_equal(h.flags[live], a.flags.cpu().numpy()[live])
    assert h[2:10] == a[2:10] and np.array_equal(h.counts_sai, a.counts_sai)
    sais = [lf[i].copy() if mask[i] else None for i in range(9)]                 # one array per SAI, NULL for the empty one
    outs = [np.zeros(lf.shape[1], np.float32) if mask[i] else None for i in range(9)]
    l = L.impulse_repair(sais, mask, 70, 37, 3, ctx=ctx, out=outs)
    assert all(np.array_equal(outs[i].view(np.uint32), _bits(a.out)[i]) for i in range(9) if mask[i])
    assert l[2:10] == a[2:10] and l.flags is None


def torch_equal(x, y):
    import torch
    return bool(torch.equal(x, y))


P1 = lambda sigma: core.make_params(sigma, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")     # the README parameters
P2 = lambda sigma: core.make_params(sigma, 2.7, 16, 18, 6, 8, 4, "dct", "sadct", "haar")
TAIL = (L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)


def _psnr(x, clean):
    return float(10.0 * np.log10(255.0 ** 2 / ((x.astype(np.float64) - clean) ** 2).mean()))


@pytest.mark.gpu
def test_repair_ahead_of_the_blind_sigma_and_the_filter(ctx):
    """3x3x64x64 golden crop, sigma = 10 (default_rng(7)), 0.5 % salt and pepper (add_impulse seed 7), README parameters.  A: blind sigma
    + denoise on the damaged light field; B: repair first.  Measured on an MI355X (profiles/impulse.txt): blind sigma 10.148 undamaged,
    13.809 (A), 10.141 (B); PSNR 36.420 dB (A), 40.228 dB (B), gain 3.81 dB; the undamaged noisy light field denoises to 40.469 dB."""
    import torch
    clean = np.ascontiguousarray(np.load(GOLDEN)[:, :, :64, :64], np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    z = (clean + np.random.default_rng(7).normal(0.0, 10.0, clean.shape)).astype(np.float32)
    damaged, hit = synth.add_impulse(z, 0.005, seed=7)
    s0 = ctx.noise_level(_dev(z), mask, 64, 64, 3).sigma

    def run(noisy):
        s = ctx.noise_level(noisy, mask, 64, 64, 3).sigma
        basic, den = torch.zeros_like(noisy), torch.zeros_like(noisy)
        ctx.denoise(P1(s), P2(s), noisy.clone(), mask, basic, den, *TAIL)
        return s, _psnr(den.cpu().numpy(), clean)

    sA, pA = run(_dev(damaged))
    rep = ctx.impulse_repair(_dev(damaged), mask, 64, 64, 3)
    sB, pB = run(rep.out)
    print(f"end to end: sigma undamaged {s0:.4f}, A (damaged) {sA:.4f}, B (repaired) {sB:.4f}; PSNR A {pA:.4f} dB, B {pB:.4f} dB, "
          f"gain {pB - pA:.4f} dB; flagged {sum(rep.flagged)} of {int(hit.sum())} hits, thresholds {rep.threshold}")
    assert abs(sB / s0 - 1.0) <= 0.10
    assert abs(sA / s0 - 1.0) > 0.10
    assert pB > pA
    assert pB - pA >= GAIN_FLOOR_DB


GAIN_FLOOR_DB = 1.9   # half the gain measured on an MI355X: 3.8075 dB (profiles/impulse.txt, tools/impulse_time.py endtoend)


def _write_source_lf(tmp):
    from PIL import Image
    lf = np.load(GOLDEN)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
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


def _repair_line(stdout):
    m = re.search(r"Impulse repair: (\d+) of (\d+) values flagged \(([0-9.eE+-]+) %\), (\d+) left; thresholds ([0-9.eE+-]+) ([0-9.eE+-]+) ([0-9.eE+-]+)",
                  stdout)
    assert m, stdout[-2000:]
    return int(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4)), [float(m.group(i)) for i in (5, 6, 7)]


def _psnrs(tmp):
    txt = open(f"{tmp}/measures.txt").read()
    return {k: float(txt.split(f"-> Average PSNR {k} = ")[1].split()[0]) for k in ("noisy", "basic", "denoised")}


@pytest.mark.gpu
def test_cli_repairs_the_impulses_it_adds(tmp_path):
    """sigma = 25 and 0.5 % salt and pepper on the golden 3 x 3 files: about 8850 impulses in 1769472 values.  At this sigma an impulse
    on a mid-grey pixel has R of about 4 x 125 against a threshold of 8 x 51, so a large part hides in the noise: the band asks for at
    least a quarter of the impulses and at most all of them plus 0.2 % of false positives (measured: 4522 flagged, 0.256 %)."""
    tmp = str(tmp_path)
    src = _write_source_lf(tmp)
    env = dict(os.environ, LFBM5D_SEED="1", LFBM5D_IMPULSE="auto", LFBM5D_IMPULSE_ADD="0.005")
    out = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:]
    n, N, pct, left, T = _repair_line(out.stdout)
    vals = _psnrs(tmp)
    print(f"LFBM5D_IMPULSE=auto LFBM5D_IMPULSE_ADD=0.005: {n} of {N} flagged ({pct} %), {left} left, thresholds {T}, PSNR {vals}")
    assert N == 9 * 3 * 256 * 256 and 0.00125 * N <= n <= 0.007 * N and abs(pct - 100.0 * n / N) < 1e-3
    assert "values replaced by 0 or 255" in out.stdout
    assert all(t > 0 for t in T)
    assert vals["denoised"] > vals["basic"] > vals["noisy"]
    assert os.path.exists(f"{tmp}/denoised/SAI_02_02.png")
    # LFBM3Ddenoising, with a factor of its own and the blind sigma behind the repair
    tmp3 = os.path.join(tmp, "bm3d")
    os.makedirs(tmp3)
    src3 = _write_source_lf(tmp3)
    env3 = dict(env, LFBM5D_IMPULSE="6", LFBM5D_SIGMA="auto")
    out = subprocess.run(_readme_args(CLI3, tmp3, src3), capture_output=True, text=True, env=env3)
    assert out.returncode == 0, out.stdout[-2000:]
    n3, N3, _, _, T3 = _repair_line(out.stdout)
    assert N3 == 4 * 3 * 256 * 256 and 0.00125 * N3 <= n3 <= 0.007 * N3
    assert out.stdout.index("Impulse repair:") < out.stdout.index("Estimated noise level:")
    est = float(out.stdout.split("Estimated noise level: sigma = ")[1].split()[0])
    print(f"LFBM3Ddenoising LFBM5D_IMPULSE=6 LFBM5D_SIGMA=auto: {n3} of {N3} flagged, thresholds {T3}, estimated sigma {est}")
    assert abs(est - 25.0) <= 2.5
    # a bad value ends the command with the message
    bad = subprocess.run(_readme_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_IMPULSE="bogus"))
    assert bad.returncode != 0 and "LFBM5D_IMPULSE must be" in bad.stdout
