"""CPU tests of the defect inpainting (lfbm5d_inpaint_*, include/lfbm5d.h): the exports and struct sizes, the invariants of the numpy
model (tests/inpaint_model.py), the synthetic defect map, and what the composition of the model with the checker's run_step1 gains on
the golden crop (profiles/inpaint_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from oracle import oracle as O
import inpaint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")      # N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D: the super-resolution tests' parameters
# the CPU composition on the golden crop (rows and columns 80..143, add_defects seed 3, clean data, K = 4, sigma 30 -> 5), PSNR over
# the flagged values: fill, loop (profiles/inpaint_parity.txt)
CPU_FILL_DB, CPU_LOOP_DB = 25.5188, 35.7081


def test_library_exports_the_inpaint_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_inpaint_defaults", "lfbm5d_inpaint_fill_device", "lfbm5d_inpaint_project_device", "lfbm5d_inpaint_device",
              "lfbm5d_inpaint_host_sai"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.InpaintParamsStruct) == 4 * 4
    assert C.sizeof(core.InpaintResultStruct) == 10 * 8 + 2 * 4
    P = L.inpaint_params()
    assert P.iterations >= 1 and 0.0 < P.sigma_end <= P.sigma_start and P.sigma_noise == 0.0
    P = L.inpaint_params(iterations=0, sigma_start=12.0, sigma_end=3.0, sigma_noise=2.0)
    assert (P.iterations, P.sigma_start, P.sigma_end, P.sigma_noise) == (0, 12.0, 3.0, 2.0)
    hdr = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    assert f"#define LFBM5D_INPAINT_PASSES_PER_LAUNCH {core.INPAINT_PASSES_PER_LAUNCH}" in hdr
    for n in ("inpaint", "inpaint_params", "Inpaint"):
        assert n in L.__all__
    assert np.array_equal(M.RECIP[1:], (1.0 / np.arange(1, 9)).astype(np.float32)) and M.RECIP[3] == np.float32(1.0 / 3.0)


def _plane(H, W, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 255.0, (H, W)).astype(np.float32)


def test_unflagged_values_are_untouched_and_fills_lie_between_their_sources():
    I = _plane(40, 50)
    f = synth.add_defects((1, 1, 40, 40), 5)[0, 0]
    f = np.pad(f, ((0, 0), (0, 10)))
    f[0:3, 0:3] = True                                                         # a corner
    f[37:40, 47:50] = True
    out, code, passes = M.fill_plane(I, f)
    assert np.array_equal(out[~f].view(np.uint32), I[~f].view(np.uint32))
    assert np.array_equal(code != 0, f) and (code[f] == 1).all()
    # every filled value is a mean of values that are sound values or such means: within the extremes of the sound values of its 3 x 3
    # hull grown by the pass count, and with a margin of one rounding per pass; the whole plane's extremes bound all of them
    lo, hi = I[~f].min(), I[~f].max()
    assert (out[f] >= lo * (1 - 1e-6)).all() and (out[f] <= hi * (1 + 1e-6)).all()
    # first ring: exactly the float32 mean of its sound neighbours, inside their min and max
    q, ok = M.neighbours(I), ~M.neighbours(f)
    ring = f & ok.any(axis=0)
    qmin = np.where(ok, q, np.inf).min(axis=0)
    qmax = np.where(ok, q, -np.inf).max(axis=0)
    assert (out[ring] >= qmin[ring] * (1 - 2e-7)).all() and (out[ring] <= qmax[ring] * (1 + 2e-7)).all()
    assert passes == M.chebyshev_depth(f)


@pytest.mark.parametrize("side", [1, 2, 3, 6, 7, 19])
def test_the_pass_count_is_the_chebyshev_depth(side):
    I = _plane(30, 33, seed=side)
    f = np.zeros(I.shape, bool)
    f[5:5 + side, 4:4 + side] = True
    out, code, passes = M.fill_plane(I, f)
    assert passes == (side + 1) // 2 == M.chebyshev_depth(f)
    g = np.zeros(I.shape, bool)
    g[:side, :side] = True                                                     # in a corner the mirror closes two sides: twice as deep
    assert M.fill_plane(I, g)[2] == side == M.chebyshev_depth(g)
    assert np.isfinite(out).all() and (code[f] == 1).all()


def test_a_fully_flagged_plane_is_left_and_a_nan_is_flagged():
    I = _plane(6, 7)
    out, code, passes = M.fill_plane(I, np.ones(I.shape, bool))
    assert passes == 0 and (code == 2).all() and np.array_equal(out, I)
    J = I.copy()
    J[2, 3] = np.nan
    J[4, 0] = np.inf
    out, code, passes = M.fill_plane(J, np.zeros(I.shape, bool))               # not named in the map
    assert code[2, 3] == 1 and code[4, 0] == 1 and int((code != 0).sum()) == 2 and passes == 1
    assert np.isfinite(out).all()
    others = [J[2 + dy, 3 + dx] for dy, dx in M.OFFS]
    s = np.float32(0.0)
    for v in others:
        s = np.float32(s + v)
    assert out[2, 3] == np.float32(s * np.float32(0.125))
    # at the edge the mirrored neighbours count twice: (4, 0) sees (3, 1), (4, 1), (5, 1) twice and (3, 0), (5, 0) once
    s = np.float32(0.0)
    for y, x in ((3, 1), (3, 0), (3, 1), (4, 1), (4, 1), (5, 1), (5, 0), (5, 1)):
        s = np.float32(s + J[y, x])
    assert out[4, 0] == np.float32(s * np.float32(0.125))
    r = M.fill(np.stack([I.reshape(-1), J.reshape(-1)]), np.stack([np.ones(42, np.uint8), np.zeros(42, np.uint8)]), np.ones(2, np.uint32), 7, 6, 1)
    assert list(r["left"]) == [42] and list(r["filled"]) == [2] and list(r["flagged"]) == [44] and r["passes"] == 1
    with pytest.raises(ValueError):
        M.loop(np.stack([I.reshape(-1), J.reshape(-1)]), np.stack([np.ones(42, np.uint8), np.zeros(42, np.uint8)]), np.ones(2, np.uint32),
               7, 6, 1, 1, 30.0, 5.0, lambda z, s: z)


def test_projection_and_schedule():
    x, y = _plane(5, 6, 1), _plane(5, 6, 2)
    y[1, 1] = np.nan
    f = np.zeros((5, 6), np.uint8)
    f[1, 1] = 7
    f[3, 2] = 1
    out = M.project(f, x, y)
    assert out[1, 1] == x[1, 1] and out[3, 2] == x[3, 2] and np.array_equal(out[f == 0], y[f == 0])
    assert M.sigma_schedule(1, 30.0, 5.0) == [30.0] and M.sigma_schedule(0, 30.0, 5.0) == []
    s = M.sigma_schedule(4, 30.0, 5.0)
    assert s[0] == 30.0 and abs(s[-1] - 5.0) < 1e-12 and abs(s[1] / s[0] - s[2] / s[1]) < 1e-12
    assert M.sigma_schedule(4, 30.0, 5.0, 10.0)[-2:] == [10.0, 10.0]


def test_add_defects_is_deterministic():
    a = synth.add_defects((9, 3, 64, 64), 3)
    b = synth.add_defects((9, 3, 64, 64), 3)
    assert a.dtype == bool and a.shape == (9, 3, 64, 64) and np.array_equal(a, b)
    assert np.array_equal(a[:, 0], a[:, 1]) and np.array_equal(a[:, 0], a[:, 2])
    assert not np.array_equal(a, synth.add_defects((9, 3, 64, 64), 4))
    for seed in (1, 2, 3, 4):
        share = synth.add_defects((9, 1, 64, 64), seed).mean()
        assert 0.05 <= share <= 0.07, (seed, share)
    assert abs(a.mean() - 0.0604) < 1e-4
    assert all(a[st, 0].all(axis=0).sum() >= 2 for st in range(9))             # a full-height column pair in every SAI
    with pytest.raises(ValueError):
        synth.add_defects((9, 3, 64, 32), 3)


@pytest.fixture(scope="module")
def composition():
    """The golden crop, add_defects(seed=3), clean data with the flagged values zeroed, K = 4, sigma 30 -> 5: model + run_step1, once."""
    clean = np.load(GOLDEN)[:, :, 80:144, 80:144].astype(np.float32).reshape(9, -1)
    fl = synth.add_defects((9, 3, 64, 64), 3).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    y = np.where(fl, np.float32(0.0), clean)

    def step(z, sig):
        _, basic, _ = O.run_step1(O.make_params(sig, 2.7, *HT), z.reshape(9, -1), mask, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        return basic
    x, x0, r = M.loop(y, fl, mask, 64, 64, 3, 4, 30.0, 5.0, step)
    return clean, fl, y, x, x0, r


def test_the_loop_gains_on_the_golden_crop(composition):
    clean, fl, y, x, x0, r = composition
    fill, loop = M.psnr_on(x0, clean, fl), M.psnr_on(x, clean, fl)
    print(f"CPU composition: flagged {int(fl.sum())} of {fl.size} ({100.0 * fl.mean():.4f} %), {r['passes']} passes; PSNR over the flagged "
          f"values: fill {fill:.4f} dB, loop {loop:.4f} dB, gain {loop - fill:.4f} dB")
    assert abs(fill - CPU_FILL_DB) < 2e-3 and abs(loop - CPU_LOOP_DB) < 2e-3   # the recorded values
    assert loop - fill >= 5.0                                                  # half of the roughly 10 dB measured
    assert np.array_equal(x[~fl].view(np.uint32), y[~fl].view(np.uint32))      # the sound data is back after every step
    assert np.isfinite(x).all() and int(r["left"].sum()) == 0 and int(r["flagged"].sum()) == int(fl.sum())


def _readme_args(cli, tmp, src):
    if cli.endswith("LFBM3Ddenoising"):
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_defect_variables(tmp_path, cli):
    """Malformed values stop the command before it reads a file; well-formed ones get as far as the (missing) input files."""
    import subprocess
    args = _readme_args(os.path.join(ROOT, "lfbm5d_amd", cli), str(tmp_path), str(tmp_path / "missing"))
    for bad in ("bogus", "", "-1", "1.5", " 2", "2x", "1001"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_DEFECTS=str(tmp_path), LFBM5D_DEFECTS_ITER=bad))
        assert r.returncode != 0 and "LFBM5D_DEFECTS_ITER must be" in r.stdout, bad
        assert "Read input image" not in r.stdout, bad
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_DEFECTS=""))
    assert r.returncode != 0 and "LFBM5D_DEFECTS must name" in r.stdout and "Read input image" not in r.stdout
    for good in (dict(LFBM5D_DEFECTS=str(tmp_path)), dict(LFBM5D_DEFECTS=str(tmp_path), LFBM5D_DEFECTS_ITER="0"), dict(LFBM5D_DEFECTS_ITER="3")):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **good))
        assert r.returncode != 0 and "must" not in r.stdout, good
        assert "not found or not a correct png image" in r.stdout, good
