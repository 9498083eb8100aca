"""CPU tests of the blind noise-level estimate (lfbm5d_noise_level_*, include/lfbm5d.h): the exports, the host-only statistic
against the float64 numpy model (tests/noise_model.py), and the CLIs' LFBM5D_SIGMA parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
from noise_model import model, statistic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")

# the model's estimates (r = 8, MT19937 float noise, seed 1): golden light field, then the same rounded and clipped to 0..255
TABLE_GOLDEN = {2: 2.648, 5: 5.293, 10: 10.174, 25: 25.119, 50: 50.134}
TABLE_GOLDEN_CLIPPED = {2: 2.661, 5: 5.283, 10: 10.097, 25: 24.111, 50: 45.102}


def test_library_exports_the_noise_level_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_noise_level_device", "lfbm5d_noise_level_host_sai", "lfbm5d_noise_level_statistic"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.NoiseLevelStruct) == 8 + 3 * 8 + 4 + 4 + 8


def _check(cov):
    s_m, m_m, lam_m = statistic(cov)
    s_g, m_g, lam_g = L.noise_level_statistic(cov)
    assert m_g == m_m
    assert abs(s_g - s_m) <= 1e-7 * s_m
    assert np.abs(lam_g - lam_m).max() <= 1e-12 * np.abs(lam_m).max()
    return m_g


@pytest.mark.parametrize("d", [16, 36, 64])
def test_statistic_matches_the_model_on_random_psd_matrices(d):
    rng = np.random.default_rng(d)
    ms = set()
    for trial in range(20):
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        k = int(rng.integers(1, d // 2))                          # a signal subspace of k directions over white noise
        lam = rng.uniform(3.0, 5.0, d) * rng.uniform(0.5, 2.0)
        lam[:k] += 10.0 ** rng.uniform(1, 5, k)
        ms.add(_check((q * lam) @ q.T))
        w = rng.standard_normal((d, 3 * d))                       # and plain Wishart matrices
        _check(w @ w.T / (3 * d))
    assert len(ms) > 3                                            # the stopping rule takes different m


def test_statistic_on_the_pooled_covariances_of_the_golden_light_field():
    lf = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    for sigma in sorted(TABLE_GOLDEN):
        noisy = synth.add_noise_mt19937(lf, sigma, seed=1)
        for x, table in ((noisy, TABLE_GOLDEN), (np.clip(np.round(noisy), 0, 255), TABLE_GOLDEN_CLIPPED)):
            r = model(x, np.ones(9), 256, 256, 3)
            _check(r["cov"])
            assert round(r["sigma"], 3) == table[sigma]


def test_statistic_rejects_bad_sizes():
    for d in (0, 65):
        with pytest.raises(L.LfBm5dError):
            L.noise_level_statistic(np.eye(max(d, 1)) if d else np.zeros((0, 0)))
    lib = core.lib()
    s, m = C.c_double(), C.c_uint()
    assert lib.lfbm5d_noise_level_statistic(4, None, C.byref(s), C.byref(m), None) == 1


def _readme_args(cli, tmp, src="none"):
    if cli.endswith("LFBM3Ddenoising"):
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_rejects_an_unknown_sigma_mode(tmp_path, cli):
    """LFBM5D_SIGMA accepts "auto" only; anything else stops the command before it reads a file or touches a GPU."""
    args = _readme_args(os.path.join(ROOT, "lfbm5d_amd", cli), str(tmp_path))
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_SIGMA="25"))
    assert r.returncode != 0 and "LFBM5D_SIGMA must be" in r.stdout
