"""CPU tests of the Poisson-Gaussian noise routines (lfbm5d_pg_*, include/lfbm5d.h): the exports, the host-only fit and scale against
the numpy model (tests/pg_model.py), the accuracy of the definition on the golden light field, a Monte-Carlo check of the transform
model, and the CLIs' LFBM5D_SIGMA=poisson parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import pg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")

# true (a, b) -> allowed relative error of the fitted variance at the light field's mean level 121.4 (seed 1)
CASES = {(1.0, 0.0): 0.15, (0.5, 4.0): 0.15, (2.0, 25.0): 0.15, (0.0, 100.0): 0.15, (0.25, 1.0): 0.20}
MEAN_LEVEL = 121.4


def test_library_exports_the_pg_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_pg_histogram_device", "lfbm5d_pg_fit", "lfbm5d_pg_estimate_device", "lfbm5d_pg_estimate_host_sai", "lfbm5d_pg_scale",
              "lfbm5d_pg_forward_device", "lfbm5d_pg_inverse_device", "lfbm5d_denoise_pg_device", "lfbm5d_denoise_pg_host_sai"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.PgModelStruct) == 6 * 8
    assert C.sizeof(core.PgEstimateStruct) == 8 * 8 + 2 * 8
    assert (core.PG_LEVELS, core.PG_KEYS) == (M.L, M.Q) == (64, 322)


@pytest.fixture(scope="module")
def golden_estimates():
    """The model's statistics and fits of the whole golden light field under every noise of CASES (seed 1), computed once."""
    lf = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    return {ab: M.estimate(synth.add_poisson_gaussian(lf, ab[0], ab[1], 1), mask, 256, 256, 3) for ab in CASES}


def _close(x, want):
    return abs(x - want) <= 1e-10 * abs(want) + 1e-12


def test_fit_matches_the_model_on_the_golden_light_field(golden_estimates):
    for ab, r in golden_estimates.items():
        hist, sm = r["hist"], r["sum_m"]
        assert r["blocks"] == 9 * 3 * 128 * 128 and r["skipped"] == 0
        assert int(hist.sum()) == r["blocks"]                       # every block sits in exactly one bin
        a, b = L.pg_fit(hist.sum(axis=0), sm.sum(axis=0))
        assert _close(a, r["a"]) and _close(b, r["b"]), (ab, a, b, r["a"], r["b"])
        for c in range(3):
            a, b = L.pg_fit(hist[c], sm[c])
            assert _close(a, r["a_channel"][c]) and _close(b, r["b_channel"][c]), (ab, c)


def test_accuracy_of_the_definition(golden_estimates):
    for (a, b), tol in CASES.items():
        r = golden_estimates[(a, b)]
        true = a * MEAN_LEVEL + b
        err = (r["a"] * MEAN_LEVEL + r["b"]) / true - 1.0
        print(f"true ({a}, {b}): fitted a = {r['a']:.4f}, b = {r['b']:.4f}, variance at {MEAN_LEVEL}: {100 * err:+.1f} %")
        assert abs(err) <= tol, ((a, b), err)


def _level(hist, sm, lev, sigma, n, x):
    """Fill level `lev` with n samples of |N(0, sigma^2)| placed at their expected bin counts, at mean level x (0..255)."""
    from math import erf, sqrt
    e = M.edges()
    cdf = np.array([erf(v / (sigma * sqrt(2.0))) for v in e] + [1.0])
    cnt = np.floor(n * np.diff(cdf) + 0.5).astype(np.uint64)
    hist[lev] = cnt
    sm[lev] = np.uint64(round(x * 256.0)) * cnt.sum()


def _both(hist, sm):
    got, want = L.pg_fit(hist, sm), M.fit(hist, sm)
    assert _close(got[0], want[0]) and _close(got[1], want[1]), (got, want)
    return got


def test_fit_branches_on_hand_made_histograms():
    z = lambda: (np.zeros((M.L, M.Q), np.uint64), np.zeros(M.L, np.uint64))
    # two levels on a line v = 0.5 x + 4: the plain least-squares branch
    h, s = z()
    _level(h, s, 10, np.sqrt(0.5 * 40 + 4), 100000, 40.0)
    _level(h, s, 40, np.sqrt(0.5 * 160 + 4), 100000, 160.0)
    a, b = _both(h, s)
    assert abs(a - 0.5) < 0.05 and abs(b - 4.0) < 2.0
    # one valid level (the other holds fewer than 256 blocks): a = 0, b = that level's variance
    h, s = z()
    _level(h, s, 10, 5.0, 100000, 40.0)
    _level(h, s, 40, 9.0, 200, 160.0)
    a, b = _both(h, s)
    assert a == 0.0 and abs(b - 25.0) < 1.0
    # negative slope: a = 0, b = the weighted mean variance
    h, s = z()
    _level(h, s, 10, 9.0, 100000, 40.0)
    _level(h, s, 40, 5.0, 100000, 160.0)
    a, b = _both(h, s)
    assert a == 0.0 and 25.0 < b < 81.0
    # negative intercept: b = 0, a = Swxv / Swxx
    h, s = z()
    _level(h, s, 10, np.sqrt(10.0), 100000, 40.0)
    _level(h, s, 40, np.sqrt(100.0), 100000, 160.0)
    a, b = _both(h, s)
    assert b == 0.0 and 0.25 < a < 0.625
    # no valid level -> 1; so do quantiles that fall into key 0 or key 321
    h, s = z()
    assert M.fit(h, s) is None
    with pytest.raises(L.LfBm5dError):
        L.pg_fit(h, s)
    for key in (0, M.Q - 1):
        h, s = z()
        h[20, key] = 1000
        s[20] = 1000 * 80 * 256
        assert M.fit(h, s) is None
        with pytest.raises(L.LfBm5dError):
            L.pg_fit(h, s)
        _level(h, s, 30, 5.0, 100000, 120.0)               # ... and such a level is skipped, not fatal, next to a valid one
        a, b = _both(h, s)
        assert a == 0.0 and abs(b - 25.0) < 1.0
    lib = core.lib()
    x = C.c_double()
    assert lib.lfbm5d_pg_fit(None, None, C.byref(x), C.byref(x)) == 1


def test_scale_closed_forms_and_rejections():
    assert L.pg_scale((0.0, 400.0)) == 20.0
    assert L.pg_scale((0.0, 2.0), chnls=1) == np.sqrt(2.0)
    for a, b in ((1.0, 0.0), (2.0, 25.0), (8.0, 0.0)):
        c = 0.375 * a * a + b
        want = (np.sqrt(255.0 * a + c) + np.sqrt(c)) / 2.0
        assert abs(L.pg_scale((a, b)) - want) <= 1e-14 * want
        assert abs(M.scale([a] * 3, [b] * 3) - want) <= 1e-14 * want
    av, bv = [1.0, 2.0, 0.0], [0.0, 25.0, 9.0]
    assert abs(L.pg_scale((av, bv)) - M.scale(av, bv)) <= 1e-14 * M.scale(av, bv)
    for a, b in ((0.0, 0.0), (1.0, -0.375), (1.0, -1.0), (-1.0, 5.0), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0)):
        assert M.scale([a], [b]) is None
        with pytest.raises(L.LfBm5dError):
            L.pg_scale((a, b))
    with pytest.raises(L.LfBm5dError):
        L.pg_scale(([1.0, 1.0, -1.0], [1.0, 1.0, 1.0]))          # one bad channel is enough
    with pytest.raises(L.LfBm5dError):
        L.pg_scale(([1.0, 1.0], [1.0, 1.0]), chnls=2)
    s = C.c_double()
    assert core.lib().lfbm5d_pg_scale(None, 3, C.byref(s)) == 1


@pytest.mark.parametrize("a,b", [(1.0, 0.0), (2.0, 25.0)])
def test_monte_carlo_check_of_the_transform_model(a, b):
    s = M.scale([a], [b])
    rng = np.random.default_rng(7)
    for y in (2.0, 10.0, 100.0):
        z = a * rng.poisson(y / a, 2_000_000) + rng.normal(0.0, np.sqrt(b), 2_000_000)
        t = M.forward(z, a, b, s)
        back = float(M.inverse(np.array([t.mean()]), a, b, s)[0])
        print(f"a = {a}, b = {b}, y = {y}: std / s = {t.std() / s:.4f}, inverse of the mean = {back:.4f}")
        assert abs(t.std() / s - 1.0) <= 0.07
        assert abs(back - y) <= 0.1


def test_synthetic_noise_has_the_model_s_moments():
    clean = np.full(400000, 60.0, np.float32)
    for a, b in ((2.0, 25.0), (0.0, 100.0), (4.0, 0.0)):
        z = synth.add_poisson_gaussian(clean, a, b, 3)
        assert z.dtype == np.float32
        assert abs(z.mean() - 60.0) < 0.1 and abs(z.var() / (a * 60.0 + b) - 1.0) < 0.02
        assert np.array_equal(z, synth.add_poisson_gaussian(clean, a, b, 3))


def _readme_args(cli, tmp, src="none"):
    if cli.endswith("LFBM3Ddenoising"):
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_poisson_modes(tmp_path, cli):
    """Malformed models stop the command before it reads a file; well-formed ones get as far as the (missing) input files."""
    args = _readme_args(os.path.join(ROOT, "lfbm5d_amd", cli), str(tmp_path), src=str(tmp_path / "missing"))
    for bad in ("poisson:x", "poisson:1", "25", "poisson:1,", "poisson:1,2x", "poisson:-1,2", "poisson:0,0", "poisson:1;2", "Poisson"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_SIGMA=bad))
        assert r.returncode != 0 and "LFBM5D_SIGMA must be" in r.stdout, bad
        assert "Read input image" not in r.stdout, bad
    for good in ("poisson", "poisson:8,0", "poisson:0.5,4", "poisson:0,100"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_SIGMA=good))
        assert r.returncode != 0 and "LFBM5D_SIGMA must be" not in r.stdout, good
        assert "not found or not a correct png image" in r.stdout, good
