"""CPU tests of the clipping-aware routines (lfbm5d_clip_*, lfbm5d_declip_*, include/lfbm5d.h): the exports, the identities of the
clipped-mean map of the numpy model (tests/clip_model.py), the host-only fit against the model, its ladder on synthetic counts, and the
accuracy of the definition on the golden light field."""
import ctypes as C
from math import erf, sqrt

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import clip_model as M
import noise_model
import pg_model
from helpers import noisy_lf, source_lf

MASK = np.ones(9, np.uint32)


def test_library_exports_the_clip_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_clip_histogram_device", "lfbm5d_clip_fit", "lfbm5d_noise_level_clipped_device", "lfbm5d_noise_level_clipped_host_sai",
              "lfbm5d_declip_device", "lfbm5d_declip_host_sai", "lfbm5d_denoise_clipped_device", "lfbm5d_denoise_clipped_host_sai"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.ClipEstimateStruct) == 6 * 8 + 4 * 4 + 2 * 8
    for n in ("noise_level_clipped", "denoise_clipped", "clip_fit", "ClipNoiseLevel"):
        assert hasattr(L, n), n
    for n in ("clip_histogram", "clip_fit", "declip", "noise_level_clipped", "denoise_clipped"):
        assert hasattr(L.Context, n), n


def test_clip_round_rounds_then_clips():
    x = np.array([-3.2, -0.4, 0.5, 1.5, 2.5, 254.6, 255.4, 300.0, np.nan], np.float32)
    got = synth.clip_round(x)
    assert got.dtype == np.float32
    assert np.array_equal(got[:-1], np.array([0, 0, 0, 2, 2, 255, 255, 255], np.float32)) and np.isnan(got[-1])
    assert np.array_equal(synth.clip_round(x[:-1], 16, 235), np.array([16, 16, 16, 16, 16, 235, 235, 235], np.float32))
    with pytest.raises(ValueError):
        synth.clip_round(x, 5, 5)


# ---- the map ----

RANGES = [(0.0, 255.0), (16.0, 235.0)]
SIGMAS = [1.0, 5.0, 25.0, 50.0, 100.0]


@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_map_identities(sigma, lo, hi):
    e_lo, e_hi = float(M.clipped_mean(lo, sigma, lo, hi)), float(M.clipped_mean(hi, sigma, lo, hi))
    assert lo < e_lo < e_hi < hi
    d = np.linspace(e_lo, e_hi, 4001)
    y = M.declip(d, sigma, lo, hi)
    assert np.abs(M.clipped_mean(y, sigma, lo, hi) - d).max() <= 1e-9                                   # E(E^-1(d)) = d
    assert (np.diff(y) >= 0).all() and y[0] == lo and y[-1] == hi
    yy = np.linspace(lo, hi, 4001)
    E = M.clipped_mean(yy, sigma, lo, hi)
    assert np.abs(M.clipped_mean(lo + hi - yy, sigma, lo, hi) - (lo + hi - E)).max() <= 1e-9            # point symmetry
    far = (yy - lo > 8.0 * sigma) & (hi - yy > 8.0 * sigma)
    if sigma <= 5.0:
        assert far.any()
    assert np.abs(E[far] - yy[far]).max(initial=0.0) <= 1e-9                                             # the identity far from the bounds
    assert (np.diff(E) > 0).all()
    s = M.slope(yy, sigma, lo, hi)
    assert s.min() >= 0.5 * erf((hi - lo) / (sigma * sqrt(2.0))) - 1e-12                                 # Phi((hi - lo) / sigma) - 1/2
    num = (M.clipped_mean(yy + 1e-4, sigma, lo, hi) - M.clipped_mean(yy - 1e-4, sigma, lo, hi)) / 2e-4
    assert np.abs(num - s).max() <= 1e-6
    # outside [E(lo), E(hi)] the result is the bound; non-finite values pass through
    out = M.declip(np.array([lo - 50.0, e_lo, e_hi, hi + 50.0, np.nan, np.inf, -np.inf]), sigma, lo, hi)
    assert list(out[:4]) == [lo, lo, hi, hi] and np.isnan(out[4]) and out[5] == np.inf and out[6] == -np.inf


def test_clipped_mean_at_the_bounds_is_the_documented_bias():
    for sigma in (10.0, 25.0):
        assert abs(float(M.clipped_mean(0.0, sigma)) - sigma / sqrt(2.0 * np.pi)) <= 1e-9        # sigma phi(0) at y = lo
        assert abs(255.0 - float(M.clipped_mean(255.0, sigma)) - sigma / sqrt(2.0 * np.pi)) <= 1e-9


# ---- the fit ----

@pytest.fixture(scope="module")
def golden():
    """The model's statistics and fits of the whole golden light field, noise of helpers.noisy_lf (MT19937 seed 1) then rint and clip,
    computed once; key "float": the unclipped float noise at sigma = 25."""
    out = {}
    for sigma in (10.0, 25.0, 50.0, 75.0):
        clean, noisy = noisy_lf(source_lf(), sigma)
        out[sigma] = (M.estimate(synth.clip_round(noisy), MASK, 256, 256, 3), synth.clip_round(noisy))
        if sigma == 25.0:
            out["float"] = (M.estimate(noisy, MASK, 256, 256, 3), noisy)
    return out


def _close(x, want, rel=1e-9):
    return abs(x - want) <= rel * abs(want)


def _same(got, want, C_=3):
    assert _close(got.sigma, want["sigma"]), (got, want["sigma"])
    for c in range(C_):
        assert _close(got.sigma_channel[c], want["sigma_channel"][c]), c
    assert (got.levels, got.f_max, got.heavily_clipped, got.quantised) == (want["levels"], want["f_max"], want["heavily_clipped"],
                                                                           want["quantised"])
    assert _close(got.censored, want["censored"])


def test_fit_matches_the_model_on_the_golden_light_field(golden):
    for key, (r, _) in golden.items():
        assert r["blocks"] == 9 * 3 * 128 * 128 and r["skipped"] == 0 and int(r["hist"].sum()) == r["blocks"]
        assert r["quantised"] == (key != "float")
        got = L.clip_fit(r["hist"], r["sum_m"], r["cens"], r["whole"])
        _same(got, r)
        _same(L.clip_fit(r["hist"], None, r["cens"], r["whole"]), r)                  # the level means are not read
        g1 = L.clip_fit(r["hist"][:1], r["sum_m"][:1], r["cens"][:1], r["whole"][:1])   # one channel alone: its own fit
        assert _close(g1.sigma, r["sigma_channel"][0]) and g1.sigma_channel == (g1.sigma,)


def test_statistics_of_the_default_range_are_the_poisson_gaussian_ones(golden):
    r, lf = golden[25.0]
    hist, sm, _, _ = pg_model.histogram(lf, MASK, 256, 256, 3)
    assert np.array_equal(hist, r["hist"]) and np.array_equal(sm, r["sum_m"])
    # a censored block holds a 0 or a 255; every value is whole
    x = lf.reshape(9, 3, 128, 2, 128, 2)
    want = ((x <= 0) | (x >= 255)).any(axis=(3, 5)).sum()
    assert int(r["cens"].sum()) == int(want) and int(r["whole"].sum()) == r["blocks"]


def test_accuracy_of_the_definition(golden):
    """sigma-hat on the clipped, rounded golden light field (noise of helpers.noisy_lf): within 3 % at sigma = 10, 25, 50, and at most
    half the error of the blind estimate (tests/noise_model.py) on the same input at 25 and 50."""
    for sigma in (10.0, 25.0, 50.0):
        r, lf = golden[sigma]
        print(f"sigma = {sigma}: clipping-aware {r['sigma']:.3f} ({r['levels']} levels, f_max = {r['f_max']}, censored blocks "
              f"{100 * r['censored']:.1f} %), per channel {[round(v, 3) for v in r['sigma_channel']]}")
        assert abs(r["sigma"] / sigma - 1.0) <= 0.03, (sigma, r["sigma"])
        assert not r["heavily_clipped"]
        if sigma >= 25.0:
            blind = noise_model.model(lf, MASK, 256, 256, 3)["sigma"]
            print(f"sigma = {sigma}: blind estimate on the same input {blind:.3f}")
            assert abs(r["sigma"] - sigma) <= 0.5 * abs(blind - sigma), (sigma, r["sigma"], blind)
    r, _ = golden[75.0]
    print(f"sigma = 75: clipping-aware {r['sigma']:.3f} ({r['levels']} levels, f_max = {r['f_max']})")
    assert np.isfinite(r["sigma"]) and r["heavily_clipped"] and r["f_max"] > 0.1
    r, _ = golden["float"]
    print(f"sigma = 25, float noise: {r['sigma']:.3f}")
    assert abs(r["sigma"] / 25.0 - 1.0) <= 0.03 and not r["quantised"]


def _level(hist, lev, sigma, n):
    """Fill level `lev` with n samples of |N(0, sigma^2)| placed at their expected bin counts."""
    e = pg_model.edges()
    cdf = np.array([erf(v / (sigma * sqrt(2.0))) for v in e] + [1.0])
    hist[lev] = np.floor(n * np.diff(cdf) + 0.5).astype(np.uint64)


def _counts(levels, sigma=20.0, n=50000):
    """One channel: `levels` maps a level to its censored fraction."""
    hist, cens = np.zeros((1, M.L, M.Q), np.uint64), np.zeros((1, M.L), np.uint64)
    for lev, f in levels.items():
        _level(hist[0], lev, sigma, n)
        cens[0, lev] = int(f * hist[0, lev].sum())
    return hist, np.zeros((1, M.L), np.uint64), cens, np.zeros(1, np.uint64)


def _both(hist, sm, cens, whole, lo=0.0, hi=255.0):
    got, want = L.clip_fit(hist, sm, cens, whole, lo, hi), M.fit(hist, cens, whole, lo, hi)
    _same(got, want, C_=hist.shape[0])
    return got


def test_ladder_on_synthetic_counts():
    # four clean levels: the first rung
    g = _both(*_counts({10: 0.0, 20: 0.01, 30: 0.04, 40: 0.05}))
    assert (g.levels, g.f_max, g.heavily_clipped) == (4, 0.05, False) and abs(g.sigma - 20.0) < 0.1
    # exactly three clean levels force the next rung, which admits the levels up to 10 %
    g = _both(*_counts({10: 0.0, 20: 0.0, 30: 0.05, 40: 0.08, 50: 0.1, 60: 0.3}))
    assert (g.levels, g.f_max, g.heavily_clipped) == (5, 0.1, False)
    # ... and two rungs further when the rest is censored more heavily
    g = _both(*_counts({10: 0.0, 20: 0.0, 30: 0.05, 40: 0.3, 50: 0.4, 60: 0.9}))
    assert (g.levels, g.f_max, g.heavily_clipped) == (5, 0.4, True)
    g = _both(*_counts({10: 0.5, 20: 0.6, 30: 0.7, 40: 1.0}))
    assert (g.levels, g.f_max, g.heavily_clipped) == (4, 1.0, True) and abs(g.censored - 0.7) < 1e-3
    # a level under 256 blocks is not populated, whatever its censoring
    hist, sm, cens, whole = _counts({10: 0.0, 20: 0.0, 30: 0.0, 40: 0.0})
    hist[0, 40] //= 400
    assert hist[0, 40].sum() < 256
    assert M.fit(hist, cens, whole) is None
    with pytest.raises(L.LfBm5dError, match="fewer than 4 levels"):
        L.clip_fit(hist, sm, cens, whole)
    # fewer than four populated levels altogether: an error, not a guess
    for levels in ({}, {10: 0.0}, {10: 0.0, 20: 0.0, 30: 1.0}):
        hist, sm, cens, whole = _counts(levels)
        assert M.fit(hist, cens, whole) is None
        with pytest.raises(L.LfBm5dError):
            L.clip_fit(hist, sm, cens, whole)
    # another range: the fit scales sigma back by s = (float)(255 / (hi - lo))
    g = _both(*_counts({10: 0.0, 20: 0.0, 30: 0.0, 40: 0.0}), lo=16.0, hi=235.0)
    assert abs(g.sigma - 20.0 / float(np.float32(255.0 / 219.0))) < 0.1
    # rejected arguments
    hist, sm, cens, whole = _counts({10: 0.0, 20: 0.0, 30: 0.0, 40: 0.0})
    for lo, hi in ((5.0, 5.0), (9.0, 3.0), (float("nan"), 255.0), (0.0, float("inf"))):
        with pytest.raises(L.LfBm5dError):
            L.clip_fit(hist, sm, cens, whole, lo, hi)
    with pytest.raises(L.LfBm5dError):
        L.clip_fit(hist[0], sm[0], cens[0], whole)
    res = core.ClipEstimateStruct()
    assert core.lib().lfbm5d_clip_fit(None, None, None, None, 1, 0.0, 255.0, C.byref(res)) == 1


def test_quantised_counts_shift_the_edges():
    """Whole-numbered data at 0..255: d is a multiple of 1/2.  Samples of round(N(0, sigma^2) / delta) delta placed into the keys: read
    with whole = total the fit returns sigma; read as continuous data it is biased by about delta / 2 / 0.3186."""
    sigma, n, delta = 30.0, 200000, 0.5          # the quartile, 9.56, lies where the keys are as wide as delta
    e = pg_model.edges()
    k = np.arange(0, 600)
    mass = np.array([erf((v + 0.5) * delta / (sigma * sqrt(2.0))) - erf(max(v - 0.5, 0.0) * delta / (sigma * sqrt(2.0))) for v in k])
    key = np.clip(np.searchsorted(e, k * delta, side="right") - 1, 0, M.Q - 1)
    row = np.bincount(key, weights=np.floor(n * mass + 0.5), minlength=M.Q).astype(np.uint64)
    hist, cens = np.zeros((1, M.L, M.Q), np.uint64), np.zeros((1, M.L), np.uint64)
    for lev in (10, 20, 30, 40):
        hist[0, lev] = row
    total = np.array([hist.sum()], np.uint64)
    q = _both(hist, None, cens, total)
    c = _both(hist, None, cens, total - np.uint64(1))
    assert q.quantised and not c.quantised
    assert abs(np.sqrt(q.sigma ** 2 + delta ** 2 / 3.0) - sigma) < 0.05
    assert 0.6 < c.sigma - q.sigma < 1.0
