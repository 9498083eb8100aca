"""CPU tests of the clipped Poisson-Gaussian stage (lfbm5d_pgclip_*, include/lfbm5d_pgclip.h): the exports, the censored fit against the
numpy model and against the truth on the golden light field, the curves against the numpy construction, their properties (monotone,
inverse of G, Monte-Carlo round trip and deviation), the degenerate affine case and what is refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import clip_model as CM
import pgclip_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
MASK = np.ones(9, np.uint32)
MEAN_LEVEL = 121.4

# true (a, b) -> allowed relative error of the fitted variance at the light field's mean level (noise of seed 1, rounded and clipped)
FIT_CASES = {(2.0, 25.0): 0.05, (1.0, 100.0): 0.05, (0.0, 625.0): 0.05, (4.0, 50.0): 0.05, (0.5, 4.0): 0.10}
# (a, b, lo, hi) of the curves
CURVE_CASES = [(0.0, 625.0, 0.0, 255.0), (0.0, 2500.0, 0.0, 255.0), (2.0, 25.0, 0.0, 255.0), (1.0, 100.0, 0.0, 255.0),
               (0.0, 625.0, 16.0, 235.0)]


def test_library_exports_the_pgclip_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_pgclip_fit", "lfbm5d_pgclip_curves", "lfbm5d_pgclip_curves_error", "lfbm5d_pgclip_estimate_device",
              "lfbm5d_pgclip_estimate_host_sai", "lfbm5d_pgclip_forward_device", "lfbm5d_pgclip_inverse_device",
              "lfbm5d_denoise_pgclip_device", "lfbm5d_denoise_pgclip_host_sai"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.PgclipModelStruct) == 4 * 8
    assert C.sizeof(core.PgclipEstimateStruct) == 4 * 8 + 6 * 8 + 2 * 8 + 4 * 4 + 2 * 8
    assert C.sizeof(core.PgclipCurvesStruct) == 4 * 8 + 5 * 8 + 2 * 4 * 4097
    assert core.PGCLIP_KNOTS == M.KNOTS == 4097
    hdr = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    assert hdr.index('#include "lfbm5d_photo.h"') < hdr.index('#include "lfbm5d_pgclip.h"') < hdr.rindex("#endif")
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d_pgclip.h")).read(), flags=re.S)
    for n in ("lfbm5d_pgclip_model", "lfbm5d_pgclip_estimate", "struct lfbm5d_pgclip_curves", "lfbm5d_denoise_pgclip_device"):
        assert n in own, n


# ---- the fit ----

@pytest.fixture(scope="module")
def golden():
    """The model's statistics and fits of the whole golden light field under every noise of FIT_CASES (seed 1), rounded and clipped."""
    lf = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    out = {}
    for a, b in FIT_CASES:
        z = synth.clip_round(synth.add_poisson_gaussian(lf, a, b, 1))
        out[(a, b)] = (M.estimate(z, MASK, 256, 256, 3), z)
    return out


def _close(x, want, rel=1e-9):
    return abs(x - want) <= rel * abs(want) or (np.isnan(x) and np.isnan(want))


def _same(got, want, C_=3):
    assert _close(got.a, want["a"]) and _close(got.b, want["b"]), (got, want["a"], want["b"])
    for c in range(C_):
        assert _close(got.a_channel[c], want["a_channel"][c]) and _close(got.b_channel[c], want["b_channel"][c]), c
    assert (got.levels, got.f_max, got.heavily_clipped, got.quantised) == (want["levels"], want["f_max"], want["heavily_clipped"],
                                                                           want["quantised"])
    assert _close(got.censored, want["censored"])


def test_fit_matches_the_model_on_the_golden_light_field(golden):
    for ab, (r, _) in golden.items():
        assert r["blocks"] == 9 * 3 * 128 * 128 and r["skipped"] == 0 and r["quantised"]
        got = L.pgclip_fit(r["hist"], r["sum_m"], r["cens"], r["whole"])
        _same(got, r)
        assert (got.lo, got.hi) == (0.0, 255.0)
        g1 = L.pgclip_fit(r["hist"][:1], r["sum_m"][:1], r["cens"][:1], r["whole"][:1])   # one channel alone: its own fit
        assert _close(g1.a, r["a_channel"][0]) and _close(g1.b, r["b_channel"][0])


def test_fit_on_another_range_matches_the_model(golden):
    """16..235: the levels, the censoring and the conversion of a and b back from the rescaled range."""
    _, z = golden[(2.0, 25.0)]
    z = np.clip(z, 16.0, 235.0)
    r = M.estimate(z, MASK, 256, 256, 3, 16.0, 235.0)
    got = L.pgclip_fit(r["hist"], r["sum_m"], r["cens"], r["whole"], 16.0, 235.0)
    _same(got, r)
    assert (got.lo, got.hi) == (16.0, 235.0)
    # the variance at the mean level is that of the same noise: the photon term now counts from lo = 16
    err = (got.a * (MEAN_LEVEL - 16.0) + got.b) / (2.0 * MEAN_LEVEL + 25.0) - 1.0
    print(f"range 16..235: a = {got.a:.4f}, b = {got.b:.4f}, variance at {MEAN_LEVEL}: {100 * err:+.1f} %")
    assert abs(err) <= 0.05


def test_the_counts_at_the_default_range_are_the_clipped_stage_s(golden):
    r, z = golden[(1.0, 100.0)]
    hist, sm, cens, whole, blocks, skipped = CM.histogram(z, MASK, 256, 256, 3)
    assert np.array_equal(hist, r["hist"]) and np.array_equal(sm, r["sum_m"]) and np.array_equal(cens, r["cens"])
    assert np.array_equal(whole, r["whole"]) and (blocks, skipped) == (r["blocks"], r["skipped"])


def test_accuracy_of_the_fit(golden):
    for (a, b), tol in FIT_CASES.items():
        r, _ = golden[(a, b)]
        true = a * MEAN_LEVEL + b
        err = (r["a"] * MEAN_LEVEL + r["b"]) / true - 1.0
        print(f"true ({a}, {b}): fitted a = {r['a']:.4f}, b = {r['b']:.4f} ({r['levels']} levels, f_max {r['f_max']}), "
              f"variance at {MEAN_LEVEL}: {100 * err:+.1f} %")
        assert abs(err) <= tol, ((a, b), err)


def test_fit_refuses_bad_arguments_and_too_few_levels():
    hist, z2, wh = np.zeros((1, 64, 322), np.uint64), np.zeros((1, 64), np.uint64), np.zeros(1, np.uint64)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_fit"):
        L.pgclip_fit(hist, z2, z2, wh)                                # nothing populated
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_fit"):
        L.pgclip_fit(hist, z2, z2, wh, 255.0, 0.0)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_fit"):
        L.pgclip_fit(hist[0], z2, z2, wh)
    lib, res = core.lib(), core.PgclipEstimateStruct()
    assert lib.lfbm5d_pgclip_fit(None, None, None, None, 1, 0.0, 255.0, C.byref(res)) == 1


# ---- the curves ----

@pytest.fixture(scope="module")
def curves():
    """(the library's curves, the numpy construction) of every case, built once."""
    return {case: (L.pgclip_curves(*case), M.curves(*case)) for case in CURVE_CASES}


def test_curves_match_the_numpy_construction(curves):
    for case, (got, want) in curves.items():
        assert _close(got.s, want["s"]), (case, got.s, want["s"])
        for k in ("fwd_x0", "fwd_dx", "inv_x0", "inv_dx"):
            assert abs(getattr(got, k) - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (case, k)
        df = float(np.abs(got.fwd.astype(np.float64) - want["fwd64"]).max())
        di = float(np.abs(got.inv.astype(np.float64) - want["inv64"]).max())
        print(f"{case}: s = {got.s:.6f}, max |fwd - model| = {df:.2e}, max |inv - model| = {di:.2e}")
        # the library's tables are the model's float64 tables rounded to float32 (half an ulp of 255: 7.7e-6), and equal the model's
        # own float32 tables within the 1e-6 that two erfc implementations may differ by
        assert np.abs(got.fwd.astype(np.float64) - want["fwd"].astype(np.float64)).max() <= 1e-6, case
        assert np.abs(got.inv.astype(np.float64) - want["inv"].astype(np.float64)).max() <= 1e-6, case
        assert (got.a, got.b, got.lo, got.hi) == case
        assert got.fwd[0] < 0.0 < got.fwd[-1] and got.inv[0] == np.float32(case[2]) and got.inv[-1] == np.float32(case[3])


def test_tables_are_strictly_increasing_and_invert_G(curves):
    for case, (got, want) in curves.items():
        assert (np.diff(got.fwd) > 0).all() and (np.diff(got.inv) > 0).all(), case
        assert (np.diff(want["G"]) > 0).all() and (np.diff(want["mean"]) > 0).all()
        # inv(G(y)) = y on a grid finer than the knots: G between its knots is piecewise linear, as G^-1 is defined
        y = np.linspace(case[2], case[3], 20001)
        g = np.interp(y, want["y"], want["G"])
        back = M.curve_map(g.astype(np.float32), got.inv, got.inv_x0, got.inv_dx, True).astype(np.float64)
        err = float(np.abs(back - y).max())
        slope = float((np.diff(want["G"]) / np.diff(want["y"])).min())
        print(f"{case}: max |inv(G(y)) - y| = {err:.2e}, smallest slope of G = {slope:.3f}")
        assert err <= 1e-3, (case, err)


def test_monte_carlo_round_trip_and_deviation(curves):
    """z = clip(y + sigma(y) n) through the float32 tables: the inverse of the mean of F(z) returns y within 0.3 grey levels and the
    deviation of F(z) lies within [0.70 s, 1.15 s] (0.75 s at the bounds, where half the mass is a point)."""
    rng = np.random.default_rng(7)
    N = 400000
    worst_bias, dev_lo, dev_hi = 0.0, np.inf, -np.inf
    for (a, b, lo, hi), (got, _) in curves.items():
        for y in (lo, lo + 5, lo + 20, 0.5 * (lo + hi), hi - 20, hi - 5, hi):
            z = np.clip(y + float(M.sigma_of(y, a, b, lo)) * rng.standard_normal(N), lo, hi).astype(np.float32)
            f = M.curve_map(z, got.fwd, got.fwd_x0, got.fwd_dx, False).astype(np.float64)
            back = float(M.curve_map(np.float32(f.mean()), got.inv, got.inv_x0, got.inv_dx, True))
            d = float(f.std()) / got.s
            worst_bias, dev_lo, dev_hi = max(worst_bias, abs(back - y)), min(dev_lo, d), max(dev_hi, d)
            assert abs(back - y) <= 0.3, ((a, b, lo, hi), y, back)
            assert 0.70 <= d <= 1.15, ((a, b, lo, hi), y, d)
    print(f"largest round-trip bias {worst_bias:.3f} grey levels, std F / s in [{dev_lo:.3f}, {dev_hi:.3f}]")


def test_forward_map_is_affine_when_nothing_is_clipped():
    """a = 0 and sigma far below the range: in mid-range the clipped moments are the plain ones and F is a line of slope s / sigma."""
    got = L.pgclip_curves(0.0, 4.0, 0.0, 255.0)
    x = got.fwd_x0 + got.fwd_dx * np.arange(4097)
    mid = (x >= 32.0) & (x <= 223.0)
    f = got.fwd.astype(np.float64)
    line = f[2048] + (x - x[2048]) * (got.s / 2.0)
    assert np.abs(f[mid] - line[mid]).max() <= 1e-3
    assert abs(got.s - 2.0) <= 0.05                                     # the span is 255 up to the two ends' loss of deviation


@pytest.mark.parametrize("a,b,lo,hi", [(-1.0, 25.0, 0.0, 255.0), (1.0, -1.0, 0.0, 255.0), (0.0, 0.0, 0.0, 255.0), (1.0, 100.0, 255.0, 0.0),
                                       (1.0, 100.0, 5.0, 5.0), (float("nan"), 1.0, 0.0, 255.0), (1.0, float("inf"), 0.0, 255.0),
                                       (1.0, 100.0, float("-inf"), 255.0)])
def test_invalid_models_are_refused(a, b, lo, hi):
    with pytest.raises(L.LfBm5dError, match="lfbm5d_pgclip_curves: bad model"):
        L.pgclip_curves(a, b, lo, hi)
    assert M.curves(a, b, lo, hi) is None


@pytest.mark.parametrize("a,b", [(8.0, 0.0), (1.0, 0.0), (2.0, 3.9), (5.5, 1000.0)])
def test_models_outside_the_accepted_domain_are_refused(a, b):
    with pytest.raises(L.LfBm5dError, match="accepted domain.*denoise_pg"):
        L.pgclip_curves(a, b)
    assert M.curves(a, b) is None


def test_models_at_the_edge_of_the_domain_are_accepted():
    assert L.pgclip_curves(4.0, 50.0).s > 0 and L.pgclip_curves(0.5, 4.0).s > 0 and L.pgclip_curves(5.0, 50.0).s > 0
    lib = core.lib()
    assert lib.lfbm5d_pgclip_curves(None, None) == 1 and b"NULL" in lib.lfbm5d_pgclip_curves_error()
