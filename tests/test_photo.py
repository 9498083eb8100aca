"""CPU tests of the photometric equalisation (lfbm5d_photo_*, include/lfbm5d_photo.h): the exports, struct sizes and defaults; the
host-only functions of the library (edges, ratio of a histogram, solve) against the numpy model (tests/photo_model.py) bit for bit; and
the properties of the model that pin the definition: planted gains come back on exact translations, a dimmed view stops being a bad
view, a vignette stops blinding the consistency check, and a field with nothing planted is left alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import consist_model as K
import photo_model as M
import view_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")


def test_library_exports_and_binds_the_photo_entry_points():
    lib = core.lib()
    assert '#include "lfbm5d_photo.h"' in open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d_photo.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lfbm5d_photo_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["lfbm5d_photo_apply_device", "lfbm5d_photo_apply_host_sai", "lfbm5d_photo_defaults", "lfbm5d_photo_device",
                        "lfbm5d_photo_edges", "lfbm5d_photo_host_sai", "lfbm5d_photo_ratio", "lfbm5d_photo_solve"]
    for n in declared:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n       # exported, and bound in core.py
    assert C.sizeof(core.PhotoParamsStruct) == 8 * 4 + 8 + 3 * 8
    assert C.sizeof(core.PhotoResultStruct) == 3 * 8 + 3 * 8 + 5 * 4 + 4       # five unsigned, padding
    for n in ("PhotoParamsStruct", "PhotoResultStruct", "Equalise", "photo_params", "photo_edges", "photo_ratio", "photo_solve", "equalise"):
        assert n in L.__all__ and hasattr(L, n), n
    assert hasattr(L.Context, "equalise") and hasattr(L.Context, "apply_gains")
    assert hasattr(synth, "vignette_gains") and hasattr(synth, "apply_gains")
    assert (M.KEYS, M.N_EDGES) == (core.PHOTO_KEYS, core.PHOTO_EDGES) == (1026, 1025)


def test_defaults_work_without_a_gpu():
    P, Q = L.photo_params(), L.consist_params()
    assert (P.max_disparity, P.box_radius, P.ang_radius) == (Q.max_disparity, Q.box_radius, Q.ang_radius)   # the consistency check's sweep
    assert (P.steps, P.min_sources, P.max_rounds, P.per_channel, P.anchor, P.min_count) == (1, 3, 3, 1, core.PHOTO_NO_ANCHOR, 256)
    assert P.tol == 1.0 / 256
    txt = open(os.path.join(ROOT, "profiles", "photo_defaults.txt")).read()           # lo, hi and max_rounds are the row the sweep's rule picks
    rule = re.search(r"^rule .*: lo = ([0-9.]+), hi = ([0-9.]+), max_rounds = (\d+): ([0-9.]+) %$", txt, re.M)
    shipped = re.search(r"^shipped: lo = ([0-9.]+), hi = ([0-9.]+), max_rounds = (\d+): ([0-9.]+) %$", txt, re.M)
    assert rule and shipped and rule.groups() == shipped.groups()
    assert (P.lo, P.hi, P.max_rounds) == (float(rule.group(1)), float(rule.group(2)), int(rule.group(3)))
    P = L.photo_params(max_disparity=0, box_radius=0, ang_radius=2, steps=4, min_sources=5, max_rounds=1, per_channel=0, anchor=4,
                       min_count=10, tol=0.5, lo=1, hi=2)
    assert (P.max_disparity, P.box_radius, P.ang_radius, P.steps, P.min_sources, P.max_rounds, P.per_channel, P.anchor, P.min_count) == \
        (0, 0, 2, 4, 5, 1, 0, 4, 10)
    assert (P.tol, P.lo, P.hi) == (0.5, 1.0, 2.0)


def test_edges_equal_the_formula_bit_for_bit():
    e = L.photo_edges()
    assert e.dtype == np.float32 and e.shape == (1025,)
    want = np.array([2.0 ** (j // 256 - 2) * (1 + (j % 256) / 256) for j in range(1025)], np.float64)
    assert np.array_equal(e.astype(np.float64), want)                          # every edge is a float32
    assert np.array_equal(e.view(np.uint32), M.EDGES.view(np.uint32))
    assert (np.diff(e.astype(np.float64)) > 0).all() and e[0] == 0.25 and e[1024] == 4.0 and e[512] == 1.0


def test_the_models_key_search_equals_the_count_over_all_edges():
    rng = np.random.default_rng(5)
    mu = rng.uniform(0.0, 300.0, 4000).astype(np.float32)
    I = (mu * rng.uniform(0.1, 6.0, 4000).astype(np.float32)).astype(np.float32)
    j = rng.integers(0, 1025, 4000)
    I[:1500] = (M.EDGES[j[:1500]] * mu[:1500]).astype(np.float32)               # exactly on an edge's product
    I[1500:2500] = np.nextafter(I[:1000], np.float32(-np.inf))                  # and just below one
    I[2500:2520] = -3.0
    mu[2520:2540] = 0.0
    k = M.keys(I, mu)
    assert np.array_equal(k, M.keys_by_definition(I, mu))
    assert k.min() == 0 and k.max() == 1025 and len(np.unique(k)) > 900
    assert M.keys(np.float32(100.0), np.float32(100.0)) == 513                  # ratio 1 sits at the bottom of key 513


def _histograms():
    rng = np.random.default_rng(11)
    out = [np.zeros(M.KEYS, np.uint64)]                                         # empty
    for k in (0, 1, 513, 1024, 1025):                                           # single-bin, the end keys among them
        h = np.zeros(M.KEYS, np.uint64)
        h[k] = 7
        out.append(h)
    for lo_, hi_ in ((0, 40), (990, 1026), (400, 600), (0, 1026), (512, 515)):
        for n in (1, 2, 300, 100000):
            h = np.zeros(M.KEYS, np.uint64)
            h[lo_:hi_] = np.bincount(rng.integers(0, hi_ - lo_, n), minlength=hi_ - lo_).astype(np.uint64)
            out.append(h)
    h = np.zeros(M.KEYS, np.uint64)
    h[0], h[700] = 5, 5                                                         # T lands on the last value of the end key
    out.append(h)
    h = h.copy()
    h[700] = 6                                                                  # ... and on the first value behind it
    out.append(h)
    return out


def test_photo_ratio_equals_the_model_bit_for_bit():
    fits = 0
    for h in _histograms():
        for min_count in (1, 256):
            got, want = L.photo_ratio(h, min_count), M.ratio(h, min_count)
            assert got[1] == want[1] and np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes(), (h.nonzero(), min_count)
            fits += got[1]
            if not got[1]:
                assert got[0] == 1.0
    assert fits > 20
    one = np.zeros(M.KEYS, np.uint64)
    one[513] = 1
    assert L.photo_ratio(one) == (float(M.EDGES[512]) + (float(M.EDGES[513]) - float(M.EDGES[512])) * 0.5, True)
    assert L.photo_ratio(one, min_count=2) == (1.0, False)
    r = C.c_double(5.0)
    assert core.lib().lfbm5d_photo_ratio(None, 1, C.byref(r)) == 1 and r.value == 1.0
    with pytest.raises(L.LfBm5dError):
        L.photo_ratio(np.zeros(1025, np.uint64))


def _layout(aw, ah, ang_radius=1, ang_major=V.ROWMAJOR):
    A = aw * ah
    mask = np.ones(A, np.uint32)
    nb = {}
    for m in range(A):
        missing = np.zeros(A, np.uint32)
        missing[m] = 1
        nb[m] = [q for q, _, _ in V.sources(m, mask, missing, ang_major, aw, ah, ang_radius)]
    return nb


@pytest.mark.parametrize("aw,ah", [(3, 3), (5, 5), (3, 1), (1, 3)])
def test_photo_solve_equals_the_model_bit_for_bit(aw, ah):
    A = aw * ah
    nb = _layout(aw, ah)
    rng = np.random.default_rng(aw * 10 + ah)
    g = rng.uniform(0.5, 1.5, A)
    r = np.array([g[m] / np.mean(g[nb[m]]) for m in range(A)]) * rng.uniform(0.999, 1.001, A)
    for unfit in (None, A - 1, 0):
        fitted = np.ones(A, bool)
        if unfit is not None:
            fitted[unfit] = False
        for anchor in (None, A // 2):
            got, want = L.photo_solve(r, nb, fitted, anchor), M.solve(r, nb, fitted, anchor)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (unfit, anchor)
            assert np.isfinite(got).all() and (got > 0).all()
            if unfit is not None:
                assert got[unfit] == 1.0
            if anchor is not None:
                assert got[anchor] == 1.0
            else:
                assert K.lower_median([got[m] for m in range(A) if fitted[m]]) == 1.0
    with pytest.raises(L.LfBm5dError):
        L.photo_solve(r, {m: [A] for m in range(A)}, np.ones(A, bool))            # a source out of range
    with pytest.raises(L.LfBm5dError):
        L.photo_solve(r, nb, np.ones(A, bool), anchor=A)


@pytest.mark.parametrize("aw,ah", [(3, 1), (1, 3), (3, 3)])
def test_the_solve_converges_and_recovers_the_gains(aw, ah):
    """On 1 x 3 and 3 x 1 the neighbour graph is bipartite (ends <-> middle): the undamped iteration g <- r mean(g) oscillates, the
    damped one settles.  With all three fitted, successive iterates differ by less than 1e-12 at S = 512."""
    A = aw * ah
    nb = _layout(aw, ah)
    g = np.linspace(0.6, 1.3, A)
    r = np.array([g[m] / np.mean(g[nb[m]]) for m in range(A)])
    trace = []
    got = M.solve(r, nb, np.ones(A, bool), None, trace=trace)
    assert len(trace) == M.SOLVE_STEPS == 512
    assert np.abs(np.array(trace[-1]) - np.array(trace[-2])).max() < 1e-12
    assert np.abs(got / got[0] * g[0] / g - 1.0).max() < 1e-9                    # the planted gains up to the free common factor
    assert np.array_equal(got, L.photo_solve(r, nb, np.ones(A, bool)))


def test_vignette_gains_and_apply_gains():
    g = synth.vignette_gains(3, 3, 0.6)
    assert np.allclose(g, [0.6, 0.8, 0.6, 0.8, 1.0, 0.8, 0.6, 0.8, 0.6], rtol=0, atol=1e-15)
    g = synth.vignette_gains(5, 3, 0.5).reshape(3, 5)
    assert g[1, 2] == 1.0 and np.allclose(g[[0, 0, 2, 2], [0, 4, 0, 4]], 0.5) and (np.diff(g[1, 2:]) < 0).all()
    assert np.array_equal(synth.vignette_gains(1, 1, 0.7), [1.0]) and np.array_equal(synth.vignette_gains(4, 2, 1.0), np.ones(8))
    with pytest.raises(ValueError):
        synth.vignette_gains(3, 3, 0.0)
    lf = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    out = synth.apply_gains(lf, [0.5, 1.1])
    assert out.dtype == np.float32 and np.array_equal(out[0], lf[0] * np.float32(0.5)) and np.array_equal(out[1], lf[1] * np.float32(1.1))
    out = synth.apply_gains(lf, [[1, 2, 3], [1, 1, 0.3]])
    assert np.array_equal(out[0, 2], lf[0, 2] * np.float32(3)) and np.array_equal(out[1, 2], lf[1, 2] * np.float32(0.3))
    assert np.array_equal(synth.apply_gains(lf.reshape(2, -1), [0.5, 1.1]), synth.apply_gains(lf, [0.5, 1.1]).reshape(2, -1))
    with pytest.raises(ValueError):
        synth.apply_gains(lf, [1.0, 2.0, 3.0])


def _rolled(aw, ah, n=64, step=2):
    """The golden centre view's middle n x n, rolled by `step` pixels per view: an exact integer translation (with wrap-around)."""
    base = np.load(GOLDEN)[4][:, 128 - n // 2:128 + n // 2, 128 - n // 2:128 + n // 2].astype(np.float32)
    return np.stack([np.roll(base, (step * (s - ah // 2), step * (t - aw // 2)), axis=(1, 2)) for s in range(ah) for t in range(aw)])


def _common_factor_removed(gain, planted):
    q = np.asarray(gain) / np.asarray(planted)
    return q / np.median(q)


@pytest.mark.parametrize("aw,ah", [(3, 3), (5, 5)])
def test_planted_gains_come_back_on_exact_translations(aw, ah):
    """A key is 0.2-0.4 % wide and the solve compounds a few of them; the prototype gave 0.13 % (3 x 3) and 0.31 % (5 x 5)."""
    A = aw * ah
    planted = synth.vignette_gains(aw, ah, 0.6)
    lf = synth.apply_gains(_rolled(aw, ah), planted)
    res = M.equalise(lf.reshape(A, -1), np.ones(A, np.uint32), V.ROWMAJOR, aw, ah, 64, 64, 3, D=3, r=2)
    err = np.abs(_common_factor_removed(res["gain"], planted[:, None]) - 1.0).max()
    print(f"{aw} x {ah}: {res['rounds']} sweeps, converged {res['converged']}, residual {res['residual']:.5f}, largest relative gain error {err:.5f}")
    assert err < 0.01
    assert res["fitted"] == A and list(res["state"]) == [M.FITTED] * A


def _golden_crop():
    return np.load(GOLDEN)[:, :, 64:160, 64:160].astype(np.float32)


def _consist_at_defaults(lf):
    P = L.consist_params()
    A, C_, H, W = lf.shape
    return K.consist(lf.reshape(A, -1), np.ones(A, np.uint32), V.ROWMAJOR, 3, 3, W, H, C_, D=P.max_disparity, r=P.box_radius,
                     ang_radius=P.ang_radius, k=P.k, min_threshold=P.min_threshold, spread=P.spread, min_sources=P.min_sources,
                     sai_factor=P.sai_factor, min_scale=P.min_scale, max_rounds=P.max_rounds)


def _equalise_at_defaults(lf):
    P = L.photo_params()
    A, C_, H, W = lf.shape
    return M.equalise(lf.reshape(A, -1), np.ones(A, np.uint32), V.ROWMAJOR, 3, 3, W, H, C_, D=P.max_disparity, r=P.box_radius,
                      ang_radius=P.ang_radius, steps=P.steps, min_sources=P.min_sources, max_rounds=P.max_rounds, tol=P.tol,
                      min_count=P.min_count, per_channel=P.per_channel, anchor=None, lo=P.lo, hi=P.hi)


def test_a_dimmed_view_is_no_longer_a_bad_view():
    """Golden rows and columns 64..159, SAI 5 times 0.5, no noise, everything at the shipped defaults: the consistency check calls
    SAI 5 bad before the equalisation and no SAI bad after it."""
    lf = synth.degrade_sai(_golden_crop(), 5, "dim")
    before = _consist_at_defaults(lf)
    res = _equalise_at_defaults(lf)
    after = _consist_at_defaults(res["out"].reshape(lf.shape))
    print(f"bad before {before['bad']} (s_5 {before['scale_sai'][5]:.1f}), after {after['bad']} (s_5 {after['scale_sai'][5]:.1f}); "
          f"gain of SAI 5 {res['gain'][5]}")
    assert before["bad"] == [5] and after["bad"] == []
    assert np.abs(res["gain"][5] / np.median(res["gain"][[0, 1, 2, 3, 4, 6, 7, 8]], axis=0) / 0.5 - 1.0).max() < 0.03


def test_a_vignette_no_longer_blinds_the_consistency_check():
    """The same crop under vignette_gains(edge=0.6): the largest per-SAI median residual after the equalisation is at most a quarter of
    the largest before (the prototype: 33.2 -> 2.3)."""
    lf = synth.apply_gains(_golden_crop(), synth.vignette_gains(3, 3, 0.6))
    before = _consist_at_defaults(lf)["trace"][0]["scale_sai"]
    res = _equalise_at_defaults(lf)
    after = _consist_at_defaults(res["out"].reshape(lf.shape))["trace"][0]["scale_sai"]
    print("s_m before " + " ".join(f"{before[m]:.1f}" for m in range(9)) + ", after " + " ".join(f"{after[m]:.1f}" for m in range(9)))
    assert max(after.values()) <= 0.25 * max(before.values())


def test_a_field_with_nothing_planted_is_left_alone():
    res = _equalise_at_defaults(_golden_crop())
    print(f"gains {res['gain_min']:.4f}..{res['gain_max']:.4f}, {res['rounds']} sweeps, residual {res['residual']:.5f}")
    assert np.abs(res["gain"] - 1.0).max() < 0.02 and res["gain_min"] == res["gain"].min() and res["gain_max"] == res["gain"].max()
