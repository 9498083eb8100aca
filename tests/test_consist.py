"""CPU tests of the consistency check (lfbm5d_consist_*, include/lfbm5d.h): the exports, struct sizes and defaults, and the properties of
the numpy model (tests/consist_model.py) that pin the definition: a light field that is a pure translation per view is consistent, a
planted block is flagged exactly and throws no shadow on the other views, a bad SAI is the local maximum of the per-SAI scales and is
excluded in the second round, and the model's counts on the golden crop at the shipped defaults are the recorded ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import helpers
import consist_model as M
import view_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(k=8.0, min_threshold=0.0, spread=3.0, min_sources=2, sai_factor=2.0, min_scale=0.5, max_rounds=3)


def test_library_exports_and_binds_the_consist_entry_points():
    lib = core.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lfbm5d_consist_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["lfbm5d_consist_defaults", "lfbm5d_consist_device", "lfbm5d_consist_host_sai"]
    for n in declared:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n       # exported, and bound in core.py
    assert C.sizeof(core.ConsistParamsStruct) == 5 * 4 + 4 + 5 * 8               # five unsigned, padding, five doubles
    assert C.sizeof(core.ConsistResultStruct) == 3 * 8 + 3 * 8 + 6 * 8 + 2 * 8 + 4 * 4
    for n in ("ConsistParamsStruct", "ConsistResultStruct", "Consist", "consist_params", "consist"):
        assert n in L.__all__ and hasattr(L, n), n
    assert hasattr(L.Context, "consist") and hasattr(synth, "degrade_sai")
    assert M.Q == core.IMPULSE_KEYS == 386


def test_defaults_work_without_a_gpu_and_lie_in_the_allowed_ranges():
    P = L.consist_params()
    vp = L.view_params()
    assert (P.max_disparity, P.box_radius, P.ang_radius) == (vp.max_disparity, vp.box_radius, vp.ang_radius)   # the view synthesis' sweep
    assert 2 <= P.min_sources <= 24 and 1 <= P.max_rounds <= 64
    assert P.k > 0 and P.min_threshold >= 0 and P.spread >= 1 and P.sai_factor > 1 and P.min_scale >= 0
    P = L.consist_params(max_disparity=8, box_radius=0, ang_radius=2, min_sources=5, max_rounds=1, k=6, min_threshold=2, spread=2,
                         sai_factor=0, min_scale=1)
    assert (P.max_disparity, P.box_radius, P.ang_radius, P.min_sources, P.max_rounds) == (8, 0, 2, 5, 1)
    assert (P.k, P.min_threshold, P.spread, P.sai_factor, P.min_scale) == (6.0, 2.0, 2.0, 0.0, 1.0)


def test_degrade_sai():
    lf = helpers.textured_lf(3, 3, 24, 20, 1).astype(np.float32)
    for kind in ("dim", "noise", "shift"):
        out = synth.degrade_sai(lf, 4, kind, seed=3)
        assert out.dtype == np.float32 and out.shape == lf.shape
        sound = [i for i in range(9) if i != 4]
        assert np.array_equal(out[sound], lf[sound]) and not np.array_equal(out[4], lf[4])
        assert np.array_equal(out, synth.degrade_sai(lf, 4, kind, seed=3))
    assert np.array_equal(synth.degrade_sai(lf, 4, "dim")[4], lf[4] * np.float32(0.5))
    assert np.array_equal(synth.degrade_sai(lf, 4, "shift")[4], np.roll(lf[4], (7, 5), axis=(1, 2)))
    assert 0.0 <= synth.degrade_sai(lf, 0, "noise")[0].min() and synth.degrade_sai(lf, 0, "noise")[0].max() < 255.0
    with pytest.raises(ValueError):
        synth.degrade_sai(lf, 4, "bogus")


def _translation(disparity, ah=3, aw=3, H=48, W=40):
    return helpers.textured_lf(ah, aw, H, W, disparity).astype(np.float32)


@pytest.mark.parametrize("disparity", [1, 2, 3])
def test_pure_translation_is_consistent(disparity):
    D, r = 3, 3
    lf = _translation(disparity)
    res = M.consist(lf.reshape(9, -1), np.ones(9, np.uint32), V.ROWMAJOR, 3, 3, 40, 48, 3, D=D, r=r, **KW)
    b = D + r
    assert not res["flags"].reshape(9, 3, 48, 40)[:, :, b:-b, b:-b].any()        # away from the border the prediction is the view
    assert res["bad"] == [] and res["rounds"] == 1 and res["untested"] == [] and list(res["state"]) == [M.TESTED] * 9
    assert res["pixels"] == 9 * 3 * 48 * 40 and res["skipped"] == 0 and int(res["hist"].sum()) == res["pixels"]


@pytest.mark.parametrize("spread", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("st", [4, 0, 1], ids=["centre", "corner", "edge"])
def test_a_planted_block_is_flagged_exactly_and_throws_no_shadow(st, spread):
    """The block is the view plus 15 grey levels.  The derivation of the spread test (next test) takes the neighbours' d* as given: a
    defect delta in one source adds delta^2 (n - 1) / n per covered pixel of the box to E at the true d and about as much at a wrong one,
    so it cannot move d* as long as that stays below what the photograph's own mismatch costs at a wrong d (some hundreds per pixel and
    channel here); 15^2 = 225 does, and the test asserts that premise.  A block that does move d* is another matter and a documented
    limit: written as 255 - value it leaves 436 / 207 / 51 shadow values flagged around the centre SAI's block at
    spread 1 / 2 / 3 (corner SAI: 61 / 5 / 0), all of them at positions whose d* it changed."""
    D, r = 3, 3
    lf = _translation(2)
    clean = M.consist(lf.reshape(9, -1), np.ones(9, np.uint32), V.ROWMAJOR, 3, 3, 40, 48, 3, D=D, r=r, **dict(KW, spread=spread))
    lf[st, :, 20:25, 16:21] += 15.0
    res = M.consist(lf.reshape(9, -1), np.ones(9, np.uint32), V.ROWMAJOR, 3, 3, 40, 48, 3, D=D, r=r, **dict(KW, spread=spread))
    f = res["flags"].reshape(9, 3, 48, 40)
    b = D + r
    assert np.array_equal(res["disp"].reshape(9, 48, 40)[:, b:-b, b:-b], clean["disp"].reshape(9, 48, 40)[:, b:-b, b:-b])   # the premise
    inner = f[:, :, b:-b, b:-b]
    want = np.zeros_like(f)
    want[st, :, 20:25, 16:21] = 1
    assert np.array_equal(inner, want[:, :, b:-b, b:-b])                        # the block, all of it, in that SAI only
    assert res["bad"] == []


def test_the_shadow_of_a_neighbours_defect_fails_the_spread_test():
    """A defect delta in one source of n moves the mean by delta / n: rho = -delta / n, v = delta^2 (n - 1) / n, so
    rho^2 (n - 1) / (spread^2 v) = 1 / (n spread^2): no spread >= 1 flags the shadow, for any n and delta."""
    for aw, ah, m in ((3, 3, 4), (3, 3, 0), (3, 1, 1), (5, 5, 12)):      # n = 8, 3, 2, 24
        for delta in (3.0, 100.0, -155.0):
            A = aw * ah
            x = np.full((A, 1, 6, 6), 100.0, np.float32)
            mask = np.ones(A, np.uint32)
            missing = np.zeros(A, np.uint32)
            missing[m] = 1
            R = 2 if A == 25 else 1
            srcs = V.sources(m, mask, missing, V.ROWMAJOR, aw, ah, R)
            n = len(srcs)
            x[srcs[-1][0], 0, 3, 3] += np.float32(delta)                         # the defect sits in a source of m
            mu, disp, v = M.predict(x, srcs, 0, 0)
            rho = float(x[m, 0, 3, 3] - mu[0, 3, 3])
            assert abs(rho + delta / n) < 1e-4 * abs(delta) and abs(float(v[0, 3, 3]) - delta * delta * (n - 1) / n) < 1e-3 * delta * delta
            ratio = rho * rho * (n - 1) / float(v[0, 3, 3])
            assert abs(ratio - 1.0 / n) < 1e-4
            for spread, flagged in ((1.0, False), (3.0, False), (0.9 / np.sqrt(n), True)):   # below 1 / sqrt(n) the test lets it through
                res = M.consist(x.reshape(A, -1), mask, V.ROWMAJOR, aw, ah, 6, 6, 1, D=0, r=0, ang_radius=R,
                                **dict(KW, spread=spread, k=0.0, sai_factor=0.0))
                assert bool(res["flags"][m].reshape(6, 6)[3, 3]) == flagged, (n, delta, spread)
                if res["state"][srcs[-1][0]] == M.TESTED:                          # (the end of a 1 x 3 field is not)
                    assert res["flags"][srcs[-1][0]].reshape(6, 6)[3, 3] == 1     # the defect itself is flagged in its own SAI


@pytest.mark.parametrize("st", [12, 2, 0], ids=["centre", "edge", "corner"])
def test_a_noise_sai_alone_is_bad(st):
    lf = synth.degrade_sai(_translation(1, 5, 5, 40, 36), st, "noise", seed=st + 1)
    res = M.consist(lf.reshape(25, -1), np.ones(25, np.uint32), V.ROWMAJOR, 5, 5, 36, 40, 3, D=2, r=2, **KW)
    assert res["bad"] == [st] and res["rounds"] == 2 and res["state"][st] == M.BAD
    first, second = res["trace"]
    s, t = V.coords(st, V.ROWMAJOR, 5, 5)
    neighbours = [q for q in range(25) if q != st and max(abs(V.coords(q, V.ROWMAJOR, 5, 5)[0] - s), abs(V.coords(q, V.ROWMAJOR, 5, 5)[1] - t)) <= 1]
    assert set(neighbours) <= set(first["exceeds"]) and first["bad"] == [st]    # contaminated by about delta / n, but not bad
    assert all(first["scale_sai"][q] < first["scale_sai"][st] for q in neighbours)
    assert list(np.nonzero(second["exclude"])[0]) == [st] and second["bad"] == [] and second["exceeds"] == []
    assert not res["flags"][st].any() and res["scale_sai"][st] == first["scale_sai"][st]
    assert sorted(res["tested"] + [st]) == list(range(25))


def test_rounds_sources_and_non_finite_values():
    lf = synth.degrade_sai(_translation(1, 5, 5, 40, 36), 12, "noise", seed=1).reshape(25, -1)
    mask = np.ones(25, np.uint32)
    off = M.consist(lf, mask, V.ROWMAJOR, 5, 5, 36, 40, 3, D=2, r=2, **dict(KW, sai_factor=0.0))
    assert off["rounds"] == 1 and off["bad"] == [] and off["state"][12] == M.TESTED     # the decision is off: one sweep
    one = M.consist(lf, mask, V.ROWMAJOR, 5, 5, 36, 40, 3, D=2, r=2, **dict(KW, max_rounds=1))
    assert one["rounds"] == 2 and one["bad"] == [12] and len(one["trace"]) == 2          # the last decision found one: one more sweep
    given = np.zeros(25, np.uint32)
    given[12] = 1
    ex = M.consist(lf, mask, V.ROWMAJOR, 5, 5, 36, 40, 3, D=2, r=2, exclude=given, **KW)
    assert ex["rounds"] == 1 and ex["bad"] == [] and ex["state"][12] == M.EXCLUDED
    assert np.array_equal(ex["flags"], one["flags"]) and np.array_equal(ex["hist"], one["hist"])   # the same final sweep
    # 1 x 3 views: the ends have one source
    line = _translation(1, 1, 3, 20, 24).reshape(3, -1)
    res = M.consist(line, np.ones(3, np.uint32), V.ROWMAJOR, 3, 1, 24, 20, 3, D=1, r=1, **KW)
    assert res["untested"] == [0, 2] and res["tested"] == [1] and list(res["state"]) == [M.UNTESTED, M.TESTED, M.UNTESTED]
    assert not res["flags"][[0, 2]].any() and res["pixels"] == 3 * 20 * 24
    all3 = M.consist(line, np.ones(3, np.uint32), V.ROWMAJOR, 3, 1, 24, 20, 3, D=1, r=1, **dict(KW, min_sources=3))
    assert all3["tested"] == [] and all3["untested"] == [0, 1, 2] and all3["pixels"] == 0 and not all3["flags"].any()
    # a value that is not finite: code 2, counted in skipped, not in the histogram
    x = _translation(1).copy()
    x[4, 1, 20, 20] = np.nan
    x[4, 2, 21, 20] = np.inf
    res = M.consist(x.reshape(9, -1), np.ones(9, np.uint32), V.ROWMAJOR, 3, 3, 40, 48, 3, D=1, r=1, **KW)
    f = res["flags"].reshape(9, 3, 48, 40)
    assert f[4, 1, 20, 20] == 2 and f[4, 2, 21, 20] == 2 and (f == 2).sum() == 2
    assert res["skipped"] == 2 and int(res["hist"].sum()) == res["pixels"] - 2 and list(res["counts"][:, 1]) == [0, 1, 1]


def test_both_angular_orders():
    ah, aw, H, W = 2, 3, 21, 40
    lf = _translation(2, ah, aw, H, W)
    lf[1, :, 8:11, 20:23] = 0.0
    row = M.consist(lf.reshape(6, -1), np.ones(6, np.uint32), V.ROWMAJOR, aw, ah, W, H, 3, D=3, r=2, **KW)
    perm = [(st % ah) * aw + st // ah for st in range(6)]                       # column-major index -> row-major index
    col = M.consist(lf[perm].reshape(6, -1), np.ones(6, np.uint32), V.COLMAJOR, aw, ah, W, H, 3, D=3, r=2, **KW)
    assert np.array_equal(col["flags"], row["flags"][perm]) and np.array_equal(col["disp"], row["disp"][perm])
    assert np.array_equal(col["hist"], row["hist"][perm]) and np.array_equal(col["counts"], row["counts"])
    assert col["scale_channel"] == row["scale_channel"] and row["flags"][1].any()


def _recorded_row():
    txt = open(os.path.join(ROOT, "profiles", "consist_defaults.txt")).read()
    m = re.search(r"^shipped: k = ([0-9.]+), spread = ([0-9.]+), min_sources = (\d+), sai_factor = ([0-9.]+), min_scale = ([0-9.]+); golden crop "
                  r"clean, add_defects\(seed=2\) as 0 / 255: flagged (\d+), true hits (\d+), false hits (\d+), bad SAIs \[([0-9, ]*)\]$", txt, re.M)
    assert m, "profiles/consist_defaults.txt has no shipped row"
    return m.groups()


def test_the_models_counts_on_the_golden_crop_at_the_shipped_defaults():
    """Golden rows and columns 64..191, add_defects(seed=2) written as 0 or 255 (whichever is farther from the value), at the library's
    defaults: the model is deterministic, so flagged, true hits, false hits and the bad SAIs equal the row recorded by
    tools/consist_sweep.py."""
    k, spread, min_sources, sai_factor, min_scale, flagged, hits, false, bad = _recorded_row()
    P = L.consist_params()
    assert (P.k, P.spread, P.min_sources, P.sai_factor, P.min_scale) == (float(k), float(spread), int(min_sources), float(sai_factor), float(min_scale))
    clean = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy"))[:, :, 64:192, 64:192].astype(np.float32)
    fl = synth.add_defects(clean.shape, seed=2)
    y = np.where(fl, np.where(clean > 127.0, np.float32(0.0), np.float32(255.0)), clean).astype(np.float32)
    res = M.consist(y.reshape(9, -1), np.ones(9, np.uint32), V.ROWMAJOR, 3, 3, 128, 128, 3, D=P.max_disparity, r=P.box_radius,
                    ang_radius=P.ang_radius, k=P.k, min_threshold=P.min_threshold, spread=P.spread, min_sources=P.min_sources,
                    sai_factor=P.sai_factor, min_scale=P.min_scale, max_rounds=P.max_rounds)
    got = res["flags"].reshape(clean.shape) != 0
    print(f"flagged {int(got.sum())}, true hits {int((got & fl).sum())}, false hits {int((got & ~fl).sum())}, bad {res['bad']}")
    assert (int(got.sum()), int((got & fl).sum()), int((got & ~fl).sum())) == (int(flagged), int(hits), int(false))
    assert res["bad"] == [int(v) for v in bad.replace(" ", "").split(",") if v]
