"""CPU tests of the per-view noise levels (include/lfbm5d_views.h): the host rule lfbm5d_views_window_sigma against the numpy model of
tests/views_model.py for every window of the plan, float bits equal; the uniform branch; lfbm5d_views_from_gains against the model; the
rejections; synth.add_view_noise against add_noise_mt19937.  Needs no GPU."""
import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth

import views_model as M


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _table(asize, seed):
    return np.random.default_rng(seed).uniform(3.0, 60.0, asize)


CASES = [
    # name, aheight, awidth, empty SAIs, major
    ("5x5", 5, 5, (), L.ROWMAJOR),
    ("7x9-holes", 7, 9, (0, 11, 40, 62), L.ROWMAJOR),
    ("7x9-holes-col", 7, 9, (0, 11, 40, 62), L.COLMAJOR),
    ("5x5-col", 5, 5, (), L.COLMAJOR),
]


@pytest.mark.parametrize("an", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_window_sigma_equals_the_model_on_every_window_of_the_plan(case, an):
    name, ah, aw, holes, major = case
    mask = np.ones(ah * aw, np.uint32)
    mask[list(holes)] = 0
    table = _table(ah * aw, 7)
    table[list(holes)] = np.nan                                      # entries of empty SAIs are ignored
    plan = core.plan_windows(aw, ah, an, major, mask)
    assert list(plan) == M.plan_windows(mask, aw, ah, an, major)
    want = M.window_sigmas(table, mask, aw, ah, an, major)
    got = []
    for pst in plan:
        ps, pt = M.coords(int(pst), aw, ah, major)
        got.append(L.window_sigma(table, aw, ah, ps, pt, an, major, mask))
    assert np.array_equal(_bits(got), _bits(want)), name
    assert len(plan) == 1 or len(set(_bits(want).tolist())) > 1       # the table does make the windows differ (5x5, an = 2: one window)
    # ... and on every SAI as a window centre, not only the plan's
    for st in range(ah * aw):
        ps, pt = M.coords(st, aw, ah, major)
        slots = M.window_slots(ps, pt, an, aw, ah, major)
        if not any(mask[s] for s in slots):
            continue
        assert _bits(L.window_sigma(table, aw, ah, ps, pt, an, major, mask)) == _bits(M.window_sigma(table, mask, ps, pt, an, aw, ah, major))


def test_uniform_table_returns_the_value_itself():
    """All values equal: (float)s, not the root mean square -- which differs from s for some doubles.  One is searched for here."""
    rng = np.random.default_rng(3)
    found = None
    for s in rng.uniform(1.0, 100.0, 20000):
        acc = np.float64(0.0)
        for _ in range(9):
            acc = acc + s * s
        r = np.sqrt(acc / np.float64(9.0))
        if r != s and np.float32(r) != np.float32(s):
            found = s
            break
    if found is None:                                                 # (float32 rounding hides most double differences: keep a double one)
        for s in rng.uniform(1.0, 100.0, 20000):
            acc = np.float64(0.0)
            for _ in range(9):
                acc = acc + s * s
            if np.sqrt(acc / np.float64(9.0)) != s:
                found = s
                break
    assert found is not None
    for s in (25.0, 10.0, found, float(np.nextafter(np.float32(25.0), np.float32(26.0))) + 1e-9):
        for an, aw, ah in ((1, 5, 5), (2, 7, 9), (1, 3, 3)):
            t = np.full(aw * ah, s)
            for ps, pt in ((0, 0), (ah // 2, aw // 2), (ah - 1, aw - 1)):
                assert _bits(L.window_sigma(t, aw, ah, ps, pt, an)) == _bits(np.float32(s)), (s, an, ps, pt)
    # uniform over the window's non-empty SAIs is enough: the one other value sits on an empty SAI
    t = np.full(9, 25.0)
    t[4] = 99.0
    mask = np.ones(9, np.uint32)
    mask[4] = 0
    assert L.window_sigma(t, 3, 3, 1, 1, 1, mask=mask) == np.float32(25.0)
    mask[4] = 1
    assert L.window_sigma(t, 3, 3, 1, 1, 1, mask=mask) == M.window_sigma(t, mask, 1, 1, 1, 3, 3, L.ROWMAJOR) != np.float32(25.0)


def test_views_from_gains_equals_the_model():
    rng = np.random.default_rng(5)
    for C_ in (1, 3):
        g = rng.uniform(0.4, 1.6, (63, C_))
        mask = np.ones(63, np.uint32)
        mask[[0, 11, 40, 62]] = 0
        g[0] = 0.0                                                    # a bad gain on an empty SAI is ignored
        got = L.views_from_gains(15.0, g, mask)
        want = M.from_gains(15.0, g, mask)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert (got[mask == 0] == 0).all() and (got[mask != 0] > 0).all()
    assert np.array_equal(L.views_from_gains(10.0, np.ones(9)), np.full(9, 10.0))
    v = L.views_from_gains(10.0, synth.vignette_gains(3, 3, 0.5))
    assert abs(v[0] - 20.0) < 1e-5 and v[4] == 10.0                   # half the brightness, twice the noise
    for bad in (np.nan, 0.0, -1.0, np.inf):
        g = np.ones((9, 3))
        g[5, 1] = bad
        with pytest.raises(L.LfBm5dError, match=r"gain\[5\]\[1\]"):
            L.views_from_gains(10.0, g)
    for bad in (np.nan, 0.0, -2.0, np.inf):
        with pytest.raises(L.LfBm5dError, match="sigma"):
            L.views_from_gains(bad, np.ones(9))


def test_bad_table_entries_are_rejected_with_the_sai_named():
    import ctypes as C
    lib = core.lib()
    mask = np.ones(25, np.uint32)
    out = C.c_float(-1.0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint)
    for bad in (np.nan, 0.0, -3.0, np.inf, -np.inf):
        t = np.full(25, 20.0)
        t[7] = bad
        rc = lib.lfbm5d_views_window_sigma(t.ctypes.data_as(dp), mask.ctypes.data_as(up), L.ROWMAJOR, 5, 5, 1, 1, 1, C.byref(out))
        assert rc == 1 and "sigma_sai[7]" in lib.lfbm5d_views_error().decode(), bad
        with pytest.raises(L.LfBm5dError, match=r"sigma_sai\[7\]"):
            L.window_sigma(t, 5, 5, 1, 1, 1, mask=mask)
        # ... only where the window holds the SAI, and not on an empty one
        assert L.window_sigma(t, 5, 5, 4, 4, 1, mask=mask) == np.float32(20.0)
        m2 = mask.copy()
        m2[7] = 0
        assert L.window_sigma(t, 5, 5, 1, 1, 1, mask=m2) == np.float32(20.0)
    t = np.full(25, 20.0)
    for kw, msg in ((dict(an=3), "larger than the light field"), (dict(ps=5), "outside"), (dict(ang_major=3), "ang_major")):
        args = dict(ps=1, pt=1, an=1, ang_major=L.ROWMAJOR)
        args.update(kw)
        with pytest.raises(L.LfBm5dError, match=msg):
            L.window_sigma(t, 5, 5, args["ps"], args["pt"], args["an"], args["ang_major"])
    with pytest.raises(L.LfBm5dError, match="no non-empty SAI"):
        L.window_sigma(t, 5, 5, 1, 1, 1, mask=np.zeros(25, np.uint32))
    assert lib.lfbm5d_views_window_sigma(None, None, L.ROWMAJOR, 5, 5, 1, 1, 1, C.byref(out)) == 1
    assert "NULL" in lib.lfbm5d_views_error().decode()


def test_add_view_noise_with_a_uniform_table_is_add_noise_mt19937():
    clean = synth.make_lf(3, 3, 24, 20).astype(np.float32)
    for seed in (1, 7):
        assert np.array_equal(synth.add_view_noise(clean, np.full(9, 25.0), seed=seed), synth.add_noise_mt19937(clean, 25.0, seed=seed))
    flat = clean.reshape(9, -1)
    assert np.array_equal(L.add_view_noise(flat, np.full(9, 10.0)), synth.add_noise_mt19937(flat, 10.0))
    # a table: every view's noise has its own level, and view v's draws do not depend on the other views' levels
    t = np.linspace(5.0, 45.0, 9)
    noisy = synth.add_view_noise(clean, t, seed=2)
    ref = synth.add_noise_mt19937(clean, 1.0, seed=2)
    for v in range(9):
        got = (noisy[v] - clean[v]).std()
        assert abs(got / t[v] - 1.0) < 0.1, (v, got)
        assert np.allclose(noisy[v] - clean[v], (ref[v] - clean[v]) * t[v], rtol=1e-4, atol=1e-3)
    with pytest.raises(ValueError):
        synth.add_view_noise(clean, np.ones(8))
