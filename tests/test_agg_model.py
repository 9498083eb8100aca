"""CPU tests of the aggregation model and of the cases the GPU test runs through the kernel (tests/agg_model.py, tests/agg_cases.py):
the model is a correct scatter, it does not depend on how a pass is cut into bands, every case respects the kernel's precondition,
and the census proves that every designated case reaches the path it was built for."""
import numpy as np
import pytest

import agg_cases as K
import agg_model as M
from oracle import oracle as O

CASES = K.template_cases() + K.special_cases() + [K.nonfinite_case()]
IDS = [c.name for c in CASES]
_model = {}


def model(case):
    """The float32 model of the whole pass as one launch (computed once per case)."""
    if case.name not in _model:
        g = case.g
        _model[case.name] = M.aggregate(g, case.num0, case.den0, K.patches_of(case), case.wgt, case.aggpos, M.kaiser_table(g.k))
    return _model[case.name]


def test_kaiser_tables_are_the_reference_ones():
    for k in (8, 12, 16, 6, 4, 2):
        w = np.zeros(k * k, np.float32)
        O.lib().orc_kaiser_window(w, k)
        assert np.array_equal(w, M.kaiser_table(k)), k


def test_case_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_positions_respect_the_search_reach(case):
    assert M.check_reach(case.g, case.aggpos, case.refs_yx) == 0
    present = sum(int((case.aggpos[st] != M.ABSENT).sum()) for st in M.live_slots(case.g))
    assert 0 < present < 2e5   # the model's loop is the cost of a case


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_agrees_with_a_float64_scatter(case):
    """rtol 1e-5.  den is a sum of terms of one sign (the weights are not negative), so the bound is relative to the sum itself.  num's
    terms have both signs and cancel: its bound is relative to the sum of their magnitudes -- the same scatter over |values| -- which
    is what float32 summation of a few hundred terms can be held to (error <= terms * 2^-24 * sum of magnitudes; 1e-5 allows 167)."""
    g = case.g
    pat, kai = K.patches_of(case), M.kaiser_table(g.k)
    n32, d32 = model(case)
    n64, d64 = M.aggregate(g, case.num0, case.den0, pat, case.wgt, case.aggpos, kai, dtype=np.float64)
    mag, _ = M.aggregate(g, np.abs(case.num0), case.den0, lambda gi, n, st: np.abs(pat(gi, n, st)), case.wgt, case.aggpos, kai, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(n64) & np.isfinite(d64) & np.isfinite(mag)
        assert np.array_equal(np.isnan(n32), np.isnan(n64)) and np.array_equal(np.isnan(d32), np.isnan(d64))
        assert np.array_equal(n32[~fin & ~np.isnan(n64)], n64[~fin & ~np.isnan(n64)].astype(np.float32))   # infinities: the same ones
        assert np.all(np.abs(d32[fin] - d64[fin]) <= 1e-5 * np.abs(d64[fin]))
        assert np.all(np.abs(n32[fin] - n64[fin]) <= 1e-5 * mag[fin])
    assert not np.array_equal(d32, case.den0)   # (something was added)


@pytest.mark.parametrize("case", [c for c in CASES if not c.g.irregular], ids=[c.name for c in CASES if not c.g.irregular])
def test_model_does_not_depend_on_the_bands(case):
    g = case.g
    pat, kai = K.patches_of(case), M.kaiser_table(g.k)
    num, den = case.num0, case.den0
    for rb, nb in K.row_bands(g, 2):
        num, den = M.aggregate(M.band(g, rb, nb), num, den, pat, case.wgt, case.aggpos, kai)
    n1, d1 = model(case)
    assert M.same_bits(num, n1).all() and M.same_bits(den, d1).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_census_reports_the_designed_path(case):
    g = case.g
    cen = M.census(g, case.aggpos)
    assert cen.n_tiles > 0
    assert cen.vec4 == (g.N % 4 == 0 and g.k < 12)
    assert not M.census(g, case.aggpos, scalar_scan=True).vec4
    for w in case.wants:
        if w == "not_small24":
            assert not cen.small24
        else:
            assert getattr(cen, w) > 0, (w, case.name)
    if "not_small24" not in case.wants:
        assert cen.small24
    if "n_exact_div" not in case.wants:
        assert cen.n_exact_div == 0
    if not cen.vec4:
        assert cen.n_overflow == 0          # the one-per-lane scan's round always fits
    # the bands' launches see every candidate the single launch sees: the hits add up
    if len(case.bands) > 1:
        total = sum(int(t.hits.sum()) for t in cen.tiles)
        parts = sum(int(t.hits.sum()) for rb, nb in case.bands for t in M.census(M.band(g, rb, nb), case.aggpos).tiles)
        assert parts == total


def test_census_of_the_overflow_case_in_detail():
    case = next(c for c in CASES if c.name == "overflow")
    cen = M.census(case.g, case.aggpos)
    assert (cen.cap, cen.round) == (256, 256)
    over = [t for t in cen.tiles if any(t.overflow)]
    # the designed sequence: a round with 1 .. 63 hits, then one with more hits than the room left
    assert any(0 < t.carry[j] < M.FLUSH and t.carry[j] + t.hits[j] > cen.cap for t in over for j in range(len(t.hits)) if t.overflow[j])
    exact = [t for t in cen.tiles if any(t.exact_fill)]
    assert any(t.carry[j] + t.hits[j] == cen.cap for t in exact for j in range(len(t.hits)) if t.exact_fill[j])
    # dense data alone never gets there: with every patch on its reference no round overflows
    refs = (case.refs_yx[:, 0] << 16 | case.refs_yx[:, 1]).astype(np.uint32)
    dense = np.broadcast_to(refs[None, :, None], case.aggpos.shape)
    assert M.census(case.g, dense).n_overflow == 0


def test_ragged_cases_put_patches_on_the_windows_rim():
    for case in (c for c in CASES if c.name.startswith(("ragged", "smallest"))):
        g = case.g
        p = np.concatenate([case.aggpos[st].reshape(-1) for st in M.live_slots(g) if st != g.pst]).astype(np.int64)
        py, px = p >> 16, p & 0xFFFF
        assert {0, g.Hb - g.k} <= set(py.tolist()) and {0, g.Wb - g.k} <= set(px.tolist()), case.name
    ragged = next(c for c in CASES if c.name == "ragged-k8")
    assert ragged.g.Wb % 8 and ragged.g.Hb % 8      # partial tiles on both axes


def test_template_grid_covers_every_instantiation():
    seen = {(M.tile_config(c.g.k), M.uses_vec4(c.g.k, c.g.N), c.g.C) for c in K.template_cases()}
    for k in (8, 12, 16, 6):
        for C in (1, 3):
            assert (M.tile_config(k), False, C) in seen
            assert ((M.tile_config(k), True, C) in seen) == (k < 12)
