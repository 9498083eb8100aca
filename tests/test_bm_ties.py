"""Block matching on EXACT ties (CPU): the oracle against the int64 model on quantised, saturated, flat and periodic planes --
every reference patch, every position of the compared region, every non-centre view, no `clear` mask and no skipped case
(tests/test_oracle_pins.py, on float data, has to skip exactly those) -- the conditions that make the case list a tie test at
all, and the tie census (tests/bm_tie_census.py).  The GPU side of the same cases: tests/test_gpu_bm_ties.py."""
import numpy as np
import pytest

import bm_tie_cases as Cs
import bm_tie_census as Census
import bm_tie_model as M


@pytest.mark.parametrize("name", Cs.IDS)
def test_oracle_equals_exact_model(name):
    c = Cs.by_name(name)
    N, nSim, nDisp, k, p = c[5][:5]
    b, m = Cs.build(name), Cs.model(name)
    idx, cnt, disp = Census.oracle_tables(b["est"], b["cc"], k, N, nSim, nDisp, b["tau"], m["refs"])
    assert np.array_equal(cnt, m["self"]["cnt"])
    used = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    assert np.array_equal(np.where(used, idx, 0), np.where(used, m["self"]["idx"], 0))
    assert sorted(disp) == sorted(m["disp"]) and len(disp) == b["A"] - 1
    for st, (best, shape) in disp.items():
        assert np.array_equal(best, m["disp"][st]["best"]), st
        assert np.array_equal(shape, m["disp"][st]["shape"]), st


def test_flat_plane_selects_scan_order_zero_everywhere():
    """Every candidate of a flat plane ties at 0: the disparity winner is scan order 0, displacement (-nDisp, -nDisp), and the
    self-search of a reference whose search window lies in the band takes the first N candidates of the scan: dj = -nSim,
    di = 0 .. nSim, then -nSim, ..."""
    for name in ("flat-k8-nsim5", "flat-k16-nsim6-nd3"):
        c = Cs.by_name(name)
        N, nSim, nDisp, k, p = c[5][:5]
        b, m = Cs.build(name), Cs.model(name)
        Hb, Wb = b["Hb"], b["Wb"]
        rows, cols = M.region(Hb, Wb, k, nDisp)
        pos = np.arange(Hb * Wb).reshape(Hb, Wb)[rows, cols]
        for st, d in m["disp"].items():
            assert np.array_equal(d["best"], pos - nDisp * Wb - nDisp) and d["shape"].all() and d["tie_min"].all()
        refs = m["refs"].astype(np.int64)
        nHW = nSim + nDisp
        ri, rj = refs // Wb, refs % Wb       # backward candidates outside the band score 2 * threshold: interior references only
        inner = (ri >= nHW + nSim) & (ri < Hb - nHW - nSim) & (rj >= nHW + nSim) & (rj < Wb - nHW - nSim)
        di = np.array((list(range(0, nSim + 1)) + list(range(-nSim, 0)))[:N])
        assert inner.any() and np.array_equal(m["self"]["idx"][inner], refs[inner, None] - nSim + Wb * di[None, :])


def test_case_conditions():
    """Conditions on the INPUTS, by the model alone: tie shares of the natural cases, a tested value on the threshold, and every
    class of passing-candidate count the selection kernel treats differently."""
    reached = set()
    for c in Cs.CASES:
        name, kind, N, nSim = c[0], c[1], c[5][0], c[5][1]
        m = Cs.model(name)
        s = m["self"]
        if kind in Cs.NATURAL:
            assert s["tie_cut"].mean() >= 0.01, (name, s["tie_cut"].mean())
            tied = np.concatenate([d["tie_min"].reshape(-1) for d in m["disp"].values()])
            assert tied.mean() >= 0.10, (name, tied.mean())
        if kind == "threq":
            assert s["thr_equal"].any(), name
            assert (s["n_pass"] < (2 * nSim + 1) ** 2).any() and (s["n_pass"] > 1).all()        # both sides of the strict <
        reached |= Cs.path_classes(s["n_pass"], N)
    assert reached == {"<N,not-pow2", "1", "2..64", "65..128", ">128"}, reached
    assert any(c[5][1] == 18 and (Cs.model(c[0])["self"]["n_pass"] > 128).any() for c in Cs.CASES)     # the README's nSim


@pytest.fixture(scope="module")
def census():
    return Census.rows()


def test_census_orders_agree_where_the_model_sees_no_tie(census):
    """Asserted: only what follows from the definition.  Without two equal scores among the nSx + 1 best, partial_sort has one
    possible outcome; without a tie at the cut, one possible set; a minimum attained once is found by any sort."""
    exact = 0
    for label, row, masks in census:
        assert row["set"] + row["order"] <= row["refs"] and row["disp"] <= row["positions"]
        if masks is None:
            continue
        exact += 1
        assert not masks["seq"][~masks["tie_any"]].any(), label
        assert not masks["sets"][~masks["tie_cut"]].any(), label
        for st, (tie, diff) in masks["disp"].items():
            assert not diff[~tie].any(), (label, st)
    assert exact >= 5 + sum(c[1] in Cs.NATURAL for c in Cs.CASES)
    print("\n" + Census.fmt(census))


def test_census_switch_is_off_by_default_and_restored(census):
    from oracle import oracle as O
    name = "q16-k8-ht"
    c = Cs.by_name(name)
    N, nSim, nDisp, k, p = c[5][:5]
    b, m = Cs.build(name), Cs.model(name)
    idx, cnt, _ = Census.oracle_tables(b["est"], b["cc"], k, N, nSim, nDisp, b["tau"], m["refs"], views=())
    assert np.array_equal(idx, m["self"]["idx"]) and m["self"]["tie_any"].any()
    O.lib().orc_set_tie_order(1)
    O.lib().orc_set_tie_order(0)
    idx2, _, _ = Census.oracle_tables(b["est"], b["cc"], k, N, nSim, nDisp, b["tau"], m["refs"], views=())
    assert np.array_equal(idx, idx2)
