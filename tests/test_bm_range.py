"""Block matching across its search range and at its smallest windows (CPU): the streaming form of the exact model against the
dense one on every tie case, the census of tests/bm_range_cases.py (every tag proven on its case, every tag used), exact_domain
on every plane, and the oracle against the int64 model on every integer case -- idx[:cnt], cnt, best and shape over the whole
region(), no position excluded.  That the reference side holds at nSim = 48 and nDisp = 24 is settled here, before the GPU is asked
(tests/test_gpu_bm_range.py)."""
import numpy as np
import pytest

import bm_range_cases as Rc
import bm_tie_cases as Ts
import bm_tie_census as Census
import bm_tie_model as M


@pytest.mark.parametrize("name", Ts.IDS)
def test_streaming_model_equals_dense_model(name):
    c = Ts.by_name(name)
    N, nSim, nDisp, k, p = c[5][:5]
    b, dense = Ts.build(name), Ts.model(name)
    Hb, Wb, nHW, Ns = b["Hb"], b["Wb"], nSim + nDisp, 2 * nSim + 1
    s, rows = M.self_search_stream(b["est"][b["cc"]], k, N, nSim, nDisp, b["tau"], dense["refs"])
    assert sorted(s) == sorted(dense["self"])
    for key, v in dense["self"].items():
        assert s[key].dtype == v.dtype and np.array_equal(s[key], v), key
    # the score rows: 0 at the patch itself, 2 * threshold exactly where the scored position lies outside the band, and the
    # selection recomputed from the rows alone (forward test value = own entry, backward = the mirrored entry) gives n_pass
    thr = M.threshold(b["tau"], k)
    refs = dense["refs"].astype(np.int64)
    e = np.arange(Ns * Ns)
    djp, r = e // Ns - nSim, e % Ns
    dip = np.where(r <= nSim, r, r - Ns)
    y, x = refs[:, None] // Wb + np.where(dip < 0, dip, 0)[None, :], refs[:, None] % Wb + np.where(dip < 0, djp, 0)[None, :]
    outside = ~((y >= nHW) & (y < Hb - nHW) & (x >= nHW) & (x < Wb - nHW))
    assert (rows[outside] == 2 * thr).all() and outside.any() and (rows[:, nSim * Ns] == 0).all() and rows.min() >= 0
    mirror = (-djp + nSim) * Ns + (-dip)
    tests = np.where((dip >= 0)[None, :], rows, rows[:, np.where(dip < 0, mirror, 0)])
    ok = tests < thr
    assert np.array_equal(ok.sum(1), dense["self"]["n_pass"])
    order = np.argsort(np.where(ok, rows, M.BIG), axis=1, kind="stable")          # the selection again, from the rows alone
    pos = refs[:, None] + dip[None, :] * Wb + djp[None, :]
    for i in range(len(refs)):
        n = int(dense["self"]["cnt"][i]) if dense["self"]["n_pass"][i] > 1 else 1
        assert np.array_equal(pos[i, order[i, :n]], dense["self"]["idx"][i, :n]), (name, i)


def test_census_tags_hold_and_every_tag_occurs():
    used = set()
    for c in Rc.CASES:
        g = Rc.geometry(c)
        N, nSim, nDisp, k, p = c["pk"][:5]
        assert c["Hb"] >= Rc.wmin(nSim, nDisp, k) and c["Wb"] >= Rc.wmin(nSim, nDisp, k), c["name"]     # pass_impl accepts the window
        assert 1 <= nSim <= 48 and 1 <= nDisp <= 24 and g["scores_bytes"] < 20e6, c["name"]              # validate() does; table size
        for t in c["tags"]:
            assert Rc.TAGS[t](g), (c["name"], t, g)
        used |= set(c["tags"])
    assert used == set(Rc.TAGS), set(Rc.TAGS) ^ used
    print()
    for c in Rc.CASES:
        print(Rc.census_line(c))


def test_census_covers_the_issue_s_geometry():
    """What the case table has to contain, stated on the census numbers (not on names)."""
    G = {c["name"]: Rc.geometry(c) for c in Rc.CASES}
    sel = [g for n, g in G.items() if Rc.by_name(n)["group"] == "selection"]
    assert sorted(g["nSim"] for g in sel) == [1, 2, 4, 7, 10, 11, 15, 16, 19, 22] and {g["ROWS"] for g in sel} == {1, 2, 4, 8, 16, 22, 32}
    kss = [g for n, g in G.items() if Rc.by_name(n)["group"] == "k_self_select"]
    assert sorted((g["nSim"], g["k"], g["p"]) for g in kss) == [(23, 8, 3), (30, 8, 5), (32, 8, 3), (44, 8, 3), (45, 8, 3), (48, 8, 3), (48, 16, 3)]
    assert max(g["select_lds"] for g in kss) == 75272 and all(not g["regs"] for g in kss)
    dis = [g for n, g in G.items() if Rc.by_name(n)["group"] == "disparity"]
    assert {g["nDisp"] for g in dis if g["k"] == 8} == {1, 4, 5, 7, 12, 24}
    assert {(g["nDisp"], g["scan_version"]) for g in dis if g["k"] == 16} == {(16, 3), (17, 1)}
    mins = [g for g in G.values() if g["Hb"] == g["Wb"] == Rc.wmin(g["nSim"], g["nDisp"], g["k"])]
    assert sorted((g["nSim"], g["nDisp"], g["k"]) for g in mins) == sorted([(1, 1, 8), (3, 2, 16), (6, 6, 8), (18, 6, 8), (2, 1, 12), (2, 1, 4), (1, 1, 32)])
    edges = [g for n, g in G.items() if Rc.by_name(n)["group"] == "edges"]
    for k in (8, 16):
        assert {g["self_cols"] for g in edges if g["k"] == k} >= {65, 66, 129} and {g["disp_cols"] for g in edges if g["k"] == k} >= {65, 66, 129}
        assert {g["disp_row_rem"] for g in edges if g["k"] == k} == {0, 15}
    assert any(g["slots"] == 24 and g["nDisp"] == 12 for g in G.values())


def test_data_tags():
    """By the exact model alone: within the nSim >= 23 group every passing-candidate class the selection kernel treats differently
    occurs, with ties at the cut and tied disparity minima; the same over the register-resident instantiations."""
    for group in ("k_self_select", "selection"):
        reached = set()
        for c in Rc.CASES:
            if c["group"] == group:
                reached |= Rc.data_tags(c["name"])
        assert reached >= Rc.SELECTION_CLASSES | {"tie-cut", "tie-disp"}, (group, reached)
    top = Rc.data_tags("kss-nsim48-k8-p3")          # the largest window by itself
    assert top >= {"2..64", "65..128", ">128", "<N,not-pow2", "tie-cut"}, top
    assert all("tie-disp" in Rc.data_tags(c["name"]) for c in Rc.CASES if c["group"] == "disparity")


def _planes():
    for c in Rc.CASES:
        yield c["name"], Rc.build(c["name"])["est"], c["pk"][3]
    for s in Rc.SUBSET:
        yield s["name"], Rc.integer_planes(s["kind"], 3, s["Hb"], s["Wb"], s["pk"][3]), s["pk"][3]
    b = Rc.BM3D
    yield b["name"], Rc.integer_planes(b["kind"], 3, b["side"], b["side"], b["k"])[4:5], b["k"]


def test_every_plane_is_in_the_exact_domain():
    for name, est, k in _planes():
        for a in range(est.shape[0]):
            R = M.exact_domain(est[a], k)
            assert R > 0, name
        if k == 32:
            assert R <= 63


@pytest.mark.parametrize("name", Rc.IDS)
def test_oracle_equals_exact_model(name):
    c = Rc.by_name(name)
    N, nSim, nDisp, k, p = c["pk"][:5]
    b, m = Rc.build(name), Rc.model(name)
    idx, cnt, disp = Census.oracle_tables(b["est"], b["cc"], k, N, nSim, nDisp, b["tau"], m["refs"], views=Rc.views_of(b))
    assert np.array_equal(cnt, m["self"]["cnt"])
    used = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    assert np.array_equal(np.where(used, idx, 0), np.where(used, m["self"]["idx"], 0))
    assert sorted(disp) == sorted(m["disp"]) == Rc.views_of(b)
    rows, cols = M.region(b["Hb"], b["Wb"], k, nDisp)
    for st, (best, shape) in disp.items():
        assert best.shape == (rows.stop - rows.start, cols.stop - cols.start)
        assert np.array_equal(best, m["disp"][st]["best"]), st
        assert np.array_equal(shape, m["disp"][st]["shape"]), st


def test_oracle_equals_exact_model_on_the_bm3d_plane():
    """The per-SAI BM3D flavour: search band = search window (nDisp = 0), nHard = 48 on the smallest image for it."""
    from oracle import oracle as O
    b = Rc.BM3D
    est = Rc.integer_planes(b["kind"], 3, b["side"], b["side"], b["k"])[4]
    refs, s, _ = Rc.bm3d_model()
    idx, cnt = np.zeros((len(refs), b["N"]), np.uint32), np.zeros(len(refs), np.uint32)
    assert O.lib().orc_bm_self(np.ascontiguousarray(est.reshape(-1)), b["side"], b["side"], b["k"], b["N"], b["nHard"], b["nHard"],
                               Rc.bm3d_tau(), refs, len(refs), idx.reshape(-1), cnt) == 0
    used = np.arange(b["N"])[None, :] < cnt[:, None]
    assert np.array_equal(cnt, s["cnt"]) and np.array_equal(np.where(used, idx, 0), np.where(used, s["idx"], 0))
    assert len(refs) == 4 and len(set(s["n_pass"].tolist())) > 1
