"""Block matching across its whole search range and at its smallest windows (GPU): one core pass per case of
tests/bm_range_cases.py on a greyscale window (channel 0 of the input is the matching estimate), then everything the context reads
back against the int64 model, bit for bit and with no position excluded -- refs, self_idx[:cnt], self_cnt, best and shape of every
non-centre SAI over region(), the whole score table (2 * threshold entries included) and the generation of the table kernel the
census predicts.  The float twin of every case against the oracle; a named subset again under every alternative form; the subset
pass at nSim = 22 and 30; the per-SAI BM3D step at nHard = 48; the refusals past the range.  tests/test_bm_range.py holds the
oracle to the model on the same cases.  Every test prints one result line (profiles/bm_range.txt)."""
import functools

import numpy as np
import pytest
import torch

import bm_range_cases as Rc
import bm_tie_census as Census
import bm_tie_model as M
import helpers as Hh
from oracle import oracle as O
from test_gpu_parity import gpu_pass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def _pass(ctx, name, twin=False):
    """One default-geometry pass of a case: dict(refs, idx (unused entries zeroed), cnt, best / shape {st: region}, scores, version)."""
    c = Rc.by_name(name)
    N, nSim, nDisp, k, p = c["pk"][:5]
    b = Rc.build(name, twin)
    Wb, Hb, A, cc = b["Wb"], b["Hb"], b["A"], b["cc"]
    win = np.ascontiguousarray(b["est"].reshape(A, -1))
    gpu_pass(ctx, 1, c["sigma"], c["pk"], win, None, Wb, Hb, 1, mask=b["mask"], cst=cc, pst=cc, aw=c["aw"])
    version = ctx.last_scan_version()
    refs, idx, cnt, best, shape = ctx.last_bm(N, A, Wb * Hb)
    ncand = (2 * nSim + 1) ** 2
    scores = ctx.last_scores(len(refs) * ncand)
    assert scores.size == len(refs) * ncand
    used = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    rows, cols = M.region(Hb, Wb, k, nDisp)
    return dict(refs=refs, idx=np.where(used, idx, 0), cnt=cnt, scores=scores.reshape(len(refs), ncand), version=version,
                best={st: best[st].reshape(Hb, Wb)[rows, cols].copy() for st in Rc.views_of(b)},
                shape={st: shape[st].reshape(Hb, Wb)[rows, cols].copy() for st in Rc.views_of(b)})


def _same_tables(name, got, want, scores=True):
    """got, want: dicts of _pass (or the model's / oracle's in that form)."""
    assert np.array_equal(got["refs"], want["refs"]), name
    assert np.array_equal(got["cnt"], want["cnt"]), (name, np.argwhere(got["cnt"] != want["cnt"])[:4].tolist())
    bad = np.argwhere(got["idx"] != want["idx"])
    assert len(bad) == 0, (name, len(bad), bad[:4].tolist())
    assert sorted(got["best"]) == sorted(want["best"]) and len(got["best"]) > 0
    for st in want["best"]:
        gb, wb = got["best"][st], want["best"][st]
        assert gb.shape == wb.shape and np.array_equal(gb, wb), (name, st, int((gb != wb).sum()), np.argwhere(gb != wb)[:4].tolist())
        assert np.array_equal(got["shape"][st], want["shape"][st]), (name, st, int((got["shape"][st] != want["shape"][st]).sum()))
    if scores:
        gs, ws = got["scores"], want["scores"]
        assert gs.shape == ws.shape and gs.dtype == ws.dtype == np.float32
        bad = np.argwhere(gs.view(np.uint32) != ws.view(np.uint32))
        assert len(bad) == 0, (name, len(bad), bad[:4].tolist())


@functools.lru_cache(maxsize=None)
def _model_tables(name):
    m = Rc.model(name)
    used = np.arange(m["self"]["idx"].shape[1])[None, :] < m["self"]["cnt"][:, None]
    assert np.array_equal(m["rows"].astype(np.float32).astype(np.int64), m["rows"])       # (2 thr at k = 32 is above 2^24, and a float32)
    return dict(refs=m["refs"], idx=np.where(used, m["self"]["idx"], 0), cnt=m["self"]["cnt"], scores=m["rows"].astype(np.float32),
                best={st: d["best"] for st, d in m["disp"].items()}, shape={st: d["shape"] for st, d in m["disp"].items()})


def _line(name, form, r, against):
    print(f"\n{name:26s} {form:16s} scan=v{r['version']} refs={len(r['refs']):<5d} sum(cnt)={int(r['cnt'].sum()):<6d} views={len(r['best'])} "
          f"positions={sum(v.size for v in r['best'].values()):<7d} scores={r['scores'].size:<8d} 2thr-entries={int((r['scores'] == r['scores'].max()).sum()):<7d} == {against}", end="")


@pytest.mark.parametrize("name", Rc.IDS)
def test_tables_match_exact_model(ctx, name):
    r = _pass(ctx, name)
    assert r["version"] == Rc.geometry(Rc.by_name(name))["scan_version"]
    _same_tables(name, r, _model_tables(name))
    _line(name, "default", r, "model")


@pytest.mark.parametrize("name", Rc.IDS)
def test_float_twin_matches_oracle(ctx, name):
    """The same windows with the suite's Gaussian noise on the photograph: float scores, compared with the oracle (which hands
    out no score table)."""
    c = Rc.by_name(name)
    N, nSim, nDisp, k, p = c["pk"][:5]
    b = Rc.build(name, True)
    refs = Rc.refs_of(c)
    idx, cnt, disp = Census.oracle_tables(b["est"], b["cc"], k, N, nSim, nDisp, b["tau"], refs, views=Rc.views_of(b))
    used = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    want = dict(refs=refs, idx=np.where(used, idx, 0), cnt=cnt, best={st: v[0] for st, v in disp.items()}, shape={st: v[1] for st, v in disp.items()})
    r = _pass(ctx, name, twin=True)
    assert r["version"] == Rc.geometry(c)["scan_version"]
    _same_tables(name, r, want, scores=False)
    _line(name, "float twin", r, "oracle")


def _forms(name):
    """The alternative forms that apply to a case: (option, table-kernel generation it must report)."""
    g = Rc.geometry(Rc.by_name(name))
    out = []
    if g["regs"]:
        out.append(("select_prefill", g["scan_version"]))          # k_self_select on a filled table instead of k_self_select_regs
    if g["scan_version"] == 3:
        out += [("scan_v1", 1), ("scan_full_tables", 2)]            # round 2's kernel; the ring-sharing kernel with tables in memory
    if g["k"] in (8, 12, 16):
        out.append(("scan_any", 1))                                 # the any-patch-size kernel in place of a dedicated one
    return out


ALTERNATIVES = [(n, o, v) for n in Rc.alternative_cases() for o, v in _forms(n)]


@pytest.mark.parametrize("name,option,version", ALTERNATIVES, ids=[f"{n}-{o}" for n, o, _ in ALTERNATIVES])
def test_alternative_forms_equal_the_default(ctx, name, option, version):
    default = _pass(ctx, name)
    ctx.set_option(option, 1)
    try:
        r = _pass(ctx, name)
    finally:
        ctx.set_option(option, None)
    assert r["version"] == version
    _same_tables(name, r, default)
    _same_tables(name, r, _model_tables(name))
    _line(name, option, r, "default, model")


def test_alternative_subset_is_what_the_issue_names():
    names = Rc.alternative_cases()
    for g in Rc.GROUPS:
        mine = [c["name"] for c in Rc.CASES if c["group"] == g]
        assert mine[0] in names and mine[-1] in names
    assert all(c["name"] in names for c in Rc.CASES if c["group"] == "smallest")
    assert {o for _, o, _ in ALTERNATIVES} == {"select_prefill", "scan_v1", "scan_full_tables", "scan_any"}
    assert ("min-w-k8-h200-p1", "scan_v1", 1) in ALTERNATIVES          # k_bm_scan<8, true>: more than 127 reference rows


@pytest.mark.parametrize("case", Rc.SUBSET, ids=[s["name"] for s in Rc.SUBSET])
def test_subset_pass_matches_exact_model(ctx, case):
    """pst != cst as in test_gpu_bm_ties.py: den = 1 and num = the window on the left part of every plane, so the matching planes
    stay the integer planes and the den-aware reference list is the right part.  Scored on the full grid (the default: the
    selection reads its rows through grid_cols != 0 -- k_self_select_regs<32, 22> on an unfilled table at nSim = 22, k_self_select
    at nSim = 30) and through the position map of subset_scan_v1."""
    pk, Hb, Wb, sigma = case["pk"], case["Hb"], case["Wb"], case["sigma"]
    N, nSim, nDisp, k, p = pk[:5]
    est = Rc.integer_planes(case["kind"], 3, Hb, Wb, k)
    win = np.ascontiguousarray(est.reshape(9, -1))
    tau = Hh.tau_match(sigma, 1, 1)
    den0 = np.zeros((9, Hb, Wb), np.float32)
    den0[:, :, :(3 * Wb) // 5] = 1.0
    den0 = den0.reshape(9, -1)
    num0 = (win * den0).astype(np.float32)
    proc = np.zeros(9, np.uint32)
    proc[4] = 1
    pst = 8
    _, _, st = Hh.oracle_pass(1, sigma, pk, win, None, Wb, Hb, 1, num=num0.copy(), den=den0.copy(), proc=proc, pst=pst)
    assert st.groups > 0
    rows, cols = M.region(Hb, Wb, k, nDisp)
    disp = {}
    # a window's subset passes follow its centre pass, whose reference grid the full-grid form scores on
    gpu_pass(ctx, 1, sigma, pk, win, None, Wb, Hb, 1)
    for v1, version in ((None, 3), (1, 1)):
        ctx.set_option("subset_scan_v1", v1)
        try:
            ctx.reset_stats()
            gpu_pass(ctx, 1, sigma, pk, win, None, Wb, Hb, 1, num=num0.copy(), den=den0.copy(), proc=proc, pst=pst)
            s = ctx.stats()
            refs, idx, cnt, best, shape = ctx.last_bm(N, 9, Wb * Hb)
            assert ctx.last_scan_version() == version
        finally:
            ctx.set_option("subset_scan_v1", None)
        assert (s.groups, s.stack_patches, s.sadct_groups) == (st.groups, st.stack_patches, st.sadct_groups)
        assert len(refs) == st.groups and 0 < len(refs) < len(M.ref_grid(Hb, k, nSim + nDisp, p)) * len(M.ref_grid(Wb, k, nSim + nDisp, p))
        m, _ = M.self_search_stream(est[pst], k, N, nSim, nDisp, tau, refs)
        used = np.arange(N)[None, :] < cnt[:, None]
        assert np.array_equal(cnt, m["cnt"]) and np.array_equal(np.where(used, idx, 0), np.where(used, m["idx"], 0))
        sel = np.unique(idx[used])            # the positions the groups read their disparities at
        for st_i in range(9):
            if st_i == pst:
                continue
            if st_i not in disp:
                d = M.disparity_search(est[pst], est[st_i], k, nDisp, tau)
                full_b, full_s = np.zeros((Hb, Wb), np.uint32), np.zeros((Hb, Wb), np.uint8)
                full_b[rows, cols], full_s[rows, cols] = d["best"], d["shape"]
                disp[st_i] = (full_b.reshape(-1), full_s.reshape(-1))
            assert np.array_equal(best[st_i][sel], disp[st_i][0][sel]), (v1, st_i)
            assert np.array_equal(shape[st_i][refs], disp[st_i][1][refs]), (v1, st_i)
        print(f"\n{case['name']:26s} {'subset_scan_v1' if v1 else 'default':16s} scan=v{version} refs={len(refs):<5d} sum(cnt)={int(cnt.sum()):<6d} "
              f"positions={len(sel) * 8:<7d} == model", end="")


def test_bm3d_step_at_nhard_48_matches_exact_model(ctx):
    """bm3d_step with nHard = 48 on the smallest image for it (105 x 105 padded, a two-by-two reference grid): the selection is
    k_self_select with 75 272 bytes of LDS; tables and score rows against the model, group statistics against the oracle."""
    from lfbm5d_amd import core
    b = Rc.BM3D
    side, N, k = b["side"], b["N"], b["k"]
    est = Rc.integer_planes(b["kind"], 3, side, side, k)[4]
    refs, m, rows = Rc.bm3d_model()
    _, st = O.bm3d_step(1, b["sigma"], 2.7, est.reshape(-1), None, side, side, 1, b["nHard"], k, N, b["p"], "dct", 0)
    d_win = torch.from_numpy(np.ascontiguousarray(est.reshape(-1))).cuda()
    d_out = torch.zeros_like(d_win)
    ctx.reset_stats()
    ctx.bm3d_step(1, core.make_bm3d_params(b["sigma"], 2.7, N, b["nHard"], k, b["p"], "dct", 0), side, side, 1, d_win, None, d_out)
    s = ctx.stats()
    g_refs, idx, cnt, _, _ = ctx.last_bm(N, 1, side * side)
    ncand = (2 * b["nHard"] + 1) ** 2
    scores = ctx.last_scores(len(g_refs) * ncand)
    assert (s.groups, s.stack_patches) == (st.groups, st.stack_patches)
    used = np.arange(N)[None, :] < cnt[:, None]
    assert np.array_equal(g_refs, refs) and np.array_equal(cnt, m["cnt"])
    assert np.array_equal(np.where(used, idx, 0), np.where(used, m["idx"], 0))
    assert np.array_equal(scores.view(np.uint32), rows.astype(np.float32).reshape(-1).view(np.uint32))
    assert np.isfinite(d_out.cpu().numpy()).all()
    print(f"\n{b['name']:26s} {'bm3d_step':16s} refs={len(refs):<5d} sum(cnt)={int(cnt.sum()):<6d} scores={scores.size:<8d} == model", end="")


@pytest.mark.parametrize("nSim,nDisp", [(49, 1), (1, 25)])
def test_search_ranges_past_the_limit_are_refused(ctx, nSim, nDisp):
    import lfbm5d_amd as L
    side = Rc.wmin(nSim, nDisp, 8) + 8
    win = np.ascontiguousarray(Rc.integer_planes("q16", 3, side, side, 8).reshape(9, -1))
    before = _pass(ctx, "min-nsim1-nd1-k8")
    ctx.reset_stats()
    with pytest.raises(L.LfBm5dError, match="nSim > 48 or nDisp > 24"):
        gpu_pass(ctx, 1, 25.0, (8, nSim, nDisp, 8, 3) + Rc.ID3, win, None, side, side, 1)
    assert ctx.stats().groups == 0        # refused by validate(), in front of every launch: the context still holds the pass before
    refs, idx, cnt, _, _ = ctx.last_bm(8, 9, 13 * 13)
    assert np.array_equal(refs, before["refs"]) and np.array_equal(cnt, before["cnt"])
    if nSim == 49:
        with pytest.raises(L.LfBm5dError, match="bad search window"):
            from lfbm5d_amd import core
            d = torch.zeros(side * side, device="cuda")
            ctx.bm3d_step(1, core.make_bm3d_params(25.0, 2.7, 16, 49, 8, 3, "dct", 0), side, side, 1, d, None, torch.zeros_like(d))
