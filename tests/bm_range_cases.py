"""Block matching across its whole search range and at its smallest windows: the geometry axis of the block-matching tests
(tests/bm_tie_cases.py is the data axis).  validate() accepts nSim 1..48 and nDisp 1..24 and pass_impl any window with
Wb, Hb >= 2 nHW + k + 1; the cases below sit on the code paths the search geometry alone chooses.

Data.  A case's matching planes are [A][Hb][Wb] crops of tests/golden/sourceLF_3x3_256_u8.npy (red channel; the 5x5 case cuts its
views from the centre view like helpers.textured_lf), taken at the window's own size -- a core pass takes any window, and the
smallest ones (k + 1 pixels inside the search margins) are below what mirror padding can make.  Integer form: bm_tie_cases' q16
construction, floor(g / 16) * 16 / scale with scale 2 for 8 < k <= 16 and 4 for k = 32 (exact_domain: 4 k^2 R^2 < 2^24, R <= 63 at
k = 32); the kinds "n<sd>" add seeded Gaussian noise of that standard deviation before quantising, "r<sd>" noise whose standard
deviation ramps from 0.4 sd to sd over the 20 columns around the window's centre (the reference patches then run from "most of the
window passes" to "nothing but the patch itself does"), so that the threshold tau k^2 cuts inside the search window and every
passing-candidate class of the selection kernel is reached.  Float twin: the same crop plus the suite's Gaussian noise
(helpers.noisy_lf), compared with the oracle only.

A case: dict(name, group, pk = (N, nSim, nDisp, k, p, "id", "sadct", "haar"), Hb, Wb, kind, sigma, aw, mask, tags).
The census (geometry(), TAGS) is pure arithmetic on the parameters, restated from the dispatch in lfbm5d_pass.hip,
lfbm5d_bm.hip (launch_self_select_regs, launch_bm_scan), lfbm5d_scan2.hip (scan2_plan, scan2_lds_bytes) and the layout functions of
lfbm5d_kernels.h; data_tags() are predicates on the exact model's result.  tests/test_bm_range.py proves every tag on its case.
"""
import functools

import numpy as np

import bm_tie_cases as Ts
import bm_tie_model as M
import helpers as Hh

ID3 = ("id", "sadct", "haar")
Y0, X0 = 24, 40          # where the crops start in the 256 x 256 views
CASES = []


def wmin(nSim, nDisp, k):
    return 2 * (nSim + nDisp) + k + 1


def _c(name, group, N, nSim, nDisp, k, p, Hb, Wb, tags, kind="q16", sigma=25.0, aw=3, mask=None):
    CASES.append(dict(name=name, group=group, pk=(N, nSim, nDisp, k, p) + ID3, Hb=Hb, Wb=Wb, kind=kind, sigma=sigma, aw=aw,
                      mask=mask, tags=tuple(tags)))


# ---- selection instantiations: first and last nSim of every ROWS class of launch_self_select_regs the suite did not run
for _nSim, _rows in ((1, 1), (2, 1), (4, 2), (7, 4), (10, 8), (11, 16), (15, 16), (16, 22), (19, 32), (22, 32)):
    _m = wmin(_nSim, 2, 8) + 9
    _c(f"sel-nsim{_nSim}", "selection", 8 if _nSim == 1 else 16, _nSim, 2, 8, 3, _m, _m, [f"rows{_rows}", "regs", "scan3"] + (["ragged-tiles"] if (_nSim + 1) % 4 and (2 * _nSim + 1) % 11 else []),
       kind="r160" if _nSim in (15, 22) else "q16")
# ---- k_self_select as the default selection (nSim >= 23): prefill, 20-bit reciprocal with Ns up to 97, LDS up to 75 272 bytes
for _nSim, _k, _p, _kind, _sigma, _extra in ((23, 8, 3, "q16", 25.0, []), (32, 8, 3, "r160", 25.0, []), (44, 8, 3, "r130", 25.0, ["lds-last-under-64K"]),
                                              (45, 8, 3, "r160", 25.0, ["lds-over-64K"]), (48, 8, 3, "r160", 25.0, ["lds-over-64K"]),
                                              (48, 16, 3, "r160", 25.0, ["lds-over-64K"]), (30, 8, 5, "r130", 40.0, ["stores-lookup"])):
    _m = wmin(_nSim, 1, _k) + (8 if _p == 5 else 10)
    _c(f"kss-nsim{_nSim}-k{_k}-p{_p}", "k_self_select", 16, _nSim, 1, _k, _p, _m, _m, ["select-lds", "scan3"] + _extra, kind=_kind, sigma=_sigma)
# ---- disparity range
for _nD, _tags in ((1, ["idle-table-waves", "nwg<=16"]), (4, ["nwg<=16"]), (5, ["nwg<=16"]), (7, ["nwg>16"]), (12, ["nwg>16"]), (24, ["nwg220", "nwg>16", "edge-trips19"])):
    _m = wmin(1, _nD, 8) + 16
    _c(f"disp-nd{_nD}", "disparity", 8, 1, _nD, 8, 3, _m, _m, ["scan3", "self-one-tile"] + _tags)
_c("disp-nd16-k16", "disparity", 8, 1, 16, 16, 3, wmin(1, 16, 16) + 12, wmin(1, 16, 16) + 12, ["scan3", "scan2-last-ring"])
_c("disp-nd17-k16", "disparity", 8, 1, 17, 16, 3, wmin(1, 17, 16) + 12, wmin(1, 17, 16) + 12, ["scan1", "scan2-ring-too-wide"])
_c("disp-nd24-two-strips", "disparity", 8, 1, 24, 8, 3, 75, 140, ["scan3", "nwg220", "disp-strips2"])
_c("disp-nd24-empty-sais", "disparity", 8, 1, 24, 8, 3, 75, 75, ["scan3", "nwg220", "masked"], mask=(1, 0, 1, 1, 1, 1, 1, 0, 1))
# ---- smallest windows: Wb = Hb = 2 nHW + k + 1
for _nSim, _nD, _k in ((1, 1, 8), (3, 2, 16), (6, 6, 8), (18, 6, 8), (2, 1, 12), (2, 1, 4), (1, 1, 32)):
    _m = wmin(_nSim, _nD, _k)
    _c(f"min-nsim{_nSim}-nd{_nD}-k{_k}", "smallest", 8, _nSim, _nD, _k, 3, _m, _m,
       ["grid2x2", "scan3" if _k in (8, 16) else "scan1"] + (["disp-rows<8"] if _nSim < 3 else []) + (["self-9-lanes"] if _k == 8 else []))
_c("min-w-k12-h200-p1", "smallest", 8, 2, 1, 12, 1, 200, wmin(2, 1, 12), ["wide", "scan1"])
_c("min-w-k8-h200-p1", "smallest", 8, 1, 1, 8, 1, 200, wmin(1, 1, 8), ["wide", "scan3", "stores-pattern"])
_c("min-h-k8-three-strips", "smallest", 8, 1, 1, 8, 3, wmin(1, 1, 8), 150, ["scan3", "self-strips3", "disp-strips3", "disp-rows<8"])
# ---- strip and chunk edges: self-table widths Wb - 2 nHW and disparity widths Wb - 2 nDisp - k + 1 of 65, 66, 128, 129;
# disparity heights with (nrows + 62) % 16 of 0 and 15
for _k, _nSim, _nD in ((8, 2, 2), (16, 3, 1)):
    _nHW = _nSim + _nD
    for _i, _w in enumerate((65, 66, 128, 129)):
        _rem = {65: 0, 66: 1, 128: 63, 129: 0}[_w]
        _rows = (18, 17, 34, 33)[_i] if 2 * _nSim + 2 <= 17 else (34, 33, 34, 33)[_i]
        _Hb = _rows + 2 * _nD + _k - 1
        _c(f"edge-self-w{_w}-k{_k}", "edges", 8, _nSim, _nD, _k, 3, _Hb, _w + 2 * _nHW, ["scan3", f"self-col-rem{_rem}", f"disp-row-rem{(_rows + 62) % 16}"])
        _c(f"edge-disp-w{_w}-k{_k}", "edges", 8, _nSim, _nD, _k, 3, _Hb, _w + 2 * _nD + _k - 1, ["scan3", f"disp-col-rem{_rem}", f"disp-row-rem{(_rows + 62) % 16}"])
# ---- wider angular window
_c("aw5-nd12", "angular", 8, 1, 12, 8, 3, wmin(1, 12, 8) + 8, wmin(1, 12, 8) + 8, ["scan3", "slots24", "nwg>16"], aw=5)

IDS = [c["name"] for c in CASES]
GROUPS = ("selection", "k_self_select", "disparity", "smallest", "edges", "angular")
# the subset passes (pst != cst, built as in test_gpu_bm_ties.py) and the per-SAI BM3D step are driven by the GPU test itself
SUBSET = [dict(name="subset-nsim22", pk=(16, 22, 1, 8, 3) + ID3, Hb=wmin(22, 1, 8) + 24, Wb=wmin(22, 1, 8) + 30, kind="q16", sigma=25.0),
          dict(name="subset-nsim30", pk=(16, 30, 1, 8, 3) + ID3, Hb=wmin(30, 1, 8) + 24, Wb=wmin(30, 1, 8) + 30, kind="q16", sigma=25.0)]
BM3D = dict(name="bm3d-nhard48", N=16, nHard=48, k=8, p=3, side=2 * 48 + 8 + 1, kind="r130", sigma=25.0)


def by_name(name):
    return CASES[IDS.index(name)]


def alternative_cases():
    """The subset that runs again under the alternative forms: first and last case of each group, and every smallest window."""
    out = []
    for g in GROUPS:
        names = [c["name"] for c in CASES if c["group"] == g]
        out += names if g == "smallest" else [names[0], names[-1]] if len(names) > 1 else names
    return out


def scale(k):
    return 4 if k > 16 else Ts._scale(k)


def _views(aw, Hb, Wb):
    """[A][Hb][Wb] float64 grey levels 0..255."""
    if aw == 3:
        return Hh.source_lf()[:, 0, Y0:Y0 + Hb, X0:X0 + Wb].astype(np.float64)
    return Hh.textured_lf(aw, aw, Hb, Wb)[:, 0].astype(np.float64)


def integer_planes(kind, aw, Hb, Wb, k):
    g = _views(aw, Hb, Wb)
    if kind != "q16":
        noise = np.random.default_rng(int(kind[1:])).normal(0, float(kind[1:]), g.shape)
        if kind[0] == "r":
            noise *= (0.4 + 0.6 * np.clip((np.arange(Wb) - (Wb // 2 - 10)) / 20.0, 0, 1))[None, None, :]
        g = np.clip(g + noise, 0, 255)
    return (np.floor(g / 16) * (16 // scale(k))).astype(np.float32)


def float_planes(aw, Hb, Wb, sigma):
    g = _views(aw, Hb, Wb)
    A = g.shape[0]
    return Hh.noisy_lf(g.reshape(A, 1, Hb, Wb), sigma)[1].reshape(A, Hb, Wb)


@functools.lru_cache(maxsize=None)
def build(name, twin=False):
    """-> dict(est [A][Hb][Wb] float32 (the window: C = 1), Wb, Hb, A, cc, tau, mask)."""
    c = by_name(name)
    k, aw, Hb, Wb = c["pk"][3], c["aw"], c["Hb"], c["Wb"]
    est = float_planes(aw, Hb, Wb, c["sigma"]) if twin else integer_planes(c["kind"], aw, Hb, Wb, k)
    A = aw * aw
    mask = np.ones(A, np.uint32) if c["mask"] is None else np.array(c["mask"], np.uint32)
    return dict(est=np.ascontiguousarray(est, np.float32), Wb=Wb, Hb=Hb, A=A, cc=A // 2, tau=Hh.tau_match(c["sigma"], 1, 1), mask=mask)


def refs_of(c):
    N, nSim, nDisp, k, p = c["pk"][:5]
    rows, cols = M.ref_grid(c["Hb"], k, nSim + nDisp, p), M.ref_grid(c["Wb"], k, nSim + nDisp, p)
    return (rows[:, None] * c["Wb"] + cols[None, :]).reshape(-1).astype(np.uint32)


def views_of(b):
    return [st for st in range(b["A"]) if st != b["cc"] and b["mask"][st]]


@functools.lru_cache(maxsize=None)
def model(name):
    """The exact model of a case: refs, self (dict of bm_tie_model.self_search), rows (the filled score table), disp[st]."""
    c = by_name(name)
    N, nSim, nDisp, k, p = c["pk"][:5]
    b = build(name)
    refs = refs_of(c)
    s, rows = M.self_search_stream(b["est"][b["cc"]], k, N, nSim, nDisp, b["tau"], refs)
    return dict(refs=refs, self=s, rows=rows,
                disp={st: M.disparity_search(b["est"][b["cc"]], b["est"][st], k, nDisp, b["tau"]) for st in views_of(b)})


# ------------------------------------------------------------------------------------------------------------------------------
# the census: arithmetic on the parameters alone
# ------------------------------------------------------------------------------------------------------------------------------
S2NW, S2NI = 11, 6      # lfbm5d_scan2.hip: tables of a workgroup, 16-byte pieces per loader lane


def _scan2_fits(k, H, nDisp, n_self):
    """scan2_plan's answer and its LDS bytes (S2Geom, scan2_lds_bytes)."""
    rh, ch = max(3 if n_self else 0, 2 * nDisp), max(S2NW - 1 if n_self else 0, 2 * nDisp)
    lag, lead1 = (63 - k + 7) // 8, (k + 7) // 8
    rrp1 = 8 * (lag + lead1 + 2) + 13
    rrp2 = 8 * (lag + (7 + k + rh) // 8 + 2) + 13
    cw2 = (64 + k + ch + 3) & ~3
    tail = max((H + 64) * 2 if n_self else 0, 2 * S2NW * 512 * 4)
    lds = ((64 + k) * rrp1 + cw2 * rrp2 + 2 * S2NW * 8) * 4 + tail + 16
    return 2 * (64 + k) + 2 * cw2 <= 64 * S2NI and lds <= 160 * 1024, lds


def geometry(c):
    N, nSim, nDisp, k, p = c["pk"][:5]
    Hb, Wb = c["Hb"], c["Wb"]
    nHW, Ns, Nd = nSim + nDisp, 2 * nSim + 1, 2 * nDisp + 1
    g = dict(N=N, nSim=nSim, nDisp=nDisp, k=k, p=p, Hb=Hb, Wb=Wb, ncand=Ns * Ns, tables=Nd * Nd)
    g["regs"] = N > 1 and Ns * Ns <= 64 * 32                                              # self_select_regs_covers
    rows = (Ns * Ns + 63) // 64
    g["ROWS"] = next(r for r in (1, 2, 4, 8, 16, 22, 32, 1 << 30) if rows <= r) if g["regs"] else 0
    g["select_lds"] = 0 if g["regs"] else Ns * Ns * 8                                      # launch_self_select
    fits, g["scan_lds"] = _scan2_fits(k, Hb, nDisp, N > 1)
    g["scan_version"] = 3 if k in (8, 16) and fits else 1                                  # bm_scan_version, default options, centre pass
    per_class = [sum(1 for o in range(Nd * Nd) if ((o // Nd + o % Nd) & 3) == cls) for cls in range(4)]
    g["class_tables"] = per_class
    g["nwg_slot"] = sum((n + S2NW - 1) // S2NW for n in per_class)                          # scan2_plan
    g["argmin_wg_trips"] = (g["nwg_slot"] + 15) // 16                                       # k_stereo_argmin3: j0 += 16
    g["argmin_edge_trips"] = (Nd * Nd + 127) // 128                                         # ... d0 += 128
    g["slots"] = int(sum(c["mask"]) - 1) if c["mask"] is not None else c["aw"] ** 2 - 1
    g["self_rows"], g["self_cols"] = Hb - 2 * nHW, Wb - 2 * nHW
    g["disp_rows"], g["disp_cols"] = Hb - 2 * nDisp - k + 1, Wb - 2 * nDisp - k + 1
    g["self_strips"], g["disp_strips"] = (g["self_cols"] - 1 + 63) // 64, (g["disp_cols"] - 1 + 63) // 64
    g["self_col_rem"], g["disp_col_rem"] = (g["self_cols"] - 1) % 64, (g["disp_cols"] - 1) % 64
    g["disp_row_rem"] = (g["disp_rows"] - 1 + 63) % 16
    g["ref_rows"], g["ref_cols"] = len(M.ref_grid(Hb, k, nHW, p)), len(M.ref_grid(Wb, k, nHW, p))
    g["self_tiles"] = ((nSim + 1 + 3) // 4, (Ns + S2NW - 1) // S2NW)
    g["ragged_tiles"] = (nSim + 1) % 4 != 0 and Ns % S2NW != 0
    ex_r, ex_c = Hb - k - 2 * nHW, Wb - k - 2 * nHW                                         # last grid row / column minus nHW
    g["pattern"] = ex_r % p == 0 and ex_c % p == 0
    g["lookup"] = ex_r % p != 0
    g["wide"] = g["ref_rows"] > 127                                                         # launch_bm_scan
    g["scores_bytes"] = g["ref_rows"] * g["ref_cols"] * Ns * Ns * 4
    return g


TAGS = {
    "regs": lambda g: g["regs"],
    "select-lds": lambda g: not g["regs"] and g["nSim"] >= 23 and g["select_lds"] == (2 * g["nSim"] + 1) ** 2 * 8,
    "lds-last-under-64K": lambda g: g["select_lds"] == 63368 and (2 * g["nSim"] + 3) ** 2 * 8 > 65536,
    "lds-over-64K": lambda g: 65536 < g["select_lds"] <= 97 * 97 * 8,
    "scan3": lambda g: g["scan_version"] == 3,
    "scan1": lambda g: g["scan_version"] == 1,
    "scan2-last-ring": lambda g: g["scan_version"] == 3 and not _scan2_fits(g["k"], g["Hb"], g["nDisp"] + 1, True)[0],
    "scan2-ring-too-wide": lambda g: g["k"] in (8, 16) and g["scan_version"] == 1 and _scan2_fits(g["k"], g["Hb"], g["nDisp"] - 1, True)[0],
    "nwg<=16": lambda g: g["nwg_slot"] <= 16 and g["argmin_wg_trips"] == 1,
    "nwg>16": lambda g: g["nwg_slot"] > 16 and g["argmin_wg_trips"] > 1,
    "nwg220": lambda g: g["nwg_slot"] == 220 and g["argmin_wg_trips"] == 14 and g["tables"] * g["slots"] in (19208, 14406) and g["scan_lds"] > 130 * 1024,
    "edge-trips19": lambda g: g["argmin_edge_trips"] == 19,
    "idle-table-waves": lambda g: max(g["class_tables"]) <= 3 and g["tables"] == 9,
    "self-one-tile": lambda g: g["self_tiles"] == (1, 1) and 2 * g["nSim"] + 1 == 3,
    "self-9-lanes": lambda g: g["self_cols"] == 9 and g["self_strips"] == 1,
    "self-strips3": lambda g: g["self_strips"] == 3,
    "disp-strips2": lambda g: g["disp_strips"] == 2,
    "disp-strips3": lambda g: g["disp_strips"] == 3,
    "self-col-rem0": lambda g: g["self_col_rem"] == 0 and g["self_cols"] > 1,          # whole strips, the last one full
    "self-col-rem1": lambda g: g["self_col_rem"] == 1 and g["self_strips"] > 1,
    "self-col-rem63": lambda g: g["self_col_rem"] == 63 and g["self_strips"] > 1,
    "disp-col-rem0": lambda g: g["disp_col_rem"] == 0 and g["disp_cols"] > 1,          # whole strips, the last one full
    "disp-col-rem1": lambda g: g["disp_col_rem"] == 1 and g["disp_strips"] > 1,
    "disp-col-rem63": lambda g: g["disp_col_rem"] == 63 and g["disp_strips"] > 1,
    "disp-row-rem0": lambda g: g["disp_row_rem"] == 0,
    "disp-row-rem15": lambda g: g["disp_row_rem"] == 15,
    "disp-rows<8": lambda g: g["disp_rows"] < 8 and g["disp_rows"] == 2 * g["nSim"] + 2,
    "grid2x2": lambda g: (g["ref_rows"], g["ref_cols"]) == (2, 2) and g["Hb"] == g["Wb"] == wmin(g["nSim"], g["nDisp"], g["k"]),
    "stores-pattern": lambda g: g["scan_version"] == 3 and g["pattern"],
    "stores-lookup": lambda g: g["scan_version"] == 3 and g["lookup"],
    "wide": lambda g: g["wide"],
    "masked": lambda g: g["slots"] == 6,
    "slots24": lambda g: g["slots"] == 24,
}
TAGS.update({f"rows{r}": (lambda g, r=r: g["regs"] and g["ROWS"] == r) for r in (1, 2, 4, 8, 16, 22, 32)})
TAGS["ragged-tiles"] = lambda g: g["ragged_tiles"]

# data tags: predicates on model(name) -- the selection classes the passing-candidate counts reach, ties at the cut, disparity ties
SELECTION_CLASSES = {"<N,not-pow2", "1", "2..64", "65..128", ">128"}


def data_tags(name):
    c, m = by_name(name), model(name)
    out = set(Ts.path_classes(m["self"]["n_pass"], c["pk"][0]))
    if m["self"]["tie_cut"].any():
        out.add("tie-cut")
    if any(d["tie_min"].any() for d in m["disp"].values()):
        out.add("tie-disp")
    return out


def census_line(c):
    g = geometry(c)
    sel = f"regs<{g['ROWS']}>" if g["regs"] else f"k_self_select lds={g['select_lds']}"
    return (f"{c['name']:26s} {g['Hb']:3d}x{g['Wb']:<3d} N={g['N']:<2d} nSim={g['nSim']:<2d} nDisp={g['nDisp']:<2d} k={g['k']:<2d} p={g['p']} {sel:28s} scan=v{g['scan_version']} "
            f"nwg/slot={g['nwg_slot']:<3d} slots={g['slots']:<2d} refs={g['ref_rows']}x{g['ref_cols']} self={g['self_rows']}x{g['self_cols']} ({g['self_strips']} strips) "
            f"disp={g['disp_rows']}x{g['disp_cols']} ({g['disp_strips']} strips, row-rem {g['disp_row_rem']}) {'pattern' if g['pattern'] else 'look-up' if g['lookup'] else 'mixed'}"
            f"{' wide' if g['wide'] else ''}")


def bm3d_tau():
    """tauMatch of the BM3D hard-thresholding step on one channel, sigma < 35 (lfbm5d_pass.hip: 3 * 2500)."""
    return 7500.0


@functools.lru_cache(maxsize=None)
def bm3d_model():
    """-> (refs, dict of the exact self search, score rows) of the BM3D case: centre view, search band = search window."""
    b = BM3D
    est = integer_planes(b["kind"], 3, b["side"], b["side"], b["k"])[4]
    g = M.ref_grid(b["side"], b["k"], b["nHard"], b["p"])
    refs = (g[:, None] * b["side"] + g[None, :]).reshape(-1).astype(np.uint32)
    s, rows = M.self_search_stream(est, b["k"], b["N"], b["nHard"], 0, bm3d_tau(), refs)
    return refs, s, rows
