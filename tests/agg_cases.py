"""Seeded synthetic launches for the aggregation kernel's own tests (test_agg_model.py on the CPU, test_gpu_aggregate.py on the GPU).

A case is a namespace: `g` (agg_model.Geom of the whole pass), `aggpos` uint32 [A][R][N], `wgt` float32 [R][C], `refs_yx` int [R][2],
`num0` / `den0` (the sums on entry), `bands` (the launches the pass is cut into, [(ref_begin, n_groups)]), `wants` (census totals that
must be non-zero: the path the case was designed for) and either `filt` (dense float32, uniform in +-255, in the layout `g` names)
or `sparse` ({(g, n, st): patch}; the dense array is then filled from sparse_value, on the device).
Each case is as small as its path allows: SAIs are masked off and entries marked absent rather than the geometry shrunk.
"""
from types import SimpleNamespace

import numpy as np

import agg_model as M

ABSENT = M.ABSENT


def _positions(rng, g, refs_yx, reach_of, mode):
    """aggpos [A][R][N]: every patch within the slot's reach of its reference.  mode: "random", or "rim": offsets of the full reach,
    so that the references on the grid's rim put patches at row / column 0 and at Hb - k / Wb - k."""
    R = len(refs_yx)
    pos = np.empty((g.A, R, g.N), np.uint32)
    for st in range(g.A):
        r = reach_of(st)
        if mode == "rim":
            d = rng.choice([-r, r], size=(2, R, g.N))
            for ax in (0, 1):   # the first match of a reference on the rim points outwards
                c = refs_yx[:, ax]
                d[ax, :, 0] = np.where(c == c.min(), -r, np.where(c == c.max(), r, d[ax, :, 0]))
        else:
            d = rng.integers(-r, r + 1, size=(2, R, g.N))
        py, px = refs_yx[:, 0:1] + d[0], refs_yx[:, 1:2] + d[1]
        pos[st] = (py << 16 | px).astype(np.uint32)
    return pos


def build(name, seed, *, Wb, Hb, C, A, k, N, p, nSim, nDisp, live, proc=(), pst=None, absent=0.0, trailing=False, mode="random",
          weights="uniform", wchan0=0, direct=None, sai_major=False, subset=None, pos_fn=None, bands=None, wants=(), nonfinite=False):
    rng = np.random.default_rng(seed)
    mask = np.zeros(A, np.uint32)
    mask[list(live) + list(proc)] = 1
    pr = np.zeros(A, np.uint32)
    pr[list(proc)] = 1
    g = M.Geom(Wb=Wb, Hb=Hb, C=C, A=A, k=k, N=N, p=p, nSim=nSim, nDisp=nDisp, pst=pst, mask=mask, proc=pr, wchan0=wchan0)
    rows, cols = M.grid_coords(Hb, k, g.nHW, p), M.grid_coords(Wb, k, g.nHW, p)
    refs_yx = np.stack(np.meshgrid(rows, cols, indexing="ij"), -1).reshape(-1, 2)
    if subset is not None:          # an irregular list: a subset of the grid, still in raster order
        refs_yx = refs_yx[np.sort(rng.choice(len(refs_yx), size=int(subset * len(refs_yx)), replace=False))]
        g.irregular, g.R, g.n_groups = 1, len(refs_yx), len(refs_yx)
    R = g.R
    reach_of = lambda st: g.nSim if st == g.pst else g.nHW
    aggpos = pos_fn(rng, g, refs_yx) if pos_fn else _positions(rng, g, refs_yx, reach_of, mode)
    if absent:
        aggpos[rng.random(aggpos.shape) < absent] = ABSENT
    if trailing:                    # as self_cnt < N leaves them: the same tail of every slot's stack
        cnt = rng.integers(1, N + 1, size=R)
        aggpos[:, np.arange(N)[None, :] >= cnt[:, None]] = ABSENT
    wgt = rng.uniform(0.01, 1.0, size=(R, C)).astype(np.float32)
    if weights == "special":        # zeros, denormals, one inf (the Wiener quirk of core:1219)
        wgt[rng.random(R) < 0.2] = 0.0
        wgt[rng.random(R) < 0.2] = np.float32(1e-40)
        wgt[R // 2, 0] = np.inf
    k2 = k * k
    if sai_major:
        g.filt_sai_stride = R * N * C * k2 + 32      # (some slack between the SAIs)
        filt = rng.uniform(-255, 255, size=A * g.filt_sai_stride).astype(np.float32)
    else:
        filt = rng.uniform(-255, 255, size=R * N * A * C * k2).astype(np.float32)
    if direct:                      # the light field's sums: n_sai SAIs of [C][H][W], lf_stride apart; window slot -> SAI
        n_sai, sai = direct
        g.direct, g.sai = 1, np.asarray(sai, np.uint32)
        g.lf_stride = C * (Wb - 2 * g.nHW) * (Hb - 2 * g.nHW) + 48
        n_sums = n_sai * g.lf_stride
    else:
        n_sums = A * C * Wb * Hb
    num0 = rng.uniform(-100, 100, size=n_sums).astype(np.float32)
    den0 = rng.uniform(0.5, 10, size=n_sums).astype(np.float32)
    case = SimpleNamespace(name=name, g=g, aggpos=aggpos, wgt=wgt, refs_yx=refs_yx, filt=filt, sparse=None, num0=num0, den0=den0,
                           bands=bands or [(0, R)], wants=tuple(wants), nonfinite=nonfinite)
    if nonfinite:                   # a NaN and an inf at clamped-corner elements of two present patches of the first live slot
        st = live[0]
        there = np.argwhere(aggpos[st] != ABSENT)
        pat = M.dense_patches(filt, g)
        (g1, n1), (g2, n2) = there[len(there) // 3], there[2 * len(there) // 3]
        pat(g1, n1, st)[0, 0] = np.nan
        pat(g2, n2, st)[C - 1, k2 - 1] = np.inf
    return case


def row_bands(g, rows_per_band):
    out, r = [], 0
    while r < g.n_ref_rows:
        n = min(rows_per_band, g.n_ref_rows - r)
        out.append((r * g.n_ref_cols, n * g.n_ref_cols))
        r += n
    return out


def _overflow_positions(rng, g, refs_yx):
    """p = 1, reach 1 in slot pst: for an 8 x 8 tile at row ty0 the candidate rows start at reference rows ty0 - 8 and ty0 - 7.  The
    patches of reference rows y = 0 (mod 8) sit one row ABOVE their reference and miss the tile below, apart from the first m(x)
    matches of each reference (one row below: hits); those of rows y = 1 (mod 8) sit above too; every other patch sits on its reference.
    A tile's first scan round (32 references: candidate row 0 and most of row 1) then collects sum m(x) hits over its 15 columns --
    fewer than 64, so they stay in the list -- and the second round is dense: 216 hits in an interior tile (15 references of candidate
    row 2, 12 of row 3, eight matches each), against a capacity of 256.  m(x) = 3 gives 45 + 216: an overflow; m(x) = 2 in columns
    9 .. 13 gives the tiles at column 16 40 + 216: the list filled exactly."""
    R = len(refs_yx)
    y, x = refs_yx[:, 0], refs_yx[:, 1]
    dy = np.zeros((R, g.N), np.int64)
    m = np.where((x >= 9) & (x <= 13), 2, 3)                          # per reference COLUMN, the same in every row
    top = (y % 8 == 0)[:, None]
    dy[:] = np.where(top, np.where(np.arange(g.N)[None, :] < m[:, None], 1, -1), 0)
    dy[(y % 8 == 1)] = -1
    pos = ((y[:, None] + dy) << 16 | x[:, None]).astype(np.uint32)
    return np.broadcast_to(pos, (g.A, R, g.N)).copy()


def sparse_value(i):
    """Element i (int64 array) of the device-filled filt of the 32-bit-index case: integers in -255 .. 255, exact in float32 and
    computable with integer arithmetic alone, so the host and the device agree on them."""
    h = (i * 2654435761 + 40503) % (1 << 32)
    return ((h >> 13) % 511 - 255).astype(np.float32)


def index32_case():
    """Group-major with (R N + 1) A >= 2^24: A = 81, N = 32, an 81 x 81 grid, k = 2, C = 1 (filt: 68 M floats, filled on the device).
    The 24-bit products go wrong from ((g N + n) A + st) >= 2^24 on, i.e. in the last 90 groups: most present patches are there."""
    rng = np.random.default_rng(32)
    A, N, k, C = 81, 32, 2, 1
    live = [0, 40, 80]
    mask = np.zeros(A, np.uint32)
    mask[live] = 1
    g = M.Geom(Wb=86, Hb=86, C=C, A=A, k=k, N=N, p=1, nSim=1, nDisp=1, mask=mask)
    assert (g.n_ref_rows, g.n_ref_cols) == (81, 81)
    rows = M.grid_coords(86, k, 2, 1)
    refs_yx = np.stack(np.meshgrid(rows, rows, indexing="ij"), -1).reshape(-1, 2)
    R = g.R
    aggpos = np.full((A, R, N), ABSENT, np.uint32)
    gs = np.concatenate([rng.integers(0, R, 1500), rng.integers(R - 90, R, 2500)])
    sparse = {}
    for gi in gs:
        st, n = live[rng.integers(3)], int(rng.integers(N))
        r = g.nSim if st == g.pst else g.nHW
        py, px = refs_yx[gi] + rng.integers(-r, r + 1, size=2)
        aggpos[st, gi, n] = py << 16 | px
        base = ((int(gi) * N + n) * A + st) * C * k * k
        sparse[(int(gi), n, st)] = sparse_value(base + np.arange(C * k * k, dtype=np.int64)).reshape(C, k * k)
    wgt = rng.uniform(0.01, 1.0, size=(R, C)).astype(np.float32)
    n_sums = A * C * 86 * 86
    return SimpleNamespace(name="index32", g=g, aggpos=aggpos, wgt=wgt, refs_yx=refs_yx, filt=None, sparse=sparse,
                           num0=rng.uniform(-100, 100, size=n_sums).astype(np.float32), den0=rng.uniform(0.5, 10, size=n_sums).astype(np.float32),
                           bands=[(0, R)], wants=("not_small24",), nonfinite=False)


def template_cases():
    """Every kernel instantiation x every scan: k = 8 (windowed 8 x 8 tiles), 12 (windowed 16 x 4), 16 (16 x 4), 6 and 4 (plain 8 x 8);
    N = 1, 2 (scalar scan), 4, 8, 16 (four per lane below k = 12); C = 1 and 3."""
    out = []
    for k in (8, 12, 16, 6, 4):
        for N in (1, 2, 4, 8, 16):
            for C in (1, 3):
                side = 48 + (k >= 12) * 8 + 3 * (N % 3) + C      # 48 .. 72, ragged
                out.append(build(f"grid-k{k}-n{N}-c{C}", 1000 * k + 10 * N + C, Wb=side, Hb=side - 5, C=C, A=9, k=k, N=N, p=3,
                                 nSim=5, nDisp=2, live=[1, 4, 6], absent=0.1))
    return out


def special_cases():
    B = build
    c = []
    # ragged geometry: partial tiles on both axes, forced last index closer than p, full-reach offsets on the rim
    c.append(B("ragged-k8", 1, Wb=61, Hb=53, C=3, A=9, k=8, N=4, p=3, nSim=4, nDisp=2, live=[0, 4, 8], mode="rim", wants=("n_partial",)))
    c.append(B("ragged-k16", 2, Wb=67, Hb=58, C=1, A=9, k=16, N=2, p=4, nSim=4, nDisp=2, live=[3, 4], mode="rim", wants=("n_partial",)))
    # a forced last index right behind its predecessor, tiles whose r_lo / c_lo point past the grid (:77-78)
    # (grid 3, 8, .. 38, then 42: one short of the regular 43; the tile at row / column 48 starts behind what slot pst can reach)
    c.append(B("clamp-lo", 3, Wb=49, Hb=49, C=1, A=9, k=4, N=4, p=5, nSim=1, nDisp=2, live=[4, 5], mode="rim", wants=("n_clamped_lo",)))
    # the smallest legal window, 2 nHW + k + 1 a side
    c.append(B("smallest-k8", 4, Wb=25, Hb=25, C=3, A=9, k=8, N=8, p=3, nSim=6, nDisp=2, live=[2, 4], mode="rim"))
    c.append(B("smallest-k12", 5, Wb=23, Hb=23, C=1, A=9, k=12, N=1, p=3, nSim=3, nDisp=2, live=[4, 7], mode="rim"))
    # holes: random and trailing absent entries, masked and processed slots, sums already there
    c.append(B("holes-k8", 6, Wb=56, Hb=50, C=3, A=9, k=8, N=8, p=3, nSim=5, nDisp=2, live=[0, 4, 5], proc=[2, 7], absent=0.4, trailing=True))
    c.append(B("holes-k16", 7, Wb=64, Hb=58, C=1, A=9, k=16, N=4, p=3, nSim=5, nDisp=2, live=[4, 8], proc=[0], absent=0.3, trailing=True))
    # weights: zeros, denormals, one inf; channel 0's weight for every channel
    c.append(B("weights-special", 8, Wb=50, Hb=50, C=3, A=9, k=8, N=4, p=3, nSim=5, nDisp=2, live=[3, 4], weights="special"))
    c.append(B("wchan0", 9, Wb=50, Hb=50, C=3, A=9, k=6, N=2, p=3, nSim=5, nDisp=2, live=[4, 6], wchan0=1))
    # bands: one launch / row bands in raster order
    for nm, k, N in (("bands-k8", 8, 8), ("bands-k16", 16, 2)):
        cs = B(nm, 10 + k, Wb=60, Hb=60, C=3, A=9, k=k, N=N, p=3, nSim=5, nDisp=2, live=[0, 4])
        cs.bands = row_bands(cs.g, 3)
        c.append(cs)
    # irregular list
    c.append(B("irregular-n1", 12, Wb=56, Hb=56, C=3, A=9, k=8, N=1, p=3, nSim=5, nDisp=2, live=[4, 5], subset=0.4))
    c.append(B("irregular-n8", 13, Wb=56, Hb=56, C=1, A=9, k=8, N=8, p=3, nSim=5, nDisp=2, live=[1, 4], subset=0.4))
    # direct form: a 5 x 5 light field, the window's slots somewhere inside; nHW = 7 is no multiple of a tile side
    sai = [(1 + st // 3) * 5 + 2 + st % 3 for st in range(9)]
    c.append(B("direct-k8", 14, Wb=59, Hb=52, C=3, A=9, k=8, N=4, p=3, nSim=5, nDisp=2, live=[0, 4, 8], proc=[3], direct=(25, sai)))
    c.append(B("direct-k16", 15, Wb=62, Hb=55, C=1, A=9, k=16, N=2, p=3, nSim=5, nDisp=2, live=[4, 5], direct=(25, sai[::-1])))
    # SAI-major filt: 11 x 11 SAIs, a handful there
    c.append(B("sai-major", 16, Wb=48, Hb=48, C=3, A=121, k=8, N=4, p=3, nSim=5, nDisp=2, live=[0, 60, 77, 120], sai_major=True))
    # hit-list overflow of the four-per-lane scan
    c.append(B("overflow", 17, Wb=61, Hb=61, C=1, A=9, k=8, N=8, p=1, nSim=1, nDisp=1, live=[4, 5], pos_fn=_overflow_positions,
               wants=("n_overflow", "n_exact_fill")))
    # exact division: n_rr * ncols_span >= 2^20 (p = 1, reach 45, 105 grid columns)
    c.append(B("exact-div", 18, Wb=201, Hb=201, C=1, A=9, k=6, N=4, p=1, nSim=40, nDisp=5, live=[4, 5], absent=0.75, wants=("n_exact_div",)))
    c.append(index32_case())
    return c


def nonfinite_case():
    return build("nonfinite", 19, Wb=50, Hb=50, C=3, A=9, k=8, N=4, p=3, nSim=5, nDisp=2, live=[4, 5], nonfinite=True)


def patches_of(case, g=None):
    """agg_model's patches() of a case."""
    if case.sparse is not None:
        return lambda gi, n, st: case.sparse[(gi, n, st)]
    return M.dense_patches(case.filt, g or case.g)


def band_filt(case, rb, nb):
    """The filt buffer of one launch: the band's groups only (group-major: a slice; SAI-major cases run as one launch)."""
    g = case.g
    if g.filt_sai_stride or (rb, nb) == (0, g.R):
        return case.filt, g.filt_sai_stride
    per_group = g.N * g.A * g.C * g.k * g.k
    return case.filt[rb * per_group:(rb + nb) * per_group], 0
