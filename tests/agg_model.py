"""A model of the aggregation kernel alone (lfbm5d_amd/csrc/lfbm5d_aggregate.hip, k_aggregate), in plain numpy: no GPU, no oracle.

aggregate()  what the kernel promises to compute: core:484-528 as a scatter in the reference's order, every operation rounded to
             float32 on its own.  A scatter that visits the patches in the order (SAI slot; group in list order; match n) gives every
             pixel its terms in exactly the order the kernel's gather adds them, so num / den are predictable bit for bit.
census()     what the kernel's scan does on the way, from the inputs alone: the candidate range of every tile, the hits of every
             scan round, the carry between rounds, whether a round overflows the hit list, and which index arithmetic runs.  It is
             the only evidence that a test case reaches a given path of the kernel, so the tests assert on it.

Both take the launch as a `Geom` (the fields of lfbm5d_agg_debug, include/lfbm5d.h) plus host arrays:
  aggpos  uint32 [A][R][N]   (row << 16) | column of each patch in the padded window, ABSENT where there is none
  wgt     float32 [R][C]
  patches a function (g, n, st) -> float32 [C][k*k]: the filtered patch of ABSOLUTE group g (dense_patches / a dict's lookup)
  num/den float32, flat: [A][C][Hb][Wb], or (direct form) [SAI of the light field][lf_stride] holding [C][H][W] each
"""
from types import SimpleNamespace

import numpy as np

ABSENT = 0xFFFFFFFF

# ---- constants copied from the kernel source; keep the line references current ----
FLUSH = 64                      # lfbm5d_aggregate.hip:32   kAggFlush: hits that start a consume phase
VEC4_ROUND = 256                # :225  the four-per-lane scan takes 64 lanes x 4 candidates per round
VEC4_RUN = 64                   # :227  after an overflow: sixteen lanes (64 candidates) at a time


def tile_config(k):
    """(tile width, tile height, kAggPF, windowed) as launch_aggregate picks them (:293-316)."""
    if k == 12:
        return 16, 4, 3, True   # :313
    if k == 8:
        return 8, 8, 3, True    # :314  kAgg8TW, kAgg8TH, kAgg8PF (:312)
    if k >= 12:
        return 16, 4, 3, False  # :315  kAgg16TW, kAgg16TH, kAgg16PF (:312)
    return 8, 8, 2, False       # :316


def list_capacity(k):
    """cap_hits = kAggCap - kAggU = kAggFlush + 64 kAggPF (:41, :168)."""
    return FLUSH + 64 * tile_config(k)[2]


def uses_vec4(k, N, scalar_scan=False):
    """:305  four candidates per lane when the matches come in fours, 8 x 8 tiles only."""
    return N % 4 == 0 and k < 12 and not scalar_scan


def grid_coords(size, k, nHW, p):
    """Reference-grid coordinates along one axis: nHW + i p, plus a forced last index (utilities.cpp:697-712)."""
    max_size, v, ind = size - k + 1, [], nHW
    while ind < max_size - nHW:
        v.append(ind)
        ind += p
    if v[-1] < max_size - nHW - 1:
        v.append(max_size - nHW - 1)
    return np.array(v, np.int64)


def kaiser_table(k):
    """The Kaiser window of bm3d.cpp:1101-1146: two tables, for k = 8 and 12; ones for any other size.  [k*k] float32."""
    q8 = [[0.1924, 0.2989, 0.3846, 0.4325], [0.2989, 0.4642, 0.5974, 0.6717],
          [0.3846, 0.5974, 0.7688, 0.8644], [0.4325, 0.6717, 0.8644, 0.9718]]
    q12 = [[0.1924, 0.2615, 0.3251, 0.3782, 0.4163, 0.4362], [0.2615, 0.3554, 0.4419, 0.5139, 0.5657, 0.5927],
           [0.3251, 0.4419, 0.5494, 0.6390, 0.7033, 0.7369], [0.3782, 0.5139, 0.6390, 0.7433, 0.8181, 0.8572],
           [0.4163, 0.5657, 0.7033, 0.8181, 0.9005, 0.9435], [0.4362, 0.5927, 0.7369, 0.8572, 0.9435, 0.9885]]
    if k not in (8, 12):
        return np.ones(k * k, np.float32)
    q = np.array(q8 if k == 8 else q12, np.float32)
    full = np.block([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]])
    return np.ascontiguousarray(full.reshape(-1))


def Geom(**kw):
    """A launch's geometry and switches.  Defaults: the regular grid of the window, the whole pass, every SAI there, none processed."""
    g = SimpleNamespace(pst=None, irregular=0, wchan0=0, direct=0, lf_stride=0, sai=None, mask=None, proc=None,
                        ref_begin=0, n_groups=None, filt_sai_stride=0, n_ref_rows=None, n_ref_cols=None, R=None)
    g.__dict__.update(kw)
    g.nHW = g.nSim + g.nDisp
    if g.pst is None:
        g.pst = g.A // 2
    if g.n_ref_rows is None:
        g.n_ref_rows = len(grid_coords(g.Hb, g.k, g.nHW, g.p))
        g.n_ref_cols = len(grid_coords(g.Wb, g.k, g.nHW, g.p))
    if g.R is None:
        g.R = g.n_ref_rows * g.n_ref_cols
    if g.n_groups is None:
        g.n_groups = g.R - g.ref_begin
    g.mask = np.ones(g.A, np.uint32) if g.mask is None else np.asarray(g.mask, np.uint32)
    g.proc = np.zeros(g.A, np.uint32) if g.proc is None else np.asarray(g.proc, np.uint32)
    return g


def band(g, ref_begin, n_groups):
    b = SimpleNamespace(**g.__dict__)
    b.ref_begin, b.n_groups = ref_begin, n_groups
    return b


def live_slots(g):
    return [st for st in range(g.A) if g.mask[st] and not g.proc[st]]   # :55-56


def dense_patches(filt, g, ref_begin=0):
    """patches() over a dense filt of the groups from ref_begin on: group-major [g][n][st][c][k2], or SAI-major (filt_sai_stride > 0)."""
    k2 = g.k * g.k
    if g.filt_sai_stride:
        f = filt.reshape(g.A, -1)[:, :g.filt_sai_stride]
        return lambda gi, n, st: f[st, ((gi - ref_begin) * g.N + n) * g.C * k2:][:g.C * k2].reshape(g.C, k2)
    f = filt.reshape(-1, g.N, g.A, g.C, k2)
    return lambda gi, n, st: f[gi - ref_begin, n, st]


def _sums_view(g, buf, st):
    """(the [C][H][W] block of slot st inside the flat sums, row / column of its first pixel in padded coordinates)"""
    if g.direct:
        W, H = g.Wb - 2 * g.nHW, g.Hb - 2 * g.nHW
        o = int(g.sai[st]) * g.lf_stride
        return buf[o:o + g.C * W * H].reshape(g.C, H, W), g.nHW
    return buf[st * g.C * g.Wb * g.Hb:(st + 1) * g.C * g.Wb * g.Hb].reshape(g.C, g.Hb, g.Wb), 0


def aggregate(g, num, den, patches, wgt, aggpos, kaiser, dtype=np.float32):
    """One launch: returns new (num, den).  dtype = np.float64 gives the same scatter in double, as a cross-check of the model."""
    num, den = num.astype(dtype), den.astype(dtype)   # copies
    k, C = g.k, g.C
    kai = kaiser.astype(dtype).reshape(k, k)
    for st in live_slots(g):
        vn, org = _sums_view(g, num, st)
        vd, _ = _sums_view(g, den, st)
        if g.direct:   # scatter in padded coordinates, keep the interior (the kernel's tiles cover nothing else)
            pn, pd = np.zeros((C, g.Hb, g.Wb), dtype), np.zeros((C, g.Hb, g.Wb), dtype)
            inner = (slice(None), slice(org, g.Hb - org), slice(org, g.Wb - org))
            pn[inner], pd[inner] = vn, vd
        else:
            pn, pd = vn, vd
        pos_st = aggpos[st]
        with np.errstate(invalid="ignore", over="ignore"):
            for gi in range(g.ref_begin, g.ref_begin + g.n_groups):          # raster (list) order
                row = pos_st[gi]
                if (row == ABSENT).all():
                    continue
                w = wgt[gi].astype(dtype)
                kw = np.stack([kai * w[0 if g.wchan0 else c] for c in range(C)])   # kw = float32(kaiser * w), [C][k][k]
                for n in range(g.N):                                         # then the match index
                    p = int(row[n])
                    if p == ABSENT:
                        continue
                    py, px = p >> 16, p & 0xFFFF
                    val = patches(gi, n, st).astype(dtype).reshape(C, k, k)
                    pd[:, py:py + k, px:px + k] += kw                        # den += kw
                    pn[:, py:py + k, px:px + k] += kw * val                  # num += float32(kw * val): two roundings, no fma
        if g.direct:
            vn[...], vd[...] = pn[inner], pd[inner]
    return num, den


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays; two NaNs count as equal whatever their sign and payload (IEEE 754 leaves the
    NaN an invalid operation produces to the implementation: x86 and gfx950 differ in its sign)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check_reach(g, aggpos, refs_yx):
    """The kernel's precondition: every patch lies within the search reach of its reference -- nSim in slot pst, nSim + nDisp in the
    others (:63) -- and inside the window.  refs_yx: int [R][2].  Returns the number of violations."""
    bad = 0
    for st in range(g.A):
        reach = g.nSim if st == g.pst else g.nHW
        p = aggpos[st].astype(np.int64)
        there = p != ABSENT
        py, px = p >> 16, p & 0xFFFF
        dy, dx = np.abs(py - refs_yx[:, 0:1]), np.abs(px - refs_yx[:, 1:2])
        bad += int((there & ((dy > reach) | (dx > reach) | (py > g.Hb - g.k) | (px > g.Wb - g.k))).sum())
    return bad


def census(g, aggpos, scalar_scan=False):
    """Path bookkeeping of one launch.  Returns a namespace: `tiles`, a list of per-tile records (slot, tile_x, tile_y, r_lo, r_hi,
    c_lo, c_hi, n_cand, hits per scan round, carry into each round, overflow flags, mul_div), and totals over them."""
    k, N = g.k, g.N
    TW, TH, PF, _ = tile_config(k)
    cap = list_capacity(k)
    vec4 = uses_vec4(k, N, scalar_scan)
    rnd = VEC4_ROUND if vec4 else 64 * PF                                   # candidates per scan round (:225, :231)
    logN = N.bit_length() - 1
    org = g.nHW if g.direct else 0                                          # :48
    Wt, Ht = g.Wb - 2 * org, g.Hb - 2 * org
    gx, gy = -(-Wt // TW), -(-Ht // TH)
    last_r, last_c = g.Hb - k - g.nHW, g.Wb - k - g.nHW                     # :68
    Af = 1 if g.filt_sai_stride else g.A                                    # :104
    small24 = ((g.R << logN) + 1) * Af < (1 << 24)                          # :107

    def lo_idx(v):                                                          # :69
        d = v - g.nHW
        return 0 if d <= 0 else (d + g.p - 1) // g.p

    def hi_idx(v, n, lastv):                                                # :70-74
        if v >= lastv:
            return n - 1
        d = v - g.nHW
        if d < 0:
            return -1
        return min(d // g.p, n - 2)

    g_end = g.ref_begin + g.n_groups
    out = SimpleNamespace(tiles=[], small24=small24, vec4=vec4, cap=cap, round=rnd, n_overflow=0, n_exact_fill=0, n_exact_div=0,
                          n_clamped_lo=0, n_partial=0, n_tiles=0, max_carry=0)
    for st in live_slots(g):
        reach = g.nSim if st == g.pst else g.nHW                            # :63
        pos = aggpos[st].reshape(-1, N)
        for ty in range(gy):
            for tx in range(gx):
                tx0, ty0 = org + tx * TW, org + ty * TH                     # :57
                r_lo, r_hi = lo_idx(ty0 - k + 1 - reach), hi_idx(ty0 + TH - 1 + reach, g.n_ref_rows, last_r)   # :75
                c_lo, c_hi = lo_idx(tx0 - k + 1 - reach), hi_idx(tx0 + TW - 1 + reach, g.n_ref_cols, last_c)   # :76
                clamped = r_lo > g.n_ref_rows - 1 or c_lo > g.n_ref_cols - 1
                r_lo, c_lo = min(r_lo, g.n_ref_rows - 1), min(c_lo, g.n_ref_cols - 1)                          # :77-78
                if not g.irregular and g.n_ref_cols:                        # :83-86  the band's rows only
                    r_lo = max(r_lo, g.ref_begin // g.n_ref_cols)
                    r_hi = min(r_hi, (g_end - 1) // g.n_ref_cols)
                span = c_hi - c_lo + 1
                n_rr = g.n_groups if g.irregular else ((r_hi - r_lo + 1) * span if r_hi >= r_lo and c_hi >= c_lo else 0)   # :89
                n_cand = n_rr << logN
                if n_cand == 0:
                    continue                                                # :91
                mul_div = (not g.irregular) and n_rr * span < (1 << 20)     # :98
                rr = np.arange(n_rr)
                if g.irregular:
                    gi = g.ref_begin + rr                                   # :181 / :240
                else:
                    gi = (r_lo + rr // span) * g.n_ref_cols + c_lo + rr % span   # :185 / :245, with the exact quotient
                inb = (gi >= g.ref_begin) & (gi < g_end)                    # :187 / :247
                p = np.where(inb[:, None], pos[np.where(inb, gi, 0)], ABSENT).astype(np.int64).reshape(-1)
                py, px = p >> 16, p & 0xFFFF
                hit = (p != ABSENT) & (py < ty0 + TH) & (py + k > ty0) & (px < tx0 + TW) & (px + k > tx0)    # :193 / :264
                n_rounds = -(-n_cand // rnd)
                padded = np.zeros(n_rounds * rnd, np.int64)
                padded[:n_cand] = hit
                hits = padded.reshape(n_rounds, rnd).sum(1)
                nh, carries, over, exact = 0, [], [], []
                for j in range(n_rounds):
                    carries.append(nh)
                    if vec4 and nh + hits[j] > cap:                         # :201, :226-227
                        over.append(True)
                        exact.append(False)
                        nh = int(padded[j * rnd + rnd - VEC4_RUN:(j + 1) * rnd].sum())   # the last run's hits stay in the list
                    else:
                        over.append(False)
                        exact.append(nh > 0 and nh + hits[j] == cap)
                        nh += int(hits[j])
                    if nh >= FLUSH:                                         # :228 / :284
                        nh = 0
                partial = tx0 + TW > org + Wt or ty0 + TH > org + Ht
                out.tiles.append(SimpleNamespace(st=st, tx=tx, ty=ty, r_lo=r_lo, r_hi=r_hi, c_lo=c_lo, c_hi=c_hi, n_cand=n_cand,
                                                 hits=hits, carry=carries, overflow=over, exact_fill=exact, mul_div=mul_div,
                                                 clamped_lo=clamped, partial=partial))
                out.n_tiles += 1
                out.n_overflow += any(over)
                out.n_exact_fill += any(exact)
                out.n_exact_div += not mul_div and not g.irregular
                out.n_clamped_lo += clamped
                out.n_partial += partial
                out.max_carry = max(out.max_carry, max(carries))
    return out
