"""A numpy model of the correlated-noise feature (include/lfbm5d_corr.h): the definition the library is held to.

  - the autocorrelation of filtered white noise and the variance table v[pq] = (M R M^T)[pq][pq] / (M M^T)[pq][pq] of a 2-D transform,
    M from tests/group_model.transform_2d, R the block-Toeplitz matrix of the autocorrelation, clamped from below at 1 / 64;
  - the block autocovariance measurement, operation by operation in the order the header states (float64 adds and multiplies, no
    fused multiply-add): lfbm5d_corr_measure_* returns the same bits;
  - the group stage of tests/group_model.py extended by the table: fibre (st, pq) is thresholded at T s[pq] and Wiener-shrunk
    against sigma^2 v[pq], the group weight sums v[pq] per survivor or value v[pq]; `compare` is group_model.compare with
    per-coefficient thresholds and weights that are sums of v, not counts;
  - the cases of tests/test_gpu_corr_group.py (built with group_cases.build) and the test data of the estimator's figures.
"""
import math

import numpy as np

import group_cases as K
import group_model as M

FLOOR = 1.0 / 64.0
TABLE_TAPS_WIDTH = 0.8      # the non-trivial table of the group tests: Gaussian taps of this width
LAGS = [(0, dx) for dx in range(4)] + [(dy, dx) for dy in range(1, 4) for dx in range(-3, 4)]
CHUNK = 256
WHITE = np.zeros((7, 7))
WHITE[3, 3] = 1.0


# ---- the noise description ----
def check(acf):
    """None if acf is an autocorrelation as the header defines it, else what is wrong with it."""
    a = np.asarray(acf, np.float64)
    if a.shape != (7, 7):
        return "shape"
    if not np.isfinite(a).all() or (np.abs(a) > 1).any():
        return "not a finite value of magnitude at most 1"
    if a[3, 3] != 1.0:
        return "must be 1 at lag 0"
    if not np.array_equal(a, a[::-1, ::-1]):
        return "point-symmetric"
    return None


def from_kernel(g):
    """acf(dy, dx) = sum g[y][x] g[y + dy][x + dx] / sum g^2 at the 7 x 7 lags."""
    g = np.atleast_2d(np.asarray(g, np.float64))
    gh, gw = g.shape
    e = (g * g).sum()
    acf = np.zeros((7, 7))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            s = 0.0
            for y in range(gh):
                for x in range(gw):
                    if 0 <= y + dy < gh and 0 <= x + dx < gw:
                        s += g[y, x] * g[y + dy, x + dx]
            acf[3 + dy, 3 + dx] = s / e
    acf[3, 3] = 1.0
    return acf


def gaussian_taps(width, size=7):
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2
    g = np.exp(-0.5 * (x / float(width)) ** 2)
    g = np.outer(g, g)
    return g / np.sqrt((g * g).sum())


def toeplitz(acf, k):
    """R [k^2][k^2]: R[(y, x)][(y', x')] = acf[3 + y' - y][3 + x' - x] within the 7 x 7 lags, 0 outside."""
    acf = np.asarray(acf, np.float64)
    y, x = np.divmod(np.arange(k * k), k)
    dy, dx = y[None, :] - y[:, None], x[None, :] - x[:, None]
    inside = (np.abs(dy) <= 3) & (np.abs(dx) <= 3)
    return np.where(inside, acf[np.clip(dy, -3, 3) + 3, np.clip(dx, -3, 3) + 3], 0.0)


def table_raw(acf, tau2, k):
    """v [k^2] before the floor."""
    tau2 = M.TAU[tau2] if isinstance(tau2, str) else tau2
    if tau2 == M.ID:
        return np.ones(k * k)
    T = M.transform_2d(tau2, k, True)
    R = toeplitz(acf, k)
    return np.einsum("ij,jk,ik->i", T, R, T) / (T * T).sum(axis=1)


def table(acf, tau2, k):
    """(s, v, clamped): v clamped from below at 1 / 64, s = sqrt(v), float64."""
    raw = table_raw(acf, tau2, k)
    low = ~(raw >= FLOOR)
    v = np.where(low, FLOOR, raw)
    return np.sqrt(v), v, int(low.sum())


def log2_rms(v, truth):
    """Root-mean-square log2 error of a table against the true one, both clamped."""
    a, b = np.maximum(np.asarray(v, np.float64), FLOOR), np.maximum(np.asarray(truth, np.float64), FLOOR)
    return float(np.sqrt(np.mean(np.log2(a / b) ** 2)))


# ---- the measurement ----
def blocks_of(lf, mask, B):
    """[n][B][B] float64: every whole B x B block of every non-empty SAI and channel of lf [A][C][H][W], in the header's order."""
    lf = np.asarray(lf)
    A, C, H, W = lf.shape
    bh, bw = H // B, W // B
    out = []
    for st in range(A):
        if not mask[st]:
            continue
        for c in range(C):
            p = lf[st, c, :bh * B, :bw * B].astype(np.float64)
            out.append(p.reshape(bh, B, bw, B).transpose(0, 2, 1, 3).reshape(-1, B, B))
    return np.concatenate(out)


def block_lags(blocks):
    """A [n][25]: the lag sums of every block, every operation in the header's order."""
    n, B, _ = blocks.shape
    r = np.zeros((n, B))
    for x in range(B):
        r = r + blocks[:, :, x]
    s = np.zeros(n)
    for y in range(B):
        s = s + r[:, y]
    d = blocks - (s / float(B * B))[:, None, None]
    A = np.zeros((n, len(LAGS)))
    for l, (dy, dx) in enumerate(LAGS):
        x0, x1 = max(0, -dx), min(B, B - dx)
        p = np.zeros((n, B - dy))
        for x in range(x0, x1):
            p = p + d[:, :B - dy, x] * d[:, dy:, x + dx]
        a = np.zeros(n)
        for y in range(B - dy):
            a = a + p[:, y]
        A[:, l] = a
    return A


def measure(lf, mask, B=16, fraction=0.1):
    """dict(acf [7][7], sigma, blocks, selected, cut): lfbm5d_corr_measure_* of lf [A][C][H][W] (float32)."""
    A = block_lags(blocks_of(lf, mask, B))
    n = A.shape[0]
    score = A[:, 0]
    kth = max(1, min(n, int(math.ceil(fraction * n))))
    cut = float(np.partition(score, kth - 1)[kth - 1])
    sel = score <= cut
    pad = (-n) % CHUNK
    Ap = np.concatenate([A, np.zeros((pad, A.shape[1]))]).reshape(-1, CHUNK, A.shape[1])
    sp = np.concatenate([sel, np.zeros(pad, bool)]).reshape(-1, CHUNK)
    part = np.zeros((Ap.shape[0], A.shape[1]))
    for j in range(CHUNK):
        part = part + np.where(sp[:, j, None], Ap[:, j], 0.0)
    S = np.zeros(A.shape[1])
    for c in range(part.shape[0]):
        S = S + part[c]
    n_sel = int(sel.sum())
    acf = WHITE.copy()
    C0 = S[0] / float(n_sel * B * B)
    sigma = 0.0
    if C0 > 0.0:
        for l, (dy, dx) in enumerate(LAGS[1:], 1):
            r = min(1.0, max(-1.0, (S[l] / float(n_sel * (B - dy) * (B - abs(dx)))) / C0))
            acf[3 + dy, 3 + dx] = acf[3 - dy, 3 - dx] = r
        sigma = math.sqrt(C0 * float(B * B) / float(B * B - 1))
    return dict(acf=acf, sigma=sigma, blocks=n, selected=n_sel, cut=cut)


# ---- the group stage with a table ----
def run(case, s_tab, v_tab, dtype=np.float64):
    """group_model.run with the table (s_tab, v_tab [k^2], the float32 values the kernels take): returns the same dict, T [R][C][k2]."""
    s32, v32 = np.asarray(s_tab, np.float32), np.asarray(v_tab, np.float32)
    pos, present, zero, in_shape, aggpos = M.positions(case)
    take = present & ~zero
    S = M.gather(case, case.noisy, pos, take, dtype)
    Mx = np.abs(S).max(axis=(1, 2, 4)).astype(np.float64)
    ch = M.Chain(case, in_shape, dtype)
    R, N, A, C, k2 = S.shape
    valid = (np.arange(N)[None, :] < case.self_cnt[:, None])[:, :, None, None, None] & ch.support[:, None, :, None, None]
    sig = np.asarray(case.sigma[:C], np.float64)
    out = dict(nSx=case.self_cnt.astype(np.int64), use_sadct=ch.use_sadct.copy(), aggpos=aggpos, chain=ch, valid=valid)
    X = ch.fwd(S)
    vb = v32.astype(dtype)[None, None, None, None, :]
    if case.step == 1:
        # T s[pq] in the kernels' float32 expression, then the stack transform's factor
        T32 = M.thresholds(case)[:C].astype(np.float32)
        Tc = (T32[:, None] * s32[None, :]).astype(np.float64)                      # [C][k2]
        T = Tc[None] * ch.tfac[:, None, None]                                      # [R][C][k2]
        Tb = T[:, None, None]
        keep = (np.abs(X) > Tb.astype(dtype)) & valid
        gap = M.gap_of(Mx[:, :, None], T)[:, None, None]
        near = (np.abs(np.abs(X.astype(np.float64)) - Tb) <= gap) & valid
        count = keep.sum(axis=(1, 2, 4))
        Xf = np.where(keep | ~valid, X, 0)
        wsum = np.where(keep, vb, 0).sum(axis=(1, 2, 4), dtype=dtype).astype(np.float64)
        out.update(count=count, ingap=near.sum(axis=(1, 2, 4)), near=near, coef=X, T=T)
    else:
        P = M.gather(case, case.basic, pos, take, dtype)
        Mx = np.maximum(Mx, np.abs(P).max(axis=(1, 2, 4)))
        E = ch.fwd(P)
        s2 = (sig.astype(dtype) ** 2)[None, None, None, :, None] * vb
        if case.tau5 == M.HADAMARD:
            val = E * E * (1.0 / case.self_cnt.astype(dtype))[:, None, None, None, None]
        else:
            val = E * E
        val = val / (val + s2)
        Xf = np.where(valid, X * val, 0)
        wsum = np.where(valid, val * vb, 0).sum(axis=(1, 2, 4), dtype=dtype).astype(np.float64)
    F4 = ch.inv5(Xf)
    with np.errstate(divide="ignore", over="ignore"):
        sg = sig[None, :]
        w = np.where(wsum > 0, np.where(sg > 0, 1 / (sg * sg * np.where(wsum > 0, wsum, 1)), 1 / np.where(wsum > 0, wsum, 1)), 1.0)
    out.update(filt=ch.inv45(F4), w=w, wsum=wsum, M=Mx)
    return out


def compare(case, m, filt, w, v_tab, sl=None):
    """group_model.compare for a model of `run`: thresholds per coefficient, weights that are sums of v.  A coefficient inside the gap
    that the result decided the other way is found from the result's own forward transform; its contribution is added back before
    the values are compared, and its v is added to (taken off) the weight's sum.  Returns err, E_filt, rel_w, E_w, open_pairs, pairs."""
    sl = slice(0, case.R) if sl is None else sl
    ch = m["chain"]
    v64 = np.asarray(v_tab, np.float32).astype(np.float64)
    cmp_ = (m["aggpos"] != M.ABSENT).transpose(1, 2, 0)[sl]
    want = m["filt"][sl]
    diff = np.where(cmp_[..., None, None], filt.astype(np.float64) - want, 0.0)
    M_ = m["M"][sl]
    sig = np.asarray(case.sigma[:case.C], np.float64)
    out = dict(open_pairs=0, pairs=M_.size)
    groups = np.arange(case.R)[sl]
    wm = m["w"][sl].copy()
    if case.step == 1:
        near, X, keep_T = m["near"][sl], m["coef"][sl], m["T"][sl]
        open_ = m["ingap"][sl] > 0
        out["open_pairs"] = int(open_.sum())
        if open_.any():
            o = np.flatnonzero(open_.any(axis=1))
            go = groups[o]
            D = ch.fwd(diff[o], go)
            Xo = X[o]
            kept = np.abs(Xo) > keep_T[o][:, None, None]
            s = np.where(kept, -1.0, 1.0)
            flip = near[o] & (np.abs(D - s * Xo) < 0.5 * np.abs(Xo))
            diff[o] -= np.where(cmp_[o][..., None, None], ch.inv(np.where(flip, s * Xo, 0.0), go), 0.0)
            ws = m["wsum"][sl].copy()
            ws[o] += (flip * s * v64[None, None, None, None, :]).sum(axis=(1, 2, 4))
            with np.errstate(divide="ignore"):
                wm = np.where(ws > 0, 1 / (sig[None, :] ** 2 * np.where(ws > 0, ws, 1)), 1.0)
    out["got"], out["want"] = filt, want
    out["err"] = np.abs(diff) / np.where(M_ > 0, M_, 1.0)[:, None, None, :, None]
    out["E_filt"] = float(out["err"].max()) if not np.isnan(out["err"]).any() else float("nan")
    huge = wm > 1e30
    out["huge_bad"] = [(int(groups[g]), int(c), float(w[g, c])) for g, c in zip(*np.nonzero(huge & ~(w > 1e30)))]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rel = np.where((wm == w) | huge, 0.0, np.abs(w.astype(np.float64) - wm) / np.abs(wm))
    out["rel_w"] = rel
    out["E_w"] = float(rel.max())
    return out


def reference(case, s_tab, v_tab):
    """model: run in float64; second: the same code in float32 compared with it; E_filt, E_w: the float32 round-off the kernels are
    held to 4 x of."""
    m = run(case, s_tab, v_tab)
    m32 = run(case, s_tab, v_tab, np.float32)
    with np.errstate(over="ignore"):
        w32 = m32["w"].astype(np.float32)
    rs = compare(case, m, m32["filt"], w32, v_tab)
    return dict(model=m, second=rs, E_filt=rs["E_filt"], E_w=rs["E_w"])


def expected_kernels(case):
    """The kernel text of lfbm5d_debug_group_corr: the pre-pass, then the general kernels' table forms."""
    big_a = case.A > K.MAX_A
    stack = case.N * case.A * case.k * case.k
    rows_form = (case.tau2 == M.BIOR and case.k in (8, 16)) or (case.tau2 == M.DCT and case.k in (8, 12, 16))
    tmp = (256 // case.k) * case.k * (case.k + 1) if rows_form else max(256, case.k * case.k)
    lds = ((2 if case.step == 2 else 1) * stack + tmp) * 4
    head = ["k_group_pos", "k_group_shape<%s>" % ("true" if big_a else "false")]
    if lds > K.GENERIC_LDS_LIMIT or big_a:
        return head + ["k_group_big_corr<%d, %s>" % (case.step, "true" if big_a else "false")]
    return head + ["k_group_corr<%d>" % case.step]


def correlate(case, taps):
    """The window of a built case with its fluctuations filtered by the unit-energy taps (periodic): the noise group_cases.texture put
    in becomes noise of autocorrelation from_kernel(taps) at the same marginal level, which is what a table is for -- under white
    noise the table's small high-frequency thresholds sit in the bulk of the noise and every other pair has a coefficient inside
    the gap.  Each plane keeps its mean; empty SAIs (NaN planes) stay as they are."""
    g = np.asarray(taps, np.float64)
    g = g / np.sqrt((g * g).sum())
    gh, gw = g.shape
    img = case.noisy.reshape(case.A, case.C, case.Hb, case.Wb)
    for st in range(case.A):
        if not case.mask[st]:
            continue
        for c in range(case.C):
            p = img[st, c].astype(np.float64)
            m = p.mean()
            z = np.zeros_like(p)
            for y in range(gh):
                for x in range(gw):
                    z += g[y, x] * np.roll(p - m, (y - gh // 2, x - gw // 2), axis=(0, 1))
            img[st, c] = (m + z).astype(np.float32)
    return case


def group_cases():
    """The cases of tests/test_gpu_corr_group.py: built with group_cases.build, their windows then carry noise of the autocorrelation
    the non-trivial table is made for (`correlate`; Gaussian taps of width TABLE_TAPS_WIDTH).  Hard-threshold seeds and levels are
    chosen on the CPU (tests/test_corr.py asserts it) so that at least 90 % of the (group, channel) pairs have no coefficient inside
    group_model.gap_of of its threshold under that table."""
    out = []
    taps = gaussian_taps(TABLE_TAPS_WIDTH)
    add = lambda *a, **kw: out.append(correlate(K.build(*a, **kw), taps))
    one_missing = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], np.uint32)
    w5 = K.wide_shapes(np.random.default_rng(7), 5, 12, 40)
    add("corr-ht-dct-haar-k8", 901, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", n_groups=96)
    add("corr-wien-dct-haar-k8", 902, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", n_groups=96)
    add("corr-ht-bior-haar-k8", 903, step=1, tau2="bior", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", n_groups=96)
    add("corr-ht-dct-hw-k4", 904, step=1, tau2="dct", tau4="sadct", tau5="hw", k=4, N=8, nsx="cycle", n_groups=96)
    add("corr-wien-bior-dct5-k4", 905, step=2, tau2="bior", tau4="sadct", tau5="dct", k=4, N=8, nsx="cycle", n_groups=96)
    add("corr-ht-dct-dct5-k4", 906, step=1, tau2="dct", tau4="dct", tau5="dct", k=4, N=8, nsx="cycle", n_groups=96)
    add("corr-wien-dct-haar-k8-1empty", 907, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, mask=one_missing, nsx="cycle", n_groups=96)
    add("corr-ht-dct-haar-k8-1empty", 908, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, mask=one_missing, nsx="cycle", n_groups=96)
    add("corr-ht-dct-haar-k8-5x5", 909, sigma=35.0, lam=3.5, amp=80.0, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=4, aw=5, shapes=w5, nsx="cycle", C=1)
    add("corr-wien-dct-haar-k8-5x5", 910, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, aw=5, shapes=w5, nsx="cycle", C=1)
    add("corr-wien-dct-haar-k16-5x5-big", 911, step=2, tau2="dct", tau4="sadct", tau5="haar", k=16, N=8, aw=5, shapes=w5[:12], nsx="cycle", C=1)
    w9 = K.thin(np.random.default_rng(1912), 9, 40, 16)
    add("corr-wien-dct-haar-k8-9x9", 912, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=4, aw=9, shapes=w9, n_groups=16, nsx="cycle", C=1)
    add("corr-ht-dct-haar-k8-n2-9x9", 913, sigma=35.0, lam=3.5, amp=80.0, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=2, aw=9, shapes=w9, n_groups=16, nsx="cycle", C=1)
    return out
