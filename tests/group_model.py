"""A numpy model of the group stage of a core pass (core:277-481 / :1054-1282), written from the definitions of its transforms.

    gather -> 2-D transform -> angular transform -> transform along the stack -> hard threshold | Wiener -> group weight -> inverses

Every transform is a matrix built from its published definition in float64 (orthonormal DCT-II, the bior1.5 filter bank with periodic
extension, the shape-adaptive DCT's row-then-column packing, Haar, Hadamard), applied to all groups of a case at once.  `run` takes
the tables block matching would produce (refs, self_idx, self_cnt, best, shape) and returns what lfbm5d_debug_group returns, plus
the decision record of the hard threshold: for every (group, channel) the survivor count, how many coefficients lie within `gap`
of their threshold and where.  With dtype=float32 the same code is a second float32 evaluation of the chain (matrix products instead
of the kernels' butterflies): tests/test_group_model.py measures float32 round-off with it and with the oracle.

Scales are the reference's, not the textbook's: the shape-adaptive DCT and the DCT along the stack leave 1-D pieces longer than one
at twice the orthonormal scale (core:3229-3276), the Hadamard transform is unnormalised, and the hard threshold of each is
lambda sigma_c sqrt2 times the matching factor (core:2431).  tests/test_oracle_*.py tie those to the compiled reference.

A case with `bm3d` set is the per-SAI BM3D flavour (bm3d.cpp:315-690): one image, no angular transform, Hadamard along stacks of
2 .. N patches, the threshold lambda sigma_c without the sqrt2 (bm3d.cpp:941), the SD weight over nSx k^2 values (:1345-1373).
"""
import functools

import numpy as np

ID, DCT, SADCT, BIOR, HADAMARD, HAAR = 4, 5, 6, 7, 8, 9
TAU = {"id": ID, "dct": DCT, "sadct": SADCT, "bior": BIOR, "hw": HADAMARD, "haar": HAAR}
ABSENT = 0xFFFFFFFF
EPS32 = float(np.finfo(np.float32).eps)
K_GUARD = 3.5e-5     # the largest entry of kHtGuardAbs (lfbm5d_kernels.h)
SQRT2 = np.sqrt(2.0)


def gap_of(M, T):
    """Half-width of the band around a threshold T inside which two float32 evaluations of the chain may decide differently."""
    return 4 * K_GUARD * M + 16 * EPS32 * T


# ---- the transforms as matrices (float64) ----
@functools.lru_cache(None)
def dct_ortho(n):
    """Orthonormal DCT-II of length n: y = D x."""
    j = np.arange(n)
    D = np.cos(np.pi * (j[None, :] + 0.5) * j[:, None] / n) * np.sqrt(2.0 / n)
    D[0] /= SQRT2
    return D


@functools.lru_cache(None)
def haar_matrix(n):
    """Orthonormal Haar of length n (a power of two): averages in front, the details of each level behind them, finest last."""
    M = np.eye(n)
    m = n
    while m > 1:
        h = m // 2
        S = np.eye(n)
        S[:m] = 0
        for i in range(h):
            S[i, 2 * i] = S[i, 2 * i + 1] = 1 / SQRT2
            S[h + i, 2 * i], S[h + i, 2 * i + 1] = 1 / SQRT2, -1 / SQRT2
        M = S @ M
        m = h
    return M


@functools.lru_cache(None)
def hadamard_matrix(n):
    """Unnormalised Hadamard of length n in the reference's order (lib_transforms.cpp:290-321): sums of neighbours to the first half,
    differences to the second, both halves again."""
    if n == 1:
        return np.ones((1, 1))
    h = n // 2
    S = np.zeros((n, n))
    for i in range(h):
        S[i, 2 * i] = S[i, 2 * i + 1] = 1
        S[h + i, 2 * i], S[h + i, 2 * i + 1] = 1, -1
    if n == 2:
        return S
    H = hadamard_matrix(h)
    B = np.zeros((n, n))
    B[:h, :h] = H
    B[h:, h:] = H
    return B @ S


BIOR_CN = 1 / (SQRT2 * 128)
BIOR_LPD = np.array([3, -3, -22, 22, 128, 128, 22, -22, -3, 3], float) * BIOR_CN
BIOR_HPD = np.array([0, 0, 0, 0, -1, 1, 0, 0, 0, 0], float) / SQRT2
BIOR_LPR = np.array([0, 0, 0, 0, 1, 1, 0, 0, 0, 0], float) / SQRT2
BIOR_HPR = np.array([3, 3, -22, -22, 128, -128, 22, 22, -3, -3], float) * BIOR_CN


def _bior_fwd_1d(n1):
    """One analysis level on a periodic signal of length n1 (lib_transforms.cpp:46-120): sample j of the extension is x[(j - 4) mod n1];
    low[j] = sum_t ext[t + 2 j] lpd[t] in front, high[j] behind."""
    A = np.zeros((n1, n1))
    h = n1 // 2
    for j in range(h):
        for t in range(10):
            A[j, (t + 2 * j - 4) % n1] += BIOR_LPD[t]
            A[h + j, (t + 2 * j - 4) % n1] += BIOR_HPD[t]
    return A


def _bior_inv_1d(n1):
    """One synthesis level (lib_transforms.cpp:135-204): sample i of the extension is x[(i - 2 n1) mod n1]; with n2 = n1 / 2,
    out[2 i] = sum_t hpr[t] ext[t n2 + i], out[2 i + 1] = sum_t lpr[t] ext[t n2 + i]."""
    A = np.zeros((n1, n1))
    n2 = n1 // 2
    for i in range(n2):
        for t in range(10):
            A[2 * i, (t * n2 + i - 4 * n2) % n1] += BIOR_HPR[t]
            A[2 * i + 1, (t * n2 + i - 4 * n2) % n1] += BIOR_LPR[t]
    return A


@functools.lru_cache(None)
def bior_2d(k, forward):
    """bior1.5 on a k x k patch as a k^2 x k^2 matrix: per level rows then columns of the leading block, which halves (forward);
    columns then rows of the leading block, which doubles (inverse)."""
    M = np.eye(k * k)
    sizes = []
    n1 = k
    while n1 > 1:
        sizes.append(n1)
        n1 //= 2
    for n1 in (sizes if forward else sizes[::-1]):
        L1 = _bior_fwd_1d(n1) if forward else _bior_inv_1d(n1)
        E = np.eye(k)
        E[:n1, :n1] = L1
        P = np.zeros((k, k))
        P[:n1, :n1] = np.eye(n1)
        # only the first n1 rows and columns take part in a level: the others are left alone
        rows_op = np.kron(P, E) + np.kron(np.eye(k) - P, np.eye(k))
        cols_op = np.kron(E, P) + np.kron(np.eye(k), np.eye(k) - P)
        M = (cols_op @ rows_op @ M) if forward else (rows_op @ cols_op @ M)
    return M


@functools.lru_cache(None)
def transform_2d(tau2, k, forward):
    """The k^2 x k^2 matrix of the 2-D patch transform (row-major patches), or None for the identity."""
    if tau2 == ID:
        return None
    if tau2 == DCT:
        D = dct_ortho(k)
        M = np.kron(D, D)
        return M if forward else M.T
    return bior_2d(k, forward)


def shape_support(mask, aw):
    """The shape-adaptive DCT's bookkeeping (core:302-323): the SAIs of each row pushed left (mask_col), then each column of that
    pushed up (mask_dct, the support of the coefficients)."""
    m = np.asarray(mask, bool).reshape(aw, aw)
    mask_col = np.zeros_like(m)
    for s in range(aw):
        mask_col[s, :m[s].sum()] = True
    mask_dct = np.zeros_like(m)
    for t in range(aw):
        mask_dct[:mask_col[:, t].sum(), t] = True
    return m, mask_col, mask_dct


@functools.lru_cache(None)
def sadct_matrices(bits, aw):
    """Forward and inverse shape-adaptive DCT of the shape `bits` (bit st = s aw + t) as A x A matrices, and mask_dct.
    Forward (core:1969-2116): each row's n SAIs are packed to the left and transformed -- left as they are for n = 1, twice the
    orthonormal DCT for n > 1 --, then the same down each column of the packed array, then everything times 1 / (2 sqrt2).
    Inverse (core:2131-2264): columns first -- times 2 sqrt2 for n = 1, sqrt2 times the orthonormal inverse for n > 1 --, then rows --
    as they are for n = 1, half the orthonormal inverse for n > 1 --, back to the SAIs' places."""
    A = aw * aw
    m, mask_col, mask_dct = shape_support([(bits >> i) & 1 for i in range(A)], aw)
    rows = np.zeros((A, A))
    for s in range(aw):
        src = np.flatnonzero(m[s])
        n = len(src)
        if n:
            rows[s * aw + np.arange(n)[:, None], s * aw + src[None, :]] = dct_ortho(n) * (2 if n > 1 else 1)
    cols = np.zeros((A, A))
    for t in range(aw):
        src = np.flatnonzero(mask_col[:, t])
        n = len(src)
        if n:
            cols[np.arange(n)[:, None] * aw + t, src[None, :] * aw + t] = dct_ortho(n) * (2 if n > 1 else 1)
    F = cols @ rows / (2 * SQRT2)
    icol = np.zeros((A, A))
    for t in range(aw):
        dst = np.flatnonzero(mask_col[:, t])
        n = len(dst)
        if n:
            icol[dst[:, None] * aw + t, np.arange(n)[None, :] * aw + t] = dct_ortho(n).T * (SQRT2 if n > 1 else 2 * SQRT2)
    irow = np.zeros((A, A))
    for s in range(aw):
        dst = np.flatnonzero(m[s])
        n = len(dst)
        if n:
            irow[s * aw + dst[:, None], s * aw + np.arange(n)[None, :]] = dct_ortho(n).T * (0.5 if n > 1 else 1)
    G = irow @ icol
    return F, G, mask_dct.reshape(-1)


@functools.lru_cache(None)
def fibre_matrices(tau5, n):
    """Forward and inverse transform along a stack of n patches, and the factor of the hard threshold that goes with its scale."""
    if tau5 == HAAR:
        H = haar_matrix(n)
        return H, H.T, 1.0
    if tau5 == HADAMARD:
        H = hadamard_matrix(n)
        return H, np.linalg.inv(H), float(np.sqrt(np.float32(n)))
    D = dct_ortho(n)   # twice the orthonormal scale (core:3262-3276, :2550-2593)
    return 2 * D, 0.5 * D.T, 2.0


# ---- geometry ----
def positions(case):
    """pos[g][n][st]: flat window position of every patch (-1: none), present: the patch exists, zero: it reads as zeros (the
    never-filled table column of the centre path, core:1697); aggpos as k_group_pos stores it (lfbm5d_group_generic.hip:37-52)."""
    R, N, A, Wb = case.R, case.N, case.A, case.Wb
    plane = Wb * case.Hb
    used = np.arange(N)[None, :] < case.self_cnt[:, None].astype(np.int64)
    ind = np.where(used, case.self_idx.reshape(R, N), 0).astype(np.int64)
    pos = np.full((R, N, A), -1, np.int64)
    for st in range(A):
        if not case.mask[st]:
            continue
        p = ind if st == case.pst else case.best.reshape(A, plane)[st][ind].astype(np.int64)
        pos[:, :, st] = np.where(used, p, -1)
    present = pos >= 0
    zero = present & (pos % Wb >= Wb - case.k) if case.fill_quirk else np.zeros_like(present)
    in_shape = np.zeros((R, A), bool)
    for st in range(A):
        in_shape[:, st] = True if st == case.pst else (bool(case.mask[st]) & (case.shape.reshape(A, plane)[st][case.refs] != 0))
    ok = present & (in_shape[:, None, :] if case.tau4 == SADCT and not case.bm3d else True)
    aggpos = np.where(ok, ((pos // Wb) << 16) | (pos % Wb), ABSENT).astype(np.uint32)
    return pos, present, zero, in_shape, np.ascontiguousarray(aggpos.transpose(2, 0, 1))   # aggpos [A][R][N]


def gather(case, img, pos, take, dtype):
    """S[g][n][st][c][k*k] from img [A][C][Hb][Wb]; patches outside `take` are zeros."""
    R, N, A, C, k = case.R, case.N, case.A, case.C, case.k
    img = np.asarray(img).reshape(A, C, case.Hb, case.Wb)
    p = np.where(take, pos, 0)
    r = (p // case.Wb)[..., None, None] + np.arange(k)[:, None]
    c = (p % case.Wb)[..., None, None] + np.arange(k)[None, :]
    S = np.empty((R, N, A, C, k * k), dtype)
    for st in range(A):
        for ch in range(C):
            S[:, :, st, ch] = np.where(take[:, :, st, None], img[st, ch][r[:, :, st], c[:, :, st]].reshape(R, N, k * k), 0)
    return S


class Chain:
    """The linear parts of a case's chain: per-group angular and stack matrices, the 2-D matrix."""

    def __init__(self, case, in_shape, dtype):
        self.case, self.dtype = case, dtype
        R, N, A = case.R, case.N, case.A
        aw = int(round(np.sqrt(A)))
        self.T2f, self.T2i = transform_2d(case.tau2, case.k, True), transform_2d(case.tau2, case.k, False)
        # a shape's bits as a Python int: 17 x 17 windows have 289 of them
        bits = np.array([sum(1 << int(i) for i in np.flatnonzero(row)) for row in in_shape], dtype=object)
        full = (1 << A) - 1
        tau4 = ID if case.bm3d else case.tau4      # the per-SAI BM3D flavour has one image: no angular transform whatever tau4 says
        self.use_sadct = (bits != full).astype(bool) if tau4 == SADCT else np.zeros(R, bool)
        self.support = np.ones((R, A), bool)     # in-shape coefficients (mask_dct) of every group
        self.A4f = self.A4i = None
        if tau4 != ID:
            D = dct_ortho(aw)
            Df = np.kron(D, D)
            self.A4f = np.broadcast_to(Df, (R, A, A)).copy()
            self.A4i = np.broadcast_to(Df.T, (R, A, A)).copy()
            for b in set(bits[self.use_sadct]):
                F, G, md = sadct_matrices(int(b), aw)
                sel = self.use_sadct & (bits == b).astype(bool)
                self.A4f[sel], self.A4i[sel], self.support[sel] = F, G, md
            self.A4f, self.A4i = self.A4f.astype(dtype), self.A4i.astype(dtype)
        self.A5f, self.A5i = np.zeros((R, N, N), dtype), np.zeros((R, N, N), dtype)
        self.tfac = np.ones(R)
        for n in np.unique(case.self_cnt):
            F, G, f = fibre_matrices(case.tau5, int(n))
            sel = case.self_cnt == n
            self.A5f[sel, :n, :n], self.A5i[sel, :n, :n], self.tfac[sel] = F, G, f
        if self.T2f is not None:
            self.T2f, self.T2i = self.T2f.astype(dtype), self.T2i.astype(dtype)

    def fwd(self, S, idx=slice(None)):
        """S [groups idx][N][A][C][k2] -> coefficients"""
        if self.T2f is not None:
            S = S @ self.T2f.T
        if self.A4f is not None:
            S = np.einsum("gij,gnjcp->gnicp", self.A4f[idx], S)
        return np.einsum("gmn,gnicp->gmicp", self.A5f[idx], S)

    def inv(self, X, idx=slice(None)):
        return self.inv45(self.inv5(X, idx), idx)

    def inv45(self, X, idx=slice(None)):   # from the filtered angular coefficients on
        if self.A4i is not None:
            X = np.einsum("gij,gnjcp->gnicp", self.A4i[idx], X)
        if self.T2i is not None:
            X = X @ self.T2i.T
        return X

    def inv5(self, X, idx=slice(None)):
        return np.einsum("gmn,gnicp->gmicp", self.A5i[idx], X)


def thresholds(case):
    """T[g][c]: lambda sigma_c sqrt2 in the kernels' float32 expression, times the scale factor of the stack transform.  The per-SAI
    BM3D flavour (bm3d.cpp:941) has lambda sigma_c without the sqrt2, and no lambda / sqrt2 rule: group_args_of_pass leaves its
    lambda alone."""
    lam = np.float32(case.lam)
    if case.bm3d:
        return np.array([np.float32(lam * np.float32(s)) for s in case.sigma], np.float64)
    if case.step == 1 and case.tau2 == ID and case.tau4 == DCT:
        lam = np.float32(lam / np.float32(SQRT2))   # core:206-207
    return np.array([np.float32(np.float32(lam * np.float32(s)) * np.float32(1.41421356237309505)) for s in case.sigma], np.float64)


def run(case, dtype=np.float64):
    """The whole group stage of `case`.  Returns a dict: filt [R][N][A][C][k2], w [R][C], nSx, use_sadct, aggpos [A][R][N], M [R][C]
    (largest |input|), and for step 1: count [R][C], ingap [R][C] (coefficients within gap of their threshold), near: the boolean
    array of those coefficients [R][N][A][C][k2], coef: the coefficients in front of the threshold."""
    pos, present, zero, in_shape, aggpos = positions(case)
    take = present & ~zero
    S = gather(case, case.noisy, pos, take, dtype)
    M = np.abs(S).max(axis=(1, 2, 4)).astype(np.float64)
    ch = Chain(case, in_shape, dtype)
    R, N, A, C, k2 = S.shape
    valid = (np.arange(N)[None, :] < case.self_cnt[:, None])[:, :, None, None, None] & ch.support[:, None, :, None, None]
    sig = np.asarray(case.sigma[:C], np.float64)
    out = dict(nSx=case.self_cnt.astype(np.int64), use_sadct=ch.use_sadct.copy(), aggpos=aggpos, chain=ch, valid=valid)
    X = ch.fwd(S)
    if case.step == 1:
        T = thresholds(case)[None, :C] * ch.tfac[:, None]                      # [R][C]
        Tb = T[:, None, None, :, None]
        keep = (np.abs(X) > Tb.astype(dtype)) & valid
        gap = gap_of(M, T)[:, None, None, :, None]
        near = (np.abs(np.abs(X.astype(np.float64)) - Tb) <= gap) & valid
        count = keep.sum(axis=(1, 2, 4))
        Xf = np.where(keep | ~valid, X, 0)    # coefficients outside the shape are left alone (they are zeros)
        wsum = count.astype(np.float64)
        out.update(count=count, ingap=near.sum(axis=(1, 2, 4)), near=near, coef=X, T=T)
    else:
        P = gather(case, case.basic, pos, take, dtype)
        M = np.maximum(M, np.abs(P).max(axis=(1, 2, 4)))
        E = ch.fwd(P)
        s2 = (sig.astype(dtype) ** 2)[None, None, None, :, None]
        if case.tau5 == HADAMARD:   # the unnormalised transform: the pilot's energy over nSx (core:2706-3123)
            v = E * E * (1.0 / case.self_cnt.astype(dtype))[:, None, None, None, None]
        else:
            v = E * E
        v = v / (v + s2)
        Xf = np.where(valid, X * v, 0)
        v = np.where(valid, v, 0)
        wsum = v.sum(axis=(1, 2, 4), dtype=dtype).astype(np.float64)
    F4 = ch.inv5(Xf)
    if case.useSD:   # sd_weighting_5d (core:3140-3173) on the filtered angular coefficients, Nn = nSx A; BM3D (bm3d.cpp:1345-1373): nSx k^2
        Nn = (case.self_cnt.astype(np.float64) * (k2 if case.bm3d else A))[:, None]
        m = F4.sum(axis=(1, 2, 4), dtype=dtype).astype(np.float64)
        q = (F4 * F4).sum(axis=(1, 2, 4), dtype=dtype).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            res = (q - m * m / Nn) / (Nn - 1)
            w = np.where(res > 0, 1 / np.sqrt(np.where(res > 0, res, 1)), 0.0)
        out["res"] = res
        with np.errstate(divide="ignore", invalid="ignore"):     # how much the subtraction amplifies the sums' round-off
            out["sd_cond"] = np.where(res != 0, (q + m * m / Nn) / (Nn - 1) / np.abs(res), np.inf)
    else:
        with np.errstate(divide="ignore", over="ignore"):
            sg = sig[None, :]
            w = np.where(wsum > 0, np.where(sg > 0, 1 / (sg * sg * np.where(wsum > 0, wsum, 1)), 1 / np.where(wsum > 0, wsum, 1)), 1.0)
    out.update(filt=ch.inv45(F4), w=w, wsum=wsum, M=M)
    return out


# ---- a result (the oracle's, the float32 evaluation's, the kernels') against the float64 model ----
def f32_ht_weight(sigma, count):
    """1 / (sigma_c^2 count) as the float32 expression of core:413-421 evaluates it; count 0 gives 1."""
    s = np.float32(sigma)
    with np.errstate(divide="ignore"):
        w = np.float32(1) / (np.float32(s * s) * count.astype(np.float32))
    return np.where(count > 0, w, np.float32(1)).astype(np.float32)


def compare(case, m, filt, w, sl=None):
    """filt [R'][N][A][C][k2] and w [R'][C] of the groups `sl` (a slice of the case's groups; default all) against the float64 model
    `m` = run(case).  Only what aggpos points at is compared.  Hard-threshold step: a (group, channel) with coefficients inside the
    gap is OPEN -- its count may differ by at most that many, and a coefficient inside the gap that was decided the other way is
    found from the result's own forward transform and its contribution added back before the values are compared.  With useSD the
    count cannot be recovered from the weight, so such a flip is cross-checked against nothing: whatever looks like one coefficient
    inside the gap decided the other way is taken off; the model alone bounds which coefficients those can be.
    Returns a dict: err [R'][N][A][C][k2] = |result - model| / M, E_filt, E_w, and the lists `count_bad`, `weight_bad` of
    (group, channel, got, want) that break the exact rules."""
    sl = slice(0, case.R) if sl is None else sl
    ch = m["chain"]
    R = case.R
    cmp_ = (m["aggpos"] != ABSENT).transpose(1, 2, 0)[sl]                  # [R'][N][A]
    want = m["filt"][sl]
    diff = np.where(cmp_[..., None, None], filt.astype(np.float64) - want, 0.0)
    M_ = m["M"][sl]
    sig = np.asarray(case.sigma[:case.C], np.float64)
    out = dict(count_bad=[], weight_bad=[], open_pairs=0, pairs=M_.size)
    groups = np.arange(R)[sl]
    if case.step == 1:
        near, X, keep_T = m["near"][sl], m["coef"][sl], m["T"][sl]
        open_ = m["ingap"][sl] > 0
        out["open_pairs"] = int(open_.sum())
        flips = np.zeros(M_.shape, np.int64)
        if open_.any():
            o = np.flatnonzero(open_.any(axis=1))            # the groups with an open channel
            go = groups[o]
            D = ch.fwd(diff[o], go)
            Xo = X[o]
            kept = np.abs(Xo) > keep_T[o][:, None, None, :, None]
            s = np.where(kept, -1.0, 1.0)
            flip = near[o] & (np.abs(D - s * Xo) < 0.5 * np.abs(Xo))
            flips[o] = (flip * s).sum(axis=(1, 2, 4)).astype(np.int64)
            diff[o] -= np.where(cmp_[o][..., None, None], ch.inv(np.where(flip, s * Xo, 0.0), go), 0.0)
        if not case.useSD:
            with np.errstate(divide="ignore", invalid="ignore"):
                got = np.where(np.isfinite(w) & (w > 0), 1.0 / (sig[None, :] ** 2 * w.astype(np.float64)), -1)
            got = np.rint(got).astype(np.int64)
            cnt = m["count"][sl]
            got = np.where((cnt == 0) & (w == 1), 0, got)     # no survivor: the weight is 1
            for g, c in zip(*np.nonzero(np.where(open_, (np.abs(got - cnt) > m["ingap"][sl]) | (got - cnt != flips), got != cnt))):
                out["count_bad"].append((int(groups[g]), int(c), int(got[g, c]), int(cnt[g, c])))
            exact = np.stack([f32_ht_weight(sig[c], got[:, c]) for c in range(case.C)], 1)
            for g, c in zip(*np.nonzero(exact.view(np.uint32) != np.ascontiguousarray(w, np.float32).view(np.uint32))):
                out["weight_bad"].append((int(groups[g]), int(c), float(w[g, c]), float(exact[g, c])))
    out["got"], out["want"] = filt, want
    out["err"] = np.abs(diff) / np.where(M_ > 0, M_, 1.0)[:, None, None, :, None]
    out["E_filt"] = float(out["err"].max()) if not np.isnan(out["err"]).any() else float("nan")
    wm = m["w"][sl]
    # A weight beyond 1e30 comes from a Wiener sum in float32's denormal range (a pilot of 1e-20): float32 has it inf or anywhere
    # up there, and no relative error is asked of it -- only that it is as large.
    huge = wm > 1e30
    out["huge_bad"] = [(int(groups[g]), int(c), float(w[g, c])) for g, c in zip(*np.nonzero(huge & ~(w > 1e30)))]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rel = np.where((wm == w) | huge, 0.0, np.abs(w.astype(np.float64) - wm) / np.abs(wm))
    out["rel_w"] = rel
    out["E_w"] = float(rel.max())
    return out


def where_wrong(case, res, bound, sl=None):
    """The worst filtered value beyond `bound` as (group, stack slot, SAI, channel, row, column, error) -- what a failing rewrite needs."""
    err = res["err"]
    bad = ~(err <= bound)      # (a NaN is beyond any bound)
    if not bad.any():
        return None
    g, n, st, c, pq = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err))), err.shape)
    g0 = (sl.start or 0) if sl is not None else 0
    return dict(case=case.name, beyond=int(bad.sum()), group=int(g) + g0, slot=int(n), sai=int(st), channel=int(c),
                row=int(pq) // case.k, col=int(pq) % case.k, err=float(err[g, n, st, c, pq]), bound=float(bound),
                got=float(res["got"][g, n, st, c, pq]), want=float(res["want"][g, n, st, c, pq]))
