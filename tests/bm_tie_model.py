"""Exact model of both block-matching searches for integer-valued planes: brute-force sums of squared differences in int64,
written from the definitions in the docstrings of tests/test_oracle_pins.py (zero band, mirrored test of the backward half,
2 * threshold outside the band, scan order dj outer / di = 0..nSim then -nSim..-1, power-of-two floor, duplicate rule) -- not from
the oracle's code.

Why it can be exact: on integer pixel values every operation of the float32 integral-image recurrence the oracle and the kernels
evaluate is an exact integer operation while its largest intermediate, sum[kk-1] + sum[kk-W] <= 2 k^2 R^2 (plus at most 2 R^2 from
the four corner terms), stays below 2^24; R is the largest absolute difference of two pixel values.  exact_domain() asserts
4 k^2 R^2 < 2^24.  Inside that domain the model, the oracle and the GPU can be compared without excluded positions or tolerances,
exact ties included: a tie is then a property of the data, not of the arithmetic.
"""
import numpy as np

BIG = np.iinfo(np.int64).max


def exact_domain(plane, k):
    """Assert that block matching with k x k patches on `plane` is exact in float32; returns R."""
    p = np.asarray(plane)
    assert np.isfinite(p).all() and np.array_equal(p, np.rint(p)), "plane is not integer-valued"
    R = int(p.max() - p.min())
    assert 4 * k * k * R * R < 2 ** 24, (k, R)
    return R


def _box(D, k):
    """S[i][j] = sum of D[i:i+k, j:j+k], zeros continuing past the array (int64, same shape as D)."""
    H, W = D.shape
    c = np.zeros((H + k + 1, W + k + 1), np.int64)
    c[1:H + 1, 1:W + 1] = D.cumsum(0).cumsum(1)
    c[H + 1:, :] = c[H:H + 1, :]
    c[:, W + 1:] = c[:, W:W + 1]
    return c[k:k + H, k:k + W] - c[:H, k:k + W] - c[k:k + H, :W] + c[:H, :W]


def threshold(tau, k):
    thr = tau * k * k
    assert thr == int(thr)
    return int(thr)


def ref_grid(dim, k, nHW, p):
    """Reference rows / columns of a padded dimension: nHW, nHW + p, ... below dim - k + 1 - nHW, and that last one forced."""
    last = dim - k + 1 - nHW - 1
    g = list(range(nHW, last + 1, p))
    if g[-1] < last:
        g.append(last)
    return np.array(g, np.int64)


def self_search(plane, k, N, nSim, nDisp, tau, refs):
    """The self-similarity search on one integer plane [H][W] for the flat reference indices `refs`.
    Returns dict(idx [R][max(N,1)], cnt [R], n_pass [R], tie_cut [R], tie_any [R], thr_equal [R]):
      n_pass    candidates that pass the threshold test;
      tie_cut   the nSx-th and (nSx+1)-th best passing scores are equal (the selected SET depends on the tie order);
      tie_any   two of the nSx + 1 best passing scores are equal (set or ORDER depends on it);
      thr_equal a tested value equals the threshold exactly."""
    a = np.asarray(plane).astype(np.int64)
    H, W = a.shape
    refs = np.asarray(refs).astype(np.int64)
    R = len(refs)
    if N <= 1:
        z = np.zeros(R, bool)
        return dict(idx=refs.astype(np.uint32).reshape(R, 1), cnt=np.ones(R, np.uint32), n_pass=np.ones(R, np.int64),
                    tie_cut=z, tie_any=z.copy(), thr_equal=z.copy())
    nHW = nSim + nDisp
    thr = threshold(tau, k)
    band = np.zeros((H, W), bool)
    band[nHW:H - nHW, nHW:W - nHW] = True
    ys, xs = slice(nHW, H - nHW), slice(nHW, W - nHW)
    T = {}
    for di in range(0, nSim + 1):
        for dj in range(-nSim, nSim + 1):
            D = np.zeros((H, W), np.int64)
            D[ys, xs] = (a[nHW + di:H - nHW + di, nHW + dj:W - nHW + dj] - a[ys, xs]) ** 2
            t = np.full((H, W), 2 * thr, np.int64)
            t[band] = _box(D, k)[band]
            T[(di, dj)] = t.reshape(-1)
    tests, scores, posn = [], [], []
    for dj in range(-nSim, nSim + 1):
        for di in range(0, nSim + 1):
            v = T[(di, dj)][refs]
            tests.append(v); scores.append(v); posn.append(refs + di * W + dj)
        for di in range(-nSim, 0):
            t = T[(-di, -dj)]
            c = refs + di * W + dj
            tests.append(t[refs]); scores.append(t[c]); posn.append(c)
    tests, scores, posn = np.stack(tests, 1), np.stack(scores, 1), np.stack(posn, 1)      # [R][candidates in scan order]
    ok = tests < thr
    n_pass = ok.sum(1)
    o = np.argsort(np.where(ok, scores, BIG), axis=1, kind="stable")                     # (score, scan order)
    s_sorted = np.take_along_axis(np.where(ok, scores, BIG), o, 1)
    p_sorted = np.take_along_axis(posn, o, 1)
    idx = np.zeros((R, N), np.uint32)
    cnt = np.zeros(R, np.uint32)
    tie_cut, tie_any = np.zeros(R, bool), np.zeros(R, bool)
    for r in range(R):
        n = int(n_pass[r])
        nSx = N if n >= N else (1 << (n.bit_length() - 1) if n else 1)
        if n == 0:
            idx[r, :2] = refs[r]; cnt[r] = 2
            continue
        idx[r, :nSx] = p_sorted[r, :nSx]
        cnt[r] = nSx
        if nSx == 1:
            idx[r, 1] = idx[r, 0]; cnt[r] = 2                                             # a single survivor is stored twice
        head = s_sorted[r, :min(nSx + 1, n)]
        tie_cut[r] = nSx < n and head[nSx] == head[nSx - 1]
        tie_any[r] = bool((head[1:] == head[:-1]).any())
    return dict(idx=idx, cnt=cnt, n_pass=n_pass, tie_cut=tie_cut, tie_any=tie_any, thr_equal=(tests == thr).any(1))


def self_search_stream(plane, k, N, nSim, nDisp, tau, refs):
    """self_search with one displacement table alive at a time (memory O(plane); self_search keeps (nSim + 1)(2 nSim + 1) planes,
    4753 at nSim = 48).  From table (di, dj) it gathers the forward value at `refs` -- candidate (di, dj) -- and, for di > 0, the
    backward candidate (-di, -dj): tested with the table's value at `refs`, scored with its value at refs - (di, dj).
    Returns (the dict of self_search, rows): rows [R][(2 nSim + 1)^2] int64 are the score rows as a filled table holds them,
    candidate (dip, djp) at (djp + nSim)(2 nSim + 1) + (dip if dip >= 0 else dip + 2 nSim + 1) -- scan order -- with 2 * threshold
    where the scored position lies outside the band (what the table kernels never write)."""
    a = np.asarray(plane).astype(np.int64)
    H, W = a.shape
    refs = np.asarray(refs).astype(np.int64)
    R = len(refs)
    assert N > 1
    nHW, Ns = nSim + nDisp, 2 * nSim + 1
    thr = threshold(tau, k)
    band = np.zeros((H, W), bool)
    band[nHW:H - nHW, nHW:W - nHW] = True
    ys, xs = slice(nHW, H - nHW), slice(nHW, W - nHW)
    tests, scores, posn = (np.zeros((R, Ns * Ns), np.int64) for _ in range(3))
    for di in range(0, nSim + 1):
        for dj in range(-nSim, nSim + 1):
            D = np.zeros((H, W), np.int64)
            D[ys, xs] = (a[nHW + di:H - nHW + di, nHW + dj:W - nHW + dj] - a[ys, xs]) ** 2
            t = np.full((H, W), 2 * thr, np.int64)
            t[band] = _box(D, k)[band]
            t = t.reshape(-1)
            e = (dj + nSim) * Ns + di
            tests[:, e] = scores[:, e] = t[refs]
            posn[:, e] = refs + di * W + dj
            if di > 0:
                e, c = (-dj + nSim) * Ns + (Ns - di), refs - di * W - dj
                tests[:, e], scores[:, e], posn[:, e] = t[refs], t[c], c
    ok = tests < thr
    n_pass = ok.sum(1)
    keyed = np.where(ok, scores, BIG)
    o = np.argsort(keyed, axis=1, kind="stable")[:, :N + 1]                               # (score, scan order)
    s_sorted, p_sorted = np.take_along_axis(keyed, o, 1), np.take_along_axis(posn, o, 1)
    idx = np.zeros((R, N), np.uint32)
    cnt = np.zeros(R, np.uint32)
    tie_cut, tie_any = np.zeros(R, bool), np.zeros(R, bool)
    for r in range(R):
        n = int(n_pass[r])
        if n == 0:
            idx[r, :2] = refs[r]; cnt[r] = 2
            continue
        nSx = N if n >= N else 1 << (n.bit_length() - 1)
        idx[r, :nSx] = p_sorted[r, :nSx]
        cnt[r] = nSx
        if nSx == 1:
            idx[r, 1] = idx[r, 0]; cnt[r] = 2
        head = s_sorted[r, :min(nSx + 1, n)]
        tie_cut[r] = nSx < n and head[nSx] == head[nSx - 1]
        tie_any[r] = bool((head[1:] == head[:-1]).any())
    return dict(idx=idx, cnt=cnt, n_pass=n_pass, tie_cut=tie_cut, tie_any=tie_any, thr_equal=(tests == thr).any(1)), scores


def region(H, W, k, nDisp):
    """Rows / columns at which the disparity search is defined (and compared)."""
    return slice(nDisp, H - nDisp - k + 1), slice(nDisp, W - nDisp - k + 1)


def disparity_search(plane1, plane2, k, nDisp, tau):
    """The disparity search plane1 -> plane2 on integer planes [H][W].  Returns dict(best, shape, tie_min, thr_equal), each of
    the shape of region(H, W, k, nDisp): best = flat index in plane2, shape = minimum < threshold, tie_min = the minimum is
    attained more than once, thr_equal = the minimum equals the threshold exactly."""
    a, b = np.asarray(plane1).astype(np.int64), np.asarray(plane2).astype(np.int64)
    H, W = a.shape
    thr = threshold(tau, k)
    rows, cols = region(H, W, k, nDisp)
    ys, xs = slice(nDisp, H - nDisp), slice(nDisp, W - nDisp)
    S, off = [], []
    for dj in range(-nDisp, nDisp + 1):
        for di in range(-nDisp, nDisp + 1):
            D = np.zeros((H, W), np.int64)
            D[ys, xs] = (b[nDisp + di:H - nDisp + di, nDisp + dj:W - nDisp + dj] - a[ys, xs]) ** 2
            S.append(_box(D, k)[rows, cols]); off.append(di * W + dj)
    S = np.stack(S)                                                                       # scan order along axis 0
    first = S.argmin(0)                                                                   # numpy: first occurrence
    m = S.min(0)
    pos = np.arange(H * W, dtype=np.int64).reshape(H, W)[rows, cols]
    return dict(best=(pos + np.array(off, np.int64)[first]).astype(np.uint32), shape=(m < thr).astype(np.uint8),
                tie_min=(S == m).sum(0) > 1, thr_equal=m == thr)
