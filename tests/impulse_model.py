"""Numpy model of the impulse-noise repair (lfbm5d_impulse_*, include/lfbm5d.h): the checker of the tests, written from the definition.
R in float32 (subtractions, absolute values, selections and three additions in a fixed order), integer histograms, the quantile in
float64; the repair moves existing pixel values only.  The GPU must equal every output of this file bit for bit."""
import numpy as np

E_MIN, E_MAX = -12, 12
Q = (E_MAX - E_MIN) * 16 + 2            # 386
KEY_BASE = (E_MIN + 127) << 4           # bits >> 19 of 2^E_MIN
OFFS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def edges():
    """e[k], k = 0..Q-1: the lower edge of key k as float64 (key 0 starts at 0)."""
    e = np.zeros(Q, np.float64)
    e[1:] = ((np.arange(1, Q, dtype=np.uint32) - 1 + KEY_BASE) << np.uint32(19)).view(np.float32).astype(np.float64)
    return e


def neighbours(I):
    """[8][H][W]: the eight neighbours of every pixel of the plane I, mirrored without repeating the edge (-1 -> 1, W -> W - 2)."""
    H, W = I.shape
    P = np.pad(I, 1, mode="reflect")
    return np.stack([P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in OFFS])


def road(I):
    """(R float32, extreme bool) of every pixel of a float32 plane."""
    I = np.ascontiguousarray(I, np.float32)
    q = neighbours(I)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(I[None] - q)
        d = np.where(np.isfinite(q) & np.isfinite(I)[None], d, np.float32(np.inf)).astype(np.float32)
        d.sort(axis=0)
        R = ((d[0] + d[1]) + d[2]) + d[3]
        fin = np.isfinite(q)
        lt = (fin & (q < I[None])).sum(axis=0)
        gt = (fin & (q > I[None])).sum(axis=0)
    return R.astype(np.float32), np.minimum(lt, gt) == 0


def keys(R):
    """Histogram key of finite R >= 0."""
    return np.clip((R.view(np.uint32) >> np.uint32(19)).astype(np.int64) - KEY_BASE + 1, 0, Q - 1)


def histogram(lf, mask, W, H, C):
    """lf [asize][C*H*W] float32 -> (hist uint64 [C][Q], pixels, skipped)."""
    lf = np.ascontiguousarray(lf, np.float32).reshape(len(mask), C, H, W)
    hist = np.zeros((C, Q), np.uint64)
    pixels = skipped = 0
    for st in range(len(mask)):
        if not mask[st]:
            continue
        for c in range(C):
            R, _ = road(lf[st, c])
            ok = np.isfinite(R)
            pixels += R.size
            skipped += int((~ok).sum())
            hist[c] += np.bincount(keys(R[ok]), minlength=Q).astype(np.uint64)
    return hist, pixels, skipped


def scale(hist):
    """The 0.5 quantile of one histogram [Q], interpolated linearly inside its bin; None for an empty histogram.  A quantile in the
    last key (everything >= 2^12, no upper edge) is that key's lower edge."""
    h = np.asarray(hist).astype(np.int64)
    n = int(h.sum())
    if n == 0:
        return None
    e = edges()
    T = 0.5 * n
    cum = np.cumsum(h)
    ks = int(np.argmax(cum >= T))
    if ks == Q - 1:
        return float(e[ks])
    before = float(cum[ks - 1]) if ks else 0.0
    return float(e[ks] + (e[ks + 1] - e[ks]) * (T - before) / float(h[ks]))


def thresholds(hist, C, k=8.0, min_threshold=0.0, threshold=None):
    """(T float32 [C], scale pooled, scale per channel): T_c = (float32) max(k scale_c, min_threshold), or the given threshold[c] > 0.
    An empty histogram counts as scale 0."""
    sc = [scale(hist[c]) or 0.0 for c in range(C)]
    pooled = scale(np.asarray(hist).sum(axis=0)) or 0.0
    T = np.array([max(float(k) * sc[c], float(min_threshold)) for c in range(C)], np.float64)
    if threshold is not None:
        for c in range(C):
            if threshold[c] > 0:
                T[c] = threshold[c]
    return T.astype(np.float32), pooled, sc


def _order_key(v):
    """int32 keys that order float32 values ascending with -0 before +0 (the order of the repair's sort)."""
    i = np.ascontiguousarray(v, np.float32).view(np.int32)
    return i ^ ((i >> 31) & np.int32(0x7fffffff))


def repair_plane(I, flagged):
    """(out float32, code uint8) of one plane under the boolean flags: the lower median of the unflagged finite neighbours."""
    I = np.ascontiguousarray(I, np.float32)
    q = neighbours(I)
    ok = ~neighbours(flagged) & np.isfinite(q)
    n = ok.sum(axis=0)
    big = np.int64(1) << 40
    key = np.where(ok, _order_key(q).astype(np.int64), big)
    order = np.argsort(key, axis=0, kind="stable")
    pick = np.take_along_axis(order, (np.maximum(n, 1) - 1)[None] // 2, axis=0)[0]
    med = np.take_along_axis(q, pick[None], axis=0)[0]
    code = np.where(flagged, np.where(n > 0, 1, 2), 0).astype(np.uint8)
    out = np.where(code == 1, med.view(np.uint32), I.view(np.uint32))        # on the bits: NaN payloads of kept pixels survive
    return out.view(np.float32), code


def detect_plane(I, T):
    R, extreme = road(I)
    return ~np.isfinite(I) | ((R > np.float32(T)) & extreme)


def _counts(code):
    return [int((code != 0).sum()), int((code == 1).sum()), int((code == 2).sum())]


def repair(lf, mask, W, H, C, k=8.0, min_threshold=0.0, threshold=None, flags=None, out=None, codes=None):
    """The whole routine.  lf [asize][C*H*W] float32; flags (given flags, non-zero = defective, [asize][C*H*W]) skips the detection.
    out / codes: initial contents of the outputs (planes of empty SAIs keep them).  Returns a dict: out float32, flags uint8 (codes),
    hist, scale, scale_channel, threshold (float32 [C]), counts_sai int64 [asize][C][3] (flagged, repaired, left), flagged / repaired /
    left per channel, pixels, skipped."""
    A = len(mask)
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    res_out = np.array(x if out is None else np.asarray(out, np.float32).reshape(A, C, H, W), np.float32, copy=True)
    res_code = np.zeros((A, C, H, W), np.uint8) if codes is None else np.array(np.asarray(codes, np.uint8).reshape(A, C, H, W), copy=True)
    r = dict(hist=None, scale=0.0, scale_channel=[0.0] * C, threshold=np.zeros(C, np.float32),
             pixels=int(np.count_nonzero(mask)) * C * H * W, skipped=0)
    if flags is None:
        need_stats = threshold is None or any(not threshold[c] > 0 for c in range(C))
        if need_stats:
            r["hist"], r["pixels"], r["skipped"] = histogram(x, mask, W, H, C)
            r["threshold"], r["scale"], r["scale_channel"] = thresholds(r["hist"], C, k, min_threshold, threshold)
        else:
            r["threshold"] = np.array([threshold[c] for c in range(C)], np.float64).astype(np.float32)
    else:
        given = np.asarray(flags).reshape(A, C, H, W) != 0
    cs = np.zeros((A, C, 3), np.int64)
    for st in range(A):
        if not mask[st]:
            continue
        for c in range(C):
            f = given[st, c] if flags is not None else detect_plane(x[st, c], r["threshold"][c])
            res_out[st, c], res_code[st, c] = repair_plane(x[st, c], f)
            cs[st, c] = _counts(res_code[st, c])
    r.update(out=res_out.reshape(A, -1), flags=res_code.reshape(A, -1), counts_sai=cs, flagged=cs[:, :, 0].sum(axis=0),
             repaired=cs[:, :, 1].sum(axis=0), left=cs[:, :, 2].sum(axis=0))
    return r
