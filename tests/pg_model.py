"""Numpy model of the Poisson-Gaussian noise routines (lfbm5d_pg_*, include/lfbm5d.h): the block statistics in float32 with integer
counts (what the GPU must equal exactly), the fit and the transforms in float64."""
import numpy as np

L, E_MIN, E_MAX = 64, -12, 8
Q = (E_MAX - E_MIN) * 16 + 2
KEY_BASE = (E_MIN + 127) << 4
QUARTILE = 0.31863936396437514
G_MAX = 0.816496580927726
K1, K3 = 0.30618621784789724, 0.7654655446197431


def edges():
    """e[k], k = 0..Q-1: the lower edge of key k as float64 (key 0 starts at 0)."""
    e = np.zeros(Q, np.float64)
    e[1:] = ((np.arange(1, Q, dtype=np.uint32) - 1 + KEY_BASE) << np.uint32(19)).view(np.float32).astype(np.float64)
    return e


def histogram(lf, mask, W, H, C):
    """lf [asize][C*H*W] float32 -> (hist uint64 [C][L][Q], sum_m uint64 [C][L], blocks, skipped)."""
    lf = np.ascontiguousarray(lf, np.float32).reshape(len(mask), C, H, W)
    hist, sm = np.zeros((C, L, Q), np.uint64), np.zeros((C, L), np.uint64)
    blocks = skipped = 0
    HP, WP = H // 2, W // 2
    with np.errstate(invalid="ignore", over="ignore"):
        for st in range(len(mask)):
            if not mask[st]:
                continue
            for c in range(C):
                I = lf[st, c]
                p00, p01 = I[0:2 * HP:2, 0:2 * WP:2], I[0:2 * HP:2, 1:2 * WP:2]
                p10, p11 = I[1:2 * HP:2, 0:2 * WP:2], I[1:2 * HP:2, 1:2 * WP:2]
                m = ((p00 + p01) + (p10 + p11)) * np.float32(0.25)
                d = ((p00 - p01) - (p10 - p11)) * np.float32(0.5)
                ok = np.isfinite(m) & np.isfinite(d)
                blocks += m.size
                skipped += int((~ok).sum())
                m, d = m[ok], d[ok]
                mc = np.minimum(np.maximum(m, np.float32(0)), np.float32(255))
                lev = np.minimum(L - 1, (mc * np.float32(64.0 / 255.0)).astype(np.int32))
                key = np.clip((np.abs(d).view(np.uint32) >> np.uint32(19)).astype(np.int64) - KEY_BASE + 1, 0, Q - 1)
                hist[c] += np.bincount(lev * Q + key, minlength=L * Q).astype(np.uint64).reshape(L, Q)
                w = np.rint(mc * np.float32(256.0)).astype(np.int64)
                sm[c] += np.bincount(lev, weights=w.astype(np.float64), minlength=L).astype(np.uint64)   # exact: sums < 2^53
    return hist, sm, blocks, skipped


def fit(hist, sum_m):
    """(a, b) of one histogram [L][Q] with sum_m [L], or None when no level is valid."""
    e = edges()
    Sw = Swx = Swv = Swxx = Swxv = 0.0
    valid = 0
    for l in range(L):
        h = hist[l].astype(np.int64)
        n = int(h.sum())
        if n < 256:
            continue
        T = 0.25 * n
        cum = np.cumsum(h)
        ks = int(np.argmax(cum >= T))
        if ks == 0 or ks == Q - 1:
            continue
        Qv = e[ks] + (e[ks + 1] - e[ks]) * (T - float(cum[ks - 1])) / float(h[ks])
        r = Qv / QUARTILE
        v = r * r
        x = float(sum_m[l]) / (256.0 * n)
        w = n / (v * v)
        Sw += w; Swx += w * x; Swv += w * v; Swxx += w * x * x; Swxv += w * x * v
        valid += 1
    if not valid:
        return None
    det = Sw * Swxx - Swx * Swx
    if valid < 2 or not det > 1e-12 * Sw * Swxx:
        return 0.0, Swv / Sw
    a = (Sw * Swxv - Swx * Swv) / det
    b = (Swxx * Swv - Swx * Swxv) / det
    if a < 0.0:
        return 0.0, Swv / Sw
    if b < 0.0:
        return Swxv / Swxx, 0.0
    return a, b


def estimate(lf, mask, W, H, C):
    """dict(a, b, a_channel, b_channel, hist, sum_m, blocks, skipped): the pooled fit and every channel's."""
    hist, sm, blocks, skipped = histogram(lf, mask, W, H, C)
    pooled = fit(hist.sum(axis=0), sm.sum(axis=0))
    ch = [fit(hist[c], sm[c]) for c in range(C)]
    return dict(a=pooled[0], b=pooled[1], a_channel=[f[0] if f else np.nan for f in ch], b_channel=[f[1] if f else np.nan for f in ch],
                hist=hist, sum_m=sm, blocks=blocks, skipped=skipped)


def scale(a, b):
    """s of per-channel sequences a, b (float64), or None for a rejected model."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    c = 0.375 * a * a + b
    if not (np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (c > 0).all()):
        return None
    return float(np.mean((np.sqrt(255.0 * a + c) + np.sqrt(c)) / 2.0))


def forward(z, a, b, s):
    """float64 forward transform of one channel's values z under scalars a, b and the common scale s."""
    z = np.asarray(z, np.float64).copy()
    c = 0.375 * a * a + b
    w = a * z + c
    neg = w < 0.0
    if neg.any():
        w[neg] = 0.0
        z[neg] = -c / a
    return (s * (2.0 * z)) / (np.sqrt(w) + np.sqrt(c))


def inverse(t, a, b, s):
    """float64 exact unbiased inverse (closed form) of one channel's values t."""
    t = np.asarray(t, np.float64)
    sc = np.sqrt(0.375 * a * a + b)
    u = t / s
    q = a * u + 2.0 * sc
    with np.errstate(divide="ignore", invalid="ignore"):
        g = a / q
        y = a * u * u / 4.0 + u * sc + a / 4.0 + a * (K1 * g - 1.375 * (g * g) + K3 * (g * g * g))
    y = np.where((q > 0.0) & ~(g > G_MAX), y, 0.0)
    return np.maximum(y, 0.0)


def forward_lf(lf, a, b, C):
    """[asize][C*plane] float32 -> float32 through forward() per channel (a, b: per-channel sequences); returns (out, s)."""
    s = scale(a, b)
    x = np.asarray(lf, np.float32).reshape(lf.shape[0], C, -1)
    out = np.stack([forward(x[:, c], a[c], b[c], s) for c in range(C)], axis=1)
    return out.reshape(lf.shape), s


def inverse_lf(lf, a, b, C):
    s = scale(a, b)
    x = np.asarray(lf, np.float32).reshape(lf.shape[0], C, -1)
    out = np.stack([inverse(x[:, c], a[c], b[c], s) for c in range(C)], axis=1)
    return out.reshape(lf.shape)
