"""Numpy model of the clipped Poisson-Gaussian routines (lfbm5d_pgclip_*, include/lfbm5d_pgclip.h): the censored line fit on the
statistics of clip_model (float64), the curves of a model (clipped moments, stabiliser, exact unbiased inverse; float64, tables in
float32) and the table look-up in float32, which the GPU must equal bit for bit."""
import numpy as np
from scipy.special import erfc

import clip_model as CM

KNOTS = 4097
QUAD_N, QUAD_R = 3201, 8.0
MAX_RATIO, MAX_A = 0.5, 5.0          # the accepted domain: a^2 <= MAX_RATIO * b and a <= MAX_A
V_MIN = 1.0 / 12.0


def _Phi(x):
    return 0.5 * erfc(-x / np.sqrt(2.0))


def _phi(x):
    return np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


# ---- the fit ----

def fit_one(hist, sum_m, cens, whole, lo=0.0, hi=255.0):
    """One histogram [L][Q] with sum_m [L], cens [L] and `whole` -> dict(a, b, levels, f_max), or None when fewer than 4 levels are
    populated: clip_model's level variances, the ladder over the censored fraction, then pg_model.fit's constrained weighted line."""
    s = float(CM.rescale(lo, hi))
    delta = 0.5 * s if 0 < int(hist.sum()) == int(whole) else 0.0
    lv = CM.level_variances(hist, delta)
    for f_max in CM.LADDER:
        Sw = Swx = Swv = Swxx = Swxv = 0.0
        used = 0
        for l, (n, v) in enumerate(lv):
            if v is None or float(cens[l]) > f_max * n:
                continue
            x = float(sum_m[l]) / (256.0 * n)
            w = n / (v * v)
            Sw += w; Swx += w * x; Swv += w * v; Swxx += w * x * x; Swxv += w * x * v
            used += 1
        if used < CM.MIN_LEVELS:
            continue
        det = Sw * Swxx - Swx * Swx
        if not det > 1e-12 * Sw * Swxx:
            a, b = 0.0, Swv / Sw
        else:
            a = (Sw * Swxv - Swx * Swv) / det
            b = (Swxx * Swv - Swx * Swxv) / det
            if a < 0.0:
                a, b = 0.0, Swv / Sw
            elif b < 0.0:
                a, b = Swxv / Swxx, 0.0
        return dict(a=a / s, b=b / (s * s), levels=used, f_max=f_max)
    return None


def fit(hist, sum_m, cens, whole, lo=0.0, hi=255.0):
    """hist [C][L][Q], sum_m, cens [C][L], whole [C] -> dict(a, b, a_channel, b_channel, levels, f_max, censored, heavily_clipped,
    quantised) of the pooled channels (NaN for a channel whose own fit fails), or None when the pooled fit fails."""
    hist, sum_m = np.asarray(hist, np.uint64), np.asarray(sum_m, np.uint64)
    cens, whole = np.asarray(cens, np.uint64), np.asarray(whole, np.uint64)
    pooled = fit_one(hist.sum(axis=0), sum_m.sum(axis=0), cens.sum(axis=0), whole.sum(), lo, hi)
    if pooled is None:
        return None
    ch = [fit_one(hist[c], sum_m[c], cens[c], whole[c], lo, hi) for c in range(hist.shape[0])]
    total = int(hist.sum())
    pooled.update(a_channel=[f["a"] if f else np.nan for f in ch], b_channel=[f["b"] if f else np.nan for f in ch],
                  censored=float(int(cens.sum())) / total, heavily_clipped=pooled["f_max"] > 0.1, quantised=int(whole.sum()) == total)
    return pooled


def estimate(lf, mask, W, H, C, lo=0.0, hi=255.0):
    """fit() of clip_model.histogram(), with the statistics added to the dict; None when the fit fails."""
    hist, sm, cens, whole, blocks, skipped = CM.histogram(lf, mask, W, H, C, lo, hi)
    r = fit(hist, sm, cens, whole, lo, hi)
    if r is not None:
        r.update(hist=hist, sum_m=sm, cens=cens, whole=whole, blocks=blocks, skipped=skipped)
    return r


# ---- the curves ----

def valid(a, b, lo, hi, domain=True):
    ok = all(np.isfinite(v) for v in (a, b, lo, hi)) and a >= 0.0 and b >= 0.0 and a + b > 0.0 and lo < hi and np.isfinite(hi - lo)
    return bool(ok and (not domain or (a * a <= MAX_RATIO * b and a <= MAX_A)))


def sigma_of(y, a, b, lo):
    return np.sqrt(np.maximum(a * (np.asarray(y, np.float64) - lo) + b, V_MIN))


def clipped_moments(y, a, b, lo, hi):
    """(clipped mean, clipped deviation) of z = clip(y + sigma(y) n, lo, hi) at the true values y (float64)."""
    y = np.asarray(y, np.float64)
    sg = sigma_of(y, a, b, lo)
    al, be = (lo - y) / sg, (hi - y) / sg
    ta, tb = _Phi(al), _Phi(-be)
    pa, pb = _phi(al), _phi(be)
    mid = 1.0 - ta - tb
    mean = lo * ta + hi * tb + y * mid + sg * (pa - pb)
    var = (lo - y) ** 2 * ta + (hi - y) ** 2 * tb + sg * sg * (mid + al * pa - be * pb) - (mean - y) ** 2
    return mean, np.sqrt(var)


def _pl(x, xk, fk, s0, s1):
    """Piecewise linear through (xk, fk), extended with slopes s0 below xk[0] and s1 above xk[-1]."""
    x = np.asarray(x, np.float64)
    out = np.interp(x, xk, fk)
    out = np.where(x < xk[0], fk[0] + (x - xk[0]) * s0, out)
    return np.where(x > xk[-1], fk[-1] + (x - xk[-1]) * s1, out)


def curves(a, b, lo=0.0, hi=255.0, domain=True):
    """The curves of a model, or None when it is refused (invalid, outside the accepted domain when `domain`, or G not strictly
    increasing).  dict: s; fwd, inv float32 [4097] with fwd_x0, fwd_dx, inv_x0, inv_dx (float64); and, for the tests, the grid y, the
    clipped moments mean / dev on it, F (float64, at `mean`), G (float64, at y) and the callable F_of(z)."""
    a, b, lo, hi = float(a), float(b), float(lo), float(hi)
    if not valid(a, b, lo, hi, domain):
        return None
    n = KNOTS - 1
    y = lo + np.arange(KNOTS, dtype=np.float64) * ((hi - lo) / n)
    mean, dev = clipped_moments(y, a, b, lo, hi)
    if not (np.isfinite(mean).all() and np.isfinite(dev).all() and (dev > 0).all() and (np.diff(mean) > 0).all()):
        return None
    inv_dev = 1.0 / dev
    F0 = np.concatenate(([0.0], np.cumsum(0.5 * (inv_dev[:-1] + inv_dev[1:]) * np.diff(mean))))
    s = 255.0 / F0[-1]
    if not (np.isfinite(s) and s > 0):
        return None
    F = s * F0
    s0, s1 = s * inv_dev[0], s * inv_dev[-1]

    def F_of(z):
        return _pl(z, mean, F, s0, s1)

    fwd = F_of(y)
    nq = -QUAD_R + np.arange(QUAD_N, dtype=np.float64) * (2.0 * QUAD_R / (QUAD_N - 1))
    w = _phi(nq)
    w[0] *= 0.5; w[-1] *= 0.5
    w /= w.sum()
    sg = sigma_of(y, a, b, lo)
    G = np.empty(KNOTS)
    for i0 in range(0, KNOTS, 256):
        sl = slice(i0, min(KNOTS, i0 + 256))
        z = np.clip(y[sl, None] + sg[sl, None] * nq[None, :], lo, hi)
        G[sl] = F_of(z) @ w
    if not (np.diff(G) > 0).all():
        return None
    u = G[0] + np.arange(KNOTS, dtype=np.float64) * ((G[-1] - G[0]) / n)
    inv = np.interp(u, G, y)
    inv[0], inv[-1] = lo, hi
    return dict(a=a, b=b, lo=lo, hi=hi, s=s, fwd=fwd.astype(np.float32), inv=inv.astype(np.float32), fwd_x0=lo, fwd_dx=(hi - lo) / n,
                inv_x0=G[0], inv_dx=(G[-1] - G[0]) / n, y=y, mean=mean, dev=dev, F=F, G=G, F_of=F_of, fwd64=fwd, inv64=inv)


# ---- the look-up (float32, operation by operation as k_curve_map) ----

def curve_map(x, table, x0, dx, inverse):
    """out = T[i] + r (T[i + 1] - T[i]), t = (x - x0) inv_dx, i = clamp(floor t, 0, 4095), r = t - i (clamped to 0..1 in the inverse
    direction); non-finite values pass through.  Every operation is rounded to float32 on its own."""
    x = np.asarray(x, np.float32)
    T = np.asarray(table, np.float32)
    f32 = np.float32
    x0f, idx = f32(x0), f32(1.0 / dx)
    fin = np.isfinite(x)
    xs = np.where(fin, x, f32(0))
    t = (xs - x0f) * idx
    i = np.minimum(np.maximum(np.floor(t), f32(0)), f32(KNOTS - 2)).astype(np.int32)
    r = t - i.astype(np.float32)
    if inverse:
        r = np.minimum(np.maximum(r, f32(0)), f32(1))
    out = T[i] + r * (T[i + 1] - T[i])
    return np.where(fin, out.astype(np.float32), x)


def forward(x, cv):
    return curve_map(x, cv["fwd"], cv["fwd_x0"], cv["fwd_dx"], False)


def inverse(x, cv):
    return curve_map(x, cv["inv"], cv["inv_x0"], cv["inv_dx"], True)
