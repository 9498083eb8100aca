"""Numpy model of the clipping-aware routines (lfbm5d_clip_*, lfbm5d_declip_*, include/lfbm5d.h): the block statistics in float32 with
integer counts (what the GPU must equal exactly), the fit with its ladder and the clipped-mean map with its inverse in float64."""
import numpy as np
from scipy.special import erfc

import pg_model as PG

L, Q = PG.L, PG.Q
MIN_BLOCKS, MIN_LEVELS = 256, 4
LADDER = (0.05, 0.1, 0.2, 0.4, 1.0)


def rescale(lo, hi):
    """s = (float)(255 / (hi - lo)): the factor that takes the range onto the 0..255 of the levels and keys."""
    return np.float32(255.0 / (float(hi) - float(lo)))


def histogram(lf, mask, W, H, C, lo=0.0, hi=255.0):
    """lf [asize][C*H*W] float32 -> (hist uint64 [C][L][Q], sum_m uint64 [C][L], cens uint64 [C][L], whole uint64 [C], blocks, skipped):
    PG.histogram of p' = (p - lo) * s, per level the blocks that hold a censored pixel (p <= lo or p >= hi), per channel the blocks whose
    four pixels are whole numbers."""
    lf = np.ascontiguousarray(lf, np.float32).reshape(len(mask), C, H, W)
    lo32, hi32, s = np.float32(lo), np.float32(hi), rescale(lo, hi)
    hist, sm, cens = np.zeros((C, L, Q), np.uint64), np.zeros((C, L), np.uint64), np.zeros((C, L), np.uint64)
    whole = np.zeros(C, np.uint64)
    blocks = skipped = 0
    HP, WP = H // 2, W // 2
    with np.errstate(invalid="ignore", over="ignore"):
        for st in range(len(mask)):
            if not mask[st]:
                continue
            for c in range(C):
                I = lf[st, c]
                raw = [I[0:2 * HP:2, 0:2 * WP:2], I[0:2 * HP:2, 1:2 * WP:2], I[1:2 * HP:2, 0:2 * WP:2], I[1:2 * HP:2, 1:2 * WP:2]]
                p00, p01, p10, p11 = ((p - lo32) * s for p in raw)
                cz = (raw[0] <= lo32) | (raw[0] >= hi32)
                wh = raw[0] == np.rint(raw[0])
                for p in raw[1:]:
                    cz |= (p <= lo32) | (p >= hi32)
                    wh &= p == np.rint(p)
                m = ((p00 + p01) + (p10 + p11)) * np.float32(0.25)
                d = ((p00 - p01) - (p10 - p11)) * np.float32(0.5)
                ok = np.isfinite(m) & np.isfinite(d)
                blocks += m.size
                skipped += int((~ok).sum())
                m, d, cz = m[ok], d[ok], cz[ok]
                whole[c] += np.uint64(int(wh[ok].sum()))
                mc = np.minimum(np.maximum(m, np.float32(0)), np.float32(255))
                lev = np.minimum(L - 1, (mc * np.float32(64.0 / 255.0)).astype(np.int32))
                key = np.clip((np.abs(d).view(np.uint32) >> np.uint32(19)).astype(np.int64) - PG.KEY_BASE + 1, 0, Q - 1)
                hist[c] += np.bincount(lev * Q + key, minlength=L * Q).astype(np.uint64).reshape(L, Q)
                w = np.rint(mc * np.float32(256.0)).astype(np.int64)
                sm[c] += np.bincount(lev, weights=w.astype(np.float64), minlength=L).astype(np.uint64)   # exact: sums < 2^53
                cens[c] += np.bincount(lev[cz], minlength=L).astype(np.uint64)
    return hist, sm, cens, whole, blocks, skipped


def lattice_edges(delta):
    """The key edges as the fit reads them.  delta = 0: pg_model.edges().  delta > 0: every d is a multiple of delta (whole-numbered
    pixels: delta = s / 2) and stands for the continuous values within delta / 2 of it, so the counts below edge e[k] hold the mass
    below (the first multiple of delta >= e[k]) - delta / 2."""
    e = PG.edges()
    if delta > 0.0:
        e[1:] = np.ceil(e[1:] / delta) * delta - 0.5 * delta
    return e


def level_variances(hist, delta=0.0):
    """Per level of one histogram [L][Q]: (n, v) with v the variance from the 0.25 quantile of |d| (pg_model.fit's, on lattice_edges, less
    the rounding's own variance delta^2 / 3), v = None where the level holds fewer than 256 blocks, its quantile falls into an end key
    or v is not positive."""
    e = lattice_edges(delta)
    out = []
    for l in range(L):
        h = hist[l].astype(np.int64)
        n = int(h.sum())
        v = None
        if n >= MIN_BLOCKS:
            T = 0.25 * n
            cum = np.cumsum(h)
            ks = int(np.argmax(cum >= T))
            if 0 < ks < Q - 1:
                Qv = e[ks] + (e[ks + 1] - e[ks]) * (T - float(cum[ks - 1])) / float(h[ks])
                r = Qv / PG.QUARTILE
                v = r * r - delta * delta / 3.0
                if not v > 0.0:
                    v = None
        out.append((n, v))
    return out


def fit_one(hist, cens, whole, lo=0.0, hi=255.0):
    """One histogram [L][Q] with cens [L] and `whole`, the count of blocks of whole-numbered pixels -> dict(sigma, levels, f_max), or
    None when fewer than 4 levels are populated."""
    delta = 0.5 * float(rescale(lo, hi)) if 0 < int(hist.sum()) == int(whole) else 0.0
    lv = level_variances(hist, delta)
    for f_max in LADDER:
        Sw = Swv = 0.0
        used = 0
        for l, (n, v) in enumerate(lv):
            if v is None or float(cens[l]) > f_max * n:
                continue
            w = n / (v * v)
            Sw += w
            Swv += w * v
            used += 1
        if used >= MIN_LEVELS:
            return dict(sigma=float(np.sqrt(Swv / Sw)) / float(rescale(lo, hi)), levels=used, f_max=f_max)
    return None


def fit(hist, cens, whole, lo=0.0, hi=255.0):
    """hist [C][L][Q], cens [C][L], whole [C] -> dict(sigma, sigma_channel, levels, f_max, censored, heavily_clipped) of the pooled channels (every
    channel's own sigma, NaN where its own fit fails), or None when the pooled fit fails."""
    hist, cens, whole = np.asarray(hist, np.uint64), np.asarray(cens, np.uint64), np.asarray(whole, np.uint64)
    pooled = fit_one(hist.sum(axis=0), cens.sum(axis=0), whole.sum(), lo, hi)
    if pooled is None:
        return None
    ch = [fit_one(hist[c], cens[c], whole[c], lo, hi) for c in range(hist.shape[0])]
    total = int(hist.sum())
    pooled.update(sigma_channel=[f["sigma"] if f else np.nan for f in ch], censored=float(int(cens.sum())) / total,
                  heavily_clipped=pooled["f_max"] > 0.1, quantised=int(whole.sum()) == total)
    return pooled


def estimate(lf, mask, W, H, C, lo=0.0, hi=255.0):
    """fit() of histogram(), with the statistics added to the dict; None when the fit fails."""
    hist, sm, cens, whole, blocks, skipped = histogram(lf, mask, W, H, C, lo, hi)
    r = fit(hist, cens, whole, lo, hi)
    if r is not None:
        r.update(hist=hist, sum_m=sm, cens=cens, whole=whole, blocks=blocks, skipped=skipped)
    return r


def _Phi(x):
    return 0.5 * erfc(-x / np.sqrt(2.0))


def _phi(x):
    return np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def clipped_mean(y, sigma, lo=0.0, hi=255.0):
    """E(y) = E[clip(y + sigma n, lo, hi)], n ~ N(0, 1), float64.  The tails are written with Phi(-x) where 1 - Phi(x) would cancel."""
    y = np.asarray(y, np.float64)
    a, b = (lo - y) / sigma, (hi - y) / sigma
    return lo * _Phi(a) + hi * _Phi(-b) + y * (_Phi(b) - _Phi(a)) + sigma * (_phi(a) - _phi(b))


def slope(y, sigma, lo=0.0, hi=255.0):
    y = np.asarray(y, np.float64)
    return _Phi((hi - y) / sigma) - _Phi((lo - y) / sigma)


def declip(d, sigma, lo=0.0, hi=255.0):
    """clamp(E^-1(d), lo, hi) in float64 by bisection on [lo, hi] (E is strictly increasing); non-finite values pass through."""
    d = np.asarray(d, np.float64)
    out = d.copy()
    fin = np.isfinite(d)
    x = d[fin]
    a, b = np.full(x.shape, float(lo)), np.full(x.shape, float(hi))
    for _ in range(64):
        mid = 0.5 * (a + b)
        up = clipped_mean(mid, sigma, lo, hi) < x
        a, b = np.where(up, mid, a), np.where(up, b, mid)
    y = 0.5 * (a + b)
    y = np.where(x <= clipped_mean(float(lo), sigma, lo, hi), float(lo), np.where(x >= clipped_mean(float(hi), sigma, lo, hi), float(hi), y))
    out[fin] = y
    return out
