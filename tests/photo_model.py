"""Numpy model of the photometric equalisation (lfbm5d_photo_*, include/lfbm5d_photo.h): the checker of the tests, written from the
definition on top of the view synthesis' models (tests/view_model.py, tests/subpel_model.py), the way tests/consist_model.py is.  Every
tested SAI is predicted from its angular neighbours by the plane sweep with the SAI itself left out; the ratio of a value to its
prediction is keyed without a division, the median ratio of an SAI comes from an integer histogram, and the gains follow from the
ratios by a fixed iteration.  Keys and corrections in float32, every operation rounded on its own; histograms and counts in integers;
ratios and gains in float64.  The GPU must equal every integer and float this file returns bit for bit."""
import numpy as np

import consist_model as K
import subpel_model as S
import view_model as V

EMPTY, FITTED, UNTESTED, UNFIT = 0, 1, 2, 3
N_EDGES, KEYS = 1025, 1026
SOLVE_STEPS = 512
NO_ANCHOR = None


def edges():
    """e_j = 2^(j // 256 - 2) (1 + (j mod 256) / 256), j = 0..1024: 256 keys per octave over 1/4..4, every one a float32."""
    j = np.arange(N_EDGES)
    e = np.ldexp(1.0 + (j % 256) / 256.0, j // 256 - 2)
    assert (e.astype(np.float32).astype(np.float64) == e).all()
    return e.astype(np.float32)


EDGES = edges()


def keys(I, mu):
    """key = #{ j : I >= fl(e_j mu) } of float32 arrays (mu >= 0, both finite): the 11-step search over the monotone products."""
    I, mu = np.asarray(I, np.float32), np.asarray(mu, np.float32)
    pos = np.zeros(I.shape, np.int64)
    step = 1024
    while step:
        cand = pos + step
        ok = cand <= N_EDGES
        with np.errstate(over="ignore", invalid="ignore"):
            prod = (EDGES[np.where(ok, cand - 1, 0)] * mu).astype(np.float32)
        pos = np.where(ok & (I >= prod), cand, pos)
        step >>= 1
    return pos


def keys_by_definition(I, mu):
    """The same by counting over all 1025 edges (small inputs: the test of keys())."""
    I, mu = np.asarray(I, np.float32).ravel(), np.asarray(mu, np.float32).ravel()
    prod = (EDGES[None, :] * mu[:, None]).astype(np.float32)
    return (I[:, None] >= prod).sum(axis=1)


def ratio(h, min_count=1):
    """(r, fitted) of one histogram [1026]: the interpolated median ratio; (1.0, False) for fewer than min_count values or a median
    in an end key."""
    h = [int(v) for v in np.asarray(h).ravel()]
    assert len(h) == KEYS
    N = sum(h)
    T = (N + 1) // 2
    before = 0
    for k in range(KEYS):
        if before + h[k] >= T:
            break
        before += h[k]
    if N < int(min_count) or k == 0 or k == KEYS - 1:
        return 1.0, False
    e0, e1 = float(EDGES[k - 1]), float(EDGES[k])
    return e0 + (e1 - e0) * (float(T - before) - 0.5) / float(h[k]), True


def solve(r, neighbours, fitted, anchor=None, steps=SOLVE_STEPS, trace=None):
    """g [A] from the ratios r [A]: g = 1, then `steps` times h_m = (g_m + r_m (sum of g over m's sources, in order) / n_m) / 2 for
    every fitted m at once, divided by the lower median of the fitted h (or by h of `anchor`).  neighbours[m]: the source indices of
    m (needed for fitted m only).  trace: a list that receives every iterate."""
    A = len(r)
    g = [1.0] * A
    fit = [m for m in range(A) if fitted[m]]
    for _ in range(steps):
        h = list(g)
        for m in fit:
            s = 0.0
            for q in neighbours[m]:
                s = s + g[int(q)]
            h[m] = 0.5 * (g[m] + float(r[m]) * s / float(len(neighbours[m])))
        if fit:
            div = h[int(anchor)] if anchor is not None else K.lower_median([h[m] for m in fit])
            for m in fit:
                h[m] = h[m] / div
        g = h
        if trace is not None:
            trace.append(list(g))
    return np.array(g, np.float64)


def predict(x, srcs, D, r, steps):
    with np.errstate(invalid="ignore", over="ignore"):
        return V.synth_view(x, srcs, D, r) if steps == 1 else S.synth_view(x, srcs, D, r, steps)


def sweep(x, mask, ang_major, aw, ah, D, r, ang_radius, steps, min_sources, lo, hi):
    """One sweep: (tested, untested, sources per tested SAI, hist uint64 [A][C][1026], non-finite, out of range, mu per tested SAI)."""
    A, C, H, W = x.shape
    lo, hi = np.float32(lo), np.float32(hi)
    hist = np.zeros((A, C, KEYS), np.uint64)
    tested, untested, sources, mus = [], [], {}, {}
    nonfinite = outside = 0
    for m in range(A):
        if not mask[m]:
            continue
        missing = np.zeros(A, np.uint32)
        missing[m] = 1
        srcs = V.sources(m, mask, missing, ang_major, aw, ah, ang_radius)
        if len(srcs) < min_sources:
            untested.append(m)
            continue
        mu, _ = predict(x, srcs, D, r, steps)
        fin = np.isfinite(x[m]) & np.isfinite(mu)
        with np.errstate(invalid="ignore"):
            inside = fin & (mu >= lo) & (mu <= hi)
        nonfinite += int((~fin).sum())
        outside += int((fin & ~inside).sum())
        for c in range(C):
            hist[m, c] = np.bincount(keys(x[m, c][inside[c]], mu[c][inside[c]]), minlength=KEYS).astype(np.uint64)
        tested.append(m)
        sources[m] = [q for q, _, _ in srcs]
        mus[m] = mu
    return tested, untested, sources, hist, nonfinite, outside, mus


def factor(g, invert=False):
    """(float)(invert ? g : 1.0 / g)"""
    g = np.asarray(g, np.float64)
    return (g if invert else 1.0 / g).astype(np.float32)


def apply_gains(lf, mask, gain, C, invert=False, out=None):
    """out = in (float)(invert ? G : 1 / G) per (SAI, channel), one float32 multiplication per value; planes of empty SAIs keep `out`."""
    x = np.ascontiguousarray(lf, np.float32)
    A = x.shape[0]
    v = x.reshape(A, C, -1)
    res = np.array(x if out is None else np.asarray(out, np.float32).reshape(x.shape), np.float32, copy=True)
    f = factor(np.asarray(gain, np.float64).reshape(A, 3), invert)
    for m in range(A):
        if mask[m]:
            with np.errstate(invalid="ignore", over="ignore"):
                res[m] = (v[m] * f[m, :C, None]).astype(np.float32).reshape(-1)
    return res


def equalise(lf, mask, ang_major, aw, ah, W, H, C, D=4, r=3, ang_radius=1, steps=1, min_sources=3, max_rounds=3, tol=1.0 / 256,
             min_count=256, per_channel=1, anchor=None, lo=16.0, hi=200.0, out=None):
    """lf [asize][C*H*W] float32.  out: initial contents of the output (planes of empty SAIs keep them).  Returns a dict: out float32
    [A][C*H*W], gain float64 [A][3], state int [A], hist uint64 [A][C][1026] (the last sweep's), rounds, converged, residual, gain_min,
    gain_max, fitted, untested, unfit (SAI counts), admitted, nonfinite, outside (the last sweep's), ratios (per sweep: float64 [A][C]),
    fits (per sweep: bool [A][C]), gains (per correction: G after it)."""
    A = aw * ah
    x = np.array(np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W), copy=True)
    mask = np.asarray(mask)
    G = np.ones((A, 3), np.float64)
    rounds = converged = 0
    residual = 0.0
    all_r, all_fit, all_G = [], [], []
    while True:
        tested, untested, sources, hist, nonfinite, outside, _ = sweep(x, mask, ang_major, aw, ah, D, r, ang_radius, steps, min_sources, lo, hi)
        rounds += 1
        rr, fit = np.ones((A, C), np.float64), np.zeros((A, C), bool)
        for m in tested:
            if per_channel:
                for c in range(C):
                    rr[m, c], fit[m, c] = ratio(hist[m, c], min_count)
            else:
                rr[m, :], fit[m, :] = ratio(hist[m].sum(axis=0), min_count)
        all_r.append(rr)
        all_fit.append(fit)
        residual = max([abs(rr[m, c] - 1.0) for m in range(A) for c in range(C) if fit[m, c]], default=0.0)
        if residual <= tol:
            converged = 1
            break
        for c in range(C if per_channel else 1):
            g = solve(rr[:, c], sources, fit[:, c], anchor)
            for cc in ([c] if per_channel else range(C)):
                f = factor(g)
                for m in range(A):
                    if mask[m]:
                        with np.errstate(invalid="ignore", over="ignore"):
                            x[m, cc] = (x[m, cc] * f[m]).astype(np.float32)
                G[:, cc] = G[:, cc] * g
        all_G.append(G.copy())
        if rounds == max_rounds:
            break
    res = np.array(x.reshape(A, -1) if out is None else np.asarray(out, np.float32).reshape(A, -1), np.float32, copy=True)
    state = np.zeros(A, np.int64)
    for m in range(A):
        if mask[m]:
            res[m].view(np.uint32)[...] = x[m].reshape(-1).view(np.uint32)
            state[m] = UNTESTED if m in untested else FITTED if fit[m].all() else UNFIT
    live = [m for m in range(A) if mask[m]]
    return dict(out=res, gain=G, state=state, hist=hist, rounds=rounds, converged=converged, residual=residual,
                gain_min=float(G[live][:, :C].min()), gain_max=float(G[live][:, :C].max()), fitted=int((state == FITTED).sum()),
                untested=int((state == UNTESTED).sum()), unfit=int((state == UNFIT).sum()), admitted=int(hist.sum()), nonfinite=nonfinite,
                outside=outside, ratios=all_r, fits=all_fit, gains=all_G, tested=tested, sources=sources)
