"""Numpy model of the consistency check (lfbm5d_consist_*, include/lfbm5d.h): the checker of the tests, written from the definition on
top of the view synthesis' model (tests/view_model.py).  Every tested SAI is predicted from its angular neighbours by the plane sweep
with the SAI itself left out; the residual against that prediction is compared with a threshold taken from the light field's own median
residual and with the spread of the sources around their mean.  Residual, spread and both tests in float32, every operation rounded on
its own; histograms and counts in integers; quantiles and the bad-SAI decision in float64 on the histograms.  The GPU must equal every
integer and float this file returns bit for bit."""
import numpy as np

import impulse_model as I
import view_model as V

EMPTY, TESTED, BAD, UNTESTED, EXCLUDED = 0, 1, 2, 3, 4
Q = I.Q


def predict(x, srcs, D, r):
    """(mu [C][H][W], d* int8 [H][W], v [C][H][W]) of one SAI from its sources: the sweep's mean at d*, and
    v = sum_q (w_{q,d*} - mu)^2 from +0 in source order, per channel."""
    with np.errstate(invalid="ignore", over="ignore"):
        mu, disp = V.synth_view(x, srcs, D, r)
    C, H, W = x.shape[1:]
    ys, xs = np.mgrid[0:H, 0:W]
    d = disp.astype(np.int64)
    v = np.zeros((C, H, W), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, ds, dt in srcs:
            w = x[q][:, V.reflect(ys - d * ds, H), V.reflect(xs - d * dt, W)]
            diff = (w - mu).astype(np.float32)
            v = (v + (diff * diff).astype(np.float32)).astype(np.float32)
    return mu, disp, v


def lower_median(values):
    s = sorted(values)
    return s[(len(s) - 1) // 2]


def decide(s, tested, ang_major, aw, ah, ang_radius, sai_factor, min_scale):
    """(ref, exceeds, bad) from the per-SAI scales s (None = an empty histogram): the bad-SAI decision of include/lfbm5d.h."""
    live = [m for m in tested if s[m] is not None]
    bad = [m for m in tested if s[m] is None]
    if not live:
        return 0.0, [], sorted(bad)
    ref = lower_median([s[m] for m in live])
    limit = float(sai_factor) * max(ref, float(min_scale))
    exceeds = [m for m in live if s[m] > limit]
    for m in exceeds:
        sm, tm = V.coords(m, ang_major, aw, ah)
        beaten = False
        for q in exceeds:
            if q == m:
                continue
            sq, tq = V.coords(q, ang_major, aw, ah)
            if max(abs(sq - sm), abs(tq - tm)) <= ang_radius and (s[q] > s[m] or (s[q] == s[m] and q < m)):
                beaten = True
        if not beaten:
            bad.append(m)
    return ref, exceeds, sorted(bad)


def sweep(x, mask, excl, ang_major, aw, ah, D, r, ang_radius, min_sources, cache=None):
    """One sweep with the exclude set excl: per tested SAI the prediction and the residual statistics.  cache (a dict, or None) keeps
    the predictions of this light field at this (D, r) by (SAI, sources) for callers that sweep parameters."""
    A, C, H, W = x.shape
    tested, untested, pred = [], [], {}
    hist = np.zeros((A, C, Q), np.uint64)
    skipped = 0
    for m in range(A):
        if not mask[m] or excl[m]:
            continue
        missing = np.array(excl, np.uint32)
        missing[m] = 1
        srcs = V.sources(m, mask, missing, ang_major, aw, ah, ang_radius)
        if len(srcs) < min_sources:
            untested.append(m)
            continue
        key = (m, tuple(srcs))
        if cache is None or key not in cache:
            got = predict(x, srcs, D, r)
            if cache is not None:
                cache[key] = got
        mu, disp, v = got if cache is None else cache[key]
        with np.errstate(invalid="ignore", over="ignore"):
            rho = (x[m] - mu).astype(np.float32)
        a = np.abs(rho)
        fin = np.isfinite(x[m])
        for c in range(C):
            hist[m, c] = np.bincount(I.keys(np.ascontiguousarray(a[c][fin[c]])), minlength=Q).astype(np.uint64)
        skipped += int((~fin).sum())
        tested.append(m)
        pred[m] = (rho, a, v, disp, fin, srcs, mu)
    return tested, untested, pred, hist, skipped


def consist(lf, mask, ang_major, aw, ah, W, H, C, D=4, r=3, ang_radius=1, k=8.0, min_threshold=0.0, spread=3.0, min_sources=2,
            sai_factor=2.0, min_scale=0.5, max_rounds=3, exclude=None, flags=None, disp=None, cache=None):
    """lf [asize][C*H*W] float32.  flags / disp: initial contents of the outputs (planes of empty SAIs keep them; disparity planes are
    written for tested SAIs only).  Returns a dict: flags uint8 [A][C*H*W], state int [A], disp int8 [A][H*W], hist uint64 [A][C][386],
    scale_channel [3], threshold float32 [3], scale_sai float64 [A] (0 where there is none), counts int [3][2] (channel; code 1, code 2),
    bad, untested, tested (lists), rounds, pixels, skipped, trace (per sweep: exclude, scale_sai, ref, exceeds, bad), mu (the final
    sweep's prediction, float32 [A][C*H*W], 0 where there is none), sources (per tested SAI its source list)."""
    A = aw * ah
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    mask = np.asarray(mask)
    excl = np.zeros(A, np.uint32) if exclude is None else (np.asarray(exclude) != 0).astype(np.uint32)
    given = excl.copy()
    all_bad, trace = [], []
    sweeps = decisions = 0
    while True:
        tested, untested, pred, hist, skipped = sweep(x, mask, excl, ang_major, aw, ah, D, r, ang_radius, min_sources, cache)
        sweeps += 1
        s = {m: I.scale(hist[m].sum(axis=0)) for m in tested}
        step = dict(exclude=excl.copy(), scale_sai=dict(s), ref=0.0, exceeds=[], bad=[])
        trace.append(step)
        if sai_factor > 0 and decisions < max_rounds:
            decisions += 1
            step["ref"], step["exceeds"], step["bad"] = decide(s, tested, ang_major, aw, ah, ang_radius, sai_factor, min_scale)
            if step["bad"]:
                excl = excl.copy()
                excl[step["bad"]] = 1
                all_bad += step["bad"]
                continue
        break
    pooled = hist[tested].sum(axis=0) if tested else np.zeros((C, Q), np.uint64)
    sc = [I.scale(pooled[c]) or 0.0 for c in range(C)]
    T = np.array([max(float(k) * sc[c], float(min_threshold)) for c in range(C)], np.float64).astype(np.float32)
    g = np.float32(float(spread) * float(spread))
    out = np.zeros((A, C * H * W), np.uint8) if flags is None else np.array(np.asarray(flags, np.uint8).reshape(A, -1), copy=True)
    dsp = np.zeros((A, H * W), np.int8) if disp is None else np.array(np.asarray(disp, np.int8).reshape(A, -1), copy=True)
    state = np.zeros(A, np.int64)
    counts = np.zeros((3, 2), np.int64)
    pmu = np.zeros((A, C * H * W), np.float32)
    for m in range(A):
        if not mask[m]:
            continue
        out[m] = 0
        state[m] = EXCLUDED if given[m] else BAD if m in all_bad else UNTESTED if m in untested else TESTED
    for m in tested:
        rho, a, v, d, fin, srcs, mu = pred[m]
        n = len(srcs)
        pmu[m] = mu.reshape(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            lhs = ((rho * rho).astype(np.float32) * np.float32(n - 1)).astype(np.float32)
            rhs = (g * v).astype(np.float32)
            one = (a > T[:C, None, None]) & (lhs > rhs)
        code = np.where(~fin, 2, np.where(one, 1, 0)).astype(np.uint8)
        out[m] = code.reshape(-1)
        dsp[m] = d.reshape(-1)
        for c in range(C):
            counts[c, 0] += int((code[c] == 1).sum())
            counts[c, 1] += int((code[c] == 2).sum())
    scale_sai = np.zeros(A, np.float64)
    for step in trace:                                                         # a bad SAI keeps the scale it was judged by
        for m in step["bad"]:
            scale_sai[m] = step["scale_sai"][m] or 0.0
    for m in tested:
        scale_sai[m] = trace[-1]["scale_sai"][m] or 0.0
    thr = np.zeros(3, np.float32)
    thr[:C] = T
    return dict(flags=out, state=state, disp=dsp, hist=hist, scale_channel=sc + [0.0] * (3 - C), threshold=thr, scale_sai=scale_sai,
                counts=counts, bad=sorted(all_bad), untested=untested, tested=tested, rounds=sweeps, pixels=len(tested) * C * H * W,
                skipped=skipped, trace=trace, mu=pmu, sources={m: pred[m][5] for m in tested})
