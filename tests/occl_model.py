"""Numpy model of the occlusion-aware plane sweep (lfbm5d_view_*_occl_*, include/lfbm5d_occl.h): the checker of the tests, written from
the definition on top of the sub-pixel model (tests/subpel_model.py: its warp, hypotheses and box).  Beside the full set of sources the
sweep evaluates four half-planes of them (dt <= 0, dt >= 0, ds <= 0, ds >= 0, each including the missing view's own row or column);
per cell and hypothesis the error is the scatter normalised by n_k - 1 of the full set, or of the best admissible half-plane where
that one is `ratio` times smaller; the value is the mean of the set chosen for the cell itself at j*.  Everything in float32, every
operation rounded on its own, sums in a fixed order from +0: the GPU must equal this bit for bit, in values, in j* and in k*."""
import numpy as np

import subpel_model as S
import view_model as V

SETS = 5
G = np.array([0.0, 0.0] + [1.0 / (n - 1) for n in range(2, 25)], np.float64).astype(np.float32)     # g[n] = (float)(1.0 / (n - 1))


def check_ratio(ratio):
    r = np.float32(ratio)
    if not (r == 0 or (np.isfinite(r) and r >= 1)):
        raise ValueError("occl_ratio must be 0 or a finite number of at least 1")
    return r


def sets(srcs):
    """The five sets of a table row as lists of positions into srcs, each in increasing source order: all, dt <= 0, dt >= 0, ds <= 0,
    ds >= 0."""
    idx = range(len(srcs))
    return [list(idx), [i for i in idx if srcs[i][2] <= 0], [i for i in idx if srcs[i][2] >= 0], [i for i in idx if srcs[i][1] <= 0],
            [i for i in idx if srcs[i][1] >= 0]]


def admissible(members, n):
    return 2 <= len(members) < n


def set_errors(x, srcs, j, Q):
    """([5] of e^_k [H][W] or None where set k is not evaluated, [5] of mu_k [C][H][W] or None) for the hypothesis j / Q."""
    C, H, W = x.shape[1:]
    w, _ = S.warp_mean(x, srcs, j, Q)
    n = len(srcs)
    errs, mus = [], []
    for k, members in enumerate(sets(srcs)):
        if k and not admissible(members, n):
            errs.append(None)
            mus.append(None)
            continue
        mu = np.zeros((C, H, W), np.float32)
        for q in members:
            mu = (mu + w[q]).astype(np.float32)
        mu = (mu * V.RECIP[len(members)]).astype(np.float32)
        v = np.zeros((H, W), np.float32)
        for c in range(C):
            for q in members:
                diff = (w[q][c] - mu[c]).astype(np.float32)
                v = (v + (diff * diff).astype(np.float32)).astype(np.float32)
        errs.append((v * G[len(members)]).astype(np.float32))
        mus.append(mu)
    return errs, mus


def choose(errs, ratio):
    """(k* uint8 [H][W], e = e^_{k*} [H][W]) of one hypothesis: among the admissible candidates in order a later one replaces the best
    only if strictly smaller; the best replaces set 0 only if (e^_best ratio) < e^_0, the product rounded."""
    best = kb = None
    for k in range(1, SETS):
        if errs[k] is None:
            continue
        if best is None:
            best, kb = errs[k], np.full(errs[k].shape, k, np.uint8)
            continue
        take = errs[k] < best
        best = np.where(take, errs[k], best)
        kb = np.where(take, np.uint8(k), kb)
    if best is None:
        return np.zeros(errs[0].shape, np.uint8), errs[0]
    with np.errstate(invalid="ignore", over="ignore"):
        use = (best * np.float32(ratio)).astype(np.float32) < errs[0]
    return np.where(use, kb, np.uint8(0)), np.where(use, best, errs[0])


def box(e, r):
    H, W = e.shape
    ys, xs = np.arange(H), np.arange(W)
    h = np.zeros((H, W), np.float32)
    for k in range(-r, r + 1):
        h = (h + e[:, V.reflect(xs + k, W)]).astype(np.float32)
    E = np.zeros((H, W), np.float32)
    for k in range(-r, r + 1):
        E = (E + h[V.reflect(ys + k, H), :]).astype(np.float32)
    return E


def sweep_errors(x, srcs, D, Q):
    """[(j, errs, mus)] of every hypothesis in the sweep's order: what does not depend on ratio and r."""
    with np.errstate(invalid="ignore", over="ignore"):
        return [(j,) + set_errors(x, srcs, j, Q) for j in V.hypotheses(D * Q)]


def decide(swept, ratio, r):
    """(view [C][H][W] float32, j* int8 [H][W], k* uint8 [H][W]) from sweep_errors()."""
    best = view = disp = kset = None
    for j, errs, mus in swept:
        k, e = choose(errs, ratio)
        with np.errstate(invalid="ignore", over="ignore"):
            E = box(e, r)
        mu = mus[0]
        for kk in range(1, SETS):
            if mus[kk] is not None:
                mu = np.where((k == kk)[None], mus[kk], mu)
        if best is None:
            best, view, disp, kset = E, mu, np.zeros(E.shape, np.int8), k
            continue
        take = E < best
        best = np.where(take, E, best)
        view = np.where(take[None], mu, view)
        disp = np.where(take, np.int8(j), disp)
        kset = np.where(take, k, kset)
    return view, disp, kset


def synth_view(x, srcs, D, r, Q, ratio):
    return decide(sweep_errors(x, srcs, D, Q), ratio, r)


def fill(lf, mask, missing, ang_major, aw, ah, W, H, C, D, r, ang_radius=1, out=None, disp=None, steps=1, ratio=0.0, sets_out=None,
         swept=None):
    """subpel_model.fill with the occlusion ratio: the dict gains sets (uint8 [A][H*W], k* on the planes of synthesised SAIs, initial
    contents sets_out elsewhere) and set_hist (int64 [5]).  ratio = 0 is subpel_model.fill (sets untouched, set_hist zero).
    swept: {m: sweep_errors(...)} computed before, or None."""
    ratio = check_ratio(ratio)
    A = aw * ah
    st = np.zeros((A, H, W), np.uint8) if sets_out is None else np.array(np.asarray(sets_out, np.uint8).reshape(A, H, W), copy=True)
    if ratio == 0:
        res = S.fill(lf, mask, missing, ang_major, aw, ah, W, H, C, D, r, ang_radius, out=out, disp=disp, steps=steps)
        return dict(res, sets=st.reshape(A, -1), set_hist=np.zeros(SETS, np.int64))
    assert steps in S.STEPS
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    res = np.array(x if out is None else np.asarray(out, np.float32).reshape(A, C, H, W), np.float32, copy=True)
    dsp = np.zeros((A, H, W), np.int8) if disp is None else np.array(np.asarray(disp, np.int8).reshape(A, H, W), copy=True)
    flags = np.zeros((A, C * H * W), np.uint8)
    hist, set_hist = np.zeros(S.HIST, np.int64), np.zeros(SETS, np.int64)
    done, left = [], []
    for m in range(A):
        if not missing[m]:
            continue
        if not mask[m]:
            raise ValueError("a missing SAI must be non-empty in the mask")
        srcs = V.sources(m, mask, missing, ang_major, aw, ah, ang_radius)
        if not srcs:
            left.append(m)
            continue
        view, d, k = decide(swept[m] if swept else sweep_errors(x, srcs, D, steps), ratio, r)
        res[m].view(np.uint32)[...] = view.view(np.uint32)
        dsp[m] = d
        st[m] = k
        flags[m] = 1
        hist += np.bincount(d.astype(np.int64).ravel() + S.J_MAX, minlength=S.HIST)
        set_hist += np.bincount(k.astype(np.int64).ravel(), minlength=SETS)
        done.append(m)
    return dict(out=res.reshape(A, -1), disp=dsp.reshape(A, -1), missing=len(done) + len(left), synthesised=len(done), left=len(left),
                pixels=len(done) * H * W, hist=hist, flags=flags, sais=done, left_sais=left, sets=st.reshape(A, -1), set_hist=set_hist)
