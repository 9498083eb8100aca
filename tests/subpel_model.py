"""Numpy model of the sub-pixel plane sweep (lfbm5d_view_*_steps_* and lfbm5d_consist_steps_*, include/lfbm5d.h): the checker of the
tests, written from the definition on top of the integer models (tests/view_model.py, tests/consist_model.py).  With Q steps per pixel
the hypotheses are d = j / Q, j = 0, -1, +1, ..., -DQ, +DQ, and a source is warped by bilinear interpolation between the four values
around its shifted position; the interpolation weights depend only on (j, ds, dt).  Everything in float32, every operation rounded on
its own, sums in a fixed order from +0: the GPU must equal this bit for bit, in values and in j*."""
import numpy as np

import consist_model as K
import view_model as V

STEPS = (1, 2, 4)
J_MAX = 32                                                                     # |j*| <= D_MAX * 4
HIST = 2 * J_MAX + 1                                                           # LFBM5D_VIEW_STEPS_HIST: index j* + 32 for every Q


def split(j, ds, Q):
    """(offset, p): Q y - j ds = Q (y + offset) + p with 0 <= p < Q; j an integer or an integer array."""
    n = -np.asarray(j, np.int64) * ds
    o = np.floor_divide(n, Q)
    return o, n - Q * o


def lerp(a, b, p, w):
    """a where p = 0, else a + w (b - a): a difference, a product and a sum, each rounded on its own.  p, w: scalars or arrays."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (b - a).astype(np.float32)
        prod = (np.asarray(w, np.float32) * diff).astype(np.float32)
        t = (a + prod).astype(np.float32)
    return np.where(np.asarray(p) == 0, a, t)


def warp(plane, ds, dt, j, Q, ys, xs):
    """w_{q,j} at the positions (ys, xs) (arrays that broadcast against j) of one source's planes [C][H][W]."""
    H, W = plane.shape[1:]
    oy, py = split(j, ds, Q)
    ox, px = split(j, dt, Q)
    wy, wx = (py.astype(np.float32) / np.float32(Q)).astype(np.float32), (px.astype(np.float32) / np.float32(Q)).astype(np.float32)
    r0, r1 = V.reflect(ys + oy, H), V.reflect(ys + oy + 1, H)
    c0, c1 = V.reflect(xs + ox, W), V.reflect(xs + ox + 1, W)
    top = lerp(plane[:, r0, c0], plane[:, r0, c1], px, wx)
    bot = lerp(plane[:, r1, c0], plane[:, r1, c1], px, wx)
    return lerp(top, bot, py, wy)


def warp_mean(x, srcs, j, Q):
    """(the warped sources [n][C][H][W], their mean [C][H][W]) for the hypothesis j / Q (one j for the plane)."""
    H, W = x.shape[2:]
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    w = [warp(x[q], ds, dt, j, Q, ys, xs) for q, ds, dt in srcs]
    mu = np.zeros(x.shape[1:], np.float32)
    for wq in w:
        mu = (mu + wq).astype(np.float32)
    return w, (mu * V.RECIP[len(srcs)]).astype(np.float32)


def cost(x, srcs, j, Q, r):
    """(E_j [H][W], mu_j [C][H][W]): the integer model's error and box sums on the interpolated warp."""
    H, W = x.shape[2:]
    ys, xs = np.arange(H), np.arange(W)
    w, mu = warp_mean(x, srcs, j, Q)
    e = np.zeros((H, W), np.float32)
    for c in range(x.shape[1]):
        for wq in w:
            diff = (wq[c] - mu[c]).astype(np.float32)
            e = (e + (diff * diff).astype(np.float32)).astype(np.float32)
    h = np.zeros((H, W), np.float32)
    for k in range(-r, r + 1):
        h = (h + e[:, V.reflect(xs + k, W)]).astype(np.float32)
    E = np.zeros((H, W), np.float32)
    for k in range(-r, r + 1):
        E = (E + h[V.reflect(ys + k, H), :]).astype(np.float32)
    return E, mu


def synth_view(x, srcs, D, r, Q):
    """(view [C][H][W] float32, j* int8 [H][W]) of one missing SAI from its sources."""
    best = view = disp = None
    for j in V.hypotheses(D * Q):
        E, mu = cost(x, srcs, j, Q, r)
        if best is None:
            best, view, disp = E, mu, np.zeros(E.shape, np.int8)
            continue
        take = E < best                                                        # strictly: ties keep the smaller |j|
        best = np.where(take, E, best)
        view = np.where(take[None], mu, view)
        disp = np.where(take, np.int8(j), disp)
    return view, disp


def fill(lf, mask, missing, ang_major, aw, ah, W, H, C, D, r, ang_radius=1, out=None, disp=None, steps=1):
    """view_model.fill with `steps` hypotheses per pixel: disp holds j* (d* in units of 1 / steps), hist is int64 [65], index j* + 32."""
    assert steps in STEPS
    A = aw * ah
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    res = np.array(x if out is None else np.asarray(out, np.float32).reshape(A, C, H, W), np.float32, copy=True)
    dsp = np.zeros((A, H, W), np.int8) if disp is None else np.array(np.asarray(disp, np.int8).reshape(A, H, W), copy=True)
    flags = np.zeros((A, C * H * W), np.uint8)
    hist = np.zeros(HIST, np.int64)
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
        view, d = synth_view(x, srcs, D, r, steps)
        res[m].view(np.uint32)[...] = view.view(np.uint32)
        dsp[m] = d
        flags[m] = 1
        hist += np.bincount(d.astype(np.int64).ravel() + J_MAX, minlength=HIST)
        done.append(m)
    return dict(out=res.reshape(A, -1), disp=dsp.reshape(A, -1), missing=len(done) + len(left), synthesised=len(done), left=len(left),
                pixels=len(done) * H * W, hist=hist, flags=flags, sais=done, left_sais=left)


def predict(x, srcs, D, r, Q):
    """consist_model.predict with the sub-pixel sweep: (mu, j*, v), v = sum_q (w_{q,j*} - mu)^2 with the interpolated warp at j*."""
    with np.errstate(invalid="ignore", over="ignore"):
        mu, disp = synth_view(x, srcs, D, r, Q)
    C, H, W = x.shape[1:]
    ys, xs = np.mgrid[0:H, 0:W]
    j = disp.astype(np.int64)
    v = np.zeros((C, H, W), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, ds, dt in srcs:
            diff = (warp(x[q], ds, dt, j, Q, ys, xs) - mu).astype(np.float32)
            v = (v + (diff * diff).astype(np.float32)).astype(np.float32)
    return mu, disp, v


def consist(lf, mask, ang_major, aw, ah, W, H, C, steps=1, **kw):
    """consist_model.consist with the prediction and the spread of the sub-pixel sweep: everything else is the integer model's code."""
    assert steps in STEPS
    D, r = kw.get("D", 4), kw.get("r", 3)
    saved = K.predict
    K.predict = lambda x, srcs, D_, r_: predict(x, srcs, D_, r_, steps)
    try:
        return K.consist(lf, mask, ang_major, aw, ah, W, H, C, **dict(kw, D=D, r=r))
    finally:
        K.predict = saved


def half_pixel_lf():
    """The light field that moves half a pixel per view: the photograph at 1 pixel per view and double resolution (3 x 3 views of
    96 x 160), reduced by a 2 x 2 box mean to 48 x 80.  [9][3*48*80] float32."""
    import helpers
    big = helpers.textured_lf(3, 3, 96, 160, 1).astype(np.float64)            # [9][3][96][160]
    small = big.reshape(9, 3, 48, 2, 80, 2).mean(axis=(3, 5))
    return small.astype(np.float32).reshape(9, -1)


def interior_psnr(a, b, C, H, W, border):
    a = np.asarray(a).reshape(C, H, W)[:, border:-border, border:-border]
    b = np.asarray(b).reshape(C, H, W)[:, border:-border, border:-border]
    return V.psnr(a, b)
