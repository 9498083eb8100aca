"""Numpy model of the view synthesis (lfbm5d_view_*, include/lfbm5d.h): the checker of the tests, written from the definition.  A missing
sub-aperture image is the disparity-compensated mean of its sound angular neighbours: per integer hypothesis d the neighbours are warped
by d times their angular offset (mirrored, period 2n - 2), the squared deviations from their mean are summed over a (2r + 1)^2 box, and
the hypothesis with the smallest sum wins per pixel.  Everything in float32, every operation rounded on its own, sums in a fixed order
from +0: the GPU must equal this bit for bit, in values and in disparities.  The loop takes the regulariser as a function."""
import numpy as np

ROWMAJOR, COLMAJOR = 11, 12
RECIP = np.array([0.0] + [1.0 / n for n in range(1, 25)], np.float64).astype(np.float32)      # r[n] = (float)(1.0 / n)
D_MAX, R_MAX = 8, 7


def coords(st, ang_major, aw, ah):
    """(s, t) of SAI index st: s moves along image rows, t along columns."""
    return (st // aw, st % aw) if ang_major == ROWMAJOR else (st % ah, st // ah)


def reflect(g, n):
    """rho_n: reflection of period 2n - 2 without repeating the edge; any integer g -> 0..n-1 (n >= 2)."""
    P = 2 * (n - 1)
    g = np.mod(np.asarray(g, np.int64), P)
    return np.where(g < n, g, P - g)


def hypotheses(D):
    """0, -1, +1, -2, +2, ..., -D, +D"""
    out = [0]
    for a in range(1, D + 1):
        out += [-a, a]
    return out


def sources(m, mask, missing, ang_major, aw, ah, ang_radius):
    """[(q, s_q - s_m, t_q - t_m)] in increasing q: non-empty, not missing, within ang_radius (Chebyshev)."""
    sm, tm = coords(m, ang_major, aw, ah)
    out = []
    for q in range(aw * ah):
        if not mask[q] or missing[q]:
            continue
        s, t = coords(q, ang_major, aw, ah)
        if max(abs(s - sm), abs(t - tm)) <= ang_radius:
            out.append((q, s - sm, t - tm))
    return out


def warp_mean(x, srcs, d):
    """(the warped sources [n][C][H][W], their mean mu_d [C][H][W]) for hypothesis d; x [A][C][H][W] float32."""
    H, W = x.shape[2:]
    ys, xs = np.arange(H), np.arange(W)
    w = [x[q][:, reflect(ys - d * ds, H)][:, :, reflect(xs - d * dt, W)] for q, ds, dt in srcs]
    mu = np.zeros(x.shape[1:], np.float32)
    for wq in w:
        mu = (mu + wq).astype(np.float32)
    return w, (mu * RECIP[len(srcs)]).astype(np.float32)


def cost(x, srcs, d, r):
    """(E_d [H][W], mu_d [C][H][W])"""
    H, W = x.shape[2:]
    ys, xs = np.arange(H), np.arange(W)
    w, mu = warp_mean(x, srcs, d)
    e = np.zeros((H, W), np.float32)
    for c in range(x.shape[1]):
        for wq in w:
            diff = (wq[c] - mu[c]).astype(np.float32)
            e = (e + (diff * diff).astype(np.float32)).astype(np.float32)
    h = np.zeros((H, W), np.float32)
    for k in range(-r, r + 1):
        h = (h + e[:, reflect(xs + k, W)]).astype(np.float32)
    E = np.zeros((H, W), np.float32)
    for k in range(-r, r + 1):
        E = (E + h[reflect(ys + k, H), :]).astype(np.float32)
    return E, mu


def synth_view(x, srcs, D, r):
    """(view [C][H][W] float32, d* int8 [H][W]) of one missing SAI from its sources; x [A][C][H][W] float32."""
    best = view = disp = None
    for d in hypotheses(D):
        E, mu = cost(x, srcs, d, r)
        if best is None:
            best, view, disp = E, mu, np.zeros(E.shape, np.int8)
            continue
        take = E < best                                                    # strictly: ties keep the smaller |d|
        best = np.where(take, E, best)
        view = np.where(take[None], mu, view)
        disp = np.where(take, np.int8(d), disp)
    return view, disp


def fill(lf, mask, missing, ang_major, aw, ah, W, H, C, D, r, ang_radius=1, out=None, disp=None):
    """lf [asize][C*H*W] float32.  out / disp: initial contents of the outputs (only the planes of synthesised SAIs are written).
    Returns a dict: out float32 [A][C*H*W], disp int8 [A][H*W], missing, synthesised, left, pixels, hist (int64 [17], index d + 8),
    flags (uint8 like out: 1 on every value of a synthesised SAI), sais (the synthesised indices), left_sais."""
    A = aw * ah
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    res = np.array(x if out is None else np.asarray(out, np.float32).reshape(A, C, H, W), np.float32, copy=True)
    dsp = np.zeros((A, H, W), np.int8) if disp is None else np.array(np.asarray(disp, np.int8).reshape(A, H, W), copy=True)
    flags = np.zeros((A, C * H * W), np.uint8)
    hist = np.zeros(2 * D_MAX + 1, np.int64)
    done, left = [], []
    for m in range(A):
        if not missing[m]:
            continue
        if not mask[m]:
            raise ValueError("a missing SAI must be non-empty in the mask")
        srcs = sources(m, mask, missing, ang_major, aw, ah, ang_radius)
        if not srcs:
            left.append(m)
            continue
        view, d = synth_view(x, srcs, D, r)
        res[m].view(np.uint32)[...] = view.view(np.uint32)
        dsp[m] = d
        flags[m] = 1
        hist += np.bincount(d.astype(np.int64).ravel() + D_MAX, minlength=2 * D_MAX + 1)
        done.append(m)
    return dict(out=res.reshape(A, -1), disp=dsp.reshape(A, -1), missing=len(done) + len(left), synthesised=len(done), left=len(left),
                pixels=len(done) * H * W, hist=hist, flags=flags, sais=done, left_sais=left)


def sigma_schedule(K, sigma_start, sigma_end, sigma_noise=0.0):
    s0, s1, sn = float(np.float32(sigma_start)), float(np.float32(sigma_end)), float(np.float32(sigma_noise))
    return [max(s0 if K == 1 else s0 * (s1 / s0) ** ((k - 1) / (K - 1)), sn) for k in range(1, K + 1)]


def project(flags, x, y):
    """out = flag ? x : y, on the bits."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return np.where(np.asarray(flags) != 0, x.view(np.uint32), y.view(np.uint32)).view(np.float32)


def loop(y, mask, missing, ang_major, aw, ah, W, H, C, D, r, K, sigma_start, sigma_end, step, sigma_noise=0.0, ang_radius=1):
    """x_0 = y with the synthesised SAIs replaced; x_k = f ? step(x_{k-1}, sigma_k) : y, f = every value of the synthesised SAIs.
    step(light field [asize][C*H*W] float32, sigma) -> the basic estimate.  Returns (x_K, x_0, the synthesis' dict)."""
    y = np.ascontiguousarray(y, np.float32).reshape(aw * ah, -1)
    res = fill(y, mask, missing, ang_major, aw, ah, W, H, C, D, r, ang_radius)
    if K and res["left"]:
        raise ValueError("a missing SAI without a source cannot be refined")
    x = x0 = res["out"]
    for sig in sigma_schedule(K, sigma_start, sigma_end, sigma_noise):
        b = np.asarray(step(x.copy(), sig), np.float32).reshape(x.shape)
        x = project(res["flags"], b, y)
    return x, x0, res


def psnr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(10.0 * np.log10(255.0 ** 2 / ((a - b) ** 2).mean()))
