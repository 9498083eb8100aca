"""Float64 numpy model of the super-resolution of include/lfbm5d.h (lfbm5d_sr_* / lfbm5d_superres_*): the tap formulas of the
operators U and D, their dense application, one back-projection, and the loop with a pluggable regulariser.  Independent of the
library: the tests compare the library with it."""
import numpy as np

BICUBIC, GAUSSIAN = 0, 1


def keys(x):
    """Keys cubic convolution kernel, a = -0.5."""
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x <= 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, 0.0))


def taps_up(scale, n_in):
    """U: u = (X+0.5)/s - 0.5, first = floor(u) - 1, T = 4, w_t = keys(u - (first+t))."""
    X = np.arange(n_in * scale, dtype=np.float64)
    u = (X + 0.5) / scale - 0.5
    first = np.floor(u).astype(np.int64) - 1
    w = keys(u[:, None] - (first[:, None] + np.arange(4)[None, :]))
    return first, w


def taps_down(scale, kernel, blur_sigma, n_in):
    """D: u = (x+0.5) s - 0.5; bicubic: taps in [ceil(u-2s), floor(u+2s)], keys((u-j)/s); Gaussian: R = ceil(3 sigma_b), taps in
    [ceil(u-R), floor(u+R)], exp(-(u-j)^2 / (2 sigma_b^2)); normalised to sum 1; rows padded with zeros to the longest."""
    assert n_in % scale == 0
    sb = float(np.float32(blur_sigma))          # the library's struct holds a float
    R = float(np.ceil(3.0 * sb)) if kernel == GAUSSIAN else 2.0 * scale
    rows, first = [], []
    for x in range(n_in // scale):
        u = (x + 0.5) * scale - 0.5
        j = np.arange(int(np.ceil(u - R)), int(np.floor(u + R)) + 1)
        d = u - j
        w = np.exp(-(d * d) / (2.0 * sb * sb)) if kernel == GAUSSIAN else keys(d / scale)
        rows.append(w / w.sum())
        first.append(j[0])
    T = max(len(r) for r in rows)
    w = np.zeros((len(rows), T))
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return np.array(first, np.int64), w


def round32(taps):
    first, w = taps
    return first, w.astype(np.float32).astype(np.float64)


def apply_1d(taps, x, n_in):
    """out[..., X] = sum_t w[X][t] x[..., clamp(first[X]+t, 0, n_in-1)] along the last axis."""
    first, w = taps
    idx = np.clip(first[:, None] + np.arange(w.shape[1])[None, :], 0, n_in - 1)
    return (np.asarray(x, np.float64)[..., idx] * np.asarray(w, np.float64)).sum(-1)


def apply_2d(tx, ty, planes):
    """Ry * plane * Rx^T on [..., h, w] planes, horizontal pass first."""
    planes = np.asarray(planes, np.float64)
    t = apply_1d(tx, planes, planes.shape[-1])
    return np.swapaxes(apply_1d(ty, np.swapaxes(t, -1, -2), planes.shape[-2]), -1, -2)


class Ops:
    """U and D for one geometry (w, h = the low-resolution size).  taps = dict(ux, uy, dx, dy) replaces the model's own tables
    (the library's float32 tables: then only the accumulation differs); rounded=True rounds the model's tables to float32."""

    def __init__(self, scale, kernel, blur_sigma, w, h, taps=None, rounded=True):
        self.scale, self.w, self.h = scale, w, h
        if taps is None:
            taps = dict(ux=taps_up(scale, w), uy=taps_up(scale, h), dx=taps_down(scale, kernel, blur_sigma, w * scale),
                        dy=taps_down(scale, kernel, blur_sigma, h * scale))
            if rounded:
                taps = {k: round32(v) for k, v in taps.items()}
        self.t = {k: (np.asarray(v[0], np.int64), np.asarray(v[1], np.float64)) for k, v in taps.items()}

    def up(self, low):
        return apply_2d(self.t["ux"], self.t["uy"], low)

    def down(self, high):
        return apply_2d(self.t["dx"], self.t["dy"], high)

    def backproject(self, y, x, beta=1.0):
        return x + beta * self.up(np.asarray(y, np.float64) - self.down(x))


def sigma_schedule(K, sigma_start, sigma_end):
    s0, s1 = float(np.float32(sigma_start)), float(np.float32(sigma_end))
    return [s0 if K == 1 else s0 * (s1 / s0) ** ((k - 1) / (K - 1)) for k in range(1, K + 1)]


def loop(ops, y, K, sigma_start, sigma_end, regulariser, beta=1.0, close_projection=True):
    """x_0 = U y; x_k = regulariser(x_{k-1} + beta U (y - D x_{k-1}), sigma_k); closing projection.  regulariser = None: plain
    back-projection (the K projections without a filter)."""
    x = ops.up(y)
    for sig in sigma_schedule(K, sigma_start, sigma_end):
        z = ops.backproject(y, x, beta)
        x = z if regulariser is None else np.asarray(regulariser(z, sig), np.float64)
    return ops.backproject(y, x, beta) if close_projection else x


def psnr(a, b):
    """Mean over the SAIs (first axis) of the per-SAI PSNR."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    mse = ((a - b) ** 2).reshape(a.shape[0], -1).mean(1)
    return float(np.mean(10.0 * np.log10(255.0 ** 2 / mse)))
