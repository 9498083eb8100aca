"""Synthetic light-field generator of SURVEY.md section 8(d): integer-exact, numpy only.

Background = 3 octaves of bilinearly interpolated lattice value-noise (pitches 64/16/4, amplitudes
64/32/16) + 128 on a canvas, foreground = 12 constant-colour axis-aligned rectangles; SAI (s, t)
samples the background at integer offset 1*(s-cs, t-ct) and the foreground at 2*(s-cs, t-ct)
(disparities of 1 and 2 px per view), centre crop W x H, clipped to [0,255], integer valued.
All randomness comes from one LCG stream x <- 1664525 x + 1013904223 (mod 2^32), seed 12345,
top 16 bits of each output.
"""
import numpy as np


class _LCG:
    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def take(self, n):
        out = np.empty(n, np.int64)
        x = self.x
        for i in range(n):
            x = (1664525 * x + 1013904223) & 0xFFFFFFFF
            out[i] = x >> 16
        self.x = x
        return out


def _canvas(size, rng):
    """[3][size][size] int64 background, scaled by 1 (grey levels)."""
    acc = np.zeros((3, size, size), np.int64)
    yy = np.arange(size)
    for pitch, amp in ((64, 64), (16, 32), (4, 16)):
        n = size // pitch + 2
        for c in range(3):
            lat = (rng.take(n * n).reshape(n, n) * (2 * amp) // 65536) - amp   # ints in [-amp, amp)
            i0, f = yy // pitch, yy % pitch
            w1 = f[:, None] * np.ones((1, size), np.int64)          # fy
            w2 = np.ones((size, 1), np.int64) * f[None, :]          # fx
            a = lat[i0][:, i0]
            b = lat[i0][:, i0 + 1]
            cc = lat[i0 + 1][:, i0]
            d = lat[i0 + 1][:, i0 + 1]
            P = pitch
            v = a * (P - w1) * (P - w2) + b * (P - w1) * w2 + cc * w1 * (P - w2) + d * w1 * w2
            acc[c] += np.floor_divide(v, P * P)
    return acc + 128


def make_lf(aheight, awidth, H, W, seed=12345):
    """Returns uint8 array [aheight*awidth][3][H][W], st = s*awidth + t (row-major)."""
    cs, ct = aheight // 2, awidth // 2
    margin = 2 * max(cs, ct) + 8
    size = ((max(H, W) + 2 * margin + 63) // 64) * 64
    rng = _LCG(seed)
    bg = _canvas(size, rng)
    r = rng.take(12 * 7).reshape(12, 7)
    rects = []
    for q in r:
        x0, y0 = q[0] * size // 65536, q[1] * size // 65536
        w, h = 24 + q[2] * 96 // 65536, 24 + q[3] * 96 // 65536
        col = (q[4] * 256 // 65536, q[5] * 256 // 65536, q[6] * 256 // 65536)
        rects.append((int(x0), int(y0), int(w), int(h), col))
    oy, ox = (size - H) // 2, (size - W) // 2
    # foreground layer on its own canvas (later rectangles overwrite earlier ones)
    fg = np.zeros((3, size, size), np.uint8)
    bg = np.clip(bg, 0, 255).astype(np.uint8)
    fgm = np.zeros((size, size), bool)
    for (x0, y0, w, h, col) in rects:
        y1, x1 = min(size, y0 + h), min(size, x0 + w)
        fgm[y0:y1, x0:x1] = True
        for c in range(3):
            fg[c, y0:y1, x0:x1] = col[c]
    out = np.empty((aheight * awidth, 3, H, W), np.uint8)
    for s in range(aheight):
        for t in range(awidth):
            ds, dt = s - cs, t - ct
            img = bg[:, oy + ds:oy + ds + H, ox + dt:ox + dt + W]
            y2, x2 = oy + 2 * ds, ox + 2 * dt                     # foreground sampled at 2*(ds, dt)
            m = fgm[y2:y2 + H, x2:x2 + W]
            img = np.where(m[None], fg[:, y2:y2 + H, x2:x2 + W], img)
            out[s * awidth + t] = img
    return out


def add_noise_mt19937(clean, sigma, seed=1, out=None):
    """Additive white Gaussian noise exactly as the reference's add_noise draws it (utilities.cpp:176-183 with
    mt19937ar.c): ONE MT19937 stream seeded with init_genrand(seed), samples in memory order (SAIs in st order,
    planar pixels), per sample a = genrand_res53(), b = genrand_res53(), z = sigma * sqrt(-2 ln a) * cos(2 pi b)
    in double, added as float.  numpy's legacy RandomState(seed) is that generator (init_genrand seeding, and
    random_sample() is genrand_res53), so no C code is needed.  clean: float32 array of any shape; returns float32.
    """
    import os
    from concurrent.futures import ThreadPoolExecutor
    clean = np.ascontiguousarray(clean, dtype=np.float32)
    res = np.empty_like(clean) if out is None else out
    flat_in, flat_out = clean.reshape(-1), res.reshape(-1)
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    workers = max(1, min(32, (os.cpu_count() or 1)))
    piece = 1 << 18

    def box_muller(args):          # numpy releases the GIL inside log / sqrt / cos
        u, i, n = args
        z = float(sigma) * np.sqrt(-2.0 * np.log(u[0:2 * n:2])) * np.cos(2.0 * np.pi * u[1:2 * n:2])
        flat_out[i:i + n] = flat_in[i:i + n] + z.astype(np.float32)

    with ThreadPoolExecutor(workers) as pool:
        chunk = piece * workers
        for i0 in range(0, flat_in.size, chunk):      # the stream itself is drawn sequentially, in order
            n0 = min(chunk, flat_in.size - i0)
            u = rs.random_sample(2 * n0)
            jobs = [(u[2 * j:2 * min(j + piece, n0)], i0 + j, min(piece, n0 - j)) for j in range(0, n0, piece)]
            list(pool.map(box_muller, jobs))
    return res


def add_view_noise(clean, sigma_sai, seed=1):
    """Additive white Gaussian noise of standard deviation sigma_sai[v] on view v of `clean` ([A][...]): the generator, its seeding and
    the two draws per sample of add_noise_mt19937 -- ONE MT19937 stream, drawn SAI after SAI in memory order -- with the SAI's own sigma
    in z = sigma_v * sqrt(-2 ln a) * cos(2 pi b).  A uniform table returns add_noise_mt19937's result.  Returns float32."""
    clean = np.ascontiguousarray(clean, dtype=np.float32)
    sig = np.asarray(sigma_sai, dtype=np.float64).reshape(-1)
    if clean.ndim < 1 or sig.size != clean.shape[0]:
        raise ValueError("add_view_noise: sigma_sai needs one value per view")
    res = np.empty_like(clean)
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    for v in range(clean.shape[0]):
        n = clean[v].size
        u = rs.random_sample(2 * n)
        z = float(sig[v]) * np.sqrt(-2.0 * np.log(u[0::2])) * np.cos(2.0 * np.pi * u[1::2])
        res[v] = clean[v] + z.astype(np.float32).reshape(clean[v].shape)
    return res


def gaussian_taps(width, size=7):
    """size x size taps of a Gaussian of standard deviation `width` pixels, normalised to unit energy (sum of squares 1)."""
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2
    g = np.exp(-0.5 * (x / float(width)) ** 2)
    g = np.outer(g, g)
    return g / np.sqrt((g * g).sum())


def add_correlated_noise(clean, sigma, kernel, seed=1):
    """Spatially correlated Gaussian noise of marginal standard deviation `sigma` on `clean` ([...][H][W]: the last two axes are a
    plane): white noise of add_noise_mt19937's generator -- one MT19937 stream, two draws per sample, plane after plane in memory
    order -- filtered by `kernel` (up to 7 x 7 taps, any scale: it is normalised to unit energy, so the marginal level stays sigma).
    Each plane draws (H + gh - 1) x (W + gw - 1) samples and keeps the part the taps cover fully: the noise is stationary up to
    the border.  Its autocorrelation is corr_from_kernel(kernel).  Returns float32."""
    clean = np.ascontiguousarray(clean, dtype=np.float32)
    g = np.atleast_2d(np.asarray(kernel, dtype=np.float64))
    if clean.ndim < 2 or g.ndim != 2 or not (g * g).sum() > 0:
        raise ValueError("add_correlated_noise: clean is [...][H][W], kernel a 2-D array of taps that are not all zero")
    g = g / np.sqrt((g * g).sum())
    gh, gw = g.shape
    H, W = clean.shape[-2:]
    planes = clean.reshape(-1, H, W)
    res = np.empty_like(planes)
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    for i in range(planes.shape[0]):
        n = (H + gh - 1) * (W + gw - 1)
        u = rs.random_sample(2 * n)
        w = (np.sqrt(-2.0 * np.log(u[0::2])) * np.cos(2.0 * np.pi * u[1::2])).reshape(H + gh - 1, W + gw - 1)
        z = np.zeros((H, W), np.float64)
        for y in range(gh):
            for x in range(gw):
                z += g[y, x] * w[y:y + H, x:x + W]
        res[i] = planes[i] + (float(sigma) * z).astype(np.float32)
    return res.reshape(clean.shape)


def add_poisson_gaussian(clean, a, b, seed=1):
    """Poisson-Gaussian noise var(z | y) = a y + b on `clean` (any shape, nominally 0..255) from numpy's default_rng(seed):
    a * poisson(clean / a) + normal(0, sqrt(b)); a = 0 gives the Gaussian part alone.  Negative values of `clean` count as 0 for the
    Poisson part.  Returns float32."""
    clean = np.asarray(clean, dtype=np.float64)
    rng = np.random.default_rng(seed)
    z = float(a) * rng.poisson(np.maximum(clean, 0.0) / float(a)) if a > 0 else clean.copy()
    if b > 0:
        z = z + rng.normal(0.0, np.sqrt(float(b)), clean.shape)
    return z.astype(np.float32)


def clip_round(lf, lo=0.0, hi=255.0):
    """What storing `lf` (any shape) in an integer format of range lo..hi does to it: round to the nearest whole number (ties to even),
    then clip to lo..hi (an infinite value goes to its bound; NaN stays).  Returns float32."""
    if not float(lo) < float(hi):
        raise ValueError("clip_round: the range needs lo < hi")
    return np.clip(np.rint(np.asarray(lf, dtype=np.float32)), np.float32(lo), np.float32(hi)).astype(np.float32)


def add_impulse(lf, p, seed=1, kind="salt_pepper"):
    """Impulse noise on `lf` (any shape, nominally 0..255) from numpy's default_rng(seed): every value is hit with probability p and
    replaced -- "salt_pepper": by 0 or 255 with equal probability, "random": by a uniform value of [0, 255), "hot": by 255.  The draws
    are one array of uniforms for the hits, then (not for "hot") one for the values, both of lf's shape.  Returns (damaged float32
    array, boolean hit mask); a hit may leave a value unchanged (a 255 replaced by 255)."""
    lf = np.asarray(lf, dtype=np.float32)
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError("add_impulse: p must lie in [0, 1]")
    rng = np.random.default_rng(seed)
    hit = rng.random(lf.shape) < float(p)
    if kind == "salt_pepper":
        val = np.where(rng.random(lf.shape) < 0.5, np.float32(0.0), np.float32(255.0))
    elif kind == "random":
        val = (rng.random(lf.shape) * 255.0).astype(np.float32)
    elif kind == "hot":
        val = np.float32(255.0)
    else:
        raise ValueError('add_impulse: kind must be "salt_pepper", "random" or "hot"')
    return np.where(hit, val, lf).astype(np.float32), hit


def add_defects(shape, seed=1):
    """Defect map for a light field of `shape` = (A, C, n, n), n >= 17, from numpy's default_rng(seed): per SAI three squares of side
    3..7, one full-height pair of columns and one disc of radius 4 (centre at least 8 from the edges), the same in every channel.  The
    draws per SAI, in this order: for each square its side, row and column; the column pair's first column; the disc's centre (row,
    column) in one call.  Returns a boolean array of `shape`; about 6 % of the values are flagged at n = 64."""
    A, C, H, W = (int(v) for v in shape)
    if H != W or H < 17:
        raise ValueError("add_defects: shape must be (A, C, n, n) with n >= 17")
    n = H
    rng = np.random.default_rng(seed)
    fl = np.zeros((A, 1, n, n), bool)
    yy, xx = np.mgrid[:n, :n]
    for st in range(A):
        for _ in range(3):
            s = rng.integers(3, 8)
            i = rng.integers(0, n - s + 1)
            j = rng.integers(0, n - s + 1)
            fl[st, 0, i:i + s, j:j + s] = True
        j = rng.integers(0, n - 2)
        fl[st, 0, :, j:j + 2] = True
        ci, cj = rng.integers(8, n - 8, 2)
        fl[st, 0][(yy - ci) ** 2 + (xx - cj) ** 2 <= 16] = True
    return np.ascontiguousarray(np.broadcast_to(fl, (A, C, n, n)))


def degrade_sai(lf, st, kind, seed=1):
    """A copy of the light field `lf` ([A][...], nominally 0..255) with the sub-aperture image `st` made bad, from numpy's
    default_rng(seed): "dim": every value times 0.5 (a vignetted or under-exposed view); "noise": every value replaced by a uniform value
    of [0, 255) (a corrupt file, a failed camera); "shift": the view rolled by 7 rows and 5 columns in its last two axes (a view filed
    under the wrong angular position).  lf is [A][C][H][W]; "dim" and "noise" also take [A][C*H*W].  Returns float32."""
    out = np.array(lf, dtype=np.float32, copy=True)
    if kind == "dim":
        out[st] = out[st] * np.float32(0.5)
    elif kind == "noise":
        out[st] = (np.random.default_rng(seed).random(out[st].shape) * 255.0).astype(np.float32)
    elif kind == "shift":
        if out[st].ndim < 2:
            raise ValueError('degrade_sai: "shift" needs the light field as [A][C][H][W]')
        out[st] = np.roll(out[st], (7, 5), axis=(-2, -1))
    else:
        raise ValueError('degrade_sai: kind must be "dim", "noise" or "shift"')
    return out


def vignette_gains(awidth, aheight, edge):
    """The gains of a smooth vignette over the views: g(s, t) = 1 - (1 - edge) rho^2, rho the angular distance of view (s, t) from the
    centre of the aheight x awidth array, normalised to 1 at the corners (so the corner views get `edge`; 3 x 3 at edge 0.6: corners
    0.6, edge views 0.8, centre 1).  float64 [aheight * awidth], s along the first axis (row-major)."""
    if not 0.0 < float(edge) <= 1.0:
        raise ValueError("vignette_gains: edge must be in (0, 1]")
    cs, ct = (aheight - 1) / 2.0, (awidth - 1) / 2.0
    s, t = np.mgrid[0:aheight, 0:awidth]
    corner = cs * cs + ct * ct
    rho2 = ((s - cs) ** 2 + (t - ct) ** 2) / corner if corner else np.zeros((aheight, awidth))
    return (1.0 - (1.0 - float(edge)) * rho2).reshape(-1)


def apply_gains(lf, gains):
    """A copy of the light field `lf` ([A][...]) with view m multiplied by gains[m] (gains [A]), or, with lf as [A][C][...] and gains
    [A][C], channel c of view m by gains[m][c]: one float32 multiplication per value.  Returns float32."""
    out = np.array(lf, dtype=np.float32, copy=True)
    g = np.asarray(gains, np.float64).astype(np.float32)
    if g.shape != out.shape[:g.ndim] or g.ndim not in (1, 2):
        raise ValueError("apply_gains: gains must be [A] or [A][C] like the light field's first axes")
    return out * g.reshape(g.shape + (1,) * (out.ndim - g.ndim))
