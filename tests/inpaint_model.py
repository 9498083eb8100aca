"""Numpy model of the defect inpainting (lfbm5d_inpaint_*, include/lfbm5d.h): the checker of the tests, written from the definition.
The fill in float32 (sums of the unflagged neighbours in raster order from +0, one product with the table entry (float)(1 / n)), Jacobi
passes on whole planes; the projection is a selection; the loop takes the regulariser as a function.  The GPU must equal the fill and
the projection bit for bit."""
import numpy as np

OFFS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]      # raster order of the 3 x 3, centre skipped
RECIP = np.array([0.0] + [1.0 / n for n in range(1, 9)], np.float64).astype(np.float32)


def neighbours(I):
    """[8][H][W]: the eight neighbours of every value of the plane I, mirrored without repeating the edge (-1 -> 1, W -> W - 2)."""
    H, W = I.shape
    P = np.pad(I, 1, mode="reflect")
    return np.stack([P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in OFFS])


def fill_plane(I, flagged):
    """(out float32, code uint8, passes) of one plane under the boolean map: onion peel, a non-finite value counts as flagged."""
    v = np.array(I, np.float32, copy=True)
    st = np.asarray(flagged, bool) | ~np.isfinite(v)
    code = np.zeros(v.shape, np.uint8)
    passes = t = 0
    while st.any():
        t += 1
        q, ok = neighbours(v), ~neighbours(st)
        n = ok.sum(axis=0)
        s = np.zeros(v.shape, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(8):
                s = np.where(ok[i], s + q[i], s).astype(np.float32)
            new = (s * RECIP[n]).astype(np.float32)
        fillable = st & (n > 0)
        if not fillable.any():
            break
        v = np.where(fillable, new, v)
        st &= ~fillable
        code[fillable] = 1
        passes = t
    code[st] = 2
    return v, code, passes


def fill(lf, flags, mask, W, H, C, out=None, codes=None):
    """lf [asize][C*H*W] float32, flags of that shape (non-zero = defective).  out / codes: initial contents of the outputs (planes of
    empty SAIs keep them).  Returns a dict: out float32, flags uint8 (codes), flagged / filled / left per channel, pixels, passes."""
    A = len(mask)
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    f = np.asarray(flags).reshape(A, C, H, W) != 0
    res_out = np.array(x if out is None else np.asarray(out, np.float32).reshape(A, C, H, W), np.float32, copy=True)
    res_code = np.zeros((A, C, H, W), np.uint8) if codes is None else np.array(np.asarray(codes, np.uint8).reshape(A, C, H, W), copy=True)
    filled, left = np.zeros(C, np.int64), np.zeros(C, np.int64)
    passes = 0
    for st in range(A):
        if not mask[st]:
            continue
        for c in range(C):
            v, code, p = fill_plane(x[st, c], f[st, c])
            res_out[st, c].view(np.uint32)[...] = np.where(code == 1, v.view(np.uint32), x[st, c].view(np.uint32))   # on the bits
            res_code[st, c] = code
            filled[c] += int((code == 1).sum())
            left[c] += int((code == 2).sum())
            passes = max(passes, p)
    return dict(out=res_out.reshape(A, -1), flags=res_code.reshape(A, -1), flagged=filled + left, filled=filled, left=left,
                pixels=int(np.count_nonzero(mask)) * C * H * W, passes=passes)


def project(flags, x, y):
    """out = flag ? x : y, on the bits."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return np.where(np.asarray(flags) != 0, x.view(np.uint32), y.view(np.uint32)).view(np.float32)


def sigma_schedule(K, sigma_start, sigma_end, sigma_noise=0.0):
    s0, s1, sn = float(np.float32(sigma_start)), float(np.float32(sigma_end)), float(np.float32(sigma_noise))
    return [max(s0 if K == 1 else s0 * (s1 / s0) ** ((k - 1) / (K - 1)), sn) for k in range(1, K + 1)]


def loop(y, flags, mask, W, H, C, K, sigma_start, sigma_end, step, sigma_noise=0.0):
    """x_0 = fill(y, f); x_k = f ? step(x_{k-1}, sigma_k) : y.  step(light field [asize][C*H*W] float32, sigma) -> the basic estimate.
    Returns (x_K, x_0, the fill's dict)."""
    r = fill(y, flags, mask, W, H, C)
    if K and r["left"].sum():
        raise ValueError("a plane without one sound value cannot be refined")
    x = x0 = r["out"]
    for sig in sigma_schedule(K, sigma_start, sigma_end, sigma_noise):
        b = np.asarray(step(x.copy(), sig), np.float32).reshape(x.shape)
        x = project(r["flags"], b, y)
    return x, x0, r


def chebyshev_depth(flagged):
    """The largest Chebyshev distance of a flagged value of the boolean plane to the nearest unflagged one (0: nothing flagged;
    None: nothing unflagged), by erosion with the 3 x 3."""
    st = np.asarray(flagged, bool).copy()
    if st.all():
        return None
    d = 0
    while st.any():
        st = st & neighbours(st).all(axis=0)      # survives a pass: no unflagged neighbour
        d += 1
    return d


def psnr_on(a, b, where):
    """PSNR over the values selected by `where`."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(10.0 * np.log10(255.0 ** 2 / ((a - b)[where] ** 2).mean()))


def psnr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(10.0 * np.log10(255.0 ** 2 / ((a - b) ** 2).mean()))
