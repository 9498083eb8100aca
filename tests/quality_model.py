"""Float64 numpy model of the quality metrics (lfbm5d_quality_*, include/lfbm5d.h), written from the definition: per SAI the mean
squared error over all C*H*W values, rmse = sqrt(mse), psnr = 10 log10(peak^2 / mse), and the SSIM of Wang, Bovik, Sheikh &
Simoncelli (2004) with the 11 x 11 Gaussian window (sigma 1.5) over every valid position; the summary is the mean and the population
standard deviation over the non-empty SAIs.  The window sum is the plain 121-term 2-D sum, not the separable form the kernel uses."""
import numpy as np

WIN = 11


def window():
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    g /= g.sum()
    return np.outer(g, g)


def _wsum(x, w):
    H, W = x.shape
    out = np.zeros((H - WIN + 1, W - WIN + 1), np.float64)
    for i in range(WIN):
        for j in range(WIN):
            out += w[i, j] * x[i:i + H - WIN + 1, j:j + W - WIN + 1]
    return out


def ssim_map(a, b, peak=255.0):
    """The SSIM map of two planes [H][W]: (H-10) x (W-10) values."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = window()
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    ma, mb = _wsum(a, w), _wsum(b, w)
    sa, sb, sab = _wsum(a * a, w) - ma * ma, _wsum(b * b, w) - mb * mb, _wsum(a * b, w) - ma * mb
    return (2.0 * ma * mb + c1) * (2.0 * sab + c2) / ((ma * ma + mb * mb + c1) * (sa + sb + c2))


def ssim(a, b, C, H, W, peak=255.0):
    """SSIM of one SAI [C*H*W]: the mean of the map over channels and positions."""
    a, b = np.asarray(a).reshape(C, H, W), np.asarray(b).reshape(C, H, W)
    return float(np.mean([ssim_map(a[c], b[c], peak) for c in range(C)]))


def mse(a, b):
    d = np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)
    return float(np.sum(d * d) / d.size)


def psnr_of(m, peak=255.0):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.float64(peak) ** 2 / np.asarray(m, np.float64))


def summary(mse_sai, ssim_sai, mask, peak=255.0):
    on = np.asarray(mask) != 0
    m = np.asarray(mse_sai, np.float64)[on]
    out = {"count": int(on.sum()), "mse": float(m.mean())}
    with np.errstate(invalid="ignore"):
        for name, v in (("psnr", psnr_of(m, peak)), ("rmse", np.sqrt(m)), ("ssim", None if ssim_sai is None else np.asarray(ssim_sai, np.float64)[on])):
            if v is not None:
                out[name + "_mean"] = float(v.mean())
                out[name + "_std"] = float(np.sqrt(np.mean((v - v.mean()) ** 2)))
    return out


def model(ref, test, mask, W, H, C, peak=255.0, want_ssim=True):
    """ref, test [asize][C*H*W] float32 -> dict(mse_sai, psnr_sai, rmse_sai, ssim_sai, and the summary's fields); entries of empty
    SAIs are 0 and their planes are not read."""
    mask = np.asarray(mask)
    A = mask.size
    m, s = np.zeros(A, np.float64), np.zeros(A, np.float64)
    for st in range(A):
        if mask[st]:
            m[st] = mse(ref[st], test[st])
            if want_ssim:
                s[st] = ssim(ref[st], test[st], C, H, W, peak)
    on = mask != 0
    out = summary(m, s if want_ssim else None, mask, peak)
    out.update(mse_sai=m, psnr_sai=np.where(on, psnr_of(np.where(on, m, 1.0), peak), 0.0), rmse_sai=np.sqrt(m), ssim_sai=s if want_ssim else None)
    return out
