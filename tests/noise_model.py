"""float64 numpy model of the blind noise-level statistic (lfbm5d_noise_level_*, include/lfbm5d.h): the checker of the tests,
written from the definition (direct patch Gram matrices), not from the GPU's lag form."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def scatter(img, r):
    """(n, s, M) of one image plane: patches at stride 1 as row-major vectors, M = S - s s^T / n."""
    X = sliding_window_view(np.asarray(img, np.float64), (r, r)).reshape(-1, r * r)
    n = X.shape[0]
    s = X.sum(0)
    return n, s, X.T @ X - np.outer(s, s) / n


def statistic(cov):
    """(sigma, m, eigenvalues ascending): the first m = d, d-1, ... where as many of lambda_1..m lie above their mean as below it."""
    lam = np.sort(np.linalg.eigvalsh(np.asarray(cov, np.float64)))
    for m in range(lam.size, 0, -1):
        mu = lam[:m].mean()
        if (lam[:m] > mu).sum() == (lam[:m] < mu).sum():
            return float(np.sqrt(max(mu, 0.0))), m, lam
    raise AssertionError("unreachable: m = 1 always splits evenly")


def model(lf, mask, W, H, C, r=8, per_sai=False):
    """lf [asize][C*H*W] (any float dtype, read as given); returns a dict like lfbm5d_amd.noise_level's result plus the covariances."""
    lf = np.asarray(lf).reshape(len(mask), C, H, W)
    d = r * r
    Ms = {}
    n = None
    for a in range(len(mask)):
        if mask[a]:
            for c in range(C):
                n, _, Ms[a, c] = scatter(lf[a, c], r)
    sais = sorted({a for a, _ in Ms})
    cov = sum(Ms.values()) / (n * len(Ms))
    cov_ch = [sum(Ms[a, c] for a in sais) / (n * len(sais)) for c in range(C)]
    sigma, m, lam = statistic(cov)
    out = {"sigma": sigma, "components": m, "eigen": lam, "patches": n * len(Ms), "cov": cov,
           "sigma_channel": np.array([statistic(cc)[0] for cc in cov_ch] + [0.0] * (3 - C)), "sigma_sai": None}
    if per_sai:
        out["sigma_sai"] = np.array([statistic(sum(Ms[a, c] for c in range(C)) / (n * C))[0] if mask[a] else 0.0
                                     for a in range(len(mask))])
    return out
