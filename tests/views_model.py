"""Numpy model of the per-view noise levels (lfbm5d_views_*, include/lfbm5d_views.h): the checker of the tests, written from the
definition.  A view table holds one sigma per SAI; the sigma of an angular window is the table's value where the window's non-empty
SAIs agree on one, else the root mean square of theirs, summed in ascending window-slot order in float64 and rounded to float32 once.
The library must equal every float this file returns bit for bit."""
import numpy as np

ROWMAJOR, COLMAJOR = 11, 12


def index(s, t, awidth, aheight, ang_major):
    return s * awidth + t if ang_major == ROWMAJOR else s + t * aheight


def coords(st, awidth, aheight, ang_major):
    return (st // awidth, st % awidth) if ang_major == ROWMAJOR else (st % aheight, st // aheight)


def _range(idx, size, an):
    """The 2 an + 1 indices around idx, shifted into 0..size-1."""
    lo = idx - an
    lo += max(0, -lo)
    lo -= max(0, lo + 2 * an - (size - 1))
    return lo


def window_slots(ps, pt, an, awidth, aheight, ang_major):
    """Light-field index of every slot of the window around SAI (ps, pt), in ascending slot order: the slots form a (2 an + 1)^2 grid
    in the light field's own major order."""
    asw = 2 * an + 1
    s0, t0 = _range(ps, aheight, an), _range(pt, awidth, an)
    out = [0] * (asw * asw)
    for si in range(asw):
        for ti in range(asw):
            slot = si * asw + ti if ang_major == ROWMAJOR else si + ti * asw
            out[slot] = index(s0 + si, t0 + ti, awidth, aheight, ang_major)
    return out


def window_sigma(sigma_sai, mask, ps, pt, an, awidth, aheight, ang_major):
    """float32 window sigma; the sum of squares starts at +0 and runs over the non-empty SAIs in slot order."""
    sig = np.asarray(sigma_sai, np.float64)
    vals = [sig[st] for st in window_slots(ps, pt, an, awidth, aheight, ang_major) if mask[st]]
    assert vals and all(np.isfinite(v) and v > 0 for v in vals)
    if all(v == vals[0] for v in vals):
        return np.float32(vals[0])
    acc = np.float64(0.0)
    for v in vals:
        acc = acc + v * v
    return np.float32(np.sqrt(acc / np.float64(len(vals))))


def plan_windows(mask, awidth, aheight, an, ang_major):
    """The processed SAI of every window of a step: the centre SAI first if it is not empty, then always the unprocessed SAI of the
    largest index; a window processes all its non-empty SAIs."""
    asize = awidth * aheight
    proc = [not mask[st] for st in range(asize)]
    cst = index(aheight // 2, awidth // 2, awidth, aheight, ang_major)
    out = []
    first = True
    while not all(proc):
        pst = cst if first and mask[cst] else max(st for st in range(asize) if not proc[st])
        first = False
        ps, pt = coords(pst, awidth, aheight, ang_major)
        for st in window_slots(ps, pt, an, awidth, aheight, ang_major):
            if mask[st]:
                proc[st] = True
        out.append(pst)
    return out


def window_sigmas(sigma_sai, mask, awidth, aheight, an, ang_major):
    """The window sigma of every window of plan_windows, in order (float32)."""
    out = []
    for pst in plan_windows(mask, awidth, aheight, an, ang_major):
        ps, pt = coords(pst, awidth, aheight, ang_major)
        out.append(window_sigma(sigma_sai, mask, ps, pt, an, awidth, aheight, ang_major))
    return np.array(out, np.float32)


def from_gains(sigma, gain, mask):
    """sigma_v = sigma sqrt((sum_c g[v][c]^-2) / C) with the gains as float32 [asize][C], in float64, c ascending from +0; 0 for empty SAIs."""
    g = np.asarray(gain, np.float32).astype(np.float64)
    out = np.zeros(g.shape[0], np.float64)
    for v in range(g.shape[0]):
        if not mask[v]:
            continue
        acc = np.float64(0.0)
        for c in range(g.shape[1]):
            acc = acc + np.float64(1.0) / (g[v, c] * g[v, c])
        out[v] = np.float64(sigma) * np.sqrt(acc / np.float64(g.shape[1]))
    return out


def radial_table(awidth, aheight, sigma, edge, ang_major=ROWMAJOR):
    """sigma / g with the vignette g(s, t) = 1 - (1 - edge) rho^2 of synth.vignette_gains, in the light field's SAI order."""
    cs, ct = (aheight - 1) / 2.0, (awidth - 1) / 2.0
    corner = cs * cs + ct * ct
    out = np.zeros(awidth * aheight, np.float64)
    for s in range(aheight):
        for t in range(awidth):
            rho2 = ((s - cs) ** 2 + (t - ct) ** 2) / corner if corner else 0.0
            out[index(s, t, awidth, aheight, ang_major)] = sigma / (1.0 - (1.0 - edge) * rho2)
    return out
