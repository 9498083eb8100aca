"""Numpy model of the joint repair (lfbm5d_repair_*, include/lfbm5d_repair.h): the checker of the tests, written from the definition on
top of tests/view_model.py (warp, reflection, hypotheses, source lists) and tests/inpaint_model.py (the onion-peel fill).  Defective
values and missing SAIs are one set of unsound values; the plane sweep skips unsound source values (validity per position), scales the
error of a cell by (n - 1) / (n_d - 1) and the box sum by (2r + 1)^2 / S_k, and fills the unsound values of a target where n_{d*} >=
min_valid; the rim fill takes the rest.  Everything in float32, every operation rounded on its own, sums in a fixed order from +0: the
GPU must equal this bit for bit, in values, codes, disparities and counts.  The loop takes the regulariser as a function."""
import numpy as np

import inpaint_model as IM
import view_model as VM

D_MAX, R_MAX, SRC_MAX = VM.D_MAX, VM.R_MAX, 24
RECIP = VM.RECIP                                                                     # r[k] = (float)(1.0 / k), r[0] = 0


def f_table():
    """f[n][k] = (float)((n - 1) / (k - 1)) computed in double, n, k = 2..24; 0 elsewhere."""
    f = np.zeros((SRC_MAX + 1, SRC_MAX + 1), np.float32)
    for n in range(2, SRC_MAX + 1):
        for k in range(2, SRC_MAX + 1):
            f[n, k] = np.float32(np.float64(n - 1) / np.float64(k - 1))
    return f


def g_table(r):
    """g[k] = (float)((2r + 1)^2 / k) computed in double, k = 1..(2r + 1)^2; g[0] = 0."""
    box = (2 * r + 1) ** 2
    g = np.zeros(box + 1, np.float32)
    for k in range(1, box + 1):
        g[k] = np.float32(np.float64(box) / np.float64(k))
    return g


F = f_table()


def unsound_values(lf, flags, mask, missing, W, H, C):
    """bool [A][C][H][W]: the SAI is missing, the value is flagged or not finite (False on empty SAIs)."""
    A = len(mask)
    x = np.asarray(lf, np.float32).reshape(A, C, H, W)
    u = ~np.isfinite(x)
    if flags is not None:
        u |= np.asarray(flags).reshape(A, C, H, W) != 0
    for q in range(A):
        if missing is not None and missing[q]:
            u[q] = True
        if not mask[q]:
            u[q] = False
    return u


def sources(m, mask, missing, ang_major, aw, ah, ang_radius):
    miss = np.zeros(aw * ah, np.uint32) if missing is None else missing
    return [s for s in VM.sources(m, mask, miss, ang_major, aw, ah, ang_radius) if s[0] != m]


def warp(p, d, ds, dt):
    """plane(s) [..., H, W] warped by hypothesis d towards a target at angular offset (-ds, -dt)"""
    H, W = p.shape[-2:]
    return p[..., VM.reflect(np.arange(H) - d * ds, H), :][..., VM.reflect(np.arange(W) - d * dt, W)]


def cost(x, v, srcs, d, r):
    """(E_d [H][W] with +inf where the box has no evidence, mu_d [C][H][W], n_d [H][W]); x [A][C][H][W] float32, v [A][H][W] bool."""
    C, H, W = x.shape[1:]
    n = len(srcs)
    ys, xs = np.arange(H), np.arange(W)
    w = [warp(x[q], d, ds, dt) for q, ds, dt in srcs]
    a = [warp(v[q], d, ds, dt) for q, ds, dt in srcs]
    nd = np.zeros((H, W), np.int64)
    for aq in a:
        nd += aq
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.zeros((C, H, W), np.float32)
        for wq, aq in zip(w, a):
            S = np.where(aq[None], (S + wq).astype(np.float32), S)
        mu = (S * RECIP[nd][None]).astype(np.float32)
        e = np.zeros((H, W), np.float32)
        for c in range(C):
            for wq, aq in zip(w, a):
                diff = (wq[c] - mu[c]).astype(np.float32)
                e = np.where(aq, (e + (diff * diff).astype(np.float32)).astype(np.float32), e)
        ev = nd >= 2
        es = np.where(ev, (e * F[n][np.minimum(nd, SRC_MAX)]).astype(np.float32), np.float32(0.0)).astype(np.float32)
        h = np.zeros((H, W), np.float32)
        kh = np.zeros((H, W), np.int64)
        for k in range(-r, r + 1):
            cols = VM.reflect(xs + k, W)
            h = (h + es[:, cols]).astype(np.float32)
            kh = kh + ev[:, cols]
        Se = np.zeros((H, W), np.float32)
        Sk = np.zeros((H, W), np.int64)
        for k in range(-r, r + 1):
            rows = VM.reflect(ys + k, H)
            Se = (Se + h[rows, :]).astype(np.float32)
            Sk = Sk + kh[rows, :]
        E = np.where(Sk > 0, (Se * g_table(r)[Sk]).astype(np.float32), np.float32(np.inf)).astype(np.float32)
    return E, mu, nd


def sweep_target(x, v, srcs, D, r):
    """(mu_{d*} [C][H][W], n_{d*} [H][W], d* int8 [H][W]) of one target"""
    best = view = cnt = disp = None
    for d in VM.hypotheses(D):
        E, mu, nd = cost(x, v, srcs, d, r)
        if best is None:
            best, view, cnt, disp = E, mu, nd, np.zeros(E.shape, np.int8)
            continue
        take = E < best                                                    # strictly: ties keep the smaller |d|; +inf never wins
        best = np.where(take, E, best)
        view = np.where(take[None], mu, view)
        cnt = np.where(take, nd, cnt)
        disp = np.where(take, np.int8(d), disp)
    return view, cnt, disp


def fill(lf, flags, mask, missing, ang_major, aw, ah, W, H, C, D=4, r=3, ang_radius=1, min_valid=3, out=None, codes=None, disp=None):
    """lf [asize][C*H*W] float32; flags like lf or None; missing [asize] or None.  out / codes / disp: initial contents of the outputs.
    Returns a dict: out float32 [A][C*H*W], codes uint8 like out, disp int8 [A][H*W], missing, targets, swept, passes, values, flagged,
    unsound / views / rim / left (int64 [3]), positions, hist (int64 [17], index d + 8), sweep / rem (the light field and the flags of what is still unsound after the sweep alone), valid (the planes v_q)."""
    A = aw * ah
    mask = np.asarray(mask)
    x = np.ascontiguousarray(lf, np.float32).reshape(A, C, H, W)
    u = unsound_values(x, flags, mask, missing, W, H, C)
    v = ~u.any(axis=1)
    for q in range(A):
        if not mask[q]:
            v[q] = False
    mid = x.copy()
    rem = u.copy()
    dsp = np.zeros((A, H, W), np.int8) if disp is None else np.array(np.asarray(disp, np.int8).reshape(A, H, W), copy=True)
    hist = np.zeros(2 * D_MAX + 1, np.int64)
    targets = swept = 0
    for m in range(A):
        if not mask[m] or v[m].all():
            continue
        targets += 1
        srcs = sources(m, mask, missing, ang_major, aw, ah, ang_radius)
        if not srcs:
            continue
        swept += 1
        view, cnt, d = sweep_target(x, v, srcs, D, r)
        bad = ~v[m]
        dsp[m] = np.where(bad, d, dsp[m])
        take = bad & (cnt >= min_valid)
        put = u[m] & take[None]
        mid[m].view(np.uint32)[...] = np.where(put, view.view(np.uint32), mid[m].view(np.uint32))
        rem[m] &= ~put
        hist += np.bincount(d[take].astype(np.int64) + D_MAX, minlength=2 * D_MAX + 1)
    if not targets:
        raise ValueError("nothing to repair")
    ir = IM.fill(mid.reshape(A, -1), rem.reshape(A, -1), mask, W, H, C, out=out)
    st = ir["flags"].reshape(A, C, H, W)
    code = np.where(st != 0, st + 1, u.astype(np.uint8)).astype(np.uint8)
    res_codes = code if codes is None else np.array(np.asarray(codes, np.uint8).reshape(A, C, H, W), copy=True)
    for q in range(A):
        if mask[q]:
            res_codes[q] = code[q]
    per = lambda k: np.array([int((code[:, c] == k).sum()) for c in range(C)] + [0] * (3 - C), np.int64)
    nne = int(np.count_nonzero(mask))
    fl = 0 if flags is None else int(((np.asarray(flags).reshape(A, C, H, W) != 0) & (mask != 0)[:, None, None, None]).sum())
    return dict(out=ir["out"], codes=res_codes.reshape(A, -1), disp=dsp.reshape(A, -1), missing=0 if missing is None else int(np.count_nonzero(missing)),
                targets=targets, swept=swept, passes=ir["passes"], values=nne * C * H * W, flagged=fl, unsound=per(1) + per(2) + per(3),
                views=per(1), rim=per(2), left=per(3), positions=int(hist.sum()), hist=hist, sweep=mid.reshape(A, -1), rem=rem.reshape(A, -1).astype(np.uint8),
                valid=v.reshape(A, -1).astype(np.uint8))


sigma_schedule = IM.sigma_schedule
project = IM.project


def loop(y, flags, mask, missing, ang_major, aw, ah, W, H, C, D, r, K, sigma_start, sigma_end, step, sigma_noise=0.0, ang_radius=1,
         min_valid=3):
    """x_0 = fill(y); x_k = f ? step(x_{k-1}, sigma_k) : y with f = code != 0.  step(light field [asize][C*H*W] float32, sigma) -> the
    basic estimate.  Returns (x_K, x_0, the fill's dict)."""
    y = np.ascontiguousarray(y, np.float32).reshape(aw * ah, -1)
    res = fill(y, flags, mask, missing, ang_major, aw, ah, W, H, C, D, r, ang_radius, min_valid)
    if K and res["left"].sum():
        raise ValueError("a value that nothing can fill cannot be refined")
    x = x0 = res["out"]
    for sig in sigma_schedule(K, sigma_start, sigma_end, sigma_noise):
        b = np.asarray(step(x.copy(), sig), np.float32).reshape(x.shape)
        x = project(res["codes"], b, y)
    return x, x0, res


psnr = VM.psnr
psnr_on = IM.psnr_on
