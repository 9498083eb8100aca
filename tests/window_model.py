"""A model of the window-schedule kernels alone (lfbm5d_amd/csrc/lfbm5d_window.hip), in plain numpy float32: no GPU, no oracle.

Written from the definitions, not from the kernels:
  color()          the three forward and three inverse matrices of utilities.cpp:482-599 as the reference writes them -- every product
                   and every sum rounded to float32 on its own, left to right, zero coefficients multiplied and added like any other
                   (the YUV inverse alone leaves its zero terms out);
  symetrize()      mirror padding: np.pad(mode="symmetric");  crop(): slicing;
  estimate()       num / den in float32 where den != 0, else the substitute (-0.0 takes the substitute, NaN divides);
  coverage()       the (c, i, j) with den > 0 over the (H-k+1) x (W-k+1) patch origins of the unpadded image;
  zeros()          den == 0 over a segment.
run() applies one op of lfbm5d_debug_window (include/lfbm5d.h) to host copies of its buffers, composing the fused ends from those:
window_begin = padding of noisy, basic, num and den + the channel-0 estimate from the padded sums; window_end = the crop of both sums +
the count; finalize = estimate, inverse, forward; output = estimate + the inverse of the result, of basic and of noisy.
tests/test_window_model.py pins the primitives against the CPU oracle; tests/test_gpu_window.py holds the kernels to run()."""
from types import SimpleNamespace

import numpy as np

F = np.float32
EMPTY = 0xFFFFFFFF
YUV, YCBCR, OPP, RGB = 0, 1, 2, 3
COUNTERS = 32                   # partial coverage counters of a window (kWinCounters, lfbm5d_kernels.h)

# (colour space, forward) -> three rows of (coefficient, input channel); None: the operand itself, no product
_ROWS = {
    (YUV, 1): (((0.299, 0), (0.587, 1), (0.114, 2)), ((-0.14713, 0), (-0.28886, 1), (0.436, 2)), ((0.615, 0), (-0.51498, 1), (-0.10001, 2))),
    (YUV, 0): (((None, 0), (1.13983, 2)), ((None, 0), (-0.39465, 1), (-0.5806, 2)), ((None, 0), (2.03211, 1))),
    (YCBCR, 1): (((0.299, 0), (0.587, 1), (0.114, 2)), ((-0.169, 0), (-0.331, 1), (0.500, 2)), ((0.500, 0), (-0.419, 1), (-0.081, 2))),
    (YCBCR, 0): (((1.000, 0), (0.000, 1), (1.402, 2)), ((1.000, 0), (-0.344, 1), (-0.714, 2)), ((1.000, 0), (1.772, 1), (0.000, 2))),
    (OPP, 1): (((0.333, 0), (0.333, 1), (0.333, 2)), ((0.500, 0), (0.000, 1), (-0.500, 2)), ((0.250, 0), (-0.500, 1), (0.250, 2))),
    (OPP, 0): (((1.0, 0), (1.0, 1), (0.666, 2)), ((1.0, 0), (0.0, 1), (-1.333, 2)), ((1.0, 0), (-1.0, 1), (0.666, 2))),
}


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays; two NaNs count as equal (agg_model.same_bits has the reason)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def color(img, cs, forward):
    """img float32 [3][...]: the colour transform of every pixel.  a - m x is a + (-m) x in IEEE arithmetic, so signed coefficients
    and sums alone describe the reference's expressions."""
    img = np.asarray(img, F)
    out = np.empty_like(img)
    with np.errstate(all="ignore"):
        for r, row in enumerate(_ROWS[(int(cs), 1 if forward else 0)]):
            acc = None
            for m, ch in row:
                term = img[ch] if m is None else F(m) * img[ch]
                acc = term if acc is None else acc + term
            out[r] = acc
    assert out.dtype == F
    return out


def symetrize(img, N):
    """img [C][H][W] -> [C][H + 2 N][W + 2 N] (symetrize, utilities.cpp:215-263; defined for N <= W, N <= H)"""
    C, H, W = img.shape
    assert N <= W and N <= H
    return np.pad(img, ((0, 0), (N, N), (N, N)), mode="symmetric")


def crop(sym, W, H, off):
    return sym[:, off:off + H, off:off + W]


def estimate(num, den, sub):
    with np.errstate(all="ignore"):
        return np.where(den != 0, np.asarray(num, F) / np.where(den != 0, den, F(1)), sub).astype(F)


def coverage(den, k):
    """den [C][H][W] of the unpadded image: LF_denoised_percent's numerator (utilities_LF.cpp:985-992) for one SAI"""
    C, H, W = den.shape
    with np.errstate(invalid="ignore"):
        return int((den[:, :H - k + 1, :W - k + 1] > 0).sum())


def zeros(seg):
    return int((seg == 0).sum())


def n_sais(buf, stride, img):
    return (len(buf) - img) // stride + 1


def run(op, bufs, alias=None, lst=None, slot_mask=None, **kw):
    """One op on host copies of its buffers.  bufs: name -> flat array (or None); alias: name -> the buffer it shares (in-place
    operands); kw: the scalar fields.  Returns name -> the expected contents of every buffer the op writes; for window_end and the two
    counting ops `counters` is the amount the op must ADD (a number for window_end, whose spread over the 32 words is free; an
    array per word else)."""
    alias = alias or {}
    g = SimpleNamespace(**kw)
    res = {}

    def rd(name):
        return bufs.get(alias.get(name, name))

    def wr(name):
        name = alias.get(name, name)
        if name not in res:
            res[name] = bufs[name].copy()
        return res[name]

    def sai(buf, st, shape, stride):
        n = int(np.prod(shape))
        return buf[st * stride:st * stride + n].reshape(shape)

    mask = None if rd("dmask") is None else rd("dmask")
    live = lambda s: mask is None or mask[s] != 0
    if op in ("color", "color_roundtrip"):
        src, shape = rd("noisy"), (3, g.H * g.W)
        new = []
        for s in range(g.n_sai):
            v = sai(src, s, shape, g.lf_stride)
            new.append(color(v, g.cs, g.forward) if op == "color" else color(color(v, g.cs, 0), g.cs, 1))
        dst = wr("noisy" if op == "color" else "out")
        for s in range(g.n_sai):
            if live(s):
                sai(dst, s, shape, g.lf_stride)[...] = new[s]
    elif op == "symetrize":
        wr("w_noisy")[:g.C * (g.H + 2 * g.N) * (g.W + 2 * g.N)] = symetrize(sai(rd("noisy"), 0, (g.C, g.H, g.W), 0), g.N).ravel()
    elif op == "crop":
        sym = sai(rd("w_noisy"), 0, (g.C, g.H + 2 * g.N, g.W + 2 * g.N), 0)
        wr("out")[:g.C * g.H * g.W] = crop(sym, g.W, g.H, g.off).ravel()
    elif op == "symetrize_multi":
        dst = wr("w_noisy")
        for i, st in enumerate(lst):
            if st != EMPTY:
                sai(dst, i, (g.C, g.H + 2 * g.N, g.W + 2 * g.N), g.w_stride)[...] = symetrize(sai(rd("noisy"), st, (g.C, g.H, g.W), g.lf_stride), g.N)
    elif op == "unsymetrize_multi":
        dst = wr("out")
        for i, st in enumerate(lst):
            if st != EMPTY:
                sai(dst, st, (g.C, g.H, g.W), g.lf_stride)[...] = crop(sai(rd("w_noisy"), i, (g.C, g.H + 2 * g.N, g.W + 2 * g.N), g.w_stride), g.W, g.H, g.N)
    elif op == "estimate":
        wr("est")[:g.n] = estimate(rd("num")[:g.n], rd("den")[:g.n], rd("sub")[:g.n])
    elif op == "estimate_multi":
        dst = wr("est")
        for i, on in enumerate(slot_mask):
            if on:
                ch0 = lambda name: sai(rd(name), i, (g.C, g.n), g.C * g.n)[0]
                dst[i * g.n:(i + 1) * g.n] = estimate(ch0("w_num"), ch0("w_den"), ch0("w_noisy"))
    elif op == "estimate_lf":
        new = [estimate(*(rd(name)[s * g.n:(s + 1) * g.n] for name in ("num", "den", "sub"))) for s in range(g.n_sai)]
        dst = wr("out")
        for s in range(g.n_sai):
            if live(s):
                dst[s * g.n:(s + 1) * g.n] = new[s]
    elif op == "window_begin":
        lf, win, planeb = (g.C, g.H, g.W), (g.C, g.H + 2 * g.N, g.W + 2 * g.N), (g.H + 2 * g.N) * (g.W + 2 * g.N)
        sums = rd("w_num") is not None
        est = wr("est")
        for i, st in enumerate(lst):
            if st == EMPTY:
                continue
            pad = {name: symetrize(sai(rd(name), st, lf, g.lf_stride), g.N) for name in ("noisy", "basic", "num", "den") if rd(name) is not None}
            for name in pad:
                if name in ("noisy", "basic") or sums:
                    sai(wr("w_" + name), i, win, g.w_stride)[...] = pad[name]
            est[i * planeb:(i + 1) * planeb] = estimate(pad["num"][0], pad["den"][0], pad["basic" if "basic" in pad else "noisy"][0]).ravel()
        wr("counters")[:COUNTERS] = 0
    elif op == "window_end":
        lf, win = (g.C, g.H, g.W), (g.C, g.H + 2 * g.N, g.W + 2 * g.N)
        sums = rd("w_num") is not None
        count = 0
        for i, st in enumerate(lst):
            if st == EMPTY:
                continue
            if sums:
                for name in ("num", "den"):
                    sai(wr(name), st, lf, g.lf_stride)[...] = crop(sai(rd("w_" + name), i, win, g.w_stride), g.W, g.H, g.N)
                count += coverage(crop(sai(rd("w_den"), i, win, g.w_stride), g.W, g.H, g.N), g.k)
            else:
                count += coverage(sai(rd("den"), st, lf, g.lf_stride), g.k)
        res["counters"] = count
    elif op in ("finalize", "output"):
        shape = (3, g.H * g.W)
        v = lambda name, st: sai(rd(name), st, shape, g.lf_stride)
        inv = lambda x: color(x, g.cs, 0) if g.colour else np.array(x, F)
        new = {}
        for st in lst:   # (in-place operands are read before anything is written; every SAI stands alone)
            e = estimate(v("num", st), v("den", st), v("sub", st))
            if op == "finalize":
                new[st] = {"basic": color(inv(e), g.cs, 1) if g.colour else e}
            else:
                new[st] = {"out": inv(e), "noisy_dst": inv(v("noisy", st))}
                if rd("basic") is not None:
                    new[st]["basic"] = inv(v("basic", st))
        for st, d in new.items():
            for name, val in d.items():
                sai(wr(name), st, shape, g.lf_stride)[...] = val
    elif op == "count_zeros":
        res["counters"] = np.array([zeros(rd("den")[s * g.n:(s + 1) * g.n]) for s in range(g.n_sai)], np.uint32)
    elif op == "count_denoised":
        win = (g.C, g.H + 2 * g.N, g.W + 2 * g.N)
        res["counters"] = np.array([sum(coverage(crop(sai(rd("w_den"), i, win, g.w_stride), g.W, g.H, g.N), g.k)
                                        for i, on in enumerate(slot_mask) if on)], np.uint32)
    elif op == "copy_rect":
        dst = wr("out")
        for i, on in enumerate(slot_mask):
            if on:
                s = sai(rd("w_noisy"), i, (g.C, g.sH, g.sW), g.w_stride)
                sai(dst, i, (g.C, g.H, g.W), g.lf_stride)[:, g.dy0:g.dy0 + g.rh, g.dx0:g.dx0 + g.rw] = s[:, g.sy0:g.sy0 + g.rh, g.sx0:g.sx0 + g.rw]
    elif op == "copy_rows":
        s = rd("w_noisy")[:g.n_sai * g.sH * g.W].reshape(g.n_sai, g.sH, g.W)
        wr("out")[:g.n_sai * g.H * g.W].reshape(g.n_sai, g.H, g.W)[:, g.dy0:g.dy0 + g.rh] = s[:, g.sy0:g.sy0 + g.rh]
    else:
        raise ValueError(op)
    return res
