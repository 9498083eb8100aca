"""The cases of the window-schedule kernels' tests: one launch of lfbm5d_debug_window each (tests/test_gpu_window.py runs them, the
model of tests/window_model.py predicts them, tests/test_window_model.py proves on the CPU that each has the edges it is named for).

A case is a namespace: op; bufs (name -> flat host array in the buffer's initial state, or None = NULL pointer); alias (in-place
operands); lst / slot_mask; kw (the scalar fields of lfbm5d_window_debug); edges: the tags of EDGES this case is there for.
Buffers an op writes start as the sentinel SENT -- whatever the op must leave alone (SAIs not in the list, masked-out slots, the slack
between SAIs) must come back as that; the test adds guard words around every buffer.  All sizes are the smallest at which these
kernels can go wrong; the largest buffer is 4.3 MB."""
from types import SimpleNamespace

import numpy as np

import window_model as M

F = np.float32
EMPTY = M.EMPTY
SENT = np.array([0xCAFEF00D], np.uint32).view(F)[0]     # a finite float no case produces
DENORMAL = np.array([1], np.uint32).view(F)[0]          # the smallest denormal
DEN_SPECIALS = np.array([0.0, -0.0, DENORMAL, -3.5, np.inf, np.nan], F)
NUM_SPECIALS = np.array([0.0, DENORMAL, 1e30], F)


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 32))


def values(rng, n):
    """pixel-like values with the colour edges: negative, above 255, zero, minus zero and denormal"""
    v = rng.uniform(-300, 600, n).astype(F)
    v[rng.integers(0, n, max(4, n // 50))] = rng.choice(np.array([0.0, -0.0, DENORMAL, -DENORMAL, 255.5, 1e30, -1e-3], F), max(4, n // 50))
    return v


def den_values(rng, n):
    """aggregation-weight-like values with every special den a kernel may meet, a tenth of the elements"""
    v = rng.uniform(0.5, 40, n).astype(F)
    at = rng.permutation(n)[:max(len(DEN_SPECIALS), n // 10)]
    v[at] = DEN_SPECIALS[np.arange(len(at)) % len(DEN_SPECIALS)]
    return v


def num_values(rng, n):
    v = rng.uniform(-2000, 9000, n).astype(F)
    at = rng.permutation(n)[:max(len(NUM_SPECIALS), n // 10)]
    v[at] = NUM_SPECIALS[np.arange(len(at)) % len(NUM_SPECIALS)]
    return v


def sent(n):
    return np.full(n, SENT, F)


def sai_list(rng, n_slots, n_sai, empties=()):
    """n_slots distinct SAIs of a light field of n_sai in shuffled (non-monotone) order, the highest among them; `empties`: slots left empty"""
    assert n_sai >= n_slots
    st = rng.permutation(n_sai - 1)[:n_slots - 1].tolist() + [n_sai - 1]
    st = np.array(st, np.uint32)[rng.permutation(n_slots)]
    if n_slots > 1 and np.all(np.diff(st.astype(np.int64)) > 0):
        st = st[::-1].copy()
    top = int(np.argmax(st))
    if top in [e % n_slots for e in empties]:   # the highest SAI stays in the list
        keep = next(i for i in range(n_slots) if i not in [e % n_slots for e in empties])
        st[[top, keep]] = st[[keep, top]]
    for e in empties:
        st[e] = EMPTY
    return st


def two_word_mask(rng, n):
    m = (rng.uniform(size=n) < 0.6).astype(np.uint32)
    m[[0, 1]] = 1, 0
    if n > 66:
        m[[64, 65, n - 1]] = 0, 1, 1
    return m


def case(name, op, bufs, edges, alias=None, lst=None, slot_mask=None, **kw):
    return SimpleNamespace(name=name, op=op, bufs=bufs, alias=alias or {}, lst=lst, slot_mask=slot_mask, kw=kw, edges=tuple(edges))


def expected(c):
    return M.run(c.op, c.bufs, alias=c.alias, lst=c.lst, slot_mask=c.slot_mask, **c.kw)


# ---------------------------------------------------------------- the edges, and how a case proves it has one
def _live(c):
    return [int(s) for s in c.lst if s != EMPTY]


def _n_sai_of(c):
    g = c.kw
    img = g["C"] * g["W"] * g["H"]
    lf = [v for k, v in c.bufs.items() if k in ("noisy", "basic", "num", "den", "sub", "out", "noisy_dst") and v is not None]
    return M.n_sais(lf[0], g["lf_stride"], img)


def _has_all(v, specials):
    b = v.view(np.uint32)
    return all((np.isnan(v).any() if np.isnan(s) else (b == np.array([s], F).view(np.uint32)[0]).any()) for s in specials)


def _den_of(c):
    return [c.bufs[n] for n in ("den", "w_den") if c.bufs.get(n) is not None and not np.all(c.bufs[n] == SENT)]   # (the inputs among them)


EDGES = {
    "tile-exact": lambda c: c.op == "window_end" and c.kw["W"] % 64 == 0 and c.kw["H"] % 32 == 0,
    "ragged": lambda c: c.kw["W"] % 64 != 0 and c.kw["H"] % 4 != 0,
    "wide-and-low": lambda c: c.kw["W"] > 128 and c.kw["H"] < 16,
    "count-two-columns": lambda c: c.kw["W"] - c.kw["k"] + 1 == 2,
    "count-ends-on-a-block": lambda c: (c.kw["W"] - c.kw["k"] + 1) % 64 == 0,
    "k-2": lambda c: c.kw["k"] == 2,
    "k-equals-W": lambda c: c.kw["k"] == c.kw["W"],
    "N-1": lambda c: c.kw["N"] == 1,
    "N-7": lambda c: c.kw["N"] == 7,
    "N-16": lambda c: c.kw["N"] == 16,
    "N-equals-W": lambda c: c.kw["N"] == c.kw["W"],
    "N-equals-H": lambda c: c.kw["N"] == c.kw["H"],
    "C-1": lambda c: c.kw["C"] == 1,
    "C-3": lambda c: c.kw["C"] == 3,
    "slots-1": lambda c: len(c.lst) == 1,
    "slots-9": lambda c: len(c.lst) == 9,
    "slots-25": lambda c: len(c.lst) == 25,
    "slots-81": lambda c: len(c.lst if c.lst is not None else c.slot_mask) == 81,
    "list-non-monotone": lambda c: np.any(np.diff(np.array(_live(c))) < 0),
    "list-highest-sai": lambda c: max(_live(c)) == _n_sai_of(c) - 1,
    "empty-front": lambda c: c.lst[0] == EMPTY,
    "empty-middle": lambda c: any(s == EMPTY for s in c.lst[1:-1]),
    "empty-end": lambda c: c.lst[-1] == EMPTY,
    "untouched-sais": lambda c: len(set(_live(c))) < _n_sai_of(c),
    "mask-both-words": lambda c: all(len(set(c.slot_mask[a:b].tolist())) == 2 for a, b in ((0, 64), (64, len(c.slot_mask)))),
    "den-specials": lambda c: all(_has_all(v, DEN_SPECIALS) for v in _den_of(c)) and len(_den_of(c)) > 0,
    "num-specials": lambda c: all(_has_all(c.bufs[n], NUM_SPECIALS) for n in ("num", "w_num") if c.bufs.get(n) is not None and not np.all(c.bufs[n] == SENT)),
    "counters-garbage": lambda c: c.op == "window_begin" and np.all(c.bufs["counters"][:32] != 0),
    "counters-prefilled": lambda c: c.op != "window_begin" and np.all(c.bufs["counters"] != 0),
    "zeros-grid-stride": lambda c: c.kw["n"] > 256 * 256 * 8 and c.kw["n"] % 256 != 0,
    "denoised-grid-stride": lambda c: c.kw["C"] * (c.kw["W"] - c.kw["k"] + 1) * (c.kw["H"] - c.kw["k"] + 1) > 128 * 256,
    "direct-form": lambda c: c.bufs["w_num"] is None and c.bufs["w_den"] is None,
    "sums-form": lambda c: c.bufs["w_num"] is not None and c.bufs["w_den"] is not None,
    "step-1": lambda c: c.bufs["basic"] is None,
    "step-2": lambda c: c.bufs["basic"] is not None,
    "in-place": lambda c: len(c.alias) > 0,
    "no-pilot": lambda c: c.op == "output" and c.bufs["basic"] is None,
    "colour-off": lambda c: c.kw["colour"] == 0,
    "dmask-holes": lambda c: len(set(c.bufs["dmask"].tolist())) == 2,
    "dmask-null": lambda c: c.bufs["dmask"] is None,
    "yuv": lambda c: c.kw["cs"] == M.YUV, "ycbcr": lambda c: c.kw["cs"] == M.YCBCR, "opp": lambda c: c.kw["cs"] == M.OPP,
    "forward": lambda c: c.kw["forward"] == 1, "inverse": lambda c: c.kw["forward"] == 0,
    "colour-values": lambda c: all(f(c.bufs["noisy"]).any() for f in (lambda v: v < 0, lambda v: v > 255, lambda v: v == 0,
                                                                     lambda v: v.view(np.uint32) == 1)),
    "several-blocks": lambda c: c.kw.get("n", c.kw.get("W", 0) * c.kw.get("H", 0)) > 256 and c.kw.get("n", c.kw.get("W", 0) * c.kw.get("H", 0)) % 256 != 0,
    "stride-slack": lambda c: c.kw["lf_stride"] > c.kw["C"] * c.kw["W"] * c.kw["H"],
    "crop-off-differs": lambda c: c.kw["off"] != c.kw["N"],
    "rect-offsets-both": lambda c: min(c.kw[n] for n in ("sx0", "sy0", "dx0", "dy0")) > 0,
    "rect-right-bottom": lambda c: c.kw["dx0"] + c.kw["rw"] == c.kw["W"] and c.kw["dy0"] + c.kw["rh"] == c.kw["H"]
                                   and c.kw["sx0"] + c.kw["rw"] == c.kw["sW"] and c.kw["sy0"] + c.kw["rh"] == c.kw["sH"],
    "rows-top": lambda c: c.kw["sy0"] == 0 and c.kw["rh"] > 0,
    "rows-middle": lambda c: c.kw["sy0"] > 0 and c.kw["sy0"] + c.kw["rh"] < c.kw["sH"],
    "rows-bottom": lambda c: c.kw["rh"] > 0 and c.kw["sy0"] + c.kw["rh"] == c.kw["sH"],
    "rows-none": lambda c: c.kw["rh"] == 0,
    "rows-grid-stride": lambda c: c.kw["rh"] * c.kw["W"] > 256 * min(256, (c.kw["rh"] * c.kw["W"] + 1023) // 1024),
}


# ---------------------------------------------------------------- builders
def light_field(rng, gen, n_sai, img, slack):
    """[n_sai][img + slack]: values in the images, the sentinel in the slack between them"""
    buf = sent(n_sai * (img + slack)).reshape(n_sai, img + slack)
    buf[:, :img] = gen(rng, n_sai * img).reshape(n_sai, img)
    return buf.reshape(-1)[:(n_sai - 1) * (img + slack) + img].copy()


def colour_cases():
    out = []
    for cs, cs_name in ((M.YUV, "yuv"), (M.YCBCR, "ycbcr"), (M.OPP, "opp")):
        for fwd in (1, 0):
            name = f"color-{cs_name}-{'fwd' if fwd else 'inv'}"
            rng = _rng(name)
            W, H, n_sai, slack = 67, 37, 5, 5
            holes = cs != M.YCBCR
            out.append(case(name, "color", dict(noisy=light_field(rng, values, n_sai, 3 * W * H, slack),
                                                dmask=np.array([1, 0, 1, 1, 0], np.uint32) if holes else None),
                            [cs_name, "forward" if fwd else "inverse", "colour-values", "several-blocks", "stride-slack",
                             "dmask-holes" if holes else "dmask-null"],
                            W=W, H=H, C=3, cs=cs, forward=fwd, n_sai=n_sai, lf_stride=3 * W * H + slack))
        for inplace in (1, 0):
            name = f"roundtrip-{cs_name}-{'inplace' if inplace else 'apart'}"
            rng = _rng(name)
            W, H, n_sai = 64, 32, 3
            src = light_field(rng, values, n_sai, 3 * W * H, 0)
            out.append(case(name, "color_roundtrip", dict(noisy=src, out=None if inplace else sent(len(src)),
                                                          dmask=None if inplace else np.array([0, 1, 1], np.uint32)),
                            [cs_name, "in-place" if inplace else "dmask-holes"], alias={"out": "noisy"} if inplace else None,
                            W=W, H=H, C=3, cs=cs, forward=1, n_sai=n_sai, lf_stride=3 * W * H))
    return out


SHAPES = [   # (W, H, C, N) of the padding ops, with the edge each is there for
    (64, 32, 3, 16, ["N-16", "C-3"]), (67, 37, 1, 7, ["N-7", "C-1", "ragged"]), (9, 70, 3, 9, ["N-equals-W"]),
    (130, 9, 1, 9, ["N-equals-H", "wide-and-low"]), (65, 33, 3, 1, ["N-1"]),
]


def padding_cases():
    out = []
    for W, H, C, N, edges in SHAPES:
        name = f"symetrize-{W}x{H}x{C}-N{N}"
        rng = _rng(name)
        out.append(case(name, "symetrize", dict(noisy=values(rng, C * W * H), w_noisy=sent(C * (W + 2 * N) * (H + 2 * N))), edges,
                        W=W, H=H, C=C, N=N))
    for W, H, C, N, off, edges in ((67, 37, 3, 7, 7, ["N-7", "ragged"]), (64, 32, 1, 16, 7, ["crop-off-differs", "C-1"]),
                                   (65, 33, 3, 4, 0, ["crop-off-differs"]), (9, 70, 1, 9, 18, ["crop-off-differs", "N-equals-W"])):
        name = f"crop-{W}x{H}x{C}-N{N}-off{off}"
        rng = _rng(name)
        out.append(case(name, "crop", dict(w_noisy=values(rng, C * (W + 2 * N) * (H + 2 * N)), out=sent(C * W * H)), edges,
                        W=W, H=H, C=C, N=N, off=off))
    return out


MULTI = [   # (slots, SAIs of the light field, empty slots, W, H, C, N, slack of the light field, of the window)
    (1, 3, (), 130, 9, 3, 7, 0, 0, ["slots-1", "wide-and-low", "N-7", "list-highest-sai", "untouched-sais"]),
    (9, 12, (0, 4, 8), 67, 37, 3, 16, 3, 5, ["slots-9", "empty-front", "empty-middle", "empty-end", "ragged", "N-16", "stride-slack",
                                              "list-non-monotone", "list-highest-sai", "untouched-sais"]),
    (25, 30, (7,), 65, 33, 1, 1, 0, 0, ["slots-25", "N-1", "C-1", "list-non-monotone", "list-highest-sai", "empty-middle"]),
    (81, 81, (), 9, 70, 1, 9, 0, 0, ["slots-81", "N-equals-W", "list-non-monotone", "list-highest-sai"]),
    (9, 9, (), 20, 16, 3, 16, 0, 0, ["N-equals-H", "N-16", "C-3"]),
]


def multi_cases():
    out = []
    for n, S, empties, W, H, C, N, sl, sw, edges in MULTI:
        img, imgb = C * W * H, C * (W + 2 * N) * (H + 2 * N)
        name = f"symetrize_multi-{n}of{S}-{W}x{H}x{C}-N{N}"
        rng = _rng(name)
        lst = sai_list(rng, n, S, empties)
        out.append(case(name, "symetrize_multi", dict(noisy=light_field(rng, values, S, img, sl), w_noisy=sent((n - 1) * (imgb + sw) + imgb)),
                        edges, lst=lst, W=W, H=H, C=C, N=N, lf_stride=img + sl, w_stride=imgb + sw))
        name = f"unsymetrize_multi-{n}of{S}-{W}x{H}x{C}-N{N}"
        rng = _rng(name)
        lst = sai_list(rng, n, S, empties)
        out.append(case(name, "unsymetrize_multi", dict(w_noisy=light_field(rng, values, n, imgb, sw), out=sent((S - 1) * (img + sl) + img)),
                        edges, lst=lst, W=W, H=H, C=C, N=N, lf_stride=img + sl, w_stride=imgb + sw))
    return out


def estimate_cases():
    out = []
    rng = _rng("estimate")
    n = 1000
    out.append(case("estimate-1000", "estimate", dict(num=num_values(rng, n), den=den_values(rng, n), sub=num_values(rng, n), est=sent(n)),
                    ["den-specials", "num-specials", "several-blocks"], n=n))
    for C in (3, 1):
        name = f"estimate_multi-81-C{C}"
        rng = _rng(name)
        A, plane = 81, 300
        out.append(case(name, "estimate_multi", dict(w_num=num_values(rng, A * C * plane), w_den=den_values(rng, A * C * plane),
                                                     w_noisy=num_values(rng, A * C * plane), est=sent(A * plane)),
                        ["slots-81", "mask-both-words", "den-specials", "num-specials", f"C-{C}", "several-blocks"],
                        slot_mask=two_word_mask(rng, A), n=plane, C=C, W=1, H=1))
    for holes in (1, 0):
        name = f"estimate_lf-{'holes' if holes else 'all'}"
        rng = _rng(name)
        n, S = 777, 6
        out.append(case(name, "estimate_lf", dict(num=num_values(rng, S * n), den=den_values(rng, S * n), sub=num_values(rng, S * n), out=sent(S * n),
                                                  dmask=np.array([1, 1, 0, 1, 0, 1], np.uint32) if holes else None),
                        ["den-specials", "num-specials", "several-blocks", "dmask-holes" if holes else "dmask-null"], n=n, n_sai=S))
    return out


BEGIN = [   # (slots, SAIs, empties, W, H, C, N, step, sums form, slack of the light field / of the window)
    (9, 12, (0, 4, 8), 67, 37, 3, 7, 2, 1, 3, 5, ["slots-9", "empty-front", "empty-middle", "empty-end", "ragged", "N-7", "C-3", "step-2",
                                                   "sums-form", "stride-slack", "list-non-monotone", "list-highest-sai", "untouched-sais"]),
    (9, 9, (), 64, 32, 3, 16, 1, 1, 0, 0, ["N-16", "step-1", "sums-form"]),
    (9, 10, (3,), 64, 32, 3, 16, 2, 0, 0, 0, ["direct-form", "step-2", "C-3"]),
    (9, 9, (), 67, 37, 1, 7, 1, 0, 0, 0, ["direct-form", "step-1", "C-1"]),
    (1, 2, (), 130, 9, 1, 9, 1, 1, 0, 0, ["slots-1", "N-equals-H", "wide-and-low", "C-1"]),
    (25, 25, (), 9, 70, 3, 9, 2, 1, 0, 0, ["slots-25", "N-equals-W"]),
    (81, 81, (40,), 20, 12, 1, 1, 2, 1, 0, 0, ["slots-81", "N-1", "list-non-monotone"]),
]


def window_begin_cases():
    out = []
    for n, S, empties, W, H, C, N, step, sums, sl, sw, edges in BEGIN:
        img, imgb, planeb = C * W * H, C * (W + 2 * N) * (H + 2 * N), (W + 2 * N) * (H + 2 * N)
        name = f"window_begin-{n}of{S}-{W}x{H}x{C}-N{N}-step{step}-{'sums' if sums else 'direct'}"
        rng = _rng(name)
        wlen = (n - 1) * (imgb + sw) + imgb
        bufs = dict(noisy=light_field(rng, values, S, img, sl), basic=light_field(rng, num_values, S, img, sl) if step == 2 else None,
                    num=light_field(rng, num_values, S, img, sl), den=light_field(rng, den_values, S, img, sl),
                    w_noisy=sent(wlen), w_basic=sent(wlen) if step == 2 else None, w_num=sent(wlen) if sums else None,
                    w_den=sent(wlen) if sums else None, est=sent(n * planeb),
                    counters=rng.integers(1, 1 << 32, 40, dtype=np.uint64).astype(np.uint32))
        out.append(case(name, "window_begin", bufs, edges + ["den-specials", "num-specials", "counters-garbage"], lst=sai_list(rng, n, S, empties),
                        W=W, H=H, C=C, N=N, lf_stride=img + sl, w_stride=imgb + sw))
    return out


END = [   # (slots, SAIs, empties, W, H, C, N, k, sums form, slack of the light field / of the window)
    (9, 9, (), 64, 32, 3, 16, 8, 1, 0, 0, ["tile-exact", "N-16", "sums-form"]),
    (9, 12, (0, 4, 8), 67, 37, 3, 7, 8, 1, 3, 5, ["ragged", "empty-front", "empty-middle", "empty-end", "stride-slack", "list-non-monotone",
                                                   "list-highest-sai", "untouched-sais", "slots-9"]),
    (9, 10, (2,), 67, 37, 3, 7, 8, 0, 0, 0, ["direct-form", "ragged", "C-3"]),
    (1, 1, (), 130, 9, 1, 9, 4, 1, 0, 0, ["wide-and-low", "slots-1", "C-1", "N-equals-H"]),
    (9, 9, (), 9, 70, 3, 9, 8, 1, 0, 0, ["count-two-columns", "N-equals-W"]),
    (9, 9, (), 9, 70, 1, 2, 8, 0, 0, 0, ["count-two-columns", "direct-form", "C-1"]),
    (9, 9, (), 71, 40, 3, 7, 8, 1, 0, 0, ["count-ends-on-a-block"]),
    (9, 9, (), 71, 40, 3, 7, 8, 0, 0, 0, ["count-ends-on-a-block", "direct-form"]),
    (25, 25, (), 65, 33, 1, 1, 2, 1, 0, 0, ["k-2", "slots-25", "N-1"]),
    (9, 9, (), 9, 70, 3, 3, 9, 1, 0, 0, ["k-equals-W"]),
    (81, 81, (80,), 20, 12, 1, 1, 8, 1, 0, 0, ["slots-81", "empty-end"]),
]


def window_end_cases():
    out = []
    for n, S, empties, W, H, C, N, k, sums, sl, sw, edges in END:
        img, imgb = C * W * H, C * (W + 2 * N) * (H + 2 * N)
        name = f"window_end-{n}of{S}-{W}x{H}x{C}-N{N}-k{k}-{'sums' if sums else 'direct'}"
        rng = _rng(name)
        if sums:   # the light field's sums start as the sentinel: only the SAIs of the list may change
            bufs = dict(num=sent((S - 1) * (img + sl) + img), den=sent((S - 1) * (img + sl) + img),
                        w_num=light_field(rng, num_values, n, imgb, sw), w_den=light_field(rng, den_values, n, imgb, sw))
        else:      # the sums are in the light field already and must stay as they are
            bufs = dict(num=light_field(rng, num_values, S, img, sl), den=light_field(rng, den_values, S, img, sl), w_num=None, w_den=None)
        bufs["counters"] = rng.integers(1, 1000, 32).astype(np.uint32)
        out.append(case(name, "window_end", bufs, edges + ["den-specials", "counters-prefilled"], lst=sai_list(rng, n, S, empties),
                        W=W, H=H, C=C, N=N, k=k, lf_stride=img + sl, w_stride=imgb + sw))
    return out


def job_end_cases():
    out = []
    W, H, S = 67, 37, 7
    img = 3 * W * H
    for cs, cs_name, colour, sl in ((M.YUV, "yuv", 1, 0), (M.YCBCR, "ycbcr", 1, 5), (M.OPP, "opp", 1, 0), (M.OPP, "opp", 0, 0)):
        name = f"finalize-{cs_name}-colour{colour}"
        rng = _rng(name)
        lf = lambda gen: light_field(rng, gen, S, img, sl)
        out.append(case(name, "finalize", dict(num=lf(num_values), den=lf(den_values), sub=lf(values), basic=sent((S - 1) * (img + sl) + img)),
                        [cs_name, "den-specials", "num-specials", "list-non-monotone", "list-highest-sai", "untouched-sais", "several-blocks"]
                        + ([] if colour else ["colour-off"]) + (["stride-slack"] if sl else []),
                        lst=sai_list(rng, 4, S), W=W, H=H, C=3, cs=cs, colour=colour, lf_stride=img + sl))
    for cs, cs_name, colour, pilot, inplace in ((M.YUV, "yuv", 1, 1, 1), (M.YCBCR, "ycbcr", 1, 1, 0), (M.OPP, "opp", 1, 0, 0), (M.YCBCR, "ycbcr", 0, 1, 1),
                                                (M.OPP, "opp", 1, 0, 1)):
        name = f"output-{cs_name}-colour{colour}-{'pilot' if pilot else 'nopilot'}-{'inplace' if inplace else 'apart'}"
        rng = _rng(name)
        lf = lambda gen: light_field(rng, gen, S, img, 0)
        bufs = dict(num=lf(num_values), den=lf(den_values), out=sent(S * img), noisy=lf(values), basic=lf(values) if pilot else None)
        alias = {}
        if inplace:
            bufs["noisy_dst"] = None
            alias["noisy_dst"] = "noisy"
            if pilot:
                bufs["sub"] = None
                alias["sub"] = "basic"
            else:
                bufs["sub"] = lf(values)
        else:
            bufs["noisy_dst"], bufs["sub"] = sent(S * img), lf(values)
        out.append(case(name, "output", bufs, [cs_name, "den-specials", "num-specials", "list-non-monotone", "list-highest-sai", "untouched-sais"]
                        + ([] if colour else ["colour-off"]) + ([] if pilot else ["no-pilot"]) + (["in-place"] if inplace else []),
                        alias=alias, lst=sai_list(rng, 4, S), W=W, H=H, C=3, cs=cs, colour=colour, lf_stride=img))
    return out


def count_cases():
    out = []
    rng = _rng("count_zeros")
    n, S = 256 * 256 * 8 + 1000 + 37, 2
    den = rng.uniform(0.5, 40, S * n).astype(F)
    at = rng.permutation(S * n)[:S * n // 7]
    den[at] = DEN_SPECIALS[np.arange(len(at)) % len(DEN_SPECIALS)]
    out.append(case("count_zeros-grid-stride", "count_zeros", dict(den=den, counters=np.array([17, 4000000000], np.uint32)),
                    ["zeros-grid-stride", "den-specials", "counters-prefilled"], n=n, n_sai=S))
    rng = _rng("count_zeros-small")
    out.append(case("count_zeros-small", "count_zeros", dict(den=den_values(rng, 5 * 300), counters=np.arange(1, 6, dtype=np.uint32)),
                    ["den-specials", "counters-prefilled"], n=300, n_sai=5))
    for name, A, W, H, C, N, k, sw, edges in (("count_denoised-grid-stride", 3, 200, 180, 1, 1, 8, 9, ["denoised-grid-stride", "C-1", "N-1"]),
                                              ("count_denoised-81", 81, 20, 12, 3, 7, 8, 0, ["slots-81", "mask-both-words", "C-3", "N-7"]),
                                              ("count_denoised-two-columns", 9, 9, 70, 3, 9, 8, 0, ["count-two-columns", "N-equals-W"]),
                                              ("count_denoised-k-equals-W", 9, 9, 70, 1, 2, 9, 0, ["k-equals-W"]),
                                              ("count_denoised-k2", 9, 65, 33, 3, 16, 2, 0, ["k-2", "count-ends-on-a-block", "N-16"])):
        rng = _rng(name)
        imgb = C * (W + 2 * N) * (H + 2 * N)
        mask = two_word_mask(rng, A) if A == 81 else np.array(([1, 0, 1] * 3)[:A], np.uint32)
        out.append(case(name, "count_denoised", dict(w_den=light_field(rng, den_values, A, imgb, sw), counters=np.array([123456], np.uint32)),
                        edges + ["den-specials", "counters-prefilled"], slot_mask=mask, W=W, H=H, C=C, N=N, k=k, w_stride=imgb + sw))
    return out


def copy_cases():
    out = []
    for name, A, C, sW, sH, W, H, sx0, sy0, dx0, dy0, rw, rh, edges in (
            ("copy_rect-offsets", 9, 3, 40, 30, 50, 45, 7, 5, 11, 13, 20, 17, ["rect-offsets-both", "C-3"]),
            ("copy_rect-right-bottom", 9, 1, 40, 30, 50, 45, 9, 6, 19, 21, 31, 24, ["rect-right-bottom", "rect-offsets-both", "C-1"]),
            ("copy_rect-81", 81, 3, 12, 10, 14, 12, 0, 1, 2, 0, 9, 8, ["slots-81", "mask-both-words"])):
        rng = _rng(name)
        simg, img = C * sW * sH, C * W * H
        mask = two_word_mask(rng, A) if A == 81 else np.array([1, 0, 1, 1, 1, 0, 1, 1, 1], np.uint32)
        out.append(case(name, "copy_rect", dict(w_noisy=values(rng, A * simg), out=sent(A * img)), edges, slot_mask=mask,
                        W=W, H=H, C=C, sW=sW, sH=sH, sx0=sx0, sy0=sy0, dx0=dx0, dy0=dy0, rw=rw, rh=rh, lf_stride=img, w_stride=simg))
    for name, sy0, dy0, rh, edges in (("copy_rows-top", 0, 3, 40, ["rows-top", "rows-grid-stride"]), ("copy_rows-middle", 11, 0, 13, ["rows-middle"]),
                                      ("copy_rows-bottom", 37, 7, 13, ["rows-bottom"]), ("copy_rows-none", 5, 5, 0, ["rows-none"])):
        rng = _rng(name)
        planes, W, sH, H = 6, 77, 50, 60
        out.append(case(name, "copy_rows", dict(w_noisy=values(rng, planes * sH * W), out=sent(planes * H * W)), edges,
                        W=W, H=H, sH=sH, sy0=sy0, dy0=dy0, rh=rh, n_sai=planes))
    return out


def all_cases():
    cases = (colour_cases() + padding_cases() + multi_cases() + estimate_cases() + window_begin_cases() + window_end_cases() + job_end_cases()
             + count_cases() + copy_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases
