"""CPU model of the guard band of the fast hard-thresholding chain (k_group_id_haar_fast, lfbm5d_group_ht.hip).

The fast chain runs the 3x3 angular DCT and the Haar fibre transform unnormalised and compares with rescaled thresholds Tq; a wave
in which a coefficient comes within the guard band Gq of its threshold hands its (group, channel) to the reference-order list
launch.  The guarantee -- every decision is the reference-order form's -- holds only if Gq is wider than the float difference of
the two forms wherever they decide differently.  That difference is absolute (round-off of sums of up to 72 pixel values, and of
the cos3 / cn4 constants), so the band has a relative part and an absolute floor:

    Gq = Tq * max(ht_guard(st), K[c][st] * M),   K[c][st] = max over l of kHtGuardAbs[st][l] / Tq[c][st][l]

with M the largest |value| of the lane's NS * 9 inputs, i.e. Gq >= kHtGuardAbs[st][l] * M at every Haar level l.  This file models
both forms in float32, one lane = one pixel of all NS * 9 patches, 64 lanes a wave, and checks on adversarial inputs (the golden
light field at sigma 0.5 ... 50, 16x and 256x its range, a bright low-contrast window, the signed opponent channels U and V,
N = 1 ... 8, thresholds placed on a coefficient) that every decision where the forms differ lies in a wave the guard flags.  The
reference-order form is evaluated with and without multiply-add contraction (the compiler's choice is not pinned).  The guard
constants are read from the kernel sources, so the model cannot drift from them."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lfbm5d_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
F32 = np.float32
LAMBDA = F32(2.7)
LANES = 64


def kernel_guard_constants():
    """(relative band per angular frequency, absolute floor per angular frequency) as the kernel sources define them"""
    src = open(os.path.join(CSRC, "lfbm5d_group_ht.hip")).read()
    m = re.search(r"float ht_guard\(int st\)\s*\{\s*return st == 0 \? 1\.0f / (\d+)\.0f : \(st == 3 \|\| st == 6\) \? 1\.0f / (\d+)\.0f : "
                  r"1\.0f / (\d+)\.0f;", src)
    assert m, "ht_guard definition not found in lfbm5d_group_ht.hip"
    r0, r36, r = (1.0 / float(x) for x in m.groups())
    rel = np.array([r0, r, r, r36, r, r, r36, r, r], np.float32)
    hdr = open(os.path.join(CSRC, "lfbm5d_kernels.h")).read()
    m = re.search(r"constexpr float kHtGuardAbs\[9\]\[4\]\s*=\s*\{(.*?)\};", hdr, flags=re.S)
    if not m:   # (a kernel without an absolute floor)
        return rel, np.zeros((9, 4), np.float32)
    vals = [float(v.rstrip("f")) for v in re.findall(r"[0-9.]+e-?[0-9]+f?|[0-9.]+f?", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))]
    assert len(vals) == 36, vals
    return rel, np.array(vals, np.float32).reshape(9, 4)


def tables():
    """cos3, cn4 and F = ht3_f as build_tables (lfbm5d_pass.hip) computes them for a 3x3 window"""
    kSqrt2Inv = 0.7071067811865475
    c4 = F32(0.5) / (F32(np.sqrt(F32(3))) * F32(np.sqrt(F32(3))))
    cn4 = np.zeros(9, np.float32)
    for i in range(3):
        for j in range(3):
            cn4[i * 3 + j] = F32(F32(0.5) * c4) if i == 0 and j == 0 else (F32(kSqrt2Inv * float(c4)) if i * j == 0 else c4)
    cos3 = np.array([np.cos(np.pi * (j + 0.5) * u / 3.0) for u in range(3) for j in range(3)], np.float32)
    r3 = np.sqrt(3.0)
    alpha = (2.0, r3, 1.0)
    F = np.array([alpha[v] * alpha[u] * float(cn4[v * 3 + u]) for v in range(3) for u in range(3)], np.float32)
    return cos3, cn4, F


COS3, CN4, FF = tables()


def sigma_table(sigma, C):
    """channel sigma of the opponent colour space (sigma_table, lfbm5d_pass.hip)"""
    s = F32(sigma)
    if C == 1:
        return np.array([s], np.float32)
    q = F32(0.333)
    return np.array([F32(np.sqrt(q * q + q * q + q * q)) * s, F32(np.sqrt(F32(0.5) * F32(0.5) + F32(0.5) * F32(0.5))) * s,
                     F32(np.sqrt(F32(0.25) * F32(0.25) + F32(0.5) * F32(0.5) + F32(0.25) * F32(0.25))) * s], np.float32)


def thresholds(sig_c):
    """T (float, the kernels' expression) and Tq[st][l] = T / (F[st] 2^(-l/2)) in double rounded to float (run_pass); sig_c: [...]"""
    T = (LAMBDA * np.asarray(sig_c, np.float32)).astype(np.float32) * F32(1.41421356237309505)
    Tq = (T.astype(np.float64)[..., None, None] / (FF.astype(np.float64)[:, None] * 2.0 ** (-0.5 * np.arange(4)))).astype(np.float32)
    return T.astype(np.float32), Tq


def guard_K(Tq, gabs):
    """K[st] = max over l of gabs[st][l] / Tq[st][l] (run_pass, in double), rounded up to float"""
    k = (gabs.astype(np.float64) / Tq.astype(np.float64)).max(axis=-1)
    return np.nextafter(k.astype(np.float32), np.float32(np.inf))


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def haar_levels(P, NS, fwd_pair):
    """the Haar butterflies over the NS patches in the kernels' pair layout P[h] = {patch h, patch h + NS/2}: list of (coefficient, level)"""
    if NS == 1:
        return [(P[0], 0)]
    if NS == 2:
        s, d = fwd_pair(P[0][0], P[0][1])
        return [(s, 1), (d, 1)]
    if NS == 4:
        S = fwd_pair(P[0], P[1])           # {p0 + p1, p2 + p3}, {p0 - p1, p2 - p3}
        s, d = fwd_pair(S[0][0], S[0][1])
        return [(s, 2), (d, 2), (S[1][0], 1), (S[1][1], 1)]
    S01, D01 = fwd_pair(P[0], P[1])
    S23, D23 = fwd_pair(P[2], P[3])
    SS, DD = fwd_pair(S01, S23)
    s, d = fwd_pair(SS[0], SS[1])
    return [(s, 3), (d, 3), (DD[0], 2), (DD[1], 2), (D01[0], 1), (D01[1], 1), (D23[0], 1), (D23[1], 1)]


def pairs(x, NS):
    """x [..., NS, 9] -> the pair layout: P[h] = (patch h, patch h + NS/2) as a tuple of two [..., 9] arrays"""
    if NS == 1:
        return [x[..., 0, :]]
    h = NS // 2
    return [(x[..., i, :], x[..., i + h, :]) for i in range(h)]


def fast_fwd(x, NS):
    """group_id_compute_fast: unnormalised 3x3 (rows along u, then columns along s) and Haar by sums and differences"""
    y = np.empty_like(x)
    t = np.empty_like(x)
    for s in range(3):
        a, b, c = x[..., s * 3], x[..., s * 3 + 1], x[..., s * 3 + 2]
        p = a + c
        t[..., s * 3], t[..., s * 3 + 1], t[..., s * 3 + 2] = p + b, a - c, p - F32(2) * b
    for u in range(3):
        a, b, c = t[..., u], t[..., 3 + u], t[..., 6 + u]
        p = a + c
        y[..., u], y[..., 3 + u], y[..., 6 + u] = p + b, a - c, p - F32(2) * b

    def fp(P0, P1):
        if isinstance(P0, tuple):
            return (P0[0] + P1[0], P0[1] + P1[1]), (P0[0] - P1[0], P0[1] - P1[1])
        return P0 + P1, P0 - P1
    return haar_levels(pairs(y, NS), NS, fp)


def ref_fwd(x, NS, contract):
    """dct9_fwd2 then haar_fwd_pairs (lfbm5d_group_device.h): the reference's operation order, normalised"""
    c3, cn = COS3, CN4

    def dot3(a0, b0, a1, b1, a2, b2):
        if contract:   # ((a0 b0 + a1 b1) + a2 b2) with both additions fused: fma(a2, b2, fma(a0, b0, a1 b1))
            return fma(a2, np.float32(b2), fma(a0, np.float32(b0), a1 * b1))
        return (a0 * b0 + a1 * b1) + a2 * b2
    t = np.empty_like(x)
    y = np.empty_like(x)
    for s in range(3):
        for u in range(3):
            t[..., s * 3 + u] = F32(2) * dot3(x[..., s * 3], c3[u * 3], x[..., s * 3 + 1], c3[u * 3 + 1], x[..., s * 3 + 2], c3[u * 3 + 2])
    for v in range(3):
        for u in range(3):
            y[..., v * 3 + u] = (F32(2) * dot3(t[..., u], c3[v * 3], t[..., 3 + u], c3[v * 3 + 1], t[..., 6 + u], c3[v * 3 + 2])) * cn[v * 3 + u]
    s_ = F32(0.70710678118654752)

    def fp(P0, P1):
        if isinstance(P0, tuple):
            return ((P0[0] + P1[0]) * s_, (P0[1] + P1[1]) * s_), ((P0[0] - P1[0]) * s_, (P0[1] - P1[1]) * s_)
        return (P0 + P1) * s_, (P0 - P1) * s_
    return haar_levels(pairs(y, NS), NS, fp)


def evaluate(x, NS, T, Tq, rel, gabs):
    """x [waves, 64, NS, 9] float32 inputs of one channel; T [waves], Tq [waves, 9, 4].  Returns (decisions that differ, of them in
    waves the guard does not flag, the same with the relative band alone, max (form difference - half the relative band) / M per
    (st, l), flagged waves)"""
    W = x.shape[0]
    M = np.abs(x).reshape(W, LANES, -1).max(axis=-1)                           # [waves, lanes]
    K = guard_K(Tq, gabs)                                                     # [waves, 9]
    gs = np.maximum(rel, K[:, None, :] * M[..., None]).astype(np.float32)     # [waves, lanes, 9]
    cf = fast_fwd(x, NS)
    flag_new = np.zeros(W, bool)
    flag_old = np.zeros(W, bool)
    differ = np.zeros(W, np.int64)
    ratio = np.zeros((9, 4))
    Tw = T[:, None, None]
    for contract in (False, True):
        cr = ref_fwd(x, NS, contract)
        for (a, l), (b, _) in zip(cf, cr):
            tq = Tq[:, None, :, l]                                                # [waves, 1, 9]
            ax, bx = np.abs(a), np.abs(b)
            kf, kr = ax > tq, bx > Tw
            dist = np.abs(ax - tq)
            if not contract:
                flag_old |= (dist < tq * rel).any(axis=(1, 2))
                flag_new |= (dist < tq * gs).any(axis=(1, 2))
            differ += (kf != kr).sum(axis=(1, 2))
            # the form difference in the fast chain's units (the rounding of Tq itself is the relative band's business)
            d = np.abs(ax.astype(np.float64) - bx.astype(np.float64) / (FF.astype(np.float64) * 2.0 ** (-0.5 * l)))
            # what the relative band does not cover near a threshold: Gq = max(Tq rel, K Tq M) >= (rel / 2) |c| + (gabs / 2) M
            # at |c| ~ Tq, so half of each suffices, and gabs[st][l] >= 2 max(d - (rel / 2) |c|) / M keeps the guard sound
            d = np.maximum(d - 0.5 * rel.astype(np.float64) * ax, 0.0)
            ratio[:, l] = np.maximum(ratio[:, l], (d / np.maximum(M, 1e-30)[..., None]).max(axis=(0, 1)))
    bad = differ > 0
    return int(differ.sum()), int((bad & ~flag_new).sum()), int((bad & ~flag_old).sum()), ratio, int(flag_new.sum())


def golden_channels(scale, offset, sigma, rng, grey):
    """the golden light field as x * scale + offset plus N(0, sigma) noise, opponent-transformed (or its red plane for grey):
    [9][C][256][256] float32 and the channel sigmas"""
    lf = np.load(GOLDEN).astype(np.float32)
    lf = lf * F32(scale) + F32(offset)
    if grey:
        lf = lf[:, :1]
    lf = lf + rng.standard_normal(lf.shape).astype(np.float32) * F32(sigma)
    if grey:
        return lf, sigma_table(sigma, 1)
    R, G, B = lf[:, 0], lf[:, 1], lf[:, 2]
    q = F32(0.333)
    opp = np.stack([q * R + q * G + q * B, F32(0.5) * R + F32(0.0) * G - F32(0.5) * B, F32(0.25) * R - F32(0.5) * G + F32(0.25) * B], axis=1)
    return opp.astype(np.float32), sigma_table(sigma, 3)


def waves(img, c, NS, n, rng):
    """n waves of 64 lanes (one 8x8 patch), NS patches at offsets of +-6 pixels around a random point, all 9 SAIs at the same
    position: [n, 64, NS, 9]"""
    H, W = img.shape[2], img.shape[3]
    y0 = rng.integers(8, H - 16, n)
    x0 = rng.integers(8, W - 16, n)
    dy = rng.integers(-6, 7, (n, NS))
    dx = rng.integers(-6, 7, (n, NS))
    dy[:, 0] = 0
    dx[:, 0] = 0
    ly, lx = np.divmod(np.arange(LANES), 8)
    yy = (y0[:, None, None] + dy[:, None, :] + ly[None, :, None])             # [n, 64, NS]
    xx = (x0[:, None, None] + dx[:, None, :] + lx[None, :, None])
    plane = img[:, c]                                                        # [9, H, W]
    return np.ascontiguousarray(np.moveaxis(plane[:, yy, xx], 0, -1))        # [n, 64, NS, 9]


def on_threshold(x, NS, rng, lo, hi):
    """per wave a threshold placed ON one of its coefficients (reference form, double): the channel sigma that puts T at |c| for a
    random coefficient whose normalised value lies in [lo, hi) times the lane's M -- the decisions the band exists for"""
    W = x.shape[0]
    cr = ref_fwd(x.astype(np.float32), NS, False)
    M = np.abs(x).reshape(W, LANES, -1).max(axis=-1)
    sig = np.empty(W, np.float32)
    for w in range(W):
        i = rng.integers(len(cr))
        c = np.abs(cr[i][0][w].astype(np.float64))                              # [64, 9]
        ok = (c >= lo * M[w][:, None]) & (c < hi * M[w][:, None])
        cand = c[ok] if ok.any() else c.reshape(-1)
        sig[w] = np.float32(cand[rng.integers(len(cand))] / (float(LAMBDA) * np.sqrt(2.0)))
    return np.maximum(sig, np.float32(1e-3))


# name, scale, offset, user sigma, grey, N values, waves per (channel, N); sigma None: thresholds placed on coefficients
CASES = [
    ("golden-s0.5", 1.0, 0.0, 0.5, False, (8,), 700),
    ("golden-s1", 1.0, 0.0, 1.0, False, (8,), 700),
    ("golden-s2", 1.0, 0.0, 2.0, False, (8, 4), 500),
    ("golden-s5-10", 1.0, 0.0, 5.0, False, (8,), 400),
    ("golden-s25-50", 1.0, 0.0, 25.0, False, (8,), 400),
    ("grey-s1", 1.0, 0.0, 1.0, True, (8, 2, 1), 800),
    ("x16-s25", 16.0, 0.0, 25.0, False, (8,), 700),
    ("x256-s400", 256.0, 0.0, 400.0, False, (8,), 400),
    ("bright-flat-s5", 0.25, 190.0, 5.0, False, (8,), 700),
    ("on-threshold", 1.0, 0.0, None, False, (8, 4, 2, 1), 300),
    ("on-threshold-grey-x16", 16.0, 0.0, None, True, (8, 1), 400),
]


def run_case(case, rel, gabs, seed=7):
    name, scale, offset, sigma, grey, nss, n = case
    rng = np.random.default_rng(seed)
    img, sig = golden_channels(scale, offset, 1.0 if sigma is None else sigma, rng, grey)
    tot = dict(differ=0, escaped=0, escaped_rel_only=0, flagged=0, waves=0)
    ratio = np.zeros((9, 4))
    for c in range(img.shape[1]):
        for NS in nss:
            x = waves(img, c, NS, n, rng)
            if sigma is None:
                sw = on_threshold(x, NS, rng, 2e-3, 5e-2)
                T, Tq = thresholds(sw)
            else:
                T, Tq = thresholds(np.full(n, sig[c], np.float32))
            d, e, eo, r, fl = evaluate(x, NS, T, Tq, rel, gabs)
            tot["differ"] += d; tot["escaped"] += e; tot["escaped_rel_only"] += eo; tot["flagged"] += fl; tot["waves"] += n
            ratio = np.maximum(ratio, r)
    return tot, ratio


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_differing_decision_is_in_a_flagged_wave(case):
    rel, gabs = kernel_guard_constants()
    tot, ratio = run_case(case, rel, gabs)
    print(f"{case[0]}: waves {tot['waves']}, decisions that differ {tot['differ']}, in unflagged waves {tot['escaped']} "
          f"(relative band alone: {tot['escaped_rel_only']}), flagged waves {tot['flagged']}, "
          f"max (form difference - rel |c| / 2) / M {ratio.max():.3g}")
    assert tot["escaped"] == 0, tot
    # the absolute floor keeps a factor of two over the largest form difference the model sees (net of half the relative band)
    assert np.all(gabs >= 2.0 * ratio.astype(np.float32)), (gabs.tolist(), ratio.tolist())


def test_relative_band_alone_lets_decisions_escape():
    """the floor is needed: with the relative band alone (the kernel before the floor), thresholds placed on small coefficients of
    bright or wide-range data give decisions that differ from the reference-order form in waves the guard does not flag"""
    rel, gabs = kernel_guard_constants()
    tot, _ = run_case(("on-threshold", 1.0, 0.0, None, False, (8,), 200), rel, gabs)
    assert tot["escaped_rel_only"] > 0 and tot["escaped"] == 0, tot


if __name__ == "__main__":   # calibration of kHtGuardAbs: the largest (form difference - rel |c| / 2) / M per (st, l) over the cases, larger samples
    import sys
    rel, _ = kernel_guard_constants()
    worst = np.zeros((9, 4))
    for case in CASES:
        case = case[:-1] + (case[-1] * int(sys.argv[1]) if len(sys.argv) > 1 else case[-1],)
        tot, ratio = run_case(case, rel, np.zeros((9, 4), np.float32), seed=11)
        worst = np.maximum(worst, ratio)
        print(case[0], tot, flush=True)
    print("max (form difference - rel |c| / 2) / M per (st, l):", np.array2string(worst, precision=3))
