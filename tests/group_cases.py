"""Seeded synthetic launches for the group kernels' own tests (test_group_model.py on the CPU, test_gpu_group.py on the GPU).

A case is a namespace holding what lfbm5d_debug_group takes: the padded window `noisy` (and `basic`) [A][C][Hb][Wb], the tables
block matching would have produced -- refs [R], self_idx [R][N], self_cnt [R], best [A][Wb*Hb], shape [A][Wb*Hb] --, the pass's
parameters, the SAI mask, pst, fill_quirk, and `runs`: the option sets the GPU test launches it with.  Tables are synthetic, so the
windows are tiny (40 x 40 for patches up to 8 x 8, 48 x 48 for 12 and 16, 64 x 64 for 32): every group has a reference position of
its own, so its angular shape (shape[st][refs[g]]) is chosen per group, and its stack and disparity matches point anywhere in the
window.  Pixels are a smooth texture plus Gaussian noise of sigma 25 in 0..255 (more where a case
would otherwise have more than 5 % of its (group, channel) pairs within the decision gap of a hard threshold, see test_group_model.py; the
cases with the most coefficients per pair -- 16 x 16 patches, 5 x 5 windows -- also take lambda 3.5 instead of 2.7: the shape-adaptive
DCT leaves its coefficients at sqrt2 times the orthonormal scale, so at 2.7 their threshold sits at 2.7 noise sigmas and one
coefficient in 10^5 lands inside the gap whatever sigma is); channels 1 and 2 are signed like the opponent
transform's; the pilot of the Wiener step is a smoothed copy.

`expected_kernels` restates the dispatch of launch_group (lfbm5d_group_*.hip) in Python: what each run is meant to reach.

Sections F and G (wide_cases, bm3d_cases) hold windows of 7 x 7 to 17 x 17 SAIs and the per-SAI BM3D flavour (A = 1).  Their
hard-threshold cases run lambda 3.5; default-lambda decisions on wide windows stay with the whole-pass tests.
"""
from types import SimpleNamespace

import numpy as np

import group_model as M

ID, DCT, SADCT, BIOR, HADAMARD, HAAR = M.ID, M.DCT, M.SADCT, M.BIOR, M.HADAMARD, M.HAAR


def sigma_table(sigma, C):
    """utilities.cpp:633-684 for the opponent colour space, in float32."""
    f = np.float32
    if C == 1:
        return [float(f(sigma))]
    w = [(f(0.333), f(0.333), f(0.333)), (f(0.5), f(0.0), f(0.5)), (f(0.25), f(0.5), f(0.25))]
    return [float(f(np.sqrt(f(a * a + b * b + c * c))) * f(sigma)) for a, b, c in w]


def window_side(k):
    return 40 if k <= 8 else (48 if k <= 16 else 64)


def texture(rng, A, C, Hb, Wb, sigma, scale=1.0, const=False, amp=6.0):
    y, x = np.mgrid[0:Hb, 0:Wb].astype(np.float64)
    img = np.empty((A, C, Hb, Wb))
    sig_c = sigma_table(sigma, C)     # white noise of sigma behind the opponent transform
    for st in range(A):
        for c in range(C):
            ph = rng.uniform(0, 6.28, 3)
            if const:
                base = np.full((Hb, Wb), 100.0 if c == 0 else 12.0 * (c - 1.5))
            else:
                base = amp * np.sin(x / 9.0 + ph[0] + 0.2 * st) * np.cos(y / 7.0 + ph[1]) + 0.5 * amp * np.sin((x + y) / 5.0 + ph[2])
                base = base + (128 if c == 0 else 0)
                if c:
                    base *= 0.4
            img[st, c] = base if const else base + rng.normal(0, sig_c[c], (Hb, Wb))
    if not const:
        img[:, 0] = np.clip(img[:, 0], 0, 255)
    return (img * scale).astype(np.float32)


def smooth(img):
    p = np.pad(img.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    H, W = img.shape[2:]
    return (sum(p[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9).astype(np.float32)


def all_shapes(A, pst, mask):
    """Every subset of the masked SAIs that contains pst, as bit masks."""
    others = [st for st in range(A) if st != pst and mask[st]]
    out = []
    for b in range(1 << len(others)):
        bits = 1 << pst
        for i, st in enumerate(others):
            if (b >> i) & 1:
                bits |= 1 << st
        out.append(bits)
    return out


def wide_shapes(rng, aw, pst, n_random):
    """Windows of 5 x 5 SAIs and more: seeded random shapes, plus every shape with a single SAI in some row or column besides pst's."""
    A = aw * aw
    out = [int(sum(1 << int(st) for st in np.flatnonzero(rng.random(A) < rng.uniform(0.2, 0.95))) | (1 << pst)) for _ in range(n_random)]
    ps, pt = divmod(pst, aw)
    for st in range(A):
        s, t = divmod(st, aw)
        if s != ps or t != pt:
            out.append((1 << pst) | (1 << st))                                  # a lone SAI in another row or column
            out.append(sum(1 << (ps * aw + j) for j in range(aw)) | (1 << st))  # ... next to pst's full row
    return out


def build(name, seed, *, step, tau2, tau4, tau5, k, N, C=3, aw=3, mask=None, pst=None, fill_quirk=1, useSD=0, sigma=25.0, lam=2.7,
          shapes="all", nsx="each", n_groups=None, scale=1.0, pilot="smooth", const=False, edges=False, same=False, runs=((),),
          ref_begin=0, launch=None, sai_major=None, bm3d=False, section="", amp=None):
    rng = np.random.default_rng(seed)
    if bm3d:   # the per-SAI flavour: one image, stacks of 2 .. N (block matching stores a single match twice), Hadamard along the stack
        aw, shapes = 1, ([1] * n_groups if shapes == "all" else shapes)
    A = aw * aw
    sai_major = A >= SAI_MAJOR_MIN_A if sai_major is None else sai_major      # what a pass does
    pst = A // 2 if pst is None else pst
    mask = np.ones(A, np.uint32) if mask is None else np.asarray(mask, np.uint32)
    Wb = Hb = window_side(k)
    t = lambda v: M.TAU[v] if isinstance(v, str) else v
    tau2, tau4, tau5 = t(tau2), t(tau4), t(tau5)
    if shapes == "all":
        shapes = all_shapes(A, pst, mask)
    sizes = [1 << i for i in range(1 if bm3d else 0, N.bit_length())]          # 1, 2, ..., N (BM3D: from 2)
    if nsx == "each":
        groups = [(sh, n) for sh in shapes for n in sizes]
    else:   # one group per shape; the stack sizes in equal shares, dealt by a seeded permutation (not by the shape's bits)
        deal = rng.permutation(len(shapes))
        groups = [(sh, sizes[int(deal[i]) % len(sizes)]) for i, sh in enumerate(shapes)]
    if n_groups is not None:
        groups = groups[:n_groups]
    R = len(groups)
    # positions: the window without the column the centre path reads as zeros (those are placed on purpose, `edges`)
    rows, cols = np.arange(Hb - k + 1), np.arange(Wb - k)
    allowed = (rows[:, None] * Wb + cols[None, :]).reshape(-1)
    assert R <= len(allowed), (name, R, len(allowed))
    refs = rng.permutation(allowed)[:R].astype(np.uint32)
    cnt = np.array([n for _, n in groups], np.uint32)
    idx = rng.choice(allowed, size=(R, N)).astype(np.uint32)
    idx[:, 0] = refs
    plane = Wb * Hb
    best = rng.choice(allowed, size=(A, plane)).astype(np.uint32)
    shape = np.zeros((A, plane), np.uint8)
    for g, (bits, _) in enumerate(groups):
        for st in range(A):
            shape[st, refs[g]] = (bits >> st) & 1
    if edges:   # stack entries in the corners and in the column Wb - k (zero patches of the centre path; still aggregated)
        corner0, corner1 = 0, (Hb - k) * Wb + (Wb - k)
        for g in range(R):
            if cnt[g] > 1:
                idx[g, 1] = (corner0, corner1, (g % (Hb - k + 1)) * Wb + (Wb - k))[g % 3]
        best[:, corner0], best[:, corner1] = corner1, corner0
        for st in range(A):
            best[st, refs[st::A]] = ((refs[st::A] // Wb) * Wb + (Wb - k)).astype(np.uint32)
    if same:    # a stack whose entries are all one position
        idx[:] = refs[:, None]
    # With a 2-D transform the texture is strong, so that more than the DC of a patch survives the threshold and the filtered patches
    # have structure; without one every pixel is a coefficient set of its own, a strong texture under stacks from anywhere in the
    # window puts a fifth of the pairs inside the gap, and the noise alone tells the pixels apart.
    noisy = texture(rng, A, C, Hb, Wb, sigma, scale, const, amp=(6.0 if tau2 == ID else 40.0) if amp is None else amp)
    basic = None
    if step == 2:
        basic = smooth(noisy)
        if pilot == "zero":
            basic[:] = 0
        elif pilot == "tiny":
            basic = (rng.choice([-1.0, 1.0], size=basic.shape) * 1e-20).astype(np.float32)
    for st in range(A):
        if not mask[st]:
            noisy[st] = np.nan            # an empty SAI is never read
            if basic is not None:
                basic[st] = np.nan
    return SimpleNamespace(name=name, step=step, tau2=tau2, tau4=tau4, tau5=tau5, k=k, N=N, C=C, aw=aw, A=A, mask=mask, pst=pst,
                           fill_quirk=fill_quirk, useSD=useSD, sigma_in=float(sigma) * scale, sigma=sigma_table(float(sigma) * scale, C),
                           lam=lam, Wb=Wb, Hb=Hb, R=R, refs=refs, self_idx=idx, self_cnt=cnt, best=best, shape=shape, noisy=noisy,
                           basic=basic, runs=tuple(tuple(r) for r in runs), ref_begin=ref_begin,
                           launch=R - ref_begin if launch is None else launch, sai_major=sai_major, bm3d=bool(bm3d), section=section,
                           nSim=6, nDisp=2, p=3)


def params_tuple(case):
    """(sigma, lambda, N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D, useSD): the arguments of make_params (product and oracle)."""
    return (case.sigma_in, case.lam, case.N, case.nSim, case.nDisp, case.k, case.p, case.tau2, case.tau4, case.tau5, case.useSD)


# ---- the dispatch of launch_group, restated ----
GENERIC_LDS_LIMIT = 160 * 1024 - 8192
SLAB_FLOATS, SLAB_FLOATS_MAX = 18432, 28800
MAX_A = 49                  # kMaxA: beyond it k_group_shape<true> and k_group_big<., true>, the large shape record
SAI_MAJOR_MIN_A = 121       # kSaiMajorMinA: a pass writes filt SAI-major from 11 x 11 SAIs on


def _uses_slab(c, opt):
    if "no_slab_kernel" in opt or c.bm3d or c.useSD or c.aw not in range(3, 18, 2) or c.N > (16 if c.aw > 9 else 32):
        return False
    if c.tau2 == DCT and c.k not in (8, 12, 16):
        return False
    if c.tau2 == BIOR and c.k not in (8, 16):
        return False
    if c.tau2 == ID and c.k > 16:
        return False
    S = 2 if c.step == 2 else 1
    if S * c.N * c.A * 2 > SLAB_FLOATS_MAX:
        return False
    return S * c.N * c.A * c.k * c.k * 4 > (150 if c.tau2 == ID else 64) * 1024


def slab_log2(c):
    """slab_log2 of lfbm5d_group_slab.hip: log2 of the pixels a slab of k_group_slab holds."""
    per_px = (2 if c.step == 2 else 1) * c.N * c.A
    ls = 6
    while ls > 2 and (per_px << ls) > SLAB_FLOATS:
        ls -= 1
    if (per_px << ls) > SLAB_FLOATS_MAX:
        ls = 1
    return ls


def expected_kernels(c, opt=()):
    k2, bytes_ = c.k * c.k, c.A * c.C * c.Wb * c.Hb * 4
    names = ["k_group_pos", "k_group_shape<true>" if c.A > MAX_A else "k_group_shape<false>"]
    all_sa = c.tau4 == SADCT and not c.mask.all() and "no_sa_kernels" not in opt
    haar = c.tau5 == HAAR
    if "group_generic" not in opt:
        if c.tau2 == ID and c.N <= 8 and k2 <= 256 and c.step == 1 and c.A == 9 and bytes_ < 0x7fffffff:
            if all_sa:
                return names + ["k_group_id_haar_sa" if haar else "k_group_id_any_sa"]
            fast = haar and c.tau4 in (DCT, SADCT) and "ht_reference_order" not in opt
            names.append("k_group_id_haar_fast" if fast else ("k_group_id_haar" if haar else "k_group_id_any"))
            if c.tau4 == SADCT or fast:
                names.append("k_group_id_haar_list" if haar else "k_group_id_any_list")
            return names
        if c.tau2 in (BIOR, DCT) and c.k == 16 and c.N <= 8 and c.step == 1 and c.A == 9:
            stem = "k_group_bior16" if c.tau2 == BIOR else "k_group_dct16"
            if c.N == 1 and c.tau5 != DCT:
                return names + [stem + ("_n1_sa" if all_sa else "_n1")]
            return names + [stem + ("_haar" if haar else "_any")]
        if c.tau2 == BIOR and c.k == 8 and c.A == 9 and c.step == 2 and c.N <= 16:
            return names + ["k_group_dct8w<true>" if haar else "k_group_dct8w<false>"]
        if c.tau2 == DCT and c.k == 8 and c.A == 9 and c.N <= 16:
            if c.step == 1:
                return names + ["k_group_dct8"]
            if haar and "dct8w_v2" not in opt:
                if all_sa:
                    return names + ["k_group_dct8w3<true>"]
                if c.tau4 in (DCT, SADCT):
                    return names + ["k_group_dct8w3_u"] + (["k_group_dct8w3_list"] if c.tau4 == SADCT else [])
                return names + ["k_group_dct8w3<false>"]
            return names + ["k_group_dct8w2<true>" if haar else "k_group_dct8w2<false>"]
        if c.aw >= 5 and c.tau2 == ID and c.step == 1 and not c.bm3d and c.N <= 8 and k2 <= 256 and bytes_ < 0x7fffffff:
            split = not (c.useSD or "wide_nosplit" in opt)
            return names + (["k_group_idw<AW, SLAB, true>", "k_group_idw_weight"] if split else ["k_group_idw<AW, SLAB, false>"])
        if c.bm3d and c.A == 1 and c.k == 8 and c.tau5 == HADAMARD and c.tau2 in (DCT, BIOR):
            return names + ["k_group_bm3d8<%d, %s>" % (c.step, "true" if c.tau2 == BIOR else "false")]
        if _uses_slab(c, opt):
            return names + ["k_group_slab<%d, WA, MAXN>" % c.step]
    rows_form = (c.tau2 == BIOR and c.k in (8, 16)) or (c.tau2 == DCT and c.k in (8, 12, 16))
    tmp = (256 // c.k) * c.k * (c.k + 1) if rows_form else max(256, k2)
    lds = ((2 if c.step == 2 else 1) * c.N * c.A * k2 + tmp) * 4
    if lds > GENERIC_LDS_LIMIT or c.A > MAX_A:
        return names + ["k_group_big<%d, %s>" % (c.step, "true" if c.A > MAX_A else "false")]
    return names + ["k_group<%d>" % c.step]


# every __global__ of lfbm5d_group_{ht,wiener,generic,wide,slab}.hip, by the text the dispatchers record
ALL_KERNELS = [
    "k_group_pos", "k_group_shape<false>", "k_group_shape<true>", "k_group<1>", "k_group<2>",
    "k_group_big<1, false>", "k_group_big<2, false>", "k_group_big<1, true>", "k_group_big<2, true>",
    "k_group_bm3d8<1, true>", "k_group_bm3d8<1, false>", "k_group_bm3d8<2, true>", "k_group_bm3d8<2, false>",
    "k_group_id_haar_fast", "k_group_id_haar", "k_group_id_any", "k_group_id_haar_list", "k_group_id_any_list",
    "k_group_id_haar_sa", "k_group_id_any_sa",
    "k_group_bior16_haar", "k_group_bior16_any", "k_group_dct16_haar", "k_group_dct16_any",
    "k_group_bior16_n1", "k_group_dct16_n1", "k_group_bior16_n1_sa", "k_group_dct16_n1_sa",
    "k_group_dct8", "k_group_dct8w<true>", "k_group_dct8w<false>", "k_group_dct8w2<true>", "k_group_dct8w2<false>",
    "k_group_dct8w3<true>", "k_group_dct8w3<false>", "k_group_dct8w3_u", "k_group_dct8w3_list",
    "k_group_idw<AW, SLAB, true>", "k_group_idw<AW, SLAB, false>", "k_group_idw_weight",
    "k_group_slab<1, WA, MAXN>", "k_group_slab<2, WA, MAXN>",
]


def cases():
    out = []
    add = lambda *a, **kw: out.append(build(*a, **kw))
    one_missing = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], np.uint32)
    two_missing = np.array([0, 1, 1, 1, 1, 1, 1, 0, 1], np.uint32)
    # A. every angular shape of a 3 x 3 window
    add("ht-id-haar-k8", 101, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, runs=((), ("ht_reference_order",)))
    add("ht-id-hw-k8", 102, step=1, tau2="id", tau4="sadct", tau5="hw", k=8, N=8)
    add("ht-id-haar-k4", 103, step=1, tau2="id", tau4="sadct", tau5="haar", k=4, N=8, nsx="cycle")
    add("ht-id-haar-k16", 104, sigma=75.0, lam=3.5, step=1, tau2="id", tau4="sadct", tau5="haar", k=16, N=8, nsx="cycle")
    add("ht-dct-haar-k8", 105, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8)
    for i, (t2, t5) in enumerate((("bior", "haar"), ("bior", "hw"), ("dct", "haar"), ("dct", "hw"))):
        add("ht-%s-%s-k16" % (t2, t5), 110 + i, sigma=75.0, lam=3.5, step=1, tau2=t2, tau4="sadct", tau5=t5, k=16, N=8, C=1)
        # ... and at the default lambda, with stacks of two (a pair then holds as many coefficients as an 8 x 8 one with eight)
        add("ht-%s-%s-k16-n2" % (t2, t5), 210 + i, sigma=60.0, step=1, tau2=t2, tau4="sadct", tau5=t5, k=16, N=2, nsx="cycle")
    add("ht-bior-k16-n1", 115, sigma=40.0, step=1, tau2="bior", tau4="sadct", tau5="haar", k=16, N=1)
    add("ht-dct-k16-n1", 116, step=1, tau2="dct", tau4="sadct", tau5="haar", k=16, N=1)
    add("wien-dct-haar-k8", 120, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8,
        runs=((), ("dct8w_v2",), ("group_generic",)))
    add("wien-dct-haar-k8-n16", 121, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=16, C=1, nsx="cycle")
    add("wien-dct-hw-k8", 122, step=2, tau2="dct", tau4="sadct", tau5="hw", k=8, N=8)
    add("wien-dct-haar-k8-id4", 123, step=2, tau2="dct", tau4="id", tau5="haar", k=8, N=8, shapes=[0x1ff] * 64)
    add("wien-bior-haar-k8", 124, step=2, tau2="bior", tau4="sadct", tau5="haar", k=8, N=8)
    add("wien-bior-hw-k8", 125, step=2, tau2="bior", tau4="sadct", tau5="hw", k=8, N=8)
    # tau_4D = dct: shapes are ignored, the full DCT is taken
    add("ht-id-haar-k8-dct4", 130, sigma=60.0, lam=3.5, step=1, tau2="id", tau4="dct", tau5="haar", k=8, N=8, nsx="cycle")
    add("wien-dct-haar-k8-dct4", 131, step=2, tau2="dct", tau4="dct", tau5="haar", k=8, N=8, nsx="cycle")
    add("ht-id-hw-k8-dct4", 132, sigma=60.0, step=1, tau2="id", tau4="dct", tau5="hw", k=8, N=8, shapes=[0x1ff] * 64, nsx="cycle")
    add("ht-dct-haar-k8-dct4", 133, sigma=60.0, step=1, tau2="dct", tau4="dct", tau5="haar", k=8, N=8, shapes=[0x1ff] * 64, nsx="cycle")
    for i, (t2, t5) in enumerate((("bior", "haar"), ("bior", "hw"), ("dct", "haar"), ("dct", "hw"))):
        add("ht-%s-%s-k16-dct4" % (t2, t5), 220 + i, sigma=100.0, step=1, tau2=t2, tau4="dct", tau5=t5, k=16, N=8, shapes=[0x1ff] * 32, nsx="cycle")
    add("wien-dct-hw-k8-dct4", 134, step=2, tau2="dct", tau4="dct", tau5="hw", k=8, N=8, shapes=[0x1ff] * 64, nsx="cycle")
    add("wien-bior-haar-k8-dct4", 226, step=2, tau2="bior", tau4="dct", tau5="haar", k=8, N=8, shapes=[0x1ff] * 64, nsx="cycle")
    add("wien-bior-hw-k8-dct4", 227, step=2, tau2="bior", tau4="dct", tau5="hw", k=8, N=8, shapes=[0x1ff] * 64, nsx="cycle")
    # the general kernel
    add("ht-dct-k10", 135, sigma=40.0, step=1, tau2="dct", tau4="sadct", tau5="haar", k=10, N=8, nsx="cycle")
    add("ht-bior-k4", 136, step=1, tau2="bior", tau4="sadct", tau5="hw", k=4, N=8, nsx="cycle")
    add("wien-dct-k8-n32-dct5", 137, step=2, tau2="dct", tau4="sadct", tau5="dct", k=8, N=32, C=1, nsx="cycle",
        runs=((), ("no_slab_kernel",)))
    add("ht-id-k8-n16-dct5", 138, step=1, tau2="id", tau4="sadct", tau5="dct", k=8, N=16, C=1, nsx="cycle")
    # B. empty SAIs: every shape inside the mask
    add("ht-id-haar-k8-1empty", 140, sigma=40.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, mask=one_missing, nsx="cycle",
        runs=((), ("no_sa_kernels",)))
    add("ht-id-hw-k8-2empty", 141, step=1, tau2="id", tau4="sadct", tau5="hw", k=8, N=8, mask=two_missing, nsx="cycle")
    add("wien-dct-haar-k8-1empty", 142, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, mask=one_missing, nsx="cycle",
        runs=((), ("no_sa_kernels",)))
    add("ht-bior-k16-n1-1empty", 143, sigma=50.0, step=1, tau2="bior", tau4="sadct", tau5="haar", k=16, N=1, mask=one_missing)
    add("ht-dct-k16-n1-2empty", 144, step=1, tau2="dct", tau4="sadct", tau5="haar", k=16, N=1, mask=two_missing)
    add("ht-id-haar-k8-pst1-subset", 145, sigma=40.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, mask=one_missing, pst=1, fill_quirk=0,
        nsx="cycle")
    add("wien-dct-haar-k8-pst8-subset", 146, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, pst=8, fill_quirk=0, nsx="cycle")
    # C. launch edges
    for n in (1, 7, 9):
        add("ht-id-haar-k8-%dgroups" % n, 150 + n, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", n_groups=n)
        add("wien-dct-haar-k8-%dgroups" % n, 160 + n, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", n_groups=n)
    add("ht-id-haar-k8-band", 170, sigma=40.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", ref_begin=37, launch=101)
    add("wien-dct-haar-k8-band", 171, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", ref_begin=37, launch=101)
    add("ht-id-haar-k8-edges", 172, sigma=75.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", edges=True)
    add("ht-id-haar-k8-edges-subset", 173, sigma=50.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", edges=True, fill_quirk=0)
    add("wien-dct-haar-k8-edges", 174, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", edges=True)
    add("wien-dct-haar-k8-same", 175, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", same=True)
    add("ht-id-haar-k8-same", 176, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", same=True)
    # D. values
    add("wien-pilot-zero", 180, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", pilot="zero", n_groups=64)
    add("wien-pilot-tiny", 181, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", pilot="tiny", n_groups=64)
    rev = all_shapes(9, 4, np.ones(9, np.uint32))[::-1]     # the whole window first
    add("ht-constant", 182, shapes=rev, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", const=True, n_groups=64)
    add("ht-constant-sd", 183, shapes=rev, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", const=True, n_groups=64, useSD=1)
    add("ht-id-haar-k8-x16", 184, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", scale=16.0)
    add("wien-dct-haar-k8-x16", 185, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", scale=16.0)
    add("ht-id-haar-k8-sd", 186, sigma=40.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", useSD=1)
    add("wien-dct-haar-k8-sd", 187, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, nsx="cycle", useSD=1)
    # E. a 5 x 5 window
    rng = np.random.default_rng(7)
    w5 = wide_shapes(rng, 5, 12, 200)
    add("ht-id-haar-k8-5x5", 190, sigma=75.0, lam=3.5, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, aw=5, shapes=w5, nsx="cycle",
        runs=((), ("wide_nosplit",)))
    add("ht-id-haar-k8-n2-5x5", 195, sigma=50.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=2, aw=5, shapes=w5, nsx="cycle")   # the default lambda
    add("ht-id-haar-k8-5x5-sd", 191, sigma=75.0, lam=3.5, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, aw=5, shapes=w5, nsx="cycle", useSD=1)
    add("wien-dct-haar-k8-5x5", 192, step=2, tau2="dct", tau4="sadct", tau5="haar", k=8, N=8, aw=5, shapes=w5, nsx="cycle", C=1,
        runs=((), ("no_slab_kernel",)))
    add("ht-dct-haar-k8-n32-5x5", 194, lam=4.0, sigma=75.0, step=1, tau2="dct", tau4="sadct", tau5="haar", k=8, N=32, aw=5, shapes=w5[::4], nsx="cycle",
        C=1, runs=((), ("no_slab_kernel",)))
    add("ht-id-haar-k8-5x5-saimajor", 193, sigma=100.0, step=1, tau2="id", tau4="sadct", tau5="haar", k=8, N=8, aw=5, shapes=w5[:40], nsx="cycle",
        sai_major=True, C=1)
    out += wide_cases() + bm3d_cases()
    return out


def thin(rng, aw, pst, count):
    """`count` shapes of an aw x aw window from wide_shapes: half seeded random ones, the rest drawn from the lone-SAI shapes (a lone
    SAI in another row or column, and the same next to pst's full row)."""
    n_random = count // 2
    sh = wide_shapes(rng, aw, pst, n_random)
    pick = np.sort(rng.choice(np.arange(n_random, len(sh)), size=count - n_random, replace=False))
    return sh[:n_random] + [sh[int(i)] for i in pick]


def wide_cases():
    """F. windows of 7 x 7 to 17 x 17 SAIs.  Hard-threshold cases take lambda 3.5, with a sigma of 75 .. 100 without a 2-D transform and of 30 .. 50 and a
    texture of twice the amplitude with one (so that more than k^2 coefficients survive in a quarter of the pairs): at the default 2.7 a pair
    of such a window holds so many coefficients that more than 5 % of the pairs are open whatever sigma is (7 x 7: 5 / 64, 9 x 9:
    7 / 64, 17 x 17 with N = 1: 16 / 64); default-lambda decisions on wide windows stay with the whole-pass tests.  The Wiener cases
    run the default parameters.  C = 1 unless a case says otherwise; from 11 x 11 on filt is SAI-major, as in a pass."""
    out = []

    def add(name, seed, aw, n, pst=None, **kw):
        kw.setdefault("C", 1)
        pst_ = aw * aw // 2 if pst is None else pst
        shapes = thin(np.random.default_rng(1000 + seed), aw, pst_, max(n, 4))      # (one group: the first, a random shape)
        out.append(build(name, seed, aw=aw, pst=pst, shapes=shapes, n_groups=n, nsx="cycle", tau4="sadct", section="F", **kw))

    ht = dict(step=1, lam=3.5)
    idw = dict(step=1, lam=3.5, tau2="id", tau5="haar")
    # k_group_idw<AW, SLAB, .> of every window side
    add("ht-id-haar-k8-n8-7x7", 301, 7, 56, sigma=75.0, k=8, N=8, **idw)
    add("ht-id-haar-k16-9x9", 302, 9, 48, sigma=75.0, k=16, N=4, **idw)
    add("ht-id-haar-k6-11x11", 303, 11, 32, sigma=75.0, k=6, N=4, runs=((), ("filt_group_major",)), **idw)     # 36 pixels: a slab tail
    add("ht-id-haar-k8-c3-13x13", 304, 13, 24, sigma=75.0, k=8, N=2, C=3, **idw)
    add("ht-id-haar-k10-15x15", 305, 15, 24, sigma=75.0, k=10, N=2, runs=((), ("wide_nosplit",)), **idw)        # 100 pixels: a slab tail
    add("ht-id-haar-k8-15x15-sd", 306, 15, 24, sigma=75.0, k=8, N=4, useSD=1, **idw)
    add("ht-id-haar-k8-17x17", 307, 17, 16, sigma=75.0, k=8, N=2, **idw)
    # k_group_slab<STEP, WA, MAXN> of every window side, and every slab tier (ls) of slab_log2
    add("ht-bior-haar-k8-n8-7x7", 310, 7, 56, sigma=35.0, amp=80.0, tau2="bior", tau5="haar", k=8, N=8, **ht)                          # ls 5
    add("wien-id-haar-k8-7x7", 311, 7, 48, step=2, tau2="id", tau5="haar", k=8, N=8)                             # ls 4; 196 KB of stacks
    add("ht-dct-hw-k8-9x9", 312, 9, 48, sigma=35.0, amp=80.0, tau2="dct", tau5="hw", k=8, N=8, runs=((), ("no_slab_kernel",)), **ht)   # ls 4
    add("ht-dct-haar-k12-n2-9x9", 315, 9, 48, sigma=30.0, amp=80.0, tau2="dct", tau5="haar", k=12, N=2, **ht)                          # ls 6
    add("wien-dct-haar-k8-n32-9x9", 314, 9, 32, step=2, tau2="dct", tau5="haar", k=8, N=32)                      # ls 2, MAXN = 32, 81 KB of LDS
    add("wien-dct-haar-k8-11x11", 315, 11, 32, step=2, tau2="dct", tau5="haar", k=8, N=8, runs=((), ("filt_group_major",)))   # ls 3
    add("wien-dct-haar-k8-n16-13x13", 316, 13, 24, step=2, tau2="dct", tau5="haar", k=8, N=16, runs=((), ("no_slab_kernel",)))   # ls 2 beyond 72 KB
    add("ht-bior-dct5-k8-15x15", 317, 15, 24, sigma=50.0, amp=80.0, tau2="bior", tau5="dct", k=8, N=8, **ht)                           # ls 3
    add("wien-dct-haar-k8-n16-17x17", 318, 17, 12, step=2, tau2="dct", tau5="haar", k=8, N=16)                   # ls 1
    # the general kernels: k_group<.> at A = 49 (stacks below the slab rule's 64 KB), k_group_big<., true> beyond
    add("ht-bior-haar-k4-7x7", 320, 7, 56, sigma=35.0, amp=80.0, tau2="bior", tau5="haar", k=4, N=8, **ht)
    add("wien-dct-haar-k8-n2-7x7", 321, 7, 56, step=2, tau2="dct", tau5="haar", k=8, N=2)
    add("ht-dct-haar-k8-9x9-sd", 322, 9, 48, sigma=35.0, amp=80.0, tau2="dct", tau5="haar", k=8, N=4, useSD=1, **ht)
    add("wien-dct-haar-k8-9x9-sd", 323, 9, 48, step=2, tau2="dct", tau5="haar", k=8, N=4, useSD=1)
    add("ht-dct-haar-k10-9x9", 324, 9, 48, sigma=35.0, amp=80.0, tau2="dct", tau5="haar", k=10, N=4, **ht)
    # empty SAIs (every group is shape-adaptive), and a subset pass: pst off-centre, no zero column
    m9, m13 = np.ones(81, np.uint32), np.ones(169, np.uint32)
    m9[[0, 13, 44, 80]] = 0
    m13[[5, 30, 31, 100, 168]] = 0
    add("ht-id-haar-k8-9x9-empty", 330, 9, 48, sigma=75.0, k=8, N=4, mask=m9, **idw)
    add("wien-dct-haar-k8-13x13-empty", 331, 13, 24, step=2, tau2="dct", tau5="haar", k=8, N=8, mask=m13)
    add("ht-id-haar-k8-11x11-subset", 332, 11, 32, pst=3 * 11 + 8, sigma=75.0, k=8, N=4, fill_quirk=0, **idw)
    # launch edges
    add("ht-id-haar-k8-9x9-band", 340, 9, 48, sigma=75.0, k=8, N=4, ref_begin=5, launch=21, **idw)
    add("wien-dct-haar-k8-9x9-band", 341, 9, 48, step=2, tau2="dct", tau5="haar", k=8, N=8, ref_begin=5, launch=21)
    add("ht-id-haar-k8-9x9-1group", 350, 9, 1, sigma=75.0, k=8, N=4, **idw)
    add("wien-dct-haar-k8-9x9-1group", 343, 9, 1, step=2, tau2="dct", tau5="haar", k=8, N=8)
    add("ht-id-haar-k8-9x9-edges", 344, 9, 48, sigma=100.0, k=8, N=4, edges=True, **idw)
    add("wien-dct-haar-k8-9x9-edges", 345, 9, 48, step=2, tau2="dct", tau5="haar", k=8, N=8, edges=True)
    return out


def bm3d_cases():
    """G. the per-SAI BM3D flavour: one image (A = 1), 2-D transform and Hadamard along stacks of 2 .. N patches.  With useSD the
    reference weights every channel by channel 0's deviation (the aggregation's wchan0); the group kernels store each channel's own,
    so those cases have one channel."""
    out = []

    def add(name, seed, n, **kw):
        kw.setdefault("C", 1)
        kw.setdefault("k", 8)
        out.append(build(name, seed, bm3d=True, n_groups=n, nsx="cycle", tau4="id", tau5="hw", section="G", **kw))

    ht = dict(step=1, lam=3.5, sigma=25.0, amp=80.0)
    add("bm3d-ht-bior-n16-c3", 401, 64, tau2="bior", N=16, C=3, runs=((), ("group_generic",)), **ht)
    add("bm3d-ht-dct-n32", 402, 60, tau2="dct", N=32, **ht)
    add("bm3d-wien-bior-n32", 403, 60, step=2, tau2="bior", N=32)
    add("bm3d-wien-dct-n16-c3", 404, 64, step=2, tau2="dct", N=16, C=3, runs=((), ("group_generic",)))
    add("bm3d-ht-dct-n16-sd", 405, 64, tau2="dct", N=16, useSD=1, **ht)
    add("bm3d-wien-bior-n16-sd", 406, 64, step=2, tau2="bior", N=16, useSD=1)
    add("bm3d-ht-bior-n16-edges", 407, 64, tau2="bior", N=16, edges=True, **ht)
    add("bm3d-wien-dct-n16-same", 408, 64, step=2, tau2="dct", N=16, same=True)
    for n in (1, 3, 4, 5):      # the kernel packs four groups into a workgroup
        add("bm3d-ht-dct-n16-%dgroups" % n, 410 + n, n, tau2="dct", N=16, **ht)
        add("bm3d-wien-bior-n16-%dgroups" % n, 420 + n, n, step=2, tau2="bior", N=16)
    add("bm3d-ht-bior-n16-band", 430, 13, tau2="bior", N=16, ref_begin=3, launch=6, **ht)
    add("bm3d-wien-dct-n16-band", 431, 13, step=2, tau2="dct", N=16, ref_begin=3, launch=6)
    # 12 x 12 patches (BM3D's choice at high sigma): the general kernel under bm3d
    add("bm3d-ht-dct-k12-n16", 440, 48, tau2="dct", k=12, N=16, **ht)
    add("bm3d-wien-dct-k12-n16", 441, 48, step=2, tau2="dct", k=12, N=16)
    return out
