/*
 * lfbm5d_group_generic.hip -- the group stage of a core pass (core:277-481 / :1054-1282) for gfx950: the geometry pre-pass
 * (k_group_pos, k_group_shape), the GENERAL group kernel -- any patch size, any transform combination, any angular window,
 * stacks in LDS (k_group) or in HBM scratch slices (k_group_big) -- and launch_group, which hands a configuration to its dedicated
 * kernel (lfbm5d_group_ht.hip, lfbm5d_group_wiener.hip) when there is one.  Split from lfbm5d_kernels.hip in round 5.
 */
#include "lfbm5d_group_generic.h"

namespace lfbm5d {

namespace {

/* ------------------------------------------------------------------------------------------
 * Group geometry pre-pass (core:286-323, :503): for every group of the launch, the window position
 * of each of its N x A patches (0xffffffff: no patch), the positions the aggregation kernel adds
 * them at, and the 9-bit angular shape.  Doing this once, fully parallel, takes the
 * self_idx -> best -> patch dependent-load chain out of every group workgroup.
 * ------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void k_group_pos(GroupArgs a) {
    /* one thread per (group, match): the A disparity look-ups of a match are independent loads */
    const int A = a.A, N = a.N, NA = N * A;
    const size_t plane = (size_t)a.Wb * a.Hb;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0 && a.sa_list) a.sa_list[0] = 0u;   /* (k_group_shape, the next launch on the stream, appends) */
    if (idx >= (size_t)a.n_groups * N) return;
    const unsigned g = a.ref_begin + (unsigned)(idx / N);
    const int n = (int)(idx % N);
    const int nSx = (int)a.self_cnt[g];
    const unsigned k_r = a.refs[g];
    const unsigned ind_pst = n < nSx ? a.self_idx[(size_t)g * N + n] : 0u;
    /* byte offsets and presence bits for the scalar loads of the register-resident HT kernel (launch_group) */
    const bool want_ofs = A == 9 && a.tau2 == 4 && a.step == 1 && (size_t)A * a.C * plane * 4 < 0x7fffffffull;
    unsigned bits = 0;
    for (int st = 0; st < A; st++) {
        const bool masked = a.mask_bits.test((unsigned)st);
        unsigned p = 0xffffffffu;
        if (n < nSx && masked) p = (st == (int)a.pst) ? ind_pst : a.best[(size_t)st * plane + ind_pst];
        /* gather position: patches whose column equals Wb-k read the reference's never-filled table
         * column, i.e. zeros (core:1697, bm3d.cpp:737) on the centre path -- they are still aggregated */
        const bool zero_patch = a.fill_quirk && p != 0xffffffffu && (p % a.Wb) >= a.Wb - a.k;
        const int i = n * A + st;
        a.gpos[(size_t)g * NA + i] = zero_patch ? 0xffffffffu : p;
        if (want_ofs) {
            const bool there = !zero_patch && p != 0xffffffffu;
            a.gofs[(size_t)g * NA + i] = there ? (unsigned)(((size_t)st * a.C * plane + p) * 4) : 0u;
            bits |= there ? 1u << st : 0u;
        }
        const bool in_shape = st == (int)a.pst || (masked && a.shape[(size_t)st * plane + k_r]);
        /* positions the aggregation kernel will add this group's patches at; 0xffffffff = none
         * (match slot unused, empty SAI, or SAI outside the SADCT shape, core:503) */
        /* stored as (row << 16) | column: the aggregation kernel tests each position against many tiles */
        a.aggpos[((size_t)st * a.n_refs_total + g) * N + n] = ((a.tau4 != 6 || in_shape) && p != 0xffffffffu) ? ((p / a.Wb) << 16) | (p % a.Wb) : 0xffffffffu;
    }
    if (want_ofs) a.gok[(size_t)g * N + n] = bits;
}
template <bool BIG>   /* BIG: windows of more than 7x7 SAIs (records of kShapeInfoBigBytes, built in place in global memory) */
__global__ __launch_bounds__(256) void k_group_shape(GroupArgs a) {
    typedef typename std::conditional<BIG, ShapeInfoBig, ShapeInfo>::type SH;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_groups) return;
    const unsigned g = a.ref_begin + i;
    const size_t plane = (size_t)a.Wb * a.Hb;
    const unsigned k_r = a.refs[g];
    /* only what the group kernels read is written: the first A entries of each array (the record is sized for a 7x7
     * window, a 3x3 one uses a fifth of it), and nothing but the flag when the angular transform is not shape-adaptive */
    SH* out = reinterpret_cast<SH*>(a.gshape) + g;
    if (a.tau4 != 6) { out->use_sadct = 0; return; }
    const int A = (int)a.A, aw = window_side(A);
    if (BIG) {
        int* m = out->mask_dct;   /* (scratch until build_shape overwrites it: the shape goes in through a second array) */
        int full = 0;
        for (int st = 0; st < A; st++) {
            const bool masked = a.mask_bits.test((unsigned)st);
            m[st] = (st == (int)a.pst || (masked && a.shape[(size_t)st * plane + k_r])) ? 1 : 0;
            full += m[st];
        }
        if (full == A) { out->use_sadct = 0; return; }
        for (int st = 0; st < A; st++) out->mask[st] = m[st];
        build_shape(*out, out->mask, aw);
        return;
    }
    SH sh;
    int m[BIG ? 1 : kMaxA], full = 0;
    for (int st = 0; st < A; st++) {
        const bool masked = a.mask_bits.test((unsigned)st);
        m[st] = (st == (int)a.pst || (masked && a.shape[(size_t)st * plane + k_r])) ? 1 : 0;
        full += m[st];
    }
    /* the usual case, every SAI in the shape: the plain angular DCT, and the group kernels read nothing but the flag */
    if (full == A) { out->use_sadct = 0; return; }
    build_shape(sh, m, aw);
    for (int q = 0; q < A; q++) {
        out->mask[q] = sh.mask[q]; out->idx[q] = sh.idx[q]; out->mask_col[q] = sh.mask_col[q];
        out->idx_col[q] = sh.idx_col[q]; out->mask_dct[q] = sh.mask_dct[q];
    }
    for (int q = 0; q < aw; q++) { out->row_n[q] = sh.row_n[q]; out->col_n[q] = sh.col_n[q]; }
    out->use_sadct = sh.use_sadct;
    if (sh.use_sadct && a.sa_list) a.sa_list[1u + atomicAdd(&a.sa_list[0], 1u)] = g | (7u << 29);   /* every channel */
}

template <int STEP>
__global__ __launch_bounds__(kThreads) void k_group(GroupArgs a) {
    extern __shared__ float lds[];
    __shared__ unsigned pos[kMaxN3 * kMaxA];
    __shared__ float red[3][kThreads / 64];
    const unsigned g = a.ref_begin + blockIdx.x;
    const int stack = (int)a.self_cnt[g] * (int)a.A * (int)(a.k * a.k);
    group_generic<STEP>(a, g, (int)blockIdx.y, lds, STEP == 2 ? lds + stack : nullptr, lds + (STEP == 2 ? 2 : 1) * stack, pos, red);
}

/* Stacks beyond the LDS (a 5x5 window with the README's 16x16 patches: 8 x 25 x 256 floats = 200 KiB per stack; N = 32
 * with 16x16 patches): a persistent launch, every workgroup owns a slice of an HBM scratch buffer for its stack(s) and
 * walks over (group, channel) items.  Global memory written by a workgroup is visible to it after a barrier (one CU, one
 * vector L1), so the phases are the LDS kernel's, only slower; the 2-D stage's work area stays in LDS. */
template <int STEP, bool BIG>
__global__ __launch_bounds__(kThreads) void k_group_big(GroupArgs a, float* scratch, unsigned long long slice_floats, unsigned tmp_floats) {
    extern __shared__ float lds[];
    __shared__ unsigned pos_small[BIG ? 1 : kMaxN3 * kMaxA];
    __shared__ float red[3][kThreads / 64];
    unsigned* pos = BIG ? reinterpret_cast<unsigned*>(lds + tmp_floats) : pos_small;   /* BIG: N x A positions behind the 2-D work area */
    float* S0 = scratch + (size_t)blockIdx.x * slice_floats;
    const unsigned items = a.n_groups * a.C;
    for (unsigned it = blockIdx.x; it < items; it += gridDim.x) {
        const unsigned g = a.ref_begin + it / a.C;
        const int stack = (int)a.self_cnt[g] * (int)a.A * (int)(a.k * a.k);
        group_generic<STEP, BIG>(a, g, (int)(it % a.C), S0, STEP == 2 ? S0 + stack : nullptr, lds, pos, red);
        __syncthreads();   /* pos / red / the scratch slice are reused by the next item */
    }
}

} /* namespace */

/* Kernels whose LDS stack can exceed the 64 KiB a launch gets by default: raise the limit once per device
 * (called from lfbm5d_create after hipSetDevice; the attribute belongs to the device's code object). */
hipError_t prepare_group_kernels() {
    const void* fns[] = {reinterpret_cast<const void*>(&k_group<1>), reinterpret_cast<const void*>(&k_group<2>)};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kGenericLdsLimit);
        if (e != hipSuccess) return e;
    }
    hipError_t e = prepare_group_ht();
    if (e == hipSuccess) e = prepare_group_wiener();
    if (e == hipSuccess) e = prepare_group_wide();
    if (e == hipSuccess) e = prepare_group_slab();
    if (e == hipSuccess) e = prepare_group_corr();
    return e;
}

size_t group_tmp_floats(const GroupArgs& a) {
    /* the 2-D stage's work area: one patch per wave-quarter for the generic path, [patch][k][k+1] for bior1.5 */
    const bool rows_form = (a.tau2 == 7 && (a.k == 8 || a.k == 16)) || (a.tau2 == 5 && (a.k == 8 || a.k == 12 || a.k == 16));   /* bior2d_fast, fwd2d_dct */
    return rows_form ? (size_t)(kThreads / a.k) * a.k * (a.k + 1) : std::max<size_t>(256, (size_t)a.k * a.k);
}
size_t group_lds_bytes(const GroupArgs& a) {
    const size_t stack = (size_t)a.N * a.A * a.k * a.k;
    return ((a.step == 2 ? 2 : 1) * stack + group_tmp_floats(a)) * sizeof(float);
}
static bool group_uses_generic(const GroupArgs& a) {   /* mirrors the dispatch of launch_group_ht / launch_group_wiener */
    if (a.opt & kOptGroupGeneric) return true;
    bool wide_window = false;
    for (unsigned w = 5; w <= 17; w += 2) wide_window |= a.A == w * w;
    if (wide_window && a.tau2 == 4 && a.step == 1 && !a.bm3d && a.N <= 8 && a.k * a.k <= 256 && (size_t)a.A * a.C * a.Wb * a.Hb * 4 < 0x7fffffffull) return false;   /* lfbm5d_group_wide.hip */
    if (a.A != 9 && !(a.bm3d && a.A == 1)) return true;
    if (a.A == 9 && a.tau2 == 4 && a.N <= 8 && a.k * a.k <= 256 && a.step == 1) return false;
    if (a.A == 9 && (a.tau2 == 7 || a.tau2 == 5) && a.k == 16 && a.N <= 8 && a.step == 1) return false;
    if (a.A == 9 && a.tau2 == 7 && a.k == 8 && a.step == 2 && a.N <= (unsigned)kMaxN) return false;
    if (a.A == 9 && a.tau2 == 5 && a.k == 8 && a.N <= (unsigned)kMaxN) return false;
    if (a.bm3d && a.A == 1 && a.k == 8 && a.tau5 == 8 && (a.tau2 == 5 || a.tau2 == 7)) return false;
    return true;
}
size_t group_scratch_bytes(const GroupArgs& a) {
    if (group_uses_generic(a) && !(a.opt & kOptGroupGeneric) && group_uses_slab(a)) return group_slab_scratch_bytes(a);
    if (!group_uses_generic(a) || (group_lds_bytes(a) <= (size_t)kGenericLdsLimit && a.A <= (unsigned)kMaxA)) return 0;
    return (size_t)kBigBlocks * (a.step == 2 ? 2 : 1) * a.N * a.A * a.k * a.k * sizeof(float);
}
hipError_t launch_group(hipStream_t s, const GroupArgs& a, std::string* trace, const float* corr_tab) {
    /* geometry pre-pass: patch positions, aggregation positions, angular shapes */
    LFBM5D_LAUNCH(trace, k_group_pos, grid1d((size_t)a.n_groups * a.N), dim3(256), 0, s, a);
    const bool bigA = a.A > (unsigned)kMaxA;
    if (bigA) LFBM5D_LAUNCH(trace, k_group_shape<true>, grid1d(a.n_groups), dim3(256), 0, s, a);
    else      LFBM5D_LAUNCH(trace, k_group_shape<false>, grid1d(a.n_groups), dim3(256), 0, s, a);
    /* a window with an empty SAI: tau_4D is the shape-adaptive transform (bm5d.cpp:276-280) and every group uses it */
    const bool all_sa = a.tau4 == 6 && !a.mask_bits.holds_all(a.A) && !(a.opt & kOptNoSaKernels);
    /* a variance table (include/lfbm5d_corr.h): the general kernels' table forms, whatever the configuration */
    if (corr_tab) return launch_group_corr(s, a, corr_tab, trace);
    /* option group_generic: test hook, every configuration through the generic LDS kernel (the dedicated kernels' cross-check) */
    if (!(a.opt & kOptGroupGeneric)) {
        bool launched = false;
        hipError_t e = launch_group_ht(s, a, all_sa, &launched, trace);
        if (launched) return e;
        e = launch_group_wiener(s, a, all_sa, &launched, trace);
        if (launched) return e;
        e = launch_group_wide(s, a, &launched, trace);
        if (launched) return e;
        e = launch_group_slab(s, a, &launched, trace);
        if (launched) return e;
    }
    const size_t lds = group_lds_bytes(a);
    if (lds > (size_t)kGenericLdsLimit || bigA) {   /* stacks in HBM scratch slices, persistent workgroups */
        const unsigned long long slice = (unsigned long long)(a.step == 2 ? 2 : 1) * a.N * a.A * a.k * a.k;
        if (!a.scratch || a.scratch_floats < slice * kBigBlocks) return hipErrorInvalidValue;
        const unsigned blocks = std::min<unsigned>(kBigBlocks, a.n_groups * a.C);
        const unsigned tf = (unsigned)group_tmp_floats(a);
        const size_t ltmp = (size_t)tf * sizeof(float) + (bigA ? (size_t)a.N * a.A * sizeof(unsigned) : 0);
        if (bigA) {
            if (a.step == 2) LFBM5D_LAUNCH(trace, (k_group_big<2, true>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf);
            else             LFBM5D_LAUNCH(trace, (k_group_big<1, true>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf);
        }
        else if (a.step == 2) LFBM5D_LAUNCH(trace, (k_group_big<2, false>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf);
        else                  LFBM5D_LAUNCH(trace, (k_group_big<1, false>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf);
        return hipGetLastError();
    }
    if (a.step == 2) LFBM5D_LAUNCH(trace, k_group<2>, dim3(a.n_groups, a.C), dim3(kThreads), lds, s, a);
    else             LFBM5D_LAUNCH(trace, k_group<1>, dim3(a.n_groups, a.C), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}
} /* namespace lfbm5d */
