/*
 * lfbm5d_group_generic.h -- one (group, channel) of the general group kernel as a device function, shared by its launches in
 * lfbm5d_group_generic.hip (k_group, k_group_big) and their variance-table forms in lfbm5d_corr.hip (k_group_corr, k_group_big_corr).
 * Internal.
 */
#ifndef LFBM5D_GROUP_GENERIC_H
#define LFBM5D_GROUP_GENERIC_H

#include "lfbm5d_group_device.h"

namespace lfbm5d {

namespace {

/* One (group, channel) of the generic path.  S0 / S1: the group's stack(s) [n][st][pq] -- in LDS (k_group) or, when the
 * stacks do not fit the 160 KiB, in a per-workgroup slice of an HBM scratch buffer (k_group_big); tmp: the 2-D stage's
 * LDS work area.  Any patch size, any transform combination, 3x3 and 5x5 angular windows.
 * CORR (include/lfbm5d_corr.h): tab [2][k*k] holds s = sqrt(v) and v, the variance factor of every 2-D coefficient under the noise's
 * autocorrelation; fibre (st, pq) is thresholded at T s[pq], Wiener-shrunk against sigma^2 v[pq] and weighted by v[pq]. */
template <int STEP, bool BIG = false, bool CORR = false>
__device__ __forceinline__ void group_generic(const GroupArgs& a, const unsigned g, const int c, float* S0, float* S1, float* tmp,
                                              unsigned* pos, float (*red)[kThreads / 64], const float* tab = nullptr) {
    const int tid = threadIdx.x;
    const int k = a.k, k2 = k * k, A = a.A, N = a.N;
    const int aw = window_side(A);
    const int nSx = (int)a.self_cnt[g];
    const size_t plane = (size_t)a.Wb * a.Hb;
    const int stack = nSx * A * k2;
    const TbPtr tb = (TbPtr)a.tb;

    /* patch positions (core:286-299) and the SADCT shape of this group (core:302-323): from the pre-pass */
    for (int i = tid; i < nSx * A; i += kThreads) pos[i] = a.gpos[(size_t)g * N * A + i];   /* up to 32 x 9 > 256 */
    typename std::conditional<BIG, ShRefBig, ShRef>::type sh = [&]() -> typename std::conditional<BIG, ShRefBig, ShRef>::type {
        if constexpr (BIG) return group_shape_big(a, g); else return group_shape(a, g); }();
    __syncthreads();
    const bool use_sadct = a.tau4 == 6 && sh.use_sadct;

    /* gather (core:286-299).  Patches whose column equals Wb-k read the reference's never-filled
     * table column, i.e. zeros (core:1697, bm3d.cpp:737) -- reproduce. */
    {
        constexpr int G = 12; /* loads in flight per thread and stack */
        for (int e0 = tid; e0 < stack; e0 += kThreads * G) {
            float v0[G], v1[G];
#pragma unroll
            for (int u = 0; u < G; u++) {
                const int e = e0 + u * kThreads;
                v0[u] = 0.0f; v1[u] = 0.0f;
                if (e < stack) {
                    const int pq = e % k2, ns = e / k2;
                    const int st = ns % A;
                    const unsigned p = pos[ns];
                    if (p != 0xffffffffu) {   /* the pre-pass folds the never-filled table column in */
                        const size_t off = ((size_t)st * a.C + c) * plane + p + (size_t)(pq / k) * a.Wb + pq % k;
                        v0[u] = a.noisy[off];
                        if (STEP == 2) v1[u] = a.basic[off];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < G; u++) {
                const int e = e0 + u * kThreads;
                if (e < stack) { S0[e] = v0[u]; if (STEP == 2) S1[e] = v1[u]; }
            }
        }
    }
    __syncthreads();

    if (a.tau2 != 4) {
        fwd2d(S0, tmp, nSx * A, k, a.tau2, tb);
        if (STEP == 2) fwd2d(S1, tmp, nSx * A, k, a.tau2, tb);
    }

    /* 4-D forward (core:353-360): one (n, pq) fibre of A values per thread */
    const bool do_dct4 = a.tau4 == 5 || (a.tau4 == 6 && !use_sadct);
    const bool do_sa4 = !do_dct4 && a.tau4 == 6;
    if (do_dct4 || do_sa4) {
        for (int f = tid; f < nSx * k2; f += kThreads) {
            const int n = f / k2, pq = f % k2;
            for (int s = 0; s < (STEP == 2 ? 2 : 1); s++) {
                float* S = s ? S1 : S0;
                if constexpr (BIG) {   /* more than 7x7 SAIs: run-time sizes, the vector in scratch memory */
                    float x[kBigA], t[kBigA];
                    for (int st = 0; st < A; st++) x[st] = S[(size_t)(n * A + st) * k2 + pq];
                    if (do_dct4) dctw_fwd_rt(x, t, aw, tb); else sadctw_fwd<ShRefBig>(x, aw, sh, tb);
                    for (int st = 0; st < A; st++) S[(size_t)(n * A + st) * k2 + pq] = x[st];
                } else
                if (A == 9) {
                    float x[9];
#pragma unroll
                    for (int st = 0; st < 9; st++) x[st] = S[(n * A + st) * k2 + pq];
                    if (do_dct4) dct9_fwd(x, tb); else sadct9_fwd(x, sh, tb);
#pragma unroll
                    for (int st = 0; st < 9; st++) S[(n * A + st) * k2 + pq] = x[st];
                } else if (do_dct4 && A == 25) {   /* 5x5 / 7x7 window, plain DCT: in registers */
                    float x[25];
#pragma unroll
                    for (int st = 0; st < 25; st++) x[st] = S[(n * 25 + st) * k2 + pq];
                    dctw_fwd_t<5>(x, tb);
#pragma unroll
                    for (int st = 0; st < 25; st++) S[(n * 25 + st) * k2 + pq] = x[st];
                } else if (do_dct4) {
                    float x[49];
#pragma unroll
                    for (int st = 0; st < 49; st++) x[st] = S[(n * 49 + st) * k2 + pq];
                    dctw_fwd_t<7>(x, tb);
#pragma unroll
                    for (int st = 0; st < 49; st++) S[(n * 49 + st) * k2 + pq] = x[st];
                } else {   /* shape-adaptive: the call form */
                    float x[kMaxA];
                    for (int st = 0; st < A; st++) x[st] = S[(n * A + st) * k2 + pq];
                    if constexpr (!BIG) sadctw_fwd<ShRef>(x, aw, sh, tb);
                    for (int st = 0; st < A; st++) S[(n * A + st) * k2 + pq] = x[st];
                }
            }
        }
        __syncthreads();
    }

    /* 5th dimension + shrinkage (core:371-410): one (st, pq) fibre of nSx values per thread */
    float wacc = 0.0f, s1 = 0.0f, s2 = 0.0f;
    {
        const float sig = a.sigma[c];
        const float T = a.bm3d ? a.lambda * sig : a.lambda * sig * 1.41421356237309505f; /* core:2431; bm3d.cpp:941 */
        const float sig2 = sig * sig;
        for (int f = tid; f < A * k2; f += kThreads) {
            const int st = f / k2, pq = f % k2;
            const bool in_shape = !use_sadct || sh.mask_dct[st];
            const int base = st * k2 + pq, stride = A * k2;
            if constexpr (CORR) {
                const float vw = tab[k2 + pq], Tc = T * tab[pq], sc = sig2 * vw;
                switch (nSx) {
                    case 1:  filter5<1, STEP, true>(S0, S1, base, stride, a.tau5, Tc, sc, in_shape, wacc, s1, s2, tb, vw); break;
                    case 2:  filter5<2, STEP, true>(S0, S1, base, stride, a.tau5, Tc, sc, in_shape, wacc, s1, s2, tb, vw); break;
                    case 4:  filter5<4, STEP, true>(S0, S1, base, stride, a.tau5, Tc, sc, in_shape, wacc, s1, s2, tb, vw); break;
                    case 8:  filter5<8, STEP, true>(S0, S1, base, stride, a.tau5, Tc, sc, in_shape, wacc, s1, s2, tb, vw); break;
                    case 16: filter5<16, STEP, true>(S0, S1, base, stride, a.tau5, Tc, sc, in_shape, wacc, s1, s2, tb, vw); break;
                    default: filter5<32, STEP, true>(S0, S1, base, stride, a.tau5, Tc, sc, in_shape, wacc, s1, s2, tb, vw); break;
                }
            } else
            switch (nSx) {
                case 1:  filter5<1, STEP>(S0, S1, base, stride, a.tau5, T, sig2, in_shape, wacc, s1, s2, tb); break;
                case 2:  filter5<2, STEP>(S0, S1, base, stride, a.tau5, T, sig2, in_shape, wacc, s1, s2, tb); break;
                case 4:  filter5<4, STEP>(S0, S1, base, stride, a.tau5, T, sig2, in_shape, wacc, s1, s2, tb); break;
                case 8:  filter5<8, STEP>(S0, S1, base, stride, a.tau5, T, sig2, in_shape, wacc, s1, s2, tb); break;
                case 16: filter5<16, STEP>(S0, S1, base, stride, a.tau5, T, sig2, in_shape, wacc, s1, s2, tb); break;
                default: filter5<32, STEP>(S0, S1, base, stride, a.tau5, T, sig2, in_shape, wacc, s1, s2, tb); break;
            }
        }
    }
    /* group weight (core:412-421, sd_weighting_5d core:3140-3173) */
    for (int o = 32; o > 0; o >>= 1) { wacc += __shfl_xor(wacc, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = wacc; red[1][tid >> 6] = s1; red[2][tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) {
        float w = 0.0f, m = 0.0f, q = 0.0f;
        for (int i = 0; i < kThreads / 64; i++) { w += red[0][i]; m += red[1][i]; q += red[2][i]; }
        float wx;
        if (a.useSD) {
            const float Nn = a.bm3d ? (float)(nSx * k2) : (float)(nSx * A);
            const float res = (q - m * m / Nn) / (Nn - 1.0f);
            wx = res > 0.0f ? 1.0f / sqrtf(res) : 0.0f;
        } else {
            const float sig = a.sigma[c];
            wx = w > 0.0f ? (sig > 0.0f ? 1.0f / (sig * sig * w) : 1.0f / w) : 1.0f;
        }
        a.wgt[(size_t)g * a.C + c] = wx;
        if (c == 0) {
            atomicAdd(&a.counters[0], (unsigned long long)nSx);
            if (use_sadct) atomicAdd(&a.counters[1], 1ull);
        }
    }
    float* F = STEP == 2 ? S1 : S0;

    /* 4-D inverse (core:431-451) */
    if (do_dct4 || do_sa4) {
        for (int f = tid; f < nSx * k2; f += kThreads) {
            const int n = f / k2, pq = f % k2;
            if constexpr (BIG) {
                float x[kBigA], t[kBigA];
                for (int st = 0; st < A; st++) x[st] = F[(size_t)(n * A + st) * k2 + pq];
                if (do_dct4) dctw_inv_rt(x, t, aw, tb); else sadctw_inv<ShRefBig>(x, aw, sh, tb);
                for (int st = 0; st < A; st++) F[(size_t)(n * A + st) * k2 + pq] = x[st];
            } else
            if (A == 9) {
                float x[9];
#pragma unroll
                for (int st = 0; st < 9; st++) x[st] = F[(n * A + st) * k2 + pq];
                if (do_dct4) dct9_inv(x, tb); else sadct9_inv(x, sh, tb);
#pragma unroll
                for (int st = 0; st < 9; st++) F[(n * A + st) * k2 + pq] = x[st];
            } else if (do_dct4 && A == 25) {
                float x[25];
#pragma unroll
                for (int st = 0; st < 25; st++) x[st] = F[(n * 25 + st) * k2 + pq];
                dctw_inv_t<5>(x, tb);
#pragma unroll
                for (int st = 0; st < 25; st++) F[(n * 25 + st) * k2 + pq] = x[st];
            } else if (do_dct4) {
                float x[49];
#pragma unroll
                for (int st = 0; st < 49; st++) x[st] = F[(n * 49 + st) * k2 + pq];
                dctw_inv_t<7>(x, tb);
#pragma unroll
                for (int st = 0; st < 49; st++) F[(n * 49 + st) * k2 + pq] = x[st];
            } else {
                float x[kMaxA];
                for (int st = 0; st < A; st++) x[st] = F[(n * A + st) * k2 + pq];
                if constexpr (!BIG) sadctw_inv<ShRef>(x, aw, sh, tb);
                for (int st = 0; st < A; st++) F[(n * A + st) * k2 + pq] = x[st];
            }
        }
    }
    __syncthreads();
    if (a.tau2 != 4) inv2d(F, tmp, nSx * A, k, a.tau2, tb);

    /* filtered patches out: [g][n][st][c][k2] */
    for (int e = tid; e < stack; e += kThreads) {
        const int pq = e % k2, ns = e / k2;
        filt_put(&a.filt[filt_patch(a, g, ns / A, ns % A, k2) + (size_t)c * k2 + pq], F[e]);
    }
}

} /* namespace */

} /* namespace lfbm5d */
#endif
