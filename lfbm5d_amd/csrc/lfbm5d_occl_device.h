/*
 * lfbm5d_occl_device.h -- the occlusion-aware plane sweep (include/lfbm5d_occl.h): beside the full set of a missing view's sources the
 * sweep evaluates the four half-planes of them and takes, per cell and hypothesis, the error of the best half-plane where it is
 * `ratio` times smaller than the full set's.  What one thread of k_view_sweep_occl does in the phases that differ from the sub-pixel
 * sweep's (the error phase and the store phase; the taps, the warp and the two box phases are lfbm5d_subpel_device.h's as they are),
 * written so that the same source compiles for the GPU and for the host: tools/occl_host_check.cpp runs it workgroup by workgroup under
 * the address and undefined-behaviour sanitizers against the numpy model (tests/occl_model.py).  Internal.
 *
 * The sets of a table row are five bit masks over its sources with their counts and the two factors r[n_k] = (float)(1.0 / n_k) and
 * g[n_k] = (float)(1.0 / (n_k - 1)); they are the same for every thread of a workgroup.  The masks are read into scalar registers
 * (uniform()), so every test of a membership is the wave's branch, not the lanes'; the factors stay where the workgroup keeps the
 * sets (LDS) and are read at each use: beside the eight taps of the holding form all of it does not fit the scalar registers.
 * Every float operation is rounded on its own (contraction off).
 */
#ifndef LFBM5D_OCCL_DEVICE_H
#define LFBM5D_OCCL_DEVICE_H

#include "lfbm5d_subpel_device.h"

#pragma clang fp contract(off)

namespace lfbm5d_occl {

using namespace lfbm5d_subpel;

constexpr int kSets = 5;                                          /* all, dt <= 0, dt >= 0, ds <= 0, ds >= 0 */
constexpr int kCnt = kHist + kSets;                               /* the kernel's counters: positions per j* + 32, then per k* */

/* mask[k]: the members of set k, bit q = source q of the row; 0 for a candidate that is not admissible (2 <= n_k < n), so that no
 * member of it is ever found.  adm: bit k = candidate k is admissible.  count[k] = n_k whether admissible or not. */
struct Sets { unsigned mask[kSets]; int count[kSets]; float rn[kSets], gn[kSets]; unsigned adm; };

LFBM5D_HD Sets make_sets(const int* tab) {
    Sets s;
    const int n = tab[1];
    unsigned m[kSets] = {0u, 0u, 0u, 0u, 0u};
    for (int q = 0; q < n; q++) {
        const int ds = tab[3 + 3 * q], dt = tab[4 + 3 * q];
        const unsigned bit = 1u << q;
        m[0] |= bit;
        if (dt <= 0) m[1] |= bit;
        if (dt >= 0) m[2] |= bit;
        if (ds <= 0) m[3] |= bit;
        if (ds >= 0) m[4] |= bit;
    }
    s.adm = 0u;
    for (int k = 0; k < kSets; k++) {
        int nk = 0;
        for (int q = 0; q < n; q++) nk += (int)((m[k] >> q) & 1u);
        const bool use = k == 0 || (nk >= 2 && nk < n);
        if (k && use) s.adm |= 1u << k;
        s.mask[k] = use ? m[k] : 0u;
        s.count[k] = nk;
        s.rn[k] = nk >= 1 ? (float)(1.0 / (double)nk) : 0.0f;
        s.gn[k] = nk >= 2 ? (float)(1.0 / (double)(nk - 1)) : 0.0f;
    }
    return s;
}

/* what a thread keeps of the workgroup's sets: the masks and adm as uniform values, and where the rest lies */
struct SetView { unsigned mask[kSets]; unsigned adm; const Sets* at; };
LFBM5D_HD SetView view_of(const Sets& a) {
    SetView s;
#pragma unroll
    for (int k = 0; k < kSets; k++) s.mask[k] = (unsigned)lfbm5d_subpel::uniform((int)a.mask[k]);
    s.adm = (unsigned)lfbm5d_subpel::uniform((int)a.adm);
    s.at = &a;
    return s;
}

/* A uniform value whose tests are to be made where they are used: on the GPU the compiler otherwise forms every (mask >> q) & 1 and
 * every q < n of the unrolled loops ahead of the hypothesis loop, about a hundred scalar values that do not fit the scalar registers and
 * are spilled into vector lanes; behind this it keeps the six words and tests a bit with one scalar instruction. */
LFBM5D_HD unsigned here(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    v = (unsigned)lfbm5d_subpel::uniform((int)v);
    asm volatile("" : "+s"(v));
#endif
    return v;
}

/* where the taps of a cell come from: the workgroup's table of the current hypothesis, or the table row for a j of the cell's own */
struct TableTaps {
    const Tap* taps;
    LFBM5D_HD Tap operator()(int q) const { return lfbm5d_subpel::uniform(taps[q]); }
};
struct RowTaps {
    const int* tab;
    int j, Q;
    LFBM5D_HD Tap operator()(int q) const { return make_tap(tab, q, j, Q); }
};

/* e^_k(y, x) = g[n_k] sum_c sum_{q in k} (w_q - mu_k)^2 for the sets that are evaluated (0 elsewhere), c outer, q inner, from +0;
 * mu_k = (((+0 + w_a) + w_b) + ...) r[n_k] over the members in order.  HOLD (n <= kHold): a channel's warped values stay in registers
 * while the five means and scatters are formed (loops unrolled over kHold, no array indexed by a variable); otherwise every source is
 * warped once for the five sums and once more for the five scatters. */
template <bool HOLD, class Taps>
LFBM5D_HD void cell_errors(const float* __restrict__ in, const Taps& taps, const SetView& s, int n_row, int C, int y, int x, int W, int H,
                           float (&eh)[kSets]) {
    const size_t plane = (size_t)W * H;
    const int n = (int)here((unsigned)n_row);
    float v[kSets];
    unsigned mk[kSets];
#pragma unroll
    for (int k = 0; k < kSets; k++) { v[k] = 0.0f; mk[k] = here(s.mask[k]); }
    for (int c = 0; c < C; c++) {
        if (HOLD) {
            float w[kHold];
#pragma unroll
            for (int q = 0; q < kHold; q++)
                if ((here(s.mask[0]) >> q) & 1u) {                              /* q < n */
                    const Tap t = taps(q);
                    w[q] = warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H);
                }
#pragma unroll
            for (int k = 0; k < kSets; k++) {
                if (!mk[k]) continue;
                float sum = 0.0f;
#pragma unroll
                for (int q = 0; q < kHold; q++)
                    if ((here(mk[k]) >> q) & 1u) sum = sum + w[q];
                const float mu = sum * s.at->rn[k];
#pragma unroll
                for (int q = 0; q < kHold; q++)
                    if ((here(mk[k]) >> q) & 1u) {
                        const float diff = w[q] - mu;
                        const float sq = diff * diff;
                        v[k] = v[k] + sq;
                    }
            }
        } else {
            float mu[kSets];
#pragma unroll
            for (int k = 0; k < kSets; k++) mu[k] = 0.0f;
            for (int q = 0; q < n; q++) {
                const Tap t = taps(q);
                const float w = warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H);
#pragma unroll
                for (int k = 0; k < kSets; k++)
                    if ((mk[k] >> q) & 1u) mu[k] = mu[k] + w;
            }
#pragma unroll
            for (int k = 0; k < kSets; k++) mu[k] = mu[k] * s.at->rn[k];
            for (int q = 0; q < n; q++) {
                const Tap t = taps(q);
                const float w = warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H);
#pragma unroll
                for (int k = 0; k < kSets; k++)
                    if ((mk[k] >> q) & 1u) {
                        const float diff = w - mu[k];
                        const float sq = diff * diff;
                        v[k] = v[k] + sq;
                    }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kSets; k++) eh[k] = v[k] * s.at->gn[k];
}

/* k* of a cell and e = e^_{k*}: among the admissible candidates in order a later one replaces the best so far only if strictly smaller;
 * the best replaces set 0 only if (e^_best ratio) < e^_0, the product rounded */
LFBM5D_HD int choose(const float (&eh)[kSets], unsigned adm_row, float ratio, float& e) {
    const unsigned adm = here(adm_row);
    int kb = 0;
    float eb = 0.0f;
#pragma unroll
    for (int k = 1; k < kSets; k++)
        if ((adm >> k) & 1u) {
            if (kb == 0 || eh[k] < eb) { eb = eh[k]; kb = k; }
        }
    e = eh[0];
    if (kb) {
        const float prod = eb * ratio;
        if (prod < eh[0]) { e = eb; return kb; }
    }
    return 0;
}

/* phase 1 of a hypothesis: e_j = e^_{k*} of the tile at (x0, y0) plus a halo of r into e [kEH][kEW]; a cell outside the plane is computed
 * at the position it mirrors (the same operands, the same bits) */
template <bool HOLD>
LFBM5D_HD void error_phase(const float* __restrict__ in, const Tap* taps, const SetView& s, int n, float ratio, int C, int W, int H, int x0,
                           int y0, int r, int tid, float* e) {
    const int ew = kTW + 2 * r, eh_ = kTH + 2 * r;
    const TableTaps from = {taps};
    for (int i = tid; i < ew * eh_; i += kThreads) {
        const int wy = i / ew, wx = i - wy * ew;
        float eh[kSets], chosen;
        cell_errors<HOLD>(in, from, s, n, C, mirror(y0 - r + wy, H), mirror(x0 - r + wx, W), W, H, eh);
        (void)choose(eh, s.adm, ratio, chosen);
        e[wy * kEW + wx] = chosen;
    }
}

/* the last phase: per position of this thread the choice is made again for the cell itself at its j*; the mean of the chosen set goes
 * into out, j* into disp (or NULL), k* into set (or NULL), j* + 32 and kHist + k* are counted in cnt [kCnt].  j* differs from lane to
 * lane, so the taps are made per source from the table row and nothing is held.  The phase runs once per position, so its loop over
 * the thread's positions is not unrolled (one copy of the code, not eight); j* of position k is jstar[k * jstride], of any type that
 * converts to int (the kernel parks its register array in the error plane, which is free by then, to index it by a variable). */
template <class J, class Add>
LFBM5D_HD void store_phase(const float* __restrict__ in, float* __restrict__ out, signed char* __restrict__ disp,
                           unsigned char* __restrict__ set, const int* __restrict__ tab, const SetView& s, float ratio, int Q, int C, int W,
                           int H, int x0, int y0, int tid, const J* jstar, int jstride, unsigned* cnt, Add add) {
    const size_t plane = (size_t)W * H;
    const int m = tab[0], n = tab[1];
    const int gx = x0 + (tid & (kTW - 1));
#pragma unroll 1
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gx >= W || gy >= H) continue;
        const size_t at = (size_t)gy * W + gx;
        const int j = (int)jstar[k * jstride];
        const RowTaps from = {tab, j, Q};
        float eh[kSets], chosen;
        cell_errors<false>(in, from, s, n, C, gy, gx, W, H, eh);
        const int ks = choose(eh, s.adm, ratio, chosen);
        const unsigned members = s.at->mask[ks];
        const float rn = s.at->rn[ks];
        for (int c = 0; c < C; c++) {
            float sum = 0.0f;
            for (int q = 0; q < n; q++) {
                if (!((members >> q) & 1u)) continue;
                const Tap t = from(q);
                sum = sum + warp(in + ((size_t)t.src * C + c) * plane, t, gy, gx, W, H);
            }
            out[((size_t)m * C + c) * plane + at] = sum * rn;
        }
        if (disp) disp[(size_t)m * plane + at] = (signed char)j;
        if (set) set[(size_t)m * plane + at] = (unsigned char)ks;
        add(&cnt[j + kJMax]);
        add(&cnt[kHist + ks]);
    }
}

} /* namespace lfbm5d_occl */
#endif
