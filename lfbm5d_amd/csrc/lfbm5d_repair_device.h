/*
 * lfbm5d_repair_device.h -- what one thread of the joint repair's kernels does (lfbm5d_repair.hip, include/lfbm5d_repair.h), written
 * so that the same source compiles for the GPU and for the host: tools/repair_host_check.cpp runs it under the address and
 * undefined-behaviour sanitizers against the numpy model before the kernels meet a GPU.  Internal.
 *
 * The tile, the thread-owns-a-column layout and the three phases per hypothesis are k_view_sweep's (lfbm5d_view.hip); beside every
 * float plane in LDS lies a 16-bit plane with the number of evidence cells, which goes through both box passes with the error.
 * Every float operation is rounded on its own (contraction off).
 */
#ifndef LFBM5D_REPAIR_DEVICE_H
#define LFBM5D_REPAIR_DEVICE_H

#include "lfbm5d_side_values.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace lfbm5d_repair {

using namespace lfbm5d_side;                                      /* the tile, mirror, the bit tests */

constexpr int kRMax = 7, kDMax = 8, kSrcMax = 24;                 /* box radius, disparity, sources at ang_radius 2 */
constexpr int kEW = kTW + 2 * kRMax, kEH = kTH + 2 * kRMax;       /* the error plane: tile + halo, 78 x 46 */
constexpr int kPer = kTW * kTH / kThreads;                        /* 8 positions per thread */
constexpr int kRowStep = kThreads / kTW;                          /* 4 */
constexpr int kHist = 2 * kDMax + 1;
constexpr int kTabStride = 2 + 3 * kSrcMax;                       /* per target: its index, n, n x (source index, ds, dt) */
constexpr int kBoxMax = (2 * kRMax + 1) * (2 * kRMax + 1);        /* 225 cells */
/* the float tables, one buffer: r[k] = (float)(1.0 / k), k = 0..24 (r[0] = 0); f[n][k] = (float)((n - 1.0) / (k - 1.0)), n, k = 0..24
 * (0 where k < 2); g[k] = (float)((2r + 1)^2 / (double)k), k = 0..225 for the call's r (g[0] = 0) */
constexpr int kTabR = 0, kTabF = kSrcMax + 1, kTabG = kTabF + (kSrcMax + 1) * (kSrcMax + 1), kTabFloats = kTabG + kBoxMax + 1;
static_assert(kTW * kTH % kThreads == 0 && kThreads % kTW == 0, "a thread owns one column");

/* hypothesis j = 0..2D -> d: 0, -1, +1, -2, +2, ... */
LFBM5D_HD int hypothesis(int j) { return (j & 1) ? -((j + 1) >> 1) : (j >> 1); }

/* What a workgroup reads: the light field, the validity planes [asize][H*W], one row of the source table, the float tables. */
struct Sweep {
    const float* in;
    const unsigned char* valid;
    const int* tab;
    const float* tables;
    int n, C, W, H;
};

/* bit q: source q of the row is valid at the position hypothesis d warps (y, x) to */
LFBM5D_HD unsigned valid_bits(const Sweep& s, int d, int y, int x) {
    const size_t plane = (size_t)s.W * s.H;
    unsigned bits = 0;
    for (int q = 0; q < s.n; q++) {
        const int sy = mirror(y - d * s.tab[3 + 3 * q], s.H), sx = mirror(x - d * s.tab[4 + 3 * q], s.W);
        bits |= s.valid[(size_t)s.tab[2 + 3 * q] * plane + (size_t)sy * s.W + sx] ? 1u << q : 0u;
    }
    return bits;
}

/* S: the valid warped values of channel c in source order from +0; an invalid one is passed over by a select */
LFBM5D_HD float valid_sum(const Sweep& s, unsigned bits, int d, int c, int y, int x) {
    const size_t plane = (size_t)s.W * s.H;
    float sum = 0.0f;
    for (int q = 0; q < s.n; q++) {
        const int sy = mirror(y - d * s.tab[3 + 3 * q], s.H), sx = mirror(x - d * s.tab[4 + 3 * q], s.W);
        const float w = s.in[((size_t)s.tab[2 + 3 * q] * s.C + c) * plane + (size_t)sy * s.W + sx];
        const float next = sum + w;
        sum = (bits >> q) & 1u ? next : sum;
    }
    return sum;
}

/* e'_d(y, x) and whether the cell carries evidence (n_d >= 2) */
LFBM5D_HD float cell_error(const Sweep& s, int d, int y, int x, unsigned& evidence) {
    const size_t plane = (size_t)s.W * s.H;
    const unsigned bits = valid_bits(s, d, y, x);
    const int nd = __builtin_popcount(bits);
    evidence = nd >= 2 ? 1u : 0u;
    if (nd < 2) return 0.0f;
    const float rn = s.tables[kTabR + nd];
    float e = 0.0f;
    for (int c = 0; c < s.C; c++) {
        const float mu = valid_sum(s, bits, d, c, y, x) * rn;
        for (int q = 0; q < s.n; q++) {
            const int sy = mirror(y - d * s.tab[3 + 3 * q], s.H), sx = mirror(x - d * s.tab[4 + 3 * q], s.W);
            const float diff = s.in[((size_t)s.tab[2 + 3 * q] * s.C + c) * plane + (size_t)sy * s.W + sx] - mu;
            const float sq = diff * diff;
            const float next = e + sq;
            e = (bits >> q) & 1u ? next : e;
        }
    }
    return e * s.tables[kTabF + s.n * (kSrcMax + 1) + nd];
}

/* the scaled error and the evidence of the tile plus a halo of r into e / ke (rows of kEW); a cell outside the plane is computed at
 * the position it mirrors */
LFBM5D_HD void error_phase(const Sweep& s, int d, int x0, int y0, int r, int tid, float* e, unsigned short* ke) {
    const int ew = kTW + 2 * r, eh = kTH + 2 * r;
    for (int i = tid; i < ew * eh; i += kThreads) {
        const int wy = i / ew, wx = i - wy * ew;
        unsigned ev;
        e[wy * kEW + wx] = cell_error(s, d, mirror(y0 - r + wy, s.H), mirror(x0 - r + wx, s.W), ev);
        ke[wy * kEW + wx] = (unsigned short)ev;
    }
}

/* h(row, x) = sum_k e(row, x + k), the counts beside it */
LFBM5D_HD void hbox_phase(const float* e, const unsigned short* ke, float* h, unsigned short* kh, int r, int tid) {
    const int eh = kTH + 2 * r;
    for (int i = tid; i < eh * kTW; i += kThreads) {
        const int at = (i / kTW) * kEW + (i & (kTW - 1));
        float sum = 0.0f;
        unsigned cnt = 0;
        for (int k = 0; k <= 2 * r; k++) { sum = sum + e[at + k]; cnt += ke[at + k]; }
        h[i] = sum;
        kh[i] = (unsigned short)cnt;
    }
}

/* E(y, x) = S_k = 0 ? +inf : (sum_k h(y + k, x)) g[S_k], and the running (E_best, d*) of this thread's positions */
LFBM5D_HD void vbox_phase(const Sweep& s, const float* h, const unsigned short* kh, int r, int tid, bool first, int d, float* best, int* dstar) {
    const int lx = tid & (kTW - 1), ly0 = tid / kTW;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int at = (ly0 + k * kRowStep) * kTW + lx;
        float sum = 0.0f;
        unsigned cnt = 0;
        for (int kk = 0; kk <= 2 * r; kk++) { sum = sum + h[at + kk * kTW]; cnt += kh[at + kk * kTW]; }
        const float scaled = sum * s.tables[kTabG + cnt];
        const float E = cnt ? scaled : __builtin_inff();
        if (first || E < best[k]) { best[k] = E; dstar[k] = d; }
    }
}

/* The unsound values of this thread's positions of target m become mu_{d*} where n_{d*} >= min_valid: written into mid, their flag in
 * rem cleared.  dstar[k * stride], k = 0..7: this thread's d* as floats (the kernel keeps them in LDS, so that this loop can index them
 * by a variable without scratch).  d* of every unsound position goes to disp (or NULL); hist[d* + 8] counts the positions that got a value. */
template <class Add>
LFBM5D_HD void store_phase(const Sweep& s, int m, int min_valid, float* mid, unsigned char* rem, signed char* disp, int x0, int y0, int tid,
                           const float* dstar, int stride, unsigned* hist, Add add) {
    const size_t plane = (size_t)s.W * s.H;
    const int gx = x0 + (tid & (kTW - 1));
    if (gx >= s.W) return;
#pragma unroll 1
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gy >= s.H) break;
        const size_t at = (size_t)gy * s.W + gx;
        if (s.valid[(size_t)m * plane + at]) continue;
        const int d = (int)dstar[k * stride];
        if (disp) disp[(size_t)m * plane + at] = (signed char)d;
        const unsigned bits = valid_bits(s, d, gy, gx);
        const int nd = __builtin_popcount(bits);
        if (nd < min_valid) continue;
        const float rn = s.tables[kTabR + nd];
        for (int c = 0; c < s.C; c++) {
            const size_t v = ((size_t)m * s.C + c) * plane + at;
            if (!rem[v]) continue;
            mid[v] = valid_sum(s, bits, d, c, gy, gx) * rn;
            rem[v] = 0;
        }
        add(&hist[d + kDMax]);
    }
}

/* The validity of this thread's positions of SAI q: valid[q] = 1 where every channel's value is sound; rem = 1 on every unsound value
 * (the SAI is missing, the value is flagged or not finite); mid = a copy of in.  Returns the thread's unsound positions. */
LFBM5D_HD unsigned valid_thread(const float* __restrict__ in, const unsigned char* __restrict__ flags, bool missing, int q, int C, int W, int H,
                                int x0, int y0, int tid, unsigned char* __restrict__ valid, float* __restrict__ mid,
                                unsigned char* __restrict__ rem) {
    const size_t plane = (size_t)W * H;
    const int gx = x0 + (tid & (kTW - 1));
    unsigned unsound = 0;
    if (gx >= W) return 0;
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gy >= H) break;
        const size_t at = (size_t)gy * W + gx;
        bool any = false;
        for (int c = 0; c < C; c++) {
            const size_t v = ((size_t)q * C + c) * plane + at;
            const float val = in[v];
            const bool bad = missing || (flags && flags[v]) || !finite_bits(val);
            mid[v] = val;
            rem[v] = bad ? 1 : 0;
            any = any || bad;
        }
        valid[(size_t)q * plane + at] = any ? 0 : 1;
        unsound += any ? 1u : 0u;
    }
    return unsound;
}

/* the code of a value: st = what the onion-peel fill says of it (0 untouched, 1 filled, 2 left); a value it did not touch that was
 * unsound was filled from the other views */
LFBM5D_HD unsigned code_of(unsigned st, bool unsound) { return st ? st + 1u : (unsound ? 1u : 0u); }

} /* namespace lfbm5d_repair */
#endif
