/*
 * lfbm5d_consist_device.h -- what one thread of the consistency check's two kernels does with its values (lfbm5d_consist.hip), written so
 * that the same source compiles for the GPU and for the host: tools/consist_host_check.cpp runs it under the address and
 * undefined-behaviour sanitizers against the numpy model before the kernels meet a GPU.  Internal.
 *
 * A workgroup of 256 threads owns a tile of 64 x 32 positions of one tested SAI; a thread owns one column of it and every fourth row
 * (8 positions, all channels), so the lanes of a wave run along x.  Every float operation is rounded on its own (contraction off).
 */
#ifndef LFBM5D_CONSIST_DEVICE_H
#define LFBM5D_CONSIST_DEVICE_H

#include "lfbm5d_side_values.h"
#include "lfbm5d_subpel_device.h"

#pragma clang fp contract(off)

namespace lfbm5d_consist {

using namespace lfbm5d_side;                                      /* the tile, the key layout, the thresholds, mirror, the bit tests */

constexpr int kPer = kTW * kTH / kThreads;                        /* 8 positions per thread */
constexpr int kRowStep = kThreads / kTW;                          /* 4 */
constexpr int kSrcMax = 24, kTabStride = 2 + 3 * kSrcMax;         /* k_view_sweep's table: SAI, n, n x (source, ds, dt) */
static_assert(kTW * kTH % kThreads == 0 && kThreads % kTW == 0, "a thread owns one column");

LFBM5D_HD float abs_bits(float x) { return __builtin_bit_cast(float, bits_of(x) & 0x7fffffffu); }

/* key of a >= 0 (or a NaN, whose bits land in the last key): clamp((bits >> 19) - base + 1, 0, 385) */
LFBM5D_HD int key_of(float a) {
    const int k = (int)(bits_of(a) >> 19) - kKeyBase + 1;
    return k < 0 ? 0 : k > kKeys - 1 ? kKeys - 1 : k;
}

/* The statistics of one thread's values: the key of a = |I_m - mu| goes into hist [C][386] (the workgroup's counters), a non-finite I_m
 * into *skip.  in / pred: the light field and its prediction, [asize][C][H][W]; (x0, y0) the tile's origin. */
template <class Add>
LFBM5D_HD void stats_thread(const float* __restrict__ in, const float* __restrict__ pred, int m, int C, int W, int H, int x0, int y0, int tid,
                            unsigned* hist, unsigned* skip, Add add) {
    const size_t plane = (size_t)W * H;
    const int gx = x0 + (tid & (kTW - 1));
    if (gx >= W) return;
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gy >= H) break;
        for (int c = 0; c < C; c++) {
            const size_t at = ((size_t)m * C + c) * plane + (size_t)gy * W + gx;
            const float v = in[at];
            if (!finite_bits(v)) { add(skip); continue; }
            const float rho = v - pred[at];
            add(&hist[c * kKeys + key_of(abs_bits(rho))]);
        }
    }
}

/* The decision of one thread's values.  tab: the SAI's row of the sweep's table; disp: d* [asize][H][W]; flags: [asize][C][H][W];
 * g = (float)(spread^2); cnt [3][2]: the workgroup's counters of code 1 and code 2 per channel.
 * code 2: I_m is not finite.  code 1: a > T_c and (rho rho) (float)(n - 1) > g v, v = sum_q (w_{q,d*} - mu)^2 from +0 in source order.
 * SUBPEL: disp holds j* in units of 1 / Q and w is the sweep's interpolated warp (lfbm5d_subpel_device.h); otherwise Q is not looked at. */
template <bool SUBPEL = false, class Add>
LFBM5D_HD void flag_thread(const float* __restrict__ in, const float* __restrict__ pred, const signed char* __restrict__ disp,
                           unsigned char* __restrict__ flags, const int* __restrict__ tab, int C, int W, int H, int x0, int y0, int tid,
                           Thresholds thr, float g, unsigned* cnt, Add add, int Q = 1) {
    const size_t plane = (size_t)W * H;
    const int m = tab[0], n = tab[1];
    const float n1 = (float)(n - 1);
    const int gx = x0 + (tid & (kTW - 1));
    if (gx >= W) return;
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gy >= H) break;
        const size_t pos = (size_t)gy * W + gx;
        const int d = (int)disp[(size_t)m * plane + pos];
        for (int c = 0; c < C; c++) {
            const size_t at = ((size_t)m * C + c) * plane + pos;
            const float val = in[at], mu = pred[at];
            unsigned char code = 0;
            if (!finite_bits(val)) code = 2;
            else {
                float v = 0.0f;
                for (int q = 0; q < n; q++) {
                    float w;
                    if (SUBPEL) {
                        const lfbm5d_subpel::Tap t = lfbm5d_subpel::make_tap(tab, q, d, Q);
                        w = lfbm5d_subpel::warp(in + ((size_t)t.src * C + c) * plane, t, gy, gx, W, H);
                    } else {
                        const int sy = mirror(gy - d * tab[3 + 3 * q], H), sx = mirror(gx - d * tab[4 + 3 * q], W);
                        w = in[((size_t)tab[2 + 3 * q] * C + c) * plane + (size_t)sy * W + sx];
                    }
                    const float diff = w - mu;
                    const float sq = diff * diff;
                    v = v + sq;
                }
                const float rho = val - mu;
                const float a = abs_bits(rho);
                const float rr = rho * rho;
                const float lhs = rr * n1;
                const float rhs = g * v;
                const float T = c == 0 ? thr.t[0] : c == 1 ? thr.t[1] : thr.t[2];
                if (a > T && lhs > rhs) code = 1;
            }
            flags[at] = code;
            if (code) add(&cnt[c * 2 + (code - 1)]);
        }
    }
}

} /* namespace lfbm5d_consist */
#endif
