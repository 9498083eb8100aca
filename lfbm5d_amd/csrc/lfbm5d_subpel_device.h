/*
 * lfbm5d_subpel_device.h -- the sub-pixel warp of the plane sweep (hypotheses d = j / Q, bilinear interpolation; include/lfbm5d.h) and
 * what one thread of k_view_sweep_subpel does in each of its phases (lfbm5d_view.hip), written so that the same source compiles for
 * the GPU and for the host: the consistency check's flag_thread (lfbm5d_consist_device.h) takes its spread from the same warp, and
 * tools/subpel_host_check.cpp runs the phases workgroup by workgroup under the address and undefined-behaviour sanitizers against the
 * numpy model (tests/subpel_model.py) before the kernel meets a GPU.  Internal.
 *
 * A workgroup of 256 threads owns a tile of 64 x 32 positions of one synthesised SAI; a thread owns one column of it and every fourth
 * row, so the lanes of a wave run along x in every phase.  Every float operation is rounded on its own (contraction off).
 */
#ifndef LFBM5D_SUBPEL_DEVICE_H
#define LFBM5D_SUBPEL_DEVICE_H

#include "lfbm5d_side_values.h"

#pragma clang fp contract(off)

namespace lfbm5d_subpel {

using namespace lfbm5d_side;                                      /* the tile, mirror */

constexpr int kRMax = 7, kDMax = 8, kQMax = 4, kSrcMax = 24;      /* box radius, disparity, steps per pixel, sources at ang_radius 2 */
constexpr int kJMax = kDMax * kQMax, kHist = 2 * kJMax + 1;       /* |j*| <= 32; LFBM5D_VIEW_STEPS_HIST bins, index j* + 32 */
constexpr int kTabStride = 2 + 3 * kSrcMax;                       /* the sweep's table: SAI, n, n x (source, ds, dt) */
constexpr int kEW = kTW + 2 * kRMax, kEH = kTH + 2 * kRMax;       /* the error plane: tile + halo, 78 x 46 */
constexpr int kPer = kTW * kTH / kThreads, kRowStep = kThreads / kTW;   /* 8 positions per thread, 4 rows apart */
constexpr int kHold = 8;                                          /* up to this many sources a channel's warped values stay in registers */
static_assert(kTW * kTH % kThreads == 0 && kThreads % kTW == 0, "a thread owns one column");

/* the j-th hypothesis in the order 0, -1, +1, -2, +2, ... */
LFBM5D_HD int hypothesis(int i) { return (i & 1) ? -((i + 1) >> 1) : (i >> 1); }

/* What hypothesis j makes of one source: Q y - j ds = Q (y + oy) + py with 0 <= py < Q, the same along x; the weights p / Q are exact.
 * None of it depends on the position. */
struct Tap { int src, oy, ox, py, px; float wy, wx; };

LFBM5D_HD Tap make_tap(const int* tab, int q, int j, int Q) {
    Tap t;
    t.src = tab[2 + 3 * q];
    const int ny = -j * tab[3 + 3 * q], nx = -j * tab[4 + 3 * q];
    t.oy = ny >= 0 ? ny / Q : -((-ny + Q - 1) / Q);               /* floor */
    t.ox = nx >= 0 ? nx / Q : -((-nx + Q - 1) / Q);
    t.py = ny - Q * t.oy;
    t.px = nx - Q * t.ox;
    t.wy = (float)t.py / (float)Q;
    t.wx = (float)t.px / (float)Q;
    return t;
}

/* a value that is the same in every lane of a wave (a tap of the workgroup's table): on the GPU it moves to a scalar register, so that
 * the branches on the fractions are the wave's, not the lanes' */
LFBM5D_HD int uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}
LFBM5D_HD Tap uniform(const Tap& t) { return Tap{uniform(t.src), uniform(t.oy), uniform(t.ox), uniform(t.py), uniform(t.px), t.wy, t.wx}; }

/* a + w (b - a) */
LFBM5D_HD float lerp(float a, float b, float w) {
    const float diff = b - a;
    const float prod = w * diff;
    return a + prod;
}

/* w_{q,j}(y, x) of the plane I [H][W]: 1 value where both fractions are 0, 2 where one is, 4 otherwise; every index mirrored on its own */
LFBM5D_HD float warp(const float* __restrict__ I, const Tap& t, int y, int x, int W, int H) {
    const int iy = y + t.oy, ix = x + t.ox;
    const int c0 = mirror(ix, W);
    const float* __restrict__ r0 = I + (size_t)mirror(iy, H) * W;
    if (t.px == 0) {
        if (t.py == 0) return r0[c0];
        return lerp(r0[c0], I[(size_t)mirror(iy + 1, H) * W + c0], t.wy);
    }
    const int c1 = mirror(ix + 1, W);
    const float top = lerp(r0[c0], r0[c1], t.wx);
    if (t.py == 0) return top;
    const float* __restrict__ r1 = I + (size_t)mirror(iy + 1, H) * W;
    const float bot = lerp(r1[c0], r1[c1], t.wx);
    return lerp(top, bot, t.wy);
}

/* e_j(y, x) = sum_c sum_q (w_{q,j} - mu_j)^2, c outer, q inner, from +0; mu_j = (((+0 + w_1) + w_2) + ...) rn.  HOLD: the n <= kHold
 * warped values of a channel stay in registers between the mean and the deviations (the loops are unrolled over kHold, no array is
 * indexed by a variable); otherwise they are computed again. */
template <bool HOLD>
LFBM5D_HD float cell_error(const float* __restrict__ in, const Tap* taps, int n, float rn, int C, int y, int x, int W, int H) {
    const size_t plane = (size_t)W * H;
    float e = 0.0f;
    for (int c = 0; c < C; c++) {
        if (HOLD) {
            float w[kHold];
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < kHold; q++)
                if (q < n) {
                    const Tap t = uniform(taps[q]);
                    w[q] = warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H);
                    s = s + w[q];
                }
            const float mu = s * rn;
#pragma unroll
            for (int q = 0; q < kHold; q++)
                if (q < n) {
                    const float diff = w[q] - mu;
                    const float sq = diff * diff;
                    e = e + sq;
                }
        } else {
            float s = 0.0f;
            for (int q = 0; q < n; q++) {
                const Tap t = uniform(taps[q]);
                s = s + warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H);
            }
            const float mu = s * rn;
            for (int q = 0; q < n; q++) {
                const Tap t = uniform(taps[q]);
                const float diff = warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H) - mu;
                const float sq = diff * diff;
                e = e + sq;
            }
        }
    }
    return e;
}

/* phase 1 of a hypothesis: the error plane of the tile at (x0, y0) plus a halo of r into e [kEH][kEW]; a cell outside the plane is
 * computed at the position it mirrors (the same operands, the same bits) */
template <bool HOLD>
LFBM5D_HD void error_phase(const float* __restrict__ in, const Tap* taps, int n, float rn, int C, int W, int H, int x0, int y0, int r, int tid,
                           float* e) {
    const int ew = kTW + 2 * r, eh = kTH + 2 * r;
    for (int i = tid; i < ew * eh; i += kThreads) {
        const int wy = i / ew, wx = i - wy * ew;
        e[wy * kEW + wx] = cell_error<HOLD>(in, taps, n, rn, C, mirror(y0 - r + wy, H), mirror(x0 - r + wx, W), W, H);
    }
}

/* phase 2: h(row, x) = sum_k e(row, x + k), window columns x .. x + 2r, into h [kEH][kTW] */
LFBM5D_HD void hbox_phase(const float* e, float* h, int r, int tid) {
    const int eh = kTH + 2 * r;
    for (int i = tid; i < eh * kTW; i += kThreads) {
        const float* row = e + (i / kTW) * kEW + (i & (kTW - 1));
        float s = 0.0f;
        for (int k = 0; k <= 2 * r; k++) s = s + row[k];
        h[i] = s;
    }
}

/* phase 3: E(y, x) = sum_k h(y + k, x), window rows y .. y + 2r, and the running (E_best, j*): replaced only by a strictly smaller E */
LFBM5D_HD void vbox_phase(const float* h, int r, int tid, bool first, int j, float (&best)[kPer], int (&jstar)[kPer]) {
    const int lx = tid & (kTW - 1), ly0 = tid / kTW;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const float* col = h + (ly0 + k * kRowStep) * kTW + lx;
        float s = 0.0f;
        for (int kk = 0; kk <= 2 * r; kk++) s = s + col[kk * kTW];
        if (first || s < best[k]) { best[k] = s; jstar[k] = j; }
    }
}

/* mu_{j}(c, y, x) from the sources of the table row tab, for a j that varies from position to position */
LFBM5D_HD float warped_mean(const float* __restrict__ in, const int* __restrict__ tab, int n, float rn, int j, int Q, int c, int C, int y, int x,
                            int W, int H) {
    const size_t plane = (size_t)W * H;
    float s = 0.0f;
    for (int q = 0; q < n; q++) {
        const Tap t = make_tap(tab, q, j, Q);
        s = s + warp(in + ((size_t)t.src * C + c) * plane, t, y, x, W, H);
    }
    return s * rn;
}

/* the last phase: the mean at j* of this thread's positions into out, j* into disp (or NULL), j* + 32 counted in hist [kHist] */
template <class Add>
LFBM5D_HD void store_phase(const float* __restrict__ in, float* __restrict__ out, signed char* __restrict__ disp, const int* __restrict__ tab,
                           float rn, int Q, int C, int W, int H, int x0, int y0, int tid, const int (&jstar)[kPer], unsigned* hist, Add add) {
    const size_t plane = (size_t)W * H;
    const int m = tab[0], n = tab[1];
    const int gx = x0 + (tid & (kTW - 1));
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gx >= W || gy >= H) continue;
        const size_t at = (size_t)gy * W + gx;
        for (int c = 0; c < C; c++) out[((size_t)m * C + c) * plane + at] = warped_mean(in, tab, n, rn, jstar[k], Q, c, C, gy, gx, W, H);
        if (disp) disp[(size_t)m * plane + at] = (signed char)jstar[k];
        add(&hist[jstar[k] + kJMax]);
    }
}

} /* namespace lfbm5d_subpel */
#endif
