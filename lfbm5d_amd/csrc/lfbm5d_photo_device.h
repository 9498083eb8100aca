/*
 * lfbm5d_photo_device.h -- what one thread of the photometric equalisation's two kernels does with its values (lfbm5d_photo.hip),
 * written so that the same source compiles for the GPU and for the host: tools/photo_host_check.cpp runs it under the address and
 * undefined-behaviour sanitizers against the numpy model before the kernels meet a GPU.  Internal.
 *
 * Statistics: a workgroup of 256 threads owns a tile of 64 x 32 positions of one tested SAI; a thread owns one column of it and every
 * fourth row (8 positions, all channels), so the lanes of a wave run along x and the loads of I and mu are coalesced.  Every float
 * operation is rounded on its own (contraction off).
 */
#ifndef LFBM5D_PHOTO_DEVICE_H
#define LFBM5D_PHOTO_DEVICE_H

#include "lfbm5d_side_values.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace lfbm5d_photo {

using namespace lfbm5d_side;                                      /* the tile, mirror, the bit tests */

constexpr int kEdges = 1025, kRatioKeys = kEdges + 1;             /* LFBM5D_PHOTO_EDGES, LFBM5D_PHOTO_KEYS */
constexpr int kPer = kTW * kTH / kThreads;                        /* 8 positions per thread */
constexpr int kRowStep = kThreads / kTW;                          /* 4 */
static_assert(kTW * kTH % kThreads == 0 && kThreads % kTW == 0, "a thread owns one column");

/* e_j = 2^(j / 256 - 2) (1 + (j % 256) / 256), j = 0..1024: the exponent field is 125 + j / 256 and the top 8 mantissa bits are
 * j % 256, so the edge is one shift and one add on j and needs no table (a table in LDS would be read at a different index by every
 * lane of the search) */
LFBM5D_HD float edge(int j) { return __builtin_bit_cast(float, (125u << 23) + ((unsigned)j << 15)); }

/* #{ j : v >= fl(e_j mu) } for mu >= 0: the products are monotone in j, so the count is the largest pos <= 1025 whose edge pos - 1
 * still passes; 11 steps, the same for every lane */
LFBM5D_HD int key_of(float v, float mu) {
    int pos = 0;
#pragma unroll
    for (int step = 1024; step; step >>= 1) {
        const int cand = pos + step;
        if (cand <= kEdges) {
            const float p = edge(cand - 1) * mu;
            if (v >= p) pos = cand;
        }
    }
    return pos;
}

/* The statistics of one thread's values: key(I_m, mu) goes into hist [C][1026] (the workgroup's counters); a value with I_m or mu not
 * finite into skip[0], else one with mu outside lo..hi into skip[1].  in / pred: the light field and its prediction,
 * [asize][C][H][W]; (x0, y0) the tile's origin. */
template <class Add>
LFBM5D_HD void stats_thread(const float* __restrict__ in, const float* __restrict__ pred, int m, int C, int W, int H, int x0, int y0, int tid,
                            float lo, float hi, unsigned* hist, unsigned* skip, Add add) {
    const size_t plane = (size_t)W * H;
    const int gx = x0 + (tid & (kTW - 1));
    if (gx >= W) return;
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + tid / kTW + k * kRowStep;
        if (gy >= H) break;
        for (int c = 0; c < C; c++) {
            const size_t at = ((size_t)m * C + c) * plane + (size_t)gy * W + gx;
            const float v = in[at], mu = pred[at];
            if (!finite_bits(v) || !finite_bits(mu)) { add(&skip[0]); continue; }
            if (!(mu >= lo && mu <= hi)) { add(&skip[1]); continue; }
            add(&hist[c * kRatioKeys + key_of(v, mu)]);
        }
    }
}

/* The spans of one plane of n floats read at `in` and written at `out`: `head` single values up to the first 16-byte boundary, `quads`
 * groups of four from there, the rest single again.  Where the two addresses sit differently within 16 bytes there is no such
 * boundary and every value is single. */
struct Spans { size_t head, quads; };
LFBM5D_HD Spans spans_of(const float* in, const float* out, size_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(in) & 15u, b = reinterpret_cast<uintptr_t>(out) & 15u;
    if (a != b || (a & 3u)) return {n, 0};
    const size_t head = std::min<size_t>(n, ((16u - a) & 15u) >> 2);
    return {head, (n - head) >> 2};
}

/* Thread `t` of `threads` over one plane: out = in f.  Quads go as one 16-byte load and store each.  out may be in (no restrict). */
struct alignas(16) Quad { float x, y, z, w; };
LFBM5D_HD void apply_thread(const float* in, float* out, size_t n, float f, size_t t, size_t threads) {
    const Spans s = spans_of(in, out, n);
    const Quad* qi = reinterpret_cast<const Quad*>(in + s.head);
    Quad* qo = reinterpret_cast<Quad*>(out + s.head);
    for (size_t i = t; i < s.quads; i += threads) {
        Quad q = qi[i];
        q.x = q.x * f; q.y = q.y * f; q.z = q.z * f; q.w = q.w * f;
        qo[i] = q;
    }
    const size_t body = s.head + 4 * s.quads;
    for (size_t i = t; i < s.head; i += threads) out[i] = in[i] * f;
    for (size_t i = body + t; i < n; i += threads) out[i] = in[i] * f;
}

} /* namespace lfbm5d_photo */
#endif
