/*
 * lfbm5d_view.hip -- reconstruction of whole missing sub-aperture images (lfbm5d_view_*, include/lfbm5d.h): a missing SAI is synthesised
 * from its sound angular neighbours by a plane sweep over integer disparities (per hypothesis the neighbours are warped by d times their
 * angular offset, the squared deviations from their mean are summed over a box, the smallest sum wins per pixel), and the synthesis is
 * refined by the loop "regularise with the hard-thresholding step, put the sound SAIs back, lower sigma" of the defect inpainting
 * (lfbm5d_inpaint.hip) with "every value of the synthesised SAIs" as the mask.  Not in the reference.
 *
 * Kernel (256 threads):
 *   k_view_sweep   grid (tiles, synthesised SAIs); a tile is 64 x 32 positions, a thread owns 8 of them (one column, every fourth row).
 *                  Per hypothesis: the per-pixel error of the tile plus a halo of r goes into LDS (a cell outside the plane is computed at
 *                  the position it mirrors: the same operands, the same bits), barrier, horizontal box sums into a second LDS plane,
 *                  barrier, vertical box sums into registers and the running (E_best, d*) update.  After the last hypothesis the mean at
 *                  d* is recomputed from the sources and stored with the disparity.  Lanes run along x in every phase: global loads are
 *                  rows shifted by a uniform amount, LDS reads of both box passes are consecutive words (no bank conflict).
 *   k_view_sweep_subpel   the same sweep with 2 or 4 hypotheses per pixel of disparity and a bilinear warp (the *_steps_* entry points;
 *                  steps = 1 runs k_view_sweep); its phases are lfbm5d_subpel_device.h, which also compiles for the host, and it equals
 *                  tests/subpel_model.py bit for bit.
 *   k_view_sweep_occl     the occlusion-aware sweep (the *_occl_* entry points with occl_ratio >= 1, include/lfbm5d_occl.h) for 1, 2 or
 *                  4 hypotheses per pixel: beside the full set of sources the error phase evaluates the four half-planes of them and
 *                  takes the best where it is occl_ratio times smaller; the store phase makes the choice again for the cell itself and
 *                  writes the chosen set's mean, j* and k*.  Its phases are lfbm5d_occl_device.h on top of the sub-pixel ones, and it
 *                  equals tests/occl_model.py bit for bit.
 * Sums in a fixed order from +0, no fused multiply-add, one product with a table entry, integer atomics for the histogram (LDS, then
 * global): the GPU equals tests/view_model.py bit for bit.
 */
#include "lfbm5d_side.h"
#include "lfbm5d_subpel_device.h"
#include "lfbm5d_occl_device.h"

using namespace lfbm5d_host;
using namespace lfbm5d_side;

#pragma clang fp contract(off)

namespace {

constexpr int kRMax = 7, kDMax = 8, kSrcMax = 24;                /* box radius, disparity, sources at ang_radius 2 */
constexpr int kEW = kTW + 2 * kRMax, kEH = kTH + 2 * kRMax;      /* the error plane: tile + halo, 78 x 46 */
constexpr int kPer = kTW * kTH / kThreads;                       /* 8 positions per thread */
constexpr int kHist = 2 * kDMax + 1;
constexpr int kTabStride = 2 + 3 * kSrcMax;                      /* per synthesised SAI: its index, n, n x (source index, ds, dt) */
static_assert(kTW * kTH % kThreads == 0 && kThreads % kTW == 0, "a thread owns one column");

/* r[n] = (float)(1.0 / n) */
__constant__ float kRecip[kSrcMax + 1] = {
    0.0f, 1.0f, 0.5f, (float)(1.0 / 3.0), 0.25f, (float)(1.0 / 5.0), (float)(1.0 / 6.0), (float)(1.0 / 7.0), 0.125f, (float)(1.0 / 9.0),
    (float)(1.0 / 10.0), (float)(1.0 / 11.0), (float)(1.0 / 12.0), (float)(1.0 / 13.0), (float)(1.0 / 14.0), (float)(1.0 / 15.0), 0.0625f,
    (float)(1.0 / 17.0), (float)(1.0 / 18.0), (float)(1.0 / 19.0), (float)(1.0 / 20.0), (float)(1.0 / 21.0), (float)(1.0 / 22.0),
    (float)(1.0 / 23.0), (float)(1.0 / 24.0)};

/* the sum of the n sources of channel plane c, warped by hypothesis d, at the in-plane position (y, x): ((+0 + w_1) + w_2) + ... */
__device__ __forceinline__ float warped_sum(const float* __restrict__ in, const int* __restrict__ tab, int n, int d, int c, int C, int y,
                                            int x, int W, int H) {
    const size_t plane = (size_t)W * H;
    float s = 0.0f;
    for (int q = 0; q < n; q++) {
        const int sy = mirror(y - d * tab[3 + 3 * q], H), sx = mirror(x - d * tab[4 + 3 * q], W);
        s = s + in[((size_t)tab[2 + 3 * q] * C + c) * plane + (size_t)sy * W + sx];
    }
    return s;
}

/* e_d(y, x) = sum_c sum_q (w_{q,d} - mu_d)^2, c outer, q inner, from +0 */
__device__ __forceinline__ float pixel_error(const float* __restrict__ in, const int* __restrict__ tab, int n, float rn, int d, int C, int y,
                                             int x, int W, int H) {
    const size_t plane = (size_t)W * H;
    float e = 0.0f;
    for (int c = 0; c < C; c++) {
        const float mu = warped_sum(in, tab, n, d, c, C, y, x, W, H) * rn;
        for (int q = 0; q < n; q++) {
            const int sy = mirror(y - d * tab[3 + 3 * q], H), sx = mirror(x - d * tab[4 + 3 * q], W);
            const float diff = in[((size_t)tab[2 + 3 * q] * C + c) * plane + (size_t)sy * W + sx] - mu;
            const float sq = diff * diff;
            e = e + sq;
        }
    }
    return e;
}

/* grid (tx_n * ty_n, synthesised SAIs), 256 threads.  table: kTabStride ints per synthesised SAI.  cnt[kHist]: positions per d* + 8. */
__global__ __launch_bounds__(kThreads) void k_view_sweep(const float* __restrict__ in, float* __restrict__ out, signed char* __restrict__ disp,
                                                         const int* __restrict__ table, int C, int W, int H, unsigned tx_n, int D, int r,
                                                         unsigned long long* __restrict__ cnt) {
    __shared__ float e[kEH * kEW];
    __shared__ float h[kEH * kTW];
    __shared__ unsigned hist[kHist];
    const int tid = (int)threadIdx.x;
    const int* __restrict__ tab = table + (size_t)blockIdx.y * kTabStride;
    const int m = tab[0], n = tab[1];
    const float rn = kRecip[n];
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
    const int ew = kTW + 2 * r, eh = kTH + 2 * r;
    const int lx = tid & (kTW - 1), ly0 = tid / kTW;              /* this thread's column and first row of the tile */
    if (tid < kHist) hist[tid] = 0u;

    float best[kPer];
    int dstar[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) { best[k] = 0.0f; dstar[k] = 0; }

    for (int j = 0; j <= 2 * D; j++) {
        const int d = (j & 1) ? -((j + 1) >> 1) : (j >> 1);       /* 0, -1, +1, -2, +2, ... */
        for (int i = tid; i < ew * eh; i += kThreads) {
            const int wy = i / ew, wx = i - wy * ew;
            e[wy * kEW + wx] = pixel_error(in, tab, n, rn, d, C, mirror(y0 - r + wy, H), mirror(x0 - r + wx, W), W, H);
        }
        __syncthreads();
        for (int i = tid; i < eh * kTW; i += kThreads) {          /* h(row, x) = sum_k e(row, x + k): window columns x .. x + 2r */
            const float* row = e + (i / kTW) * kEW + (i & (kTW - 1));
            float s = 0.0f;
            for (int k = 0; k <= 2 * r; k++) s = s + row[k];
            h[i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPer; k++) {                          /* E(y, x) = sum_k h(y + k, x): window rows y .. y + 2r */
            const float* col = h + (ly0 + k * (kThreads / kTW)) * kTW + lx;
            float s = 0.0f;
            for (int kk = 0; kk <= 2 * r; kk++) s = s + col[kk * kTW];
            if (j == 0 || s < best[k]) { best[k] = s; dstar[k] = d; }
        }
        /* the next hypothesis writes e at once (its readers passed the second barrier) and h only behind its first barrier */
    }

    const size_t plane = (size_t)W * H;
    const int gx = x0 + lx;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int gy = y0 + ly0 + k * (kThreads / kTW);
        if (gx >= W || gy >= H) continue;
        const size_t at = (size_t)gy * W + gx;
        for (int c = 0; c < C; c++) out[((size_t)m * C + c) * plane + at] = warped_sum(in, tab, n, dstar[k], c, C, gy, gx, W, H) * rn;
        if (disp) disp[(size_t)m * plane + at] = (signed char)dstar[k];
        atomicAdd(&hist[dstar[k] + kDMax], 1u);
    }
    __syncthreads();
    if (tid < kHist && hist[tid]) atomicAdd(&cnt[tid], (unsigned long long)hist[tid]);
}

struct AtomicInc { __device__ __forceinline__ void operator()(unsigned* p) const { atomicAdd(p, 1u); } };

/* The sweep with Q = 2 or 4 hypotheses per pixel, d = j / Q, sources warped by bilinear interpolation (lfbm5d_subpel_device.h holds
 * the phases; this is their order and the barriers).  The same grid, tile and three phases per hypothesis as k_view_sweep.  What a
 * hypothesis makes of each source (offsets, fractions, weights) is the same for every cell: n threads write it into taps ahead of the
 * error phase -- for the next hypothesis between the two barriers, when the error phase that read the table has ended.  HOLD (n <= 8):
 * a channel's warped values stay in registers between mean and deviations.  cnt[kHist]: positions per j* + 32. */
template <bool HOLD>
__global__ __launch_bounds__(kThreads) void k_view_sweep_subpel(const float* __restrict__ in, float* __restrict__ out,
                                                                signed char* __restrict__ disp, const int* __restrict__ table, int C, int W,
                                                                int H, unsigned tx_n, int J, int Q, int r, unsigned long long* __restrict__ cnt) {
    namespace S = lfbm5d_subpel;
    __shared__ float e[S::kEH * S::kEW];
    __shared__ float h[S::kEH * kTW];
    __shared__ S::Tap taps[S::kSrcMax];
    __shared__ unsigned hist[S::kHist];
    const int tid = (int)threadIdx.x;
    const int* __restrict__ tab = table + (size_t)blockIdx.y * kTabStride;
    const int n = tab[1];
    const float rn = kRecip[n];
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
    if (tid < S::kHist) hist[tid] = 0u;
    if (tid < n) taps[tid] = S::make_tap(tab, tid, 0, Q);
    __syncthreads();

    float best[S::kPer];
    int jstar[S::kPer];
#pragma unroll
    for (int k = 0; k < S::kPer; k++) { best[k] = 0.0f; jstar[k] = 0; }

    for (int i = 0; i <= 2 * J; i++) {
        const int j = S::hypothesis(i);
        S::error_phase<HOLD>(in, taps, n, rn, C, W, H, x0, y0, r, tid, e);
        __syncthreads();
        if (tid < n && i < 2 * J) taps[tid] = S::make_tap(tab, tid, S::hypothesis(i + 1), Q);
        S::hbox_phase(e, h, r, tid);
        __syncthreads();
        S::vbox_phase(h, r, tid, i == 0, j, best, jstar);
        /* the next hypothesis writes e at once (its readers passed the second barrier) and h only behind its first barrier */
    }

    S::store_phase(in, out, disp, tab, rn, Q, C, W, H, x0, y0, tid, jstar, hist, AtomicInc());
    __syncthreads();
    if (tid < S::kHist && hist[tid]) atomicAdd(&cnt[tid], (unsigned long long)hist[tid]);
}

/* The occlusion-aware sweep for Q = 1, 2 or 4 (lfbm5d_occl_device.h holds what differs from the sub-pixel sweep: the error phase with
 * the five sets, and the store phase; this is the order and the barriers).  The grid, the tile, the two LDS planes and the two barriers
 * per hypothesis are k_view_sweep_subpel's; the sets of the table row (four half-plane masks beside the full one, their counts and
 * factors) are made once by the last thread into LDS; every thread reads the masks into scalar registers and the factors at each use.  cnt[kCnt]: positions per j* + 32, then per k*. */
template <bool HOLD>
__global__ __launch_bounds__(kThreads) void k_view_sweep_occl(const float* __restrict__ in, float* __restrict__ out,
                                                              signed char* __restrict__ disp, unsigned char* __restrict__ set,
                                                              const int* __restrict__ table, int C, int W, int H, unsigned tx_n, int J, int Q,
                                                              int r, float ratio, unsigned long long* __restrict__ cnt) {
    namespace O = lfbm5d_occl;
    __shared__ float e[O::kEH * O::kEW];
    __shared__ float h[O::kEH * kTW];
    __shared__ O::Tap taps[O::kSrcMax];
    __shared__ O::Sets sets;
    __shared__ unsigned hist[O::kCnt];
    const int tid = (int)threadIdx.x;
    const int* __restrict__ tab = table + (size_t)blockIdx.y * kTabStride;
    const int n = tab[1];
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
    if (tid < O::kCnt) hist[tid] = 0u;
    if (tid < n) taps[tid] = O::make_tap(tab, tid, 0, Q);
    if (tid == kThreads - 1) sets = O::make_sets(tab);
    __syncthreads();
    const O::SetView s = O::view_of(sets);

    float best[O::kPer];
    int jstar[O::kPer];
#pragma unroll
    for (int k = 0; k < O::kPer; k++) { best[k] = 0.0f; jstar[k] = 0; }

    for (int i = 0; i <= 2 * J; i++) {
        const int j = O::hypothesis(i);
        O::error_phase<HOLD>(in, taps, s, n, ratio, C, W, H, x0, y0, r, tid, e);
        __syncthreads();
        if (tid < n && i < 2 * J) taps[tid] = O::make_tap(tab, tid, O::hypothesis(i + 1), Q);
        O::hbox_phase(e, h, r, tid);
        __syncthreads();
        O::vbox_phase(h, r, tid, i == 0, j, best, jstar);
        /* the next hypothesis writes e at once (its readers passed the second barrier) and h only behind its first barrier */
    }

    /* j* moves into the error plane (free: its last readers passed the loop's second barrier; a thread reads back its own words only),
     * so that the store phase can index it by a variable without scratch */
#pragma unroll
    for (int k = 0; k < O::kPer; k++) e[k * kThreads + tid] = (float)jstar[k];
    static_assert(O::kPer * kThreads <= O::kEH * O::kEW, "j* fits the error plane");
    O::store_phase(in, out, disp, set, tab, s, ratio, Q, C, W, H, x0, y0, tid, e + tid, kThreads, hist, AtomicInc());
    __syncthreads();
    if (tid < O::kCnt && hist[tid]) atomicAdd(&cnt[tid], (unsigned long long)hist[tid]);
}

struct Plan {
    std::vector<int> table;            /* kTabStride ints per synthesised SAI */
    std::vector<unsigned> synth, left; /* indices, increasing */
    unsigned nne = 0;
};

const char* check_steps(unsigned steps) { return steps == 1 || steps == 2 || steps == 4 ? nullptr : "steps must be 1, 2 or 4"; }

/* occl_ratio: 0 (off) or a finite number of at least 1 */
const char* check_ratio(float ratio) {
    return ratio == 0.0f || (ratio >= 1.0f && std::isfinite(ratio)) ? nullptr : "occl_ratio must be 0 or a finite number of at least 1";
}

const char* check_params(const lfbm5d_view_params* vp) {
    if (vp->max_disparity > (unsigned)kDMax) return "max_disparity must be 0..8";
    if (vp->box_radius > (unsigned)kRMax) return "box_radius must be 0..7";
    if (vp->ang_radius < 1 || vp->ang_radius > 2) return "ang_radius must be 1 or 2";
    return nullptr;
}

/* the checks on the host arguments every entry shares, and the source lists; 1 with a message */
int plan_sources(lfbm5d_ctx* c, const std::string& who, const lfbm5d_view_params* vp, unsigned steps, float ratio, const unsigned* h_mask,
                 const unsigned* h_missing, unsigned ang_major, unsigned aw, unsigned ah, unsigned W, unsigned H, unsigned C, Plan& p) {
    if (!vp || !h_mask || !h_missing) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_angular(c, who, ang_major, aw, ah)) return 1;
    if (const char* msg = check_params(vp)) return fail(c, who + msg);
    if (const char* msg = check_steps(steps)) return fail(c, who + msg);
    if (const char* msg = check_ratio(ratio)) return fail(c, who + msg);
    if (check_one_gpu(c, who, "the view synthesis runs on one GPU (this context has a communicator or a shard)")) return 1;
    const unsigned asize = aw * ah;
    unsigned n_missing = 0;
    for (unsigned st = 0; st < asize; st++) {
        if (h_mask[st]) p.nne++;
        if (!h_missing[st]) continue;
        n_missing++;
        if (!h_mask[st]) return fail(c, who + "a missing SAI is masked empty (the filter processes a reconstructed SAI: mark it non-empty)");
    }
    if (!n_missing) return fail(c, who + "no SAI is marked missing");
    TileGrid g;
    if (check_tiles(c, who, W, H, asize, 0x3fffffffull, g)) return 1;
    for (unsigned m = 0; m < asize; m++) {
        if (!h_missing[m]) continue;
        int row[kTabStride];
        if (!source_row(m, ang_major, aw, ah, (int)vp->ang_radius, [&](unsigned q) { return h_mask[q] && !h_missing[q]; }, row)) {
            p.left.push_back(m);
            continue;
        }
        p.synth.push_back(m);
        p.table.insert(p.table.end(), row, row + kTabStride);
    }
    return 0;
}

int check_buffers(lfbm5d_ctx* c, const std::string& who, const float* d_in, float* d_out, const unsigned char* d_set, unsigned asize,
                  unsigned W, unsigned H, unsigned C) {
    if (!d_in || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const size_t bytes = (size_t)asize * C * W * H * sizeof(float);
    if (overlap(d_in, bytes, d_out, bytes)) return fail(c, who + "d_out must not overlap d_in (sources are read across tile edges)");
    const size_t set_bytes = (size_t)asize * W * H;
    if (d_set && (overlap(d_set, set_bytes, d_in, bytes) || overlap(d_set, set_bytes, d_out, bytes)))
        return fail(c, who + "d_set must not overlap d_in or d_out");
    return 0;
}

/* the occlusion-aware sweep on the context's stream; d_cnt [kCnt] is accumulated into.  Enqueues only. */
int occl_sweep_launch(lfbm5d_ctx* c, const int* d_table, unsigned n_sai, const float* d_in, float* d_out, signed char* d_disp,
                      unsigned char* d_set, unsigned W, unsigned H, unsigned C, int D, int r, float ratio, unsigned long long* d_cnt,
                      unsigned steps, unsigned max_sources) {
    const unsigned tx_n = (W + kTW - 1) / kTW, ty_n = (H + kTH - 1) / kTH;
    const dim3 grid(tx_n * ty_n, n_sai);
    const bool hold = max_sources <= lfbm5d_occl::kHold;
    const auto k = hold ? k_view_sweep_occl<true> : k_view_sweep_occl<false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, c->stream, d_in, d_out, d_disp, d_set, d_table, (int)C, (int)W, (int)H, tx_n, D * (int)steps,
                       (int)steps, r, ratio, d_cnt);
    HIPCK(c, hipGetLastError());
    return 0;
}

/* the synthesis; after plan_sources().  On return the stream is idle and the planes of the synthesised SAIs of d_out (and d_disp) are
 * written.  h_hist_steps ([65] or NULL): positions per j* + 32; r.disparity_hist is filled for steps = 1 alone.  ratio >= 1: the
 * occlusion-aware sweep, which also writes d_set (or NULL) on those planes and fills ores (or NULL); ratio = 0 touches neither d_set
 * nor the kernels of the plain sweep, and ores is all zero. */
int sweep(lfbm5d_ctx* c, const Plan& p, const lfbm5d_view_params* vp, unsigned steps, float ratio, const float* d_in, float* d_out,
          signed char* d_disp, unsigned char* d_set, unsigned W, unsigned H, unsigned C, lfbm5d_view_result& r, unsigned long long* h_hist_steps,
          lfbm5d_view_occl_result* ores) {
    namespace S = lfbm5d_subpel;
    namespace O = lfbm5d_occl;
    static_assert(S::kHist == LFBM5D_VIEW_STEPS_HIST && S::kHist >= kHist, "include/lfbm5d.h");
    static_assert(O::kSets == LFBM5D_VIEW_OCCL_SETS, "include/lfbm5d_occl.h");
    std::memset(&r, 0, sizeof(r));
    if (ores) std::memset(ores, 0, sizeof(*ores));
    if (h_hist_steps) std::memset(h_hist_steps, 0, S::kHist * sizeof(unsigned long long));
    r.missing = (unsigned)(p.synth.size() + p.left.size());
    r.synthesised = (unsigned)p.synth.size();
    r.left = (unsigned)p.left.size();
    r.pixels = (unsigned long long)p.synth.size() * W * H;
    if (p.synth.empty()) return 0;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->view.table.reserve(p.table.size() * sizeof(int)));
    HIPCK(c, c->view.stats.reserve(O::kCnt * sizeof(unsigned long long)));
    unsigned long long* d_cnt = c->view.stats.as<unsigned long long>();
    HIPCK(c, hipMemcpyAsync(c->view.table.p, p.table.data(), p.table.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemsetAsync(d_cnt, 0, O::kCnt * sizeof(unsigned long long), c->stream));
    unsigned most = 0;
    for (size_t i = 0; i < p.synth.size(); i++) most = std::max(most, (unsigned)p.table[i * kTabStride + 1]);
    unsigned long long got[O::kCnt];
    if (ratio != 0.0f) {
        if (occl_sweep_launch(c, c->view.table.as<int>(), (unsigned)p.synth.size(), d_in, d_out, d_disp, d_set, W, H, C, (int)vp->max_disparity,
                              (int)vp->box_radius, ratio, d_cnt, steps, most)) return 1;
        HIPCK(c, hipMemcpyAsync(got, d_cnt, O::kCnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));   /* the table leaves a caller's object; the counters are read */
        if (steps == 1) std::memcpy(r.disparity_hist, got + S::kJMax - kDMax, kHist * sizeof(unsigned long long));
        if (h_hist_steps) std::memcpy(h_hist_steps, got, S::kHist * sizeof(unsigned long long));
        if (ores) std::memcpy(ores->set_hist, got + S::kHist, O::kSets * sizeof(unsigned long long));
        return 0;
    }
    if (view_sweep_launch(c, c->view.table.as<int>(), (unsigned)p.synth.size(), d_in, d_out, d_disp, W, H, C, (int)vp->max_disparity,
                          (int)vp->box_radius, d_cnt, steps, most)) return 1;
    const int bins = steps == 1 ? kHist : S::kHist;
    HIPCK(c, hipMemcpyAsync(got, d_cnt, bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));   /* the table leaves a caller's object; the histogram is read */
    if (steps == 1) std::memcpy(r.disparity_hist, got, kHist * sizeof(unsigned long long));
    if (h_hist_steps) std::memcpy(h_hist_steps + (steps == 1 ? S::kJMax - kDMax : 0), got, bins * sizeof(unsigned long long));
    return 0;
}

/* include/lfbm5d_occl.h, lfbm5d_view_occl_device */
int view(lfbm5d_ctx* c, const std::string& who, const lfbm5d_view_params* vp, unsigned steps, float ratio, const lfbm5d_params* P,
         const float* d_in, const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned char* d_set,
         unsigned ang_major, unsigned aw, unsigned ah, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* res,
         unsigned long long* h_hist_steps, lfbm5d_view_occl_result* ores) {
    if (!vp || !P) return fail(c, who + "NULL pointer for a required buffer");
    const unsigned asize = aw * ah;
    if (check_buffers(c, who, d_in, d_out, d_set, asize, W, H, C)) return 1;
    const LoopSchedule sched = {vp->iterations, vp->sigma_start, vp->sigma_end, vp->sigma_noise};
    if (const char* msg = check_schedule(sched)) return fail(c, who + msg);
    Plan p;
    if (plan_sources(c, who, vp, steps, ratio, h_mask, h_missing, ang_major, aw, ah, W, H, C, p)) return 1;
    lfbm5d_view_result r;
    if (sweep(c, p, vp, steps, ratio, d_in, d_out, d_disp, d_set, W, H, C, r, h_hist_steps, ores)) return 1;
    if (res) *res = r;
    const size_t img = (size_t)C * W * H;
    const auto sound = [&](unsigned st) { return h_mask[st] && !h_missing[st]; };
    const auto put_back = [&](unsigned) {                                   /* f ? b : y: a selection moves bits, so a copy is one */
        if (copy_sais(c, asize, d_out, d_in, img, sizeof(float), sound)) return 1;
        HIPCK(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    if (put_back(0)) return 1;                                              /* x_0: the input with the synthesised SAIs replaced */
    if (!sched.iterations) return 0;
    if (r.left) return fail(c, who + "a missing SAI without a source within ang_radius cannot be refined (run the synthesis alone, or widen ang_radius)");
    /* the step's input is x_{k-1}, its output b_k goes over d_out, x_k = f ? b_k : y */
    return refine_loop(c, sched, P, h_mask, p.nne, d_out, ang_major, aw, ah, an, W, H, C,
                       [&](unsigned, float* z) { return copy_sais(c, asize, z, d_out, img, sizeof(float), [&](unsigned st) { return h_mask[st] != 0; }); },
                       put_back);
}

/* include/lfbm5d_occl.h, lfbm5d_view_fill_occl_device */
int fill(lfbm5d_ctx* c, const std::string& who, const lfbm5d_view_params* vp, unsigned steps, float ratio, const float* d_in,
         const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned char* d_set, unsigned ang_major,
         unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out, unsigned long long* h_hist_steps,
         lfbm5d_view_occl_result* ores) {
    if (check_buffers(c, who, d_in, d_out, d_set, awidth * aheight, W, H, C)) return 1;
    Plan p;
    if (plan_sources(c, who, vp, steps, ratio, h_mask, h_missing, ang_major, awidth, aheight, W, H, C, p)) return 1;
    lfbm5d_view_result r;
    if (sweep(c, p, vp, steps, ratio, d_in, d_out, d_disp, d_set, W, H, C, r, h_hist_steps, ores)) return 1;
    if (out) *out = r;
    return 0;
}

/* include/lfbm5d_occl.h, lfbm5d_view_occl_host_sai */
int host_sai(lfbm5d_ctx* c, const std::string& who, const lfbm5d_view_params* vp, unsigned steps, float ratio, const lfbm5d_params* P,
             const float* const* h_in, const unsigned* h_mask, const unsigned* h_missing, float* const* h_out, signed char* const* h_disp,
             unsigned char* const* h_set, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C,
             lfbm5d_view_result* out, unsigned long long* h_hist_steps, lfbm5d_view_occl_result* ores) {
    if (!vp || !P || !h_in || !h_out || !h_mask || !h_missing) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const unsigned asize = awidth * aheight;
    const size_t img = (size_t)C * W * H, plane = (size_t)W * H, all = std::max<size_t>(1, (size_t)asize * img);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    const auto sound = [&](unsigned st) { return h_mask[st] && !h_missing[st]; };
    const auto missing = [&](unsigned st) { return h_mask[st] && h_missing[st]; };
    if (check_planes(c, who, h_out, asize, nonempty) || (h_disp && check_planes(c, who, h_disp, asize, missing))) return 1;
    if (ratio == 0.0f) h_set = nullptr;                                     /* the plain sweep writes no sets */
    if (h_set && check_planes(c, who, h_set, asize, missing)) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    HIPCK(c, c->h2d_out.reserve(all * sizeof(float)));
    if (h_disp) HIPCK(c, c->view.disp.reserve(std::max<size_t>(1, (size_t)asize * plane)));
    if (h_set) HIPCK(c, c->view.set.reserve(std::max<size_t>(1, (size_t)asize * plane)));
    float* const din = c->h2d_noisy.as<float>(); float* const dout = c->h2d_out.as<float>();
    signed char* const ddisp = h_disp ? c->view.disp.as<signed char>() : nullptr;
    unsigned char* const dset = h_set ? c->view.set.as<unsigned char>() : nullptr;
    if (upload_planes(c, who, h_in, din, asize, img, sound)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    lfbm5d_view_result r;
    std::memset(&r, 0, sizeof(r));
    const int rc = view(c, who, vp, steps, ratio, P, din, h_mask, h_missing, dout, ddisp, dset, ang_major, awidth, aheight, an, W, H, C, &r,
                        h_hist_steps, ores);
    if (out) *out = r;
    if (rc) return 1;
    /* an SAI that was left (K = 0 only) was not written on the device: its host planes stay as they are */
    Plan p;
    if (r.left && plan_sources(c, who, vp, steps, ratio, h_mask, h_missing, ang_major, awidth, aheight, W, H, C, p)) return 1;
    const auto written = [&](unsigned st) { return h_mask[st] && std::find(p.left.begin(), p.left.end(), st) == p.left.end(); };
    if (download_planes(c, h_out, dout, asize, img, written)) return 1;
    if (h_disp && download_planes(c, h_disp, ddisp, asize, plane, [&](unsigned st) { return missing(st) && written(st); })) return 1;
    if (h_set && download_planes(c, h_set, dset, asize, plane, [&](unsigned st) { return missing(st) && written(st); })) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

/* lfbm5d_ctx.h: the sweep for another stage's table (the consistency check's leave-one-out lists) */
int lfbm5d_host::view_sweep_launch(lfbm5d_ctx* c, const int* d_table, unsigned n_sai, const float* d_in, float* d_out, signed char* d_disp,
                                   unsigned W, unsigned H, unsigned C, int D, int r, unsigned long long* d_cnt, unsigned steps,
                                   unsigned max_sources) {
    static_assert(kViewTabStride == kTabStride && lfbm5d_subpel::kTabStride == kTabStride, "lfbm5d_ctx.h");
    const unsigned tx_n = (W + kTW - 1) / kTW, ty_n = (H + kTH - 1) / kTH;
    const dim3 grid(tx_n * ty_n, n_sai);
    if (steps == 1) {
        hipLaunchKernelGGL(k_view_sweep, grid, dim3(kThreads), 0, c->stream, d_in, d_out, d_disp, d_table, (int)C, (int)W, (int)H, tx_n, D, r, d_cnt);
    } else {
        /* one launch serves every row of the table: the values stay in registers only if no row has more than 8 sources */
        const bool hold = max_sources <= lfbm5d_subpel::kHold;
        const auto k = hold ? k_view_sweep_subpel<true> : k_view_sweep_subpel<false>;
        hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, c->stream, d_in, d_out, d_disp, d_table, (int)C, (int)W, (int)H, tx_n, D * (int)steps,
                           (int)steps, r, d_cnt);
    }
    HIPCK(c, hipGetLastError());
    return 0;
}

extern "C" {

void lfbm5d_view_defaults(lfbm5d_view_params* out) {
    if (!out) return;
    out->max_disparity = 4;                  /* the best row of the sweep in profiles/view_defaults.txt */
    out->box_radius = 3;
    out->ang_radius = 1;
    out->iterations = 4;
    out->sigma_start = 30.0f;
    out->sigma_end = 5.0f;
    out->sigma_noise = 0.0f;
}

int lfbm5d_view_fill_steps_device(lfbm5d_ctx* c, const lfbm5d_view_params* vp, unsigned steps, const float* d_in, const unsigned* h_mask,
                                  const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major, unsigned awidth,
                                  unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out,
                                  unsigned long long* h_hist_steps) {
    if (!c) return 1;
    return fill(c, "lfbm5d_view_fill_steps_device: ", vp, steps, 0.0f, d_in, h_mask, h_missing, d_out, d_disp, nullptr, ang_major, awidth, aheight,
                W, H, C, out, h_hist_steps, nullptr);
}

int lfbm5d_view_fill_device(lfbm5d_ctx* c, const lfbm5d_view_params* vp, const float* d_in, const unsigned* h_mask, const unsigned* h_missing,
                            float* d_out, signed char* d_disp, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H,
                            unsigned C, lfbm5d_view_result* out) {
    if (!c) return 1;
    return fill(c, "lfbm5d_view_fill_device: ", vp, 1, 0.0f, d_in, h_mask, h_missing, d_out, d_disp, nullptr, ang_major, awidth, aheight, W, H, C, out, nullptr,
                nullptr);
}

int lfbm5d_view_steps_device(lfbm5d_ctx* c, const lfbm5d_view_params* vp, unsigned steps, const lfbm5d_params* P, const float* d_in,
                             const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major,
                             unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out,
                             unsigned long long* h_hist_steps) {
    if (!c) return 1;
    return view(c, "lfbm5d_view_steps_device: ", vp, steps, 0.0f, P, d_in, h_mask, h_missing, d_out, d_disp, nullptr, ang_major, awidth, aheight, an,
                W, H, C, out, h_hist_steps, nullptr);
}

int lfbm5d_view_device(lfbm5d_ctx* c, const lfbm5d_view_params* vp, const lfbm5d_params* P, const float* d_in, const unsigned* h_mask,
                       const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major, unsigned awidth, unsigned aheight,
                       unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out) {
    if (!c) return 1;
    return view(c, "lfbm5d_view_device: ", vp, 1, 0.0f, P, d_in, h_mask, h_missing, d_out, d_disp, nullptr, ang_major, awidth, aheight, an, W, H, C, out, nullptr,
                nullptr);
}

int lfbm5d_view_steps_host_sai(lfbm5d_ctx* c, const lfbm5d_view_params* vp, unsigned steps, const lfbm5d_params* P, const float* const* h_in,
                               const unsigned* h_mask, const unsigned* h_missing, float* const* h_out, signed char* const* h_disp,
                               unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C,
                               lfbm5d_view_result* out, unsigned long long* h_hist_steps) {
    if (!c) return 1;
    return host_sai(c, "lfbm5d_view_steps_host_sai: ", vp, steps, 0.0f, P, h_in, h_mask, h_missing, h_out, h_disp, nullptr, ang_major, awidth,
                    aheight, an, W, H, C, out, h_hist_steps, nullptr);
}

int lfbm5d_view_host_sai(lfbm5d_ctx* c, const lfbm5d_view_params* vp, const lfbm5d_params* P, const float* const* h_in, const unsigned* h_mask,
                         const unsigned* h_missing, float* const* h_out, signed char* const* h_disp, unsigned ang_major, unsigned awidth,
                         unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out) {
    if (!c) return 1;
    return host_sai(c, "lfbm5d_view_host_sai: ", vp, 1, 0.0f, P, h_in, h_mask, h_missing, h_out, h_disp, nullptr, ang_major, awidth, aheight, an, W, H, C,
                    out, nullptr, nullptr);
}

float lfbm5d_view_occl_default(void) { return 4.0f; }   /* the best row of the sweep in profiles/occl_defaults.txt */

int lfbm5d_view_fill_occl_device(lfbm5d_ctx* c, const lfbm5d_view_params* vp, unsigned steps, float occl_ratio, const float* d_in,
                                 const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned char* d_set,
                                 unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C,
                                 lfbm5d_view_result* out, unsigned long long* h_hist_steps, lfbm5d_view_occl_result* occl) {
    if (!c) return 1;
    return fill(c, "lfbm5d_view_fill_occl_device: ", vp, steps, occl_ratio, d_in, h_mask, h_missing, d_out, d_disp, d_set, ang_major, awidth,
                aheight, W, H, C, out, h_hist_steps, occl);
}

int lfbm5d_view_occl_device(lfbm5d_ctx* c, const lfbm5d_view_params* vp, unsigned steps, float occl_ratio, const lfbm5d_params* P,
                            const float* d_in, const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp,
                            unsigned char* d_set, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H,
                            unsigned C, lfbm5d_view_result* out, unsigned long long* h_hist_steps, lfbm5d_view_occl_result* occl) {
    if (!c) return 1;
    return view(c, "lfbm5d_view_occl_device: ", vp, steps, occl_ratio, P, d_in, h_mask, h_missing, d_out, d_disp, d_set, ang_major, awidth,
                aheight, an, W, H, C, out, h_hist_steps, occl);
}

int lfbm5d_view_occl_host_sai(lfbm5d_ctx* c, const lfbm5d_view_params* vp, unsigned steps, float occl_ratio, const lfbm5d_params* P,
                              const float* const* h_in, const unsigned* h_mask, const unsigned* h_missing, float* const* h_out,
                              signed char* const* h_disp, unsigned char* const* h_set, unsigned ang_major, unsigned awidth, unsigned aheight,
                              unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out, unsigned long long* h_hist_steps,
                              lfbm5d_view_occl_result* occl) {
    if (!c) return 1;
    return host_sai(c, "lfbm5d_view_occl_host_sai: ", vp, steps, occl_ratio, P, h_in, h_mask, h_missing, h_out, h_disp, h_set, ang_major,
                    awidth, aheight, an, W, H, C, out, h_hist_steps, occl);
}

} /* extern "C" */
