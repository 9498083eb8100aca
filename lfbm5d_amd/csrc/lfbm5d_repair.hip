/*
 * lfbm5d_repair.hip -- joint repair (lfbm5d_repair_*, include/lfbm5d_repair.h): defective values and missing sub-aperture images are
 * one set of unsound values; a plane sweep that skips unsound source values fills them from the other views, the onion-peel fill of the
 * defect inpainting (lfbm5d_inpaint_fill_device, as it stands) takes what the sweep could not reach, and one refinement loop on the
 * hard-thresholding step serves both.  Not in the reference.
 *
 * Kernels (256 threads; the per-thread phases are lfbm5d_repair_device.h, which also compiles for the host):
 *   k_repair_valid   grid (tiles, non-empty SAIs): the validity planes v_q (uint8 per position), the flags of the unsound values, a
 *                    copy of the input the sweep writes into, and the number of unsound positions per (SAI, 64 x 32 tile).
 *   k_repair_sweep   grid (tiles, targets): k_view_sweep's tile, thread-owns-a-column layout and three phases per hypothesis, with a
 *                    16-bit plane of evidence counts beside each float plane in LDS, carried through both box passes.  A workgroup
 *                    whose tile has no unsound position returns at once (a uniform branch ahead of every barrier).
 *                    What the store phase alone needs (output pointers, min_valid, d*, the tile's origin) waits in memory or LDS, so
 *                    that no scalar register is held for it through the sweep: no scratch, no spill (tools/kernel_regs.sh).
 *   k_repair_codes   grid (blocks, non-empty SAIs): the code of every value from the onion-peel fill's states, and the counts.
 * Sums in a fixed order from +0, no fused multiply-add, products with table entries, integer atomics for the counts (LDS, then
 * global): the GPU equals tests/repair_model.py bit for bit.
 */
#include "lfbm5d_side.h"
#include "lfbm5d_repair_device.h"

using namespace lfbm5d_host;
using namespace lfbm5d_side;

#pragma clang fp contract(off)

namespace {

namespace R = lfbm5d_repair;

/* counters: [0..16] positions per d* + 8, [17 + 3 (code - 1) + channel] values per code, [26] non-zero flags */
constexpr int kCntCode = R::kHist, kCntFlag = kCntCode + 9, kCntWords = kCntFlag + 1;

struct AtomicInc { __device__ __forceinline__ void operator()(unsigned* p) const { atomicAdd(p, 1u); } };

/* grid (tx_n * ty_n, nne).  missing: unsigned [asize].  tiles: unsigned [asize][tx_n * ty_n], every word of a non-empty SAI written. */
__global__ __launch_bounds__(kThreads) void k_repair_valid(const float* __restrict__ in, const unsigned char* __restrict__ flags,
                                                           const unsigned* __restrict__ sai, const unsigned* __restrict__ missing,
                                                           unsigned char* __restrict__ valid, float* __restrict__ mid,
                                                           unsigned char* __restrict__ rem, unsigned* __restrict__ tiles, int C, int W, int H,
                                                           unsigned tx_n) {
    __shared__ unsigned total;
    const int tid = (int)threadIdx.x;
    const unsigned q = sai[blockIdx.y];
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    if (tid == 0) total = 0u;
    __syncthreads();
    const unsigned mine = R::valid_thread(in, flags, missing[q] != 0u, (int)q, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, valid, mid, rem);
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) tiles[(size_t)q * gridDim.x + blockIdx.x] = total;
}

/* what k_repair_sweep needs behind its last hypothesis only: read from memory there, so that it holds no scalar register through the
 * sweep (with these as kernel arguments the kernel spilled scalar registers) */
struct StoreArgs {
    float* mid;
    unsigned char* rem;
    signed char* disp;
    unsigned long long* cnt;   /* [kHist]: positions per d* + 8 */
    int min_valid;
};

/* grid (tx_n * ty_n, targets), 256 threads.  table: kTabStride ints per target, and one StoreArgs in front of the first row. */
__global__ __launch_bounds__(kThreads) void k_repair_sweep(const float* __restrict__ in, const unsigned char* __restrict__ valid,
                                                           const int* __restrict__ table, const float* __restrict__ tables, const unsigned* __restrict__ tiles, int C, int W,
                                                           int H, unsigned tx_n, int D, int r) {
    __shared__ float e[R::kEH * R::kEW];
    __shared__ float h[R::kEH * kTW];
    __shared__ unsigned short ke[R::kEH * R::kEW];
    __shared__ unsigned short kh[R::kEH * kTW];
    __shared__ unsigned hist[R::kHist];
    __shared__ int origin[2];
    const int tid = (int)threadIdx.x;
    const int* __restrict__ tab = table + (size_t)blockIdx.y * R::kTabStride;
    const int m = tab[0];
    if (!tiles[(size_t)m * gridDim.x + blockIdx.x]) return;       /* nothing unsound in this tile: mid is the copy already */
    const R::Sweep s = {in, valid, tab, tables, tab[1], C, W, H};
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
    if (tid == 0) { origin[0] = x0; origin[1] = y0; }             /* for the store phase: read back there, held in no register through the sweep */
    if (tid >= kThreads - R::kHist) hist[kThreads - 1 - tid] = 0u;   /* the last threads: the first ones' test at the end is then no value held through the sweep */

    float best[R::kPer];
    int dstar[R::kPer];
#pragma unroll
    for (int k = 0; k < R::kPer; k++) { best[k] = 0.0f; dstar[k] = 0; }

    for (int j = 0; j <= 2 * D; j++) {
        const int d = R::hypothesis(j);
        R::error_phase(s, d, x0, y0, r, tid, e, ke);
        __syncthreads();
        R::hbox_phase(e, ke, h, kh, r, tid);
        __syncthreads();
        R::vbox_phase(s, h, kh, r, tid, j == 0, d, best, dstar);
        /* the next hypothesis writes e at once (its readers passed the second barrier) and h only behind its first barrier */
    }

    /* d* moves into the error plane (free: its last readers passed the loop's second barrier; a thread reads back its own words only) */
#pragma unroll
    for (int k = 0; k < R::kPer; k++) e[k * kThreads + tid] = (float)dstar[k];
    static_assert(R::kPer * kThreads <= R::kEH * R::kEW, "d* fits the error plane");
    const StoreArgs a = *(reinterpret_cast<const StoreArgs*>(table) - 1);
    R::store_phase(s, tab[0], a.min_valid, a.mid, a.rem, a.disp, origin[0], origin[1], tid, e + tid, kThreads, hist, AtomicInc());
    __syncthreads();
    if (tid < R::kHist && hist[tid]) atomicAdd(&a.cnt[tid], (unsigned long long)hist[tid]);
}

/* grid (blocks, nne); n = values of one SAI, plane = W * H.  st: the onion-peel fill's states; codes may be st. */
__global__ __launch_bounds__(kThreads) void k_repair_codes(const float* __restrict__ in, const unsigned char* __restrict__ flags,
                                                           const unsigned* __restrict__ sai, const unsigned* __restrict__ missing,
                                                           const unsigned char* st, unsigned char* codes, size_t n, size_t plane,
                                                           unsigned long long* __restrict__ cnt) {
    __shared__ unsigned tally[10];
    const unsigned q = sai[blockIdx.y];
    const bool gone = missing[q] != 0u;
    const size_t base = (size_t)q * n;
    if (threadIdx.x < 10) tally[threadIdx.x] = 0u;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const bool flagged = flags && flags[base + i];
        const unsigned code = R::code_of(st[base + i], gone || flagged || !finite_bits(in[base + i]));
        codes[base + i] = (unsigned char)code;
        if (code) atomicAdd(&tally[3 * (code - 1) + (unsigned)(i / plane)], 1u);
        if (flagged) atomicAdd(&tally[9], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 10 && tally[threadIdx.x]) atomicAdd(&cnt[kCntCode + threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

constexpr const char* kOneGpu = "the joint repair runs on one GPU (this context has a communicator or a shard)";
constexpr unsigned long long kMaxPlane = 0x3fffffffull;

const char* check_params(const lfbm5d_repair_params* rp) {
    if (rp->max_disparity > (unsigned)R::kDMax) return "max_disparity must be 0..8";
    if (rp->box_radius > (unsigned)R::kRMax) return "box_radius must be 0..7";
    if (rp->ang_radius < 1 || rp->ang_radius > 2) return "ang_radius must be 1 or 2";
    if (rp->min_valid < 1 || rp->min_valid > (unsigned)R::kSrcMax) return "min_valid must be 1..24";
    return nullptr;
}

/* r, f and g of lfbm5d_repair_device.h for box radius r */
void float_tables(int r, std::vector<float>& t) {
    t.assign(R::kTabFloats, 0.0f);
    for (int k = 1; k <= R::kSrcMax; k++) t[R::kTabR + k] = (float)(1.0 / k);
    for (int n = 2; n <= R::kSrcMax; n++)
        for (int k = 2; k <= R::kSrcMax; k++) t[R::kTabF + n * (R::kSrcMax + 1) + k] = (float)((double)(n - 1) / (double)(k - 1));
    const int box = (2 * r + 1) * (2 * r + 1);
    for (int k = 1; k <= box; k++) t[R::kTabG + k] = (float)((double)box / (double)k);
}

int check_buffers(lfbm5d_ctx* c, const std::string& who, const float* d_in, const unsigned char* d_flags_in, float* d_out,
                  unsigned char* d_codes, signed char* d_disp, unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!d_in || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const size_t values = (size_t)asize * C * W * H, bytes = values * sizeof(float), positions = (size_t)asize * W * H;
    if (overlap(d_in, bytes, d_out, bytes)) return fail(c, who + "d_out must not overlap d_in (the loop puts the sound values back from d_in)");
    if (d_codes && (overlap(d_codes, values, d_in, bytes) || overlap(d_codes, values, d_out, bytes) ||
                    (d_flags_in && overlap(d_codes, values, d_flags_in, values))))
        return fail(c, who + "d_codes must not overlap d_in, d_out or d_flags_in");
    if (d_disp && (overlap(d_disp, positions, d_in, bytes) || overlap(d_disp, positions, d_out, bytes) ||
                   (d_codes && overlap(d_disp, positions, d_codes, values)) || (d_flags_in && overlap(d_disp, positions, d_flags_in, values))))
        return fail(c, who + "d_disp must not overlap d_in, d_out, d_codes or d_flags_in");
    return 0;
}

/* the fill; on return the stream is idle, d_out is written on the non-empty SAIs and *codes points at the code planes (d_codes when
 * given, else the context's scratch) */
int fill(lfbm5d_ctx* c, const std::string& who, const lfbm5d_repair_params* rp, const float* d_in, const unsigned char* d_flags_in,
         const unsigned* h_mask, const unsigned* h_missing, float* d_out, unsigned char* d_codes, signed char* d_disp, unsigned ang_major,
         unsigned aw, unsigned ah, unsigned W, unsigned H, unsigned C, lfbm5d_repair_result& res, const unsigned char** codes) {
    std::memset(&res, 0, sizeof(res));
    if (!rp || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    const unsigned asize = aw * ah;
    if (check_buffers(c, who, d_in, d_flags_in, d_out, d_codes, d_disp, asize, W, H, C)) return 1;
    if (check_size(c, who, W, H, 2, "be at least 2") || check_angular(c, who, ang_major, aw, ah)) return 1;
    if (const char* msg = check_params(rp)) return fail(c, who + msg);
    std::vector<unsigned> missing(asize, 0u);
    for (unsigned st = 0; st < asize; st++) {
        if (!h_missing || !h_missing[st]) continue;
        if (!h_mask[st]) return fail(c, who + "a missing SAI is masked empty (the filter processes a reconstructed SAI: mark it non-empty)");
        missing[st] = 1u;
        res.missing++;
    }
    Shape s;
    if (prepare_tiled(c, who, kOneGpu, h_mask, asize, W, H, C, kMaxPlane, s)) return 1;
    const unsigned nt = s.tx_n * s.ty_n;
    const size_t plane = (size_t)W * H, img = (size_t)C * plane, values = (size_t)asize * img;
    res.values = (unsigned long long)s.nne * img;

    lfbm5d_ctx::RepairBufs& B = c->repair;
    std::vector<float> ft;
    float_tables((int)rp->box_radius, ft);
    const size_t tab_bytes = (size_t)asize * R::kTabStride * sizeof(int), ft_bytes = ft.size() * sizeof(float);
    HIPCK(c, B.valid.reserve((size_t)asize * plane));
    HIPCK(c, B.mid.reserve(values * sizeof(float)));
    HIPCK(c, B.rem.reserve(values));
    HIPCK(c, B.tiles.reserve((size_t)asize * nt * sizeof(unsigned)));
    HIPCK(c, B.table.reserve(sizeof(StoreArgs) + tab_bytes + ft_bytes + asize * sizeof(unsigned)));
    HIPCK(c, B.stats.reserve(kCntWords * sizeof(unsigned long long)));
    if (!d_codes) HIPCK(c, B.codes.reserve(values));
    static_assert(sizeof(StoreArgs) % sizeof(int) == 0, "the table follows the late arguments");
    StoreArgs* const d_late = B.table.as<StoreArgs>();   /* in front of the table: the kernel finds it there */
    int* const d_table = reinterpret_cast<int*>(B.table.as<char>() + sizeof(StoreArgs));
    float* const d_ft = reinterpret_cast<float*>(B.table.as<char>() + sizeof(StoreArgs) + tab_bytes);
    unsigned* const d_missing = reinterpret_cast<unsigned*>(B.table.as<char>() + sizeof(StoreArgs) + tab_bytes + ft_bytes);
    unsigned* const d_tiles = B.tiles.as<unsigned>();
    unsigned long long* const d_cnt = B.stats.as<unsigned long long>();
    unsigned char* const d_valid = B.valid.as<unsigned char>();
    float* const d_mid = B.mid.as<float>();
    unsigned char* const d_rem = B.rem.as<unsigned char>();
    const unsigned* const d_sai = c->side.sai.as<unsigned>();

    HIPCK(c, hipMemcpyAsync(d_ft, ft.data(), ft_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(d_missing, missing.data(), asize * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemsetAsync(d_tiles, 0, (size_t)asize * nt * sizeof(unsigned), c->stream));
    HIPCK(c, hipMemsetAsync(d_cnt, 0, kCntWords * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_repair_valid, dim3(nt, s.nne), dim3(kThreads), 0, c->stream, d_in, d_flags_in, d_sai, d_missing, d_valid, d_mid, d_rem,
                       d_tiles, (int)C, (int)W, (int)H, s.tx_n);
    HIPCK(c, hipGetLastError());
    std::vector<unsigned> tiles((size_t)asize * nt);
    HIPCK(c, hipMemcpyAsync(tiles.data(), d_tiles, tiles.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));   /* the host vectors were read; the targets follow from the counts */

    std::vector<int> table;
    for (unsigned m = 0; m < asize; m++) {
        if (!h_mask[m]) continue;
        unsigned long long unsound = 0;
        for (unsigned t = 0; t < nt; t++) unsound += tiles[(size_t)m * nt + t];
        if (!unsound) continue;
        res.targets++;
        int row[R::kTabStride];
        static_assert(R::kTabStride == kViewTabStride, "lfbm5d_side.h: source_row");
        if (!source_row(m, ang_major, aw, ah, (int)rp->ang_radius, [&](unsigned q) { return q != m && h_mask[q] && !missing[q]; }, row)) continue;
        res.swept++;
        table.insert(table.end(), row, row + R::kTabStride);
    }
    if (!res.targets) return fail(c, who + "nothing to repair (no flag, no value that is not finite, no missing SAI)");
    if (res.swept) {
        const StoreArgs late = {d_mid, d_rem, d_disp, d_cnt, (int)rp->min_valid};
        HIPCK(c, hipMemcpyAsync(d_late, &late, sizeof(late), hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_repair_sweep, dim3(nt, res.swept), dim3(kThreads), 0, c->stream, d_in, d_valid, d_table, d_ft, d_tiles, (int)C,
                           (int)W, (int)H, s.tx_n, (int)rp->max_disparity, (int)rp->box_radius);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipStreamSynchronize(c->stream));   /* the table and the late arguments leave this frame */
    }
    /* the rim fill of what is still flagged, on the sweep's result */
    unsigned char* const d_st = d_codes ? d_codes : B.codes.as<unsigned char>();
    lfbm5d_inpaint_result ir;
    if (lfbm5d_inpaint_fill_device(c, d_mid, d_rem, h_mask, d_out, d_st, asize, W, H, C, &ir)) return 1;
    res.passes = ir.passes;
    const dim3 grid((unsigned)std::min<size_t>((img + kThreads - 1) / kThreads, 1024), s.nne);
    hipLaunchKernelGGL(k_repair_codes, grid, dim3(kThreads), 0, c->stream, d_in, d_flags_in, d_sai, d_missing, d_st, d_st, img, plane, d_cnt);
    HIPCK(c, hipGetLastError());
    unsigned long long cnt[kCntWords];
    HIPCK(c, hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < R::kHist; k++) { res.disparity_hist[k] = cnt[k]; res.positions += cnt[k]; }
    for (unsigned ch = 0; ch < 3; ch++) {
        res.views[ch] = cnt[kCntCode + ch]; res.rim[ch] = cnt[kCntCode + 3 + ch]; res.left[ch] = cnt[kCntCode + 6 + ch];
        res.unsound[ch] = res.views[ch] + res.rim[ch] + res.left[ch];
    }
    res.flagged = cnt[kCntFlag];
    *codes = d_st;
    return 0;
}

/* include/lfbm5d_repair.h, lfbm5d_repair_device */
int repair(lfbm5d_ctx* c, const std::string& who, const lfbm5d_repair_params* rp, const lfbm5d_params* P, const float* d_in,
           const unsigned char* d_flags_in, const unsigned* h_mask, const unsigned* h_missing, float* d_out, unsigned char* d_codes,
           signed char* d_disp, unsigned ang_major, unsigned aw, unsigned ah, unsigned an, unsigned W, unsigned H, unsigned C,
           lfbm5d_repair_result* out) {
    if (!rp || !P) return fail(c, who + "NULL pointer for a required buffer");
    const LoopSchedule sched = {rp->iterations, rp->sigma_start, rp->sigma_end, rp->sigma_noise};
    if (const char* msg = check_schedule(sched)) return fail(c, who + msg);
    lfbm5d_repair_result r;
    const unsigned char* codes = nullptr;
    const int rc = fill(c, who, rp, d_in, d_flags_in, h_mask, h_missing, d_out, d_codes, d_disp, ang_major, aw, ah, W, H, C, r, &codes);
    if (out) *out = r;
    if (rc) return 1;
    if (!sched.iterations) return 0;
    if (r.left[0] + r.left[1] + r.left[2])
        return fail(c, who + "a value that neither the other views nor its own plane can fill cannot be refined (mask its SAI as empty, or run the fill alone)");
    const unsigned asize = aw * ah;
    unsigned nne = 0;
    for (unsigned st = 0; st < asize; st++) nne += h_mask[st] ? 1u : 0u;
    /* the step's input is x_{k-1} = f ? b_{k-1} : y, formed in the scratch; its output b_k goes over d_out */
    const auto project = [&](float* z) { return lfbm5d_inpaint_project_device(c, codes, d_out, d_in, h_mask, z, asize, W, H, C); };
    if (refine_loop(c, sched, P, h_mask, nne, d_out, ang_major, aw, ah, an, W, H, C, [&](unsigned, float* z) { return project(z); },
                    [](unsigned) { return 0; })) return 1;
    return project(d_out);                                                  /* x_K */
}

} /* namespace */

extern "C" {

void lfbm5d_repair_defaults(lfbm5d_repair_params* out) {
    if (!out) return;
    lfbm5d_view_params v;
    lfbm5d_view_defaults(&v);
    out->max_disparity = 4;
    out->box_radius = 3;
    out->ang_radius = 1;
    out->min_valid = 3;                      /* the rule and the sweep of profiles/repair_defaults.txt */
    out->iterations = v.iterations;
    out->sigma_start = v.sigma_start;
    out->sigma_end = v.sigma_end;
    out->sigma_noise = v.sigma_noise;
}

int lfbm5d_repair_fill_device(lfbm5d_ctx* c, const lfbm5d_repair_params* rp, const float* d_in, const unsigned char* d_flags_in,
                              const unsigned* h_mask, const unsigned* h_missing, float* d_out, unsigned char* d_codes, signed char* d_disp,
                              unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C,
                              lfbm5d_repair_result* out) {
    if (!c) return 1;
    lfbm5d_repair_result r;
    const unsigned char* codes = nullptr;
    const int rc = fill(c, "lfbm5d_repair_fill_device: ", rp, d_in, d_flags_in, h_mask, h_missing, d_out, d_codes, d_disp, ang_major, awidth,
                        aheight, W, H, C, r, &codes);
    if (out) *out = r;
    return rc;
}

int lfbm5d_repair_device(lfbm5d_ctx* c, const lfbm5d_repair_params* rp, const lfbm5d_params* P, const float* d_in,
                         const unsigned char* d_flags_in, const unsigned* h_mask, const unsigned* h_missing, float* d_out,
                         unsigned char* d_codes, signed char* d_disp, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                         unsigned W, unsigned H, unsigned C, lfbm5d_repair_result* out) {
    if (!c) return 1;
    return repair(c, "lfbm5d_repair_device: ", rp, P, d_in, d_flags_in, h_mask, h_missing, d_out, d_codes, d_disp, ang_major, awidth, aheight,
                  an, W, H, C, out);
}

int lfbm5d_repair_host_sai(lfbm5d_ctx* c, const lfbm5d_repair_params* rp, const lfbm5d_params* P, const float* const* h_in,
                           const unsigned char* const* h_flags_in, const unsigned* h_mask, const unsigned* h_missing, float* const* h_out,
                           unsigned char* const* h_codes, signed char* const* h_disp, unsigned ang_major, unsigned awidth, unsigned aheight,
                           unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_repair_result* out) {
    if (!c) return 1;
    const std::string who = "lfbm5d_repair_host_sai: ";
    if (!rp || !P || !h_in || !h_out || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const unsigned asize = awidth * aheight;
    const size_t plane = (size_t)W * H, img = (size_t)C * plane, all = std::max<size_t>(1, (size_t)asize * img);
    const size_t positions = std::max<size_t>(1, (size_t)asize * plane);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_out, asize, nonempty) || (h_codes && check_planes(c, who, h_codes, asize, nonempty)) ||
        (h_disp && check_planes(c, who, h_disp, asize, nonempty))) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    HIPCK(c, c->h2d_out.reserve(all * sizeof(float)));
    HIPCK(c, c->repair.host.reserve(2 * all + positions));
    float* const din = c->h2d_noisy.as<float>(); float* const dout = c->h2d_out.as<float>();
    unsigned char* const dfi = c->repair.host.as<unsigned char>(); unsigned char* const dco = dfi + all;
    signed char* const ddi = reinterpret_cast<signed char*>(dco + all);
    if (upload_planes(c, who, h_in, din, asize, img, nonempty)) return 1;
    if (h_flags_in && upload_planes(c, who, h_flags_in, dfi, asize, img, nonempty)) return 1;
    if (h_disp) HIPCK(c, hipMemsetAsync(ddi, 0, positions, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    lfbm5d_repair_result r;
    std::memset(&r, 0, sizeof(r));
    const int rc = repair(c, who, rp, P, din, h_flags_in ? dfi : nullptr, h_mask, h_missing, dout, h_codes ? dco : nullptr, h_disp ? ddi : nullptr,
                          ang_major, awidth, aheight, an, W, H, C, &r);
    if (out) *out = r;
    if (rc && !r.targets) return 1;                                         /* refused ahead of the fill: nothing to hand back */
    if (download_planes(c, h_out, dout, asize, img, nonempty) || (h_codes && download_planes(c, h_codes, dco, asize, img, nonempty)) ||
        (h_disp && download_planes(c, h_disp, ddi, asize, plane, nonempty))) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return rc;
}

} /* extern "C" */
