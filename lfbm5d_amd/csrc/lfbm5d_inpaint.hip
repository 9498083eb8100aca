/*
 * lfbm5d_inpaint.hip -- defect inpainting ahead of the denoiser (lfbm5d_inpaint_*, include/lfbm5d.h): regions named by a defect map
 * (dead columns, dust shadows, hot clusters, holes of non-finite values, regions the user masks out) are filled from their rim inwards
 * (onion peel: a flagged value becomes the mean of its sound 3 x 3 neighbours, pass by pass), and the fill is refined by the loop
 * "regularise with the hard-thresholding step, put the sound data back, lower sigma" -- super-resolution's scheme (lfbm5d_resample.hip)
 * with a mask as the operator.  Not in the reference.
 *
 * Kernels (256 threads):
 *   k_inpaint_fill     grid (tiles, SAI x channel); a tile of 64 x 32 values of one channel plane plus a halo of R = 8 goes into LDS,
 *                      values and states, with the plane's mirror applied while loading.  Up to R Jacobi passes run inside LDS: every
 *                      thread computes the new values of its 15 cells into registers, barrier, writes them, barrier.  A cell at
 *                      distance d of the tile is exact through pass R - d, which is all the tile ever reads of it, so the tile is exact
 *                      through R passes.  A cell outside the plane is computed from the neighbourhood of the cell it mirrors (the same
 *                      operands in the same order: the same bits as the plane's own value).  A tile without a flagged value is copied
 *                      before its halo is loaded; the passes end when the tile is full or a pass fills nothing in the whole window.
 *                      Regions deeper than R take further launches on the ping-ponged state.
 *   k_inpaint_project  out = flag ? x : y, 16 bytes per lane where the planes allow it.
 * Sums in a fixed order, one product with a table entry, integer atomics for the counts: the GPU equals tests/inpaint_model.py bit for
 * bit, however the passes fall into launches.
 */
#include "lfbm5d_side.h"

using namespace lfbm5d_host;
using namespace lfbm5d_side;

namespace {

constexpr int kR = LFBM5D_INPAINT_PASSES_PER_LAUNCH;
constexpr int kWW = kTW + 2 * kR, kWH = kTH + 2 * kR;       /* the window: tile + halo, 80 x 48 */
constexpr int kCells = kWW * kWH, kPer = kCells / kThreads;   /* 3840 cells, 15 per thread */
constexpr unsigned kNone = 0xffffu;
static_assert(kCells % kThreads == 0 && kPer <= 16 && kCells < (int)kNone, "cells per thread");
/* counters of one launch: [0..2] filled (accumulated over the launches), [3..5] still flagged (of this launch), [6] last pass */
constexpr int kCntFilled = 0, kCntRemain = 3, kCntPass = 6, kCntWords = 7;

/* states of a value: the codes of the flag plane (include/lfbm5d.h); kOpen is "left" once no pass can fill it */
constexpr unsigned char kSound = 0, kFilled = 1, kOpen = 2;

/* r[n] = (float)(1.0 / n) */
__constant__ float kRecip[9] = {0.0f, 1.0f, 0.5f, (float)(1.0 / 3.0), 0.25f, (float)(1.0 / 5.0), (float)(1.0 / 6.0), (float)(1.0 / 7.0), 0.125f};

/* grid (tx_n * ty_n, nne * C), 256 threads.  FIRST: st_in is the caller's defect map (non-zero = defective) and a non-finite value is
 * flagged too; otherwise st_in holds the states the previous launch wrote.  pass_base = the passes run by earlier launches. */
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void k_inpaint_fill(const float* __restrict__ in, const unsigned char* __restrict__ st_in,
                                                           float* __restrict__ out, unsigned char* __restrict__ st_out,
                                                           const unsigned* __restrict__ sai, unsigned C, unsigned W, unsigned H, unsigned tx_n,
                                                           unsigned pass_base, unsigned long long* __restrict__ cnt) {
    __shared__ float v[kCells];
    __shared__ unsigned char f[kCells];
    __shared__ unsigned stat[kR + 1];     /* per pass: 1 = a value of the tile was filled, 2 = a cell of the window was, 4 = the tile has open values */
    __shared__ unsigned tally[2];         /* values of the tile filled by this launch, values still open */
    const unsigned tid = threadIdx.x, ac = blockIdx.y, ch = ac % C;
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    const int x0 = (int)(tx * kTW) - kR, y0 = (int)(ty * kTH) - kR;   /* plane coordinates of the window's first cell */
    const size_t base = ((size_t)sai[ac / C] * C + ch) * (size_t)W * H;
    if (tid <= kR) stat[tid] = 0u;
    if (tid < 2) tally[tid] = 0u;

    unsigned canon[kPer];     /* the window cell whose neighbourhood gives this cell's new value; kNone: never updated */
    unsigned tile = 0;        /* bit k: cell k is a value of the tile inside the plane */
    unsigned open0 = 0;       /* bit k: ... and was open when loaded */
    /* the tile first: without an open value it is a copy */
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int i = (int)tid + k * kThreads, ly = i / kWW, lx = i - ly * kWW;
        const int gy = y0 + ly, gx = x0 + lx;
        const bool inner = ly >= kR && ly < kR + kTH && lx >= kR && lx < kR + kTW;
        canon[k] = kNone;
        if (!inner) continue;
        const int my = mirror(gy, (int)H), mx = mirror(gx, (int)W);
        const size_t at = base + (size_t)my * W + mx;
        const float val = in[at];
        unsigned char s = st_in[at];
        if (FIRST) s = (s != 0 || !finite_bits(val)) ? kOpen : kSound;
        v[i] = val; f[i] = s;
        if (my == gy && mx == gx) {
            tile |= 1u << k;
            if (s == kOpen) open0 |= 1u << k;
        }
    }
    if (__syncthreads_or(open0 != 0u)) {
        /* the halo, and every cell's source of new values */
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int i = (int)tid + k * kThreads, ly = i / kWW, lx = i - ly * kWW;
            const int gy = y0 + ly, gx = x0 + lx;
            const bool inner = ly >= kR && ly < kR + kTH && lx >= kR && lx < kR + kTW;
            const int my = mirror(gy, (int)H), mx = mirror(gx, (int)W);
            if (!inner) {
                const size_t at = base + (size_t)my * W + mx;
                const float val = in[at];
                unsigned char s = st_in[at];
                if (FIRST) s = (s != 0 || !finite_bits(val)) ? kOpen : kSound;
                v[i] = val; f[i] = s;
            }
            const int cy = my - y0, cx = mx - x0;   /* the mirrored cell inside the window, if it is there */
            const bool ring = ly == 0 || ly == kWH - 1 || lx == 0 || lx == kWW - 1;
            if (!ring && cy >= 1 && cy < kWH - 1 && cx >= 1 && cx < kWW - 1) canon[k] = (unsigned)(cy * kWW + cx);
        }
        __syncthreads();
        unsigned last = 0;
        for (int j = 1; j <= kR; j++) {
            float nv[kPer];
            unsigned mark = 0, bits = 0;
#pragma unroll
            for (int k = 0; k < kPer; k++) {
                const unsigned c = canon[k];
                if (c == kNone || f[c] != kOpen) continue;
                const int off[8] = {-kWW - 1, -kWW, -kWW + 1, -1, 1, kWW - 1, kWW, kWW + 1};
                float s = 0.0f;
                int n = 0;
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const bool ok = f[(int)c + off[q]] != kOpen;
                    const float val = v[(int)c + off[q]];
                    s = ok ? s + val : s;
                    n += ok ? 1 : 0;
                }
                const bool mine = (tile >> k) & 1u;
                if (n) {
                    nv[k] = s * kRecip[n];
                    mark |= 1u << k;
                    bits |= mine ? 3u : 2u;
                } else if (mine) bits |= 4u;
            }
            if (bits) atomicOr(&stat[j], bits);
            __syncthreads();   /* every read of the state before this pass is done */
#pragma unroll
            for (int k = 0; k < kPer; k++)
                if ((mark >> k) & 1u) {
                    const int i = (int)tid + k * kThreads;
                    v[i] = nv[k]; f[i] = kFilled;
                }
            __syncthreads();
            const unsigned b = stat[j];
            if (b & 1u) last = (unsigned)j;
            if (!(b & 4u) || !(b & 2u)) break;   /* the tile is full, or nothing in reach can be filled */
        }
        if (tid == 0 && last) atomicMax(&cnt[kCntPass], (unsigned long long)(pass_base + last));
    }
    unsigned filled = 0, remain = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (!((tile >> k) & 1u)) continue;
        const int i = (int)tid + k * kThreads, ly = i / kWW, lx = i - ly * kWW;
        const size_t at = base + (size_t)(y0 + ly) * W + (size_t)(x0 + lx);
        const unsigned char s = f[i];
        out[at] = v[i];
        st_out[at] = s;
        if ((open0 >> k) & 1u) { if (s == kOpen) remain++; else filled++; }
    }
    if (filled) atomicAdd(&tally[0], filled);
    if (remain) atomicAdd(&tally[1], remain);
    __syncthreads();
    if (tid < 2 && tally[tid]) atomicAdd(&cnt[(tid ? kCntRemain : kCntFilled) + ch], (unsigned long long)tally[tid]);
}

/* grid (blocks, nne), 256 threads; n = values of one SAI (C*H*W).  VEC: n is a multiple of 4 and the four pointers are 16-byte aligned
 * (flags: 4-byte): a lane moves four values.  out may be x or y. */
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_inpaint_project(const unsigned char* __restrict__ fl, const float* x, const float* y, float* out,
                                                              const unsigned* __restrict__ sai, size_t n) {
    const size_t base = (size_t)sai[blockIdx.y] * n;
    const size_t step = (size_t)gridDim.x * kThreads;
    if (VEC) {
        const uchar4* f4 = reinterpret_cast<const uchar4*>(fl + base);
        const float4* x4 = reinterpret_cast<const float4*>(x + base);
        const float4* y4 = reinterpret_cast<const float4*>(y + base);
        float4* o4 = reinterpret_cast<float4*>(out + base);
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n / 4; i += step) {
            const uchar4 f = f4[i];
            const float4 a = x4[i], b = y4[i];
            float4 r;
            r.x = f.x ? a.x : b.x; r.y = f.y ? a.y : b.y; r.z = f.z ? a.z : b.z; r.w = f.w ? a.w : b.w;
            o4[i] = r;
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += step) out[base + i] = fl[base + i] ? x[base + i] : y[base + i];
    }
}

/* prepare_tiled's stage arguments */
constexpr const char* kOneGpu = "the inpainting routines run on one GPU (this context has a communicator or a shard)";
constexpr unsigned long long kMaxPlane = 0x3fffffffull;

/* out = flag ? x : y on the non-empty SAIs; after prepare_tiled(); asynchronous on the context's stream */
int project(lfbm5d_ctx* c, const Shape& s, const unsigned char* d_flags, const float* d_x, const float* d_y, float* d_out, unsigned W,
            unsigned H, unsigned C) {
    const size_t n = (size_t)C * W * H;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_out);
    const bool vec = n % 4 == 0 && bits % 16 == 0 && reinterpret_cast<uintptr_t>(d_flags) % 4 == 0;
    const size_t items = vec ? n / 4 : n;
    const dim3 grid((unsigned)std::min<size_t>((items + kThreads - 1) / kThreads, 4096), s.nne);
    if (vec) hipLaunchKernelGGL((k_inpaint_project<true>), grid, dim3(kThreads), 0, c->stream, d_flags, d_x, d_y, d_out, c->side.sai.as<unsigned>(), n);
    else hipLaunchKernelGGL((k_inpaint_project<false>), grid, dim3(kThreads), 0, c->stream, d_flags, d_x, d_y, d_out, c->side.sai.as<unsigned>(), n);
    HIPCK(c, hipGetLastError());
    return 0;
}

/* the onion-peel fill; after prepare_tiled().  On return the stream is idle, d_out holds the result and *d_codes points at the code plane
 * (d_flags_out when given, else the context's scratch). */
int fill(lfbm5d_ctx* c, const Shape& s, const float* d_in, const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out,
         unsigned char* d_flags_out, unsigned asize, unsigned W, unsigned H, unsigned C, lfbm5d_inpaint_result& r,
         const unsigned char** d_codes) {
    const size_t img = (size_t)C * W * H, values = (size_t)asize * img;
    std::memset(&r, 0, sizeof(r));
    r.pixels = (unsigned long long)s.nne * img;
    HIPCK(c, c->inp.stats.reserve(kCntWords * sizeof(unsigned long long)));
    HIPCK(c, c->inp.state[0].reserve(values));
    unsigned long long* d_cnt = c->inp.stats.as<unsigned long long>();
    HIPCK(c, hipMemsetAsync(d_cnt, 0, kCntWords * sizeof(unsigned long long), c->stream));
    const dim3 grid(s.tx_n * s.ty_n, s.nne * C);
    const unsigned* d_sai = c->side.sai.as<unsigned>();
    const float* src = d_in;
    const unsigned char* st_src = d_flags_in;
    unsigned long long cnt[kCntWords], filled_before = 0;
    for (unsigned l = 0;; l++) {
        float* dst = d_out;
        unsigned char* st_dst = d_flags_out ? d_flags_out : c->inp.state[0].as<unsigned char>();
        if (l & 1) {   /* a launch reads what the one before it wrote: odd launches write the scratch light field and the second states */
            HIPCK(c, c->side.lf.reserve(values * sizeof(float)));
            HIPCK(c, c->inp.state[1].reserve(values));
            dst = c->side.lf.as<float>();
            st_dst = c->inp.state[1].as<unsigned char>();
        }
        if (l) HIPCK(c, hipMemsetAsync(d_cnt + kCntRemain, 0, 3 * sizeof(unsigned long long), c->stream));
        if (l == 0) hipLaunchKernelGGL((k_inpaint_fill<true>), grid, dim3(kThreads), 0, c->stream, src, st_src, dst, st_dst, d_sai, C, W, H, s.tx_n,
                                       0u, d_cnt);
        else hipLaunchKernelGGL((k_inpaint_fill<false>), grid, dim3(kThreads), 0, c->stream, src, st_src, dst, st_dst, d_sai, C, W, H, s.tx_n,
                                l * (unsigned)kR, d_cnt);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        r.launches = l + 1;
        src = dst; st_src = st_dst;
        const unsigned long long filled = cnt[0] + cnt[1] + cnt[2], remain = cnt[3] + cnt[4] + cnt[5];
        if (!remain || filled == filled_before) break;   /* full, or a launch that filled nothing: what is open now stays open */
        filled_before = filled;
    }
    if (src != d_out) {
        const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
        if (copy_sais(c, asize, d_out, src, img, sizeof(float), nonempty)) return 1;
        if (d_flags_out && copy_sais(c, asize, d_flags_out, st_src, img, 1, nonempty)) return 1;
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (d_flags_out) st_src = d_flags_out;
    }
    for (unsigned ch = 0; ch < C; ch++) {
        r.filled[ch] = cnt[kCntFilled + ch]; r.left[ch] = cnt[kCntRemain + ch]; r.flagged[ch] = r.filled[ch] + r.left[ch];
    }
    r.passes = (unsigned)cnt[kCntPass];
    *d_codes = st_src;
    return 0;
}

int check_buffers(lfbm5d_ctx* c, const std::string& who, const float* d_in, const unsigned char* d_flags_in, const unsigned* h_mask,
                  float* d_out, unsigned char* d_flags_out, unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!d_in || !d_flags_in || !h_mask || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const size_t values = (size_t)asize * C * W * H;
    if (overlap(d_in, values * sizeof(float), d_out, values * sizeof(float)))
        return fail(c, who + "d_out must not overlap d_in (neighbours are read across tile edges)");
    if (d_flags_out && overlap(d_flags_in, values, d_flags_out, values))
        return fail(c, who + "d_flags must not overlap d_flags_in (neighbours are read across tile edges)");
    return 0;
}

/* include/lfbm5d.h, lfbm5d_inpaint_device */
int inpaint(lfbm5d_ctx* c, const std::string& who, const lfbm5d_inpaint_params* ip, const lfbm5d_params* P, const float* d_in,
            const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out, unsigned char* d_flags_out, unsigned ang_major, unsigned awidth,
            unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_inpaint_result* res) {
    if (!ip || !P) return fail(c, who + "NULL pointer for a required buffer");
    const unsigned asize = awidth * aheight;
    if (check_buffers(c, who, d_in, d_flags_in, h_mask, d_out, d_flags_out, asize, W, H, C)) return 1;
    const LoopSchedule sched = {ip->iterations, ip->sigma_start, ip->sigma_end, ip->sigma_noise};
    if (const char* m = check_schedule(sched)) return fail(c, who + m);
    Shape s;
    if (prepare_tiled(c, who, kOneGpu, h_mask, asize, W, H, C, kMaxPlane, s)) return 1;
    lfbm5d_inpaint_result r;
    const unsigned char* d_codes = nullptr;
    if (fill(c, s, d_in, d_flags_in, h_mask, d_out, d_flags_out, asize, W, H, C, r, &d_codes)) return 1;
    if (res) *res = r;
    if (!sched.iterations) return 0;
    if (r.left[0] + r.left[1] + r.left[2])
        return fail(c, who + "a channel plane without one sound value cannot be refined (mask its SAI as empty, or run the fill alone)");
    /* the step's input is x_{k-1} = flag ? b_{k-1} : y; its output b_k goes over d_out (the fill's result is in d_out by now, so the
     * scratch the fill's odd launches wrote is free) */
    if (refine_loop(c, sched, P, h_mask, s.nne, d_out, ang_major, awidth, aheight, an, W, H, C,
                    [&](unsigned, float* z) { return project(c, s, d_codes, d_out, d_in, z, W, H, C); }, [](unsigned) { return 0; })) return 1;
    if (project(c, s, d_codes, d_out, d_in, d_out, W, H, C)) return 1;       /* x_K */
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

void lfbm5d_inpaint_defaults(lfbm5d_inpaint_params* out) {
    if (!out) return;
    out->iterations = 8;                     /* the best of the sweep in profiles/inpaint_defaults.txt */
    out->sigma_start = 30.0f;
    out->sigma_end = 5.0f;
    out->sigma_noise = 0.0f;
}

int lfbm5d_inpaint_fill_device(lfbm5d_ctx* c, const float* d_in, const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out,
                               unsigned char* d_flags, unsigned asize, unsigned W, unsigned H, unsigned C, lfbm5d_inpaint_result* out) {
    if (!c) return 1;
    const std::string who = "lfbm5d_inpaint_fill_device: ";
    if (check_buffers(c, who, d_in, d_flags_in, h_mask, d_out, d_flags, asize, W, H, C)) return 1;
    Shape s;
    if (prepare_tiled(c, who, kOneGpu, h_mask, asize, W, H, C, kMaxPlane, s)) return 1;
    lfbm5d_inpaint_result r;
    const unsigned char* d_codes = nullptr;
    if (fill(c, s, d_in, d_flags_in, h_mask, d_out, d_flags, asize, W, H, C, r, &d_codes)) return 1;
    if (out) *out = r;
    return 0;
}

int lfbm5d_inpaint_project_device(lfbm5d_ctx* c, const unsigned char* d_flags, const float* d_x, const float* d_y, const unsigned* h_mask,
                                  float* d_out, unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    const std::string who = "lfbm5d_inpaint_project_device: ";
    if (!d_flags || !d_x || !d_y || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    Shape s;
    if (prepare_tiled(c, who, kOneGpu, h_mask, asize, W, H, C, kMaxPlane, s)) return 1;
    if (project(c, s, d_flags, d_x, d_y, d_out, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int lfbm5d_inpaint_device(lfbm5d_ctx* c, const lfbm5d_inpaint_params* ip, const lfbm5d_params* P, const float* d_in,
                          const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out, unsigned char* d_flags, unsigned ang_major,
                          unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_inpaint_result* out) {
    if (!c) return 1;
    return inpaint(c, "lfbm5d_inpaint_device: ", ip, P, d_in, d_flags_in, h_mask, d_out, d_flags, ang_major, awidth, aheight, an, W, H, C, out);
}

int lfbm5d_inpaint_host_sai(lfbm5d_ctx* c, const lfbm5d_inpaint_params* ip, const lfbm5d_params* P, const float* const* h_in,
                            const unsigned char* const* h_flags_in, const unsigned* h_mask, float* const* h_out, unsigned char* const* h_flags,
                            unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C,
                            lfbm5d_inpaint_result* out) {
    if (!c) return 1;
    const std::string who = "lfbm5d_inpaint_host_sai: ";
    if (!ip || !P || !h_in || !h_flags_in || !h_out || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const unsigned asize = awidth * aheight;
    const size_t img = (size_t)C * W * H, all = std::max<size_t>(1, (size_t)asize * img);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_out, asize, nonempty) || (h_flags && check_planes(c, who, h_flags, asize, nonempty))) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    HIPCK(c, c->h2d_out.reserve(all * sizeof(float)));
    HIPCK(c, c->inp.flags.reserve(2 * all));
    float* const din = c->h2d_noisy.as<float>(); float* const dout = c->h2d_out.as<float>();
    unsigned char* const dfi = c->inp.flags.as<unsigned char>(); unsigned char* const dfo = dfi + all;
    if (upload_planes(c, who, h_in, din, asize, img, nonempty) || upload_planes(c, who, h_flags_in, dfi, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (inpaint(c, who, ip, P, din, dfi, h_mask, dout, h_flags ? dfo : nullptr, ang_major, awidth, aheight, an, W, H, C, out)) return 1;
    if (download_planes(c, h_out, dout, asize, img, nonempty) || (h_flags && download_planes(c, h_flags, dfo, asize, img, nonempty))) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* extern "C" */
