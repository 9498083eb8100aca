/*
 * lfbm5d_impulse.hip -- impulse-noise repair ahead of the denoiser (lfbm5d_impulse_*, include/lfbm5d.h): hot and dead pixels, salt and
 * pepper, drop-outs written as 0, 255 or NaN are found by their rank-ordered absolute differences (ROAD, Garnett et al., IEEE TIP 2005)
 * against a threshold taken from the light field's own median ROAD, and replaced by the lower median of their sound neighbours.  Not in
 * the reference, whose authors run such a stage in front of it.
 *
 * Kernels (256 threads, tiles of 64 x 32 pixels of one channel plane staged in LDS with the plane's mirror applied while loading, so a
 * pixel comes from HBM once per tile that touches it and every neighbour access is an LDS read):
 *   k_impulse_stats    grid (workgroups, channel); a workgroup walks over its channel's tiles (one-pixel halo), computes R of every
 *                      pixel -- eight differences, two sorted fours, a half cleaner and a bitonic four: 18 min/max pairs -- and counts
 *                      its key in the channel's 386 LDS counters (32-bit LDS atomics); at the end one 64-bit global atomic per non-zero
 *                      counter.  Integers only: the result does not depend on any order.
 *   k_impulse_repair   grid (tiles, SAI x channel); two-pixel halo; the flags of the tile plus one ring go to LDS (detected from R, the
 *                      threshold and the extremeness test, or loaded from the caller's flag plane), barrier, then every pixel of the
 *                      tile is copied or replaced, its flag byte written and the counts added (LDS, then two global integer atomics
 *                      per workgroup).
 * Non-finite values are decided by explicit tests on the bits before any min / max: the hardware's min / max drop a NaN operand.
 * The quantile of a histogram runs on the host in double.
 */
#include "lfbm5d_side.h"

using namespace lfbm5d_host;
using namespace lfbm5d_side;

namespace {

constexpr int kS1 = kTW + 2, kR1 = kTH + 2;          /* tile with one ring */
constexpr int kS2 = kTW + 4, kR2 = kTH + 4;          /* tile with two rings */
static_assert(kKeys == LFBM5D_IMPULSE_KEYS, "include/lfbm5d.h");

#define CSWAP_F(a, b) { const float lo_ = fminf(a, b), hi_ = fmaxf(a, b); a = lo_; b = hi_; }
#define CSWAP_I(a, b) { const int lo_ = min(a, b), hi_ = max(a, b); a = lo_; b = hi_; }

/* the four smallest of eight, ascending: d[0..3].  No operand is a NaN (callers decide non-finite values first). */
__device__ __forceinline__ void smallest4(float* d) {
    CSWAP_F(d[0], d[1]) CSWAP_F(d[2], d[3]) CSWAP_F(d[0], d[2]) CSWAP_F(d[1], d[3]) CSWAP_F(d[1], d[2])
    CSWAP_F(d[4], d[5]) CSWAP_F(d[6], d[7]) CSWAP_F(d[4], d[6]) CSWAP_F(d[5], d[7]) CSWAP_F(d[5], d[6])
    d[0] = fminf(d[0], d[7]); d[1] = fminf(d[1], d[6]); d[2] = fminf(d[2], d[5]); d[3] = fminf(d[3], d[4]);
    CSWAP_F(d[0], d[2]) CSWAP_F(d[1], d[3]) CSWAP_F(d[0], d[1]) CSWAP_F(d[2], d[3])
}
__device__ __forceinline__ void smallest4(int* d) {
    CSWAP_I(d[0], d[1]) CSWAP_I(d[2], d[3]) CSWAP_I(d[0], d[2]) CSWAP_I(d[1], d[3]) CSWAP_I(d[1], d[2])
    CSWAP_I(d[4], d[5]) CSWAP_I(d[6], d[7]) CSWAP_I(d[4], d[6]) CSWAP_I(d[5], d[7]) CSWAP_I(d[5], d[6])
    d[0] = min(d[0], d[7]); d[1] = min(d[1], d[6]); d[2] = min(d[2], d[5]); d[3] = min(d[3], d[4]);
    CSWAP_I(d[0], d[2]) CSWAP_I(d[1], d[3]) CSWAP_I(d[0], d[1]) CSWAP_I(d[2], d[3])
}

/* R and the extremeness of the pixel at v[0] of an LDS tile of row stride S */
template <int S>
__device__ __forceinline__ float road(const float* v, bool& extreme) {
    const int off[8] = {-S - 1, -S, -S + 1, -1, 1, S - 1, S, S + 1};
    const float c = v[0];
    const bool cf = finite_bits(c);
    float d[8];
    int lt = 0, gt = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float q = v[off[i]];
        const bool qf = finite_bits(q);
        d[i] = (cf && qf) ? fabsf(c - q) : __builtin_inff();
        lt += (qf && q < c) ? 1 : 0;
        gt += (qf && q > c) ? 1 : 0;
    }
    smallest4(d);
    extreme = lt == 0 || gt == 0;
    return ((d[0] + d[1]) + d[2]) + d[3];
}

__device__ __forceinline__ int key_of(float R) { return min(max((int)(__float_as_uint(R) >> 19) - kKeyBase + 1, 0), kKeys - 1); }

/* grid (workgroups, C), 256 threads.  hist [C][386], skipped [1]: accumulated into. */
__global__ __launch_bounds__(kThreads) void k_impulse_stats(const float* __restrict__ lf, const unsigned* __restrict__ sai, unsigned nne, unsigned C,
                                                            unsigned W, unsigned H, unsigned tx_n, unsigned ty_n,
                                                            unsigned long long* __restrict__ hist, unsigned long long* __restrict__ skipped) {
    __shared__ float v[kR1 * kS1];
    __shared__ unsigned h[kKeys];
    const unsigned tid = threadIdx.x, c = blockIdx.y;
    for (unsigned i = tid; i < kKeys; i += kThreads) h[i] = 0u;
    const unsigned long long tpp = (unsigned long long)tx_n * ty_n, total = tpp * nne;
    unsigned skip = 0;
    for (unsigned long long t = blockIdx.x; t < total; t += gridDim.x) {
        const unsigned k = (unsigned)(t / tpp), r = (unsigned)(t - (unsigned long long)k * tpp);
        const unsigned ty = r / tx_n, tx = r - ty * tx_n;
        const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
        const float* plane = lf + ((size_t)sai[k] * C + c) * (size_t)W * H;
        __syncthreads();   /* the tile of the previous round has been read (first round: the counters are zero) */
        for (int i = tid; i < kR1 * kS1; i += kThreads) {
            const int ly = i / kS1, lx = i - ly * kS1;
            v[i] = plane[(size_t)mirror(y0 + ly - 1, (int)H) * W + mirror(x0 + lx - 1, (int)W)];
        }
        __syncthreads();
        for (int i = tid; i < kTH * kTW; i += kThreads) {
            const int ly = i / kTW, lx = i - ly * kTW;
            if (y0 + ly >= (int)H || x0 + lx >= (int)W) continue;
            bool extreme;
            const float R = road<kS1>(&v[(ly + 1) * kS1 + lx + 1], extreme);
            if (!finite_bits(R)) skip++;
            else atomicAdd(&h[key_of(R)], 1u);
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < kKeys; i += kThreads)
        if (h[i]) atomicAdd(&hist[(size_t)c * kKeys + i], (unsigned long long)h[i]);
    if (skip) atomicAdd(skipped, (unsigned long long)skip);
}

/* grid (tx_n * ty_n, nne * C), 256 threads.  counts [asize][C][2] (repaired, left): accumulated into.  GIVEN: the flags come from
 * flags_in (non-zero = defective) and thr is unused; flags_out may be NULL. */
template <bool GIVEN>
__global__ __launch_bounds__(kThreads) void k_impulse_repair(const float* __restrict__ in, const unsigned char* __restrict__ flags_in,
                                                             float* __restrict__ out, unsigned char* __restrict__ flags_out,
                                                             const unsigned* __restrict__ sai, unsigned C, unsigned W, unsigned H, unsigned tx_n,
                                                             Thresholds thr, unsigned long long* __restrict__ counts) {
    __shared__ float v[kR2 * kS2];
    __shared__ unsigned char f[kR1 * kS1];
    __shared__ unsigned cnt[2];
    const unsigned tid = threadIdx.x, ac = blockIdx.y, ch = ac % C;
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
    const size_t base = ((size_t)sai[ac / C] * C + ch) * (size_t)W * H;
    if (tid < 2) cnt[tid] = 0u;
    for (int i = tid; i < kR2 * kS2; i += kThreads) {
        const int ly = i / kS2, lx = i - ly * kS2;
        v[i] = in[base + (size_t)mirror(y0 + ly - 2, (int)H) * W + mirror(x0 + lx - 2, (int)W)];
    }
    if (GIVEN) {
        for (int i = tid; i < kR1 * kS1; i += kThreads) {
            const int ly = i / kS1, lx = i - ly * kS1;
            f[i] = flags_in[base + (size_t)mirror(y0 + ly - 1, (int)H) * W + mirror(x0 + lx - 1, (int)W)] ? 1 : 0;
        }
    } else {
        __syncthreads();
        const float T = ch == 0 ? thr.t[0] : ch == 1 ? thr.t[1] : thr.t[2];
        for (int i = tid; i < kR1 * kS1; i += kThreads) {
            const int ly = i / kS1, lx = i - ly * kS1;
            const float* p = &v[(ly + 1) * kS2 + lx + 1];
            bool extreme;
            const float R = road<kS2>(p, extreme);
            f[i] = (!finite_bits(p[0]) || (R > T && extreme)) ? 1 : 0;
        }
    }
    __syncthreads();
    for (int i = tid; i < kTH * kTW; i += kThreads) {
        const int ly = i / kTW, lx = i - ly * kTW;
        if (y0 + ly >= (int)H || x0 + lx >= (int)W) continue;
        const float* p = &v[(ly + 2) * kS2 + lx + 2];
        const unsigned char* fp = &f[(ly + 1) * kS1 + lx + 1];
        float res = p[0];
        unsigned char code = 0;
        if (fp[0]) {
            const int offv[8] = {-kS2 - 1, -kS2, -kS2 + 1, -1, 1, kS2 - 1, kS2, kS2 + 1};
            const int offf[8] = {-kS1 - 1, -kS1, -kS1 + 1, -1, 1, kS1 - 1, kS1, kS1 + 1};
            int key[8], n = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float q = p[offv[j]];
                const bool ok = !fp[offf[j]] && finite_bits(q);
                const int b = (int)__float_as_uint(q);
                key[j] = ok ? (b ^ ((b >> 31) & 0x7fffffff)) : 0x7fffffff;   /* ascending order of the values, -0 before +0 */
                n += ok ? 1 : 0;
            }
            if (n) {
                smallest4(key);
                const int m = (n - 1) >> 1;                                  /* 0..3 */
                const int kk = m == 0 ? key[0] : m == 1 ? key[1] : m == 2 ? key[2] : key[3];
                res = __uint_as_float((unsigned)(kk ^ ((kk >> 31) & 0x7fffffff)));
                code = 1;
            } else code = 2;
            atomicAdd(&cnt[code - 1], 1u);
        }
        const size_t at = base + (size_t)(y0 + ly) * W + (x0 + lx);
        out[at] = res;
        if (flags_out) flags_out[at] = code;
    }
    __syncthreads();
    if (tid < 2 && cnt[tid]) atomicAdd(&counts[(size_t)(sai[ac / C] * C + ch) * 2 + tid], (unsigned long long)cnt[tid]);
}

/* lower edge of key k (1 <= k <= 385) as a double: the float whose bits are (k - 1 + base) << 19; key 0 starts at 0 */
double key_edge(int k) {
    if (k <= 0) return 0.0;
    const unsigned bits = (unsigned)(k - 1 + kKeyBase) << 19;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return (double)f;
}

/* include/lfbm5d.h, lfbm5d_impulse_scale */
int scale_of(const unsigned long long* h, double* s) {
    unsigned long long n = 0;
    for (int k = 0; k < kKeys; k++) n += h[k];
    if (!n) return 1;
    const double T = 0.5 * (double)n;
    unsigned long long cum = 0, before = 0;
    int ks = 0;
    for (; ks < kKeys; ks++) {
        before = cum;
        cum += h[ks];
        if ((double)cum >= T) break;
    }
    if (ks >= kKeys - 1) { *s = key_edge(kKeys - 1); return 0; }
    const double e0 = key_edge(ks), e1 = key_edge(ks + 1);
    *s = e0 + (e1 - e0) * (T - (double)before) / (double)h[ks];
    return 0;
}

/* prepare_tiled's stage arguments */
constexpr const char* kOneGpu = "the impulse routines run on one GPU (this context has a communicator or a shard)";
constexpr unsigned long long kMaxPlane = 0x7fffffffull;

/* hist [C][386] (host) of the light field in HBM; after prepare_tiled() */
int histogram(lfbm5d_ctx* c, const Shape& s, const float* d_lf, unsigned W, unsigned H, unsigned C, unsigned long long* h_hist,
              unsigned long long* skipped) {
    const size_t nh = (size_t)C * kKeys, words = nh + 1;
    HIPCK(c, c->imp.stats.reserve(words * sizeof(unsigned long long)));
    unsigned long long* d = c->imp.stats.as<unsigned long long>();
    HIPCK(c, hipMemsetAsync(d, 0, words * sizeof(unsigned long long), c->stream));
    int n_cu = 0;
    HIPCK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    const unsigned long long total = (unsigned long long)s.tx_n * s.ty_n * s.nne;
    const unsigned wgs = (unsigned)std::min<unsigned long long>(total, std::max(1u, (unsigned)std::max(1, n_cu) * 8u / C));
    hipLaunchKernelGGL(k_impulse_stats, dim3(wgs, C), dim3(kThreads), 0, c->stream, d_lf, c->side.sai.as<unsigned>(), s.nne, C, W, H, s.tx_n, s.ty_n,
                       d, d + nh);
    HIPCK(c, hipGetLastError());
    std::vector<unsigned long long> host(words);
    HIPCK(c, hipMemcpyAsync(host.data(), d, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_hist, host.data(), nh * sizeof(unsigned long long));
    *skipped = host[nh];
    return 0;
}

/* detection + repair (d_flags_in NULL) or repair under given flags; include/lfbm5d.h */
int repair(lfbm5d_ctx* c, const std::string& who, const lfbm5d_impulse_params* P, const float* d_in, const unsigned char* d_flags_in,
           const unsigned* h_mask, float* d_out, unsigned char* d_flags_out, unsigned asize, unsigned W, unsigned H, unsigned C,
           lfbm5d_impulse_result* res, unsigned long long* h_counts_sai, bool given) {
    if (!d_in || !d_out || !h_mask || (given ? !d_flags_in : !P)) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const size_t values = (size_t)asize * C * W * H;
    if (overlap(d_in, values * sizeof(float), d_out, values * sizeof(float)))
        return fail(c, who + "d_out must not alias d_in (neighbours are read across tile edges)");
    if (given && d_flags_out && overlap(d_flags_in, values, d_flags_out, values))
        return fail(c, who + "d_flags_out must not alias d_flags_in (neighbours are read across tile edges)");
    if (!given) {
        if (!(P->k >= 0.0) || !std::isfinite(P->k) || !(P->min_threshold >= 0.0) || !std::isfinite(P->min_threshold))
            return fail(c, who + "k and min_threshold must be finite and not negative");
        for (unsigned ch = 0; ch < C; ch++)
            if (std::isnan(P->threshold[ch]) || std::isinf(P->threshold[ch])) return fail(c, who + "threshold must be finite (<= 0: take k x scale)");
    }
    Shape s;
    if (prepare_tiled(c, who, kOneGpu, h_mask, asize, W, H, C, kMaxPlane, s)) return 1;
    lfbm5d_impulse_result r;
    std::memset(&r, 0, sizeof(r));
    r.pixels = (unsigned long long)s.nne * C * W * H;
    Thresholds thr = {{0.0f, 0.0f, 0.0f}};
    if (!given) {
        bool need = false;
        for (unsigned ch = 0; ch < C; ch++) need = need || !(P->threshold[ch] > 0.0);
        std::vector<unsigned long long> hist((size_t)C * kKeys, 0ull), pooled(kKeys, 0ull);
        if (need) {
            if (histogram(c, s, d_in, W, H, C, hist.data(), &r.skipped)) return 1;
            for (unsigned ch = 0; ch < C; ch++) {
                for (int k = 0; k < kKeys; k++) pooled[k] += hist[(size_t)ch * kKeys + k];
                if (scale_of(&hist[(size_t)ch * kKeys], &r.scale_channel[ch])) r.scale_channel[ch] = 0.0;   /* nothing finite: scale 0 */
            }
            if (scale_of(pooled.data(), &r.scale)) r.scale = 0.0;
        }
        for (unsigned ch = 0; ch < C; ch++) {
            const double T = P->threshold[ch] > 0.0 ? P->threshold[ch] : std::max(P->k * r.scale_channel[ch], P->min_threshold);
            thr.t[ch] = (float)T;
            r.threshold[ch] = (double)thr.t[ch];
        }
    }
    const size_t nc = (size_t)asize * C * 2;
    HIPCK(c, c->imp.stats.reserve(nc * sizeof(unsigned long long)));
    unsigned long long* d_cnt = c->imp.stats.as<unsigned long long>();
    HIPCK(c, hipMemsetAsync(d_cnt, 0, nc * sizeof(unsigned long long), c->stream));
    const dim3 grid(s.tx_n * s.ty_n, s.nne * C);
    if (given) hipLaunchKernelGGL((k_impulse_repair<true>), grid, dim3(kThreads), 0, c->stream, d_in, d_flags_in, d_out, d_flags_out,
                                  c->side.sai.as<unsigned>(), C, W, H, s.tx_n, thr, d_cnt);
    else hipLaunchKernelGGL((k_impulse_repair<false>), grid, dim3(kThreads), 0, c->stream, d_in, d_flags_in, d_out, d_flags_out,
                            c->side.sai.as<unsigned>(), C, W, H, s.tx_n, thr, d_cnt);
    HIPCK(c, hipGetLastError());
    std::vector<unsigned long long> cnt(nc);
    HIPCK(c, hipMemcpyAsync(cnt.data(), d_cnt, nc * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (unsigned st = 0; st < asize; st++)
        for (unsigned ch = 0; ch < C; ch++) {
            const unsigned long long rep = cnt[((size_t)st * C + ch) * 2], left = cnt[((size_t)st * C + ch) * 2 + 1];
            r.repaired[ch] += rep; r.left[ch] += left; r.flagged[ch] += rep + left;
            if (h_counts_sai) {
                unsigned long long* o = h_counts_sai + ((size_t)st * C + ch) * 3;
                o[0] = rep + left; o[1] = rep; o[2] = left;
            }
        }
    if (res) *res = r;
    return 0;
}

} /* namespace */

extern "C" {

void lfbm5d_impulse_defaults(lfbm5d_impulse_params* out) {
    if (!out) return;
    out->k = 8.0;
    out->min_threshold = 0.0;
    out->threshold[0] = out->threshold[1] = out->threshold[2] = 0.0;
}

int lfbm5d_impulse_scale(const unsigned long long* hist, double* scale) {
    if (!hist || !scale) return 1;
    return scale_of(hist, scale);
}

int lfbm5d_impulse_histogram_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                                    unsigned long long* h_hist, unsigned long long* pixels, unsigned long long* skipped) {
    if (!c) return 1;
    const std::string who = "lfbm5d_impulse_histogram_device: ";
    if (!d_lf || !h_mask || !h_hist) return fail(c, who + "NULL pointer for a required buffer");
    Shape s;
    if (prepare_tiled(c, who, kOneGpu, h_mask, asize, W, H, C, kMaxPlane, s)) return 1;
    unsigned long long skip = 0;
    if (histogram(c, s, d_lf, W, H, C, h_hist, &skip)) return 1;
    if (pixels) *pixels = (unsigned long long)s.nne * C * W * H;
    if (skipped) *skipped = skip;
    return 0;
}

int lfbm5d_impulse_repair_device(lfbm5d_ctx* c, const lfbm5d_impulse_params* P, const float* d_in, const unsigned* h_mask, float* d_out,
                                 unsigned char* d_flags, unsigned asize, unsigned W, unsigned H, unsigned C, lfbm5d_impulse_result* out,
                                 unsigned long long* h_counts_sai) {
    if (!c) return 1;
    return repair(c, "lfbm5d_impulse_repair_device: ", P, d_in, nullptr, h_mask, d_out, d_flags, asize, W, H, C, out, h_counts_sai, false);
}

int lfbm5d_impulse_repair_flags_device(lfbm5d_ctx* c, const float* d_in, const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out,
                                       unsigned char* d_flags, unsigned asize, unsigned W, unsigned H, unsigned C, lfbm5d_impulse_result* out,
                                       unsigned long long* h_counts_sai) {
    if (!c) return 1;
    return repair(c, "lfbm5d_impulse_repair_flags_device: ", nullptr, d_in, d_flags_in, h_mask, d_out, d_flags, asize, W, H, C, out, h_counts_sai,
                  true);
}

int lfbm5d_impulse_repair_host_sai(lfbm5d_ctx* c, const lfbm5d_impulse_params* P, const float* const* h_in, const unsigned char* const* h_flags_in,
                                   const unsigned* h_mask, float* const* h_out, unsigned char* const* h_flags, unsigned asize, unsigned W,
                                   unsigned H, unsigned C, lfbm5d_impulse_result* out, unsigned long long* h_counts_sai) {
    if (!c) return 1;
    const std::string who = "lfbm5d_impulse_repair_host_sai: ";
    if (!h_in || !h_out || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const size_t img = (size_t)C * W * H, all = std::max<size_t>(1, (size_t)asize * img);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_out, asize, nonempty) || (h_flags && check_planes(c, who, h_flags, asize, nonempty))) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    HIPCK(c, c->h2d_out.reserve(all * sizeof(float)));
    HIPCK(c, c->imp.flags.reserve(2 * all));
    float* const din = c->h2d_noisy.as<float>(); float* const dout = c->h2d_out.as<float>();
    unsigned char* const dfi = c->imp.flags.as<unsigned char>(); unsigned char* const dfo = dfi + all;
    if (upload_planes(c, who, h_in, din, asize, img, nonempty) || (h_flags_in && upload_planes(c, who, h_flags_in, dfi, asize, img, nonempty))) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (repair(c, who, P, din, h_flags_in ? dfi : nullptr, h_mask, dout, h_flags ? dfo : nullptr, asize, W, H, C, out, h_counts_sai,
               h_flags_in != nullptr)) return 1;
    if (download_planes(c, h_out, dout, asize, img, nonempty) || (h_flags && download_planes(c, h_flags, dfo, asize, img, nonempty))) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* extern "C" */
