/*
 * lfbm5d_clip.hip -- data clipped to a known range lo..hi (8-bit files: 0..255): the noise level from the blocks that the clipping left
 * alone, and the inverse of the clipped mean for the denoised result (lfbm5d_clip_*, lfbm5d_noise_level_clipped_*, lfbm5d_declip_*,
 * lfbm5d_denoise_clipped_*, include/lfbm5d.h).  Not in the reference.
 *
 * Kernels:
 *   k_clip_stats   the 2 x 2 block statistics of the Poisson-Gaussian estimate (lfbm5d_pg.hip: m, d, 64 levels, 322 keys of |d|, integer
 *                  counts) on p' = (p - lo) s, plus per level the blocks that hold a censored pixel (p <= lo or p >= hi) and per channel
 *                  the blocks of whole-numbered pixels.  The same shape as k_pg_stats: grid (workgroups, channel), 1024 threads, the
 *                  channel's histogram in LDS (83 KB: one workgroup per CU), chunks of kUnroll x 1024 blocks with a chunk's loads issued
 *                  before the first is used, 8-byte loads when the rows are 8-byte aligned; LDS integer atomics, then one 64-bit integer
 *                  global atomic per non-zero counter.  The file is compiled without FMA contraction: p' feeds sums.
 *   k_declip       out = clamp(E^-1(in), lo, hi) per value (lfbm5d_clip_values.h: a fixed number of Newton steps on E with erfc from
 *                  the start value in, the first in float, the last in double), rounded once; grid (chunks, SAI x channel), 256 threads, four values per
 *                  thread as one 16-byte load and store when the planes are 16-byte aligned; non-finite values pass through; planes of
 *                  empty SAIs are not touched; in place is fine (pointwise).
 * The fit of sigma to the statistics runs on the host in double (lfbm5d_clip_values.h).
 */
#include "lfbm5d_side.h"
#include "lfbm5d_clip_values.h"

using namespace lfbm5d_host;
using namespace lfbm5d_clip;

namespace {

constexpr int kThreads = 1024;
constexpr int kUnroll = 4;
constexpr int kLdsWords = kLevels * kKeys + kLevels;          /* 32-bit counters: the histogram, the censored blocks */
constexpr size_t kLds = (size_t)kLdsWords * sizeof(unsigned) + kLevels * sizeof(unsigned long long);

/* grid (workgroups, C), 1024 threads, kLds bytes of dynamic LDS.  hist [C][64][322], sum [C][64], cens [C][64], whole [C], skipped [1]:
 * accumulated into. */
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_clip_stats(const float* __restrict__ lf, const unsigned* __restrict__ sai, unsigned nne, unsigned C,
                                                         unsigned W, unsigned H, float lo, float hi, float s,
                                                         unsigned long long* __restrict__ hist, unsigned long long* __restrict__ sum,
                                                         unsigned long long* __restrict__ cens, unsigned long long* __restrict__ whole,
                                                         unsigned long long* __restrict__ skipped) {
    extern __shared__ __attribute__((aligned(16))) unsigned clip_lds[];
    unsigned* h = clip_lds;
    unsigned* cz = clip_lds + kLevels * kKeys;
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(clip_lds + kLdsWords);
    const unsigned tid = threadIdx.x, c = blockIdx.y;
    for (unsigned i = tid; i < (unsigned)kLdsWords; i += kThreads) h[i] = 0u;
    if (tid < kLevels) sm[tid] = 0ull;
    __syncthreads();
    const unsigned WP = W / 2, HP = H / 2;
    const unsigned long long per_sai = (unsigned long long)WP * HP, total = per_sai * nne;
    const unsigned long long chunk = (unsigned long long)kThreads * kUnroll;
    unsigned skip = 0, wh = 0;
    for (unsigned long long q0 = (unsigned long long)blockIdx.x * chunk; q0 < total; q0 += (unsigned long long)gridDim.x * chunk) {
        float p[kUnroll][4];
        bool on[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const unsigned long long q = q0 + (unsigned long long)u * kThreads + tid;
            on[u] = q < total;
            if (!on[u]) continue;
            const unsigned k = (unsigned)(q / per_sai), r = (unsigned)(q - (unsigned long long)k * per_sai);
            const unsigned i = r / WP, j = r - i * WP;
            const float* row = lf + ((size_t)sai[k] * C + c) * (size_t)W * H + (size_t)(2 * i) * W + 2 * j;
            if (VEC) {
                const float2 a = *reinterpret_cast<const float2*>(row), b = *reinterpret_cast<const float2*>(row + W);
                p[u][0] = a.x; p[u][1] = a.y; p[u][2] = b.x; p[u][3] = b.y;
            } else {
                p[u][0] = row[0]; p[u][1] = row[1]; p[u][2] = row[W]; p[u][3] = row[W + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            if (!on[u]) continue;
            bool censored = false, integral = true;
            float t[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float v = p[u][e];
                censored |= v <= lo || v >= hi;
                integral &= v == rintf(v);
                t[e] = (v - lo) * s;
            }
            const float m = ((t[0] + t[1]) + (t[2] + t[3])) * 0.25f;
            const float d = ((t[0] - t[1]) - (t[2] - t[3])) * 0.5f;
            if (!(isfinite(m) && isfinite(d))) { skip++; continue; }
            const float mc = fminf(fmaxf(m, 0.0f), 255.0f);
            const int lev = min(kLevels - 1, (int)(mc * (float)(64.0 / 255.0)));
            const int key = min(max((int)(__float_as_uint(fabsf(d)) >> 19) - kKeyBase + 1, 0), kKeys - 1);
            atomicAdd(&h[lev * kKeys + key], 1u);
            atomicAdd(&sm[lev], (unsigned long long)rintf(mc * 256.0f));
            if (censored) atomicAdd(&cz[lev], 1u);
            wh += integral;
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < (unsigned)(kLevels * kKeys); i += kThreads)
        if (h[i]) atomicAdd(&hist[(size_t)c * kLevels * kKeys + i], (unsigned long long)h[i]);
    if (tid < kLevels) {
        if (sm[tid]) atomicAdd(&sum[c * kLevels + tid], sm[tid]);
        if (cz[tid]) atomicAdd(&cens[c * kLevels + tid], (unsigned long long)cz[tid]);
    }
    if (wh) atomicAdd(&whole[c], (unsigned long long)wh);
    if (skip) atomicAdd(skipped, (unsigned long long)skip);
}

__device__ __forceinline__ float declip_one(const Map& m, float x) {
    return lfbm5d_side::finite_bits(x) ? (float)declip_value(m, (double)x) : x;
}

/* grid (chunks of 1024 values, nne * C), 256 threads, four values per thread; VEC: plane % 4 == 0 and both buffers 16-byte aligned */
template <bool VEC>
__global__ __launch_bounds__(256) void k_declip(const float* in, float* out, const unsigned* __restrict__ sai, unsigned C, unsigned plane, Map m) {
    const unsigned x = (blockIdx.x * 256 + threadIdx.x) * 4, ac = blockIdx.y;
    if (x >= plane) return;
    const size_t at = ((size_t)sai[ac / C] * C + ac % C) * (size_t)plane + x;
    if (VEC) {
        float4 v = *reinterpret_cast<const float4*>(in + at);
        v.x = declip_one(m, v.x); v.y = declip_one(m, v.y); v.z = declip_one(m, v.z); v.w = declip_one(m, v.w);
        *reinterpret_cast<float4*>(out + at) = v;
    } else {
#pragma unroll
        for (unsigned e = 0; e < 4; e++)
            if (x + e < plane) out[at + e] = declip_one(m, in[at + e]);
    }
}

constexpr const char* kOneGpu = "the clipping-aware routines run on one GPU (this context has a communicator or a shard)";
constexpr const char* kBadRange = "the range needs lo < hi, both finite";
constexpr const char* kBadSigma = "sigma must be finite and positive";

/* the kernels see the bounds and the scale as floats: those have to differ and stay finite too */
bool good_range(double lo, double hi) {
    return std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo) && (float)lo < (float)hi && std::isfinite(rescale(lo, hi));
}

struct Counts { std::vector<unsigned long long> hist, sum, cens, whole; unsigned long long blocks = 0, skipped = 0; };

/* the counts (host) of the light field in HBM */
int histogram(lfbm5d_ctx* c, const std::string& who, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
              double lo, double hi, Counts& out) {
    if (!d_lf || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    if (!good_range(lo, hi)) return fail(c, who + kBadRange);
    if (sai_list(c, who, h_mask, asize)) return 1;
    const unsigned nne = (unsigned)c->side.sai_host.size();
    const size_t nh = (size_t)C * kLevels * kKeys, ns = (size_t)C * kLevels, words = nh + 2 * ns + C + 1;
    HIPCK(c, c->clip.stats.reserve(words * sizeof(unsigned long long)));
    unsigned long long* d = c->clip.stats.as<unsigned long long>();
    HIPCK(c, hipMemsetAsync(d, 0, words * sizeof(unsigned long long), c->stream));
    const unsigned long long total = (unsigned long long)(W / 2) * (H / 2) * nne, chunk = (unsigned long long)kThreads * kUnroll;
    int n_cu = 0;
    HIPCK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    const unsigned cus = (unsigned)std::max(1, n_cu);
    const unsigned wgs = (unsigned)std::min<unsigned long long>((total + chunk - 1) / chunk, std::max(1u, cus / C));
    const bool vec = W % 2 == 0 && reinterpret_cast<uintptr_t>(d_lf) % 8 == 0;
    const void* fn = vec ? reinterpret_cast<const void*>(&k_clip_stats<true>) : reinterpret_cast<const void*>(&k_clip_stats<false>);
    HIPCK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));   /* per device: cheap, so every call */
    const float flo = (float)lo, fhi = (float)hi, s = rescale(lo, hi);
    unsigned long long* const dh = d; unsigned long long* const ds = d + nh; unsigned long long* const dc = ds + ns;
    unsigned long long* const dw = dc + ns; unsigned long long* const dk = dw + C;
    if (vec) hipLaunchKernelGGL((k_clip_stats<true>), dim3(wgs, C), dim3(kThreads), kLds, c->stream, d_lf, c->side.sai.as<unsigned>(), nne, C, W, H, flo, fhi, s, dh, ds, dc, dw, dk);
    else hipLaunchKernelGGL((k_clip_stats<false>), dim3(wgs, C), dim3(kThreads), kLds, c->stream, d_lf, c->side.sai.as<unsigned>(), nne, C, W, H, flo, fhi, s, dh, ds, dc, dw, dk);
    HIPCK(c, hipGetLastError());
    std::vector<unsigned long long> host(words);
    HIPCK(c, hipMemcpyAsync(host.data(), d, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    out.hist.assign(host.begin(), host.begin() + nh);
    out.sum.assign(host.begin() + nh, host.begin() + nh + ns);
    out.cens.assign(host.begin() + nh + ns, host.begin() + nh + 2 * ns);
    out.whole.assign(host.begin() + nh + 2 * ns, host.begin() + nh + 2 * ns + C);
    out.blocks = total * C;
    out.skipped = host[words - 1];
    return 0;
}

/* include/lfbm5d.h, lfbm5d_clip_fit; 1: the pooled fit fails */
int fit(const unsigned long long* hist, const unsigned long long* cens, const unsigned long long* whole, unsigned C, double lo, double hi,
        lfbm5d_clip_estimate* out) {
    const double s = (double)rescale(lo, hi);
    const size_t nh = (size_t)kLevels * kKeys;
    std::vector<unsigned long long> ph(nh, 0ull), pc(kLevels, 0ull);
    unsigned long long pw = 0, total = 0, censored = 0;
    for (unsigned ch = 0; ch < C; ch++) {
        for (size_t i = 0; i < nh; i++) { ph[i] += hist[ch * nh + i]; total += hist[ch * nh + i]; }
        for (int l = 0; l < kLevels; l++) { pc[l] += cens[ch * kLevels + l]; censored += cens[ch * kLevels + l]; }
        pw += whole[ch];
    }
    std::memset(out, 0, sizeof(*out));
    Fit f;
    if (!fit_one(ph.data(), pc.data(), pw, s, f)) return 1;
    out->sigma = f.sigma; out->f_max = f.f_max; out->levels = f.levels;
    out->heavily_clipped = f.f_max > kHeavy;
    out->censored = (double)censored / (double)total;
    out->quantised = pw == total;
    for (unsigned ch = 0; ch < C; ch++)
        out->sigma_channel[ch] = fit_one(hist + ch * nh, cens + ch * kLevels, whole[ch], s, f) ? f.sigma : std::nan("");
    return 0;
}

int estimate(lfbm5d_ctx* c, const std::string& who, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
             double lo, double hi, lfbm5d_clip_estimate* out) {
    if (!out) return fail(c, who + "NULL pointer for a required buffer");
    Counts n;
    if (histogram(c, who, d_lf, h_mask, asize, W, H, C, lo, hi, n)) return 1;
    if (fit(n.hist.data(), n.cens.data(), n.whole.data(), C, lo, hi, out))
        return fail(c, who + "fewer than 4 intensity levels of the light field hold the 256 blocks the fit needs (or their quantiles fell into an end bin)");
    out->blocks = n.blocks;
    out->skipped = n.skipped;
    return 0;
}

/* launch only: the caller synchronises; the SAI list is the context's */
int declip_launch(lfbm5d_ctx* c, const std::string& who, const Map& m, const float* d_in, float* d_out, unsigned W, unsigned H, unsigned C) {
    const unsigned nne = (unsigned)c->side.sai_host.size();
    const unsigned long long plane = (unsigned long long)W * H;
    if (!plane || plane > 0xffffffffull - 1024 || (unsigned long long)nne * C > 65535) return fail(c, who + "light field too large (or empty)");
    const bool vec = plane % 4 == 0 && reinterpret_cast<uintptr_t>(d_in) % 16 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
    const dim3 grid((unsigned)((plane + 1023) / 1024), nne * C);
    if (vec) hipLaunchKernelGGL((k_declip<true>), grid, dim3(256), 0, c->stream, d_in, d_out, c->side.sai.as<unsigned>(), C, (unsigned)plane, m);
    else hipLaunchKernelGGL((k_declip<false>), grid, dim3(256), 0, c->stream, d_in, d_out, c->side.sai.as<unsigned>(), C, (unsigned)plane, m);
    HIPCK(c, hipGetLastError());
    return 0;
}

int declip(lfbm5d_ctx* c, const std::string& who, double sigma, double lo, double hi, const float* d_in, const unsigned* h_mask, float* d_out,
           unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!d_in || !h_mask || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    if (!good_range(lo, hi)) return fail(c, who + kBadRange);
    Map m;
    if (!make_map(lo, hi, sigma, m)) return fail(c, who + kBadSigma);
    if (sai_list(c, who, h_mask, asize)) return 1;
    if (declip_launch(c, who, m, d_in, d_out, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int denoise_clipped(lfbm5d_ctx* c, const std::string& who, double sigma, double lo, double hi, lfbm5d_clip_estimate* est, double* sigma_used,
                    const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy, const unsigned* h_mask, float* d_basic,
                    float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H,
                    unsigned C) {
    if (!P1 || !P2 || !d_noisy || !h_mask || !d_basic || !d_denoised) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    if (!good_range(lo, hi)) return fail(c, who + kBadRange);
    if (!std::isfinite(sigma)) return fail(c, who + "sigma must be finite (zero or negative: estimate it)");
    const unsigned asize = awidth * aheight;
    if (sai_list(c, who, h_mask, asize)) return 1;
    lfbm5d_clip_estimate e;
    std::memset(&e, 0, sizeof(e));
    if (!(sigma > 0.0)) {
        if (estimate(c, who, d_noisy, h_mask, asize, W, H, C, lo, hi, &e)) return 1;
        sigma = e.sigma;
    }
    Map m;
    if (!make_map(lo, hi, sigma, m)) return fail(c, who + kBadSigma);
    if (est) *est = e;
    if (sigma_used) *sigma_used = sigma;
    lfbm5d_params Q1 = *P1, Q2 = *P2;
    Q1.sigma = Q2.sigma = (float)sigma;
    if (lfbm5d_denoise_device(c, &Q1, &Q2, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2, W, H, C)) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    if (declip_launch(c, who, m, d_basic, d_basic, W, H, C) || declip_launch(c, who, m, d_denoised, d_denoised, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

int lfbm5d_clip_fit(const unsigned long long* hist, const unsigned long long* sum, const unsigned long long* cens, const unsigned long long* whole,
                    unsigned C, double lo, double hi, lfbm5d_clip_estimate* out) {
    (void)sum;   /* the level means: part of the statistics, not of a fit without a slope */
    if (!hist || !cens || !whole || !out || (C != 1 && C != 3) || !good_range(lo, hi)) return 1;
    return fit(hist, cens, whole, C, lo, hi, out);
}

int lfbm5d_clip_histogram_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                                 double lo, double hi, unsigned long long* h_hist, unsigned long long* h_sum, unsigned long long* h_cens,
                                 unsigned long long* h_whole, unsigned long long* blocks, unsigned long long* skipped) {
    if (!c) return 1;
    const std::string who = "lfbm5d_clip_histogram_device: ";
    if (!h_hist || !h_sum || !h_cens || !h_whole) return fail(c, who + "NULL pointer for a required buffer");
    Counts n;
    if (histogram(c, who, d_lf, h_mask, asize, W, H, C, lo, hi, n)) return 1;
    std::memcpy(h_hist, n.hist.data(), n.hist.size() * sizeof(unsigned long long));
    std::memcpy(h_sum, n.sum.data(), n.sum.size() * sizeof(unsigned long long));
    std::memcpy(h_cens, n.cens.data(), n.cens.size() * sizeof(unsigned long long));
    std::memcpy(h_whole, n.whole.data(), n.whole.size() * sizeof(unsigned long long));
    if (blocks) *blocks = n.blocks;
    if (skipped) *skipped = n.skipped;
    return 0;
}

int lfbm5d_noise_level_clipped_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                                      double lo, double hi, lfbm5d_clip_estimate* out) {
    if (!c) return 1;
    return estimate(c, "lfbm5d_noise_level_clipped_device: ", d_lf, h_mask, asize, W, H, C, lo, hi, out);
}

int lfbm5d_noise_level_clipped_host_sai(lfbm5d_ctx* c, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                        unsigned C, double lo, double hi, lfbm5d_clip_estimate* out) {
    if (!c) return 1;
    const std::string who = "lfbm5d_noise_level_clipped_host_sai: ";
    if (check_chnls(c, who, C)) return 1;
    if (stage(c, who, h_lf, h_mask, asize, (size_t)C * W * H, c->h2d_noisy)) return 1;
    return estimate(c, who, c->h2d_noisy.as<float>(), h_mask, asize, W, H, C, lo, hi, out);
}

int lfbm5d_declip_device(lfbm5d_ctx* c, double sigma, double lo, double hi, const float* d_in, const unsigned* h_mask, float* d_out, unsigned asize,
                         unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return declip(c, "lfbm5d_declip_device: ", sigma, lo, hi, d_in, h_mask, d_out, asize, W, H, C);
}

int lfbm5d_declip_host_sai(lfbm5d_ctx* c, double sigma, double lo, double hi, const float* const* h_in, const unsigned* h_mask, float* const* h_out,
                           unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    const std::string who = "lfbm5d_declip_host_sai: ";
    if (!h_out || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const size_t img = (size_t)C * W * H;
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_out, asize, nonempty)) return 1;
    if (stage(c, who, h_in, h_mask, asize, img, c->h2d_noisy)) return 1;
    float* const d = c->h2d_noisy.as<float>();
    if (declip(c, who, sigma, lo, hi, d, h_mask, d, asize, W, H, C)) return 1;
    if (download_planes(c, h_out, d, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int lfbm5d_denoise_clipped_device(lfbm5d_ctx* c, double sigma, double lo, double hi, lfbm5d_clip_estimate* est, double* sigma_used,
                                  const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy, const unsigned* h_mask, float* d_basic,
                                  float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W,
                                  unsigned H, unsigned C) {
    if (!c) return 1;
    return denoise_clipped(c, "lfbm5d_denoise_clipped_device: ", sigma, lo, hi, est, sigma_used, P1, P2, d_noisy, h_mask, d_basic, d_denoised,
                           ang_major, awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_denoise_clipped_host_sai(lfbm5d_ctx* c, double sigma, double lo, double hi, lfbm5d_clip_estimate* est, double* sigma_used,
                                    const lfbm5d_params* P1, const lfbm5d_params* P2, const float* const* h_noisy, const unsigned* h_mask,
                                    float* const* h_basic, float* const* h_denoised, unsigned ang_major, unsigned awidth, unsigned aheight,
                                    unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    const std::string who = "lfbm5d_denoise_clipped_host_sai: ";
    if (check_chnls(c, who, C)) return 1;
    return host_sai_job(c, who, h_noisy, h_mask, h_basic, h_denoised, awidth * aheight, (size_t)C * W * H, [&](float* dn, float* db, float* dd) {
        return denoise_clipped(c, who, sigma, lo, hi, est, sigma_used, P1, P2, dn, h_mask, db, dd, ang_major, awidth, aheight, an1, an2, W, H, C);
    });
}

} /* extern "C" */
