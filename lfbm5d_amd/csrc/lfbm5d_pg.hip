/*
 * lfbm5d_pg.hip -- signal-dependent (Poisson-Gaussian) noise, var(z | y) = a y + b (lfbm5d_pg_*, lfbm5d_denoise_pg_*, include/lfbm5d.h):
 * the model's estimate from the noisy light field, the generalised Anscombe transform that turns such noise into white Gaussian noise of
 * a known sigma, its exact unbiased inverse (Makitalo & Foi, IEEE TIP 2013, closed form), and the two-step job between the two.  Not in
 * the reference, which knows one sigma.
 *
 * Kernels:
 *   k_pg_stats     the statistics of every 2 x 2 block of every non-empty SAI and channel plane: mean m and the diagonal difference d
 *                  (float32, additions and exact scalings only), binned by level of m (64) and by |d| (322 bins: 16 per octave, straight
 *                  from the exponent and the top four mantissa bits).  Grid (workgroups, channel); a workgroup of 1024 threads keeps the
 *                  channel's whole histogram in LDS (64 x 322 32-bit counters = 82 KB: one workgroup per CU) and walks over the channel's
 *                  blocks in chunks of kPgUnroll x 1024 with all of a chunk's loads issued before the first is used; the two rows of a
 *                  block come as one 8-byte load each when the rows are 8-byte aligned.  LDS integer atomics, then one 64-bit integer
 *                  global atomic per non-zero counter.  Everything is an integer count: the result does not depend on any order.
 *   k_pg_forward   t = s 2z / (sqrt(a z + c) + sqrt(c))   (c = 3/8 a^2 + b; the form of s (f(z) - f(0)) that stays exact as a -> 0)
 *   k_pg_inverse   the closed-form exact unbiased inverse; both evaluate in double and round once, one thread per value, grid (chunks,
 *                  SAI x channel); planes of empty SAIs are not touched; in place is fine (pointwise).
 * The fit of (a, b) to a histogram (quantile of |d| per level -> variance per level -> weighted line) runs on the host in double.
 */
#include "lfbm5d_side.h"

using namespace lfbm5d_host;

namespace {

constexpr int kLevels = 64;
constexpr int kEMin = -12, kEMax = 8;
constexpr int kKeys = (kEMax - kEMin) * 16 + 2;      /* 322 */
constexpr int kKeyBase = (kEMin + 127) << 4;         /* 1840: bits >> 19 of 2^E_MIN */
constexpr int kPgThreads = 1024;
constexpr int kPgUnroll = 4;
constexpr size_t kPgLds = (size_t)kLevels * kKeys * sizeof(unsigned) + kLevels * sizeof(unsigned long long);
constexpr double kQuartile = 0.31863936396437514;    /* the 0.25 quantile of |N(0,1)| */
constexpr double kGMax = 0.816496580927726;          /* sqrt(2/3): beyond it the inverse's argument lies below the transform's range */
constexpr double kK1 = 0.30618621784789724, kK3 = 0.7654655446197431;

/* grid (workgroups, C), 1024 threads, kPgLds bytes of dynamic LDS.  hist [C][64][322], sum [C][64], skipped [1]: accumulated into. */
template <bool VEC>
__global__ __launch_bounds__(kPgThreads) void k_pg_stats(const float* __restrict__ lf, const unsigned* __restrict__ sai, unsigned nne, unsigned C,
                                                         unsigned W, unsigned H, unsigned long long* __restrict__ hist,
                                                         unsigned long long* __restrict__ sum, unsigned long long* __restrict__ skipped) {
    extern __shared__ __attribute__((aligned(16))) unsigned pg_lds[];
    unsigned* h = pg_lds;
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(pg_lds + kLevels * kKeys);
    const unsigned tid = threadIdx.x, c = blockIdx.y;
    for (unsigned i = tid; i < kLevels * kKeys; i += kPgThreads) h[i] = 0u;
    if (tid < kLevels) sm[tid] = 0ull;
    __syncthreads();
    const unsigned WP = W / 2, HP = H / 2;
    const unsigned long long per_sai = (unsigned long long)WP * HP, total = per_sai * nne;
    const unsigned long long chunk = (unsigned long long)kPgThreads * kPgUnroll;
    unsigned skip = 0;
    for (unsigned long long q0 = (unsigned long long)blockIdx.x * chunk; q0 < total; q0 += (unsigned long long)gridDim.x * chunk) {
        float p[kPgUnroll][4];
        bool on[kPgUnroll];
#pragma unroll
        for (int u = 0; u < kPgUnroll; u++) {
            const unsigned long long q = q0 + (unsigned long long)u * kPgThreads + tid;
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
        for (int u = 0; u < kPgUnroll; u++) {
            if (!on[u]) continue;
            const float m = ((p[u][0] + p[u][1]) + (p[u][2] + p[u][3])) * 0.25f;
            const float d = ((p[u][0] - p[u][1]) - (p[u][2] - p[u][3])) * 0.5f;
            if (!(isfinite(m) && isfinite(d))) { skip++; continue; }
            const float mc = fminf(fmaxf(m, 0.0f), 255.0f);
            const int lev = min(kLevels - 1, (int)(mc * (float)(64.0 / 255.0)));
            const int key = min(max((int)(__float_as_uint(fabsf(d)) >> 19) - kKeyBase + 1, 0), kKeys - 1);
            atomicAdd(&h[lev * kKeys + key], 1u);
            atomicAdd(&sm[lev], (unsigned long long)rintf(mc * 256.0f));
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < kLevels * kKeys; i += kPgThreads)
        if (h[i]) atomicAdd(&hist[(size_t)c * kLevels * kKeys + i], (unsigned long long)h[i]);
    if (tid < kLevels && sm[tid]) atomicAdd(&sum[c * kLevels + tid], sm[tid]);
    if (skip) atomicAdd(skipped, (unsigned long long)skip);
}

/* a model as the transform kernels use it: per stored channel a, c = 3/8 a^2 + b, sqrt(c); the common scale s */
struct PgCoef { double a[3], c[3], sc[3], s; };

/* grid (chunks, nne * C), 256 threads, one value per thread */
template <bool INVERSE>
__global__ __launch_bounds__(256) void k_pg_transform(const float* __restrict__ in, float* __restrict__ out, const unsigned* __restrict__ sai,
                                                      unsigned C, unsigned plane, PgCoef m) {
    const unsigned x = blockIdx.x * 256 + threadIdx.x, ac = blockIdx.y;
    if (x >= plane) return;
    const unsigned ch = ac % C;
    const size_t at = ((size_t)sai[ac / C] * C + ch) * (size_t)plane + x;
    const double a = m.a[ch], c = m.c[ch], sc = m.sc[ch];
    if (!INVERSE) {
        double z = (double)in[at];
        double w = a * z + c;
        if (w < 0.0) { w = 0.0; z = -c / a; }
        out[at] = (float)((m.s * (2.0 * z)) / (sqrt(w) + sc));
    } else {
        const double u = (double)in[at] / m.s;
        const double q = a * u + 2.0 * sc;
        double y = 0.0;
        if (q > 0.0) {
            const double g = a / q;
            if (!(g > kGMax)) y = a * u * u / 4.0 + u * sc + a / 4.0 + a * (kK1 * g - 1.375 * (g * g) + kK3 * (g * g * g));
        }
        out[at] = (float)fmax(y, 0.0);
    }
}

/* lower edge of key k (1 <= k <= 321) as a double: the float whose bits are (k - 1 + 1840) << 19; key 0 starts at 0 */
double key_edge(int k) {
    if (k <= 0) return 0.0;
    const unsigned bits = (unsigned)(k - 1 + kKeyBase) << 19;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return (double)f;
}

/* include/lfbm5d.h, lfbm5d_pg_fit */
int fit(const unsigned long long* hist, const unsigned long long* sum, double* a_out, double* b_out) {
    double Sw = 0.0, Swx = 0.0, Swv = 0.0, Swxx = 0.0, Swxv = 0.0;
    unsigned valid = 0;
    for (int l = 0; l < kLevels; l++) {
        const unsigned long long* h = hist + (size_t)l * kKeys;
        unsigned long long n = 0;
        for (int k = 0; k < kKeys; k++) n += h[k];
        if (n < 256) continue;
        const double T = 0.25 * (double)n;
        unsigned long long cum = 0, before = 0;
        int ks = 0;
        for (; ks < kKeys; ks++) {
            before = cum;
            cum += h[ks];
            if ((double)cum >= T) break;
        }
        if (ks <= 0 || ks >= kKeys - 1) continue;
        const double e0 = key_edge(ks), e1 = key_edge(ks + 1);
        const double Qv = e0 + (e1 - e0) * (T - (double)before) / (double)h[ks];
        const double r = Qv / kQuartile, v = r * r;
        const double x = (double)sum[l] / (256.0 * (double)n);
        const double w = (double)n / (v * v);
        Sw += w; Swx += w * x; Swv += w * v; Swxx += w * x * x; Swxv += w * x * v;
        valid++;
    }
    if (!valid) return 1;
    const double det = Sw * Swxx - Swx * Swx;
    double a, b;
    if (valid < 2 || !(det > 1e-12 * Sw * Swxx)) { a = 0.0; b = Swv / Sw; }
    else {
        a = (Sw * Swxv - Swx * Swv) / det;
        b = (Swxx * Swv - Swx * Swxv) / det;
        if (a < 0.0) { a = 0.0; b = Swv / Sw; }
        else if (b < 0.0) { b = 0.0; a = Swxv / Swxx; }
    }
    *a_out = a; *b_out = b;
    return 0;
}

/* a model's coefficients; false on a rejected model (a < 0, c <= 0, anything not finite) */
bool coefficients(const lfbm5d_pg_model* m, unsigned C, PgCoef& k) {
    if (!m || (C != 1 && C != 3)) return false;
    double s = 0.0;
    for (unsigned ch = 0; ch < 3; ch++) {
        const unsigned src = ch < C ? ch : 0;
        const double a = m->a[src], b = m->b[src];
        if (!std::isfinite(a) || !std::isfinite(b) || !(a >= 0.0)) return false;
        const double c = 0.375 * a * a + b;
        if (!(c > 0.0)) return false;
        k.a[ch] = a; k.c[ch] = c; k.sc[ch] = std::sqrt(c);
        if (ch < C) s += (std::sqrt(255.0 * a + c) + k.sc[ch]) / 2.0;
    }
    k.s = s / (double)C;
    return std::isfinite(k.s) && k.s > 0.0;
}

constexpr const char* kOneGpu = "the Poisson-Gaussian routines run on one GPU (this context has a communicator or a shard)";

/* hist [C][64][322], sum [C][64] (host, unsigned 64-bit) of the light field in HBM */
int histogram(lfbm5d_ctx* c, const std::string& who, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
              unsigned long long* h_hist, unsigned long long* h_sum, unsigned long long* blocks, unsigned long long* skipped) {
    if (!d_lf || !h_mask || !h_hist || !h_sum) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    const unsigned nne = (unsigned)c->side.sai_host.size();
    const size_t nh = (size_t)C * kLevels * kKeys, ns = (size_t)C * kLevels, words = nh + ns + 1;
    HIPCK(c, c->pg.stats.reserve(words * sizeof(unsigned long long)));
    unsigned long long* d = c->pg.stats.as<unsigned long long>();
    HIPCK(c, hipMemsetAsync(d, 0, words * sizeof(unsigned long long), c->stream));
    const unsigned long long total = (unsigned long long)(W / 2) * (H / 2) * nne, chunk = (unsigned long long)kPgThreads * kPgUnroll;
    int n_cu = 0;
    HIPCK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    const unsigned cus = (unsigned)std::max(1, n_cu);
    const unsigned wgs = (unsigned)std::min<unsigned long long>((total + chunk - 1) / chunk, std::max(1u, cus / C));
    const bool vec = W % 2 == 0 && reinterpret_cast<uintptr_t>(d_lf) % 8 == 0;
    const void* fn = vec ? reinterpret_cast<const void*>(&k_pg_stats<true>) : reinterpret_cast<const void*>(&k_pg_stats<false>);
    HIPCK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPgLds));   /* per device: cheap, so every call */
    if (vec) hipLaunchKernelGGL((k_pg_stats<true>), dim3(wgs, C), dim3(kPgThreads), kPgLds, c->stream, d_lf, c->side.sai.as<unsigned>(), nne, C, W, H, d, d + nh, d + nh + ns);
    else hipLaunchKernelGGL((k_pg_stats<false>), dim3(wgs, C), dim3(kPgThreads), kPgLds, c->stream, d_lf, c->side.sai.as<unsigned>(), nne, C, W, H, d, d + nh, d + nh + ns);
    HIPCK(c, hipGetLastError());
    std::vector<unsigned long long> host(words);
    HIPCK(c, hipMemcpyAsync(host.data(), d, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_hist, host.data(), nh * sizeof(unsigned long long));
    std::memcpy(h_sum, host.data() + nh, ns * sizeof(unsigned long long));
    if (blocks) *blocks = total * C;
    if (skipped) *skipped = host[nh + ns];
    return 0;
}

int estimate(lfbm5d_ctx* c, const std::string& who, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
             lfbm5d_pg_estimate* out, unsigned long long* h_hist, unsigned long long* h_sum) {
    if (!out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    std::vector<unsigned long long> hist((size_t)C * kLevels * kKeys), sum((size_t)C * kLevels);
    unsigned long long blocks = 0, skipped = 0;
    if (histogram(c, who, d_lf, h_mask, asize, W, H, C, hist.data(), sum.data(), &blocks, &skipped)) return 1;
    std::vector<unsigned long long> ph((size_t)kLevels * kKeys, 0ull), ps(kLevels, 0ull);
    for (unsigned ch = 0; ch < C; ch++) {
        for (size_t i = 0; i < ph.size(); i++) ph[i] += hist[ch * ph.size() + i];
        for (int l = 0; l < kLevels; l++) ps[l] += sum[ch * kLevels + l];
    }
    std::memset(out, 0, sizeof(*out));
    if (fit(ph.data(), ps.data(), &out->a, &out->b))
        return fail(c, who + "no intensity level of the light field holds the 256 blocks the fit needs (or every quantile fell into an end bin)");
    for (unsigned ch = 0; ch < C; ch++)
        if (fit(&hist[ch * ph.size()], &sum[ch * kLevels], &out->a_channel[ch], &out->b_channel[ch]))
            out->a_channel[ch] = out->b_channel[ch] = std::nan("");
    out->blocks = blocks;
    out->skipped = skipped;
    if (h_hist) std::memcpy(h_hist, hist.data(), hist.size() * sizeof(unsigned long long));
    if (h_sum) std::memcpy(h_sum, sum.data(), sum.size() * sizeof(unsigned long long));
    return 0;
}

/* launches only: the caller synchronises.  nne = 0: build the SAI list from the mask first. */
template <bool INVERSE>
int transform(lfbm5d_ctx* c, const std::string& who, const PgCoef& k, const float* d_in, float* d_out, unsigned nne, unsigned W, unsigned H, unsigned C) {
    const unsigned long long plane = (unsigned long long)W * H;
    if (!plane || plane > 0xffffffffull - 256 || (plane + 255) / 256 > 0x7fffffffull || (unsigned long long)nne * C > 65535)
        return fail(c, who + "light field too large (or empty)");
    hipLaunchKernelGGL((k_pg_transform<INVERSE>), dim3((unsigned)((plane + 255) / 256), nne * C), dim3(256), 0, c->stream, d_in, d_out,
                       c->side.sai.as<unsigned>(), C, (unsigned)plane, k);
    HIPCK(c, hipGetLastError());
    return 0;
}

template <bool INVERSE>
int transform_entry(lfbm5d_ctx* c, const char* name, const lfbm5d_pg_model* model, const float* d_in, const unsigned* h_mask, float* d_out,
                    unsigned asize, unsigned W, unsigned H, unsigned C) {
    const std::string who = std::string(name) + ": ";
    if (!model || !d_in || !h_mask || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    PgCoef k;
    if (!coefficients(model, C, k)) return fail(c, who + "bad model: every channel needs a >= 0 and 3/8 a^2 + b > 0, finite");
    if (check_one_gpu(c, who, kOneGpu) || sai_list(c, who, h_mask, asize)) return 1;
    if (transform<INVERSE>(c, who, k, d_in, d_out, (unsigned)c->side.sai_host.size(), W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int denoise_pg(lfbm5d_ctx* c, const std::string& who, const lfbm5d_pg_model* model, lfbm5d_pg_model* used, const lfbm5d_params* P1,
               const lfbm5d_params* P2, const float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major,
               unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!P1 || !P2 || !d_noisy || !h_mask || !d_basic || !d_denoised) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    const unsigned asize = awidth * aheight;
    lfbm5d_pg_model m;
    if (model) m = *model;
    else {   /* the pooled model of the noisy light field, for every channel */
        lfbm5d_pg_estimate e;
        if (estimate(c, who, d_noisy, h_mask, asize, W, H, C, &e, nullptr, nullptr)) return 1;
        for (int ch = 0; ch < 3; ch++) { m.a[ch] = e.a; m.b[ch] = e.b; }
    }
    PgCoef k;
    if (!coefficients(&m, C, k)) return fail(c, who + "bad model: every channel needs a >= 0 and 3/8 a^2 + b > 0, finite");
    if (used) *used = m;
    if (sai_list(c, who, h_mask, asize)) return 1;
    const unsigned nne = (unsigned)c->side.sai_host.size();
    float* t = nullptr;                                                   /* the stabilised light field: the job's input */
    if (scratch_lf(c, asize, nne, (size_t)C * W * H, t)) return 1;
    if (transform<false>(c, who, k, d_noisy, t, nne, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));                            /* the job's contract: its buffers are ready on entry */
    lfbm5d_params Q1 = *P1, Q2 = *P2;
    Q1.sigma = Q2.sigma = (float)k.s;
    if (lfbm5d_denoise_device(c, &Q1, &Q2, t, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2, W, H, C)) return 1;
    if (transform<true>(c, who, k, d_basic, d_basic, nne, W, H, C)) return 1;
    if (transform<true>(c, who, k, d_denoised, d_denoised, nne, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

int lfbm5d_pg_fit(const unsigned long long* hist, const unsigned long long* sum, double* a, double* b) {
    if (!hist || !sum || !a || !b) return 1;
    return fit(hist, sum, a, b);
}

int lfbm5d_pg_scale(const lfbm5d_pg_model* model, unsigned C, double* s) {
    PgCoef k;
    if (!s || !coefficients(model, C, k)) return 1;
    *s = k.s;
    return 0;
}

int lfbm5d_pg_histogram_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                               unsigned long long* h_hist, unsigned long long* h_sum, unsigned long long* blocks, unsigned long long* skipped) {
    if (!c) return 1;
    return histogram(c, "lfbm5d_pg_histogram_device: ", d_lf, h_mask, asize, W, H, C, h_hist, h_sum, blocks, skipped);
}

int lfbm5d_pg_estimate_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                              lfbm5d_pg_estimate* out, unsigned long long* h_hist, unsigned long long* h_sum) {
    if (!c) return 1;
    return estimate(c, "lfbm5d_pg_estimate_device: ", d_lf, h_mask, asize, W, H, C, out, h_hist, h_sum);
}

int lfbm5d_pg_estimate_host_sai(lfbm5d_ctx* c, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                                lfbm5d_pg_estimate* out, unsigned long long* h_hist, unsigned long long* h_sum) {
    if (!c) return 1;
    const std::string who = "lfbm5d_pg_estimate_host_sai: ";
    if (check_chnls(c, who, C)) return 1;
    if (stage(c, who, h_lf, h_mask, asize, (size_t)C * W * H, c->h2d_noisy)) return 1;
    return estimate(c, who, c->h2d_noisy.as<float>(), h_mask, asize, W, H, C, out, h_hist, h_sum);
}

int lfbm5d_pg_forward_device(lfbm5d_ctx* c, const lfbm5d_pg_model* model, const float* d_in, const unsigned* h_mask, float* d_out, unsigned asize,
                             unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return transform_entry<false>(c, "lfbm5d_pg_forward_device", model, d_in, h_mask, d_out, asize, W, H, C);
}

int lfbm5d_pg_inverse_device(lfbm5d_ctx* c, const lfbm5d_pg_model* model, const float* d_in, const unsigned* h_mask, float* d_out, unsigned asize,
                             unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return transform_entry<true>(c, "lfbm5d_pg_inverse_device", model, d_in, h_mask, d_out, asize, W, H, C);
}

int lfbm5d_denoise_pg_device(lfbm5d_ctx* c, const lfbm5d_pg_model* model, lfbm5d_pg_model* used, const lfbm5d_params* P1, const lfbm5d_params* P2,
                             const float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth,
                             unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return denoise_pg(c, "lfbm5d_denoise_pg_device: ", model, used, P1, P2, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2,
                      W, H, C);
}

int lfbm5d_denoise_pg_host_sai(lfbm5d_ctx* c, const lfbm5d_pg_model* model, lfbm5d_pg_model* used, const lfbm5d_params* P1, const lfbm5d_params* P2,
                               const float* const* h_noisy, const unsigned* h_mask, float* const* h_basic, float* const* h_denoised,
                               unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    const std::string who = "lfbm5d_denoise_pg_host_sai: ";
    if (check_chnls(c, who, C)) return 1;
    return host_sai_job(c, who, h_noisy, h_mask, h_basic, h_denoised, awidth * aheight, (size_t)C * W * H, [&](float* dn, float* db, float* dd) {
        return denoise_pg(c, who, model, used, P1, P2, dn, h_mask, db, dd, ang_major, awidth, aheight, an1, an2, W, H, C);
    });
}

} /* extern "C" */
