/*
 * lfbm5d_pgclip.hip -- Poisson-Gaussian noise on data clipped to a known range lo..hi (8-bit files): the censored fit of the model on the
 * clipped stage's statistics, the variance stabiliser of a clipped heteroskedastic observation and its exact unbiased inverse as tables,
 * and the two-step job between them (lfbm5d_pgclip_*, lfbm5d_denoise_pgclip_*, include/lfbm5d_pgclip.h).  Not in the reference.
 *
 * Kernel:
 *   k_curve_map    out = T[i] + r (T[i + 1] - T[i]) per value, the look-up of include/lfbm5d_pgclip.h, forward (r free: the end segments
 *                  extend the map) or inverse (r in 0..1: the output stays inside the range).  The table (4097 floats, 16 KB) is
 *                  copied into LDS once per workgroup; the grid is persistent (kWgPerCu workgroups of 256 threads per CU: all resident
 *                  at once at 16 KB of LDS each) and strides over the values of the non-empty SAIs as one index space, so a table load
 *                  is shared by every plane a workgroup touches.  Four values per thread: one 16-byte load and store when a plane is a
 *                  multiple of 4 values and both buffers are 16-byte aligned (a quad then never leaves its SAI), value by value
 *                  otherwise.  The two table reads of a value are neighbouring words (one ds_read2_b32); neighbouring pixels land on
 *                  the same or nearby knots, which broadcast or fall into different banks.  Non-finite values pass through; planes of
 *                  empty SAIs are not touched; in place is fine (pointwise).  No atomics; no value decides how long a thread runs.
 *                  The file is compiled without FMA contraction: the interpolation rounds as the numpy model's does.
 * The fit and the curves run on the host in double (lfbm5d_pgclip_values.h).
 */
#include "lfbm5d_side.h"
#include "lfbm5d_pgclip_values.h"

#include <memory>

using namespace lfbm5d_host;
using namespace lfbm5d_pgclip;

namespace {

constexpr int kThreads = 256;
constexpr unsigned kWgPerCu = 8;

template <bool INVERSE>
__device__ __forceinline__ float map_one(const float* T, float x0, float inv_dx, float x) {
    return lfbm5d_side::finite_bits(x) ? curve_value<INVERSE>(T, x0, inv_dx, x) : x;
}

/* grid (workgroups), 256 threads.  img = C * plane values per SAI, total = nne * img, quads = ceil(total / 4); a workgroup's stride of
 * gridDim.x * 1024 values is step_k SAIs and step_r values (host: no division in the loop). */
template <bool INVERSE, bool VEC>
__global__ __launch_bounds__(kThreads) void k_curve_map(const float* in, float* out, const unsigned* __restrict__ sai, unsigned long long img,
                                                        unsigned long long total, unsigned long long quads, unsigned long long step_k,
                                                        unsigned long long step_r, const float* __restrict__ table, float x0, float inv_dx) {
    __shared__ float T[kKnots];
    for (unsigned i = threadIdx.x; i < (unsigned)kKnots; i += kThreads) T[i] = table[i];
    __syncthreads();
    unsigned long long q = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    unsigned long long k = (q * 4) / img, r = q * 4 - k * img;
    for (; q < quads; q += (unsigned long long)gridDim.x * kThreads) {
        if (VEC) {
            const size_t at = (size_t)sai[k] * img + r;
            float4 v = *reinterpret_cast<const float4*>(in + at);
            v.x = map_one<INVERSE>(T, x0, inv_dx, v.x); v.y = map_one<INVERSE>(T, x0, inv_dx, v.y);
            v.z = map_one<INVERSE>(T, x0, inv_dx, v.z); v.w = map_one<INVERSE>(T, x0, inv_dx, v.w);
            *reinterpret_cast<float4*>(out + at) = v;
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; e++) {
                if (q * 4 + e >= total) break;
                unsigned long long ke = k, re = r + e;
                if (re >= img) { re -= img; ke++; }          /* img >= 4: one wrap at most */
                const size_t at = (size_t)sai[ke] * img + re;
                out[at] = map_one<INVERSE>(T, x0, inv_dx, in[at]);
            }
        }
        k += step_k; r += step_r;
        if (r >= img) { r -= img; k++; }
    }
}

constexpr const char* kOneGpu = "the clipped Poisson-Gaussian routines run on one GPU (this context has a communicator or a shard)";
constexpr const char* kFewLevels =
    "fewer than 4 intensity levels of the light field hold the 256 blocks the fit needs (or their quantiles fell into an end bin)";

thread_local std::string t_curves_error;

bool good_range(double lo, double hi) {
    return std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo) && (float)lo < (float)hi &&
           std::isfinite(lfbm5d_clip::rescale(lo, hi));
}

/* include/lfbm5d_pgclip.h, lfbm5d_pgclip_fit; 1: the pooled fit fails */
int fit(const unsigned long long* hist, const unsigned long long* sum, const unsigned long long* cens, const unsigned long long* whole, unsigned C,
        double lo, double hi, lfbm5d_pgclip_estimate* out) {
    using lfbm5d_clip::kLevels; using lfbm5d_clip::kKeys;
    const double s = (double)lfbm5d_clip::rescale(lo, hi);
    const size_t nh = (size_t)kLevels * kKeys;
    std::vector<unsigned long long> ph(nh, 0ull), ps(kLevels, 0ull), pc(kLevels, 0ull);
    unsigned long long pw = 0, total = 0, censored = 0;
    for (unsigned ch = 0; ch < C; ch++) {
        for (size_t i = 0; i < nh; i++) { ph[i] += hist[ch * nh + i]; total += hist[ch * nh + i]; }
        for (int l = 0; l < kLevels; l++) {
            ps[l] += sum[ch * kLevels + l];
            pc[l] += cens[ch * kLevels + l]; censored += cens[ch * kLevels + l];
        }
        pw += whole[ch];
    }
    std::memset(out, 0, sizeof(*out));
    Line f;
    if (!fit_one(ph.data(), ps.data(), pc.data(), pw, s, f)) return 1;
    out->model.a = f.a; out->model.b = f.b; out->model.lo = lo; out->model.hi = hi;
    out->f_max = f.f_max; out->levels = f.levels;
    out->heavily_clipped = f.f_max > lfbm5d_clip::kHeavy;
    out->censored = (double)censored / (double)total;
    out->quantised = pw == total;
    for (unsigned ch = 0; ch < C; ch++) {
        const bool ok = fit_one(hist + ch * nh, sum + ch * kLevels, cens + ch * kLevels, whole[ch], s, f);
        out->a_channel[ch] = ok ? f.a : std::nan("");
        out->b_channel[ch] = ok ? f.b : std::nan("");
    }
    return 0;
}

int estimate(lfbm5d_ctx* c, const std::string& who, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
             double lo, double hi, lfbm5d_pgclip_estimate* out) {
    using lfbm5d_clip::kLevels; using lfbm5d_clip::kKeys;
    if (!out || !d_lf || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_one_gpu(c, who, kOneGpu)) return 1;
    std::vector<unsigned long long> hist((size_t)C * kLevels * kKeys), sum((size_t)C * kLevels), cens((size_t)C * kLevels), whole(C);
    unsigned long long blocks = 0, skipped = 0;
    /* the clipped stage's counts as they are (its message, on a failure, is the context's) */
    if (lfbm5d_clip_histogram_device(c, d_lf, h_mask, asize, W, H, C, lo, hi, hist.data(), sum.data(), cens.data(), whole.data(), &blocks, &skipped))
        return 1;
    if (fit(hist.data(), sum.data(), cens.data(), whole.data(), C, lo, hi, out)) return fail(c, who + kFewLevels);
    out->blocks = blocks;
    out->skipped = skipped;
    return 0;
}

/* the public curves of a model; the message of a refusal goes to `why` */
int build_curves(const lfbm5d_pgclip_model* m, struct lfbm5d_pgclip_curves* out, std::string& why) {
    if (!m || !out) { why = "NULL pointer"; return 1; }
    Curves cv;
    const int rc = make_curves(m->a, m->b, m->lo, m->hi, true, cv);
    if (rc == 1) why = "bad model: a >= 0, b >= 0, a + b > 0 and lo < hi, all finite";
    else if (rc == 2)
        why = "the model lies outside the accepted domain a^2 <= 0.5 b, a <= 5: at so few photons per grey level a Gaussian does not describe "
              "the counts near black, and nothing is clipped there; use lfbm5d_denoise_pg (denoise_pg)";
    else if (rc) why = "the curves of this model are not strictly increasing (sigma is too large for the range)";
    if (rc) return 1;
    out->model = *m;
    out->s = cv.s; out->fwd_x0 = cv.fwd_x0; out->fwd_dx = cv.fwd_dx; out->inv_x0 = cv.inv_x0; out->inv_dx = cv.inv_dx;
    for (int i = 0; i < kKnots; i++) { out->fwd[i] = (float)cv.fwd[i]; out->inv[i] = (float)cv.inv[i]; }
    if (!std::isfinite((float)(1.0 / cv.fwd_dx)) || !std::isfinite((float)(1.0 / cv.inv_dx)) || !((float)(1.0 / cv.inv_dx) > 0.0f)) {
        why = "the curves of this model cannot be tabulated in float32";
        return 1;
    }
    return 0;
}

/* both tables -> the context's device copy [2][4097]; enqueued from the caller's memory, which HIP stages before it returns */
int upload_tables(lfbm5d_ctx* c, const struct lfbm5d_pgclip_curves* cv) {
    (void)hipSetDevice(c->device);
    HIPCK(c, c->pgclip.tables.reserve(2 * (size_t)kKnots * sizeof(float)));
    float* d = c->pgclip.tables.as<float>();
    HIPCK(c, hipMemcpyAsync(d, cv->fwd, kKnots * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(d + kKnots, cv->inv, kKnots * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return 0;
}

/* launch only: the caller synchronises; the SAI list and the tables are the context's */
template <bool INVERSE>
int map_launch(lfbm5d_ctx* c, const std::string& who, const struct lfbm5d_pgclip_curves* cv, const float* d_in, float* d_out, unsigned W, unsigned H,
               unsigned C) {
    const unsigned long long nne = c->side.sai_host.size(), plane = (unsigned long long)W * H, img = plane * C, total = nne * img;
    if (plane < 4 || plane > 0xffffffffull || total > (1ull << 60)) return fail(c, who + "light field too large (or empty)");
    const unsigned long long quads = (total + 3) / 4;
    int n_cu = 0;
    HIPCK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    const unsigned long long wgs = std::min<unsigned long long>((quads + kThreads - 1) / kThreads, (unsigned long long)std::max(1, n_cu) * kWgPerCu);
    const unsigned long long stride = wgs * kThreads * 4, step_k = stride / img, step_r = stride % img;
    const bool vec = plane % 4 == 0 && reinterpret_cast<uintptr_t>(d_in) % 16 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
    const float* table = c->pgclip.tables.as<float>() + (INVERSE ? kKnots : 0);
    const float x0 = (float)(INVERSE ? cv->inv_x0 : cv->fwd_x0), inv_dx = (float)(1.0 / (INVERSE ? cv->inv_dx : cv->fwd_dx));
    const unsigned* sai = c->side.sai.as<unsigned>();
    if (vec) hipLaunchKernelGGL((k_curve_map<INVERSE, true>), dim3((unsigned)wgs), dim3(kThreads), 0, c->stream, d_in, d_out, sai, img, total, quads, step_k, step_r, table, x0, inv_dx);
    else hipLaunchKernelGGL((k_curve_map<INVERSE, false>), dim3((unsigned)wgs), dim3(kThreads), 0, c->stream, d_in, d_out, sai, img, total, quads, step_k, step_r, table, x0, inv_dx);
    HIPCK(c, hipGetLastError());
    return 0;
}

/* the tables as a caller may hand them in: the fields the kernel reads must be what lfbm5d_pgclip_curves writes */
bool good_curves(const struct lfbm5d_pgclip_curves* cv) {
    return std::isfinite(cv->fwd_x0) && std::isfinite(cv->inv_x0) && cv->fwd_dx > 0.0 && cv->inv_dx > 0.0 &&
           std::isfinite((float)(1.0 / cv->fwd_dx)) && std::isfinite((float)(1.0 / cv->inv_dx));
}

template <bool INVERSE>
int map_entry(lfbm5d_ctx* c, const char* name, const struct lfbm5d_pgclip_curves* cv, const float* d_in, const unsigned* h_mask, float* d_out,
              unsigned asize, unsigned W, unsigned H, unsigned C) {
    const std::string who = std::string(name) + ": ";
    if (!cv || !d_in || !h_mask || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    if (!good_curves(cv)) return fail(c, who + "bad curves: build them with lfbm5d_pgclip_curves");
    const size_t bytes = (size_t)asize * C * W * H * sizeof(float);
    if (d_in != d_out && overlap(d_in, bytes, d_out, bytes)) return fail(c, who + "the output may be the input, any other overlap is refused");
    if (sai_list(c, who, h_mask, asize)) return 1;
    if (upload_tables(c, cv) || map_launch<INVERSE>(c, who, cv, d_in, d_out, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int denoise_pgclip(lfbm5d_ctx* c, const std::string& who, const lfbm5d_pgclip_model* model, double lo, double hi, lfbm5d_pgclip_model* used,
                   double* s_used, lfbm5d_pgclip_estimate* est, const lfbm5d_params* P1, const lfbm5d_params* P2, const float* d_noisy, const unsigned* h_mask,
                   float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W,
                   unsigned H, unsigned C) {
    if (!P1 || !P2 || !d_noisy || !h_mask || !d_basic || !d_denoised) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, kOneGpu)) return 1;
    const unsigned asize = awidth * aheight;
    lfbm5d_pgclip_estimate e;
    std::memset(&e, 0, sizeof(e));
    lfbm5d_pgclip_model m;
    if (model) m = *model;
    else {
        if (!good_range(lo, hi)) return fail(c, who + "the range needs lo < hi, both finite");
        if (estimate(c, who, d_noisy, h_mask, asize, W, H, C, lo, hi, &e)) return 1;
        m = e.model;
    }
    std::unique_ptr<struct lfbm5d_pgclip_curves> cv(new struct lfbm5d_pgclip_curves);
    std::string why;
    if (build_curves(&m, cv.get(), why)) return fail(c, who + why);
    if (used) *used = m;
    if (s_used) *s_used = cv->s;
    if (est) *est = e;
    if (sai_list(c, who, h_mask, asize)) return 1;
    const unsigned nne = (unsigned)c->side.sai_host.size();
    float* t = nullptr;                                                   /* the stabilised light field: the job's input */
    if (scratch_lf(c, asize, nne, (size_t)C * W * H, t)) return 1;
    if (upload_tables(c, cv.get()) || map_launch<false>(c, who, cv.get(), d_noisy, t, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));                            /* the job's contract: its buffers are ready on entry */
    lfbm5d_params Q1 = *P1, Q2 = *P2;
    Q1.sigma = Q2.sigma = (float)cv->s;
    if (lfbm5d_denoise_device(c, &Q1, &Q2, t, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2, W, H, C)) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    if (map_launch<true>(c, who, cv.get(), d_basic, d_basic, W, H, C) || map_launch<true>(c, who, cv.get(), d_denoised, d_denoised, W, H, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

int lfbm5d_pgclip_fit(const unsigned long long* hist, const unsigned long long* sum, const unsigned long long* cens, const unsigned long long* whole,
                      unsigned C, double lo, double hi, lfbm5d_pgclip_estimate* out) {
    if (!hist || !sum || !cens || !whole || !out || (C != 1 && C != 3) || !good_range(lo, hi)) return 1;
    return fit(hist, sum, cens, whole, C, lo, hi, out);
}

int lfbm5d_pgclip_curves(const lfbm5d_pgclip_model* model, struct lfbm5d_pgclip_curves* out) {
    std::string why;
    const int rc = build_curves(model, out, why);
    if (rc) t_curves_error = "lfbm5d_pgclip_curves: " + why;
    return rc;
}

const char* lfbm5d_pgclip_curves_error(void) { return t_curves_error.c_str(); }

int lfbm5d_pgclip_estimate_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                                  double lo, double hi, lfbm5d_pgclip_estimate* out) {
    if (!c) return 1;
    return estimate(c, "lfbm5d_pgclip_estimate_device: ", d_lf, h_mask, asize, W, H, C, lo, hi, out);
}

int lfbm5d_pgclip_estimate_host_sai(lfbm5d_ctx* c, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                    unsigned C, double lo, double hi, lfbm5d_pgclip_estimate* out) {
    if (!c) return 1;
    const std::string who = "lfbm5d_pgclip_estimate_host_sai: ";
    if (check_chnls(c, who, C)) return 1;
    if (stage(c, who, h_lf, h_mask, asize, (size_t)C * W * H, c->h2d_noisy)) return 1;
    return estimate(c, who, c->h2d_noisy.as<float>(), h_mask, asize, W, H, C, lo, hi, out);
}

int lfbm5d_pgclip_forward_device(lfbm5d_ctx* c, const struct lfbm5d_pgclip_curves* curves, const float* d_in, const unsigned* h_mask, float* d_out,
                                 unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return map_entry<false>(c, "lfbm5d_pgclip_forward_device", curves, d_in, h_mask, d_out, asize, W, H, C);
}

int lfbm5d_pgclip_inverse_device(lfbm5d_ctx* c, const struct lfbm5d_pgclip_curves* curves, const float* d_in, const unsigned* h_mask, float* d_out,
                                 unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return map_entry<true>(c, "lfbm5d_pgclip_inverse_device", curves, d_in, h_mask, d_out, asize, W, H, C);
}

int lfbm5d_denoise_pgclip_device(lfbm5d_ctx* c, const lfbm5d_pgclip_model* model, double lo, double hi, lfbm5d_pgclip_model* used,
                                 double* s_used, lfbm5d_pgclip_estimate* est, const lfbm5d_params* P1, const lfbm5d_params* P2, const float* d_noisy,
                                 const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight,
                                 unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return denoise_pgclip(c, "lfbm5d_denoise_pgclip_device: ", model, lo, hi, used, s_used, est, P1, P2, d_noisy, h_mask, d_basic, d_denoised, ang_major,
                          awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_denoise_pgclip_host_sai(lfbm5d_ctx* c, const lfbm5d_pgclip_model* model, double lo, double hi, lfbm5d_pgclip_model* used,
                                   double* s_used, lfbm5d_pgclip_estimate* est, const lfbm5d_params* P1, const lfbm5d_params* P2, const float* const* h_noisy,
                                   const unsigned* h_mask, float* const* h_basic, float* const* h_denoised, unsigned ang_major, unsigned awidth,
                                   unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    const std::string who = "lfbm5d_denoise_pgclip_host_sai: ";
    if (check_chnls(c, who, C)) return 1;
    return host_sai_job(c, who, h_noisy, h_mask, h_basic, h_denoised, awidth * aheight, (size_t)C * W * H, [&](float* dn, float* db, float* dd) {
        return denoise_pgclip(c, who, model, lo, hi, used, s_used, est, P1, P2, dn, h_mask, db, dd, ang_major, awidth, aheight, an1, an2, W, H, C);
    });
}

} /* extern "C" */
