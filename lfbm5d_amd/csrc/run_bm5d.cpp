/*
 * run_bm5d.cpp -- the reference's outer seam (src/bm5d.h:11-62) on top of the C-ABI.
 * Host side only: hands the library one pointer per SAI -- the vectors' own storage, no flat copy -- through
 * lfbm5d_step{1,2}_host_sai / lfbm5d_denoise_host_sai, which stream the SAIs through HBM as the window graph needs and
 * finishes them and run every kernel on the GPU (round 5; rounds 1-4 flattened, copied four light fields and unflattened).
 * Error behaviour follows the reference: message on stdout, EXIT_FAILURE.
 */
#include "run_bm5d.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iostream>
#include <memory>
#include <thread>
#include <type_traits>
#include <utility>

#include "../../include/lfbm5d.h"

namespace {

typedef std::vector<std::vector<float> > LF;
typedef std::vector<unsigned> Mask;

/* the line a refusal of the library ends in */
int report(lfbm5d_ctx* ctx) {
    std::cout << "LFBM5D GPU backend: " << lfbm5d_last_error(ctx) << std::endl;
    return EXIT_FAILURE;
}

lfbm5d_ctx* context() {
    static lfbm5d_ctx* ctx = nullptr;
    if (!ctx) {
        const char* dev = std::getenv("LFBM5D_DEVICE");
        if (lfbm5d_create(&ctx, dev ? std::atoi(dev) : 0) != 0) {
            report(nullptr);
            ctx = nullptr;
        }
    }
    return ctx;
}

/* the SAIs of the reference's vector-of-vectors light field <-> one flat buffer, by a few threads: at 17 x 17 x 512 x 512 x 3 a light
 * field is 0.9 GB and a step moves three to five of them -- one thread's memcpy of that is longer than the step on the GPU */
template <class F> void for_sais(size_t n, F fn) {
    const unsigned nt = (unsigned)std::min<size_t>(std::min(8u, std::max(1u, std::thread::hardware_concurrency())), std::max<size_t>(1, n));
    std::atomic<size_t> next(0);
    auto work = [&]() { for (size_t i = next++; i < n; i = next++) fn(i); };
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nt; i++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
}
/* flat buffers: uninitialised storage (every byte is written by flatten or by the library's device-to-host copy) */
typedef std::unique_ptr<float[]> Flat;
Flat flat_alloc(size_t n) { return Flat(new float[n]); }
void flatten(const LF& lf, const Mask& mask, size_t img, Flat& flat) {
    flat = flat_alloc(lf.size() * img);
    for_sais(lf.size(), [&](size_t st) {
        if (mask[st] && lf[st].size() == img) std::memcpy(&flat[st * img], lf[st].data(), img * sizeof(float));
        else std::memset(&flat[st * img], 0, img * sizeof(float));
    });
}
void unflatten(LF& lf, const Mask& mask, size_t img, const Flat& flat) {
    for_sais(lf.size(), [&](size_t st) {
        if (!mask[st]) return;
        if (lf[st].size() != img) lf[st].resize(img);
        std::memcpy(lf[st].data(), &flat[st * img], img * sizeof(float));
    });
}

/* One pointer per SAI into the caller's vectors, for planes of float, const float and unsigned char alike.  output (float planes): the vectors of
 * non-empty SAIs get their size first (the reference resizes them where it forms the estimates, utilities_LF.cpp:936-941); otherwise
 * a non-empty SAI of another size is refused under `who`'s name (tail: " and flags" where values and flags are checked as a pair).
 * Empty SAIs are left alone. */
template <class V> using Plane = decltype(std::declval<V&>()[0].data());
template <class V>
bool sai_ptrs(const char* who, V& lf, const Mask& mask, size_t img, bool output, std::vector<Plane<V> >& p, const char* tail = "") {
    p = std::vector<Plane<V> >(lf.size(), nullptr);
    if constexpr (std::is_same<V, LF>::value)
        if (output) for_sais(lf.size(), [&](size_t st) { if (mask[st] && lf[st].size() != img) lf[st].resize(img); });
    for (size_t st = 0; st < lf.size(); st++) {
        if (!mask[st]) continue;
        if (lf[st].size() != img) { std::cout << who << ": a non-empty SAI does not hold width*height*chnls values" << tail << std::endl; return false; }
        p[st] = lf[st].data();
    }
    return true;
}

/* one (possibly empty) vector per SAI: what the reference does to its outputs where it enters a step (bm5d.cpp:129-130, :823-824) */
void size_sais(LF& lf, size_t asize) { if (lf.size() != asize) lf.resize(asize); }

/* the nine parameters of a step, in the order of the reference's argument lists */
struct Step { unsigned N, nSim, nDisp, k, p; bool useSD; unsigned tau_2D, tau_4D, tau_5D; };

lfbm5d_params make(float sigma, float lambda, const Step& s, unsigned cs) {
    lfbm5d_params P;
    P.sigma = sigma; P.lambda = lambda; P.N = s.N; P.nSim = s.nSim; P.nDisp = s.nDisp; P.k = s.k; P.p = s.p;
    P.useSD = s.useSD ? 1u : 0u; P.tau_2D = s.tau_2D; P.tau_4D = s.tau_4D; P.tau_5D = s.tau_5D; P.color_space = cs;
    return P;
}

/* nb_threads selects the reference's tile mode (bm5d.cpp:411-708), whose result depends on the caller's core count and is
 * about 0.5 dB below the untiled one.  The GPU path therefore ignores it -- nb_threads == 1 semantics -- unless
 * LFBM5D_TILED is set in the environment: then nb_threads tiles (floored to a power of two) are reproduced. */
int tiles_for(unsigned nb_threads) {
    const char* e = std::getenv("LFBM5D_TILED");
    return (e && *e && *e != '0' && nb_threads > 1) ? (int)nb_threads : 1;
}

/* What the two steps and the jobs over both share, up to the library call: the count check (`counts` is the sentence it prints; ok:
 * what the job checks next to the sizes), the context, the tile mode, the outputs' sizes, one pointer per SAI of each light field --
 * the vectors' own storage, no copy -- and both steps' parameters.  basic_out: LF_basic is written, not read; LF_denoised may be NULL
 * (the first step has none). */
const char* const kCounts = "light field and mask must hold awidth*aheight SAIs";
template <class V> struct Job {
    lfbm5d_ctx* ctx = nullptr;
    std::vector<Plane<V> > noisy;
    std::vector<float*> basic, den;
    lfbm5d_params P1, P2;

    /* false: refused, and the message is out */
    bool open(const char* who, const char* counts, bool ok, V& LF_noisy, const Mask& mask, LF& LF_basic, bool basic_out, LF* LF_denoised,
              unsigned awidth, unsigned aheight, unsigned width, unsigned height, unsigned chnls, float sigma, float lambda, const Step& hard,
              const Step& wien, unsigned color_space, unsigned nb_threads) {
        const unsigned asize = awidth * aheight;
        if (LF_noisy.size() != asize || mask.size() != asize || (!basic_out && LF_basic.size() != asize) || !ok) {
            std::cout << who << ": " << counts << std::endl;
            return false;
        }
        if (!(ctx = context())) return false;
        lfbm5d_set_tiles(ctx, tiles_for(nb_threads));
        size_sais(LF_basic, asize);
        if (LF_denoised) size_sais(*LF_denoised, asize);
        const size_t img = (size_t)width * height * chnls;
        if (!sai_ptrs(who, LF_noisy, mask, img, false, noisy) || !sai_ptrs(who, LF_basic, mask, img, basic_out, basic)) return false;
        if (LF_denoised) sai_ptrs(who, *LF_denoised, mask, img, true, den);
        P1 = make(sigma, lambda, hard, color_space);
        P2 = make(sigma, 0.0f, wien, color_space);
        return true;
    }
};

/* the stages on one light field of any number of SAIs: the count check, the context, the planes.  NULL: refused, the message is out */
template <class V>
lfbm5d_ctx* open_stage(const char* who, V& lf, const Mask& mask, unsigned width, unsigned height, unsigned chnls, std::vector<Plane<V> >& p) {
    if (lf.size() != mask.size()) {
        std::cout << who << ": light field and mask must hold the same number of SAIs" << std::endl;
        return nullptr;
    }
    lfbm5d_ctx* ctx = context();
    return ctx && sai_ptrs(who, lf, mask, (size_t)width * height * chnls, false, p) ? ctx : nullptr;
}

/* Light fields through device buffers of this call, for what the library has a device form of only: the first is flattened and
 * uploaded, call(d) runs on one buffer per light field, every one comes back into its vectors.  The sentences a failure outside the
 * library prints differ between the callers (NULL: none). */
struct Dev {
    void* p = nullptr;
    Dev() {}
    Dev(const Dev&) = delete;
    ~Dev() { if (p) lfbm5d_free(p); }
};
struct TripWords { const char *memory, *upload, *download; };
const TripWords kTransformWords = {"out of device memory", nullptr, nullptr};
const TripWords kBm3dWords = {"no device memory for the light fields", "no device memory for the light fields", "device-to-host copy failed"};
template <class Call>
int device_round_trip(const char* who, const TripWords& words, lfbm5d_ctx* ctx, std::initializer_list<LF*> lfs, const Mask& mask, size_t img, Call call) {
    const auto refuse = [&](const char* what) { if (what) std::cout << who << ": " << what << std::endl; return EXIT_FAILURE; };
    const size_t bytes = mask.size() * img * sizeof(float);
    Flat flat;
    flatten(**lfs.begin(), mask, img, flat);
    std::vector<Dev> d(lfs.size());
    for (Dev& x : d) if (lfbm5d_malloc(&x.p, std::max(sizeof(float), bytes)) != 0) return refuse(words.memory);
    if (lfbm5d_memcpy_h2d(d[0].p, flat.get(), bytes) != 0) return refuse(words.upload);
    if (call(d) != 0) return report(ctx);
    size_t i = 0;
    for (LF* lf : lfs) {
        if (lfbm5d_memcpy_d2h(flat.get(), d[i++].p, bytes) != 0) return refuse(words.download);
        unflatten(*lf, mask, img, flat);
    }
    return EXIT_SUCCESS;
}

/* The test hooks' light fields: vectors from a flat copy [asize][n] and back, for the SAIs that `take` names (the others stay empty,
 * their part of the flat copy untouched; a NULL flat copy is skipped). */
template <class T> std::vector<std::vector<T> > from_flat(const T* flat, const Mask& take, size_t n) {
    std::vector<std::vector<T> > lf(take.size());
    for (size_t st = 0; st < take.size(); st++) if (take[st]) lf[st].assign(flat + st * n, flat + (st + 1) * n);
    return lf;
}
template <class T> void to_flat(const std::vector<std::vector<T> >& lf, const Mask& take, size_t n, T* flat) {
    if (!flat) return;
    for (size_t st = 0; st < take.size(); st++) if (take[st] && lf[st].size() == n) std::memcpy(flat + st * n, lf[st].data(), n * sizeof(T));
}

} // namespace

int run_bm5d_1st_step(const float sigma, const float lambdaHard5D, std::vector<std::vector<float> >& LF_noisy,
                      std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_basic,
                      const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard,
                      const unsigned width, const unsigned height, const unsigned chnls, const unsigned NHard,
                      const unsigned nSim, const unsigned nDisp, const unsigned kHard, const unsigned pHard,
                      const bool useSD, const unsigned tau_2D, unsigned tau_4D, const unsigned tau_5D,
                      const unsigned color_space, const unsigned nb_threads) {
    const Step step = {NHard, nSim, nDisp, kHard, pHard, useSD, tau_2D, tau_4D, tau_5D};
    Job<LF> j;
    if (!j.open("run_bm5d_1st_step", kCounts, true, LF_noisy, LF_SAI_mask, LF_basic, true, nullptr, awidth, aheight, width, height, chnls, sigma, lambdaHard5D,
                step, step, color_space, nb_threads)) return EXIT_FAILURE;
    if (lfbm5d_step1_host_sai(j.ctx, &j.P1, j.noisy.data(), LF_SAI_mask.data(), j.basic.data(), ang_major, awidth, aheight, anHard, width, height,
                              chnls) != 0) return report(j.ctx);
    return EXIT_SUCCESS;
}

int run_bm5d_2nd_step(const float sigma, std::vector<std::vector<float> >& LF_noisy, std::vector<unsigned>& LF_SAI_mask,
                      std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised,
                      const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anWien,
                      const unsigned width, const unsigned height, const unsigned chnls, const unsigned NWien,
                      const unsigned nSim, const unsigned nDisp, const unsigned kWien, const unsigned pWien,
                      const bool useSD, const unsigned tau_2D, unsigned tau_4D, const unsigned tau_5D,
                      const unsigned color_space, const unsigned nb_threads) {
    const Step step = {NWien, nSim, nDisp, kWien, pWien, useSD, tau_2D, tau_4D, tau_5D};
    Job<LF> j;
    if (!j.open("run_bm5d_2nd_step", "light fields and mask must hold awidth*aheight SAIs", true, LF_noisy, LF_SAI_mask, LF_basic, false, &LF_denoised,
                awidth, aheight, width, height, chnls, sigma, 0.0f, step, step, color_space, nb_threads)) return EXIT_FAILURE;
    if (lfbm5d_step2_host_sai(j.ctx, &j.P2, j.noisy.data(), LF_SAI_mask.data(), j.basic.data(), j.den.data(), ang_major, awidth, aheight, anWien, width,
                              height, chnls) != 0) return report(j.ctx);
    return EXIT_SUCCESS;
}

/* main.cpp:195 + :242 as one job (lfbm5d_denoise_host): same buffers on return as the two calls.  The tile mode (LFBM5D_TILED) has no
 * graph form: the library then runs the two steps one after the other behind the same entry point. */
int run_bm5d(const float sigma, const float lambdaHard5D, std::vector<std::vector<float> >& LF_noisy, std::vector<unsigned>& LF_SAI_mask,
             std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised, const unsigned ang_major,
             const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned anWien, const unsigned width,
             const unsigned height, const unsigned chnls, const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard,
             const unsigned kHard, const unsigned pHard, const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard,
             const unsigned tau_5D_hard, const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien,
             const unsigned pWien, const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien,
             const unsigned color_space, const unsigned nb_threads) {
    Job<LF> j;
    if (!j.open("run_bm5d", kCounts, true, LF_noisy, LF_SAI_mask, LF_basic, true, &LF_denoised, awidth, aheight, width, height, chnls, sigma, lambdaHard5D,
                {NHard, nSimHard, nDispHard, kHard, pHard, useSDHard, tau_2D_hard, tau_4D_hard, tau_5D_hard},
                {NWien, nSimWien, nDispWien, kWien, pWien, useSDWien, tau_2D_wien, tau_4D_wien, tau_5D_wien}, color_space, nb_threads)) return EXIT_FAILURE;
    if (lfbm5d_denoise_host_sai(j.ctx, &j.P1, &j.P2, j.noisy.data(), LF_SAI_mask.data(), j.basic.data(), j.den.data(), ang_major, awidth, aheight,
                                anHard, anWien, width, height, chnls) != 0) return report(j.ctx);
    return EXIT_SUCCESS;
}

/* blind noise level on the caller's vectors (one pointer per SAI, no flat copy) */
int noise_level_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width, unsigned height,
                   unsigned chnls, float& sigma) {
    std::vector<const float*> p;
    lfbm5d_ctx* ctx = open_stage("noise_level_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    lfbm5d_noise_level r;
    if (lfbm5d_noise_level_host_sai(ctx, p.data(), LF_SAI_mask.data(), (unsigned)LF.size(), width, height, chnls, 0, &r, nullptr, nullptr) != 0) return report(ctx);
    sigma = (float)r.sigma;
    return EXIT_SUCCESS;
}

/* Poisson-Gaussian noise model on the caller's vectors (one pointer per SAI, no flat copy) */
int pg_estimate_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width, unsigned height,
                   unsigned chnls, double& a, double& b) {
    std::vector<const float*> p;
    lfbm5d_ctx* ctx = open_stage("pg_estimate_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    lfbm5d_pg_estimate r;
    if (lfbm5d_pg_estimate_host_sai(ctx, p.data(), LF_SAI_mask.data(), (unsigned)LF.size(), width, height, chnls, &r, nullptr, nullptr) != 0) return report(ctx);
    a = r.a; b = r.b;
    return EXIT_SUCCESS;
}

/* impulse repair on the caller's vectors, in place for the caller (one pointer per SAI; the library stages in and out apart) */
int impulse_repair_LF(std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width, unsigned height,
                      unsigned chnls, double k, unsigned long long& flagged, unsigned long long& left, double thresholds[3]) {
    std::vector<float*> p;
    lfbm5d_ctx* ctx = open_stage("impulse_repair_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    lfbm5d_impulse_params P;
    lfbm5d_impulse_defaults(&P);
    P.k = k;
    lfbm5d_impulse_result r;
    if (lfbm5d_impulse_repair_host_sai(ctx, &P, p.data(), nullptr, LF_SAI_mask.data(), p.data(), nullptr, (unsigned)LF.size(), width, height, chnls,
                                       &r, nullptr) != 0) return report(ctx);
    flagged = left = 0;
    for (unsigned c = 0; c < 3; c++) { flagged += r.flagged[c]; left += r.left[c]; thresholds[c] = r.threshold[c]; }
    return EXIT_SUCCESS;
}

namespace {

lfbm5d_pg_model pg_model_of(double a, double b) {
    lfbm5d_pg_model m;
    for (int c = 0; c < 3; c++) { m.a[c] = a; m.b[c] = b; }
    return m;
}

/* the transforms have device forms only: the light field goes through a device buffer of this call */
int pg_transform_LF(const char* who, bool inverse, double a, double b, std::vector<std::vector<float> >& LF, const std::vector<unsigned>& mask,
                    unsigned width, unsigned height, unsigned chnls, float* sigma) {
    if (LF.size() != mask.size()) { std::cout << who << ": light field and mask must hold the same number of SAIs" << std::endl; return EXIT_FAILURE; }
    const lfbm5d_pg_model m = pg_model_of(a, b);
    double s = 0.0;
    if (lfbm5d_pg_scale(&m, chnls, &s) != 0) {
        std::cout << who << ": bad noise model (needs a >= 0 and 3/8 a^2 + b > 0; chnls 1 or 3)" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<float*> p;
    if (!sai_ptrs(who, LF, mask, img, false, p)) return EXIT_FAILURE;
    const int rc = device_round_trip(who, kTransformWords, ctx, {&LF}, mask, img, [&](const std::vector<Dev>& d) {
        return (inverse ? lfbm5d_pg_inverse_device : lfbm5d_pg_forward_device)(ctx, &m, (const float*)d[0].p, mask.data(), (float*)d[0].p,
                                                                               (unsigned)LF.size(), width, height, chnls);
    });
    if (rc == EXIT_SUCCESS && sigma) *sigma = (float)s;
    return rc;
}

} // namespace

int pg_forward_LF(double a, double b, std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width,
                  unsigned height, unsigned chnls, float& sigma) {
    return pg_transform_LF("pg_forward_LF", false, a, b, LF, LF_SAI_mask, width, height, chnls, &sigma);
}

int pg_inverse_LF(double a, double b, std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width,
                  unsigned height, unsigned chnls) {
    return pg_transform_LF("pg_inverse_LF", true, a, b, LF, LF_SAI_mask, width, height, chnls, nullptr);
}

int denoise_pg_LF(double& a, double& b, const bool estimate, float& sigma, const float lambdaHard5D, const std::vector<std::vector<float> >& LF_noisy,
                  std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised,
                  const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned anWien,
                  const unsigned width, const unsigned height, const unsigned chnls, const unsigned NHard, const unsigned nSimHard,
                  const unsigned nDispHard, const unsigned kHard, const unsigned pHard, const bool useSDHard, const unsigned tau_2D_hard,
                  unsigned tau_4D_hard, const unsigned tau_5D_hard, const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien,
                  const unsigned kWien, const unsigned pWien, const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien,
                  const unsigned tau_5D_wien, const unsigned color_space, const unsigned nb_threads) {
    Job<const LF> j;
    if (!j.open("denoise_pg_LF", kCounts, true, LF_noisy, LF_SAI_mask, LF_basic, true, &LF_denoised, awidth, aheight, width, height, chnls, 0.0f, lambdaHard5D,
                {NHard, nSimHard, nDispHard, kHard, pHard, useSDHard, tau_2D_hard, tau_4D_hard, tau_5D_hard},
                {NWien, nSimWien, nDispWien, kWien, pWien, useSDWien, tau_2D_wien, tau_4D_wien, tau_5D_wien}, color_space, nb_threads)) return EXIT_FAILURE;
    const lfbm5d_pg_model given = pg_model_of(a, b);
    lfbm5d_pg_model used;
    double s = 0.0;
    if (lfbm5d_denoise_pg_host_sai(j.ctx, estimate ? nullptr : &given, &used, &j.P1, &j.P2, j.noisy.data(), LF_SAI_mask.data(), j.basic.data(),
                                   j.den.data(), ang_major, awidth, aheight, anHard, anWien, width, height, chnls) != 0 ||
        lfbm5d_pg_scale(&used, chnls, &s) != 0) return report(j.ctx);
    a = used.a[0]; b = used.b[0];
    sigma = (float)s;
    return EXIT_SUCCESS;
}

/* clipping-aware noise level on the caller's vectors (one pointer per SAI, no flat copy) */
int noise_level_clipped_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width, unsigned height,
                           unsigned chnls, double lo, double hi, float& sigma, unsigned& levels, double& f_max) {
    std::vector<const float*> p;
    lfbm5d_ctx* ctx = open_stage("noise_level_clipped_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    lfbm5d_clip_estimate r;
    if (lfbm5d_noise_level_clipped_host_sai(ctx, p.data(), LF_SAI_mask.data(), (unsigned)LF.size(), width, height, chnls, lo, hi, &r) != 0) return report(ctx);
    sigma = (float)r.sigma; levels = r.levels; f_max = r.f_max;
    return EXIT_SUCCESS;
}

/* the inverse of the clipped mean on the caller's vectors, in place for the caller (one pointer per SAI; the library stages them) */
int declip_LF(double sigma, double lo, double hi, std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width,
              unsigned height, unsigned chnls) {
    std::vector<float*> p;
    lfbm5d_ctx* ctx = open_stage("declip_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    if (lfbm5d_declip_host_sai(ctx, sigma, lo, hi, p.data(), LF_SAI_mask.data(), p.data(), (unsigned)LF.size(), width, height, chnls) != 0) return report(ctx);
    return EXIT_SUCCESS;
}

int denoise_clipped_LF(float& sigma, double lo, double hi, const float lambdaHard5D, const std::vector<std::vector<float> >& LF_noisy,
                       std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised,
                       const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned anWien,
                       const unsigned width, const unsigned height, const unsigned chnls, const unsigned NHard, const unsigned nSimHard,
                       const unsigned nDispHard, const unsigned kHard, const unsigned pHard, const bool useSDHard, const unsigned tau_2D_hard,
                       unsigned tau_4D_hard, const unsigned tau_5D_hard, const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien,
                       const unsigned kWien, const unsigned pWien, const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien,
                       const unsigned tau_5D_wien, const unsigned color_space, const unsigned nb_threads) {
    Job<const LF> j;
    if (!j.open("denoise_clipped_LF", kCounts, true, LF_noisy, LF_SAI_mask, LF_basic, true, &LF_denoised, awidth, aheight, width, height, chnls, 0.0f, lambdaHard5D,
                {NHard, nSimHard, nDispHard, kHard, pHard, useSDHard, tau_2D_hard, tau_4D_hard, tau_5D_hard},
                {NWien, nSimWien, nDispWien, kWien, pWien, useSDWien, tau_2D_wien, tau_4D_wien, tau_5D_wien}, color_space, nb_threads)) return EXIT_FAILURE;
    double used = 0.0;
    if (lfbm5d_denoise_clipped_host_sai(j.ctx, (double)sigma, lo, hi, nullptr, &used, &j.P1, &j.P2, j.noisy.data(), LF_SAI_mask.data(), j.basic.data(),
                                        j.den.data(), ang_major, awidth, aheight, anHard, anWien, width, height, chnls) != 0) return report(j.ctx);
    sigma = (float)used;
    return EXIT_SUCCESS;
}

/* clipped Poisson-Gaussian model on the caller's vectors (one pointer per SAI, no flat copy) */
int pgclip_estimate_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, unsigned width, unsigned height,
                       unsigned chnls, double lo, double hi, double& a, double& b, unsigned& levels, double& f_max) {
    std::vector<const float*> p;
    lfbm5d_ctx* ctx = open_stage("pgclip_estimate_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    lfbm5d_pgclip_estimate r;
    if (lfbm5d_pgclip_estimate_host_sai(ctx, p.data(), LF_SAI_mask.data(), (unsigned)LF.size(), width, height, chnls, lo, hi, &r) != 0) return report(ctx);
    a = r.model.a; b = r.model.b; levels = r.levels; f_max = r.f_max;
    return EXIT_SUCCESS;
}

namespace {

/* the maps have device forms only: the light field goes through a device buffer of this call */
int pgclip_map_LF(const char* who, bool inverse, double a, double b, double lo, double hi, std::vector<std::vector<float> >& LF,
                  const std::vector<unsigned>& mask, unsigned width, unsigned height, unsigned chnls, float* sigma) {
    if (LF.size() != mask.size()) { std::cout << who << ": light field and mask must hold the same number of SAIs" << std::endl; return EXIT_FAILURE; }
    const lfbm5d_pgclip_model m = {a, b, lo, hi};
    std::vector<struct lfbm5d_pgclip_curves> cv(1);
    if (lfbm5d_pgclip_curves(&m, cv.data()) != 0) { std::cout << who << ": " << lfbm5d_pgclip_curves_error() << std::endl; return EXIT_FAILURE; }
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<float*> p;
    if (!sai_ptrs(who, LF, mask, img, false, p)) return EXIT_FAILURE;
    const int rc = device_round_trip(who, kTransformWords, ctx, {&LF}, mask, img, [&](const std::vector<Dev>& d) {
        return (inverse ? lfbm5d_pgclip_inverse_device : lfbm5d_pgclip_forward_device)(ctx, cv.data(), (const float*)d[0].p, mask.data(), (float*)d[0].p,
                                                                                       (unsigned)LF.size(), width, height, chnls);
    });
    if (rc == EXIT_SUCCESS && sigma) *sigma = (float)cv[0].s;
    return rc;
}

} // namespace

int pgclip_forward_LF(double a, double b, double lo, double hi, std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask,
                      unsigned width, unsigned height, unsigned chnls, float& sigma) {
    return pgclip_map_LF("pgclip_forward_LF", false, a, b, lo, hi, LF, LF_SAI_mask, width, height, chnls, &sigma);
}

int pgclip_inverse_LF(double a, double b, double lo, double hi, std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask,
                      unsigned width, unsigned height, unsigned chnls) {
    return pgclip_map_LF("pgclip_inverse_LF", true, a, b, lo, hi, LF, LF_SAI_mask, width, height, chnls, nullptr);
}

int denoise_pgclip_LF(double& a, double& b, double lo, double hi, const bool estimate, float& sigma, unsigned& levels, double& f_max,
                      const float lambdaHard5D, const std::vector<std::vector<float> >& LF_noisy, std::vector<unsigned>& LF_SAI_mask,
                      std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised, const unsigned ang_major,
                      const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned anWien, const unsigned width,
                      const unsigned height, const unsigned chnls, const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard,
                      const unsigned kHard, const unsigned pHard, const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard,
                      const unsigned tau_5D_hard, const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien,
                      const unsigned pWien, const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien,
                      const unsigned color_space, const unsigned nb_threads) {
    Job<const LF> j;
    if (!j.open("denoise_pgclip_LF", kCounts, true, LF_noisy, LF_SAI_mask, LF_basic, true, &LF_denoised, awidth, aheight, width, height, chnls, 0.0f, lambdaHard5D,
                {NHard, nSimHard, nDispHard, kHard, pHard, useSDHard, tau_2D_hard, tau_4D_hard, tau_5D_hard},
                {NWien, nSimWien, nDispWien, kWien, pWien, useSDWien, tau_2D_wien, tau_4D_wien, tau_5D_wien}, color_space, nb_threads)) return EXIT_FAILURE;
    const lfbm5d_pgclip_model given = {a, b, lo, hi};
    lfbm5d_pgclip_model used;
    lfbm5d_pgclip_estimate est;
    double s = 0.0;
    if (lfbm5d_denoise_pgclip_host_sai(j.ctx, estimate ? nullptr : &given, lo, hi, &used, &s, &est, &j.P1, &j.P2, j.noisy.data(), LF_SAI_mask.data(),
                                       j.basic.data(), j.den.data(), ang_major, awidth, aheight, anHard, anWien, width, height, chnls) != 0) return report(j.ctx);
    a = used.a; b = used.b; levels = est.levels; f_max = est.f_max;
    sigma = (float)s;
    return EXIT_SUCCESS;
}

int report_ssim_mode() {
    const char* e = std::getenv("LFBM5D_REPORT_SSIM");
    if (!e) return 0;
    if (!std::strcmp(e, "1")) return 1;
    std::cout << "LFBM5D_REPORT_SSIM must be \"1\" (report SSIM next to PSNR) or unset; got \"" << e << "\"" << std::endl;
    return -1;
}

/* quality metrics on the caller's vectors (one pointer per SAI, no flat copy) */
int quality_LF(const std::vector<std::vector<float> >& LF_1, const std::vector<std::vector<float> >& LF_2, const std::vector<unsigned>& LF_SAI_mask,
               unsigned width, unsigned height, unsigned chnls, std::vector<float>& psnr, float& avg_psnr, float& std_psnr, std::vector<float>& rmse,
               float& avg_rmse, float& std_rmse, std::vector<float>& ssim, float& avg_ssim, float& std_ssim) {
    const size_t asize = LF_SAI_mask.size();
    if (LF_1.size() != asize || LF_2.size() != asize) {
        std::cout << "quality_LF: light fields and mask must hold the same number of SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<const float*> p1, p2;
    if (!sai_ptrs("quality_LF", LF_1, LF_SAI_mask, img, false, p1) || !sai_ptrs("quality_LF", LF_2, LF_SAI_mask, img, false, p2)) return EXIT_FAILURE;
    lfbm5d_quality q;
    std::vector<double> mse(asize, 0.0), ss(asize, 0.0);
    if (lfbm5d_quality_host_sai(ctx, p1.data(), p2.data(), LF_SAI_mask.data(), (unsigned)asize, width, height, chnls, 255.0, 1, &q, mse.data(), ss.data()) != 0)
        return report(ctx);
    psnr.assign(asize, 0.0f); rmse.assign(asize, 0.0f); ssim.assign(asize, 0.0f);
    for (size_t st = 0; st < asize; st++) {
        if (!LF_SAI_mask[st]) continue;
        psnr[st] = (float)(10.0 * std::log10(255.0 * 255.0 / mse[st])); rmse[st] = (float)std::sqrt(mse[st]); ssim[st] = (float)ss[st];
    }
    avg_psnr = (float)q.psnr_mean; std_psnr = (float)q.psnr_std;
    avg_rmse = (float)q.rmse_mean; std_rmse = (float)q.rmse_std;
    avg_ssim = (float)q.ssim_mean; std_ssim = (float)q.ssim_std;
    return EXIT_SUCCESS;
}

/* super-resolution on the caller's vectors (one pointer per SAI, no flat copy) */
int superres_LF(const std::vector<std::vector<float> >& LF_low, const std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_high,
                const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned width,
                const unsigned height, const unsigned chnls, const unsigned scale, const unsigned kernel, const float blurSigma,
                const unsigned iterations, const float sigmaStart, const float sigmaEnd, const float lambdaHard5D, const unsigned NHard,
                const unsigned nSim, const unsigned nDisp, const unsigned kHard, const unsigned pHard, const bool useSD, const unsigned tau_2D,
                unsigned tau_4D, const unsigned tau_5D, const unsigned color_space) {
    const unsigned asize = awidth * aheight;
    if (LF_low.size() != asize || LF_SAI_mask.size() != asize) {
        std::cout << "superres_LF: light field and mask must hold awidth*aheight SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_sr_params sr;
    if (lfbm5d_sr_defaults(scale, &sr) != 0) { std::cout << "superres_LF: scale must be 2, 3 or 4" << std::endl; return EXIT_FAILURE; }
    sr.kernel = kernel;
    if (kernel == LFBM5D_SR_GAUSSIAN) sr.blur_sigma = blurSigma;
    if (iterations) sr.iterations = iterations;
    if (sigmaStart != 0.0f) sr.sigma_start = sigmaStart;
    if (sigmaEnd != 0.0f) sr.sigma_end = sigmaEnd;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    size_sais(LF_high, asize);
    const size_t lo = (size_t)width * height * chnls, hi = lo * scale * scale;
    std::vector<const float*> low;
    std::vector<float*> high;
    if (!sai_ptrs("superres_LF", LF_low, LF_SAI_mask, lo, false, low)) return EXIT_FAILURE;
    sai_ptrs("superres_LF", LF_high, LF_SAI_mask, hi, true, high);
    const lfbm5d_params P = make(0.0f, lambdaHard5D, {NHard, nSim, nDisp, kHard, pHard, useSD, tau_2D, tau_4D, tau_5D}, color_space);
    if (lfbm5d_superres_host_sai(ctx, &sr, &P, low.data(), LF_SAI_mask.data(), high.data(), ang_major, awidth, aheight, anHard, width, height,
                                 chnls) != 0) return report(ctx);
    return EXIT_SUCCESS;
}

/* Test hook: superres_LF on vector<vector<float>> light fields built from a flat low-resolution copy [asize][chnls*height*width]; the
 * result goes to high_out [asize][chnls*scale*height*scale*width].  sr = {scale, kernel, iterations}, srf = {blurSigma, sigmaStart,
 * sigmaEnd, lambda}, hard = {N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D}. */
extern "C" int lfbm5d_superres_probe(const float* low_flat, const unsigned* mask, float* high_out, unsigned ang_major, unsigned awidth,
                                     unsigned aheight, unsigned an, unsigned width, unsigned height, unsigned chnls, const unsigned* sr,
                                     const float* srf, const unsigned* hard, unsigned color_space) {
    const size_t asize = (size_t)awidth * aheight, lo = (size_t)width * height * chnls, hi = lo * sr[0] * sr[0];
    std::vector<unsigned> m(mask, mask + asize);
    std::vector<std::vector<float> > LF_low = from_flat(low_flat, m, lo), LF_high;
    if (superres_LF(LF_low, m, LF_high, ang_major, awidth, aheight, an, width, height, chnls, sr[0], sr[1], srf[0], sr[2], srf[1], srf[2], srf[3],
                    hard[0], hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], color_space) != EXIT_SUCCESS) return 1;
    to_flat(LF_high, m, hi, high_out);
    return 0;
}

/* defect inpainting on the caller's vectors, in place for the caller (one pointer per SAI; the library stages in and out apart) */
int inpaint_LF(std::vector<std::vector<float> >& LF, const std::vector<std::vector<unsigned char> >& flags, const std::vector<unsigned>& LF_SAI_mask,
               const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned width,
               const unsigned height, const unsigned chnls, const int iterations, const float sigmaStart, const float sigmaEnd,
               const float sigmaNoise, const float lambdaHard5D, const unsigned NHard, const unsigned nSim, const unsigned nDisp,
               const unsigned kHard, const unsigned pHard, const bool useSD, const unsigned tau_2D, unsigned tau_4D, const unsigned tau_5D,
               const unsigned color_space, unsigned long long& flagged, unsigned long long& left, unsigned& passes) {
    const unsigned asize = awidth * aheight;
    if (LF.size() != asize || flags.size() != asize || LF_SAI_mask.size() != asize) {
        std::cout << "inpaint_LF: light field, flags and mask must hold awidth*aheight SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_inpaint_params ip;
    lfbm5d_inpaint_defaults(&ip);
    if (iterations >= 0) ip.iterations = (unsigned)iterations;
    if (sigmaStart != 0.0f) ip.sigma_start = sigmaStart;
    if (sigmaEnd != 0.0f) ip.sigma_end = sigmaEnd;
    ip.sigma_noise = sigmaNoise;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<float*> p;
    std::vector<const unsigned char*> f;
    if (!sai_ptrs("inpaint_LF", LF, LF_SAI_mask, img, false, p, " and flags") || !sai_ptrs("inpaint_LF", flags, LF_SAI_mask, img, false, f, " and flags"))
        return EXIT_FAILURE;
    const lfbm5d_params P = make(0.0f, lambdaHard5D, {NHard, nSim, nDisp, kHard, pHard, useSD, tau_2D, tau_4D, tau_5D}, color_space);
    lfbm5d_inpaint_result r;
    std::memset(&r, 0, sizeof(r));
    const int rc = lfbm5d_inpaint_host_sai(ctx, &ip, &P, p.data(), f.data(), LF_SAI_mask.data(), p.data(), nullptr, ang_major, awidth, aheight,
                                           anHard, width, height, chnls, &r);
    flagged = left = 0;
    for (unsigned c = 0; c < 3; c++) { flagged += r.flagged[c]; left += r.left[c]; }
    passes = r.passes;
    return rc != 0 ? report(ctx) : EXIT_SUCCESS;
}

/* Test hook: inpaint_LF on vector<vector<float>> light fields built from flat copies [asize][chnls*height*width]; the result goes to
 * out_flat.  ipf = {sigmaStart, sigmaEnd, sigmaNoise, lambda}, hard = {N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D},
 * counts = {flagged, left, passes}. */
extern "C" int lfbm5d_inpaint_probe(const float* in_flat, const unsigned char* flags_flat, const unsigned* mask, float* out_flat,
                                    unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned width, unsigned height,
                                    unsigned chnls, int iterations, const float* ipf, const unsigned* hard, unsigned color_space,
                                    unsigned long long* counts) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize);
    std::vector<std::vector<float> > LF = from_flat(in_flat, m, img);
    const std::vector<std::vector<unsigned char> > fl = from_flat(flags_flat, m, img);
    unsigned long long flagged = 0, left = 0; unsigned passes = 0;
    if (inpaint_LF(LF, fl, m, ang_major, awidth, aheight, an, width, height, chnls, iterations, ipf[0], ipf[1], ipf[2], ipf[3], hard[0], hard[1],
                   hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], color_space, flagged, left, passes) != EXIT_SUCCESS) return 1;
    to_flat(LF, m, img, out_flat);
    if (counts) { counts[0] = flagged; counts[1] = left; counts[2] = passes; }
    return 0;
}

/* view synthesis on the caller's vectors, in place for the caller (one pointer per SAI; the library stages in and out apart) */
int view_synth_LF(std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, const std::vector<unsigned>& missing,
                  const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned width,
                  const unsigned height, const unsigned chnls, const int maxDisparity, const int boxRadius, const int angRadius,
                  const int iterations, const float sigmaStart, const float sigmaEnd, const float sigmaNoise, const float lambdaHard5D,
                  const unsigned NHard, const unsigned nSim, const unsigned nDisp, const unsigned kHard, const unsigned pHard, const bool useSD,
                  const unsigned tau_2D, unsigned tau_4D, const unsigned tau_5D, const unsigned color_space, unsigned& synthesised,
                  unsigned& left, int& dmin, int& dmax, const unsigned disparity_steps, const float occl_ratio, unsigned long long* set_hist) {
    const unsigned asize = awidth * aheight;
    synthesised = left = 0; dmin = dmax = 0;
    if (set_hist) std::memset(set_hist, 0, LFBM5D_VIEW_OCCL_SETS * sizeof(unsigned long long));
    if (LF.size() != asize || LF_SAI_mask.size() != asize || missing.size() != asize) {
        std::cout << "view_synth_LF: light field, mask and missing must hold awidth*aheight SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_view_params vp;
    lfbm5d_view_defaults(&vp);
    if (maxDisparity >= 0) vp.max_disparity = (unsigned)maxDisparity;
    if (boxRadius >= 0) vp.box_radius = (unsigned)boxRadius;
    if (angRadius >= 0) vp.ang_radius = (unsigned)angRadius;
    if (iterations >= 0) vp.iterations = (unsigned)iterations;
    if (sigmaStart != 0.0f) vp.sigma_start = sigmaStart;
    if (sigmaEnd != 0.0f) vp.sigma_end = sigmaEnd;
    vp.sigma_noise = sigmaNoise;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<float*> p(asize, nullptr);
    for (size_t st = 0; st < asize; st++)
        if (LF_SAI_mask[st]) {
            if (missing[st]) LF[st].resize(img);
            else if (LF[st].size() != img) {
                std::cout << "view_synth_LF: a sound SAI does not hold width*height*chnls values" << std::endl;
                return EXIT_FAILURE;
            }
            p[st] = LF[st].data();
        }
    const lfbm5d_params P = make(0.0f, lambdaHard5D, {NHard, nSim, nDisp, kHard, pHard, useSD, tau_2D, tau_4D, tau_5D}, color_space);
    lfbm5d_view_result r;
    std::memset(&r, 0, sizeof(r));
    unsigned long long hist[LFBM5D_VIEW_STEPS_HIST] = {0};
    int rc;
    if (occl_ratio != 0.0f) {                                                   /* (a NaN goes this way too, and is rejected there) */
        lfbm5d_view_occl_result o = {};
        rc = lfbm5d_view_occl_host_sai(ctx, &vp, disparity_steps, occl_ratio, &P, p.data(), LF_SAI_mask.data(), missing.data(), p.data(), nullptr,
                                       nullptr, ang_major, awidth, aheight, anHard, width, height, chnls, &r, hist, &o);
        if (set_hist) std::memcpy(set_hist, o.set_hist, sizeof(o.set_hist));
    } else if (disparity_steps == 1) {                                          /* the integer form: its name in the messages */
        rc = lfbm5d_view_host_sai(ctx, &vp, &P, p.data(), LF_SAI_mask.data(), missing.data(), p.data(), nullptr, ang_major, awidth, aheight,
                                  anHard, width, height, chnls, &r);
        for (int d = -8; d <= 8; d++) hist[d + 32] = r.disparity_hist[d + 8];
    } else
        rc = lfbm5d_view_steps_host_sai(ctx, &vp, disparity_steps, &P, p.data(), LF_SAI_mask.data(), missing.data(), p.data(), nullptr,
                                        ang_major, awidth, aheight, anHard, width, height, chnls, &r, hist);
    synthesised = r.synthesised; left = r.left;
    bool any = false;
    for (int j = -32; j <= 32; j++)
        if (hist[j + 32]) { if (!any) dmin = j; dmax = j; any = true; }
    return rc != 0 ? report(ctx) : EXIT_SUCCESS;
}

/* Test hook: view_synth_LF on a vector<vector<float>> light field built from a flat copy [asize][chnls*height*width] (the vectors of
 * missing SAIs stay empty); the result goes to out_flat.  vpi = {maxDisparity, boxRadius, angRadius, iterations},
 * vpf = {sigmaStart, sigmaEnd, sigmaNoise, lambda}, hard = {N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D},
 * counts = {synthesised, left, dmin, dmax}. */
static int view_synth_probe(const float* in_flat, const unsigned* mask, const unsigned* missing, float* out_flat, unsigned ang_major,
                            unsigned awidth, unsigned aheight, unsigned an, unsigned width, unsigned height, unsigned chnls, const int* vpi,
                            const float* vpf, const unsigned* hard, unsigned color_space, int* counts, unsigned disparity_steps,
                            float occl_ratio = 0.0f, unsigned long long* set_hist = nullptr) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize), ms(missing, missing + asize), sound(asize);
    for (size_t st = 0; st < asize; st++) sound[st] = m[st] && !ms[st];
    std::vector<std::vector<float> > LF = from_flat(in_flat, sound, img);
    unsigned synthesised = 0, left = 0; int dmin = 0, dmax = 0;
    const int rc = view_synth_LF(LF, m, ms, ang_major, awidth, aheight, an, width, height, chnls, vpi[0], vpi[1], vpi[2], vpi[3], vpf[0], vpf[1],
                                 vpf[2], vpf[3], hard[0], hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], color_space,
                                 synthesised, left, dmin, dmax, disparity_steps, occl_ratio, set_hist);
    if (counts) { counts[0] = (int)synthesised; counts[1] = (int)left; counts[2] = dmin; counts[3] = dmax; }
    if (rc != EXIT_SUCCESS) return 1;
    to_flat(LF, m, img, out_flat);
    return 0;
}

extern "C" int lfbm5d_view_synth_probe(const float* in_flat, const unsigned* mask, const unsigned* missing, float* out_flat, unsigned ang_major,
                                       unsigned awidth, unsigned aheight, unsigned an, unsigned width, unsigned height, unsigned chnls,
                                       const int* vpi, const float* vpf, const unsigned* hard, unsigned color_space, int* counts) {
    return view_synth_probe(in_flat, mask, missing, out_flat, ang_major, awidth, aheight, an, width, height, chnls, vpi, vpf, hard, color_space,
                            counts, 1);
}

/* The same with view_synth_LF's disparity_steps; dmin and dmax are then in units of 1 / disparity_steps. */
extern "C" int lfbm5d_view_synth_steps_probe(const float* in_flat, const unsigned* mask, const unsigned* missing, float* out_flat,
                                             unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned width, unsigned height,
                                             unsigned chnls, const int* vpi, const float* vpf, const unsigned* hard, unsigned color_space,
                                             int* counts, unsigned disparity_steps) {
    return view_synth_probe(in_flat, mask, missing, out_flat, ang_major, awidth, aheight, an, width, height, chnls, vpi, vpf, hard, color_space,
                            counts, disparity_steps);
}

/* The same with view_synth_LF's occl_ratio; set_hist [5]: the positions per set chosen. */
extern "C" int lfbm5d_view_synth_occl_probe(const float* in_flat, const unsigned* mask, const unsigned* missing, float* out_flat,
                                            unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned width, unsigned height,
                                            unsigned chnls, const int* vpi, const float* vpf, const unsigned* hard, unsigned color_space,
                                            int* counts, unsigned disparity_steps, float occl_ratio, unsigned long long* set_hist) {
    return view_synth_probe(in_flat, mask, missing, out_flat, ang_major, awidth, aheight, an, width, height, chnls, vpi, vpf, hard, color_space,
                            counts, disparity_steps, occl_ratio, set_hist);
}

/* joint repair on the caller's vectors, in place for the caller (one pointer per SAI; the library stages in and out apart) */
int repair_LF(std::vector<std::vector<float> >& LF, const std::vector<std::vector<unsigned char> >& flags, const std::vector<unsigned>& LF_SAI_mask,
              const std::vector<unsigned>& missing, const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard,
              const unsigned width, const unsigned height, const unsigned chnls, const int maxDisparity, const int boxRadius, const int angRadius,
              const int minValid, const int iterations, const float sigmaStart, const float sigmaEnd, const float sigmaNoise,
              const float lambdaHard5D, const unsigned NHard, const unsigned nSim, const unsigned nDisp, const unsigned kHard,
              const unsigned pHard, const bool useSD, const unsigned tau_2D, unsigned tau_4D, const unsigned tau_5D, const unsigned color_space,
              unsigned long long counts[6], int& dmin, int& dmax) {
    const unsigned asize = awidth * aheight;
    lfbm5d_repair_result result;
    std::memset(&result, 0, sizeof(result));
    std::memset(counts, 0, 6 * sizeof(unsigned long long));
    dmin = dmax = 0;
    if (LF.size() != asize || LF_SAI_mask.size() != asize || (!flags.empty() && flags.size() != asize) || (!missing.empty() && missing.size() != asize)) {
        std::cout << "repair_LF: light field and mask must hold awidth*aheight SAIs, flags and missing that many or none" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_repair_params rp;
    lfbm5d_repair_defaults(&rp);
    if (maxDisparity >= 0) rp.max_disparity = (unsigned)maxDisparity;
    if (boxRadius >= 0) rp.box_radius = (unsigned)boxRadius;
    if (angRadius >= 0) rp.ang_radius = (unsigned)angRadius;
    if (minValid >= 0) rp.min_valid = (unsigned)minValid;
    if (iterations >= 0) rp.iterations = (unsigned)iterations;
    if (sigmaStart != 0.0f) rp.sigma_start = sigmaStart;
    if (sigmaEnd != 0.0f) rp.sigma_end = sigmaEnd;
    rp.sigma_noise = sigmaNoise;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<float*> p;
    std::vector<const unsigned char*> f;
    if (!sai_ptrs("repair_LF", LF, LF_SAI_mask, img, false, p, " and flags") || !sai_ptrs("repair_LF", flags, LF_SAI_mask, img, false, f, " and flags"))
        return EXIT_FAILURE;
    const lfbm5d_params P = make(0.0f, lambdaHard5D, {NHard, nSim, nDisp, kHard, pHard, useSD, tau_2D, tau_4D, tau_5D}, color_space);
    const int rc = lfbm5d_repair_host_sai(ctx, &rp, &P, p.data(), flags.empty() ? nullptr : f.data(), LF_SAI_mask.data(),
                                          missing.empty() ? nullptr : missing.data(), p.data(), nullptr, nullptr, ang_major, awidth, aheight, anHard,
                                          width, height, chnls, &result);
    counts[0] = result.values; counts[1] = result.flagged; counts[2] = result.missing;
    for (unsigned c = 0; c < 3; c++) { counts[3] += result.views[c]; counts[4] += result.rim[c]; counts[5] += result.left[c]; }
    bool any = false;
    for (int d = -8; d <= 8; d++)
        if (result.disparity_hist[d + 8]) { if (!any) dmin = d; dmax = d; any = true; }
    return rc != 0 ? report(ctx) : EXIT_SUCCESS;
}

/* Test hook: repair_LF on vector<vector<float>> light fields built from flat copies [asize][chnls*height*width] (flags_flat or NULL,
 * missing or NULL); the result goes to out_flat.  rpi = {maxDisparity, boxRadius, angRadius, minValid, iterations}, rpf = {sigmaStart,
 * sigmaEnd, sigmaNoise, lambda}, hard = {N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D}; counts [6] as repair_LF's;
 * range = {dmin, dmax}. */
extern "C" int lfbm5d_repair_probe(const float* in_flat, const unsigned char* flags_flat, const unsigned* mask, const unsigned* missing,
                                   float* out_flat, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned width,
                                   unsigned height, unsigned chnls, const int* rpi, const float* rpf, const unsigned* hard, unsigned color_space,
                                   unsigned long long* counts, int* range) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize), ms;
    if (missing) ms.assign(missing, missing + asize);
    std::vector<std::vector<float> > LF = from_flat(in_flat, m, img);
    std::vector<std::vector<unsigned char> > fl;
    if (flags_flat) fl = from_flat(flags_flat, m, img);
    unsigned long long r[6];
    int dmin = 0, dmax = 0;
    const int rc = repair_LF(LF, fl, m, ms, ang_major, awidth, aheight, an, width, height, chnls, rpi[0], rpi[1], rpi[2], rpi[3], rpi[4], rpf[0],
                             rpf[1], rpf[2], rpf[3], hard[0], hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8],
                             color_space, r, dmin, dmax);
    if (counts) std::memcpy(counts, r, sizeof(r));
    if (range) { range[0] = dmin; range[1] = dmax; }
    if (rc != EXIT_SUCCESS) return 1;
    to_flat(LF, m, img, out_flat);
    return 0;
}

int consist_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, const std::vector<unsigned>& exclude,
               const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned width, const unsigned height,
               const unsigned chnls, const int maxDisparity, const int boxRadius, const int angRadius, const int minSources, const int maxRounds,
               const double k, const double spread, const double saiFactor, std::vector<std::vector<unsigned char> >& flags,
               std::vector<unsigned>& state, unsigned long long& flagged, unsigned long long& nonfinite, unsigned& bad, unsigned& untested,
               unsigned& rounds, double scales[3], const unsigned disparity_steps) {
    const unsigned asize = awidth * aheight;
    lfbm5d_consist_result result;
    std::memset(&result, 0, sizeof(result));
    flagged = nonfinite = 0; bad = untested = rounds = 0;
    scales[0] = scales[1] = scales[2] = 0.0;
    if (LF.size() != asize || LF_SAI_mask.size() != asize || (!exclude.empty() && exclude.size() != asize)) {
        std::cout << "consist_LF: light field, mask and exclude must hold awidth*aheight SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_consist_params cp;
    lfbm5d_consist_defaults(&cp);
    if (maxDisparity >= 0) cp.max_disparity = (unsigned)maxDisparity;
    if (boxRadius >= 0) cp.box_radius = (unsigned)boxRadius;
    if (angRadius >= 0) cp.ang_radius = (unsigned)angRadius;
    if (minSources >= 0) cp.min_sources = (unsigned)minSources;
    if (maxRounds >= 0) cp.max_rounds = (unsigned)maxRounds;
    if (k >= 0.0) cp.k = k;
    if (spread >= 0.0) cp.spread = spread;
    if (saiFactor >= 0.0) cp.sai_factor = saiFactor;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<const float*> p;
    std::vector<unsigned char*> f;
    flags.assign(asize, std::vector<unsigned char>());
    state.assign(asize, 0u);
    if (!sai_ptrs("consist_LF", LF, LF_SAI_mask, img, false, p)) return EXIT_FAILURE;
    for (size_t st = 0; st < asize; st++) if (LF_SAI_mask[st]) flags[st].assign(img, 0);
    sai_ptrs("consist_LF", flags, LF_SAI_mask, img, false, f);
    const unsigned* ex = exclude.empty() ? nullptr : exclude.data();
    const int rc = disparity_steps == 1                                         /* the integer form: its name in the messages */
        ? lfbm5d_consist_host_sai(ctx, &cp, p.data(), LF_SAI_mask.data(), ex, f.data(), state.data(), nullptr, nullptr, nullptr, ang_major, awidth,
                                  aheight, width, height, chnls, &result)
        : lfbm5d_consist_steps_host_sai(ctx, &cp, disparity_steps, p.data(), LF_SAI_mask.data(), ex, f.data(), state.data(), nullptr, nullptr,
                                        nullptr, ang_major, awidth, aheight, width, height, chnls, &result);
    if (rc != 0) return report(ctx);
    for (unsigned c = 0; c < 3; c++) { flagged += result.flagged[c][0]; nonfinite += result.flagged[c][1]; scales[c] = result.scale_channel[c]; }
    bad = result.bad; untested = result.untested; rounds = result.rounds;
    return EXIT_SUCCESS;
}

/* Test hook: consist_LF on a vector<vector<float>> light field built from a flat copy [asize][chnls*height*width]; the flags go to
 * flags_flat (planes of empty SAIs untouched), the states to state_out.  cpi = {maxDisparity, boxRadius, angRadius, minSources, maxRounds},
 * cpd = {k, spread, saiFactor}; exclude may be NULL;
 * counts = {flagged, nonfinite, bad, untested, rounds}, scales [3]. */
static int consist_probe(const float* in_flat, const unsigned* mask, const unsigned* exclude, unsigned char* flags_flat, unsigned* state_out,
                         unsigned ang_major, unsigned awidth, unsigned aheight, unsigned width, unsigned height, unsigned chnls, const int* cpi,
                         const double* cpd, unsigned long long* counts, double* scales, unsigned disparity_steps) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize), ex, state;
    if (exclude) ex.assign(exclude, exclude + asize);
    const std::vector<std::vector<float> > LF = from_flat(in_flat, m, img);
    std::vector<std::vector<unsigned char> > fl;
    unsigned long long flagged = 0, nonfinite = 0; unsigned bad = 0, untested = 0, rounds = 0; double sc[3];
    if (consist_LF(LF, m, ex, ang_major, awidth, aheight, width, height, chnls, cpi[0], cpi[1], cpi[2], cpi[3], cpi[4], cpd[0], cpd[1], cpd[2], fl,
                   state, flagged, nonfinite, bad, untested, rounds, sc, disparity_steps) != EXIT_SUCCESS) return 1;
    std::copy(state.begin(), state.end(), state_out);
    to_flat(fl, m, img, flags_flat);
    if (counts) { counts[0] = flagged; counts[1] = nonfinite; counts[2] = bad; counts[3] = untested; counts[4] = rounds; }
    if (scales) { scales[0] = sc[0]; scales[1] = sc[1]; scales[2] = sc[2]; }
    return 0;
}

extern "C" int lfbm5d_consist_probe(const float* in_flat, const unsigned* mask, const unsigned* exclude, unsigned char* flags_flat,
                                    unsigned* state_out, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned width, unsigned height,
                                    unsigned chnls, const int* cpi, const double* cpd, unsigned long long* counts, double* scales) {
    return consist_probe(in_flat, mask, exclude, flags_flat, state_out, ang_major, awidth, aheight, width, height, chnls, cpi, cpd, counts, scales, 1);
}

/* The same with consist_LF's disparity_steps. */
extern "C" int lfbm5d_consist_steps_probe(const float* in_flat, const unsigned* mask, const unsigned* exclude, unsigned char* flags_flat,
                                          unsigned* state_out, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned width,
                                          unsigned height, unsigned chnls, const int* cpi, const double* cpd, unsigned long long* counts,
                                          double* scales, unsigned disparity_steps) {
    return consist_probe(in_flat, mask, exclude, flags_flat, state_out, ang_major, awidth, aheight, width, height, chnls, cpi, cpd, counts, scales,
                         disparity_steps);
}

/* photometric equalisation on the caller's vectors (one pointer per SAI; the library stages in and out) */
int equalise_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_out,
                const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned width, const unsigned height,
                const unsigned chnls, const int maxDisparity, const int boxRadius, const int angRadius, const int minSources, const int maxRounds,
                const int perChannel, const int anchor, const double tol, const double lo, const double hi, std::vector<double>& gains,
                std::vector<unsigned>& state, unsigned& fitted, unsigned& untested, unsigned& unfit, unsigned& rounds, double& residual,
                double& gainMin, double& gainMax, const unsigned disparity_steps) {
    const unsigned asize = awidth * aheight;
    lfbm5d_photo_result result;
    std::memset(&result, 0, sizeof(result));
    fitted = untested = unfit = rounds = 0;
    residual = 0.0; gainMin = gainMax = 1.0;
    if (LF.size() != asize || LF_SAI_mask.size() != asize) {
        std::cout << "equalise_LF: light field and mask must hold awidth*aheight SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_photo_params pp;
    lfbm5d_photo_defaults(&pp);
    if (maxDisparity >= 0) pp.max_disparity = (unsigned)maxDisparity;
    if (boxRadius >= 0) pp.box_radius = (unsigned)boxRadius;
    if (angRadius >= 0) pp.ang_radius = (unsigned)angRadius;
    if (minSources >= 0) pp.min_sources = (unsigned)minSources;
    if (maxRounds >= 0) pp.max_rounds = (unsigned)maxRounds;
    if (perChannel >= 0) pp.per_channel = (unsigned)perChannel;
    if (anchor >= 0) pp.anchor = (unsigned)anchor;
    if (tol >= 0.0) pp.tol = tol;
    if (lo >= 0.0) pp.lo = lo;
    if (hi >= 0.0) pp.hi = hi;
    pp.steps = disparity_steps;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    const size_t img = (size_t)width * height * chnls;
    std::vector<const float*> p;
    std::vector<float*> o;
    if (!sai_ptrs("equalise_LF", LF, LF_SAI_mask, img, false, p)) return EXIT_FAILURE;
    if (&LF_out != &LF) LF_out = LF;
    sai_ptrs("equalise_LF", LF_out, LF_SAI_mask, img, false, o);
    gains.assign((size_t)asize * 3, 1.0);
    state.assign(asize, 0u);
    if (lfbm5d_photo_host_sai(ctx, &pp, p.data(), LF_SAI_mask.data(), o.data(), gains.data(), state.data(), nullptr, ang_major, awidth, aheight,
                              width, height, chnls, &result) != 0) return report(ctx);
    fitted = result.fitted; untested = result.untested; unfit = result.unfit; rounds = result.rounds;
    residual = result.residual; gainMin = result.gain_min; gainMax = result.gain_max;
    return EXIT_SUCCESS;
}

int apply_gains_LF(std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, const std::vector<double>& gains,
                   const bool invert, const unsigned awidth, const unsigned aheight, const unsigned width, const unsigned height,
                   const unsigned chnls) {
    const unsigned asize = awidth * aheight;
    const size_t img = (size_t)width * height * chnls;
    if (LF.size() != asize || LF_SAI_mask.size() != asize || gains.size() != (size_t)asize * 3) {
        std::cout << "apply_gains_LF: light field and mask must hold awidth*aheight SAIs, gains 3 values per SAI" << std::endl;
        return EXIT_FAILURE;
    }
    std::vector<float*> p;
    if (!sai_ptrs("apply_gains_LF", LF, LF_SAI_mask, img, false, p)) return EXIT_FAILURE;
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    if (lfbm5d_photo_apply_host_sai(ctx, p.data(), LF_SAI_mask.data(), gains.data(), invert ? 1u : 0u, p.data(), awidth, aheight, width, height,
                                    chnls) != 0) return report(ctx);
    return EXIT_SUCCESS;
}

/* Test hook: equalise_LF, then (apply = 1) apply_gains_LF with invert on its output, on a vector<vector<float>> light field built from a
 * flat copy [asize][chnls*height*width]; the result goes to out_flat (planes of empty SAIs untouched).  ppi = {maxDisparity, boxRadius,
 * angRadius, minSources, maxRounds, perChannel, anchor, disparity_steps}, ppd = {tol, lo, hi}; gains [asize][3], state [asize],
 * counts = {fitted, untested, unfit, rounds}, figures = {residual, gainMin, gainMax}. */
extern "C" int lfbm5d_equalise_probe(const float* in_flat, const unsigned* mask, float* out_flat, unsigned ang_major, unsigned awidth,
                                     unsigned aheight, unsigned width, unsigned height, unsigned chnls, const int* ppi, const double* ppd,
                                     double* gains_out, unsigned* state_out, unsigned* counts, double* figures, int apply) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize), state;
    const std::vector<std::vector<float> > LF = from_flat(in_flat, m, img);
    std::vector<std::vector<float> > out;
    std::vector<double> gains;
    if (equalise_LF(LF, m, out, ang_major, awidth, aheight, width, height, chnls, ppi[0], ppi[1], ppi[2], ppi[3], ppi[4], ppi[5], ppi[6], ppd[0],
                    ppd[1], ppd[2], gains, state, counts[0], counts[1], counts[2], counts[3], figures[0], figures[1], figures[2],
                    (unsigned)ppi[7]) != EXIT_SUCCESS) return 1;
    if (apply && apply_gains_LF(out, m, gains, true, awidth, aheight, width, height, chnls) != EXIT_SUCCESS) return 1;
    std::copy(state.begin(), state.end(), state_out);
    to_flat(out, m, img, out_flat);
    std::memcpy(gains_out, gains.data(), asize * 3 * sizeof(double));
    return 0;
}

/* run_bm5d with a view table (include/lfbm5d_views.h): the caller's vectors, one pointer per SAI */
int denoise_views_LF(std::vector<double>& sigma_sai, std::vector<float>& window_sigmas, const float lambdaHard5D,
                     std::vector<std::vector<float> >& LF_noisy, std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_basic,
                     std::vector<std::vector<float> >& LF_denoised, const unsigned ang_major, const unsigned awidth, const unsigned aheight,
                     const unsigned anHard, const unsigned anWien, const unsigned width, const unsigned height, const unsigned chnls,
                     const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard,
                     const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard, const unsigned NWien,
                     const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien, const bool useSDWien,
                     const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien, const unsigned color_space,
                     const unsigned nb_threads) {
    Job<LF> j;
    if (!j.open("denoise_views_LF", "light field, mask and view table must hold awidth*aheight SAIs", sigma_sai.empty() || sigma_sai.size() == awidth * aheight,
                LF_noisy, LF_SAI_mask, LF_basic, true, &LF_denoised, awidth, aheight, width, height, chnls, 0.0f, lambdaHard5D,
                {NHard, nSimHard, nDispHard, kHard, pHard, useSDHard, tau_2D_hard, tau_4D_hard, tau_5D_hard},
                {NWien, nSimWien, nDispWien, kWien, pWien, useSDWien, tau_2D_wien, tau_4D_wien, tau_5D_wien}, color_space, nb_threads)) return EXIT_FAILURE;
    std::vector<double> used(awidth * aheight, 0.0);
    if (lfbm5d_denoise_views_host_sai(j.ctx, sigma_sai.empty() ? nullptr : sigma_sai.data(), used.data(), &j.P1, &j.P2, j.noisy.data(), LF_SAI_mask.data(),
                                      j.basic.data(), j.den.data(), ang_major, awidth, aheight, anHard, anWien, width, height, chnls) != 0) return report(j.ctx);
    sigma_sai = used;
    const int n = lfbm5d_last_window_sigmas(j.ctx, nullptr, 0);
    window_sigmas.assign((size_t)std::max(n, 0), 0.0f);
    if (n > 0) lfbm5d_last_window_sigmas(j.ctx, window_sigmas.data(), (unsigned)n);
    return EXIT_SUCCESS;
}

/* run_bm5d under spatially correlated noise (include/lfbm5d_corr.h): the caller's vectors, one pointer per SAI */
int denoise_corr_LF(const std::vector<double>& acf, const float sigma, const float lambdaHard5D, std::vector<std::vector<float> >& LF_noisy,
                    std::vector<unsigned>& LF_SAI_mask, std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised,
                    const unsigned ang_major, const unsigned awidth, const unsigned aheight, const unsigned anHard, const unsigned anWien,
                    const unsigned width, const unsigned height, const unsigned chnls, const unsigned NHard, const unsigned nSimHard,
                    const unsigned nDispHard, const unsigned kHard, const unsigned pHard, const bool useSDHard, const unsigned tau_2D_hard,
                    unsigned tau_4D_hard, const unsigned tau_5D_hard, const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien,
                    const unsigned kWien, const unsigned pWien, const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien,
                    const unsigned tau_5D_wien, const unsigned color_space, const unsigned nb_threads) {
    Job<LF> j;
    if (!j.open("denoise_corr_LF", "light field and mask must hold awidth*aheight SAIs, the autocorrelation 49 values", acf.size() == 49, LF_noisy,
                LF_SAI_mask, LF_basic, true, &LF_denoised, awidth, aheight, width, height, chnls, sigma, lambdaHard5D,
                {NHard, nSimHard, nDispHard, kHard, pHard, useSDHard, tau_2D_hard, tau_4D_hard, tau_5D_hard},
                {NWien, nSimWien, nDispWien, kWien, pWien, useSDWien, tau_2D_wien, tau_4D_wien, tau_5D_wien}, color_space, nb_threads)) return EXIT_FAILURE;
    if (lfbm5d_denoise_corr_host_sai(j.ctx, acf.data(), &j.P1, &j.P2, j.noisy.data(), LF_SAI_mask.data(), j.basic.data(), j.den.data(), ang_major,
                                     awidth, aheight, anHard, anWien, width, height, chnls) != 0) return report(j.ctx);
    return EXIT_SUCCESS;
}

int corr_measure_LF(const std::vector<std::vector<float> >& LF, const std::vector<unsigned>& LF_SAI_mask, const unsigned width,
                    const unsigned height, const unsigned chnls, const unsigned block, const double fraction, std::vector<double>& acf,
                    double& sigma) {
    std::vector<const float*> p;
    lfbm5d_ctx* ctx = open_stage("corr_measure_LF", LF, LF_SAI_mask, width, height, chnls, p);
    if (!ctx) return EXIT_FAILURE;
    lfbm5d_corr_estimate r;
    if (lfbm5d_corr_measure_host_sai(ctx, p.data(), LF_SAI_mask.data(), (unsigned)LF.size(), width, height, chnls, block, fraction, &r) != 0) return report(ctx);
    acf.assign(r.acf, r.acf + 49);
    sigma = r.sigma;
    return EXIT_SUCCESS;
}

int views_from_gains(const double sigma, const std::vector<double>& gains, const unsigned chnls, const std::vector<unsigned>& LF_SAI_mask,
                     std::vector<double>& sigma_sai) {
    const size_t asize = LF_SAI_mask.size();
    if (gains.size() != 3 * asize || chnls < 1 || chnls > 3) {
        std::cout << "views_from_gains: gains must hold 3 values per SAI of the mask, chnls 1..3" << std::endl;
        return EXIT_FAILURE;
    }
    std::vector<float> g(asize * chnls);
    for (size_t st = 0; st < asize; st++) for (unsigned c = 0; c < chnls; c++) g[st * chnls + c] = (float)gains[3 * st + c];
    sigma_sai.assign(asize, 0.0);
    if (lfbm5d_views_from_gains(sigma, g.data(), chnls, LF_SAI_mask.data(), (unsigned)asize, sigma_sai.data()) != 0) {
        std::cout << lfbm5d_views_error() << std::endl;
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

/* Test hook: denoise_views_LF on a vector<vector<float>> light field built from a flat copy [asize][chnls*height*width].  table [asize]
 * or NULL (the estimate); used_out [asize]; hard / wien = {N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D}; win_out [win_cap] receives
 * the window sigmas, *n_win their count.  The light fields are copied to the non-NULL flat outputs. */
extern "C" int lfbm5d_denoise_views_probe(const float* noisy_flat, const unsigned* mask, const double* table, double* used_out, float* noisy_out,
                                          float* basic_out, float* denoised_out, unsigned ang_major, unsigned awidth, unsigned aheight,
                                          unsigned anHard, unsigned anWien, unsigned width, unsigned height, unsigned chnls, float lambda,
                                          const unsigned* hard, const unsigned* wien, unsigned color_space, float* win_out, unsigned win_cap,
                                          unsigned* n_win) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize);
    std::vector<std::vector<float> > LF_noisy = from_flat(noisy_flat, m, img), LF_basic, LF_denoised;
    std::vector<double> t;
    if (table) t.assign(table, table + asize);
    std::vector<float> ws;
    if (denoise_views_LF(t, ws, lambda, LF_noisy, m, LF_basic, LF_denoised, ang_major, awidth, aheight, anHard, anWien, width, height, chnls,
                         hard[0], hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8],
                         wien[0], wien[1], wien[2], wien[3], wien[4], wien[5] != 0, wien[6], wien[7], wien[8], color_space, 1) != EXIT_SUCCESS) return 1;
    if (used_out) std::copy(t.begin(), t.end(), used_out);
    to_flat(LF_noisy, m, img, noisy_out);
    to_flat(LF_basic, m, img, basic_out);
    to_flat(LF_denoised, m, img, denoised_out);
    if (n_win) *n_win = (unsigned)ws.size();
    for (size_t i = 0; i < ws.size() && i < win_cap && win_out; i++) win_out[i] = ws[i];
    return 0;
}

/* both steps' parameters from run_bm3d_LF's argument list */
static void bm3d_pair(float sigma, float lambda3D, unsigned nHard, unsigned nWien, unsigned kHard, unsigned kWien, unsigned NHard, unsigned NWien,
                      unsigned pHard, unsigned pWien, bool useSD_h, bool useSD_w, unsigned tau_2D_hard, unsigned tau_2D_wien, unsigned color_space,
                      lfbm5d_bm3d_params& Hd, lfbm5d_bm3d_params& Wn) {
    Hd.sigma = sigma; Hd.lambda3D = lambda3D; Hd.N = NHard; Hd.nHW = nHard; Hd.k = kHard; Hd.p = pHard;
    Hd.useSD = useSD_h ? 1u : 0u; Hd.tau_2D = tau_2D_hard; Hd.color_space = color_space;
    Wn = Hd; Wn.N = NWien; Wn.nHW = nWien; Wn.k = kWien; Wn.p = pWien; Wn.useSD = useSD_w ? 1u : 0u; Wn.tau_2D = tau_2D_wien;
}

/* run_bm3d_LF (src/bm3d_LF.h:10-35, bm3d_LF.cpp:75-125): BM3D on every SAI of the mask */
#include "run_bm3d_lf.h"
int run_bm3d_LF(const float sigma, std::vector<std::vector<float> >& LF_noisy, std::vector<unsigned>& LF_SAI_mask,
                std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised,
                const unsigned width, const unsigned height, const unsigned chnls, const unsigned nHard, const unsigned nWien,
                const unsigned kHard, const unsigned kWien, const unsigned NHard, const unsigned NWien, const unsigned pHard,
                const unsigned pWien, const bool useSD_h, const bool useSD_w, const unsigned tau_2D_hard,
                const unsigned tau_2D_wien, const float lambdaHard3D, const unsigned color_space, unsigned /*nb_threads*/,
                char* sub_img_name) {
    const size_t asize = LF_noisy.size();
    if (LF_SAI_mask.size() != asize) {
        std::cout << "run_bm3d_LF: light field and mask must hold the same number of SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    size_sais(LF_basic, asize);
    size_sais(LF_denoised, asize);
    const size_t img = (size_t)width * height * chnls;
    Flat noisy, basic = flat_alloc(asize * img), den = flat_alloc(asize * img);
    flatten(LF_noisy, LF_SAI_mask, img, noisy);
    lfbm5d_bm3d_params Hd, Wn;
    bm3d_pair(sigma, lambdaHard3D, nHard, nWien, kHard, kWien, NHard, NWien, pHard, pWien, useSD_h, useSD_w, tau_2D_hard, tau_2D_wien, color_space, Hd, Wn);
    std::cout << " - > Running BM3D filter on every " << (sub_img_name ? sub_img_name : "SAI") << " (GPU)" << std::endl;
    if (lfbm5d_bm3d_lf_host(ctx, &Hd, &Wn, noisy.get(), LF_SAI_mask.data(), basic.get(), den.get(), (unsigned)asize, width,
                            height, chnls) != 0) return report(ctx);
    unflatten(LF_noisy, LF_SAI_mask, img, noisy);
    unflatten(LF_basic, LF_SAI_mask, img, basic);
    unflatten(LF_denoised, LF_SAI_mask, img, den);
    return EXIT_SUCCESS;
}

/* run_bm3d_LF with a view table: the device form on buffers staged here (the library has no host form of it) */
int bm3d_views_LF(std::vector<double>& sigma_sai, std::vector<std::vector<float> >& LF_noisy, std::vector<unsigned>& LF_SAI_mask,
                  std::vector<std::vector<float> >& LF_basic, std::vector<std::vector<float> >& LF_denoised, const unsigned width,
                  const unsigned height, const unsigned chnls, const unsigned nHard, const unsigned nWien, const unsigned kHard,
                  const unsigned kWien, const unsigned NHard, const unsigned NWien, const unsigned pHard, const unsigned pWien,
                  const bool useSD_h, const bool useSD_w, const unsigned tau_2D_hard, const unsigned tau_2D_wien, const float lambdaHard3D,
                  const unsigned color_space) {
    const size_t asize = LF_noisy.size();
    if (LF_SAI_mask.size() != asize || (!sigma_sai.empty() && sigma_sai.size() != asize)) {
        std::cout << "bm3d_views_LF: light field, mask and view table must hold the same number of SAIs" << std::endl;
        return EXIT_FAILURE;
    }
    lfbm5d_ctx* ctx = context();
    if (!ctx) return EXIT_FAILURE;
    size_sais(LF_basic, asize);
    size_sais(LF_denoised, asize);
    lfbm5d_bm3d_params Hd, Wn;
    bm3d_pair(0.0f, lambdaHard3D, nHard, nWien, kHard, kWien, NHard, NWien, pHard, pWien, useSD_h, useSD_w, tau_2D_hard, tau_2D_wien, color_space, Hd, Wn);
    return device_round_trip("bm3d_views_LF", kBm3dWords, ctx, {&LF_noisy, &LF_basic, &LF_denoised}, LF_SAI_mask, (size_t)width * height * chnls,
                             [&](const std::vector<Dev>& d) {
        std::vector<double> used(asize, 0.0);
        std::cout << " - > Running BM3D filter on every SAI with its own sigma (GPU)" << std::endl;
        const int rc = lfbm5d_bm3d_lf_views_device(ctx, sigma_sai.empty() ? nullptr : sigma_sai.data(), used.data(), &Hd, &Wn, (float*)d[0].p,
                                                   LF_SAI_mask.data(), (float*)d[1].p, (float*)d[2].p, (unsigned)asize, width, height, chnls);
        if (rc == 0) sigma_sai = used;
        return rc;
    });
}

/* Measurement hook (bench.py `seam.dropin_vectors`, tests): the interval the reference times -- main.cpp:189-201 around
 * run_bm5d_1st_step plus :241-247 around run_bm5d_2nd_step -- through THIS file's functions on vector<vector<float>> light fields
 * built from a flat copy, output vectors sized beforehand like main.cpp:158-165 does.  mode 0: the two calls, 1: run_bm5d (one job).
 * hard / wien = {N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D}.  ms_out[2 * rep + {0, 1}] = the two intervals (mode 1: the job,
 * 0).  The last repetition's light fields are copied to the non-NULL flat outputs. */
extern "C" int lfbm5d_dropin_probe(int mode, const float* noisy_flat, const unsigned* mask, float* noisy_out, float* basic_out,
                                   float* denoised_out, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned anHard,
                                   unsigned anWien, unsigned width, unsigned height, unsigned chnls, float sigma, float lambda,
                                   const unsigned* hard, const unsigned* wien, unsigned color_space, int reps, double* ms_out) {
    const size_t asize = (size_t)awidth * aheight, img = (size_t)width * height * chnls;
    std::vector<unsigned> m(mask, mask + asize);
    std::vector<std::vector<float> > LF_noisy(asize), LF_basic(asize), LF_denoised(asize);
    for_sais(asize, [&](size_t st) { LF_noisy[st].resize(img, 0.0f); LF_basic[st].resize(img, 0.0f); LF_denoised[st].resize(img, 0.0f); });
    typedef std::chrono::steady_clock clk;
    for (int r = 0; r < reps; r++) {
        for_sais(asize, [&](size_t st) { std::memcpy(LF_noisy[st].data(), noisy_flat + st * img, img * sizeof(float)); });
        const clk::time_point t0 = clk::now();
        clk::time_point t1 = t0, t2 = t0;
        if (mode == 1) {
            if (run_bm5d(sigma, lambda, LF_noisy, m, LF_basic, LF_denoised, ang_major, awidth, aheight, anHard, anWien, width, height, chnls,
                         hard[0], hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8],
                         wien[0], wien[1], wien[2], wien[3], wien[4], wien[5] != 0, wien[6], wien[7], wien[8], color_space, 1) != EXIT_SUCCESS) return 1;
            t1 = t2 = clk::now();
        } else {
            if (run_bm5d_1st_step(sigma, lambda, LF_noisy, m, LF_basic, ang_major, awidth, aheight, anHard, width, height, chnls, hard[0], hard[1],
                                  hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], color_space, 1) != EXIT_SUCCESS) return 1;
            t1 = clk::now();
            if (run_bm5d_2nd_step(sigma, LF_noisy, m, LF_basic, LF_denoised, ang_major, awidth, aheight, anWien, width, height, chnls, wien[0],
                                  wien[1], wien[2], wien[3], wien[4], wien[5] != 0, wien[6], wien[7], wien[8], color_space, 1) != EXIT_SUCCESS) return 1;
            t2 = clk::now();
        }
        if (ms_out) {
            ms_out[2 * r] = std::chrono::duration<double, std::milli>(t1 - t0).count();
            ms_out[2 * r + 1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
        }
    }
    for_sais(asize, [&](size_t st) {
        if (!m[st]) return;
        if (noisy_out) std::memcpy(noisy_out + st * img, LF_noisy[st].data(), img * sizeof(float));
        if (basic_out) std::memcpy(basic_out + st * img, LF_basic[st].data(), img * sizeof(float));
        if (denoised_out) std::memcpy(denoised_out + st * img, LF_denoised[st].data(), img * sizeof(float));
    });
    return 0;
}
