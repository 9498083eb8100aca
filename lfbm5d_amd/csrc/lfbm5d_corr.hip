/*
 * lfbm5d_corr.hip -- spatially correlated noise (include/lfbm5d_corr.h; the autocorrelation and its variance table on the host are in
 * lfbm5d_corr_host.hip): the block autocovariance measured on the GPU (k_corr_blocks, k_corr_pool), the general group kernels in their variance-table form
 * (k_group_corr, k_group_big_corr: group_generic<.., CORR> of lfbm5d_group_generic.h) and the jobs that run with a table.  A job
 * places its tables in the context, group_args_of_pass / launch_group pick them up, and they are gone when the entry point returns.
 */
#include "lfbm5d_side.h"
#include "lfbm5d_group_generic.h"

using namespace lfbm5d_host;

namespace lfbm5d {

namespace {

/* ------------------------------------------------------------------------------------------
 * The general group kernels with a variance table: k_group / k_group_big of lfbm5d_group_generic.hip, the table a kernel argument
 * of its own (GroupArgs is as it was).
 * ------------------------------------------------------------------------------------------ */
template <int STEP>
__global__ __launch_bounds__(kThreads) void k_group_corr(GroupArgs a, const float* tab) {
    extern __shared__ float lds[];
    __shared__ unsigned pos[kMaxN3 * kMaxA];
    __shared__ float red[3][kThreads / 64];
    const unsigned g = a.ref_begin + blockIdx.x;
    const int stack = (int)a.self_cnt[g] * (int)a.A * (int)(a.k * a.k);
    group_generic<STEP, false, true>(a, g, (int)blockIdx.y, lds, STEP == 2 ? lds + stack : nullptr, lds + (STEP == 2 ? 2 : 1) * stack, pos, red, tab);
}

template <int STEP, bool BIG>
__global__ __launch_bounds__(kThreads) void k_group_big_corr(GroupArgs a, float* scratch, unsigned long long slice_floats, unsigned tmp_floats,
                                                             const float* tab) {
    extern __shared__ float lds[];
    __shared__ unsigned pos_small[BIG ? 1 : kMaxN3 * kMaxA];
    __shared__ float red[3][kThreads / 64];
    unsigned* pos = BIG ? reinterpret_cast<unsigned*>(lds + tmp_floats) : pos_small;   /* BIG: N x A positions behind the 2-D work area */
    float* S0 = scratch + (size_t)blockIdx.x * slice_floats;
    const unsigned items = a.n_groups * a.C;
    for (unsigned it = blockIdx.x; it < items; it += gridDim.x) {
        const unsigned g = a.ref_begin + it / a.C;
        const int stack = (int)a.self_cnt[g] * (int)a.A * (int)(a.k * a.k);
        group_generic<STEP, BIG, true>(a, g, (int)(it % a.C), S0, STEP == 2 ? S0 + stack : nullptr, lds, pos, red, tab);
        __syncthreads();   /* pos / red / the scratch slice are reused by the next item */
    }
}

/* ------------------------------------------------------------------------------------------
 * The measurement.  One wave per B x B block, four blocks per workgroup; the block sits in LDS as doubles with an odd row stride
 * (lanes on consecutive rows read different banks).  Every sum is a chain of double adds and multiplies in the order the header states,
 * compiled with contraction off (a product and the add behind it round one after the other, as the numpy model's do): no fused
 * multiply-add, no atomics, nothing that depends on the launch shape.
 * ------------------------------------------------------------------------------------------ */
constexpr int kCorrLags = 25;      /* dy = 0: dx = 0..3; dy = 1..3: dx = -3..3 */
constexpr int kCorrChunk = 256;    /* blocks per chunk of the pooled sums */

__host__ __device__ inline void corr_lag(int l, int& dy, int& dx) {
    if (l < 4) { dy = 0; dx = l; } else { dy = 1 + (l - 4) / 7; dx = (l - 4) % 7 - 3; }
}

template <int B>
__global__ __launch_bounds__(256) void k_corr_blocks(const float* lf, const unsigned* sai, unsigned C, unsigned W, unsigned H, unsigned bw,
                                                     unsigned bh, unsigned long long n_blocks, double* lags, double* score) {
#pragma clang fp contract(off)
    constexpr int P = B + 1;
    __shared__ double d_all[4][B * P];
    __shared__ double part_all[4][kCorrLags][B];
    __shared__ double rsum_all[4][B];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long blk = (unsigned long long)blockIdx.x * 4 + wave;
    const bool active = blk < n_blocks;      /* (an idle wave of the last workgroup still meets every barrier) */
    double* d = d_all[wave];
    double (*part)[B] = part_all[wave];
    double* rsum = rsum_all[wave];
    if (active) {
        const unsigned long long per = (unsigned long long)bw * bh, pl = blk / per, r = blk % per;
        const unsigned by = (unsigned)(r / bw), bx = (unsigned)(r % bw);
        const unsigned st = sai[pl / C], ch = (unsigned)(pl % C);
        const float* base = lf + ((size_t)st * C + ch) * W * H + (size_t)by * B * W + (size_t)bx * B;
        for (int e = lane; e < B * B; e += 64) d[(e / B) * P + e % B] = (double)base[(size_t)(e / B) * W + e % B];
    }
    __syncthreads();
    if (active && lane < B) {
        double s = 0.0;
        for (int x = 0; x < B; x++) s = s + d[lane * P + x];
        rsum[lane] = s;
    }
    __syncthreads();
    if (active) {
        double s = 0.0;
        for (int y = 0; y < B; y++) s = s + rsum[y];
        const double m = s / (double)(B * B);
        for (int e = lane; e < B * B; e += 64) d[(e / B) * P + e % B] = d[(e / B) * P + e % B] - m;
    }
    __syncthreads();
    if (active) {
        for (int t = lane; t < kCorrLags * B; t += 64) {
            const int l = t / B, y = t % B;
            int dy, dx;
            corr_lag(l, dy, dx);
            if (y >= B - dy) continue;
            const int x0 = dx < 0 ? -dx : 0, x1 = dx > 0 ? B - dx : B;
            double p = 0.0;
            for (int x = x0; x < x1; x++) { const double q = d[y * P + x] * d[(y + dy) * P + x + dx]; p = p + q; }
            part[l][y] = p;
        }
    }
    __syncthreads();
    if (active && lane < kCorrLags) {
        int dy, dx;
        corr_lag(lane, dy, dx);
        double a = 0.0;
        for (int y = 0; y < B - dy; y++) a = a + part[lane][y];
        lags[blk * kCorrLags + lane] = a;
        if (lane == 0) score[blk] = a;
    }
}

/* 32 threads per chunk of kCorrChunk blocks: thread l < 25 sums lag l of the chunk's selected blocks in block order, thread 25 counts them */
__global__ __launch_bounds__(256) void k_corr_pool(const double* lags, const double* score, unsigned long long n_blocks, unsigned n_chunks,
                                                   double cut, double* part, unsigned* cnt) {
    const unsigned t = blockIdx.x * 256 + threadIdx.x, chunk = t / 32, l = t % 32;
    if (chunk >= n_chunks || l > (unsigned)kCorrLags) return;
    const unsigned long long b0 = (unsigned long long)chunk * kCorrChunk, b1 = b0 + kCorrChunk < n_blocks ? b0 + kCorrChunk : n_blocks;
    if (l < (unsigned)kCorrLags) {
        double acc = 0.0;
        for (unsigned long long b = b0; b < b1; b++)
            if (score[b] <= cut) acc = acc + lags[b * kCorrLags + l];
        part[(size_t)chunk * kCorrLags + l] = acc;
    } else {
        unsigned n = 0;
        for (unsigned long long b = b0; b < b1; b++) n += score[b] <= cut ? 1u : 0u;
        cnt[chunk] = n;
    }
}

} /* namespace */

hipError_t prepare_group_corr() {
    const void* fns[] = {reinterpret_cast<const void*>(&k_group_corr<1>), reinterpret_cast<const void*>(&k_group_corr<2>)};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kGenericLdsLimit);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

/* launch_group's tail for a pass with a variance table: the dispatch of the general kernels (lfbm5d_group_generic.hip), table forms */
hipError_t launch_group_corr(hipStream_t s, const GroupArgs& a, const float* tab, std::string* trace) {
    const bool bigA = a.A > (unsigned)kMaxA;
    const size_t lds = group_lds_bytes(a);
    if (lds > (size_t)kGenericLdsLimit || bigA) {   /* stacks in HBM scratch slices, persistent workgroups */
        const unsigned long long slice = (unsigned long long)(a.step == 2 ? 2 : 1) * a.N * a.A * a.k * a.k;
        if (!a.scratch || a.scratch_floats < slice * kBigBlocks) return hipErrorInvalidValue;
        const unsigned blocks = std::min<unsigned>(kBigBlocks, a.n_groups * a.C);
        const unsigned tf = (unsigned)group_tmp_floats(a);
        const size_t ltmp = (size_t)tf * sizeof(float) + (bigA ? (size_t)a.N * a.A * sizeof(unsigned) : 0);
        if (bigA) {
            if (a.step == 2) LFBM5D_LAUNCH(trace, (k_group_big_corr<2, true>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf, tab);
            else             LFBM5D_LAUNCH(trace, (k_group_big_corr<1, true>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf, tab);
        }
        else if (a.step == 2) LFBM5D_LAUNCH(trace, (k_group_big_corr<2, false>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf, tab);
        else                  LFBM5D_LAUNCH(trace, (k_group_big_corr<1, false>), dim3(blocks), dim3(kThreads), ltmp, s, a, a.scratch, slice, tf, tab);
        return hipGetLastError();
    }
    if (a.step == 2) LFBM5D_LAUNCH(trace, k_group_corr<2>, dim3(a.n_groups, a.C), dim3(kThreads), lds, s, a, tab);
    else             LFBM5D_LAUNCH(trace, k_group_corr<1>, dim3(a.n_groups, a.C), dim3(kThreads), lds, s, a, tab);
    return hipGetLastError();
}

} /* namespace lfbm5d */

namespace {

constexpr int L = LFBM5D_CORR_LAGS, LH = LFBM5D_CORR_LAGS / 2;

int corr_measure(lfbm5d_ctx* c, const float* d_lf, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                 unsigned C, unsigned block, double fraction, lfbm5d_corr_estimate* out) {
    (void)hipSetDevice(c->device);
    const std::string who = h_lf ? "lfbm5d_corr_measure_host_sai: " : "lfbm5d_corr_measure_device: ";
    if (!h_mask || !out || (!d_lf && !h_lf)) return fail(c, who + "NULL pointer for a required buffer");
    const unsigned B = block ? block : 16;
    if (check_chnls(c, who, C)) return 1;
    if (B != 8 && B != 16 && B != 32) return fail(c, who + "block must be 8, 16 or 32 (0 = 16)");
    if (check_size(c, who, W, H, B, "be at least the block size")) return 1;
    if (fraction == 0.0) fraction = LFBM5D_CORR_DEFAULT_FRACTION;
    if (!(fraction > 0.0 && fraction <= 1.0)) return fail(c, who + "fraction must be in (0, 1] (0 = the default)");
    if (check_one_gpu(c, who, "the correlated-noise routines run on one GPU (this context has a communicator or a shard)")) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    const unsigned nne = (unsigned)c->side.sai_host.size(), bw = W / B, bh = H / B;
    const unsigned long long n_blocks = (unsigned long long)nne * C * bw * bh;
    if ((unsigned long long)W * H > 0x7fffffffull || n_blocks > (1ull << 28)) return fail(c, who + "light field too large");
    const unsigned n_chunks = (unsigned)((n_blocks + kCorrChunk - 1) / kCorrChunk);
    const size_t img = (size_t)C * W * H;
    lfbm5d_ctx::CorrBufs& Bf = c->corrm;
    HIPCK(c, Bf.lags.reserve((size_t)n_blocks * kCorrLags * sizeof(double)));
    HIPCK(c, Bf.score.reserve((size_t)n_blocks * sizeof(double)));
    HIPCK(c, Bf.part.reserve((size_t)n_chunks * (kCorrLags * sizeof(double) + sizeof(unsigned))));
    const float* lf = d_lf;
    if (h_lf) {   /* stage the non-empty SAIs through HBM, at their places in [asize][C*H*W] */
        HIPCK(c, c->h2d_noisy.reserve((size_t)asize * img * sizeof(float)));
        if (upload_planes(c, who, h_lf, c->h2d_noisy.as<float>(), asize, img, [&](unsigned st) { return h_mask[st] != 0; })) return 1;
        lf = c->h2d_noisy.as<float>();
    }
    const unsigned* ds = c->side.sai.as<unsigned>();
    double *lags = Bf.lags.as<double>(), *score = Bf.score.as<double>(), *part = Bf.part.as<double>();
    unsigned* cnt = reinterpret_cast<unsigned*>(part + (size_t)n_chunks * kCorrLags);
    const dim3 grid((unsigned)((n_blocks + 3) / 4));
    switch (B) {
        case 8:  hipLaunchKernelGGL(k_corr_blocks<8>, grid, dim3(256), 0, c->stream, lf, ds, C, W, H, bw, bh, n_blocks, lags, score); break;
        case 16: hipLaunchKernelGGL(k_corr_blocks<16>, grid, dim3(256), 0, c->stream, lf, ds, C, W, H, bw, bh, n_blocks, lags, score); break;
        default: hipLaunchKernelGGL(k_corr_blocks<32>, grid, dim3(256), 0, c->stream, lf, ds, C, W, H, bw, bh, n_blocks, lags, score); break;
    }
    HIPCK(c, hipGetLastError());
    std::vector<double> sc((size_t)n_blocks);
    HIPCK(c, hipMemcpyAsync(sc.data(), score, sc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (double v : sc) if (!std::isfinite(v)) return fail(c, who + "the light field holds values that are not finite");
    /* exact selection: the kth smallest score is the cut, ties at the cut are selected */
    const double want = std::ceil(fraction * (double)n_blocks);
    const unsigned long long kth = want < 1.0 ? 1ull : std::min<unsigned long long>(n_blocks, (unsigned long long)want);
    std::nth_element(sc.begin(), sc.begin() + (size_t)(kth - 1), sc.end());
    const double cut = sc[(size_t)(kth - 1)];
    hipLaunchKernelGGL(k_corr_pool, dim3((n_chunks * 32 + 255) / 256), dim3(256), 0, c->stream, lags, score, n_blocks, n_chunks, cut, part, cnt);
    HIPCK(c, hipGetLastError());
    std::vector<double> hp((size_t)n_chunks * kCorrLags);
    std::vector<unsigned> hc(n_chunks);
    HIPCK(c, hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(hc.data(), cnt, hc.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    double S[kCorrLags];
    unsigned long long n_sel = 0;
    for (int l = 0; l < kCorrLags; l++) S[l] = 0.0;
    for (unsigned ch = 0; ch < n_chunks; ch++) {
        for (int l = 0; l < kCorrLags; l++) S[l] += hp[(size_t)ch * kCorrLags + l];
        n_sel += hc[ch];
    }
    std::memset(out, 0, sizeof(*out));
    out->blocks = n_blocks; out->selected = n_sel; out->cut = cut; out->block = B;
    const double C0 = S[0] / ((double)n_sel * (double)B * (double)B);
    for (int i = 0; i < L * L; i++) out->acf[i] = 0.0;
    out->acf[LH * L + LH] = 1.0;
    if (!(C0 > 0.0)) { out->sigma = 0.0; return 0; }   /* a constant light field: white, level 0 */
    for (int l = 1; l < kCorrLags; l++) {
        int dy, dx;
        corr_lag(l, dy, dx);
        const double Cd = S[l] / ((double)n_sel * (double)(B - (unsigned)dy) * (double)(B - (unsigned)std::abs(dx)));
        const double r = std::min(1.0, std::max(-1.0, Cd / C0));   /* (lags are normalised by their own pair counts: a valid autocorrelation whatever the data) */
        out->acf[(LH + dy) * L + LH + dx] = r;
        out->acf[(LH - dy) * L + LH - dx] = r;
    }
    out->sigma = std::sqrt(C0 * (double)(B * B) / (double)(B * B - 1));
    return 0;
}

/* The variance tables of one job: placed in the context by set(), removed when the entry point returns, whichever way (as the view
 * table of lfbm5d_views.hip): no later job on this context can see them. */
struct CorrScope {
    lfbm5d_ctx* const c;
    explicit CorrScope(lfbm5d_ctx* cc) : c(cc) { c->corr_store.n = 0; }
    ~CorrScope() { c->corr_store.n = 0; }
    int set(const std::string& who, const double* h_acf, const lfbm5d_params* Pa, const lfbm5d_params* Pb) {
        if (check_one_gpu(c, who, "correlated noise runs on one GPU (this context has a communicator or a shard)")) return 1;
        if (!h_acf) return fail(c, who + "NULL pointer for the autocorrelation");
        if (lfbm5d_corr_check(h_acf)) return fail(c, who + lfbm5d_corr_error());
        lfbm5d_ctx::CorrTables T;   /* (built aside: the context's own stays empty until the upload has succeeded) */
        std::vector<float> host;
        for (const lfbm5d_params* P : {Pa, Pb}) {
            if (!P) continue;
            bool have = false;
            for (unsigned i = 0; i < T.n; i++) have |= T.tau2[i] == P->tau_2D && T.k[i] == P->k;
            if (have) continue;
            const size_t k2 = (size_t)P->k * P->k, at = host.size();
            if (P->k < 2 || P->k > 32) continue;   /* (the job refuses such parameters with its own message) */
            host.resize(at + 2 * k2);
            if (lfbm5d_corr_table(h_acf, P->tau_2D, P->k, &host[at], &host[at + k2], nullptr)) { host.resize(at); continue; }
            T.tau2[T.n] = P->tau_2D; T.k[T.n] = P->k; T.off[T.n] = at; T.n++;
        }
        if (!T.n) return 0;
        (void)hipSetDevice(c->device);
        HIPCK(c, hipStreamSynchronize(c->stream));
        HIPCK(c, c->corr_store.dev.reserve(host.size() * sizeof(float)));
        HIPCK(c, hipMemcpy(c->corr_store.dev.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        for (unsigned i = 0; i < T.n; i++) { c->corr_store.tau2[i] = T.tau2[i]; c->corr_store.k[i] = T.k[i]; c->corr_store.off[i] = T.off[i]; }
        c->corr_store.n = T.n;
        return 0;
    }
};

} /* namespace */

extern "C" {

int lfbm5d_corr_measure_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                               unsigned block, double fraction, lfbm5d_corr_estimate* out) {
    if (!c) return 1;
    if (!d_lf) return fail(c, "lfbm5d_corr_measure_device: NULL pointer for a required buffer");
    return corr_measure(c, d_lf, nullptr, h_mask, asize, W, H, C, block, fraction, out);
}

int lfbm5d_corr_measure_host_sai(lfbm5d_ctx* c, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                 unsigned C, unsigned block, double fraction, lfbm5d_corr_estimate* out) {
    if (!c) return 1;
    if (!h_lf) return fail(c, "lfbm5d_corr_measure_host_sai: NULL pointer for a required buffer");
    return corr_measure(c, nullptr, h_lf, h_mask, asize, W, H, C, block, fraction, out);
}

int lfbm5d_denoise_corr_device(lfbm5d_ctx* c, const double* h_acf, const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy,
                               const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight,
                               unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    CorrScope tables(c);
    if (tables.set("lfbm5d_denoise_corr_device: ", h_acf, P1, P2)) return 1;
    return lfbm5d_denoise_device(c, P1, P2, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_denoise_corr_host_sai(lfbm5d_ctx* c, const double* h_acf, const lfbm5d_params* P1, const lfbm5d_params* P2, float* const* h_noisy,
                                 const unsigned* h_mask, float* const* h_basic, float* const* h_denoised, unsigned ang_major, unsigned awidth,
                                 unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    CorrScope tables(c);
    if (tables.set("lfbm5d_denoise_corr_host_sai: ", h_acf, P1, P2)) return 1;
    return lfbm5d_denoise_host_sai(c, P1, P2, h_noisy, h_mask, h_basic, h_denoised, ang_major, awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_step1_corr_device(lfbm5d_ctx* c, const double* h_acf, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask, float* d_basic,
                             unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    CorrScope tables(c);
    if (tables.set("lfbm5d_step1_corr_device: ", h_acf, P, nullptr)) return 1;
    return lfbm5d_step1_device(c, P, d_noisy, h_mask, d_basic, ang_major, awidth, aheight, an, W, H, C);
}

int lfbm5d_step2_corr_device(lfbm5d_ctx* c, const double* h_acf, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask, float* d_basic,
                             float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H,
                             unsigned C) {
    if (!c) return 1;
    CorrScope tables(c);
    if (tables.set("lfbm5d_step2_corr_device: ", h_acf, P, nullptr)) return 1;
    return lfbm5d_step2_device(c, P, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an, W, H, C);
}

int lfbm5d_debug_group_corr(lfbm5d_ctx* c, const lfbm5d_group_debug* d, const double* h_acf) {
    if (!c) return 1;
    if (!d) return fail(c, "debug_group_corr: no arguments");
    if (d->kernels && d->kernels_cap) d->kernels[0] = 0;
    if (d->bm3d) return fail(c, "debug_group_corr: the per-SAI BM3D flavour is not covered (include/lfbm5d_corr.h)");
    CorrScope tables(c);
    if (tables.set("debug_group_corr: ", h_acf, d->params, nullptr)) return 1;
    return lfbm5d_debug_group(c, d);
}

} /* extern "C" */
