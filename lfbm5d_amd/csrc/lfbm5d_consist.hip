/*
 * lfbm5d_consist.hip -- the consistency check (lfbm5d_consist_*, include/lfbm5d.h): defective values and bad sub-aperture images are
 * found by what the other views say.  Every tested SAI is predicted from its angular neighbours by the view synthesis' plane sweep
 * (k_view_sweep of lfbm5d_view.hip as it stands, launched with leave-one-out source tables through view_sweep_launch), the residual
 * against the prediction is compared with a threshold from the light field's own median residual and with the spread of the sources
 * around their mean, and an SAI whose median residual stands out among its neighbours' is bad.  Not in the reference.
 *
 * Kernels (256 threads, wave64, a tile of 64 x 32 positions of one tested SAI per workgroup, lanes along x; the per-value code is
 * lfbm5d_consist_device.h, which also compiles for the host):
 *   k_consist_stats   grid (tiles, tested SAIs): rho = I_m - mu and the key of |rho| per value, counted in C x 386 LDS counters
 *                     (32-bit LDS atomics); the non-zero counters are flushed by 64-bit global atomics into [SAI][C][386].
 *   k_consist_flag    (k_consist_flag_subpel behind a sweep with 2 or 4 steps per pixel) grid (tiles, tested SAIs): per value mu from the prediction plane, v = the sources' squared deviations at d*
 *                     (d* varies per pixel: cached gathers), the two tests, the code byte; counts per (SAI, channel, code) through LDS.
 * Integer atomics only; the quantiles and the bad-SAI decision run on the host in double on the integer histograms.
 */
#include "lfbm5d_side.h"
#include "lfbm5d_consist_device.h"

using namespace lfbm5d_host;
using namespace lfbm5d_consist;

#pragma clang fp contract(off)

namespace {

static_assert(kKeys == LFBM5D_IMPULSE_KEYS, "include/lfbm5d.h");
static_assert(kTabStride == kViewTabStride, "lfbm5d_view.hip's table");
constexpr int kHistD = lfbm5d_subpel::kHist;   /* the sweep's histogram: 17 bins at steps = 1, 65 otherwise */

struct AtomicInc { __device__ __forceinline__ void operator()(unsigned* p) const { atomicAdd(p, 1u); } };

/* grid (tx_n * ty_n, tested SAIs).  table: kTabStride ints per tested SAI.  hist [asize][C][386], skipped [1]: accumulated into. */
__global__ __launch_bounds__(kThreads) void k_consist_stats(const float* __restrict__ in, const float* __restrict__ pred,
                                                            const int* __restrict__ table, int C, int W, int H, unsigned tx_n,
                                                            unsigned long long* __restrict__ hist, unsigned long long* __restrict__ skipped) {
    __shared__ unsigned h[3 * kKeys];
    __shared__ unsigned skip;
    const int tid = (int)threadIdx.x;
    const int m = table[(size_t)blockIdx.y * kTabStride];
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    for (int i = tid; i < C * kKeys; i += kThreads) h[i] = 0u;
    if (tid == 0) skip = 0u;
    __syncthreads();
    stats_thread(in, pred, m, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, h, &skip, AtomicInc());
    __syncthreads();
    for (int i = tid; i < C * kKeys; i += kThreads)
        if (h[i]) atomicAdd(&hist[(size_t)m * C * kKeys + i], (unsigned long long)h[i]);
    if (tid == 0 && skip) atomicAdd(skipped, (unsigned long long)skip);
}

/* grid (tx_n * ty_n, tested SAIs).  counts [asize][3][2] (code 1, code 2): accumulated into. */
__global__ __launch_bounds__(kThreads) void k_consist_flag(const float* __restrict__ in, const float* __restrict__ pred,
                                                           const signed char* __restrict__ disp, unsigned char* __restrict__ flags,
                                                           const int* __restrict__ table, int C, int W, int H, unsigned tx_n, Thresholds thr,
                                                           float g, unsigned long long* __restrict__ counts) {
    __shared__ unsigned cnt[6];
    const int tid = (int)threadIdx.x;
    const int* __restrict__ tab = table + (size_t)blockIdx.y * kTabStride;
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    if (tid < 6) cnt[tid] = 0u;
    __syncthreads();
    flag_thread(in, pred, disp, flags, tab, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, thr, g, cnt, AtomicInc());
    __syncthreads();
    if (tid < 6 && cnt[tid]) atomicAdd(&counts[(size_t)tab[0] * 6 + tid], (unsigned long long)cnt[tid]);
}

/* the same behind the sweep with Q = 2 or 4 hypotheses per pixel: disp holds j*, the spread comes from the interpolated warp */
__global__ __launch_bounds__(kThreads) void k_consist_flag_subpel(const float* __restrict__ in, const float* __restrict__ pred,
                                                                  const signed char* __restrict__ disp, unsigned char* __restrict__ flags,
                                                                  const int* __restrict__ table, int C, int W, int H, unsigned tx_n,
                                                                  Thresholds thr, float g, unsigned long long* __restrict__ counts, int Q) {
    __shared__ unsigned cnt[6];
    const int tid = (int)threadIdx.x;
    const int* __restrict__ tab = table + (size_t)blockIdx.y * kTabStride;
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    if (tid < 6) cnt[tid] = 0u;
    __syncthreads();
    flag_thread<true>(in, pred, disp, flags, tab, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, thr, g, cnt, AtomicInc(), Q);
    __syncthreads();
    if (tid < 6 && cnt[tid]) atomicAdd(&counts[(size_t)tab[0] * 6 + tid], (unsigned long long)cnt[tid]);
}

struct Geometry { unsigned ang_major, aw, ah, asize, W, H, C, tx_n, ty_n; };

/* the leave-one-out tables under the exclude set: one row per tested SAI; SAIs with fewer than min_sources sources are untested */
void plan(const Geometry& G, const lfbm5d_consist_params* P, const unsigned* h_mask, const std::vector<unsigned char>& excl,
          std::vector<int>& table, std::vector<unsigned>& tested, std::vector<unsigned>& untested) {
    table.clear(); tested.clear(); untested.clear();
    for (unsigned m = 0; m < G.asize; m++) {
        if (!h_mask[m] || excl[m]) continue;
        int row[kTabStride];
        const int n = source_row(m, G.ang_major, G.aw, G.ah, (int)P->ang_radius, [&](unsigned q) { return q != m && h_mask[q] && !excl[q]; }, row);
        if ((unsigned)n < P->min_sources) { untested.push_back(m); continue; }
        tested.push_back(m);
        table.insert(table.end(), row, row + kTabStride);
    }
}

/* one histogram's median; 0 with ok = false for an empty one */
double median_of(const unsigned long long* h, bool& ok) {
    double s = 0.0;
    ok = lfbm5d_impulse_scale(h, &s) == 0;
    return ok ? s : 0.0;
}

/* s_m of every tested SAI (its histogram pooled over channels) */
void sai_scales(const Geometry& G, const std::vector<unsigned>& tested, const std::vector<unsigned long long>& hist, std::vector<double>& s,
                std::vector<unsigned char>& has) {
    s.assign(G.asize, 0.0); has.assign(G.asize, 0);
    for (unsigned m : tested) {
        unsigned long long pooled[kKeys] = {0};
        for (unsigned c = 0; c < G.C; c++)
            for (int k = 0; k < kKeys; k++) pooled[k] += hist[((size_t)m * G.C + c) * kKeys + k];
        bool ok;
        s[m] = median_of(pooled, ok);
        has[m] = ok ? 1 : 0;
    }
}

/* the bad-SAI decision of include/lfbm5d.h, from the scales of one sweep; bad in increasing order */
void decide(const Geometry& G, const lfbm5d_consist_params* P, const std::vector<unsigned>& tested, const std::vector<double>& s,
            const std::vector<unsigned char>& has, std::vector<unsigned>& bad) {
    bad.clear();
    std::vector<double> live;
    for (unsigned m : tested) if (has[m]) live.push_back(s[m]);
    std::vector<unsigned char> exceeds(G.asize, 0);
    if (!live.empty()) {
        std::sort(live.begin(), live.end());
        const double ref = live[(live.size() - 1) / 2];
        const double limit = P->sai_factor * std::max(ref, P->min_scale);
        for (unsigned m : tested) exceeds[m] = has[m] && s[m] > limit;
    }
    const int R = (int)P->ang_radius;
    for (unsigned m : tested) {
        if (!has[m]) { bad.push_back(m); continue; }
        if (!exceeds[m]) continue;
        int sm, tm;
        sai_coords(m, G.ang_major, G.aw, G.ah, sm, tm);
        bool beaten = false;
        for (unsigned q : tested) {
            if (q == m || !exceeds[q]) continue;
            int sq, tq;
            sai_coords(q, G.ang_major, G.aw, G.ah, sq, tq);
            if (std::abs(sq - sm) > R || std::abs(tq - tm) > R) continue;
            if (s[q] > s[m] || (s[q] == s[m] && q < m)) beaten = true;
        }
        if (!beaten) bad.push_back(m);
    }
}

const char* check_params(const lfbm5d_consist_params* P) {
    if (P->max_disparity > 8) return "max_disparity must be 0..8";
    if (P->box_radius > 7) return "box_radius must be 0..7";
    if (P->ang_radius < 1 || P->ang_radius > 2) return "ang_radius must be 1 or 2";
    if (P->min_sources < 2 || P->min_sources > (unsigned)kSrcMax) return "min_sources must be 2..24";
    if (P->max_rounds < 1 || P->max_rounds > 64) return "max_rounds must be 1..64";
    if (!(P->k >= 0.0) || !std::isfinite(P->k) || !(P->min_threshold >= 0.0) || !std::isfinite(P->min_threshold))
        return "k and min_threshold must be finite and not negative";
    if (!(P->spread >= 0.0) || !std::isfinite(P->spread)) return "spread must be finite and not negative";
    if (!(P->sai_factor >= 0.0) || !std::isfinite(P->sai_factor)) return "sai_factor must be finite and not negative (0 switches the decision off)";
    if (!(P->min_scale >= 0.0) || !std::isfinite(P->min_scale)) return "min_scale must be finite and not negative";
    return nullptr;
}

/* include/lfbm5d.h, lfbm5d_consist_steps_device */
int consist(lfbm5d_ctx* c, const std::string& who, const lfbm5d_consist_params* P, unsigned steps, const float* d_in, const unsigned* h_mask,
            const unsigned* h_exclude, unsigned char* d_flags, unsigned* h_state, signed char* d_disp, double* h_scale_sai,
            unsigned long long* h_hist, unsigned ang_major, unsigned aw, unsigned ah, unsigned W, unsigned H, unsigned C,
            lfbm5d_consist_result* res) {
    if (!P || !d_in || !h_mask || !d_flags || !h_state) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_angular(c, who, ang_major, aw, ah)) return 1;
    if (const char* msg = check_params(P)) return fail(c, who + msg);
    if (steps != 1 && steps != 2 && steps != 4) return fail(c, who + "steps must be 1, 2 or 4");
    if (check_one_gpu(c, who, "the consistency check runs on one GPU (this context has a communicator or a shard)")) return 1;
    TileGrid tiles;
    if (check_tiles(c, who, W, H, aw * ah, 0x3fffffffull, tiles)) return 1;
    const Geometry G = {ang_major, aw, ah, aw * ah, W, H, C, tiles.tx_n, tiles.ty_n};
    std::vector<unsigned char> excl(G.asize, 0), found(G.asize, 0);
    unsigned nne = 0;
    for (unsigned st = 0; st < G.asize; st++) {
        if (h_mask[st]) nne++;
        if (h_exclude && h_exclude[st] && h_mask[st]) excl[st] = 1;
    }
    if (!nne) return fail(c, who + "the mask has no non-empty SAI");

    (void)hipSetDevice(c->device);
    const size_t plane = (size_t)W * H, img = plane * C;
    const size_t n_hist = (size_t)G.asize * C * kKeys, n_cnt = (size_t)G.asize * 6;
    /* stats: [hist n_hist][skipped 1][counts n_cnt][the sweep's disparity histogram 17] */
    const size_t words = n_hist + 1 + n_cnt + kHistD;
    HIPCK(c, c->consist.stats.reserve(words * sizeof(unsigned long long)));
    HIPCK(c, c->consist.table.reserve((size_t)G.asize * kTabStride * sizeof(int)));
    HIPCK(c, c->consist.pred.reserve((size_t)G.asize * img * sizeof(float)));
    HIPCK(c, c->consist.disp.reserve((size_t)G.asize * plane));
    unsigned long long* const d_hist = c->consist.stats.as<unsigned long long>();
    unsigned long long* const d_skip = d_hist + n_hist;
    unsigned long long* const d_cnt = d_skip + 1;
    unsigned long long* const d_dh = d_cnt + n_cnt;
    float* const d_pred = c->consist.pred.as<float>();
    signed char* const d_dstar = c->consist.disp.as<signed char>();   /* a sweep of an earlier round must not reach the caller's planes */
    int* const d_table = c->consist.table.as<int>();

    lfbm5d_consist_result r;
    std::memset(&r, 0, sizeof(r));
    std::vector<int> table;
    std::vector<unsigned> tested, untested, bad;
    std::vector<unsigned long long> host(words);
    std::vector<double> s, s_report(G.asize, 0.0);
    std::vector<unsigned char> has;
    unsigned decisions = 0;
    for (;;) {
        plan(G, P, h_mask, excl, table, tested, untested);
        HIPCK(c, hipMemsetAsync(d_hist, 0, words * sizeof(unsigned long long), c->stream));
        if (!tested.empty()) {
            HIPCK(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            unsigned most = 0;
            for (size_t i = 0; i < tested.size(); i++) most = std::max(most, (unsigned)table[i * kTabStride + 1]);
            if (view_sweep_launch(c, d_table, (unsigned)tested.size(), d_in, d_pred, d_dstar, W, H, C, (int)P->max_disparity,
                                  (int)P->box_radius, d_dh, steps, most)) return 1;
            hipLaunchKernelGGL(k_consist_stats, dim3(G.tx_n * G.ty_n, (unsigned)tested.size()), dim3(kThreads), 0, c->stream, d_in, d_pred,
                               d_table, (int)C, (int)W, (int)H, G.tx_n, d_hist, d_skip);
            HIPCK(c, hipGetLastError());
        }
        HIPCK(c, hipMemcpyAsync(host.data(), d_hist, (n_hist + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));   /* the table leaves a host object; the histograms are read */
        r.rounds++;
        sai_scales(G, tested, host, s, has);
        if (P->sai_factor > 0.0 && decisions < P->max_rounds) {
            decisions++;
            decide(G, P, tested, s, has, bad);
            if (!bad.empty()) {
                for (unsigned m : bad) { excl[m] = 1; found[m] = 1; s_report[m] = s[m]; }
                continue;
            }
        }
        break;
    }
    for (unsigned m : tested) s_report[m] = s[m];
    r.skipped = host[n_hist];
    r.tested = (unsigned)tested.size();
    r.untested = (unsigned)untested.size();
    r.pixels = (unsigned long long)tested.size() * img;
    Thresholds thr = {{0.0f, 0.0f, 0.0f}};
    for (unsigned ch = 0; ch < C; ch++) {
        unsigned long long pooled[kKeys] = {0};
        for (unsigned m : tested)
            for (int k = 0; k < kKeys; k++) pooled[k] += host[((size_t)m * C + ch) * kKeys + k];
        bool ok;
        r.scale_channel[ch] = median_of(pooled, ok);
        thr.t[ch] = (float)std::max(P->k * r.scale_channel[ch], P->min_threshold);
        r.threshold[ch] = (double)thr.t[ch];
    }
    const float g = (float)(P->spread * P->spread);

    for (unsigned st = 0; st < G.asize; st++) {
        if (!h_mask[st]) { h_state[st] = 0; continue; }
        HIPCK(c, hipMemsetAsync(d_flags + (size_t)st * img, 0, img, c->stream));
        h_state[st] = h_exclude && h_exclude[st] ? 4u : found[st] ? 2u : 3u;
        if (found[st]) r.bad++;
    }
    for (unsigned m : tested) h_state[m] = 1u;
    std::vector<unsigned long long> cnt(n_cnt, 0ull);
    if (!tested.empty()) {
        const dim3 grid(G.tx_n * G.ty_n, (unsigned)tested.size());
        if (steps == 1)
            hipLaunchKernelGGL(k_consist_flag, grid, dim3(kThreads), 0, c->stream, d_in, d_pred, d_dstar, d_flags, d_table, (int)C, (int)W, (int)H,
                               G.tx_n, thr, g, d_cnt);
        else
            hipLaunchKernelGGL(k_consist_flag_subpel, grid, dim3(kThreads), 0, c->stream, d_in, d_pred, d_dstar, d_flags, d_table, (int)C, (int)W,
                               (int)H, G.tx_n, thr, g, d_cnt, (int)steps);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(cnt.data(), d_cnt, n_cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        if (d_disp && copy_sais(c, G.asize, d_disp, d_dstar, plane, 1, [&](unsigned st) { return h_state[st] == 1u; })) return 1;
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (unsigned m : tested)
        for (unsigned ch = 0; ch < C; ch++) {
            r.flagged[ch][0] += cnt[(size_t)m * 6 + ch * 2];
            r.flagged[ch][1] += cnt[(size_t)m * 6 + ch * 2 + 1];
        }
    if (h_scale_sai) std::memcpy(h_scale_sai, s_report.data(), G.asize * sizeof(double));
    if (h_hist) std::memcpy(h_hist, host.data(), n_hist * sizeof(unsigned long long));
    if (res) *res = r;
    return 0;
}

/* include/lfbm5d.h, lfbm5d_consist_steps_host_sai */
int host_sai(lfbm5d_ctx* c, const std::string& who, const lfbm5d_consist_params* P, unsigned steps, const float* const* h_in,
             const unsigned* h_mask, const unsigned* h_exclude, unsigned char* const* h_flags, unsigned* h_state, signed char* const* h_disp,
             double* h_scale_sai, unsigned long long* h_hist, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H,
             unsigned C, lfbm5d_consist_result* out) {
    if (!P || !h_in || !h_mask || !h_flags || !h_state) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const unsigned asize = awidth * aheight;
    const size_t plane = (size_t)W * H, img = plane * C, all = std::max<size_t>(1, (size_t)asize * img);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_flags, asize, nonempty) || (h_disp && check_planes(c, who, h_disp, asize, nonempty))) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    HIPCK(c, c->consist.flags.reserve(all + std::max<size_t>(1, (size_t)asize * plane)));
    float* const din = c->h2d_noisy.as<float>();
    unsigned char* const dfl = c->consist.flags.as<unsigned char>();
    signed char* const ddisp = h_disp ? reinterpret_cast<signed char*>(dfl + all) : nullptr;
    if (upload_planes(c, who, h_in, din, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (consist(c, who, P, steps, din, h_mask, h_exclude, dfl, h_state, ddisp, h_scale_sai, h_hist, ang_major, awidth, aheight, W, H, C, out))
        return 1;
    if (download_planes(c, h_flags, dfl, asize, img, nonempty)) return 1;
    if (ddisp && download_planes(c, h_disp, ddisp, asize, plane, [&](unsigned st) { return h_state[st] == 1u; })) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

void lfbm5d_consist_defaults(lfbm5d_consist_params* out) {
    if (!out) return;
    out->max_disparity = 4;                  /* the view synthesis' D and r */
    out->box_radius = 3;
    out->ang_radius = 1;
    out->min_sources = 3;                    /* the row picked in profiles/consist_defaults.txt (one light field) */
    out->max_rounds = 3;
    out->k = 8.0;
    out->min_threshold = 0.0;
    out->spread = 4.0;
    out->sai_factor = 1.5;
    out->min_scale = 0.5;                   /* half a grey level of 8-bit data: below the quantisation step a ratio of scales means nothing */
}

int lfbm5d_consist_steps_device(lfbm5d_ctx* c, const lfbm5d_consist_params* P, unsigned steps, const float* d_in, const unsigned* h_mask,
                                const unsigned* h_exclude, unsigned char* d_flags, unsigned* h_state, signed char* d_disp, double* h_scale_sai,
                                unsigned long long* h_hist, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H,
                                unsigned C, lfbm5d_consist_result* out) {
    if (!c) return 1;
    return consist(c, "lfbm5d_consist_steps_device: ", P, steps, d_in, h_mask, h_exclude, d_flags, h_state, d_disp, h_scale_sai, h_hist, ang_major,
                   awidth, aheight, W, H, C, out);
}

int lfbm5d_consist_device(lfbm5d_ctx* c, const lfbm5d_consist_params* P, const float* d_in, const unsigned* h_mask, const unsigned* h_exclude,
                          unsigned char* d_flags, unsigned* h_state, signed char* d_disp, double* h_scale_sai, unsigned long long* h_hist,
                          unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C,
                          lfbm5d_consist_result* out) {
    if (!c) return 1;
    return consist(c, "lfbm5d_consist_device: ", P, 1, d_in, h_mask, h_exclude, d_flags, h_state, d_disp, h_scale_sai, h_hist, ang_major, awidth,
                   aheight, W, H, C, out);
}

int lfbm5d_consist_steps_host_sai(lfbm5d_ctx* c, const lfbm5d_consist_params* P, unsigned steps, const float* const* h_in,
                                  const unsigned* h_mask, const unsigned* h_exclude, unsigned char* const* h_flags, unsigned* h_state,
                                  signed char* const* h_disp, double* h_scale_sai, unsigned long long* h_hist, unsigned ang_major,
                                  unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_consist_result* out) {
    if (!c) return 1;
    return host_sai(c, "lfbm5d_consist_steps_host_sai: ", P, steps, h_in, h_mask, h_exclude, h_flags, h_state, h_disp, h_scale_sai, h_hist,
                    ang_major, awidth, aheight, W, H, C, out);
}

int lfbm5d_consist_host_sai(lfbm5d_ctx* c, const lfbm5d_consist_params* P, const float* const* h_in, const unsigned* h_mask,
                            const unsigned* h_exclude, unsigned char* const* h_flags, unsigned* h_state, signed char* const* h_disp,
                            double* h_scale_sai, unsigned long long* h_hist, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W,
                            unsigned H, unsigned C, lfbm5d_consist_result* out) {
    if (!c) return 1;
    return host_sai(c, "lfbm5d_consist_host_sai: ", P, 1, h_in, h_mask, h_exclude, h_flags, h_state, h_disp, h_scale_sai, h_hist, ang_major,
                    awidth, aheight, W, H, C, out);
}

} /* extern "C" */
