/*
 * lfbm5d_photo.hip -- the photometric equalisation (lfbm5d_photo_*, include/lfbm5d_photo.h): one gain per sub-aperture image and stored
 * channel, estimated from what the other views say and divided out.  Every tested SAI is predicted from its angular neighbours by the
 * view synthesis' plane sweep (k_view_sweep / the sub-pixel sweep of lfbm5d_view.hip as they stand, launched with leave-one-out source
 * tables through view_sweep_launch, as the consistency check does); the ratio of a value to its prediction is keyed without a division
 * and counted; the median ratios and the gains are worked out on the host in double.  Not in the reference.
 *
 * Kernels (256 threads, wave64; the per-value code is lfbm5d_photo_device.h, which also compiles for the host):
 *   k_photo_stats   grid (tiles, tested SAIs), a tile of 64 x 32 positions of one tested SAI per workgroup, lanes along x: the key of
 *                   (I_m, mu) per admitted value, counted in C x 1026 LDS counters (32-bit LDS atomics); the non-zero counters are
 *                   flushed by 64-bit global atomics into [SAI][C][1026], the two skip counters the same way.
 *   k_photo_apply   grid (blocks, non-empty SAIs x C): out = in f with one factor per plane from a small table; 16-byte loads and
 *                   stores from the plane's first 16-byte boundary on, single values in front of it and behind the last group.
 * Integer atomics only: the result does not depend on the order of arrival.
 */
#include "lfbm5d_side.h"
#include "lfbm5d_photo_device.h"

using namespace lfbm5d_host;
using namespace lfbm5d_photo;

#pragma clang fp contract(off)

namespace {

static_assert(kRatioKeys == LFBM5D_PHOTO_KEYS && kEdges == LFBM5D_PHOTO_EDGES, "include/lfbm5d_photo.h");
constexpr int kTabStride = kViewTabStride, kSrcMax = 24;
constexpr int kHistD = 65;                       /* the sweep's own histogram: 17 bins at steps = 1, 65 otherwise */
constexpr unsigned kApplyBlocks = 256;           /* at most, per plane */

struct AtomicInc { __device__ __forceinline__ void operator()(unsigned* p) const { atomicAdd(p, 1u); } };

/* grid (tx_n * ty_n, tested SAIs).  table: kTabStride ints per tested SAI.  hist [asize][C][1026], skipped [2]: accumulated into. */
__global__ __launch_bounds__(kThreads) void k_photo_stats(const float* __restrict__ in, const float* __restrict__ pred,
                                                          const int* __restrict__ table, int C, int W, int H, unsigned tx_n, float lo, float hi,
                                                          unsigned long long* __restrict__ hist, unsigned long long* __restrict__ skipped) {
    __shared__ unsigned h[3 * kRatioKeys];
    __shared__ unsigned skip[2];
    const int tid = (int)threadIdx.x;
    const int m = table[(size_t)blockIdx.y * kTabStride];
    const unsigned ty = blockIdx.x / tx_n, tx = blockIdx.x - ty * tx_n;
    for (int i = tid; i < C * kRatioKeys; i += kThreads) h[i] = 0u;
    if (tid < 2) skip[tid] = 0u;
    __syncthreads();
    stats_thread(in, pred, m, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, lo, hi, h, skip, AtomicInc());
    __syncthreads();
    for (int i = tid; i < C * kRatioKeys; i += kThreads)
        if (h[i]) atomicAdd(&hist[(size_t)m * C * kRatioKeys + i], (unsigned long long)h[i]);
    if (tid < 2 && skip[tid]) atomicAdd(&skipped[tid], (unsigned long long)skip[tid]);
}

/* grid (blocks, planes).  planes [gridDim.y]: SAI * C + channel of the row's plane; factors [gridDim.y]; n = W * H. */
__global__ __launch_bounds__(kThreads) void k_photo_apply(const float* in, float* out, const unsigned* __restrict__ planes,
                                                          const float* __restrict__ factors, size_t n) {
    const size_t at = (size_t)planes[blockIdx.y] * n;
    apply_thread(in + at, out + at, n, factors[blockIdx.y], (size_t)blockIdx.x * kThreads + threadIdx.x, (size_t)gridDim.x * kThreads);
}

struct Geometry { unsigned ang_major, aw, ah, asize, W, H, C, tx_n, ty_n; };

double edge_d(int j) { return (double)edge(j); }

/* include/lfbm5d_photo.h, "Ratio of a histogram" */
bool ratio_of(const unsigned long long* h, unsigned long long min_count, double& r) {
    unsigned long long N = 0, before = 0;
    for (int k = 0; k < kRatioKeys; k++) N += h[k];
    const unsigned long long T = (N + 1) / 2;
    int k = 0;
    for (; k < kRatioKeys - 1; k++) {
        if (before + h[k] >= T) break;
        before += h[k];
    }
    r = 1.0;
    if (N < min_count || k == 0 || k == kRatioKeys - 1) return false;
    const double e0 = edge_d(k - 1), e1 = edge_d(k);
    r = e0 + (e1 - e0) * ((double)(T - before) - 0.5) / (double)h[k];
    return true;
}

/* include/lfbm5d_photo.h, "Solve".  src: kSrcMax entries per SAI.  The caller has checked the indices. */
void solve(unsigned A, const double* r, const unsigned* n_src, const unsigned* src, const unsigned char* fitted, unsigned anchor, double* g) {
    std::vector<double> h(A), live;
    std::vector<unsigned> fit;
    for (unsigned m = 0; m < A; m++) { g[m] = 1.0; if (fitted[m]) fit.push_back(m); }
    if (fit.empty()) return;
    for (int it = 0; it < LFBM5D_PHOTO_SOLVE_STEPS; it++) {
        std::copy(g, g + A, h.begin());
        for (unsigned m : fit) {
            double s = 0.0;
            for (unsigned q = 0; q < n_src[m]; q++) s = s + g[src[(size_t)m * kSrcMax + q]];
            const double t = r[m] * s / (double)n_src[m];
            h[m] = 0.5 * (g[m] + t);
        }
        double div;
        if (anchor != LFBM5D_PHOTO_NO_ANCHOR) div = h[anchor];
        else {
            live.clear();
            for (unsigned m : fit) live.push_back(h[m]);
            std::nth_element(live.begin(), live.begin() + (live.size() - 1) / 2, live.end());   /* the lower median */
            div = live[(live.size() - 1) / 2];
        }
        for (unsigned m : fit) h[m] = h[m] / div;
        std::copy(h.begin(), h.end(), g);
    }
}

const char* check_params(const lfbm5d_photo_params* P, unsigned asize, const unsigned* h_mask) {
    if (P->max_disparity > 8) return "max_disparity must be 0..8";
    if (P->box_radius > 7) return "box_radius must be 0..7";
    if (P->ang_radius < 1 || P->ang_radius > 2) return "ang_radius must be 1 or 2";
    if (P->steps != 1 && P->steps != 2 && P->steps != 4) return "steps must be 1, 2 or 4";
    if (P->min_sources < 2 || P->min_sources > (unsigned)kSrcMax) return "min_sources must be 2..24";
    if (P->max_rounds < 1 || P->max_rounds > 64) return "max_rounds must be 1..64";
    if (P->per_channel > 1) return "per_channel must be 0 or 1";
    if (P->anchor != LFBM5D_PHOTO_NO_ANCHOR && (P->anchor >= asize || !h_mask[P->anchor]))
        return "anchor must be a non-empty SAI or LFBM5D_PHOTO_NO_ANCHOR";
    if (P->min_count < 1) return "min_count must be at least 1";
    if (!(P->tol >= 0.0) || !std::isfinite(P->tol)) return "tol must be finite and not negative";
    if (!(P->lo >= 0.0) || !(P->hi >= P->lo) || !(P->hi <= 1e30)) return "lo and hi must satisfy 0 <= lo <= hi <= 1e30";
    return nullptr;
}

/* the planes of the non-empty SAIs and their factors -> the device table; enqueues the kernel.  The host vectors are the context's:
 * they outlive the copies. */
int launch_apply(lfbm5d_ctx* c, const Geometry& G, const unsigned* h_mask, const double* gain, bool invert, const float* d_in, float* d_out) {
    std::vector<unsigned>& planes = c->photo.planes_host;
    std::vector<float>& factors = c->photo.factors_host;
    HIPCK(c, hipStreamSynchronize(c->stream));   /* an earlier launch's copies have left the vectors */
    planes.clear(); factors.clear();
    for (unsigned st = 0; st < G.asize; st++) {
        if (!h_mask[st]) continue;
        for (unsigned ch = 0; ch < G.C; ch++) {
            const double g = gain[(size_t)st * 3 + ch];
            planes.push_back(st * G.C + ch);
            factors.push_back((float)(invert ? g : 1.0 / g));
        }
    }
    const size_t rows = planes.size(), n = (size_t)G.W * G.H;
    HIPCK(c, c->photo.table.reserve(rows * (sizeof(unsigned) + sizeof(float))));
    unsigned* const d_planes = c->photo.table.as<unsigned>();
    float* const d_factors = reinterpret_cast<float*>(d_planes + rows);
    HIPCK(c, hipMemcpyAsync(d_planes, planes.data(), rows * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(d_factors, factors.data(), rows * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const unsigned blocks = (unsigned)std::min<size_t>(kApplyBlocks, (n / 4 + kThreads) / kThreads);
    hipLaunchKernelGGL(k_photo_apply, dim3(blocks, (unsigned)rows), dim3(kThreads), 0, c->stream, d_in, d_out, d_planes, d_factors, n);
    HIPCK(c, hipGetLastError());
    return 0;
}

/* include/lfbm5d_photo.h, lfbm5d_photo_device */
int photo(lfbm5d_ctx* c, const std::string& who, const lfbm5d_photo_params* P, const float* d_in, const unsigned* h_mask, float* d_out,
          double* h_gain, unsigned* h_state, unsigned long long* h_hist, unsigned ang_major, unsigned aw, unsigned ah, unsigned W, unsigned H,
          unsigned C, lfbm5d_photo_result* res) {
    if (!P || !d_in || !h_mask || !d_out || !h_gain || !h_state) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_angular(c, who, ang_major, aw, ah)) return 1;
    if (const char* msg = check_params(P, aw * ah, h_mask)) return fail(c, who + msg);
    if (check_one_gpu(c, who, "the photometric equalisation runs on one GPU (this context has a communicator or a shard)")) return 1;
    TileGrid tiles;
    if (check_tiles(c, who, W, H, (unsigned long long)aw * ah * C, 0x3fffffffull, tiles)) return 1;
    const Geometry G = {ang_major, aw, ah, aw * ah, W, H, C, tiles.tx_n, tiles.ty_n};
    const size_t plane = (size_t)W * H, img = plane * C;
    if (overlap(d_in, (size_t)G.asize * img * sizeof(float), d_out, (size_t)G.asize * img * sizeof(float)))
        return fail(c, who + "d_in and d_out must not overlap");
    unsigned nne = 0;
    for (unsigned st = 0; st < G.asize; st++) nne += h_mask[st] != 0;
    if (!nne) return fail(c, who + "the mask has no non-empty SAI");

    /* the leave-one-out tables: one row per tested SAI; they do not change from round to round */
    std::vector<int> table;
    std::vector<unsigned> tested, untested, n_src(G.asize, 0), src((size_t)G.asize * kSrcMax, 0);
    unsigned most = 0;
    for (unsigned m = 0; m < G.asize; m++) {
        if (!h_mask[m]) continue;
        int row[kTabStride];
        const int n = source_row(m, G.ang_major, G.aw, G.ah, (int)P->ang_radius, [&](unsigned q) { return q != m && h_mask[q]; }, row);
        if ((unsigned)n < P->min_sources) { untested.push_back(m); continue; }
        tested.push_back(m);
        table.insert(table.end(), row, row + kTabStride);
        n_src[m] = (unsigned)n;
        for (int q = 0; q < n; q++) src[(size_t)m * kSrcMax + q] = (unsigned)row[2 + 3 * q];
        most = std::max(most, (unsigned)n);
    }

    (void)hipSetDevice(c->device);
    const size_t n_hist = (size_t)G.asize * C * kRatioKeys;
    /* stats: [hist n_hist][skipped 2][the sweep's disparity histogram 65] */
    const size_t words = n_hist + 2 + kHistD;
    HIPCK(c, c->photo.stats.reserve(words * sizeof(unsigned long long)));
    HIPCK(c, c->photo.sweep_table.reserve(std::max<size_t>(1, table.size()) * sizeof(int)));
    HIPCK(c, c->photo.pred.reserve((size_t)G.asize * img * sizeof(float)));
    HIPCK(c, c->photo.disp.reserve((size_t)G.asize * plane));
    unsigned long long* const d_hist = c->photo.stats.as<unsigned long long>();
    unsigned long long* const d_skip = d_hist + n_hist;
    unsigned long long* const d_dh = d_skip + 2;
    float* const d_pred = c->photo.pred.as<float>();
    int* const d_table = c->photo.sweep_table.as<int>();
    if (!tested.empty()) HIPCK(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));

    lfbm5d_photo_result r;
    std::memset(&r, 0, sizeof(r));
    const float lo = (float)P->lo, hi = (float)P->hi;
    const unsigned n_fit = P->per_channel ? C : 1;    /* histograms (and solves) per SAI */
    std::vector<unsigned long long> host(n_hist + 2), pooled(kRatioKeys);
    std::vector<double> ratio((size_t)n_fit * G.asize), g((size_t)G.asize * 3), gain((size_t)G.asize * 3, 1.0);
    std::vector<unsigned char> fitted((size_t)n_fit * G.asize);
    const float* x = d_in;                           /* the current light field: the input, then d_out, corrected in place */
    for (;;) {
        HIPCK(c, hipMemsetAsync(d_hist, 0, words * sizeof(unsigned long long), c->stream));
        if (!tested.empty()) {
            if (view_sweep_launch(c, d_table, (unsigned)tested.size(), x, d_pred, c->photo.disp.as<signed char>(), W, H, C, (int)P->max_disparity,
                                  (int)P->box_radius, d_dh, P->steps, most)) return 1;
            hipLaunchKernelGGL(k_photo_stats, dim3(G.tx_n * G.ty_n, (unsigned)tested.size()), dim3(kThreads), 0, c->stream, x, d_pred, d_table,
                               (int)C, (int)W, (int)H, G.tx_n, lo, hi, d_hist, d_skip);
            HIPCK(c, hipGetLastError());
        }
        HIPCK(c, hipMemcpyAsync(host.data(), d_hist, (n_hist + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        r.rounds++;
        std::fill(ratio.begin(), ratio.end(), 1.0);
        std::fill(fitted.begin(), fitted.end(), 0);
        r.residual = 0.0;
        for (unsigned m : tested)
            for (unsigned k = 0; k < n_fit; k++) {
                const unsigned long long* h = &host[((size_t)m * C + k) * kRatioKeys];
                if (!P->per_channel) {
                    for (int i = 0; i < kRatioKeys; i++) {
                        pooled[i] = 0;
                        for (unsigned ch = 0; ch < C; ch++) pooled[i] += host[((size_t)m * C + ch) * kRatioKeys + i];
                    }
                    h = pooled.data();
                }
                double rr;
                if (!ratio_of(h, P->min_count, rr)) continue;
                fitted[(size_t)k * G.asize + m] = 1;
                ratio[(size_t)k * G.asize + m] = rr;
                r.residual = std::max(r.residual, std::fabs(rr - 1.0));
            }
        if (r.residual <= P->tol) { r.converged = 1; break; }
        for (unsigned st = 0; st < G.asize; st++) g[st * 3] = g[st * 3 + 1] = g[st * 3 + 2] = 1.0;
        std::vector<double> gk(G.asize);
        for (unsigned k = 0; k < n_fit; k++) {
            solve(G.asize, &ratio[(size_t)k * G.asize], n_src.data(), src.data(), &fitted[(size_t)k * G.asize], P->anchor, gk.data());
            for (unsigned st = 0; st < G.asize; st++)
                for (unsigned ch = P->per_channel ? k : 0; ch < (P->per_channel ? k + 1 : C); ch++) {
                    g[(size_t)st * 3 + ch] = gk[st];
                    gain[(size_t)st * 3 + ch] = gain[(size_t)st * 3 + ch] * gk[st];
                }
        }
        if (launch_apply(c, G, h_mask, g.data(), false, x, d_out)) return 1;
        x = d_out;
        if (r.rounds == P->max_rounds) break;
    }
    if (x == d_in && copy_sais(c, G.asize, d_out, d_in, img, sizeof(float), [&](unsigned st) { return h_mask[st] != 0; })) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));

    r.gain_min = r.gain_max = 1.0;
    bool first = true;
    for (unsigned st = 0; st < G.asize; st++) {
        h_state[st] = 0u;
        if (!h_mask[st]) continue;
        h_state[st] = 2u;
        for (unsigned ch = 0; ch < C; ch++) {
            const double v = gain[(size_t)st * 3 + ch];
            r.gain_min = first ? v : std::min(r.gain_min, v);
            r.gain_max = first ? v : std::max(r.gain_max, v);
            first = false;
        }
    }
    for (unsigned m : tested) {
        h_state[m] = 1u;
        for (unsigned k = 0; k < n_fit; k++) if (!fitted[(size_t)k * G.asize + m]) h_state[m] = 3u;
    }
    for (unsigned st = 0; st < G.asize; st++) {
        r.fitted += h_state[st] == 1u; r.untested += h_state[st] == 2u; r.unfit += h_state[st] == 3u;
    }
    for (size_t i = 0; i < n_hist; i++) r.admitted += host[i];
    r.skipped_nonfinite = host[n_hist];
    r.skipped_range = host[n_hist + 1];
    std::memcpy(h_gain, gain.data(), gain.size() * sizeof(double));
    if (h_hist) std::memcpy(h_hist, host.data(), n_hist * sizeof(unsigned long long));
    if (res) *res = r;
    return 0;
}

/* include/lfbm5d_photo.h, lfbm5d_photo_host_sai */
int photo_host_sai(lfbm5d_ctx* c, const std::string& who, const lfbm5d_photo_params* P, const float* const* h_in, const unsigned* h_mask,
                   float* const* h_out, double* h_gain, unsigned* h_state, unsigned long long* h_hist, unsigned ang_major, unsigned aw,
                   unsigned ah, unsigned W, unsigned H, unsigned C, lfbm5d_photo_result* out) {
    if (!P || !h_in || !h_mask || !h_out || !h_gain || !h_state) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const unsigned asize = aw * ah;
    const size_t img = (size_t)W * H * C, all = std::max<size_t>(1, (size_t)asize * img);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_out, asize, nonempty)) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    HIPCK(c, c->photo.x.reserve(all * sizeof(float)));
    float* const din = c->h2d_noisy.as<float>();
    float* const dout = c->photo.x.as<float>();
    if (upload_planes(c, who, h_in, din, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (photo(c, who, P, din, h_mask, dout, h_gain, h_state, h_hist, ang_major, aw, ah, W, H, C, out)) return 1;
    if (download_planes(c, h_out, dout, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int check_gains(lfbm5d_ctx* c, const std::string& who, const unsigned* h_mask, const double* h_gain, unsigned asize, unsigned C) {
    for (unsigned st = 0; st < asize; st++)
        for (unsigned ch = 0; h_mask[st] && ch < C; ch++) {
            const double g = h_gain[(size_t)st * 3 + ch];
            if (!(g > 0.0) || !std::isfinite(g)) return fail(c, who + "every gain of a non-empty SAI must be finite and positive");
        }
    return 0;
}

/* include/lfbm5d_photo.h, lfbm5d_photo_apply_device */
int apply(lfbm5d_ctx* c, const std::string& who, const float* d_in, const unsigned* h_mask, const double* h_gain, unsigned invert, float* d_out,
          unsigned aw, unsigned ah, unsigned W, unsigned H, unsigned C) {
    if (!d_in || !h_mask || !h_gain || !d_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 1, "not be 0")) return 1;
    if (!aw || !ah) return fail(c, who + "awidth and aheight must be at least 1");
    if (invert > 1) return fail(c, who + "invert must be 0 or 1");
    if (check_one_gpu(c, who, "the photometric equalisation runs on one GPU (this context has a communicator or a shard)")) return 1;
    TileGrid tiles;
    if (check_tiles(c, who, W, H, (unsigned long long)aw * ah * C, 0x3fffffffull, tiles)) return 1;
    const Geometry G = {0, aw, ah, aw * ah, W, H, C, tiles.tx_n, tiles.ty_n};
    const size_t bytes = (size_t)G.asize * W * H * C * sizeof(float);
    if (d_in != d_out && overlap(d_in, bytes, d_out, bytes)) return fail(c, who + "d_out must be d_in or not overlap it");
    if (check_gains(c, who, h_mask, h_gain, G.asize, C)) return 1;
    unsigned nne = 0;
    for (unsigned st = 0; st < G.asize; st++) nne += h_mask[st] != 0;
    if (!nne) return fail(c, who + "the mask has no non-empty SAI");
    (void)hipSetDevice(c->device);
    if (launch_apply(c, G, h_mask, h_gain, invert != 0, d_in, d_out)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int apply_host_sai(lfbm5d_ctx* c, const std::string& who, const float* const* h_in, const unsigned* h_mask, const double* h_gain,
                   unsigned invert, float* const* h_out, unsigned aw, unsigned ah, unsigned W, unsigned H, unsigned C) {
    if (!h_in || !h_mask || !h_gain || !h_out) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    const unsigned asize = aw * ah;
    const size_t img = (size_t)W * H * C, all = std::max<size_t>(1, (size_t)asize * img);
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_out, asize, nonempty)) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, c->h2d_noisy.reserve(all * sizeof(float)));
    float* const d = c->h2d_noisy.as<float>();
    if (upload_planes(c, who, h_in, d, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (apply(c, who, d, h_mask, h_gain, invert, d, aw, ah, W, H, C)) return 1;
    if (download_planes(c, h_out, d, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

void lfbm5d_photo_defaults(lfbm5d_photo_params* out) {
    if (!out) return;
    out->max_disparity = 4;                  /* the consistency check's sweep */
    out->box_radius = 3;
    out->ang_radius = 1;
    out->steps = 1;
    out->min_sources = 3;
    out->max_rounds = 3;
    out->per_channel = 1;
    out->anchor = LFBM5D_PHOTO_NO_ANCHOR;
    out->min_count = 256;
    out->tol = 1.0 / 256.0;                  /* one key */
    out->lo = 4.0;                           /* the row picked in profiles/photo_defaults.txt (one light field and a translated view of */
    out->hi = 240.0;                         /* it, unclipped: the sweep cannot weigh hi's guard against saturated values) */
}

void lfbm5d_photo_edges(float* out) {
    if (!out) return;
    for (int j = 0; j < kEdges; j++) out[j] = edge(j);
}

int lfbm5d_photo_ratio(const unsigned long long* hist, unsigned long long min_count, double* ratio) {
    if (ratio) *ratio = 1.0;
    if (!hist || !ratio) return 1;
    return ratio_of(hist, min_count, *ratio) ? 0 : 1;
}

int lfbm5d_photo_solve(unsigned asize, const double* ratio, const unsigned* n_src, const unsigned* src, const unsigned* fitted,
                       unsigned anchor, double* gain) {
    if (!ratio || !n_src || !src || !fitted || !gain) return 1;
    if (anchor != LFBM5D_PHOTO_NO_ANCHOR && anchor >= asize) return 1;
    std::vector<unsigned char> fit(asize, 0);
    for (unsigned m = 0; m < asize; m++) {
        if (!fitted[m]) continue;
        fit[m] = 1;
        if (!n_src[m] || n_src[m] > (unsigned)kSrcMax) return 1;
        for (unsigned q = 0; q < n_src[m]; q++) if (src[(size_t)m * kSrcMax + q] >= asize) return 1;
    }
    solve(asize, ratio, n_src, src, fit.data(), anchor, gain);
    return 0;
}

int lfbm5d_photo_device(lfbm5d_ctx* c, const lfbm5d_photo_params* P, const float* d_in, const unsigned* h_mask, float* d_out, double* h_gain,
                        unsigned* h_state, unsigned long long* h_hist, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W,
                        unsigned H, unsigned C, lfbm5d_photo_result* out) {
    if (!c) return 1;
    return photo(c, "lfbm5d_photo_device: ", P, d_in, h_mask, d_out, h_gain, h_state, h_hist, ang_major, awidth, aheight, W, H, C, out);
}

int lfbm5d_photo_host_sai(lfbm5d_ctx* c, const lfbm5d_photo_params* P, const float* const* h_in, const unsigned* h_mask, float* const* h_out,
                          double* h_gain, unsigned* h_state, unsigned long long* h_hist, unsigned ang_major, unsigned awidth,
                          unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_photo_result* out) {
    if (!c) return 1;
    return photo_host_sai(c, "lfbm5d_photo_host_sai: ", P, h_in, h_mask, h_out, h_gain, h_state, h_hist, ang_major, awidth, aheight, W, H, C,
                          out);
}

int lfbm5d_photo_apply_device(lfbm5d_ctx* c, const float* d_in, const unsigned* h_mask, const double* h_gain, unsigned invert, float* d_out,
                              unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return apply(c, "lfbm5d_photo_apply_device: ", d_in, h_mask, h_gain, invert, d_out, awidth, aheight, W, H, C);
}

int lfbm5d_photo_apply_host_sai(lfbm5d_ctx* c, const float* const* h_in, const unsigned* h_mask, const double* h_gain, unsigned invert,
                                float* const* h_out, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    return apply_host_sai(c, "lfbm5d_photo_apply_host_sai: ", h_in, h_mask, h_gain, invert, h_out, awidth, aheight, W, H, C);
}

} /* extern "C" */
