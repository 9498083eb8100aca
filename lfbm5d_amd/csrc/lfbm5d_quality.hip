/*
 * lfbm5d_quality.hip -- quality of a light field against a reference (lfbm5d_quality_*, include/lfbm5d.h): per SAI the mean squared
 * error (hence RMSE and PSNR: compute_psnr / compute_psnr_LF, utilities_LF.cpp:639-692, in double instead of float) and the SSIM of
 * Wang, Bovik, Sheikh & Simoncelli (2004; 11 x 11 Gaussian window of sigma 1.5, every valid position, no padding), and their mean
 * and population standard deviation over the non-empty SAIs.  SSIM is not in the reference.
 *
 * Kernels, in stream order:
 *   k_quality<SSIM>   grid (SAI x channel, column tile, row tile), 256 threads.  A workgroup takes kCols x kRows window positions of
 *                     one plane: it stages the kRows + 10 input rows of both images through LDS as doubles, 11 rows at a time (kCols
 *                     + 10 columns); each of its four waves takes 64 columns, one per lane, and walks down the rows: the five
 *                     horizontal 11-tap sums (a, b, a^2, b^2, ab) of the new row go into a ring of 11 rows in registers, the
 *                     vertical 11-tap sums over the ring give one row of the SSIM map.  The squared differences are summed while
 *                     staging, every pixel by the one workgroup that owns it (the tile's own kCols x kRows pixels; the last tiles
 *                     also own the 10 border columns / rows).  SSIM = false is the same kernel without the tile and the filter: the
 *                     same pixels in the same order, so the same bits of the squared error.  Every workgroup writes its two sums
 *                     into a slot of its own.
 *   k_quality_reduce  one thread per SAI: the slots of every channel in order, then the channels in order.
 * Only two doubles per SAI go to the host, which forms the per-SAI values and the summary (lfbm5d_quality_summary: host only).
 * Precision: everything is a double sum (products of two floats are exact in double); determinism: no atomics, every sum in a
 * fixed order -- two calls, the device and host forms, and SSIM on / off (for the squared error) give the same bits.  The inputs
 * are only read; planes of empty SAIs are not touched.
 */
#include "lfbm5d_side.h"

using namespace lfbm5d_host;

namespace {

constexpr int kWin = 11;                         /* the SSIM window */
constexpr int kStrip = 64;                       /* window positions per row and wave: one per lane */
constexpr int kWaves = 4;
constexpr int kCols = kStrip * kWaves;           /* window positions per row of a workgroup's tile */
constexpr int kRows = 56;                        /* rows of window positions of a tile: kRows + kWin - 1 input rows = 6 chunks of kWin */
constexpr int kPitch = kCols + kWin - 1;         /* input columns of a tile */

struct Taps { double g[kWin]; };

/* grid (ac, xtiles, ytiles).  part[(((ac * ytiles + yt) * xtiles + xt) * 2 + {0, 1}] = {sum of (a - b)^2 over the pixels the workgroup
 * owns, sum of its SSIM map values}.  xtiles = ceil((W - 10) / kCols), ytiles = ceil((H - 10) / kRows) (1 when W / H <= 10: SSIM off). */
template <bool SSIM>
__global__ __launch_bounds__(256) void k_quality(const float* __restrict__ ref, const float* __restrict__ test, const unsigned* __restrict__ sai,
                                                 unsigned C, unsigned W, unsigned H, unsigned xtiles, unsigned ytiles, Taps taps, double c1,
                                                 double c2, double* __restrict__ part) {
    __shared__ double2 tile[SSIM ? kWin * kPitch : 1];
    __shared__ double red[kWaves][2];
    const unsigned ac = blockIdx.x, xt = blockIdx.y, yt = blockIdx.z;
    const size_t plane = ((size_t)sai[ac / C] * C + ac % C) * (size_t)W * H;
    const float* A = ref + plane;
    const float* B = test + plane;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned x0 = xt * kCols, y0 = yt * kRows;
    /* pixels owned: [y0, own_y1) x [x0, own_x1); input rows staged: [y0, y_end) (the last tiles reach the image's edge) */
    const unsigned own_x1 = xt + 1 == xtiles ? W : x0 + kCols, own_y1 = yt + 1 == ytiles ? H : y0 + kRows;
    const unsigned y_end = min(H, y0 + kRows + kWin - 1);
    const bool col_ok = x0 + wave * kStrip + lane + (kWin - 1) < W;   /* the lane's column holds window positions */
    double se = 0.0, ss = 0.0;
    double ring[kWin][5];

    auto stage = [&](unsigned k, unsigned col, unsigned y) {
        const unsigned x = x0 + col;
        const bool own = y < own_y1 && x < own_x1;
        double a = 0.0, b = 0.0;
        if (SSIM ? (y < y_end && x < W) : own) {
            a = (double)A[(size_t)y * W + x];
            b = (double)B[(size_t)y * W + x];
            if (own) { const double d = a - b; se = fma(d, d, se); }
        }
        if (SSIM) tile[k * kPitch + col] = make_double2(a, b);
    };

    for (unsigned yb = y0; yb < y_end; yb += kWin) {
        if (SSIM) __syncthreads();
#pragma unroll
        for (unsigned k = 0; k < kWin; k++) stage(k, tid, yb + k);
        if (tid < kWin * (kWin - 1)) stage(tid / (kWin - 1), kCols + tid % (kWin - 1), yb + tid / (kWin - 1));
        if (!SSIM) continue;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kWin; k++) {
            const unsigned y = yb + k;                    /* input row; its place in the ring is k (chunks start at y0) */
            if (y >= y_end) break;
            const double2* t = tile + k * kPitch + wave * kStrip + lane;
            double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < kWin; j++) {
                const double2 v = t[j];
                const double g = taps.g[j];
                h[0] = fma(g, v.x, h[0]);
                h[1] = fma(g, v.y, h[1]);
                h[2] = fma(g, v.x * v.x, h[2]);
                h[3] = fma(g, v.y * v.y, h[3]);
                h[4] = fma(g, v.x * v.y, h[4]);
            }
#pragma unroll
            for (int q = 0; q < 5; q++) ring[k][q] = h[q];
            if (y < y0 + kWin - 1) continue;              /* the ring is not full yet */
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      /* window row y - 10 + j sits in ring[(k + 1 + j) % kWin] */
#pragma unroll
            for (int j = 0; j < kWin; j++)
#pragma unroll
                for (int q = 0; q < 5; q++) v[q] = fma(taps.g[j], ring[(k + 1 + j) % kWin][q], v[q]);
            const double ma = v[0], mb = v[1];
            const double sa = v[2] - ma * ma, sb = v[3] - mb * mb, sab = v[4] - ma * mb;
            const double num = (2.0 * ma * mb + c1) * (2.0 * sab + c2);
            const double den = (ma * ma + mb * mb + c1) * (sa + sb + c2);
            if (col_ok) ss += num / den;
        }
    }
    /* fixed-order reduction: the wave's 64 lanes, then the four waves */
    for (int off = 32; off > 0; off >>= 1) {
        se += __shfl_down(se, off, 64);
        ss += __shfl_down(ss, off, 64);
    }
    if (lane == 0) { red[wave][0] = se; red[wave][1] = ss; }
    __syncthreads();
    if (tid == 0) {
        double e = 0.0, s = 0.0;
        for (int w = 0; w < kWaves; w++) { e += red[w][0]; s += red[w][1]; }
        double* p = part + (((size_t)ac * ytiles + yt) * xtiles + xt) * 2;
        p[0] = e;
        p[1] = s;
    }
}

/* out[2 k + {0, 1}] = the sums of SAI k (k-th non-empty SAI): per channel the slots in order, then the channels in order */
__global__ __launch_bounds__(64) void k_quality_reduce(const double* __restrict__ part, unsigned nne, unsigned C, unsigned slots,
                                                       double* __restrict__ out) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nne) return;
    double se = 0.0, ss = 0.0;
    for (unsigned c = 0; c < C; c++) {
        const double* p = part + ((size_t)k * C + c) * slots * 2;
        double e = 0.0, s = 0.0;
        for (unsigned i = 0; i < slots; i++) { e += p[2 * i]; s += p[2 * i + 1]; }
        se += e;
        ss += s;
    }
    out[2 * k] = se;
    out[2 * k + 1] = ss;
}

int summary(const double* mse, const double* ssim, const unsigned* mask, unsigned asize, double peak, lfbm5d_quality* out) {
    if (!mse || !mask || !out || !(peak >= 0.0) || !std::isfinite(peak)) return 1;
    const double pk = peak == 0.0 ? 255.0 : peak;
    unsigned cnt = 0;
    for (unsigned st = 0; st < asize; st++) cnt += mask[st] != 0;
    if (!cnt) return 1;
    auto psnr = [pk](double m) { return 10.0 * std::log10(pk * pk / m); };
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, var[3] = {0.0, 0.0, 0.0};
    for (unsigned st = 0; st < asize; st++) {
        if (!mask[st]) continue;
        sum[0] += psnr(mse[st]); sum[1] += std::sqrt(mse[st]); sum[2] += ssim ? ssim[st] : 0.0; sum[3] += mse[st];
    }
    const double n = (double)cnt, mp = sum[0] / n, mr = sum[1] / n, ms = sum[2] / n;
    for (unsigned st = 0; st < asize; st++) {
        if (!mask[st]) continue;
        const double dp = psnr(mse[st]) - mp, dr = std::sqrt(mse[st]) - mr, ds = (ssim ? ssim[st] : 0.0) - ms;
        var[0] += dp * dp; var[1] += dr * dr; var[2] += ds * ds;
    }
    std::memset(out, 0, sizeof(*out));
    out->psnr_mean = mp; out->psnr_std = std::sqrt(var[0] / n);
    out->rmse_mean = mr; out->rmse_std = std::sqrt(var[1] / n);
    out->ssim_mean = ms; out->ssim_std = std::sqrt(var[2] / n);
    out->mse = sum[3] / n;
    out->count = cnt;
    out->has_ssim = ssim ? 1u : 0u;
    return 0;
}

int quality(lfbm5d_ctx* c, const float* d_ref, const float* d_test, const float* const* h_ref, const float* const* h_test, const unsigned* h_mask,
            unsigned asize, unsigned W, unsigned H, unsigned C, double peak, int want_ssim, lfbm5d_quality* out, double* h_mse_sai,
            double* h_ssim_sai) {
    const bool host = h_ref || h_test;
    const std::string who = host ? "lfbm5d_quality_host_sai: " : "lfbm5d_quality_device: ";
    if (!h_mask || !out || (host ? (!h_ref || !h_test) : (!d_ref || !d_test))) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C)) return 1;
    if (!(peak >= 0.0) || !std::isfinite(peak)) return fail(c, who + "peak must be finite and not negative (0 = 255)");
    if (check_size(c, who, W, H, 1, "not be 0")) return 1;
    if (want_ssim && check_size(c, who, W, H, kWin, "be at least 11 for SSIM")) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    const std::vector<unsigned>& sai = c->side.sai_host;
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    const unsigned nne = (unsigned)sai.size(), nac = nne * C;
    const unsigned xtiles = W >= (unsigned)kWin ? (W - kWin + 1 + kCols - 1) / kCols : 1, ytiles = H >= (unsigned)kWin ? (H - kWin + 1 + kRows - 1) / kRows : 1;
    if (ytiles > 65535 || xtiles > 65535) return fail(c, who + "width or height too large");
    const size_t img = (size_t)C * W * H;
    lfbm5d_ctx::QualityBufs& Q = c->quality;
    HIPCK(c, Q.part.reserve((size_t)nac * xtiles * ytiles * 2 * sizeof(double)));
    HIPCK(c, Q.out.reserve((size_t)nne * 2 * sizeof(double)));
    const float *ref = d_ref, *test = d_test;
    if (host) {   /* stage the non-empty SAIs through HBM, at their places in [asize][C*H*W] */
        HIPCK(c, c->h2d_noisy.reserve((size_t)asize * img * sizeof(float)));
        HIPCK(c, c->h2d_basic.reserve((size_t)asize * img * sizeof(float)));
        if (upload_planes(c, who, h_ref, c->h2d_noisy.as<float>(), asize, img, nonempty)) return 1;
        if (upload_planes(c, who, h_test, c->h2d_basic.as<float>(), asize, img, nonempty)) return 1;
        ref = c->h2d_noisy.as<float>();
        test = c->h2d_basic.as<float>();
    }
    const unsigned* d_sai = c->side.sai.as<unsigned>();
    const double pk = peak == 0.0 ? 255.0 : peak;
    Taps taps;
    double gs = 0.0;
    for (int i = 0; i < kWin; i++) { taps.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); gs += taps.g[i]; }
    for (int i = 0; i < kWin; i++) taps.g[i] /= gs;
    const double c1 = (0.01 * pk) * (0.01 * pk), c2 = (0.03 * pk) * (0.03 * pk);
    const dim3 grid(nac, xtiles, ytiles);
    if (want_ssim)
        hipLaunchKernelGGL((k_quality<true>), grid, dim3(256), 0, c->stream, ref, test, d_sai, C, W, H, xtiles, ytiles, taps, c1, c2, Q.part.as<double>());
    else
        hipLaunchKernelGGL((k_quality<false>), grid, dim3(256), 0, c->stream, ref, test, d_sai, C, W, H, xtiles, ytiles, taps, c1, c2, Q.part.as<double>());
    hipLaunchKernelGGL(k_quality_reduce, dim3((nne + 63) / 64), dim3(64), 0, c->stream, Q.part.as<double>(), nne, C, xtiles * ytiles, Q.out.as<double>());
    HIPCK(c, hipGetLastError());
    std::vector<double> sums((size_t)nne * 2);
    HIPCK(c, hipMemcpyAsync(sums.data(), Q.out.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));

    std::vector<double> mse(asize, 0.0), ssim(asize, 0.0);
    const double n_px = (double)C * (double)W * (double)H;
    const double n_pos = want_ssim ? (double)C * (double)(W - kWin + 1) * (double)(H - kWin + 1) : 1.0;
    for (unsigned k = 0; k < nne; k++) { mse[sai[k]] = sums[2 * k] / n_px; ssim[sai[k]] = sums[2 * k + 1] / n_pos; }
    if (summary(mse.data(), want_ssim ? ssim.data() : nullptr, h_mask, asize, peak, out)) return fail(c, who + "summary failed");
    if (h_mse_sai) std::memcpy(h_mse_sai, mse.data(), asize * sizeof(double));
    if (h_ssim_sai) std::memcpy(h_ssim_sai, ssim.data(), asize * sizeof(double));
    return 0;
}

} /* namespace */

extern "C" {

int lfbm5d_quality_summary(const double* h_mse_sai, const double* h_ssim_sai, const unsigned* h_mask, unsigned asize, double peak,
                           lfbm5d_quality* out) {
    return summary(h_mse_sai, h_ssim_sai, h_mask, asize, peak, out);
}

int lfbm5d_quality_device(lfbm5d_ctx* c, const float* d_ref, const float* d_test, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                          unsigned C, double peak, int want_ssim, lfbm5d_quality* out, double* h_mse_sai, double* h_ssim_sai) {
    if (!c) return 1;
    return quality(c, d_ref, d_test, nullptr, nullptr, h_mask, asize, W, H, C, peak, want_ssim, out, h_mse_sai, h_ssim_sai);
}

int lfbm5d_quality_host_sai(lfbm5d_ctx* c, const float* const* h_ref, const float* const* h_test, const unsigned* h_mask, unsigned asize,
                            unsigned W, unsigned H, unsigned C, double peak, int want_ssim, lfbm5d_quality* out, double* h_mse_sai,
                            double* h_ssim_sai) {
    if (!c) return 1;
    if (!h_ref || !h_test) return fail(c, "lfbm5d_quality_host_sai: NULL pointer for a required buffer");
    return quality(c, nullptr, nullptr, h_ref, h_test, h_mask, asize, W, H, C, peak, want_ssim, out, h_mse_sai, h_ssim_sai);
}

} /* extern "C" */
