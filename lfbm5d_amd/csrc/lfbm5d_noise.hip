/*
 * lfbm5d_noise.hip -- blind estimate of the level of additive white Gaussian noise in a light field (lfbm5d_noise_level_*,
 * include/lfbm5d.h): the PCA statistic of Chen, Zhu & Heng, "An Efficient Statistical Method for Image Noise Level Estimation"
 * (ICCV 2015), pooled over the sub-aperture images.  Not in the reference, which needs sigma from its caller.
 *
 * For every non-empty SAI a and channel c the r x r patches at stride 1 give n = (H-r+1)(W-r+1), s = sum x, S = sum x x^T and the
 * centred scatter M = S - s s^T / n; the pooled covariances are sums of M over (a, c), over a, or over c, divided by the patches.
 *
 * Lag form.  S[(u1,v1),(u2,v2)] is the sum of P_L(y,x) = I(y,x) I(y+du,x+dv), L = (du,dv) = (u2-u1,v2-v1), over the rectangle
 * [u1, u1+H-r] x [v1, v1+W-r] (I is zero outside the image; no product a rectangle holds touches the outside).  Rows fall into
 * 2r-1 classes -- the top r-1 rows one by one, the middle rows, the bottom r-1 rows one by one -- and so do columns; every
 * rectangle is the union of r x r consecutive cells of that grid.  So the work is one sum per (lag, cell): r + (r-1)(2r-1)
 * = 113 products per pixel for r = 8 (the lags with du > 0, or du = 0 and dv >= 0: S is symmetric), plus the plain sums of I for
 * s (one more "lag").  Kernels, in stream order:
 *   k_noise_bulk      every pixel, every lag: the sum over the whole image, per column strip of 64 pixels (one lane per column, the
 *                     lags split over the workgroup's four waves, the strip's rows staged through LDS as doubles)
 *   k_noise_edges     the cells of the 2(r-1) border rows (all 2r-1 column classes) and of the 2(r-1) border columns (middle rows)
 *   k_noise_assemble  middle x middle cell = whole image - border cells; then M (d x d) of the (SAI, channel)
 *   k_noise_pool      the light field's, every channel's and (on request) every SAI's covariance
 * Only the pooled d x d matrices go to the host, which finds the eigenvalues (Householder tridiagonalisation + implicit QL, double).
 * Precision: products of float pixels are exact in double and every sum is a double sum, so the centring S - s s^T / n (which
 * cancels about 14 bits) leaves ~1e-12 relative.  Determinism: every sum runs in a fixed order (no atomics): two calls, and the
 * device and host forms, give the same bits.  The input is only read.
 */
#include "lfbm5d_side.h"

using namespace lfbm5d_host;

namespace {

constexpr int kStrip = 64;        /* columns of a bulk strip: one per lane */
constexpr int kChunk = 32;        /* rows of a strip staged at a time */

/* lag l -> (du, dv): l < r: (0, l); then du = 1..r-1 with dv = -(r-1)..r-1.  The last index (n_lags - 1) is the plain sum. */
__host__ __device__ constexpr int n_lags(int R) { return R + (R - 1) * (2 * R - 1) + 1; }
__host__ __device__ constexpr int lag_du(int R, int l) { return l < R ? 0 : 1 + (l - R) / (2 * R - 1); }
__host__ __device__ constexpr int lag_dv(int R, int l) { return l < R ? l : (l - R) % (2 * R - 1) - (R - 1); }
__host__ __device__ constexpr int lag_index(int R, int du, int dv) { return du == 0 ? dv : R + (du - 1) * (2 * R - 1) + dv + R - 1; }

__device__ __forceinline__ const float* plane(const float* lf, const unsigned* sai, unsigned C, unsigned W, unsigned H, unsigned ac) {
    return lf + ((size_t)sai[ac / C] * C + ac % C) * (size_t)W * H;
}

/* one wave's lags over one staged chunk: acc[i] += I(y,x) * I(y+du,x+dv) for the wave's lags, every row of the chunk */
template <int R, int WV>
__device__ __forceinline__ void bulk_rows(const double* tile, int lane, double* acc) {
    constexpr int NL = n_lags(R), PER = (NL + 3) / 4, PITCH = kStrip + 2 * (R - 1);
    for (int ty = 0; ty < kChunk; ty++) {
        const double* t = tile + ty * PITCH + lane + (R - 1);
        const double a = t[0];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int l = WV * PER + i;
            if (l < NL - 1) acc[i] = fma(a, t[lag_du(R, l) * PITCH + lag_dv(R, l)], acc[i]);
            else if (l == NL - 1) acc[i] += a;
        }
    }
}

/* grid (ac, strip), 256 threads.  part[(ac * nstrips + strip) * NL + l] = sum over the strip's columns and every row of P_l. */
template <int R>
__global__ __launch_bounds__(256) void k_noise_bulk(const float* __restrict__ lf, const unsigned* __restrict__ sai, unsigned C, unsigned W,
                                                    unsigned H, unsigned nstrips, double* __restrict__ part) {
    constexpr int NL = n_lags(R), PER = (NL + 3) / 4, PITCH = kStrip + 2 * (R - 1), ROWS = kChunk + R - 1;
    __shared__ double tile[ROWS * PITCH];
    const unsigned ac = blockIdx.x, strip = blockIdx.y;
    const float* img = plane(lf, sai, C, W, H, ac);
    const int x0 = (int)strip * kStrip - (R - 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) acc[i] = 0.0;
    for (int y0 = 0; y0 < (int)H; y0 += kChunk) {
        __syncthreads();
        for (int i = threadIdx.x; i < ROWS * PITCH; i += 256) {
            const int y = y0 + i / PITCH, x = x0 + i % PITCH;
            tile[i] = (y < (int)H && x >= 0 && x < (int)W) ? (double)img[(size_t)y * W + x] : 0.0;
        }
        __syncthreads();
        switch (wave) {
            case 0: bulk_rows<R, 0>(tile, lane, acc); break;
            case 1: bulk_rows<R, 1>(tile, lane, acc); break;
            case 2: bulk_rows<R, 2>(tile, lane, acc); break;
            default: bulk_rows<R, 3>(tile, lane, acc); break;
        }
    }
    /* fixed-order reduction over the wave's 64 columns */
#pragma unroll
    for (int i = 0; i < PER; i++) {
        double v = acc[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        const int l = wave * PER + i;
        if (lane == 0 && l < NL) part[((size_t)ac * nstrips + strip) * NL + l] = v;
    }
}

/* grid (ac, line), one thread per lag.  Lines 0 .. 2(r-1)-1: border rows (top rows, then bottom rows), each gives the 2r-1 column
 * cells of its row class; lines 2(r-1) .. 4(r-1)-1: border columns (left, then right), each gives its column's cell of the middle
 * rows.  cells[(ac * NL + l) * K * K + row class * K + column class], K = 2r-1. */
template <int R>
__global__ __launch_bounds__(128) void k_noise_edges(const float* __restrict__ lf, const unsigned* __restrict__ sai, unsigned C, unsigned W,
                                                     unsigned H, double* __restrict__ cells) {
    constexpr int NL = n_lags(R), K = 2 * R - 1;
    const unsigned ac = blockIdx.x, line = blockIdx.y;
    const int l = threadIdx.x;
    if (l >= NL) return;
    const float* img = plane(lf, sai, C, W, H, ac);
    const bool plain = l == NL - 1;
    const int du = plain ? 0 : lag_du(R, l), dv = plain ? 0 : lag_dv(R, l);
    const int iW = (int)W, iH = (int)H;
    auto p = [&](int y, int x) -> double {   /* (y, x) inside the image; the partner may be outside (zero) */
        const double a = (double)img[(size_t)y * W + x];
        if (plain) return a;
        const int y2 = y + du, x2 = x + dv;
        return (y2 < iH && x2 >= 0 && x2 < iW) ? a * (double)img[(size_t)y2 * W + x2] : 0.0;
    };
    double* G = cells + ((size_t)ac * NL + l) * K * K;
    if (line < 2 * (R - 1)) {
        const int k = line < R - 1 ? (int)line : (int)line + 1;          /* row class */
        const int y = k < R - 1 ? k : iH - 2 * R + 1 + k;
        for (int j = 0; j < R - 1; j++) G[k * K + j] = p(y, j);
        double s = 0.0;
        for (int x = R - 1; x <= iW - R; x++) s += p(y, x);
        G[k * K + R - 1] = s;
        for (int j = R; j < K; j++) G[k * K + j] = p(y, iW - 2 * R + 1 + j);
    } else {
        const int q = (int)line - 2 * (R - 1);
        const int k = q < R - 1 ? q : q + 1;                            /* column class */
        const int x = k < R - 1 ? k : iW - 2 * R + 1 + k;
        double s = 0.0;
        for (int y = R - 1; y <= iH - R; y++) s += p(y, x);
        G[(R - 1) * K + k] = s;
    }
}

template <int R>
__device__ __forceinline__ double rect(const double* G, int u1, int v1) {
    constexpr int K = 2 * R - 1;
    double s = 0.0;
    for (int a = 0; a < R; a++)
        for (int b = 0; b < R; b++) s += G[(u1 + a) * K + v1 + b];
    return s;
}

/* grid (ac), 256 threads: the middle cell of every lag, then M = S - s s^T / n, [ac][d][d] (both triangles, bitwise symmetric). */
template <int R>
__global__ __launch_bounds__(256) void k_noise_assemble(const double* __restrict__ part, unsigned nstrips, double* __restrict__ cells, unsigned W,
                                                        unsigned H, double* __restrict__ M) {
    constexpr int NL = n_lags(R), K = 2 * R - 1, D = R * R;
    __shared__ double sv[D];
    const unsigned ac = blockIdx.x;
    double* Gac = cells + (size_t)ac * NL * K * K;
    for (int l = threadIdx.x; l < NL; l += blockDim.x) {
        double T = 0.0;
        for (unsigned s = 0; s < nstrips; s++) T += part[((size_t)ac * nstrips + s) * NL + l];
        double* G = Gac + (size_t)l * K * K;
        double b = 0.0;
        for (int k = 0; k < K; k++)
            if (k != R - 1)
                for (int j = 0; j < K; j++) b += G[k * K + j];
        for (int j = 0; j < K; j++)
            if (j != R - 1) b += G[(R - 1) * K + j];
        G[(R - 1) * K + R - 1] = T - b;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += blockDim.x) sv[i] = rect<R>(Gac + (size_t)(NL - 1) * K * K, i / R, i % R);
    __syncthreads();
    const double n = (double)(H - R + 1) * (double)(W - R + 1);
    double* Mac = M + (size_t)ac * D * D;
    for (int e = threadIdx.x; e < D * D; e += blockDim.x) {
        const int i = e / D, j = e % D, i0 = min(i, j), j0 = max(i, j);
        const int u1 = i0 / R, v1 = i0 % R, u2 = j0 / R, v2 = j0 % R;
        const double S = rect<R>(Gac + (size_t)lag_index(R, u2 - u1, v2 - v1) * K * K, u1, v1);
        Mac[e] = S - sv[i] * sv[j] / n;
    }
}

/* grid (entry blocks, matrix): matrix 0 = the light field (every (SAI, channel)), 1..C = channel c - 1 (every SAI), C+1.. = SAI k
 * (every channel).  Sums in (SAI, channel) order, divided by the patches pooled. */
__global__ __launch_bounds__(256) void k_noise_pool(const double* __restrict__ M, unsigned nne, unsigned C, unsigned DD, double n,
                                                    double* __restrict__ out) {
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (e >= DD) return;
    double s = 0.0, cnt;
    if (m == 0) {
        for (unsigned ac = 0; ac < nne * C; ac++) s += M[(size_t)ac * DD + e];
        cnt = (double)nne * C * n;
    } else if (m <= C) {
        for (unsigned k = 0; k < nne; k++) s += M[((size_t)k * C + m - 1) * DD + e];
        cnt = (double)nne * n;
    } else {
        const unsigned k = m - 1 - C;
        for (unsigned c = 0; c < C; c++) s += M[((size_t)k * C + c) * DD + e];
        cnt = (double)C * n;
    }
    out[(size_t)m * DD + e] = s / cnt;
}

template <int R>
void launch(hipStream_t st, const float* lf, const unsigned* sai, unsigned nac, unsigned C, unsigned W, unsigned H, unsigned nstrips,
            double* part, double* cells, double* M) {
    hipLaunchKernelGGL((k_noise_bulk<R>), dim3(nac, nstrips), dim3(256), 0, st, lf, sai, C, W, H, nstrips, part);
    hipLaunchKernelGGL((k_noise_edges<R>), dim3(nac, 4 * (R - 1)), dim3(128), 0, st, lf, sai, C, W, H, cells);
    hipLaunchKernelGGL((k_noise_assemble<R>), dim3(nac), dim3(256), 0, st, part, nstrips, cells, W, H, M);
}

/* ---- host: eigenvalues of a symmetric matrix (Householder reduction to tridiagonal form, then QL with implicit shifts) ---- */
bool sym_eigenvalues(unsigned n, const double* A, double* w) {
    std::vector<double> a(A, A + (size_t)n * n), e(n, 0.0);
    double* d = w;
    auto at = [&](unsigned i, unsigned j) -> double& { return a[(size_t)i * n + j]; };
    for (unsigned i = n - 1; i > 0; i--) {
        const unsigned l = i - 1;
        double h = 0.0;
        if (l > 0) {
            double scale = 0.0;
            for (unsigned k = 0; k <= l; k++) scale += std::fabs(at(i, k));
            if (scale == 0.0) e[i] = at(i, l);
            else {
                for (unsigned k = 0; k <= l; k++) { at(i, k) /= scale; h += at(i, k) * at(i, k); }
                double f = at(i, l);
                double g = f >= 0.0 ? -std::sqrt(h) : std::sqrt(h);
                e[i] = scale * g;
                h -= f * g;
                at(i, l) = f - g;
                f = 0.0;
                for (unsigned j = 0; j <= l; j++) {
                    g = 0.0;
                    for (unsigned k = 0; k <= j; k++) g += at(j, k) * at(i, k);
                    for (unsigned k = j + 1; k <= l; k++) g += at(k, j) * at(i, k);
                    e[j] = g / h;
                    f += e[j] * at(i, j);
                }
                const double hh = f / (h + h);
                for (unsigned j = 0; j <= l; j++) {
                    f = at(i, j);
                    e[j] = g = e[j] - hh * f;
                    for (unsigned k = 0; k <= j; k++) at(j, k) -= f * e[k] + g * at(i, k);
                }
            }
        } else e[i] = at(i, l);
    }
    for (unsigned i = 0; i < n; i++) d[i] = at(i, i);
    for (unsigned i = 1; i < n; i++) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    const double eps = 2.220446049250313e-16;
    for (unsigned l = 0; l < n; l++) {
        int iter = 0;
        unsigned m;
        do {
            for (m = l; m + 1 < n; m++) {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= eps * dd) break;
            }
            if (m != l) {
                if (iter++ == 60) return false;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = (int)m - 1; i >= (int)l; i--) {
                    double f = s * e[i], b = c * e[i];
                    e[i + 1] = (r = std::hypot(f, g));
                    if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }
                    s = f / r; c = g / r; g = d[i + 1] - p; r = (d[i] - g) * s + 2.0 * c * b;
                    d[i + 1] = g + (p = s * r); g = c * r - b;
                }
                if (r == 0.0 && i >= (int)l) continue;
                d[l] -= p; e[l] = g; e[m] = 0.0;
            }
        } while (m != l);
    }
    std::sort(w, w + n);
    return true;
}

/* the statistic of include/lfbm5d.h on ascending eigenvalues: the largest m whose mean splits lambda_1..m evenly */
void split_statistic(unsigned d, const double* lam, double* sigma, unsigned* comps) {
    double sum = 0.0;
    for (unsigned i = 0; i < d; i++) sum += lam[i];
    for (unsigned m = d; m >= 1; m--) {
        const double mu = sum / m;
        unsigned above = 0, below = 0;
        for (unsigned i = 0; i < m; i++) { above += lam[i] > mu; below += lam[i] < mu; }
        if (above == below || m == 1) { *sigma = std::sqrt(std::max(mu, 0.0)); *comps = m; return; }
        sum -= lam[m - 1];
    }
}

int noise_level(lfbm5d_ctx* c, const float* d_lf, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                unsigned C, unsigned patch, lfbm5d_noise_level* out, double* h_sigma_sai, double* h_eigen) {
    const std::string who = h_lf ? "lfbm5d_noise_level_host_sai: " : "lfbm5d_noise_level_device: ";
    if (!h_mask || !out || (!d_lf && !h_lf)) return fail(c, who + "NULL pointer for a required buffer");
    const unsigned R = patch ? patch : 8;
    if (check_chnls(c, who, C)) return 1;
    if (R < 4 || R > 8) return fail(c, who + "patch must be 4..8 (0 = 8)");
    if (check_size(c, who, W, H, 2 * R, "be at least twice the patch")) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    const std::vector<unsigned>& sai = c->side.sai_host;
    const unsigned nne = (unsigned)sai.size(), nac = nne * C, D = R * R, DD = D * D, NL = (unsigned)n_lags((int)R), K = 2 * R - 1;
    const unsigned nstrips = (W + kStrip - 1) / kStrip, nmat = 1 + C + (h_sigma_sai ? nne : 0);
    const size_t img = (size_t)C * W * H;
    lfbm5d_ctx::NoiseBufs& B = c->noise;
    HIPCK(c, B.part.reserve((size_t)nac * nstrips * NL * sizeof(double)));
    HIPCK(c, B.cells.reserve((size_t)nac * NL * K * K * sizeof(double)));
    HIPCK(c, B.m.reserve((size_t)nac * DD * sizeof(double)));
    HIPCK(c, B.pool.reserve((size_t)nmat * DD * sizeof(double)));
    const float* lf = d_lf;
    if (h_lf) {   /* stage the non-empty SAIs through HBM, at their places in [asize][C*H*W] */
        HIPCK(c, c->h2d_noisy.reserve((size_t)asize * img * sizeof(float)));
        if (upload_planes(c, who, h_lf, c->h2d_noisy.as<float>(), asize, img, [&](unsigned st) { return h_mask[st] != 0; })) return 1;
        lf = c->h2d_noisy.as<float>();
    }
    const unsigned* ds = c->side.sai.as<unsigned>();
    double *part = B.part.as<double>(), *cells = B.cells.as<double>(), *M = B.m.as<double>();
    switch (R) {
        case 4: launch<4>(c->stream, lf, ds, nac, C, W, H, nstrips, part, cells, M); break;
        case 5: launch<5>(c->stream, lf, ds, nac, C, W, H, nstrips, part, cells, M); break;
        case 6: launch<6>(c->stream, lf, ds, nac, C, W, H, nstrips, part, cells, M); break;
        case 7: launch<7>(c->stream, lf, ds, nac, C, W, H, nstrips, part, cells, M); break;
        default: launch<8>(c->stream, lf, ds, nac, C, W, H, nstrips, part, cells, M); break;
    }
    const double n = (double)(H - R + 1) * (double)(W - R + 1);
    hipLaunchKernelGGL(k_noise_pool, dim3((DD + 255) / 256, nmat), dim3(256), 0, c->stream, M, nne, C, DD, n, B.pool.as<double>());
    HIPCK(c, hipGetLastError());
    std::vector<double> cov((size_t)nmat * DD);
    HIPCK(c, hipMemcpyAsync(cov.data(), B.pool.p, cov.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));

    /* eigenvalues and the statistic of every pooled matrix; the per-SAI ones on a few threads */
    std::vector<double> lam((size_t)nmat * D), sig(nmat, 0.0);
    std::vector<unsigned> comps(nmat, 0);
    std::vector<char> ok(nmat, 1);
    auto solve = [&](unsigned i) {
        ok[i] = sym_eigenvalues(D, &cov[(size_t)i * DD], &lam[(size_t)i * D]);
        if (ok[i]) split_statistic(D, &lam[(size_t)i * D], &sig[i], &comps[i]);
    };
    {
        const unsigned nt = std::min(8u, std::max(1u, std::min(nmat / 32, std::thread::hardware_concurrency())));
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back([&, t]() { for (unsigned i = t; i < nmat; i += nt) solve(i); });
        for (unsigned i = 0; i < nmat; i += nt) solve(i);
        for (auto& x : th) x.join();
    }
    for (unsigned i = 0; i < nmat; i++) if (!ok[i]) return fail(c, who + "eigenvalue iteration did not converge");
    std::memset(out, 0, sizeof(*out));
    out->sigma = sig[0];
    for (unsigned ch = 0; ch < C; ch++) out->sigma_channel[ch] = sig[1 + ch];
    out->components = comps[0];
    out->patch = R;
    out->patches = (unsigned long long)nac * (unsigned long long)(H - R + 1) * (unsigned long long)(W - R + 1);
    if (h_eigen) std::memcpy(h_eigen, lam.data(), D * sizeof(double));
    if (h_sigma_sai) {
        for (unsigned st = 0; st < asize; st++) h_sigma_sai[st] = 0.0;
        for (unsigned k = 0; k < nne; k++) h_sigma_sai[sai[k]] = sig[1 + C + k];
    }
    return 0;
}

} /* namespace */

extern "C" {

int lfbm5d_noise_level_statistic(unsigned d, const double* cov, double* sigma, unsigned* components, double* h_eigen) {
    if (d < 1 || d > 64 || !cov || !sigma || !components) return 1;
    std::vector<double> lam(d);
    if (!sym_eigenvalues(d, cov, lam.data())) return 1;
    split_statistic(d, lam.data(), sigma, components);
    if (h_eigen) std::memcpy(h_eigen, lam.data(), d * sizeof(double));
    return 0;
}

int lfbm5d_noise_level_device(lfbm5d_ctx* c, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                              unsigned patch, lfbm5d_noise_level* out, double* h_sigma_sai, double* h_eigen) {
    if (!c) return 1;
    if (!d_lf) return fail(c, "lfbm5d_noise_level_device: NULL pointer for a required buffer");
    return noise_level(c, d_lf, nullptr, h_mask, asize, W, H, C, patch, out, h_sigma_sai, h_eigen);
}

int lfbm5d_noise_level_host_sai(lfbm5d_ctx* c, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                unsigned C, unsigned patch, lfbm5d_noise_level* out, double* h_sigma_sai, double* h_eigen) {
    if (!c) return 1;
    if (!h_lf) return fail(c, "lfbm5d_noise_level_host_sai: NULL pointer for a required buffer");
    return noise_level(c, nullptr, h_lf, h_mask, asize, W, H, C, patch, out, h_sigma_sai, h_eigen);
}

} /* extern "C" */
