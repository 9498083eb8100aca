/*
 * lfbm5d_resample.hip -- light-field super-resolution on the hard-thresholding step (lfbm5d_sr_* / lfbm5d_superres_*,
 * include/lfbm5d.h): the scheme of SR-LFBM5D (Alain & Smolic, "Light Field Super-Resolution via LFBM5D Sparse Coding", ICIP 2018) --
 * iterative back-projection whose regulariser is the basic estimate of run_bm5d_1st_step with a falling sigma -- with the
 * resampling operators defined in include/lfbm5d.h.  It is NOT the output of the reference's SR branch, whose blur models and
 * stopping rule are not reproduced.
 *
 * Operators.  U (bicubic, low -> high) and D (antialiased bicubic or Gaussian blur + decimation, high -> low) are separable; a 1-D
 * operator from n_in to n_out samples is a tap table first[n_out], w[n_out][T] built on the host in double and rounded to float:
 *   out[X] = sum_{t < T} w[X][t] * in[clamp(first[X] + t, 0, n_in - 1)],   t ascending, float32
 * (the clamp happens at read time, weights are not merged).  The 2-D operator is Ry * plane * Rx^T, horizontal pass first.
 *
 * Kernel.  k_resample: one launch applies an operator to every plane of every non-empty SAI.  A workgroup of 256 threads (four
 * waves, a wave = 64 output columns) makes a 64 x 16 output tile: it stages the tile's tap rows in LDS, runs the
 * horizontal pass over the input rows the tile's vertical taps reach (for D: scale x 16 rows + T - 1) from global memory into
 * LDS, then the vertical pass out of LDS, and stores one coalesced row of 64 floats per wave.  The horizontal intermediate never
 * reaches memory.  Epilogues fused into the store make one back-projection two launches:
 *   kResidual  r = y - D x          (aux = y, low resolution)
 *   kUpdate    z = x + beta * U r   (aux = x, high resolution; z may be x itself: an output element reads aux at its own index only)
 * No atomics, every sum in a fixed order: repeated calls return the same bits.  Planes of empty SAIs are neither read nor written.
 */
#include "lfbm5d_side.h"

using namespace lfbm5d_host;

namespace {

constexpr int kTileW = 64, kMaxT = 32;
/* rows of an output tile and the input rows its vertical taps may reach (the LDS intermediate): D reads scale x rows + T - 1 input
 * rows (scale 4, T 32), U rows / scale + 4; both operators run the same instantiation */
constexpr int kDownH = 16, kDownRows = 4 * kDownH + kMaxT - 1, kUpH = kDownH, kUpRows = kDownRows;
enum { kPlain = 0, kResidual = 1, kUpdate = 2 };

struct SrOp {
    const int* fx; const float* wx; const int* fy; const float* wy;   /* device tables: columns (n_in = win), rows (n_in = hin) */
    unsigned Tx, Ty, win, hin, wout, hout;
};

template <int MODE, int kTileH, int kMaxRows, int kMaxT>
__global__ __launch_bounds__(256) void k_resample(SrOp op, const float* in, float* out, const float* aux, float beta,
                                                  const unsigned* __restrict__ sai, unsigned C) {
    __shared__ float tmp[kMaxRows * kTileW];
    __shared__ float s_wx[kMaxT * kTileW];
    __shared__ float s_wy[kMaxT * kTileH];
    __shared__ int s_fx[kTileW], s_fy[kTileH];
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const unsigned p = blockIdx.z;
    const size_t pl = (size_t)sai[p / C] * C + p % C;
    const float* src = in + pl * (size_t)op.win * op.hin;
    const int X0 = blockIdx.x * kTileW, Y0 = blockIdx.y * kTileH;
    const int X = X0 + lx, iw = (int)op.win, ih = (int)op.hin;
    const int Tx = (int)op.Tx, Ty = (int)op.Ty;
    const int ny = min(kTileH, (int)op.hout - Y0);
    const bool col = X < (int)op.wout;

    if (ly == 0) s_fx[lx] = col ? op.fx[X] : 0;
    for (int t = ly; t < Tx; t += 4) s_wx[t * kTileW + lx] = col ? op.wx[(size_t)X * Tx + t] : 0.0f;
    for (int i = threadIdx.x; i < Ty * kTileH; i += 256) {
        const int t = i / kTileH, y = i % kTileH;
        s_wy[i] = y < ny ? op.wy[(size_t)(Y0 + y) * Ty + t] : 0.0f;
    }
    if (threadIdx.x < kTileH) s_fy[threadIdx.x] = op.fy[Y0 + min((int)threadIdx.x, ny - 1)];
    /* input rows the tile reaches: first[] ascends with the output index */
    const int rlo = min(max(op.fy[Y0], 0), ih - 1);
    const int rhi = min(max(op.fy[Y0 + ny - 1] + Ty - 1, 0), ih - 1);
    const int nrows = min(rhi - rlo + 1, kMaxRows);
    __syncthreads();

    const int fx = s_fx[lx];
    for (int r = ly; r < nrows; r += 4) {
        const float* row = src + (size_t)(rlo + r) * iw;
        float acc = 0.0f;
        if (col)
            for (int t = 0; t < Tx; t++) acc = fmaf(s_wx[t * kTileW + lx], row[min(max(fx + t, 0), iw - 1)], acc);
        tmp[r * kTileW + lx] = acc;
    }
    __syncthreads();

    if (!col) return;
    for (int y = ly; y < ny; y += 4) {
        const int fy = s_fy[y];
        float acc = 0.0f;
        for (int t = 0; t < Ty; t++) {
            const int r = min(min(max(fy + t, 0), ih - 1) - rlo, nrows - 1);
            acc = fmaf(s_wy[t * kTileH + y], tmp[r * kTileW + lx], acc);
        }
        const size_t o = pl * (size_t)op.wout * op.hout + (size_t)(Y0 + y) * op.wout + X;
        if (MODE == kResidual) acc = aux[o] - acc;
        else if (MODE == kUpdate) acc = fmaf(beta, acc, aux[o]);
        out[o] = acc;
    }
}

/* ---- host: the tap tables of include/lfbm5d.h, in double ---- */
double keys(double x) {   /* Keys cubic, a = -0.5 */
    x = std::fabs(x);
    if (x <= 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}

const char* check_operator(const lfbm5d_sr_params* sr) {
    if (!sr) return "NULL pointer for the super-resolution parameters";
    if (sr->scale < 2 || sr->scale > 4) return "scale must be 2, 3 or 4";
    if (sr->kernel != LFBM5D_SR_BICUBIC && sr->kernel != LFBM5D_SR_GAUSSIAN) return "kernel must be LFBM5D_SR_BICUBIC or LFBM5D_SR_GAUSSIAN";
    if (sr->kernel == LFBM5D_SR_GAUSSIAN && !(sr->blur_sigma > 0.0f && sr->blur_sigma <= 5.0f)) return "blur_sigma must lie in (0, 5]";
    return nullptr;
}
const char* check_beta(const lfbm5d_sr_params* sr) {
    return (sr->beta > 0.0f && sr->beta <= 2.0f) ? nullptr : "beta must lie in (0, 2]";
}
const char* check_loop(const lfbm5d_sr_params* sr) {
    if (sr->iterations == 0) return "iterations must be at least 1";
    if (!(sr->sigma_start > 0.0f) || !(sr->sigma_end > 0.0f)) return "sigma_start and sigma_end must be positive";
    if (sr->sigma_end > sr->sigma_start) return "sigma_end must not exceed sigma_start";
    return check_beta(sr);
}

/* first[n_out], w[n_out][T] of one 1-D operator; returns false when n_in does not fit the operator */
bool build_taps(unsigned op, const lfbm5d_sr_params* sr, unsigned n_in, std::vector<int>& first, std::vector<float>& w, unsigned& T) {
    const unsigned s = sr->scale;
    if (n_in == 0) return false;
    if (op == LFBM5D_SR_UP) {
        const unsigned n_out = n_in * s;
        T = 4;
        first.resize(n_out); w.resize((size_t)n_out * T);
        for (unsigned X = 0; X < n_out; X++) {
            const double u = ((double)X + 0.5) / (double)s - 0.5;
            const int f = (int)std::floor(u) - 1;
            first[X] = f;
            for (unsigned t = 0; t < T; t++) w[(size_t)X * T + t] = (float)keys(u - (double)(f + (int)t));
        }
        return true;
    }
    if (op != LFBM5D_SR_DOWN || n_in % s) return false;
    const unsigned n_out = n_in / s;
    const bool gauss = sr->kernel == LFBM5D_SR_GAUSSIAN;
    const double sb = (double)sr->blur_sigma, R = gauss ? std::ceil(3.0 * sb) : 2.0 * (double)s;
    std::vector<std::vector<double> > rows(n_out);
    first.resize(n_out);
    T = 0;
    for (unsigned x = 0; x < n_out; x++) {
        const double u = ((double)x + 0.5) * (double)s - 0.5;
        const int j0 = (int)std::ceil(u - R), j1 = (int)std::floor(u + R);
        first[x] = j0;
        std::vector<double>& r = rows[x];
        double sum = 0.0;
        for (int j = j0; j <= j1; j++) {
            const double d = u - (double)j;
            r.push_back(gauss ? std::exp(-(d * d) / (2.0 * sb * sb)) : keys(d / (double)s));
            sum += r.back();
        }
        for (double& v : r) v /= sum;
        T = std::max(T, (unsigned)r.size());
    }
    if (T > (unsigned)kMaxT) return false;
    w.assign((size_t)n_out * T, 0.0f);
    for (unsigned x = 0; x < n_out; x++)
        for (size_t t = 0; t < rows[x].size(); t++) w[(size_t)x * T + t] = (float)rows[x][t];
    return true;
}

/* the tables of both operators for one geometry on the device, and the list of non-empty SAIs; rebuilt when the key changes */
int ensure(lfbm5d_ctx* c, const char* who, const lfbm5d_sr_params* sr, const unsigned* h_mask, unsigned asize, unsigned w, unsigned h,
           unsigned C, SrOp& up, SrOp& down, unsigned& nne) {
    if (!h_mask) return fail(c, std::string(who) + "NULL pointer for a required buffer");
    if (const char* m = check_operator(sr)) return fail(c, std::string(who) + m);
    if (check_chnls(c, who, C)) return 1;
    if (w == 0 || h == 0 || asize == 0) return fail(c, std::string(who) + "empty light field");
    lfbm5d_ctx::SrBufs& B = c->sr;
    if (sai_list(c, who, h_mask, asize)) return 1;
    nne = (unsigned)c->side.sai_host.size();
    if ((size_t)nne * C > 65535) return fail(c, std::string(who) + "more than 65535 planes");
    unsigned bits; std::memcpy(&bits, &sr->blur_sigma, sizeof(bits));
    const unsigned key[5] = {sr->scale, sr->kernel, sr->kernel == LFBM5D_SR_GAUSSIAN ? bits : 0u, w, h};
    const unsigned s = sr->scale, W = w * s, H = h * s;
    if (!B.tab.p || std::memcmp(key, B.key, sizeof(key))) {
        std::vector<int> f[4]; std::vector<float> wt[4]; unsigned T[4];
        const unsigned ops[4] = {LFBM5D_SR_UP, LFBM5D_SR_UP, LFBM5D_SR_DOWN, LFBM5D_SR_DOWN}, nin[4] = {w, h, W, H};
        size_t words = 0;
        for (int i = 0; i < 4; i++) {
            if (!build_taps(ops[i], sr, nin[i], f[i], wt[i], T[i])) return fail(c, std::string(who) + "tap table longer than 32");
            words += f[i].size() + wt[i].size();
        }
        /* a tile's input rows must fit the LDS intermediate (first[] ascends by `scale` per output row of D, by at most 1 of U) */
        for (int i = 1; i < 4; i += 2) {
            const size_t th = i == 1 ? kUpH : kDownH;
            const int rows = i == 1 ? kUpRows : kDownRows;
            for (size_t y0 = 0; y0 < f[i].size(); y0 += th) {
                const size_t y1 = std::min(f[i].size(), y0 + th) - 1;
                if (f[i][y1] + (int)T[i] - f[i][y0] > rows) return fail(c, std::string(who) + "operator footprint exceeds the tile buffer");
            }
        }
        B.host.resize(words);
        size_t o = 0;
        for (int i = 0; i < 4; i++) {
            B.off[2 * i] = o; std::memcpy(&B.host[o], f[i].data(), f[i].size() * 4); o += f[i].size();
            B.off[2 * i + 1] = o; std::memcpy(&B.host[o], wt[i].data(), wt[i].size() * 4); o += wt[i].size();
            B.T[i] = T[i];
        }
        HIPCK(c, B.tab.reserve(words * 4));
        HIPCK(c, hipMemcpyAsync(B.tab.p, B.host.data(), words * 4, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        std::memcpy(B.key, key, sizeof(key));
    }
    const unsigned* base = B.tab.as<unsigned>();
    auto I = [&](int i) { return reinterpret_cast<const int*>(base + B.off[i]); };
    auto F = [&](int i) { return reinterpret_cast<const float*>(base + B.off[i]); };
    up = SrOp{I(0), F(1), I(2), F(3), B.T[0], B.T[1], w, h, W, H};
    down = SrOp{I(4), F(5), I(6), F(7), B.T[2], B.T[3], W, H, w, h};
    return 0;
}

template <int MODE>
void launch(lfbm5d_ctx* c, const SrOp& op, const float* in, float* out, const float* aux, float beta, unsigned nne, unsigned C) {
    const bool is_up = op.wout > op.win;
    const unsigned th = is_up ? kUpH : kDownH;
    const dim3 grid((op.wout + kTileW - 1) / kTileW, (op.hout + th - 1) / th, nne * C);
    if (is_up) hipLaunchKernelGGL((k_resample<MODE, kUpH, kUpRows, kMaxT>), grid, dim3(256), 0, c->stream, op, in, out, aux, beta, c->side.sai.as<unsigned>(), C);
    else hipLaunchKernelGGL((k_resample<MODE, kDownH, kDownRows, kMaxT>), grid, dim3(256), 0, c->stream, op, in, out, aux, beta, c->side.sai.as<unsigned>(), C);
}

/* z = x + beta U (y - D x): two launches; r goes through the context's low-resolution scratch */
int backproject(lfbm5d_ctx* c, const SrOp& up, const SrOp& down, const float* y, const float* x, float* z, float beta, unsigned asize,
                unsigned nne, unsigned C) {
    HIPCK(c, c->sr.lo.reserve((size_t)asize * C * up.win * up.hin * sizeof(float)));
    float* r = c->sr.lo.as<float>();
    launch<kResidual>(c, down, x, r, y, 0.0f, nne, C);
    launch<kUpdate>(c, up, r, z, x, beta, nne, C);
    HIPCK(c, hipGetLastError());
    return 0;
}

int superres(lfbm5d_ctx* c, const char* who, const lfbm5d_sr_params* sr, const lfbm5d_params* P, const float* d_low, const unsigned* h_mask,
             float* d_high, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned w, unsigned h, unsigned C) {
    if (!sr || !P || !d_low || !h_mask || !d_high) return fail(c, std::string(who) + "NULL pointer for a required buffer");
    if (const char* m = check_operator(sr)) return fail(c, std::string(who) + m);
    if (const char* m = check_loop(sr)) return fail(c, std::string(who) + m);
    if (check_one_gpu(c, who, "super-resolution runs on one GPU (this context has a communicator)")) return 1;
    const unsigned asize = awidth * aheight, s = sr->scale, W = w * s, H = h * s;
    SrOp up, down; unsigned nne = 0;
    if (ensure(c, who, sr, h_mask, asize, w, h, C, up, down, nne)) return 1;
    launch<kPlain>(c, up, d_low, d_high, nullptr, 0.0f, nne, C);            /* x_0 = U y */
    HIPCK(c, hipGetLastError());
    /* x_k = step(x_{k-1} + beta U (y - D x_{k-1})); no noise floor: the schedule ends at sigma_end */
    if (refine_loop(c, LoopSchedule{sr->iterations, sr->sigma_start, sr->sigma_end, 0.0f}, P, h_mask, nne, d_high, ang_major, awidth, aheight, an, W,
                    H, C, [&](unsigned, float* z) { return backproject(c, up, down, d_low, d_high, z, sr->beta, asize, nne, C); },
                    [](unsigned) { return 0; })) return 1;
    if (sr->close_projection && backproject(c, up, down, d_low, d_high, d_high, sr->beta, asize, nne, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* namespace */

extern "C" {

int lfbm5d_sr_defaults(unsigned scale, lfbm5d_sr_params* out) {
    if (!out || scale < 2 || scale > 4) return 1;
    std::memset(out, 0, sizeof(*out));
    out->scale = scale;
    out->kernel = LFBM5D_SR_BICUBIC;
    out->blur_sigma = 0.4f * (float)scale;   /* used once the caller selects LFBM5D_SR_GAUSSIAN */
    out->iterations = 12;                    /* the best of the sweep in profiles/sr_defaults.txt */
    out->sigma_start = 15.0f * (float)scale;
    out->sigma_end = 2.0f * (float)scale;
    out->beta = 1.0f;
    out->close_projection = 1;
    return 0;
}

int lfbm5d_sr_taps(unsigned op, const lfbm5d_sr_params* sr, unsigned n_in, int* first, float* w, unsigned* T, unsigned cap) {
    if (!T || check_operator(sr) || (op != LFBM5D_SR_UP && op != LFBM5D_SR_DOWN)) return 1;
    std::vector<int> f; std::vector<float> wt; unsigned t = 0;
    if (!build_taps(op, sr, n_in, f, wt, t)) return 1;
    *T = t;
    if (!first && !w) return 0;   /* size query */
    if (!first || !w || wt.size() > (size_t)cap) return 1;
    std::memcpy(first, f.data(), f.size() * sizeof(int));
    std::memcpy(w, wt.data(), wt.size() * sizeof(float));
    return 0;
}

int lfbm5d_sr_up_device(lfbm5d_ctx* c, const lfbm5d_sr_params* sr, const float* d_low, const unsigned* h_mask, float* d_high, unsigned asize,
                        unsigned w, unsigned h, unsigned C) {
    if (!c) return 1;
    const char* who = "lfbm5d_sr_up_device: ";
    if (!d_low || !d_high) return fail(c, std::string(who) + "NULL pointer for a required buffer");
    SrOp up, down; unsigned nne = 0;
    if (ensure(c, who, sr, h_mask, asize, w, h, C, up, down, nne)) return 1;
    launch<kPlain>(c, up, d_low, d_high, nullptr, 0.0f, nne, C);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int lfbm5d_sr_down_device(lfbm5d_ctx* c, const lfbm5d_sr_params* sr, const float* d_high, const unsigned* h_mask, float* d_low, unsigned asize,
                          unsigned w, unsigned h, unsigned C) {
    if (!c) return 1;
    const char* who = "lfbm5d_sr_down_device: ";
    if (!d_low || !d_high) return fail(c, std::string(who) + "NULL pointer for a required buffer");
    SrOp up, down; unsigned nne = 0;
    if (ensure(c, who, sr, h_mask, asize, w, h, C, up, down, nne)) return 1;
    launch<kPlain>(c, down, d_high, d_low, nullptr, 0.0f, nne, C);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int lfbm5d_sr_backproject_device(lfbm5d_ctx* c, const lfbm5d_sr_params* sr, const float* d_low_y, const float* d_high_x, const unsigned* h_mask,
                                 float* d_high_z, unsigned asize, unsigned w, unsigned h, unsigned C) {
    if (!c) return 1;
    const char* who = "lfbm5d_sr_backproject_device: ";
    if (!d_low_y || !d_high_x || !d_high_z) return fail(c, std::string(who) + "NULL pointer for a required buffer");
    SrOp up, down; unsigned nne = 0;
    if (ensure(c, who, sr, h_mask, asize, w, h, C, up, down, nne)) return 1;
    if (const char* m = check_beta(sr)) return fail(c, std::string(who) + m);
    if (backproject(c, up, down, d_low_y, d_high_x, d_high_z, sr->beta, asize, nne, C)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int lfbm5d_superres_device(lfbm5d_ctx* c, const lfbm5d_sr_params* sr, const lfbm5d_params* P, const float* d_low, const unsigned* h_mask,
                           float* d_high, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned w, unsigned h,
                           unsigned C) {
    if (!c) return 1;
    return superres(c, "lfbm5d_superres_device: ", sr, P, d_low, h_mask, d_high, ang_major, awidth, aheight, an, w, h, C);
}

int lfbm5d_superres_host_sai(lfbm5d_ctx* c, const lfbm5d_sr_params* sr, const lfbm5d_params* P, const float* const* h_low,
                             const unsigned* h_mask, float* const* h_high, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                             unsigned w, unsigned h, unsigned C) {
    if (!c) return 1;
    const char* who = "lfbm5d_superres_host_sai: ";
    if (!sr || !P || !h_low || !h_mask || !h_high) return fail(c, std::string(who) + "NULL pointer for a required buffer");
    if (const char* m = check_operator(sr)) return fail(c, std::string(who) + m);
    const unsigned asize = awidth * aheight;
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_low, asize, nonempty) || check_planes(c, who, h_high, asize, nonempty)) return 1;   /* before anything is reserved */
    (void)hipSetDevice(c->device);
    const size_t lo = (size_t)C * w * h, hi = lo * sr->scale * sr->scale;
    HIPCK(c, c->h2d_noisy.reserve((size_t)asize * lo * sizeof(float)));
    HIPCK(c, c->h2d_out.reserve((size_t)asize * hi * sizeof(float)));
    float* const d_low = c->h2d_noisy.as<float>(); float* const d_high = c->h2d_out.as<float>();
    if (upload_planes(c, who, h_low, d_low, asize, lo, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (superres(c, who, sr, P, d_low, h_mask, d_high, ang_major, awidth, aheight, an, w, h, C)) return 1;
    if (download_planes(c, h_high, d_high, asize, hi, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* extern "C" */
