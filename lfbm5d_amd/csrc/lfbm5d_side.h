/*
 * lfbm5d_side.h -- the host frame the side stages share (noise level, quality, super-resolution, Poisson-Gaussian, impulse repair,
 * inpainting, view synthesis, consistency check): the list of non-empty SAIs, the argument checks, the staging of per-SAI host planes,
 * the refinement loop on the hard-thresholding step, the plane sweep's source rows.  Plain functions; where a stage supplies behaviour
 * it hands in a lambda.  Every message is the stage's prefix `who` plus a text kept as the stages had it.  Internal.
 */
#ifndef LFBM5D_SIDE_H
#define LFBM5D_SIDE_H

#include "lfbm5d_ctx.h"
#include "lfbm5d_side_values.h"

#include <cstdint>

namespace lfbm5d_host {

/* ---- the non-empty SAIs ---- */

/* c->side.sai_host -> c->side.sai, waited for.  The source is the context's own vector: it outlives a call that fails in here. */
inline int upload_sai_list(lfbm5d_ctx* c) {
    lfbm5d_ctx::SideBufs& S = c->side;
    HIPCK(c, S.sai.reserve(S.sai_host.size() * sizeof(unsigned)));
    HIPCK(c, hipMemcpyAsync(S.sai.p, S.sai_host.data(), S.sai_host.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* The non-empty SAIs of the mask: c->side.sai_host on the host, c->side.sai on the device, uploaded (and waited for) only when the list
 * differs from the one that is there.  1 with a message when the mask has none. */
inline int sai_list(lfbm5d_ctx* c, const std::string& who, const unsigned* h_mask, unsigned asize) {
    lfbm5d_ctx::SideBufs& S = c->side;
    std::vector<unsigned> sai;
    for (unsigned st = 0; st < asize; st++) if (h_mask[st]) sai.push_back(st);
    if (sai.empty()) return fail(c, who + "the mask has no non-empty SAI");
    (void)hipSetDevice(c->device);
    if (sai == S.sai_host) return 0;
    S.sai_host.swap(sai);
    if (!upload_sai_list(c)) return 0;
    S.sai_host.clear();                       /* the device holds no list (clear() keeps the storage a pending copy reads) */
    return 1;
}

/* ---- argument checks ---- */

inline int check_chnls(lfbm5d_ctx* c, const std::string& who, unsigned C) {
    return C == 1 || C == 3 ? 0 : fail(c, who + "chnls must be 1 or 3");
}

/* `what` completes "width and height must ": "be at least 2", "be at least twice the patch", "not be 0", "be at least 11 for SSIM" */
inline int check_size(lfbm5d_ctx* c, const std::string& who, unsigned W, unsigned H, unsigned min, const char* what) {
    return W >= min && H >= min ? 0 : fail(c, who + "width and height must " + what);
}

inline int check_angular(lfbm5d_ctx* c, const std::string& who, unsigned ang_major, unsigned aw, unsigned ah) {
    if (ang_major != LFBM5D_ROWMAJOR && ang_major != LFBM5D_COLMAJOR) return fail(c, who + "ang_major must be LFBM5D_ROWMAJOR or LFBM5D_COLMAJOR");
    if (!aw || !ah) return fail(c, who + "awidth and aheight must be at least 1");
    return 0;
}

/* `sentence`: the stage's own, e.g. "the impulse routines run on one GPU (this context has a communicator or a shard)" */
inline int check_one_gpu(lfbm5d_ctx* c, const std::string& who, const char* sentence) {
    return c->world > 1 || c->comm || c->ipc ? fail(c, who + sentence) : 0;
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

/* the grid of 64 x 32 tiles over a plane; `rows`: what the launch puts on the grid's second axis; max_plane: the stage's limit of W * H */
struct TileGrid { unsigned tx_n, ty_n; };
inline int check_tiles(lfbm5d_ctx* c, const std::string& who, unsigned W, unsigned H, unsigned long long rows, unsigned long long max_plane,
                       TileGrid& g) {
    g.tx_n = (W + lfbm5d_side::kTW - 1) / lfbm5d_side::kTW; g.ty_n = (H + lfbm5d_side::kTH - 1) / lfbm5d_side::kTH;
    if ((unsigned long long)W * H > max_plane || (unsigned long long)g.tx_n * g.ty_n > 0x7fffffffull || rows > 65535)
        return fail(c, who + "light field too large");
    return 0;
}

/* What the device entries of the impulse repair and the inpainting check alike, the SAI list and the tiling */
struct Shape { unsigned nne, tx_n, ty_n; };
inline int prepare_tiled(lfbm5d_ctx* c, const std::string& who, const char* one_gpu, const unsigned* h_mask, unsigned asize, unsigned W,
                         unsigned H, unsigned C, unsigned long long max_plane, Shape& s) {
    if (!h_mask) return fail(c, who + "NULL pointer for a required buffer");
    if (check_chnls(c, who, C) || check_size(c, who, W, H, 2, "be at least 2") || check_one_gpu(c, who, one_gpu)) return 1;
    if (sai_list(c, who, h_mask, asize)) return 1;
    s.nne = (unsigned)c->side.sai_host.size();
    TileGrid g;
    if (check_tiles(c, who, W, H, (unsigned long long)s.nne * C, max_plane, g)) return 1;
    s.tx_n = g.tx_n; s.ty_n = g.ty_n;
    return 0;
}

/* ---- per-SAI host planes <-> [asize][n] device memory; take(st) chooses the SAIs ---- */

template <class T, class Take>
int check_planes(lfbm5d_ctx* c, const std::string& who, T* const* h, unsigned asize, Take take) {
    for (unsigned st = 0; st < asize; st++)
        if (take(st) && !h[st]) return fail(c, who + "NULL pointer for a non-empty SAI");
    return 0;
}

/* checks the chosen planes, then enqueues their copies; the caller synchronises */
template <class T, class Take>
int upload_planes(lfbm5d_ctx* c, const std::string& who, const T* const* h, T* d, unsigned asize, size_t n, Take take) {
    if (check_planes(c, who, h, asize, take)) return 1;
    for (unsigned st = 0; st < asize; st++)
        if (take(st)) HIPCK(c, hipMemcpyAsync(d + (size_t)st * n, h[st], n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}

/* the non-empty SAIs at their places in [asize][img] of a staging buffer of the context, waited for */
inline int stage(lfbm5d_ctx* c, const std::string& who, const float* const* h_lf, const unsigned* h_mask, unsigned asize, size_t img, DevBuf& buf) {
    if (!h_lf || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    (void)hipSetDevice(c->device);
    HIPCK(c, buf.reserve(std::max<size_t>(1, (size_t)asize * img) * sizeof(float)));
    if (upload_planes(c, who, h_lf, buf.as<float>(), asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* enqueues the copies (output planes are checked with check_planes before the stage runs); the caller synchronises */
template <class T, class Take>
int download_planes(lfbm5d_ctx* c, T* const* h, const T* d, unsigned asize, size_t n, Take take) {
    for (unsigned st = 0; st < asize; st++)
        if (take(st)) HIPCK(c, hipMemcpyAsync(h[st], d + (size_t)st * n, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

/* The host form of a two-step job on stabilised data: the output planes are checked, the noisy light field is staged, job(d_noisy,
 * d_basic, d_denoised) runs the device form on the context's staging buffers, both estimates are downloaded and waited for. */
template <class Job>
int host_sai_job(lfbm5d_ctx* c, const std::string& who, const float* const* h_noisy, const unsigned* h_mask, float* const* h_basic,
                 float* const* h_denoised, unsigned asize, size_t img, Job job) {
    if (!h_basic || !h_denoised || !h_mask) return fail(c, who + "NULL pointer for a required buffer");
    const auto nonempty = [&](unsigned st) { return h_mask[st] != 0; };
    if (check_planes(c, who, h_basic, asize, nonempty) || check_planes(c, who, h_denoised, asize, nonempty)) return 1;
    if (stage(c, who, h_noisy, h_mask, asize, img, c->h2d_noisy)) return 1;
    HIPCK(c, c->h2d_basic.reserve(std::max<size_t>(1, (size_t)asize * img) * sizeof(float)));
    HIPCK(c, c->h2d_out.reserve(std::max<size_t>(1, (size_t)asize * img) * sizeof(float)));
    float* const db = c->h2d_basic.as<float>(); float* const dd = c->h2d_out.as<float>();
    if (job(c->h2d_noisy.as<float>(), db, dd)) return 1;
    if (download_planes(c, h_basic, db, asize, img, nonempty) || download_planes(c, h_denoised, dd, asize, img, nonempty)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* planes of the chosen SAIs of src -> dst (device to device), n values of el bytes each; enqueues only */
template <class Take>
int copy_sais(lfbm5d_ctx* c, unsigned asize, void* dst, const void* src, size_t n, size_t el, Take take) {
    for (unsigned st = 0; st < asize; st++)
        if (take(st))
            HIPCK(c, hipMemcpyAsync(static_cast<char*>(dst) + (size_t)st * n * el, static_cast<const char*>(src) + (size_t)st * n * el, n * el,
                                    hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

/* ---- the refinement loop ---- */

/* The context's scratch light field [asize][img]: what a step or a job is handed as its input and may mutate.  Zero-filled when the mask
 * has holes: the step is handed defined values in empty SAIs too. */
inline int scratch_lf(lfbm5d_ctx* c, unsigned asize, unsigned nne, size_t img, float*& z) {
    const size_t bytes = (size_t)asize * img * sizeof(float);
    HIPCK(c, c->side.lf.reserve(bytes));
    z = c->side.lf.as<float>();
    if (nne < asize) HIPCK(c, hipMemsetAsync(z, 0, bytes, c->stream));
    return 0;
}

struct LoopSchedule { unsigned iterations; float sigma_start, sigma_end, sigma_noise; };

/* the schedule of a stage whose loop is optional (0 iterations: none); NULL or the message's tail */
inline const char* check_schedule(const LoopSchedule& s) {
    if (!s.iterations) return nullptr;
    if (s.iterations > 1000) return "iterations must be at most 1000";
    if (!(s.sigma_start > 0.0f) || !(s.sigma_end > 0.0f) || !std::isfinite(s.sigma_start)) return "sigma_start and sigma_end must be positive";
    if (s.sigma_end > s.sigma_start) return "sigma_end must not exceed sigma_start";
    if (!(s.sigma_noise >= 0.0f) || !std::isfinite(s.sigma_noise)) return "sigma_noise must be finite and not negative";
    return nullptr;
}

/* x_k = after(step_1(fill(x_{k-1}); sigma_k)), k = 1..iterations, on the estimate d_x: fill(k, z) enqueues what forms the step's input
 * in the scratch z from d_x, the step (run_bm5d_1st_step at P with sigma_k = loop_sigma) writes its basic estimate over d_x, after(k)
 * puts the known data back.  The stream is idle when a step starts (its contract) and as `after` leaves it at the end. */
template <class Fill, class After>
int refine_loop(lfbm5d_ctx* c, const LoopSchedule& s, const lfbm5d_params* P, const unsigned* h_mask, unsigned nne, float* d_x,
                unsigned ang_major, unsigned aw, unsigned ah, unsigned an, unsigned W, unsigned H, unsigned C, Fill fill, After after) {
    float* z = nullptr;
    if (scratch_lf(c, aw * ah, nne, (size_t)C * W * H, z)) return 1;
    for (unsigned k = 1; k <= s.iterations; k++) {
        if (fill(k, z)) return 1;
        HIPCK(c, hipStreamSynchronize(c->stream));
        lfbm5d_params Pk = *P;
        Pk.sigma = lfbm5d_side::loop_sigma(k, s.iterations, s.sigma_start, s.sigma_end, s.sigma_noise);
        if (run_step(c, 1, &Pk, z, h_mask, nullptr, d_x, ang_major, aw, ah, an, W, H, C)) return 1;
        if (after(k)) return 1;
    }
    return 0;
}

/* ---- the plane sweep's source rows (k_view_sweep's table: kViewTabStride ints per SAI) ---- */

inline void sai_coords(unsigned st, unsigned ang_major, unsigned aw, unsigned ah, int& s, int& t) {
    if (ang_major == LFBM5D_ROWMAJOR) { s = (int)(st / aw); t = (int)(st % aw); }
    else { s = (int)(st % ah); t = (int)(st / ah); }
}

/* row = {m, n, n x (source index, ds, dt)}: the usable SAIs within R of m in both angular directions, in increasing order; returns n */
template <class Usable>
int source_row(unsigned m, unsigned ang_major, unsigned aw, unsigned ah, int R, Usable usable, int* row) {
    int sm, tm;
    sai_coords(m, ang_major, aw, ah, sm, tm);
    std::fill(row, row + kViewTabStride, 0);
    row[0] = (int)m;
    for (unsigned q = 0; q < aw * ah; q++) {
        if (!usable(q)) continue;
        int s, t;
        sai_coords(q, ang_major, aw, ah, s, t);
        if (std::abs(s - sm) > R || std::abs(t - tm) > R) continue;
        int* at = row + 2 + 3 * row[1]++;
        at[0] = (int)q; at[1] = s - sm; at[2] = t - tm;
    }
    return row[1];
}

} /* namespace lfbm5d_host */
#endif
