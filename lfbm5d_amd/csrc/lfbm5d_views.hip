/*
 * lfbm5d_views.hip -- per-view noise levels (include/lfbm5d_views.h): the rule on the host, and the jobs that run with a view table.
 * No kernel of its own: a job places the table in its context, the window schedule (lfbm5d_steps.hip, lfbm5d_graph.hip) and the per-SAI
 * BM3D loop (lfbm5d_api.hip) read it where they hand a window or an SAI its copy of the parameters, and the table is gone when the
 * entry point returns.
 */
#include "lfbm5d_ctx.h"

using namespace lfbm5d_host;

namespace {

thread_local std::string t_views_error;
int host_fail(const std::string& m) { t_views_error = m; return 1; }

bool positive(double v) { return std::isfinite(v) && v > 0.0; }
std::string bad_entry(unsigned st, double v) { return "sigma_sai[" + std::to_string(st) + "] = " + std::to_string(v) + " is not a finite value greater than 0"; }

/* The view table of one job: placed in the context by set(), removed when the entry point returns, whichever way -- like pass_impl
 * consumes est_ready before anything can fail, no later job on this context can see it. */
struct TableScope {
    lfbm5d_ctx* const c;
    explicit TableScope(lfbm5d_ctx* cc) : c(cc) { c->views.table.clear(); }
    ~TableScope() { c->views.table.clear(); }
    /* h_sigma_sai == NULL: the per-SAI estimate of the noisy light field (d_noisy, or h_noisy one pointer per SAI) */
    int set(const std::string& who, const double* h_sigma_sai, double* h_sigma_used, const float* d_noisy, const float* const* h_noisy,
            const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C) {
        if (!h_mask) return fail(c, who + "NULL pointer for a required buffer");
        if (asize == 0) return fail(c, who + "a light field without SAIs");
        std::vector<double> t(asize, 0.0);
        if (h_sigma_sai) {
            for (unsigned st = 0; st < asize; st++) if (h_mask[st]) t[st] = h_sigma_sai[st];
        } else {
            lfbm5d_noise_level nl;
            if (h_noisy ? lfbm5d_noise_level_host_sai(c, h_noisy, h_mask, asize, W, H, C, 8, &nl, t.data(), nullptr)
                        : lfbm5d_noise_level_device(c, d_noisy, h_mask, asize, W, H, C, 8, &nl, t.data(), nullptr)) return 1;
            for (unsigned st = 0; st < asize; st++) if (!h_mask[st]) t[st] = 0.0;
        }
        for (unsigned st = 0; st < asize; st++)
            if (h_mask[st] && !positive(t[st])) return fail(c, who + (h_sigma_sai ? "" : "estimated ") + bad_entry(st, t[st]));
        if (h_sigma_used) std::memcpy(h_sigma_used, t.data(), asize * sizeof(double));
        c->views.table = std::move(t);
        return 0;
    }
};

} /* namespace */

extern "C" {

const char* lfbm5d_views_error(void) { return t_views_error.c_str(); }

int lfbm5d_views_window_sigma(const double* sigma_sai, const unsigned* h_mask, unsigned ang_major, unsigned awidth, unsigned aheight,
                              unsigned ps, unsigned pt, unsigned an, float* out) {
    const std::string who = "lfbm5d_views_window_sigma: ";
    if (!sigma_sai || !out) return host_fail(who + "NULL pointer for a required buffer");
    if (ang_major != LFBM5D_ROWMAJOR && ang_major != LFBM5D_COLMAJOR) return host_fail(who + "bad ang_major");
    if (an > 8 || 2 * an + 1 > awidth || 2 * an + 1 > aheight) return host_fail(who + "angular search window larger than the light field");
    if (ps >= aheight || pt >= awidth) return host_fail(who + "(ps, pt) outside the light field");
    const plan::Grid grid{awidth, aheight, ang_major};
    const plan::Window win = plan::window_at(grid, ps, pt, an);
    unsigned n = 0;
    for (unsigned st : win.st) {
        if (h_mask && !h_mask[st]) continue;
        if (!positive(sigma_sai[st])) return host_fail(who + bad_entry(st, sigma_sai[st]));
        n++;
    }
    if (n == 0) return host_fail(who + "the window holds no non-empty SAI");
    *out = plan::window_sigma(sigma_sai, win, h_mask);
    return 0;
}

int lfbm5d_views_from_gains(double sigma, const float* gain, unsigned C, const unsigned* h_mask, unsigned asize, double* sigma_sai_out) {
    const std::string who = "lfbm5d_views_from_gains: ";
    if (!gain || !sigma_sai_out) return host_fail(who + "NULL pointer for a required buffer");
    if (C < 1 || C > 3) return host_fail(who + "C must be 1, 2 or 3");
    if (!positive(sigma)) return host_fail(who + "sigma must be finite and greater than 0");
    for (unsigned st = 0; st < asize; st++) {
        if (h_mask && !h_mask[st]) { sigma_sai_out[st] = 0.0; continue; }
        double sum = 0.0;
        for (unsigned ch = 0; ch < C; ch++) {
            const double g = (double)gain[(size_t)st * C + ch];
            if (!positive(g))
                return host_fail(who + "gain[" + std::to_string(st) + "][" + std::to_string(ch) + "] = " + std::to_string(g) + " is not a finite value greater than 0");
            sum += 1.0 / (g * g);
        }
        sigma_sai_out[st] = sigma * std::sqrt(sum / (double)C);
    }
    return 0;
}

int lfbm5d_denoise_views_device(lfbm5d_ctx* c, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P1, const lfbm5d_params* P2,
                                float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth,
                                unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    (void)hipSetDevice(c->device);
    TableScope table(c);
    if (table.set("lfbm5d_denoise_views_device: ", h_sigma_sai, h_sigma_used, d_noisy, nullptr, h_mask, awidth * aheight, W, H, C)) return 1;
    return lfbm5d_denoise_device(c, P1, P2, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_denoise_views_host_sai(lfbm5d_ctx* c, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P1, const lfbm5d_params* P2,
                                  float* const* h_noisy, const unsigned* h_mask, float* const* h_basic, float* const* h_denoised,
                                  unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H,
                                  unsigned C) {
    if (!c) return 1;
    (void)hipSetDevice(c->device);
    const std::string who = "lfbm5d_denoise_views_host_sai: ";
    if (!h_noisy) return fail(c, who + "NULL pointer for a required buffer");
    TableScope table(c);
    if (table.set(who, h_sigma_sai, h_sigma_used, nullptr, h_noisy, h_mask, awidth * aheight, W, H, C)) return 1;
    return lfbm5d_denoise_host_sai(c, P1, P2, h_noisy, h_mask, h_basic, h_denoised, ang_major, awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_step1_views_device(lfbm5d_ctx* c, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P, float* d_noisy,
                              const unsigned* h_mask, float* d_basic, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W,
                              unsigned H, unsigned C) {
    if (!c) return 1;
    (void)hipSetDevice(c->device);
    TableScope table(c);
    if (table.set("lfbm5d_step1_views_device: ", h_sigma_sai, h_sigma_used, d_noisy, nullptr, h_mask, awidth * aheight, W, H, C)) return 1;
    return lfbm5d_step1_device(c, P, d_noisy, h_mask, d_basic, ang_major, awidth, aheight, an, W, H, C);
}

int lfbm5d_step2_views_device(lfbm5d_ctx* c, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P, float* d_noisy,
                              const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight,
                              unsigned an, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    (void)hipSetDevice(c->device);
    TableScope table(c);
    if (table.set("lfbm5d_step2_views_device: ", h_sigma_sai, h_sigma_used, d_noisy, nullptr, h_mask, awidth * aheight, W, H, C)) return 1;
    return lfbm5d_step2_device(c, P, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an, W, H, C);
}

int lfbm5d_bm3d_lf_views_device(lfbm5d_ctx* c, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_bm3d_params* hard,
                                const lfbm5d_bm3d_params* wien, float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised,
                                unsigned asize, unsigned W, unsigned H, unsigned C) {
    if (!c) return 1;
    (void)hipSetDevice(c->device);
    TableScope table(c);
    if (table.set("lfbm5d_bm3d_lf_views_device: ", h_sigma_sai, h_sigma_used, d_noisy, nullptr, h_mask, asize, W, H, C)) return 1;
    return lfbm5d_bm3d_lf_device(c, hard, wien, d_noisy, h_mask, d_basic, d_denoised, asize, W, H, C);
}

} /* extern "C" */
