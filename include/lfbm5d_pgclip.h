/*
 * lfbm5d_pgclip.h -- clipped Poisson-Gaussian noise: signal-dependent noise on data that were rounded and clipped to a known range
 * (8-bit files).  The censored fit of the model, the variance stabiliser of a clipped heteroskedastic observation with its exact
 * unbiased inverse, and the two-step job between them.  Part of include/lfbm5d.h, which includes this file at its end; do not include it
 * on its own.  Not in the reference.  Opt-in.  After Foi, "Clipped noisy images: heteroskedastic modeling and practical denoising",
 * Signal Processing 89 (2009): the Gaussian heteroskedastic form, no exact Poisson statistics.
 *
 * Model.  z = clip(y + sigma(y) n, lo, hi), n standard normal, sigma^2(y) = max(a (y - lo) + b, 1/12), y in [lo, hi].  1/12 is the
 * variance of rounding to whole numbers; it keeps every integrand below bounded.  With lo = 0 this is the model of lfbm5d_pg_*; the
 * offset puts the photon term above the black level.  Valid: a >= 0, b >= 0, a + b > 0, lo < hi, all finite.  Accepted domain:
 * a^2 <= 0.5 b and a <= 5 (a Monte-Carlo table with real Poisson draws): beyond it a Gaussian does not describe the photon
 * counts near black, where nothing is clipped either; that regime is lfbm5d_denoise_pg_*'s.
 *
 * Estimate.  The counts are lfbm5d_clip_histogram_device's (hist, sum, cens, whole), unchanged.  Per level: n, the variance v of
 * lfbm5d_clip_fit (the 0.25 quantile of |d| on the lattice edges, less delta^2 / 3 when every counted block is whole), x = sum / (256 n),
 * w = n / v^2.  A level counts when it is populated and cens <= f_max n; f_max runs down lfbm5d_clip_fit's ladder 0.05, 0.1, 0.2, 0.4, 1
 * until at least 4 levels count; fewer than 4 populated levels: the fit fails.  Over the levels that count, in level order, the
 * constrained weighted line v = a' x + b' of lfbm5d_pg_fit with its branches (a' < 0: a' = 0, b' the weighted mean; b' < 0: b' = 0,
 * a' = Swxv / Swxx).  Back from the rescaled range: a = a' / s_r, b = b' / s_r^2, s_r = (float)(255 / (hi - lo)).  Host, double.
 *
 * Curves (host, double; lfbm5d_pgclip_curves).  Grid y_i = lo + i (hi - lo) / 4096, i = 0..4096; sigma_i = sigma(y_i),
 * alpha = (lo - y) / sigma, beta = (hi - y) / sigma.
 *   clipped mean       m(y) = lo Phi(alpha) + hi (1 - Phi(beta)) + y (Phi(beta) - Phi(alpha)) + sigma (phi(alpha) - phi(beta))
 *   clipped deviation  d(y)^2 = (lo - y)^2 Phi(alpha) + (hi - y)^2 (1 - Phi(beta))
 *                               + sigma^2 (Phi(beta) - Phi(alpha) + alpha phi(alpha) - beta phi(beta)) - (m - y)^2
 * (the second moment about y: nothing large cancels).  Stabiliser: F0(m_i) the cumulative trapezoid of 1 / d over m, from 0; piecewise
 * linear between the m_i; below m_0 and above m_4096 extended linearly with the slopes 1 / d_0 and 1 / d_4096, so pixels that sit at lo
 * or hi stay ordered.  s = 255 / F0(m_4096), F = s F0: the stabilised data span 255 and the filter's sigma is s.  Exact unbiased
 * inverse: G(y_i) = E[F(clip(y_i + sigma_i n, lo, hi))] by the trapezoid rule over n = -8..8 in 3201 points, normalised by the sum of
 * its weights (the point masses at lo and hi fall out of the clip); G must be strictly increasing or the call fails.  The inverse map is
 * G^-1: it undoes the stabiliser and the clipping bias in one step.
 * Tables, 4097 float32 knots each: fwd[k] = F(lo + k (hi - lo) / 4096); inv[k] = G^-1(G(lo) + k (G(hi) - G(lo)) / 4096) (G^-1 piecewise
 * linear through (G(y_i), y_i); inv[0] = lo, inv[4096] = hi exactly).  The tables are the definition of the maps.
 *
 * Look-up (GPU, float32, every operation rounded on its own, in this order; x0 = (float)x0, inv_dx = (float)(1 / dx) of the table):
 * t = (x - x0) inv_dx; i = (int)min(max(floorf(t), 0), 4095); r = t - (float)i; forward: r as it is (the end segments extend the map);
 * inverse: r = min(max(r, 0), 1) (the output stays in [lo, hi]); out = T[i] + r (T[i + 1] - T[i]).  A non-finite x passes through
 * unchanged.  Planes of empty SAIs are not touched.  In place is allowed.  Equal to tests/pgclip_model.py bit for bit.
 *
 * Limits: one pooled model for all channels and SAIs; Gaussian heteroskedastic statistics (see the accepted domain); the filter sees
 * deviations between 0.75 s (at the bounds, where half the mass is a point) and 1.1 s; one GPU.
 */
#define LFBM5D_PGCLIP_KNOTS 4097

typedef struct { double a, b, lo, hi; } lfbm5d_pgclip_model;

typedef struct {
    lfbm5d_pgclip_model model;                /* the pooled model (lo and hi as given)                                     */
    double a_channel[3], b_channel[3];        /* every channel's own fit (NaN: it failed; unused channels 0)               */
    double f_max;                             /* the ladder's step the pooled fit used                                     */
    double censored;                          /* blocks that hold a censored pixel / blocks counted                        */
    unsigned levels;                          /* levels the pooled fit used                                                */
    unsigned heavily_clipped;                 /* 1 when f_max > 0.1                                                        */
    unsigned quantised;                       /* 1 when every counted block holds whole numbers                            */
    unsigned reserved;
    unsigned long long blocks, skipped;       /* 2 x 2 blocks visited and skipped (0 from lfbm5d_pgclip_fit)               */
} lfbm5d_pgclip_estimate;

/* a tag, not a typedef: the function that fills it bears the same name, so write `struct lfbm5d_pgclip_curves` */
struct lfbm5d_pgclip_curves {
    lfbm5d_pgclip_model model;
    double s;                                 /* the deviation of the stabilised data: the filter's sigma                  */
    double fwd_x0, fwd_dx;                    /* fwd[k] is F at fwd_x0 + k fwd_dx                                          */
    double inv_x0, inv_dx;                    /* inv[k] is G^-1 at inv_x0 + k inv_dx                                       */
    float fwd[LFBM5D_PGCLIP_KNOTS], inv[LFBM5D_PGCLIP_KNOTS];
};

/* ---- host only, callable without a GPU ---- */
/* The fit of the statistics hist [C][64][322], sum [C][64], cens [C][64], whole [C] of lfbm5d_clip_histogram_device.  1: a NULL
 * pointer, C not 1 or 3, a bad range, or fewer than 4 populated levels in the pooled histogram. */
int lfbm5d_pgclip_fit(const unsigned long long* hist, const unsigned long long* sum, const unsigned long long* cens,
                      const unsigned long long* whole, unsigned C, double lo, double hi, lfbm5d_pgclip_estimate* out);
/* The curves of a model.  0: built.  1 with the reason in lfbm5d_pgclip_curves_error(): a NULL pointer, an invalid model, a model
 * outside the accepted domain (the message names lfbm5d_denoise_pg), G not strictly increasing. */
int lfbm5d_pgclip_curves(const lfbm5d_pgclip_model* model, struct lfbm5d_pgclip_curves* out);
/* The message of this thread's last failed lfbm5d_pgclip_curves ("" before one). */
const char* lfbm5d_pgclip_curves_error(void);

/* ---- on the GPU ---- */
/* The model of the light field d_lf [asize][C*H*W] in HBM (only read).  1 with a message: what lfbm5d_clip_histogram_device refuses,
 * or fewer than 4 populated levels. */
int lfbm5d_pgclip_estimate_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                  unsigned C, double lo, double hi, lfbm5d_pgclip_estimate* out);
/* The same on host planes, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM: identical results. */
int lfbm5d_pgclip_estimate_host_sai(lfbm5d_ctx* ctx, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W,
                                    unsigned H, unsigned C, double lo, double hi, lfbm5d_pgclip_estimate* out);
/* d_out = fwd / inv of d_in by the look-up above, both [asize][C*H*W] in HBM; d_out may be d_in (any other overlap returns 1). */
int lfbm5d_pgclip_forward_device(lfbm5d_ctx* ctx, const struct lfbm5d_pgclip_curves* curves, const float* d_in, const unsigned* h_mask,
                                 float* d_out, unsigned asize, unsigned W, unsigned H, unsigned C);
int lfbm5d_pgclip_inverse_device(lfbm5d_ctx* ctx, const struct lfbm5d_pgclip_curves* curves, const float* d_in, const unsigned* h_mask,
                                 float* d_out, unsigned asize, unsigned W, unsigned H, unsigned C);
/* The job.  model NULL: lfbm5d_pgclip_estimate_device on d_noisy at (lo, hi) first, the pooled model; otherwise lo and hi are the
 * model's and the arguments are not read.  `used` (may be NULL) receives the model applied, `s_used` (may be NULL) the s of its curves, `est` (may be NULL) the estimate (zeros when the model was given).  Then
 * lfbm5d_pgclip_curves; lfbm5d_pgclip_forward_device of d_noisy (only read) into a scratch light field of the context;
 * lfbm5d_denoise_device on it with P1->sigma = P2->sigma = (float)s (the sigmas passed are ignored); lfbm5d_pgclip_inverse_device in
 * place on d_basic and d_denoised.  Bit-identical to those calls made by hand.  One GPU. */
int lfbm5d_denoise_pgclip_device(lfbm5d_ctx* ctx, const lfbm5d_pgclip_model* model, double lo, double hi, lfbm5d_pgclip_model* used,
                                 double* s_used, lfbm5d_pgclip_estimate* est, const lfbm5d_params* P1, const lfbm5d_params* P2, const float* d_noisy,
                                 const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth,
                                 unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C);
int lfbm5d_denoise_pgclip_host_sai(lfbm5d_ctx* ctx, const lfbm5d_pgclip_model* model, double lo, double hi, lfbm5d_pgclip_model* used,
                                   double* s_used, lfbm5d_pgclip_estimate* est, const lfbm5d_params* P1, const lfbm5d_params* P2,
                                   const float* const* h_noisy, const unsigned* h_mask, float* const* h_basic, float* const* h_denoised,
                                   unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W,
                                   unsigned H, unsigned C);
