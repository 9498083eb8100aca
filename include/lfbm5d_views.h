/*
 * lfbm5d_views.h -- per-view noise levels: one sigma per sub-aperture image, turned into one sigma per angular window.  Part of
 * include/lfbm5d.h, which includes this file at its end; do not include it on its own.  Not in the reference.  Opt-in.
 *
 * Why.  Every job takes one `sigma` for the whole light field.  A devignetted lenslet capture carries two to three times the centre's
 * noise in its outer views, the cameras of an array have a gain each, and lfbm5d_photo_* itself turns a view's sigma into sigma / g.
 *
 * View table.  const double sigma_sai[asize]: one noise level per SAI on the scale of lfbm5d_params.sigma, in the light field's own
 * SAI order.  Entries of empty SAIs (mask == 0) are ignored; every other entry must be finite and greater than 0, otherwise the call
 * fails with a message that names the SAI.
 * Window sigma.  Over the non-empty SAIs of a window (lfbm5d_plan_windows' window around (ps, pt) of half size an, shifted into the
 * light field; its slots in ascending slot order, which is the light field's major order), n of them: if all their table values are the
 * same double s, the window sigma is (float)s; otherwise it is (float)sqrt((sum sigma_v^2) / n), the sum from +0 in that order, every
 * operation in double.  A window without a non-empty SAI has no sigma (the call fails; the schedule never runs such a window).
 * Why the root mean square.  A 5-D coefficient is sum_v b_v x_v over the window's views with an angular basis vector b of unit norm;
 * with independent noise its variance is sum_v b_v^2 sigma_v^2.  For every b whose entries have equal magnitude (the DC vector of
 * the DCT and the SADCT among them) that is exactly the mean of sigma_v^2; for the others the mean is the pooled value.  The first
 * branch makes a uniform table reproduce the job with sigma = s bit for bit.
 * What a job does with it.  Where the schedule hands a window its copy of the parameters it sets that copy's sigma to the window
 * sigma: thresholds, tauMatch, weights and tables of the window's passes follow, in every schedule form (graph on lanes and ranks,
 * two calls, data-driven further passes, tile mode, spatial bands).  The window plan does not depend on the table; several ranks pass
 * the same table and stay bit-identical to one.  The kernels are untouched: a pass still has one sigma.
 * What it does not do: noise that varies inside a window is pooled, not modelled per coefficient; one level per SAI, not per channel;
 * no signal-dependent (Poisson-Gaussian, clipped) model per view; the consistency check is not told.
 * The table lives in the context for the duration of the call only: set on entry, cleared on every exit path.
 */

/* ---- host only, callable without a GPU or a context ---- */
/* The message of the last failed lfbm5d_views_* host function on this thread ("" if none). */
const char* lfbm5d_views_error(void);
/* The window sigma of the window around SAI (ps, pt) with half size an.  h_mask [asize] or NULL (no empty SAI).  1 with a message: a
 * NULL pointer, ang_major, a window larger than the light field, (ps, pt) outside it, a bad table entry on a non-empty SAI of the
 * window, a window without a non-empty SAI. */
int lfbm5d_views_window_sigma(const double* sigma_sai, const unsigned* h_mask, unsigned ang_major, unsigned awidth, unsigned aheight,
                              unsigned ps, unsigned pt, unsigned an, float* out);
/* What equalisation leaves: sigma_v = sigma sqrt((sum_c g_{v,c}^-2) / C), the channels pooled (double, c ascending from +0).
 * gain [asize][C], C = 1..3, float32 (lfbm5d_photo_device's h_gain is double [asize][3]: convert, and drop the channels that are not
 * stored).  Empty SAIs get 0.
 * 1 with a message: a NULL pointer, C, sigma not finite or <= 0, a gain that is not finite or <= 0 on a non-empty SAI. */
int lfbm5d_views_from_gains(double sigma, const float* gain, unsigned C, const unsigned* h_mask, unsigned asize, double* sigma_sai_out);

/* ---- the jobs: lfbm5d_denoise_device / _host_sai, lfbm5d_step1_device, lfbm5d_step2_device, lfbm5d_bm3d_lf_device with a view table.
 * The tail arguments are theirs; P->sigma (hard->sigma, wien->sigma) is ignored.  h_sigma_sai [asize] (host), or NULL: the per-SAI
 * estimate of lfbm5d_noise_level_device (patch 8) on the noisy light field is taken first.  h_sigma_used [asize] (host) or NULL receives
 * the table that was applied (0 for empty SAIs).  The BM3D job filters SAI v with exactly (float)sigma_v in both steps.  1 with a
 * message: what the plain jobs reject, a bad table entry on a non-empty SAI (the message names it). ---- */
int lfbm5d_denoise_views_device(lfbm5d_ctx* ctx, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P1,
                                const lfbm5d_params* P2, float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised,
                                unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H,
                                unsigned C);
int lfbm5d_denoise_views_host_sai(lfbm5d_ctx* ctx, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P1,
                                  const lfbm5d_params* P2, float* const* h_noisy, const unsigned* h_mask, float* const* h_basic,
                                  float* const* h_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1,
                                  unsigned an2, unsigned W, unsigned H, unsigned C);
int lfbm5d_step1_views_device(lfbm5d_ctx* ctx, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P, float* d_noisy,
                              const unsigned* h_mask, float* d_basic, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                              unsigned W, unsigned H, unsigned C);
int lfbm5d_step2_views_device(lfbm5d_ctx* ctx, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_params* P, float* d_noisy,
                              const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth,
                              unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C);
int lfbm5d_bm3d_lf_views_device(lfbm5d_ctx* ctx, const double* h_sigma_sai, double* h_sigma_used, const lfbm5d_bm3d_params* hard,
                                const lfbm5d_bm3d_params* wien, float* d_noisy, const unsigned* h_mask, float* d_basic,
                                float* d_denoised, unsigned asize, unsigned W, unsigned H, unsigned C);
/* The sigma applied to every window of the last lfbm5d_step* / lfbm5d_denoise_* job on this context, in the order of
 * lfbm5d_last_windows; a job without a table returns its own sigmas.  Copies min(count, cap) values (out may be NULL) and returns the
 * count, -1 on a NULL context. */
int lfbm5d_last_window_sigmas(const lfbm5d_ctx* ctx, float* out, unsigned cap);
