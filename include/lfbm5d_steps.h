/*
 * lfbm5d_steps.h -- the sub-pixel forms of the view synthesis and the consistency check: the entry points of the plane sweep with
 * `steps` = Q hypotheses per pixel.  Part of include/lfbm5d.h, which includes this file at its end and holds the definition ("Sub-pixel
 * disparities" in the view synthesis' and the consistency check's sections); do not include it on its own.
 *
 * Each function has the arguments of its sibling without `steps` (include/lfbm5d.h) plus `unsigned steps` behind `params`; the three
 * view forms also take h_hist_steps at the end.  The siblings are the steps = 1 calls of these: there is one implementation.
 *   steps          1, 2 or 4; anything else returns 1 with a message.  1 is the integer sweep: the sibling's code path and bits.
 *   d_disp/h_disp  int8, j* = d* in units of 1 / steps; |j*| <= 32.
 *   h_hist_steps   unsigned long long [LFBM5D_VIEW_STEPS_HIST] on the host, or NULL: positions per j*, index j* + 32 for every steps.
 *   out            lfbm5d_view_result.disparity_hist[17] is filled as by the sibling for steps = 1 and is all zero for steps > 1, where
 *                  h_hist_steps is the histogram.
 */
#ifndef LFBM5D_STEPS_H
#define LFBM5D_STEPS_H

#ifndef LFBM5D_H
#error "include lfbm5d.h, which includes this file"
#endif

#define LFBM5D_VIEW_STEPS_HIST 65

int lfbm5d_view_fill_steps_device(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, unsigned steps, const float* d_in,
                                  const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major,
                                  unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out,
                                  unsigned long long* h_hist_steps);
int lfbm5d_view_steps_device(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, unsigned steps, const lfbm5d_params* P, const float* d_in,
                             const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major,
                             unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out,
                             unsigned long long* h_hist_steps);
int lfbm5d_view_steps_host_sai(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, unsigned steps, const lfbm5d_params* P,
                               const float* const* h_in, const unsigned* h_mask, const unsigned* h_missing, float* const* h_out,
                               signed char* const* h_disp, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W,
                               unsigned H, unsigned C, lfbm5d_view_result* out, unsigned long long* h_hist_steps);
int lfbm5d_consist_steps_device(lfbm5d_ctx* ctx, const lfbm5d_consist_params* params, unsigned steps, const float* d_in,
                                const unsigned* h_mask, const unsigned* h_exclude, unsigned char* d_flags, unsigned* h_state,
                                signed char* d_disp, double* h_scale_sai, unsigned long long* h_hist, unsigned ang_major, unsigned awidth,
                                unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_consist_result* out);
int lfbm5d_consist_steps_host_sai(lfbm5d_ctx* ctx, const lfbm5d_consist_params* params, unsigned steps, const float* const* h_in,
                                  const unsigned* h_mask, const unsigned* h_exclude, unsigned char* const* h_flags, unsigned* h_state,
                                  signed char* const* h_disp, double* h_scale_sai, unsigned long long* h_hist, unsigned ang_major,
                                  unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_consist_result* out);

#endif
