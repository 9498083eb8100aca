/*
 * lfbm5d_repair.h -- joint repair: defective values and missing sub-aperture images repaired together by a mask-aware plane sweep
 * (lfbm5d_repair_*).  Included at the end of lfbm5d.h.  Not in the reference.  Opt-in: nothing else changes behaviour.
 *
 * The defect inpainting (lfbm5d_inpaint_*) fills a flagged region from its rim, in its own plane; the view synthesis (lfbm5d_view_*)
 * builds a missing SAI from its neighbours and assumes that every source value is sound.  Here both kinds of damage are one set of
 * unsound values, the plane sweep of the view synthesis skips unsound source values, and one refinement loop serves both.
 *
 * Data.  Light fields are [asize][C*H*W] float32, channels as stored; C = 1 or 3; W, H >= 2.  h_mask marks non-empty SAIs as
 * everywhere.  d_flags_in: uint8 per value, non-zero = defective, or NULL (no flag).  h_missing: unsigned [asize], non-zero = the whole
 * SAI is to be reconstructed, or NULL (none); a missing SAI must be non-empty in h_mask.  (s, t) of an SAI index as in the view
 * synthesis.  One GPU: contexts with a communicator or a shard return 1.
 * Unsound.  A value is unsound when its SAI is missing, or it is flagged, or it is not finite.  A position (q, y, x) is unsound when
 * any of its C values is; v_q(y, x) = 1 on sound positions, 0 on unsound ones.
 * Targets: every non-empty SAI with at least one unsound position (a missing SAI: every position).
 * Sources of target m: the SAIs q != m that are non-empty and not missing, with max(|s_q - s_m|, |t_q - t_m|) <= ang_radius, in
 * increasing index order; n <= 24 of them.  A source may itself be a target; only its sound positions count.  A target with n = 0 takes
 * no part in the sweep (its unsound values go to the rim fill below).
 * Per hypothesis d, in the order 0, -1, +1, ..., -D, +D, with the warp and the reflection rho of the view synthesis (sy = rho_H(y - d
 * (s_q - s_m)), sx = rho_W(x - d (t_q - t_m))):
 *   a_{q,d}(y, x) = v_q(sy, sx); n_d = sum_q a_{q,d}.
 *   Mean: mu_d = S r[n_d]; S adds the warped values with a_{q,d} = 1 in source order from +0.0f (a value with a_{q,d} = 0 is passed
 *   over by a selection: it never enters an operation, so a NaN in it cannot leak); r[k] = (float)(1.0 / k), r[0] = 0.
 *   Error: e_d = sum_c sum_{q: a_{q,d} = 1} (w_{q,d} - mu_d)^2 from +0.0f, c outer, q inner, every operation rounded on its own.
 *   Scaled error: for n_d >= 2 the cell carries evidence and e'_d = e_d f[n][n_d], f[n][k] = (float)((n - 1) / (k - 1)) computed in
 *   double; for n_d < 2 it carries none: e'_d = +0.0f and it does not count.
 * Box: S_e = the two-pass box sum of e' of the view synthesis (horizontal, then vertical, from +0.0f, mirrored); S_k = the number of
 * evidence cells of the same box, an integer; E_d = S_k = 0 ? +inf : S_e g[S_k], g[k] = (float)((2r + 1)^2 / k) computed in double.
 * Decision, as in the view synthesis: the first hypothesis is taken, a later one replaces the best only if E_d < E_best (ties keep the
 * smaller |d|; +inf never wins, so d* = 0 without evidence anywhere).
 * Fill.  At an unsound position (y, x) of a target with n >= 1 and n_{d*}(y, x) >= min_valid every unsound value becomes mu_{d*} of
 * its channel: code 1.  The values still unsound after that (and a mean that came out not finite) go through the onion-peel fill of
 * the defect inpainting, which sees the values just written as sound: code 2.  What that fill leaves keeps the input's bits: code 3.
 * Sound values are copied: code 0.
 * Outputs: the filled light field on every non-empty SAI (planes of empty SAIs are not written); d_codes (optional), uint8 per value on
 * the non-empty SAIs; d_disp (optional), int8 [asize][H*W], d* at the unsound positions of the targets with n >= 1 (nothing else is
 * written); the counts of lfbm5d_repair_result.
 * Loop.  f = code != 0; x_0 = the fill; x_k = f ? step1(x_{k-1}, max(tau_k, sigma_noise)) : y, on the schedule and with the shared
 * loop of the defect inpainting.  K = 0 is the fill alone.  K >= 1 with a code-3 value returns 1 with a message, after `out` is filled.
 * Exactness.  (1) With no flag, no value that is not finite and only missing SAIs as targets every table factor is exactly 1.0f: the
 * synthesised planes and d* equal lfbm5d_view_fill_device bit for bit (min_valid <= n).  (2) Sums in a fixed order, integer atomics
 * only: the GPU equals the numpy model of tests/repair_model.py bit for bit in values, codes, disparities and counts, and repeated calls
 * return the same bits.
 * Limits: integer disparities only; no occlusion reasoning; validity is per position, not per channel (one flagged channel makes the
 * position useless as a source); one sweep, the fill is not iterated (a value filled from other views is no source for another);
 * one GPU; min_valid's default is the best row of a sweep on one light field (profiles/repair_defaults.txt).
 */
#ifndef LFBM5D_REPAIR_H
#define LFBM5D_REPAIR_H

typedef struct {
    unsigned max_disparity; /* D, 0..8                                                                                 */
    unsigned box_radius;    /* r, 0..7                                                                                 */
    unsigned ang_radius;    /* 1 or 2                                                                                  */
    unsigned min_valid;     /* 1..24: valid sources at d* a position needs to be filled from the other views           */
    unsigned iterations;    /* K refinement steps; 0 = the fill alone                                                  */
    float sigma_start;      /* tau_1 > 0                                                                               */
    float sigma_end;        /* tau_K, 0 < sigma_end <= sigma_start                                                     */
    float sigma_noise;      /* the noise level of the sound values: a floor under the schedule; >= 0                   */
} lfbm5d_repair_params;
typedef struct {
    unsigned missing;       /* SAIs marked missing                                                                     */
    unsigned targets;       /* SAIs with an unsound position                                                           */
    unsigned swept;         /* ... that have a source                                                                  */
    unsigned passes;        /* of the onion-peel fill                                                                  */
    unsigned long long values;             /* values of the non-empty SAIs                                             */
    unsigned long long flagged;            /* non-zero flags on the non-empty SAIs                                     */
    unsigned long long unsound[3];         /* per stored channel: views + rim + left                                   */
    unsigned long long views[3];           /* code 1                                                                   */
    unsigned long long rim[3];             /* code 2                                                                   */
    unsigned long long left[3];            /* code 3                                                                   */
    unsigned long long positions;          /* positions the sweep wrote a value at                                     */
    unsigned long long disparity_hist[17]; /* those positions per d*, index d + 8                                      */
} lfbm5d_repair_result;
/* Host only: D = 4, r = 3, ang_radius = 1, K and the sigmas of lfbm5d_view_defaults; min_valid from profiles/repair_defaults.txt. */
void lfbm5d_repair_defaults(lfbm5d_repair_params* out);
/* The fill alone.  1 with a message: a NULL required buffer, C, W / H, a parameter out of range, ang_major, a missing SAI masked
 * empty, nothing to repair, d_out overlapping d_in, d_codes or d_disp overlapping a light field, a context with a communicator or
 * shard.  The loop's fields of params are not looked at.  out or NULL. */
int lfbm5d_repair_fill_device(lfbm5d_ctx* ctx, const lfbm5d_repair_params* params, const float* d_in, const unsigned char* d_flags_in,
                              const unsigned* h_mask, const unsigned* h_missing, float* d_out, unsigned char* d_codes, signed char* d_disp,
                              unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C,
                              lfbm5d_repair_result* out);
/* The fill and the loop: d_out = x_K on every non-empty SAI.  P = the hard-thresholding step's parameters (its sigma is replaced step
 * by step), an = its angular search window. */
int lfbm5d_repair_device(lfbm5d_ctx* ctx, const lfbm5d_repair_params* params, const lfbm5d_params* P, const float* d_in,
                         const unsigned char* d_flags_in, const unsigned* h_mask, const unsigned* h_missing, float* d_out,
                         unsigned char* d_codes, signed char* d_disp, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                         unsigned W, unsigned H, unsigned C, lfbm5d_repair_result* out);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form.  h_flags_in or NULL; h_codes or NULL: one plane [C*H*W] per non-empty SAI; h_disp or NULL: one
 * plane [H*W] per non-empty SAI (zero where nothing is written).  h_out[st] may be h_in[st]. */
int lfbm5d_repair_host_sai(lfbm5d_ctx* ctx, const lfbm5d_repair_params* params, const lfbm5d_params* P, const float* const* h_in,
                           const unsigned char* const* h_flags_in, const unsigned* h_mask, const unsigned* h_missing, float* const* h_out,
                           unsigned char* const* h_codes, signed char* const* h_disp, unsigned ang_major, unsigned awidth, unsigned aheight,
                           unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_repair_result* out);

#endif
