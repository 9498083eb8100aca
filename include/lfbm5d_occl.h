/*
 * lfbm5d_occl.h -- the occlusion-aware forms of the view synthesis: the plane sweep that, beside the full set of a missing view's
 * sources, evaluates four half-planes of them.  Part of include/lfbm5d.h, which includes this file at its end; do not include it on its
 * own.  Not in the reference.  Opt-in.
 *
 * Why.  For a hypothesis the plain sweep's cost is the scatter of all n warped sources.  Behind a depth edge the views on one side of
 * the missing SAI see the background and the views on the other side see the occluder: the scatter is large for every hypothesis, the
 * winner is arbitrary and the value mixes two surfaces.  A background point hidden from the views on one side is visible in the views
 * on the other side (Kang and Szeliski's source selection), so a half-plane of sources agrees where the full set cannot.
 *
 * Definition.  Everything in the view-synthesis section of include/lfbm5d.h stands: sources, warp for Q = steps in {1, 2, 4}, box,
 * hypothesis order, strict <, mirror rho_n.  Only the per-cell error and the output value change, under the parameter occl_ratio
 * (float, written rho below where no mirror is meant):
 *   occl_ratio = 0      the feature is off: the call is the *_steps_* call with the same arguments, in code path and bits; d_set / h_set
 *                       are not written and the occl result is all zero.
 *   occl_ratio >= 1     the feature is on (finite).
 *   anything else       (between 0 and 1, negative, NaN, infinite) returns 1 with a message.
 * Per synthesised SAI m, with (ds, dt) = (s_q - s_m, t_q - t_m) per source q:
 * Sets.  Set 0 is every source (n members).  Candidates in this order: set 1 = {dt <= 0}, set 2 = {dt >= 0}, set 3 = {ds <= 0},
 *   set 4 = {ds >= 0}; each keeps the increasing source order; n_k members.  The half-planes include the missing view's own row or
 *   column: with strict half-planes the sources of one side share dt (or ds) and the cost is blind to the disparity along that axis.
 *   A candidate is admissible when 2 <= n_k < n.  The sets depend on the table row alone, not on position or hypothesis.
 * Per set k, cell (y, x) and hypothesis j.
 *   Mean: mu_k(c) = (((+0.0f + w_a) + w_b) + ...) r[n_k] over the members in order, r[n] = (float)(1.0 / n).
 *   Scatter: v_k = sum_c sum_{q in k} (w_q - mu_k(c))^2 from +0.0f, c outer, q inner.
 *   Normalised error: e^_k = v_k g[n_k], g[n] = (float)(1.0 / (n - 1)), g[1] = 0.
 *   Every difference, product and sum is rounded on its own (no fused multiply-add).
 * Choice k*(cell, j).  Among the admissible candidates in order a later one replaces the best so far only if its e^ is strictly
 *   smaller.  The best candidate replaces set 0 only if (e^_best rho) < e^_0, the product rounded to float32.  With no admissible
 *   candidate k* = 0.  e_j = e^_{k*}.
 * Box and decision: as in include/lfbm5d.h, on e_j.
 * Output.  At j* the choice is made again for the cell itself (from the cell's own e^_k at j*, not from the boxed sums); the view is
 *   mu_{k*} for all C channels; d_disp holds j*; d_set (optional) holds k*.
 * Consequences: n = 1 gives E = 0 everywhere and a copy of the source; n = 2 has no admissible candidate and g = 1, so values and j*
 * are the plain sweep's; a corner SAI at ang_radius 1 (n = 3, the candidates have 1 or 3 members, g = 0.5 is exact) gives the plain
 * sweep's values and j*; a hypothesis with j a multiple of Q warps as the integer sweep, in bits.
 * The loop (iterations >= 1) is unchanged: the same flags, projections and refinement steps.
 * The GPU equals the numpy model of tests/occl_model.py bit for bit: values, j*, k*, both histograms; repeated calls return the same
 * bits.
 *
 * Each function has the arguments of its *_steps_* sibling (include/lfbm5d_steps.h) plus
 *   occl_ratio     float, behind `steps`.
 *   d_set / h_set  behind the disparity output: unsigned char [asize][H*W] on the device (per-SAI pointers in the host form, needed for
 *                  the missing SAIs), or NULL; k* in 0..4 on the planes of the synthesised SAIs, other planes are not written.  d_set must
 *                  not overlap d_in or d_out.
 *   occl           lfbm5d_view_occl_result* at the end, or NULL: set_hist[k] = positions of the synthesised SAIs with k* = k.
 * The *_steps_* forms are the occl_ratio = 0 calls of these: there is one implementation.
 *
 * Limits: four half-planes and nothing finer (no per-source visibility, no ordering constraint); with 3 x 3 views and the centre missing a
 * half-plane has 5 of 8 sources, so its mean averages less noise than the full set's -- occl_ratio is what keeps it from winning on
 * noise alone; at an edge SAI one candidate is every source and is not admissible, at a corner SAI none is admissible; the
 * consistency check's own sweep is the plain one (its spread test already keeps depth edges out); the default ratio is the best row of one sweep on one light field plus two synthetic scenes
 * (profiles/occl_defaults.txt); one GPU.
 */
#ifndef LFBM5D_OCCL_H
#define LFBM5D_OCCL_H

#ifndef LFBM5D_H
#error "include lfbm5d.h, which includes this file"
#endif

#define LFBM5D_VIEW_OCCL_SETS 5

typedef struct {
    unsigned long long set_hist[LFBM5D_VIEW_OCCL_SETS]; /* positions per k*: 0 the full set, 1..4 the half-planes */
} lfbm5d_view_occl_result;

/* the ratio the library ships (profiles/occl_defaults.txt); host only */
float lfbm5d_view_occl_default(void);

int lfbm5d_view_fill_occl_device(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, unsigned steps, float occl_ratio, const float* d_in,
                                 const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned char* d_set,
                                 unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C,
                                 lfbm5d_view_result* out, unsigned long long* h_hist_steps, lfbm5d_view_occl_result* occl);
int lfbm5d_view_occl_device(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, unsigned steps, float occl_ratio, const lfbm5d_params* P,
                            const float* d_in, const unsigned* h_mask, const unsigned* h_missing, float* d_out, signed char* d_disp,
                            unsigned char* d_set, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H,
                            unsigned C, lfbm5d_view_result* out, unsigned long long* h_hist_steps, lfbm5d_view_occl_result* occl);
int lfbm5d_view_occl_host_sai(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, unsigned steps, float occl_ratio, const lfbm5d_params* P,
                              const float* const* h_in, const unsigned* h_mask, const unsigned* h_missing, float* const* h_out,
                              signed char* const* h_disp, unsigned char* const* h_set, unsigned ang_major, unsigned awidth,
                              unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out,
                              unsigned long long* h_hist_steps, lfbm5d_view_occl_result* occl);

#endif
