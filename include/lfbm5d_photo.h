/*
 * lfbm5d_photo.h -- photometric equalisation: one multiplicative gain per sub-aperture image and stored channel, estimated from what
 * the other views say and divided out ahead of every other stage.  Part of include/lfbm5d.h, which includes this file at its end; do not
 * include it on its own.  Not in the reference.  Opt-in.
 *
 * Why.  Block matching across SAIs, the angular transforms, the plane sweep and the consistency check all assume that a scene point has
 * the same value in every view.  Lenslet cameras vignette (edge views are dimmer) and the cameras of an array differ in exposure and
 * white balance.  Until now the only answer was the consistency check's bad-SAI decision, which throws such a view away.
 *
 * Model.  I_{m,c} = g_{m,c} y: a gain per SAI m and stored channel c, no offset.  Data, h_mask, (s, t) by ang_major, C = 1 or 3,
 * W, H >= 2 as for the consistency check.  One GPU: contexts with a communicator or a shard return 1.
 * Prediction.  An SAI is tested if it is non-empty and has at least min_sources sources; the sources are the consistency check's with
 * an empty exclude set (every other non-empty SAI within ang_radius, in increasing index order, n of them).  mu and d* are the view
 * synthesis' sweep at (max_disparity, box_radius, ang_radius, steps in {1, 2, 4}) with the SAI itself left out.
 * Ratio key.  No division, no libm; float32, every operation rounded on its own (no fused multiply-add).  Edges e_j, j = 0..1024:
 * e_j = 2^(j div 256 - 2) (1 + (j mod 256) / 256), so e_0 = 1/4 and e_1024 = 4: 256 keys per octave, every edge a float32 (its bits
 * are (125 << 23) + (j << 15)).  key(I, mu) = #{ j : I >= fl(e_j mu) } in 0..1025 (LFBM5D_PHOTO_KEYS keys).  For mu >= 0 the products
 * are monotone in j and the key is an 11-step binary search.
 * Admission.  A value is counted when I and mu are finite and (float)lo <= mu <= (float)hi.  The test is on mu alone: selecting on the
 * noisy I would truncate its noise and bias the ratio; hi also keeps the saturated values of a brighter view out.  The others are
 * counted by reason: not finite (I or mu), else out of range.
 * Statistics.  Per tested SAI and channel an integer histogram [1026].  per_channel = 0: the channels' histograms are added and every
 * channel gets the one gain.
 * Ratio of a histogram (host, double; lfbm5d_photo_ratio).  N = sum h, T = (N + 1) div 2, k* the first key whose cumulative count
 * reaches T, `before` the count below it: r = e_{k*-1} + (e_{k*} - e_{k*-1}) ((T - before) - 0.5) / h[k*].  The (SAI, channel) is
 * unfit when N < min_count or k* is an end key (a ratio outside 1/4..4 is no photometric difference to repair): r = 1, gain 1.
 * Solve (host, double, fixed order, only + - x /; lfbm5d_photo_solve).  mu is the plain mean of n sources, so r_m = g_m / mean_q g_q.
 * g = 1; then 512 times, for every fitted m at once, h_m = (g_m + r_m (sum_q g_q, in source order, from +0) / n_m) / 2; every
 * fitted h is divided by the lower median of the fitted h, or with an anchor by h of the anchor SAI (which then stays exactly 1; an
 * anchor that is not fitted has h = 1); g <- h.  Unfit and untested SAIs keep g = 1 and still count as sources.  The 1/2 makes the
 * iteration converge on 1 x N and N x 1 layouts, whose neighbour graph is bipartite.
 * Rounds.  x = the input, G = 1.  For k = 1..max_rounds: sweep and histograms on x; the ratios; residual = max |r - 1| over the
 * fitted (SAI, channel) pairs (0 without one); residual <= tol: converged = 1, stop; otherwise solve g, x <- x (float)(1.0 / g) (one
 * float32 multiplication per value of every non-empty SAI), G <- G g.
 * Integer atomics only; ratios and gains on the host in double on integer histograms: the GPU equals the numpy model of
 * tests/photo_model.py bit for bit in every integer and float it returns, and repeated calls return the same bits.
 * Limits: gain only (no offset, no vignetting inside a view, no spatially varying gain); after the division a view's noise is sigma / g:
 * the filter is told only through the jobs of include/lfbm5d_views.h (lfbm5d_views_from_gains turns the gains into their view table),
 * the plain jobs and the consistency check are not (it still calls a view bad that is merely noisier; gain_min / gain_max tell the
 * caller); the common factor is free (lower median, or the anchor); one GPU; the defaults are one row of a sweep on one light field and
 * a translated view of it, both unclipped (profiles/photo_defaults.txt): it cannot weigh hi's guard against saturated values.
 */
#define LFBM5D_PHOTO_KEYS 1026
#define LFBM5D_PHOTO_EDGES 1025
#define LFBM5D_PHOTO_SOLVE_STEPS 512
#define LFBM5D_PHOTO_NO_ANCHOR 0xffffffffu

typedef struct {
    unsigned max_disparity;       /* D, 0..8, and                                                                     */
    unsigned box_radius;          /* r, 0..7, and                                                                     */
    unsigned ang_radius;          /* 1 or 2: the sweep's, as in lfbm5d_consist_params                                 */
    unsigned steps;               /* 1, 2 or 4 hypotheses per pixel in the sweep                                      */
    unsigned min_sources;         /* 2..24: an SAI with fewer sources is untested                                     */
    unsigned max_rounds;          /* 1..64: sweeps at most                                                            */
    unsigned per_channel;         /* 1: a gain per stored channel; 0: one gain per SAI from the pooled histograms     */
    unsigned anchor;              /* the SAI whose gain stays 1, or LFBM5D_PHOTO_NO_ANCHOR (the lower median is 1)    */
    unsigned long long min_count; /* an (SAI, channel) with fewer admitted values is unfit; >= 1                      */
    double tol;                   /* stop when every fitted ratio is within tol of 1; finite, >= 0                    */
    double lo, hi;                /* a value is admitted when (float)lo <= mu <= (float)hi; 0 <= lo <= hi <= 1e30      */
} lfbm5d_photo_params;
typedef struct {
    double residual;                      /* max |r - 1| over the fitted pairs at the last sweep                       */
    double gain_min, gain_max;            /* over the stored channels of the non-empty SAIs                            */
    unsigned long long admitted;          /* values counted by the last sweep                                          */
    unsigned long long skipped_nonfinite; /* values of that sweep with I or mu not finite                              */
    unsigned long long skipped_range;     /* finite values of that sweep with mu outside lo..hi                        */
    unsigned rounds;                      /* sweeps                                                                    */
    unsigned converged;                   /* 1: the last sweep's residual was within tol                               */
    unsigned fitted, untested, unfit;     /* SAIs in state 1, 2, 3                                                     */
} lfbm5d_photo_result;

/* ---- host only, callable without a GPU ---- */
/* D = 4, r = 3, ang_radius = 1 (the consistency check's), steps = 1, min_sources = 3, max_rounds = 3, per_channel = 1, no anchor,
 * min_count = 256, tol = 1 / 256, lo = 4, hi = 240 (the row picked by the sweep in profiles/photo_defaults.txt). */
void lfbm5d_photo_defaults(lfbm5d_photo_params* out);
/* The 1025 edges e_j as float32. */
void lfbm5d_photo_edges(float* out);
/* The ratio of one histogram [1026].  0: fitted, *ratio = r.  1: unfit (fewer than min_count values, the median in an end key) or a
 * NULL pointer; *ratio = 1. */
int lfbm5d_photo_ratio(const unsigned long long* hist, unsigned long long min_count, double* ratio);
/* The solve on asize SAIs: ratio [asize]; n_src [asize] and src [asize][24], the sources of every fitted SAI in order; fitted [asize]
 * (non-zero: fitted); anchor < asize or LFBM5D_PHOTO_NO_ANCHOR; gain [asize] is written.  1 for a NULL pointer, an anchor or a source
 * out of range, or a fitted SAI with no source or more than 24. */
int lfbm5d_photo_solve(unsigned asize, const double* ratio, const unsigned* n_src, const unsigned* src, const unsigned* fitted,
                       unsigned anchor, double* gain);

/* ---- on the GPU ---- */
/* d_in is only read.  d_out: float32 [asize][C*H*W] in HBM, x of the last round on every non-empty SAI (planes of empty SAIs are not
 * written); it may not overlap d_in.  h_gain [asize][3] (host): G, 1 for empty SAIs and channels that are not stored.  h_state [asize]
 * (host): 0 empty, 1 fitted, 2 untested, 3 unfit in some channel (at the last sweep).  Optional (NULL): h_hist [asize][C][1026] (host),
 * the last sweep's histograms; out.  1 with a message: a NULL required buffer, overlapping d_in and d_out, C, W / H, ang_major,
 * awidth / aheight, each parameter out of range, a mask without a non-empty SAI, a light field too large, a context with a
 * communicator or shard. */
int lfbm5d_photo_device(lfbm5d_ctx* ctx, const lfbm5d_photo_params* params, const float* d_in, const unsigned* h_mask, float* d_out,
                        double* h_gain, unsigned* h_state, unsigned long long* h_hist, unsigned ang_major, unsigned awidth,
                        unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_photo_result* out);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form.  h_out[st] may be h_in[st]. */
int lfbm5d_photo_host_sai(lfbm5d_ctx* ctx, const lfbm5d_photo_params* params, const float* const* h_in, const unsigned* h_mask,
                          float* const* h_out, double* h_gain, unsigned* h_state, unsigned long long* h_hist, unsigned ang_major,
                          unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_photo_result* out);
/* out = in (float)(invert ? G : 1.0 / G) per non-empty SAI and stored channel, G = h_gain [asize][3] (finite and positive); one
 * float32 multiplication per value.  invert = 1 after denoising gives every view its own photometry back.  d_out may be d_in; any
 * other overlap returns 1.  Planes of empty SAIs are not written. */
int lfbm5d_photo_apply_device(lfbm5d_ctx* ctx, const float* d_in, const unsigned* h_mask, const double* h_gain, unsigned invert,
                              float* d_out, unsigned awidth, unsigned aheight, unsigned W, unsigned H, unsigned C);
int lfbm5d_photo_apply_host_sai(lfbm5d_ctx* ctx, const float* const* h_in, const unsigned* h_mask, const double* h_gain,
                                unsigned invert, float* const* h_out, unsigned awidth, unsigned aheight, unsigned W, unsigned H,
                                unsigned C);
