/*
 * lfbm5d_corr.h -- spatially correlated noise: an autocorrelation of the noise, measured on the GPU or given, turned into one variance
 * factor per 2-D transform coefficient that the group stage thresholds and Wiener-shrinks with.  Part of include/lfbm5d.h, which
 * includes this file at its end; do not include it on its own.  Not in the reference.  Opt-in.
 *
 * Why.  A sub-aperture image decoded from a lenslet camera has been demosaicked and resampled: its noise is low-pass, not white.  The
 * filter thresholds every coefficient of a group at lambda sigma_c sqrt2 and Wiener-shrinks it against sigma_c^2, which under low-pass
 * noise leaves the low 2-D frequencies under-filtered (blotches) and over-smooths the high ones.
 *
 * Autocorrelation.  double acf[7][7], row-major, entry [3 + dy][3 + dx] for the lag (dy, dx), dy, dx = -3..3: the correlation of the
 * noise at two pixels (dy, dx) apart.  acf[3][3] == 1, acf[3 + dy][3 + dx] == acf[3 - dy][3 - dx] exactly, every entry finite and at
 * most 1 in magnitude; anything else is refused with a message.  The white autocorrelation is 1 at lag 0 and 0 elsewhere.
 *
 * Variance table.  M: the forward 2-D transform of the pass as a k^2 x k^2 matrix in double over row-major patches -- tau_2D = dct the
 * orthonormal DCT-II, bior the bior1.5 bank with periodic extension exactly as the kernels run it (k a power of two), id the identity.
 * R: the k^2 x k^2 block-Toeplitz matrix of acf, R[(y, x)][(y', x')] = acf[3 + y' - y][3 + x' - x] within the 7 x 7 lags, 0 outside.
 *     v[pq] = (M R M^T)[pq][pq] / (M M^T)[pq][pq], then v[pq] = max(v[pq], 1 / 64);   v_out = (float)v, s_out = (float)sqrt(v).
 * Numerator and denominator are summed in one order (i ascending, the inner product with R's row over the lags dy, dx ascending), so
 * that the white autocorrelation gives the same double twice and exactly 1.0f everywhere, for every tau_2D and k.  tau_2D = id always
 * gives ones (R's diagonal is 1): a job with id in a step gains nothing in that step.
 * The floor.  Truncating a wide autocorrelation to 7 x 7 lags leaves a matrix R that need not be positive semi-definite, and some v
 * come out tiny or negative (Gaussian taps of width 1.2: -0.12).  1 / 64 is a definition -- no threshold lower than an eighth of white
 * noise's --, not a measured optimum.
 * What the group stage does with it.  The variance of a 5-D coefficient is sigma_c^2 v[pq]: the angular and the stack transform see
 * independent noise and contribute a factor of 1 (the overlap of stacked patches is ignored, as the reference ignores it for white
 * noise).  Per fibre (st, pq): the hard threshold T = lambda sigma_c sqrt2 becomes T s[pq] (before the stack transform's factor), the
 * Wiener sigma_c^2 becomes sigma_c^2 v[pq]; the group weight sums v[pq] per survivor (hard threshold) or value v[pq] (Wiener) in place
 * of 1 and value; 1 / (sigma_c^2 w) and the useSD weight are as they were.  Block matching, tauMatch, aggregation and the window
 * schedule are untouched.  One autocorrelation serves all views and channels (the colour transforms are pointwise and keep its shape).
 * Which kernels.  A pass with a table always runs the general group kernels in their table form (k_group_corr, k_group_big_corr), as
 * option group_generic runs the plain ones: every configuration the general kernels accept (k 2..32, windows 3x3..17x17, every
 * transform combination), and slower than the dedicated kernels.  With the white autocorrelation a job equals the plain job under
 * option group_generic bit for bit (light fields, weights, counters): multiplying by 1.0f is exact.
 * Limits: 7 x 7 lags; one autocorrelation for all views and channels; stack overlap ignored; block matching is not told; general
 * kernels only; no per-SAI BM3D; one GPU (a context with a communicator or a shard is refused); the blind sigma is biased low.
 * The tables live in the context for the duration of the call only, one per step: set on entry, cleared on every exit path.
 *
 * Measuring it (lfbm5d_corr_measure_*).  Every non-overlapping B x B block (B = block: 8, 16 or 32; 0 = 16; whole blocks only, the
 * remainder of W and H is ignored; W, H >= B) of every non-empty SAI and stored channel, in the order SAI (ascending), channel, block
 * row, block column.  Per block, everything in double, no fused multiply-add:
 *     r[y] = x[y][0] + x[y][1] + ... (from +0, x ascending);  m = (r[0] + r[1] + ...) / B^2;  d = x - m;
 *     for the 25 lags (dy, dx), dy = 0: dx = 0..3, dy = 1..3: dx = -3..3:
 *         p[y] = sum over x with 0 <= x, x + dx < B (ascending, from +0) of d[y][x] d[y + dy][x + dx],  y = 0 .. B - dy - 1;
 *         A(dy, dx) = p[0] + p[1] + ... (from +0).
 * The score of a block is A(0, 0).  With n blocks, kth = max(1, ceil(fraction n)) (fraction in (0, 1]), the cut is the kth smallest
 * score and every block with score <= cut is selected (ties at the cut included; fraction 1 selects all).  The selected blocks are
 * summed in block order in chunks of 256 blocks (from +0 each), the chunks in order (from +0): S(d).  Then
 *     C(d) = S(d) / (n_selected (B - dy) (B - |dx|)),  acf(d) = acf(-d) = C(d) / C(0) clamped to [-1, 1],  sigma = sqrt(C(0) B^2 / (B^2 - 1)).
 * If C(0) is not greater than 0 (a constant light field) the result is the white autocorrelation and sigma 0.  Device and host forms
 * and repeated calls return the same bits: only double adds and multiplies in this order, no floating-point atomics.
 * Two uses.  fraction = 1 on a flat-field or dark-frame light field, or on the difference of two captures (sigma is then sqrt2 times
 * one capture's): the calibration, without selection bias.  A small fraction on the noisy light field itself: the blind estimate --
 * the flattest blocks carry little signal.  Selecting blocks by their own energy biases sigma low: with fraction 0.1 and B = 16 on
 * the golden 3x3x256^2 light field by 3..11 % (profiles/corr_defaults.txt has the sweep); take the shape from it and the level from
 * elsewhere (the command's sigma, lfbm5d_noise_level_*).  LFBM5D_CORR_DEFAULT_FRACTION comes from that sweep.
 */

#define LFBM5D_CORR_LAGS 7                    /* lags -3..3 in both directions */
#define LFBM5D_CORR_FLOOR (1.0 / 64.0)
#define LFBM5D_CORR_DEFAULT_FRACTION 0.1

typedef struct lfbm5d_corr_estimate {
    double acf[LFBM5D_CORR_LAGS * LFBM5D_CORR_LAGS];
    double sigma;                /* marginal level of the selected blocks (biased low when fraction < 1) */
    double cut;                  /* the largest score A(0, 0) selected */
    unsigned long long blocks;   /* all blocks */
    unsigned long long selected;
    unsigned block;              /* B as used */
    unsigned reserved;
} lfbm5d_corr_estimate;

/* ---- host only, callable without a GPU or a context ---- */
/* The message of the last failed lfbm5d_corr_* host function on this thread ("" if none). */
const char* lfbm5d_corr_error(void);
/* 0 if acf [49] is an autocorrelation as defined above, else 1 with a message. */
int lfbm5d_corr_check(const double* acf);
/* The autocorrelation of white noise filtered by the taps g [gh][gw] (gh, gw = 1..7; a demosaicking or resampling kernel):
 * acf(dy, dx) = sum_{y, x} g[y][x] g[y + dy][x + dx] / sum g^2, all 7 x 7 lags (lags beyond the taps' extent are 0).  The half with
 * (dy, dx) >= (0, 0) is computed, the other mirrored.  1 with a message: NULL, a size outside 1..7, a tap that is not finite, all taps 0. */
int lfbm5d_corr_from_kernel(const double* g, unsigned gh, unsigned gw, double* acf_out);
/* The variance table of a pass.  tau_2D: LFBM5D_ID, LFBM5D_DCT or LFBM5D_BIOR; k = 2..32 (bior: a power of two).  s_out, v_out [k*k]
 * (either may be NULL); clamped (or NULL) receives the number of entries raised to the floor.  1 with a message otherwise. */
int lfbm5d_corr_table(const double* acf, unsigned tau_2D, unsigned k, float* s_out, float* v_out, unsigned* clamped);

/* ---- measuring: see above.  d_lf [asize][C][H][W] (device) or h_lf one pointer per SAI (host; ignored for empty SAIs); h_mask [asize].
 * fraction 0 means LFBM5D_CORR_DEFAULT_FRACTION.  1 with a message: NULL pointers, chnls not 1 or 3, a block size other than 0, 8, 16,
 * 32, W or H below it, a fraction outside (0, 1] (0 apart), no non-empty SAI, a context with a communicator or a shard. ---- */
int lfbm5d_corr_measure_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                               unsigned C, unsigned block, double fraction, lfbm5d_corr_estimate* out);
int lfbm5d_corr_measure_host_sai(lfbm5d_ctx* ctx, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                 unsigned C, unsigned block, double fraction, lfbm5d_corr_estimate* out);

/* ---- the jobs: lfbm5d_denoise_device / _host_sai, lfbm5d_step1_device, lfbm5d_step2_device with an autocorrelation h_acf [49] (host).
 * The tail arguments are theirs.  1 with a message: what the plain jobs reject, a bad autocorrelation, a context with a communicator or
 * a shard. ---- */
int lfbm5d_denoise_corr_device(lfbm5d_ctx* ctx, const double* h_acf, const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy,
                               const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth,
                               unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C);
int lfbm5d_denoise_corr_host_sai(lfbm5d_ctx* ctx, const double* h_acf, const lfbm5d_params* P1, const lfbm5d_params* P2,
                                 float* const* h_noisy, const unsigned* h_mask, float* const* h_basic, float* const* h_denoised,
                                 unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H,
                                 unsigned C);
int lfbm5d_step1_corr_device(lfbm5d_ctx* ctx, const double* h_acf, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask,
                             float* d_basic, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H,
                             unsigned C);
int lfbm5d_step2_corr_device(lfbm5d_ctx* ctx, const double* h_acf, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask,
                             float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                             unsigned W, unsigned H, unsigned C);
/* lfbm5d_debug_group (the group launch of a core pass alone) with the table of h_acf: the test seam of the table kernels.  The per-SAI
 * BM3D flavour (d->bm3d) is refused. */
int lfbm5d_debug_group_corr(lfbm5d_ctx* ctx, const lfbm5d_group_debug* d, const double* h_acf);
