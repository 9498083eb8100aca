/*
 * run_bm5d.h -- drop-in declarations with the reference's exact signatures
 * (V-Sense/LFBM5D src/bm5d.h:11-35 and :38-62).  A program written against the reference's bm5d.h
 * links against liblfbm5d_dropin.so instead of the reference's bm5d.cpp / bm5d_core_processing.cpp
 * and runs the whole path on the GPU through the C-ABI of include/lfbm5d.h.
 */
#ifndef LFBM5D_RUN_BM5D_H
#define LFBM5D_RUN_BM5D_H

#include <vector>

//! Main function (hard-thresholding step) -- same argument list as the reference.  LF_noisy is
//! colour-transformed and transformed back in place (lossy for OPP, like the reference),
//! LF_basic is (re)sized and filled.  nb_threads is accepted for source compatibility; the GPU path
//! has the semantics of nb_threads == 1 (no tile-halo discard) unless LFBM5D_TILED is set in the
//! environment, in which case the reference's tile mode with nb_threads tiles is reproduced.
int run_bm5d_1st_step(
    const float sigma
,   const float lambdaHard5D
,   std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard
,   const unsigned nSim
,   const unsigned nDisp
,   const unsigned kHard
,   const unsigned pHard
,   const bool     useSD
,   const unsigned tau_2D
,         unsigned tau_4D
,   const unsigned tau_5D
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Main function (Wiener step)
int run_bm5d_2nd_step(
    const float sigma
,   std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NWien
,   const unsigned nSim
,   const unsigned nDisp
,   const unsigned kWien
,   const unsigned pWien
,   const bool     useSD
,   const unsigned tau_2D
,         unsigned tau_4D
,   const unsigned tau_5D
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Both steps as ONE job -- not in the reference (whose main.cpp:195, :242 calls the two functions above one after the other; BASELINE.json
//! names it "run_bm5d()"): == run_bm5d_1st_step(...) followed by run_bm5d_2nd_step(...) with the same arguments, bit for bit, but
//! the windows of both steps run as one dependency graph on the GPU(s) (lfbm5d_denoise_host, include/lfbm5d.h).
int run_bm5d(
    const float sigma
,   const float lambdaHard5D
,   std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard
,   const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard
,   const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien
,   const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Blind noise level -- not in the reference: the standard deviation of additive white Gaussian noise in LF (the units of `sigma`:
//! grey levels of the channels as stored), estimated on the GPU from the light field itself (lfbm5d_noise_level_host_sai,
//! include/lfbm5d.h; 8 x 8 patches pooled over every non-empty SAI and channel).  What to pass as `sigma` to the functions above
//! when nobody knows it (the reference's LFSourceDir = none).  LF is only read.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the
//! message on stdout.
int noise_level_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   float &sigma
);

//! Impulse repair -- not in the reference, whose authors run such a stage in front of it: hot and dead pixels, salt and pepper and values
//! that are not finite are detected on the GPU (rank-ordered absolute differences against k x the channel's median, include/lfbm5d.h) and
//! replaced in LF by the lower median of their sound neighbours, before noise_level_LF / pg_estimate_LF and the filter see them.  k = 8 is
//! the default of the C-ABI.  `flagged` and `left` (flagged, but without a sound neighbour: unchanged) count values over all channels;
//! thresholds[3] receives what was applied per stored channel.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int impulse_repair_LF(
    std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   double k
,   unsigned long long &flagged
,   unsigned long long &left
,   double thresholds[3]
);

//! Signal-dependent noise -- not in the reference: the Poisson-Gaussian model var(z | y) = a y + b (grey levels of the channels as stored,
//! 0..255 scale) of a noisy light field, estimated on the GPU with every non-empty SAI and channel pooled (lfbm5d_pg_estimate_host_sai,
//! include/lfbm5d.h).  LF is only read.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int pg_estimate_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   double &a
,   double &b
);

//! The generalised Anscombe transform of LF under the model (a, b) of every channel, in place, on the GPU (lfbm5d_pg_forward_device):
//! afterwards the noise is white Gaussian of standard deviation `sigma` (returned; lfbm5d_pg_scale) and any denoiser for such noise
//! applies -- run_bm5d_*, run_bm3d_LF.  pg_inverse_LF is the exact unbiased inverse for the denoised result.  A rejected model (a < 0,
//! 3/8 a^2 + b <= 0) returns EXIT_FAILURE with the message on stdout.
int pg_forward_LF(
    double a
,   double b
,   std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   float &sigma
);
int pg_inverse_LF(
    double a
,   double b
,   std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
);

//! run_bm5d under Poisson-Gaussian noise (lfbm5d_denoise_pg_host_sai): forward transform, both steps as one job with sigma = the
//! model's scale, inverse transform of LF_basic and LF_denoised.  estimate = true: (a, b) are estimated from LF_noisy first and
//! returned; otherwise they are the model to use.  LF_noisy is only read; `sigma` receives the sigma the job ran with.
int denoise_pg_LF(
    double &a
,   double &b
,   const bool estimate
,   float &sigma
,   const float lambdaHard5D
,   const std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard
,   const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard
,   const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien
,   const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Data clipped to lo..hi (8-bit files: 0..255) -- not in the reference: the noise sigma of such a light field from the intensity levels
//! the clipping left alone (lfbm5d_noise_level_clipped_host_sai, include/lfbm5d.h).  `levels` and `f_max` receive how many levels
//! counted and the largest censored fraction admitted (above 0.1: heavily clipped, the estimate leans on touched levels).  LF is only
//! read.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int noise_level_clipped_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   double lo
,   double hi
,   float &sigma
,   unsigned &levels
,   double &f_max
);

//! The inverse of the clipped mean, in place on the GPU (lfbm5d_declip_host_sai): what takes a light field denoised from data clipped
//! to lo..hi under noise of `sigma` (any denoiser: run_bm5d_*, run_bm3d_LF) back to the unclipped signal.
int declip_LF(
    double sigma
,   double lo
,   double hi
,   std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
);

//! run_bm5d on data clipped to lo..hi (lfbm5d_denoise_clipped_host_sai): sigma <= 0: the clipping-aware estimate of LF_noisy first,
//! returned in `sigma`; both steps as one job with that sigma; LF_basic and LF_denoised declipped.  LF_noisy is only read.
int denoise_clipped_LF(
    float &sigma
,   double lo
,   double hi
,   const float lambdaHard5D
,   const std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard
,   const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard
,   const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien
,   const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Poisson-Gaussian noise on data rounded and clipped to lo..hi (8-bit files) -- not in the reference: the model
//! sigma^2(y) = a (y - lo) + b of such a light field, fitted on the GPU's block statistics over the intensity levels the clipping left
//! alone (lfbm5d_pgclip_estimate_host_sai, include/lfbm5d_pgclip.h).  `levels` and `f_max` as for noise_level_clipped_LF.  LF is only read.
//! Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int pgclip_estimate_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   double lo
,   double hi
,   double &a
,   double &b
,   unsigned &levels
,   double &f_max
);

//! The stabiliser of the clipped model (a, b, lo, hi) and its exact unbiased inverse, in place on the GPU by table look-up
//! (lfbm5d_pgclip_curves, lfbm5d_pgclip_forward_device / _inverse_device): after pgclip_forward_LF the noise has the standard deviation
//! `sigma` (returned) and any denoiser applies; pgclip_inverse_LF takes the denoised result back to the unclipped signal in lo..hi.  A
//! model that is invalid or outside the accepted domain returns EXIT_FAILURE with the message on stdout.
int pgclip_forward_LF(
    double a
,   double b
,   double lo
,   double hi
,   std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   float &sigma
);
int pgclip_inverse_LF(
    double a
,   double b
,   double lo
,   double hi
,   std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
);

//! run_bm5d on clipped Poisson-Gaussian data (lfbm5d_denoise_pgclip_host_sai): estimate = true: (a, b) are estimated from LF_noisy at
//! the range lo..hi first and returned (with `levels` and `f_max`); otherwise they are the model to use.  Forward map, both steps as one
//! job with sigma = the curves' s, inverse map of LF_basic and LF_denoised.  LF_noisy is only read; `sigma` receives s.
int denoise_pgclip_LF(
    double &a
,   double &b
,   double lo
,   double hi
,   const bool estimate
,   float &sigma
,   unsigned &levels
,   double &f_max
,   const float lambdaHard5D
,   const std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard
,   const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard
,   const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien
,   const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Quality of LF_2 against LF_1 on the GPU -- compute_psnr_LF (utilities_LF.cpp:639-692) with its argument order, the sizes and the
//! SSIM triple added: per-SAI PSNR, RMSE and SSIM (0 for empty SAIs) with their mean and population standard deviation over the
//! non-empty SAIs (lfbm5d_quality_host_sai, include/lfbm5d.h: double sums, peak 255, SSIM with the 11 x 11 Gaussian window over every
//! valid position; width, height >= 11).  Both light fields are only read.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message
//! on stdout.
int quality_LF(
    const std::vector<std::vector<float> > &LF_1
,   const std::vector<std::vector<float> > &LF_2
,   const std::vector<unsigned> &LF_SAI_mask
,   unsigned width
,   unsigned height
,   unsigned chnls
,   std::vector<float> &psnr
,   float &avg_psnr
,   float &std_psnr
,   std::vector<float> &rmse
,   float &avg_rmse
,   float &std_rmse
,   std::vector<float> &ssim
,   float &avg_ssim
,   float &std_ssim
);

//! LFBM5D_REPORT_SSIM of the command lines, read here with the drop-in's other program-level variables: 0 = unset, 1 = "1" (report
//! SSIM through quality_LF next to every PSNR), -1 = any other value (the message is on stdout).
int report_ssim_mode();

//! Defect inpainting -- not in the reference: the values that `flags` names (one uint8 plane per SAI, non-zero = defective) and every value
//! that is not finite are filled on the GPU from their rim inwards and refined by `iterations` hard-thresholding steps whose sigma falls
//! from sigmaStart to sigmaEnd but not below sigmaNoise, the sound data being put back after every step (lfbm5d_inpaint_host_sai,
//! include/lfbm5d.h).  LF is repaired in place.  iterations < 0, sigmaStart = 0, sigmaEnd = 0: the library's defaults
//! (lfbm5d_inpaint_defaults); iterations = 0: the fill alone.  `flagged` and `left` (values of a plane without one sound value, unchanged)
//! count over all channels; `passes` is the depth of the deepest region.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int inpaint_LF(
    std::vector<std::vector<float> > &LF
,   const std::vector<std::vector<unsigned char> > &flags
,   const std::vector<unsigned> &LF_SAI_mask
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const int      iterations
,   const float    sigmaStart
,   const float    sigmaEnd
,   const float    sigmaNoise
,   const float    lambdaHard5D
,   const unsigned NHard
,   const unsigned nSim
,   const unsigned nDisp
,   const unsigned kHard
,   const unsigned pHard
,   const bool     useSD
,   const unsigned tau_2D
,         unsigned tau_4D
,   const unsigned tau_5D
,   const unsigned color_space
,   unsigned long long &flagged
,   unsigned long long &left
,   unsigned &passes
);

//! View synthesis -- not in the reference: the SAIs that `missing` marks (non-zero; they must be non-empty in LF_SAI_mask; their vectors
//! are not read and are resized) are synthesised on the GPU from their sound angular neighbours by a plane sweep over the integer
//! disparities -maxDisparity..maxDisparity with a (2 boxRadius + 1)^2 box, sources within angRadius views, and refined by `iterations`
//! hard-thresholding steps whose sigma falls from sigmaStart to sigmaEnd but not below sigmaNoise, the sound SAIs being put back after
//! every step (lfbm5d_view_host_sai, include/lfbm5d.h).  LF is completed in place.  maxDisparity, boxRadius, angRadius, iterations < 0,
//! sigmaStart = 0, sigmaEnd = 0: the library's defaults (lfbm5d_view_defaults); iterations = 0: the synthesis alone.  `left` counts the
//! missing SAIs without a source (unchanged); dmin..dmax is the range of the disparities chosen (0..0 when nothing was synthesised).
//! disparity_steps = 1, 2 or 4 hypotheses per pixel (lfbm5d_view_steps_host_sai; above 1 the sources are interpolated bilinearly and
//! dmin..dmax is in units of 1 / disparity_steps).  occl_ratio = 0: the plain sweep; >= 1: the occlusion-aware sweep
//! (lfbm5d_view_occl_host_sai, include/lfbm5d_occl.h; lfbm5d_view_occl_default() is the ratio the library ships), and set_hist (5
//! counters, or NULL) receives the positions per set chosen (0 the full set, 1..4 the half-planes; all zero with occl_ratio = 0).
//! Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int view_synth_LF(
    std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   const std::vector<unsigned> &missing
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const int      maxDisparity
,   const int      boxRadius
,   const int      angRadius
,   const int      iterations
,   const float    sigmaStart
,   const float    sigmaEnd
,   const float    sigmaNoise
,   const float    lambdaHard5D
,   const unsigned NHard
,   const unsigned nSim
,   const unsigned nDisp
,   const unsigned kHard
,   const unsigned pHard
,   const bool     useSD
,   const unsigned tau_2D
,         unsigned tau_4D
,   const unsigned tau_5D
,   const unsigned color_space
,   unsigned &synthesised
,   unsigned &left
,   int &dmin
,   int &dmax
,   const unsigned disparity_steps = 1
,   const float occl_ratio = 0.0f
,   unsigned long long *set_hist = nullptr
);

//! Joint repair -- not in the reference: the values that `flags` names (one uint8 plane per non-empty SAI, non-zero = defective; an empty
//! vector: no flags), every value that is not finite and every value of the SAIs that `missing` marks (non-zero; an empty vector: none;
//! they must be non-empty in LF_SAI_mask and hold width*height*chnls values, which are not used) are filled on the GPU from the other
//! views by a plane sweep that skips unsound source values, what it cannot reach from the rim of its own plane, and the fill is refined
//! by `iterations` hard-thresholding steps whose sigma falls from sigmaStart to sigmaEnd but not below sigmaNoise, the sound values
//! being put back after every step (lfbm5d_repair_host_sai, include/lfbm5d_repair.h).  LF is repaired in place.  maxDisparity,
//! boxRadius, angRadius, minValid, iterations < 0, sigmaStart = 0, sigmaEnd = 0: the library's defaults (lfbm5d_repair_defaults);
//! iterations = 0: the fill alone.  `counts` receives the values of the non-empty SAIs, the non-zero flags, the SAIs marked missing and the
//! values filled from other views, filled from the rim and left, over all channels; dmin..dmax is the range of the disparities chosen (0..0 when the sweep
//! wrote nothing).  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int repair_LF(
    std::vector<std::vector<float> > &LF
,   const std::vector<std::vector<unsigned char> > &flags
,   const std::vector<unsigned> &LF_SAI_mask
,   const std::vector<unsigned> &missing
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const int      maxDisparity
,   const int      boxRadius
,   const int      angRadius
,   const int      minValid
,   const int      iterations
,   const float    sigmaStart
,   const float    sigmaEnd
,   const float    sigmaNoise
,   const float    lambdaHard5D
,   const unsigned NHard
,   const unsigned nSim
,   const unsigned nDisp
,   const unsigned kHard
,   const unsigned pHard
,   const bool     useSD
,   const unsigned tau_2D
,         unsigned tau_4D
,   const unsigned tau_5D
,   const unsigned color_space
,   unsigned long long counts[6]
,   int &dmin
,   int &dmax
);

//! Consistency check -- not in the reference: every usable SAI is predicted on the GPU from its angular neighbours by the view synthesis'
//! plane sweep with the SAI itself left out; a value is flagged (1) when its residual exceeds k times the light field's median residual
//! and `spread` times the sources' own disagreement, or (2) when it is not finite; an SAI is bad when its median residual stands out
//! among its neighbours' (lfbm5d_consist_host_sai, include/lfbm5d.h).  LF is only read.  `exclude` (empty, or one entry per SAI,
//! non-zero = known bad) is neither tested nor used.  maxDisparity, boxRadius, angRadius, minSources, maxRounds < 0 and k, spread,
//! saiFactor < 0: the library's defaults (lfbm5d_consist_defaults); saiFactor = 0: no bad-SAI decision.  `flags` is resized to one
//! plane of width*height*chnls codes per non-empty SAI (the map of inpaint_LF), `state` to one entry per SAI (0 empty, 1 tested, 2 bad,
//! 3 untested, 4 excluded; the bad ones are the `missing` of view_synth_LF); `flagged` and `nonfinite` count the values with code 1 and
//! code 2 over all channels, `scales` receives the median residual of the three stored channels, `rounds` the sweeps.
//! disparity_steps = 1, 2 or 4 hypotheses per pixel in the sweep (lfbm5d_consist_steps_host_sai).  Returns EXIT_SUCCESS, or
//! EXIT_FAILURE with the message on stdout.
int consist_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   const std::vector<unsigned> &exclude
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const int      maxDisparity
,   const int      boxRadius
,   const int      angRadius
,   const int      minSources
,   const int      maxRounds
,   const double   k
,   const double   spread
,   const double   saiFactor
,   std::vector<std::vector<unsigned char> > &flags
,   std::vector<unsigned> &state
,   unsigned long long &flagged
,   unsigned long long &nonfinite
,   unsigned &bad
,   unsigned &untested
,   unsigned &rounds
,   double scales[3]
,   const unsigned disparity_steps = 1
);

//! Photometric equalisation -- not in the reference: every SAI with enough neighbours is predicted on the GPU from them by the view
//! synthesis' plane sweep with the SAI itself left out, the median ratio of its values to the prediction gives one gain per SAI and
//! stored channel, and the gains are divided out (lfbm5d_photo_host_sai, include/lfbm5d_photo.h).  LF is only read; LF_out is resized
//! to the light field's shape and holds the equalised non-empty SAIs (it may be LF itself).  maxDisparity, boxRadius, angRadius,
//! minSources, maxRounds, perChannel < 0 and tol, lo, hi < 0: the library's defaults (lfbm5d_photo_defaults); anchor < 0: no anchor
//! (the lower median of the gains is 1).  `gains` is resized to 3 doubles per SAI (1 for empty SAIs and channels that are not stored:
//! hand them to apply_gains_LF with invert to restore every view's own photometry), `state` to one entry per SAI (0 empty, 1 fitted,
//! 2 untested, 3 unfit in some channel).  disparity_steps = 1, 2 or 4 hypotheses per pixel in the sweep.  Returns EXIT_SUCCESS, or
//! EXIT_FAILURE with the message on stdout.
int equalise_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_out
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const int      maxDisparity
,   const int      boxRadius
,   const int      angRadius
,   const int      minSources
,   const int      maxRounds
,   const int      perChannel
,   const int      anchor
,   const double   tol
,   const double   lo
,   const double   hi
,   std::vector<double> &gains
,   std::vector<unsigned> &state
,   unsigned &fitted
,   unsigned &untested
,   unsigned &unfit
,   unsigned &rounds
,   double &residual
,   double &gainMin
,   double &gainMax
,   const unsigned disparity_steps = 1
);

//! LF = LF x (float)(invert ? G : 1 / G) per non-empty SAI and stored channel, in place, on the GPU (lfbm5d_photo_apply_host_sai);
//! `gains` holds 3 doubles per SAI, as equalise_LF returns them.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int apply_gains_LF(
    std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   const std::vector<double> &gains
,   const bool invert
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
);

//! Per-view noise levels -- not in the reference: run_bm5d with one noise level per SAI (lfbm5d_denoise_views_host_sai,
//! include/lfbm5d_views.h).  sigma_sai: one value per SAI in the units of `sigma`, or empty: the per-SAI blind estimate of LF_noisy is
//! taken first; on return it holds the table that was applied (0 for empty SAIs).  Every angular window runs with the root mean square
//! of its views' levels (their common value where they agree).  window_sigmas receives the sigma of every window that ran, the first
//! step's windows, then the second's.  Everything else as run_bm5d.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int denoise_views_LF(
    std::vector<double> &sigma_sai
,   std::vector<float> &window_sigmas
,   const float lambdaHard5D
,   std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard
,   const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard
,   const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien
,   const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien
,   const unsigned color_space
,   const unsigned nb_threads
);

//! Spatially correlated noise -- not in the reference: run_bm5d under noise of autocorrelation acf (49 doubles: the lags -3..3 row-major,
//! 1 at lag 0; include/lfbm5d_corr.h; lfbm5d_denoise_corr_host_sai): every 2-D coefficient is thresholded and Wiener-shrunk with its own
//! variance factor, sigma stays the marginal level.  General group kernels only.  Everything else as run_bm5d.  Returns EXIT_SUCCESS, or
//! EXIT_FAILURE with the message on stdout.
int denoise_corr_LF(
    const std::vector<double> &acf
,   const float sigma
,   const float lambdaHard5D
,   std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned anWien
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned NHard, const unsigned nSimHard, const unsigned nDispHard, const unsigned kHard, const unsigned pHard
,   const bool useSDHard, const unsigned tau_2D_hard, unsigned tau_4D_hard, const unsigned tau_5D_hard
,   const unsigned NWien, const unsigned nSimWien, const unsigned nDispWien, const unsigned kWien, const unsigned pWien
,   const bool useSDWien, const unsigned tau_2D_wien, unsigned tau_4D_wien, const unsigned tau_5D_wien
,   const unsigned color_space
,   const unsigned nb_threads
);

//! The autocorrelation of the noise of LF at the lags -3..3 (acf: 49 doubles) from the block autocovariance of its flattest blocks
//! (lfbm5d_corr_measure_host_sai, include/lfbm5d_corr.h): block = 8, 16, 32 or 0 (16); fraction in (0, 1] or 0 (the default, 0.1); 1 on a
//! flat-field light field is the calibration.  sigma receives the marginal level of the selected blocks (biased low when fraction < 1).
int corr_measure_LF(
    const std::vector<std::vector<float> > &LF
,   const std::vector<unsigned> &LF_SAI_mask
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned block
,   const double fraction
,   std::vector<double> &acf
,   double &sigma
);

//! The view table equalisation leaves behind: sigma_v = sigma sqrt(mean_c g_{v,c}^-2) over the stored channels (lfbm5d_views_from_gains);
//! `gains` holds 3 doubles per SAI, as equalise_LF returns them.  Host only.  Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on
//! stdout.
int views_from_gains(
    const double sigma
,   const std::vector<double> &gains
,   const unsigned chnls
,   const std::vector<unsigned> &LF_SAI_mask
,   std::vector<double> &sigma_sai
);

//! run_bm3d_LF (run_bm3d_lf.h) with one noise level per SAI (lfbm5d_bm3d_lf_views_device): SAI v is filtered with sigma_sai[v] in both
//! steps.  sigma_sai as for denoise_views_LF.
int bm3d_views_LF(
    std::vector<double> &sigma_sai
,   std::vector<std::vector<float> > &LF_noisy
,   std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_basic
,   std::vector<std::vector<float> > &LF_denoised
,   const unsigned width, const unsigned height, const unsigned chnls
,   const unsigned nHard, const unsigned nWien, const unsigned kHard, const unsigned kWien
,   const unsigned NHard, const unsigned NWien, const unsigned pHard, const unsigned pWien
,   const bool useSD_h, const bool useSD_w, const unsigned tau_2D_hard, const unsigned tau_2D_wien
,   const float lambdaHard3D, const unsigned color_space
);

//! Super-resolution -- not in the reference's master branch: the scheme of SR-LFBM5D (iterative back-projection regularised by the
//! hard-thresholding step above) with the operators of include/lfbm5d.h, on the GPU (lfbm5d_superres_host_sai).  LF_low holds
//! width x height SAIs and is only read; LF_high is (re)sized to scale*width x scale*height SAIs and filled.  kernel: 0 = bicubic,
//! 1 = Gaussian of blurSigma; iterations, sigmaStart, sigmaEnd: 0 = the library's defaults for `scale` (lfbm5d_sr_defaults).
//! Returns EXIT_SUCCESS, or EXIT_FAILURE with the message on stdout.
int superres_LF(
    const std::vector<std::vector<float> > &LF_low
,   const std::vector<unsigned> &LF_SAI_mask
,   std::vector<std::vector<float> > &LF_high
,   const unsigned ang_major
,   const unsigned awidth
,   const unsigned aheight
,   const unsigned anHard
,   const unsigned width
,   const unsigned height
,   const unsigned chnls
,   const unsigned scale
,   const unsigned kernel
,   const float    blurSigma
,   const unsigned iterations
,   const float    sigmaStart
,   const float    sigmaEnd
,   const float    lambdaHard5D
,   const unsigned NHard
,   const unsigned nSim
,   const unsigned nDisp
,   const unsigned kHard
,   const unsigned pHard
,   const bool     useSD
,   const unsigned tau_2D
,         unsigned tau_4D
,   const unsigned tau_5D
,   const unsigned color_space
);

#endif
