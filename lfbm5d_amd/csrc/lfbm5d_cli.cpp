/*
 * lfbm5d_cli.cpp -- `LFBM5Ddenoising`, the reference's command line (src/main.cpp:60-309,
 * argument order of get_params, utilities_LF.cpp:1181-1309 / README.md:83) on the GPU backend:
 *
 *   LFBM5Ddenoising LFSourceDir|none SAIName sep awidth aheight sIdxStart tIdxStart aswSizeHard
 *       aswSizeWien row|col sigma lambda LFNoisyDir LFBasicDir LFDenoisedDir LFDiffDir
 *       NHard nSimHard nDispHard kHard pHard id|dct|bior id|dct|sadct hw|haar|dct useSDHard
 *       NWien nSimWien nDispWien kWien pWien id|dct|bior id|dct|sadct hw|haar|dct useSDWien
 *       rgb|yuv|ycbcr|opp nbThreads resultsFile
 *
 * Same files in and out (<dir>/<name><sep><ss><sep><tt>.png), same PSNR report format.
 * Differences, all opt-in through the environment so the argument list stays a drop-in:
 *   LFBM5D_SEED=<n>   seed MT19937 once with n and draw the noise SAI by SAI in st order
 *                     (reproducible); unset = time + pid seeding like the reference;
 *   LFBM5D_DEVICE=<i> HIP device index;
 *   LFBM5D_TILED=1    honour nbThreads > 1 the reference's way (tiles with a discarded halo, bm5d.cpp:411-708);
 *   LFBM5D_SIGMA=auto estimate sigma from the noisy light field (noise_level_LF, run_bm5d.h) once it exists -- loaded with
 *                     LFSourceDir = none, or made with the argument's sigma from a ground truth -- and use the estimate for both
 *                     steps and the diff images;
 *   LFBM5D_SIGMA=poisson | poisson:<a>,<b>   signal-dependent noise var(z | y) = a y + b (0..255 scale; a >= 0, 3/8 a^2 + b > 0): the
 *                     model is estimated from the noisy light field (pg_estimate_LF, run_bm5d.h), or given; both steps then run as one
 *                     job between the variance-stabilising transform and its exact unbiased inverse (denoise_pg_LF; LFBM3Ddenoising:
 *                     pg_forward_LF, run_bm3d_LF, pg_inverse_LF), with the sigma the transform leaves (also used for the diff images).
 *                     With a ground truth and poisson:<a>,<b> the noise added is Poisson-Gaussian with those parameters (<random>,
 *                     seeded from LFBM5D_SEED; the argument's sigma is unused); any other value is an error;
 *   LFBM5D_SIGMA=poisson-clipped | poisson-clipped:<a>,<b>   that noise on data rounded and clipped to the range of
 *                     LFBM5D_CLIP_RANGE=<lo>,<hi> (default 0,255: 8-bit files), sigma^2(y) = a (y - lo) + b: the model is fitted over the
 *                     intensity levels the clipping left alone (pgclip_estimate_LF, run_bm5d.h; include/lfbm5d_pgclip.h), or given; both
 *                     steps run as one job between the clipped model's stabiliser and its exact unbiased inverse, which also undoes
 *                     the clipping bias (denoise_pgclip_LF; LFBM3Ddenoising: pgclip_forward_LF, run_bm3d_LF, pgclip_inverse_LF).  With a
 *                     ground truth and a given model that Poisson-Gaussian noise is added (LFBM5D_SEED), then rounded and clipped to the
 *                     range.  A model outside the accepted domain (a^2 <= 0.5 b, a <= 5) is refused: poisson is the mode for it.
 *                     Towards the other variables it behaves as poisson does (LFBM5D_CLIP and LFBM5D_EQUALISE are refused);
 *   LFBM5D_IMPULSE=auto | <k>   impulse repair (impulse_repair_LF, run_bm5d.h) of the noisy light field once it exists, loaded or
 *                     synthesised, before LFBM5D_SIGMA=auto / poisson look at it and before the filter: hot and dead pixels, salt and
 *                     pepper and values that are not finite are replaced by the lower median of their sound neighbours; auto = the
 *                     default threshold factor k = 8, <k> = that factor (finite, >= 0); prints `Impulse repair: <n> of <N> values flagged
 *                     (<pct> %), <m> left; thresholds <T0> <T1> <T2>`.  With a ground truth LFBM5D_IMPULSE_ADD=<p> (0 <= p <= 1) first
 *                     replaces that fraction of the synthesised noisy values by 0 or 255 (<random>, seeded from LFBM5D_SEED); the noisy
 *                     files are saved before the repair.  Any other value of either is an error; unset, the output is unchanged;
 *   LFBM5D_DEFECTS=<dir>   defect inpainting (inpaint_LF, run_bm5d.h) of the noisy light field once it exists: <dir> holds 8-bit PNGs
 *                     named like the SAIs, non-zero = defective (a grey file applies to every channel; a missing file = no defects in
 *                     that SAI).  Order: the fill; LFBM5D_IMPULSE if set; the sigma estimate of LFBM5D_SIGMA=auto; the refinement loop
 *                     with this command's hard-thresholding parameters and sigma_noise = sigma; the job.  LFBM5D_DEFECTS_ITER=<K>
 *                     replaces the library's number of refinement steps (0 = the fill alone).  With LFBM5D_SIGMA=poisson, and in
 *                     LFBM3Ddenoising (which has no 5-D parameters), only the fill runs, and the command says so.  Prints `Defect
 *                     inpainting: <n> of <N> values flagged (<pct> %), <m> left; <passes> fill passes, <K> refinement steps`.  The
 *                     noisy files are saved before the fill.  Unset, the output is unchanged;
 *   LFBM5D_MISSING=<s>_<t>[,<s>_<t>...]   view synthesis (view_synth_LF, run_bm5d.h): the SAIs named, in the indices the file names carry,
 *                     are reconstructed from their sound angular neighbours.  With LFSourceDir = none their files need not exist and
 *                     are not read; with a ground truth they are dropped (zeroed) from the noisy light field once it is made, before
 *                     it is saved.  Order: the synthesis; LFBM5D_IMPULSE if set; the sigma estimate of LFBM5D_SIGMA=auto, on a mask with
 *                     the missing SAIs marked empty (a mean of n sources carries less noise than a real SAI); the synthesis again (the
 *                     sources may have been repaired) and the refinement loop with this command's hard-thresholding parameters and
 *                     sigma_noise = sigma; the job.  LFBM5D_MISSING_ITER=<K> replaces the library's number of refinement steps.  With
 *                     LFBM5D_SIGMA=poisson, and in LFBM3Ddenoising (which has no 5-D parameters), only the synthesis runs, and the
 *                     command says so.  Prints `View synthesis: <n> of <A> SAIs missing, <m> left; disparities <dmin>..<dmax>, <K>
 *                     refinement steps`.  Combining it with LFBM5D_DEFECTS is an error.  Unset, the output is unchanged;
 *   LFBM5D_DETECT=auto | <k>   consistency check (consist_LF, run_bm5d.h) of the noisy light field once it exists, loaded or synthesised,
 *                     ahead of LFBM5D_IMPULSE and LFBM5D_SIGMA: every SAI is predicted from its angular neighbours; values that the other
 *                     views contradict and SAIs whose residual stands out are found (auto = the library's threshold factor, <k> = that
 *                     factor, finite, >= 0).  Prints `Consistency check: <b> of <A> SAIs bad [<s>_<t> ...], <n> of <N> values flagged
 *                     (<pct> %), <u> SAIs untested; scales <s0> <s1> <s2>; <rounds> sweeps`.  The bad SAIs then go through the view
 *                     synthesis exactly as if LFBM5D_MISSING named them (their files were read, their values are not used), the
 *                     flagged values through the defect inpainting exactly as if LFBM5D_DEFECTS gave the map: the synthesis first, the
 *                     fill second, each with its own loop (LFBM5D_MISSING_ITER, LFBM5D_DEFECTS_ITER) and report line.
 *                     LFBM5D_DETECT_SAVE=<dir> writes the maps as PNGs in LFBM5D_DEFECTS' format and the bad SAIs as one line in
 *                     LFBM5D_MISSING's format into <dir>/missing.txt (empty when none is bad), so that a camera's fixed map can be
 *                     reused.  Together with LFBM5D_DEFECTS or LFBM5D_MISSING it is an error (there is no combined loop).  The files
 *                     hold 8-bit values, so nothing here is non-finite.  Unset, the output is unchanged;
 *   LFBM5D_REPAIR=joint   joint repair (repair_LF, run_bm5d.h; include/lfbm5d_repair.h): what LFBM5D_DEFECTS, LFBM5D_MISSING -- together
 *                     or alone under this variable -- or LFBM5D_DETECT name goes to one job in place of the two stages: a plane sweep that
 *                     skips unsound source values fills flagged values and missing SAIs from the other views, the rim fill takes the
 *                     rest, one loop refines both with this command's hard-thresholding parameters and sigma_noise = sigma.
 *                     LFBM5D_REPAIR_ITER=<K> replaces the library's number of refinement steps (LFBM5D_DEFECTS_ITER and
 *                     LFBM5D_MISSING_ITER are not looked at).  It prints `Joint repair: <n> of <N> values flagged (<pct> %), <b> of <A> SAIs
 *                     missing; <v> values from other views, <r> from the rim, <l> left; disparities <dmin>..<dmax>, <K> refinement
 *                     steps`.  Errors that stop the command before it reads a file: any other value, LFBM5D_REPAIR_ITER alone, none of
 *                     the three variables above, LFBM5D_DISPARITY_STEPS other than 1, LFBM5D_OCCLUSION, LFBM5D_SIGMA=poisson*,
 *                     LFBM5D_VIEW_SIGMA.  Unset, every command behaves as before, its rejections included;
 *   LFBM5D_OCCLUSION=auto|<ratio>   the occlusion-aware plane sweep (include/lfbm5d_occl.h) in every view synthesis the command runs
 *                     (LFBM5D_MISSING, and the bad SAIs LFBM5D_DETECT hands over): `auto` is the library's ratio, <ratio> a finite
 *                     number >= 1.  The `View synthesis:` line then ends `, occlusion ratio <ratio>: <pct> % of the positions from a
 *                     half-plane`.  Any other value, and the variable without LFBM5D_MISSING or LFBM5D_DETECT, stop the command
 *                     with a message before a file is read.  Unset: the plain sweep, the output as without this variable.
 *   LFBM5D_DISPARITY_STEPS=1|2|4   hypotheses per pixel of disparity in the plane sweeps of LFBM5D_MISSING and LFBM5D_DETECT (sources are
 *                     interpolated bilinearly above 1; for light fields that move a fraction of a pixel per view).  Above 1 the
 *                     `View synthesis:` line prints the disparity range as decimals and ends `, <Q> steps per pixel`, and the
 *                     `Consistency check:` line ends the same.  Any other value, and the variable without LFBM5D_MISSING or
 *                     LFBM5D_DETECT, is an error.  Unset or 1, the output is unchanged;
 *   LFBM5D_CLIP=auto | <lo>,<hi>   the noisy light field was clipped to lo..hi (auto: 0..255, what an 8-bit file does to it).  With
 *                     LFBM5D_SIGMA=auto the clipping-aware estimate (noise_level_clipped_LF, run_bm5d.h) replaces the blind one; the
 *                     line reads `Estimated noise level: sigma = <v> (clipping-aware: <L> levels, censored blocks <= <pct> %)`.
 *                     Otherwise the argument's sigma is used.  Both steps run as one job (denoise_clipped_LF; LFBM3Ddenoising:
 *                     run_bm3d_LF, declip_LF) and the basic and the denoised light field are taken through the inverse of the clipped
 *                     mean before PSNR, SSIM and saving: `Declipping: range <lo>..<hi>, sigma = <s>`.  It runs after LFBM5D_DETECT /
 *                     MISSING / DEFECTS / IMPULSE, which stay as they are.  With LFBM5D_SIGMA=poisson it is an error, and so is any
 *                     other value.  With a ground truth LFBM5D_CLIP_ADD=1 first rounds the synthesised noisy light field to whole
 *                     numbers and clips it to the range (0..255 without LFBM5D_CLIP: the filter then runs on clipped data as it
 *                     would on a file's), before LFBM5D_IMPULSE_ADD.  Unset, the output is unchanged;
 *   LFBM5D_EQUALISE=auto | flat   photometric equalisation (equalise_LF, run_bm5d.h; include/lfbm5d_photo.h) of the noisy light field once
 *                     it exists, ahead of LFBM5D_DETECT and every later stage: one gain per SAI and stored channel is estimated from
 *                     what the neighbouring views predict and divided out, so that vignetted or differently exposed views meet the
 *                     filter's brightness-constancy assumption.  Prints `Photometric equalisation: <f> of <A> SAIs fitted, <u> untested,
 *                     <n> unfit; gains <min>..<max>; <rounds> sweeps, residual <r>`.  `auto` multiplies the gains back into the basic
 *                     and the denoised light field before PSNR, SSIM and saving (the files keep every view's own photometry); `flat`
 *                     leaves them equalised.  LFBM5D_DISPARITY_STEPS applies to its sweep.  With LFBM5D_SIGMA=poisson or LFBM5D_CLIP
 *                     it is an error (a gain changes the noise model and the clipping range), and so is any other value.  With a
 *                     ground truth LFBM5D_EQUALISE_ADD=<edge> (0 < edge <= 1) first multiplies the synthesised noisy views by a smooth
 *                     vignette, 1 at the centre view and <edge> at the corner views.  Unset, the output is unchanged;
 *   LFBM5D_VIEW_SIGMA=auto | gains   one noise level per SAI (denoise_views_LF, run_bm5d.h; include/lfbm5d_views.h): every angular window
 *                     is filtered with the root mean square of its views' levels, both steps as one job (LFBM3Ddenoising: every SAI with
 *                     its own level, bm3d_views_LF).  `auto` takes the per-view blind estimate of the noisy light field where
 *                     LFBM5D_SIGMA=auto takes the pooled one, after equalisation and impulse repair; the argument's sigma, or the
 *                     pooled estimate, is only printed.  `gains` needs LFBM5D_EQUALISE and a numeric sigma (with LFBM5D_SIGMA=auto it is
 *                     an error: use `auto`): sigma_v = sigma sqrt(mean over the channels of g^-2) for the gains that were divided out.
 *                     Prints `Per-view noise levels: <n> SAIs, sigma <min>..<max> (pooled <rms>), from <estimate|gains>; window sigmas
 *                     <min>..<max>`.  With LFBM5D_SIGMA=poisson*, LFBM5D_CLIP, LFBM5D_MISSING, LFBM5D_DEFECTS or LFBM5D_DETECT (their
 *                     models and refinement steps assume one sigma) it is an error, and so is any other value.  With a ground truth
 *                     LFBM5D_VIEW_SIGMA_ADD=<edge> (0 < edge <= 1) synthesises noise of sigma / g_v on view v in place of uniform
 *                     noise, g the vignette of LFBM5D_EQUALISE_ADD: what a devignetted capture carries.  Unset, the output is unchanged;
 *   LFBM5D_NOISE_CORR=auto | <file> | kernel:<file>   spatially correlated noise (denoise_corr_LF, run_bm5d.h; include/lfbm5d_corr.h): every
 *                     2-D coefficient is thresholded and Wiener-shrunk with its own variance factor under the noise's autocorrelation,
 *                     both steps as one job on the general group kernels (slower than the dedicated ones).  `auto` measures the
 *                     autocorrelation on the flattest blocks of the noisy light field (corr_measure_LF); <file> holds it as 49 numbers
 *                     (lags -3..3 row-major, 1 at lag 0); kernel:<file> holds the taps of the filter the noise went through, one row
 *                     per line, up to 7 x 7.  The command's sigma stays the marginal level.  Prints `Noise correlation: lag-1 <h> <v>,
 *                     variance factors <min>..<max> (step 1), <min>..<max> (step 2), <n> clamped; from <estimate|file|kernel>`.
 *                     Together with LFBM5D_SIGMA=auto|poisson*, LFBM5D_CLIP, LFBM5D_VIEW_SIGMA, LFBM5D_REPAIR, LFBM5D_DEFECTS,
 *                     LFBM5D_MISSING, LFBM5D_DETECT or LFBM5D_EQUALISE it is an error, and LFBM3Ddenoising refuses it (the per-SAI BM3D
 *                     flavour is not covered).  With a ground truth LFBM5D_NOISE_CORR_ADD=<file> (taps as for kernel:) filters the
 *                     synthesised noise by those taps, normalised to unit energy and periodic at the image border, so that its
 *                     marginal level stays sigma.  Unset, the output is unchanged;
 *   LFBM5D_REPORT_SSIM=1  the average SSIM next to every average PSNR on stdout and an SSIM block behind every PSNR block of the
 *                     results file, computed on the GPU on the images as the files hold them (cli_quality.h); any other value is an
 *                     error; unset, the output is unchanged.
 * Without LFBM5D_TILED nbThreads is parsed and ignored: the GPU path has the reference's untiled
 * (nb_threads == 1) semantics, half a dB better than its tiled mode.
 *
 * Compiled with -DLFBM3D_CLI the same file is `LFBM3Ddenoising` (src/main_bm3d_LF.cpp:56-272, arguments of
 * get_params_BM3D, utilities_LF.cpp:1342-1468 / README.md:85), BM3D on every SAI independently:
 *
 *   LFBM3Ddenoising LFSourceDir|none SAIName sep awidth aheight sIdxStart tIdxStart aswSizeHard aswSizeWien row|col
 *       sigma lambda LFNoisyDir LFBasicDir LFDenoisedDir LFDiffDir NHard nHard kHard pHard dct|bior useSDHard
 *       NWien nWien kWien pWien dct|bior useSDWien rgb|yuv|ycbcr|opp nbThreads resultsFile
 */
#include <sys/time.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>
#include <thread>
#include <atomic>
#include <mutex>

#include "../../include/lfbm5d.h"
#include "png_min.h"
#include "run_bm5d.h"
#include "run_bm3d_lf.h"
#include "cli_quality.h"

using namespace std;

namespace {

double now_s() { timeval tp; gettimeofday(&tp, nullptr); return tp.tv_sec + tp.tv_usec * 1e-6; }

/* the program-level variables of the header comment, read where they are used */
const char* env(const char* name) { return getenv(name); }

/* mt19937ar genrand_res53 on std::mt19937 (identical generator and seeding recurrence) */
struct Mt {
    std::mt19937 g;
    explicit Mt(unsigned long s) : g((uint32_t)s) {}
    double res53() { const unsigned long a = g() >> 5, b = g() >> 6; return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0); }
};

/* The SAIs are files of their own: decoded / encoded by a few threads (PNG inflate / deflate is the command's wall time once the
 * filter runs on a GPU: 18 ms per 512 x 512 colour image and thread).  LFBM5D_IO_THREADS (default: the machine's cores, at most
 * 16; 1: one after the other like the reference).  fn(i) -> false stops the loop and fails it. */
template <class F> bool parallel_sais(unsigned n, F fn) {
    const char* e = env("LFBM5D_IO_THREADS");
    unsigned nt = e && *e ? (unsigned)std::max(1, atoi(e)) : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    nt = std::min(nt, std::max(1u, n));
    std::atomic<unsigned> next(0);
    std::atomic<bool> ok(true);
    auto work = [&]() { for (unsigned i = next++; i < n && ok; i = next++) if (!fn(i)) ok = false; };
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nt; i++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    return ok;
}

string sai_path(const char* dir, const char* name, const char* sep, unsigned s, unsigned t) {
    ostringstream o;
    o << dir << "/" << name << sep << setfill('0') << setw(2) << s << sep << setfill('0') << setw(2) << t << ".png";
    return o.str();
}

/* load_LF, utilities_LF.cpp:72-167 */
int load_LF(const char* dir, const char* name, const char* sep, vector<vector<float> >& LF, vector<unsigned>& mask,
            unsigned ang_major, unsigned aw, unsigned ah, unsigned s0, unsigned t0, unsigned& W, unsigned& H, unsigned& C,
            const vector<unsigned>* skip = nullptr) {   /* skip (LFBM5D_MISSING): SAIs whose files are not read; zeros, marked non-empty */
    mask.assign(aw * ah, 0u);
    LF.assign(aw * ah, vector<float>());
    cout << endl;
    std::vector<size_t> ws(aw * ah, 0), hs(aw * ah, 0), cs(aw * ah, 0);
    std::mutex out;
    string bad;
    const bool ok = parallel_sais(aw * ah, [&](unsigned i) {
        const unsigned s = i / aw, t = i % aw;
        if (skip && (*skip)[ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah]) return true;
        const string p = sai_path(dir, name, sep, s + s0, t + t0);
        { std::lock_guard<std::mutex> g(out); cout << "\rRead input image " << p << flush; }
        vector<float> img;
        size_t w, h, c;
        if (!png_read_planar_f32(p, img, w, h, c)) { std::lock_guard<std::mutex> g(out); if (bad.empty()) bad = p; return false; }
        if (c == 2) c = 1; /* drop alpha */
        if (c > 2) {       /* really colour? (utilities_LF.cpp:118-125) */
            size_t k = 0; float acc = 0.0f;
            while (k < w * h && img[k] == img[w * h + k] && img[k] == img[2 * w * h + k]) { acc += img[k] + img[w * h + k] + img[2 * w * h + k]; k++; }
            c = (k == w * h && acc > 0.0f) ? 1 : 3;
        }
        const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
        ws[st] = w; hs[st] = h; cs[st] = c;
        LF[st].assign(img.begin(), img.begin() + w * h * c);
        for (float v : LF[st]) if (v) { mask[st] = 1; break; }
        return true;
    });
    if (!ok) { cout << endl << "error :: " << bad << " not found or not a correct png image." << endl; return EXIT_FAILURE; }
    {   /* all SAIs of the first one's size (the first in the reference's reading order: s, t = 0, 0) */
        unsigned st0 = 0;
        if (skip) {   /* the first SAI in reading order that has a file */
            unsigned i = 0;
            for (; i < aw * ah; i++) {
                const unsigned s = i / aw, t = i % aw;
                st0 = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
                if (!(*skip)[st0]) break;
            }
            if (i == aw * ah) { cout << endl << "error :: every SAI is missing" << endl; return EXIT_FAILURE; }
        }
        W = (unsigned)ws[st0]; H = (unsigned)hs[st0]; C = (unsigned)cs[st0];
        for (unsigned st = 0; st < aw * ah; st++) {
            if (skip && (*skip)[st]) { LF[st].assign((size_t)W * H * C, 0.0f); mask[st] = 1; continue; }
            if (ws[st] != W || hs[st] != H || cs[st] != C) { cout << endl << "error :: SAIs of different sizes" << endl; return EXIT_FAILURE; }
        }
    }
    cout << endl << " Light field size :" << endl << " - awidth         = " << aw << endl << " - aheight        = " << ah << endl
         << " - width          = " << W << endl << " - height         = " << H << endl << " - nb of channels = " << C << endl;
    return EXIT_SUCCESS;
}

/* save_LF + save_image, utilities_LF.cpp:182-231, utilities.cpp:118-142 */
int save_LF(const char* dir, const char* name, const char* sep, const vector<vector<float> >& LF, unsigned ang_major,
            unsigned aw, unsigned ah, unsigned s0, unsigned t0, unsigned W, unsigned H, unsigned C) {
    std::mutex out;
    string bad;
    const bool ok = parallel_sais(aw * ah, [&](unsigned i) {
        const unsigned s = i / aw, t = i % aw;
        const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
        const string p = sai_path(dir, name, sep, s + s0, t + t0);
        { std::lock_guard<std::mutex> g(out); cout << "\rWrite image " << p << flush; }
        vector<float> tmp((size_t)W * H * C, 0.0f);
        if (LF[st].size() == tmp.size())
            for (size_t k = 0; k < tmp.size(); k++) tmp[k] = LF[st][k] > 255.0f ? 255.0f : (LF[st][k] < 0.0f ? 0.0f : LF[st][k]);
        if (!png_write_planar_f32(p, tmp.data(), W, H, C)) { std::lock_guard<std::mutex> g(out); if (bad.empty()) bad = p; return false; }
        return true;
    });
    if (!ok) { cout << "... failed to save png image " << bad << endl; return EXIT_FAILURE; }
    cout << endl;
    return EXIT_SUCCESS;
}

/* compute_psnr(_LF), utilities.cpp:412-435, utilities_LF.cpp:639-692 */
void psnr_LF(const vector<vector<float> >& A, const vector<vector<float> >& B, const vector<unsigned>& mask, vector<float>& psnr,
             float& avg_p, float& std_p, vector<float>& rmse, float& avg_r, float& std_r) {
    const size_t n = mask.size();
    psnr.assign(n, 0.0f); rmse.assign(n, 0.0f);
    float cnt = 0, sp = 0, sr = 0;
    for (size_t st = 0; st < n; st++) {
        if (!mask[st]) continue;
        float tmp = 0.0f;
        for (size_t k = 0; k < A[st].size(); k++) tmp += (A[st][k] - B[st][k]) * (A[st][k] - B[st][k]);
        rmse[st] = sqrtf(tmp / (float)A[st].size());
        psnr[st] = 20.0f * log10f(255.0f / rmse[st]);
        cnt++; sp += psnr[st]; sr += rmse[st];
    }
    avg_p = sp / cnt; avg_r = sr / cnt;
    float vp = 0, vr = 0;
    for (size_t st = 0; st < n; st++) if (mask[st]) { vp += (psnr[st] - avg_p) * (psnr[st] - avg_p); vr += (rmse[st] - avg_r) * (rmse[st] - avg_r); }
    std_p = sqrtf(vp / cnt); std_r = sqrtf(vr / cnt);
}

/* write_psnr_LF, utilities_LF.cpp:782-869 */
void write_psnr(const char* file, const char* what, const vector<unsigned>& mask, unsigned ang_major, unsigned aw, unsigned ah,
                const vector<float>& psnr, float avg_p, float std_p, const vector<float>& rmse, float avg_r, float std_r) {
    ofstream f(file, ios::out | ios::app);
    if (!f) { cout << "Can't open " << file << endl; return; }
    f << endl << "******************************************" << endl;
    f << "-> Average PSNR " << what << " = " << avg_p << endl << "-> Standard deviation PSNR " << what << " = " << std_p << endl;
    f << "PSNR for all " << what << " SAIs:" << endl;
    for (unsigned s = 0; s < ah; s++) { for (unsigned t = 0; t < aw; t++) { const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah; if (mask[st]) f << psnr[st] << " "; else f << "No SAI "; } f << endl; }
    f << endl << "-> Average RMSE " << what << " = " << avg_r << endl << "-> Standard deviation RMSE " << what << " = " << std_r << endl;
    f << "RMSE for all " << what << " SAIs:" << endl;
    for (unsigned s = 0; s < ah; s++) { for (unsigned t = 0; t < aw; t++) { const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah; f << rmse[st] << " "; } f << endl; }
    f << "******************************************" << endl;
}

/* compute_diff, utilities.cpp:440-468 */
void diff_LF(const vector<vector<float> >& A, const vector<vector<float> >& B, const vector<unsigned>& mask, vector<vector<float> >& D, float sigma) {
    const float s = 4.0f * sigma;
    for (size_t st = 0; st < mask.size(); st++) {
        if (!mask[st]) continue;
        D[st].resize(A[st].size());
        for (size_t k = 0; k < A[st].size(); k++) {
            const float v = s > 0.0 ? (A[st][k] - B[st][k] + s) * 255.0f / (2.0f * s) : fabsf(A[st][k] - B[st][k]);
            D[st][k] = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        }
    }
}

/* add_noise_LF, utilities_LF.cpp:244-263 + add_noise, utilities.cpp:154-185.  The reference seeds a generator per SAI from the clock
 * and the process id: the SAIs' streams are independent and are drawn by the I/O thread pool (the SAI's index added to the seed:
 * threads that start within one millisecond must not share one).  LFBM5D_SEED (tests, benchmarks) is ONE stream through the SAIs
 * in order: its uniforms are drawn in order, SAI by SAI, and only their Box-Muller transform is spread over the threads. */
void add_noise_LF(const vector<vector<float> >& LF, const vector<unsigned>& mask, vector<vector<float> >& LF_noisy, float sigma,
                  const double* pg = nullptr, const vector<double>* view_sigma = nullptr) {
    const char* seed = env("LFBM5D_SEED");
    if (pg) {   /* Poisson-Gaussian noise {a, b}: a * Poisson(y / a) + N(0, b), one <random> stream through the SAIs in order */
        timeval tp; gettimeofday(&tp, nullptr);
        std::mt19937_64 g(seed ? strtoull(seed, nullptr, 10) : (unsigned long long)(tp.tv_sec * 1000 + tp.tv_usec / 1000 + getpid()));
        const double a = pg[0], sd = sqrt(std::max(pg[1], 0.0));
        std::normal_distribution<double> gauss(0.0, 1.0);
        for (size_t st = 0; st < LF.size(); st++) {
            if (!mask[st]) continue;
            for (size_t q = 0; q < LF[st].size(); q++) {
                const double y = LF[st][q];
                double z = y;
                if (a > 0.0) z = y > 0.0 ? a * (double)std::poisson_distribution<long long>(y / a)(g) : 0.0;
                if (sd > 0.0) z += sd * gauss(g);
                LF_noisy[st][q] = (float)z;
            }
        }
        return;
    }
    /* (LFBM5D_VIEW_SIGMA_ADD: SAI st draws with its own sigma) */
    auto gauss = [sigma, view_sigma](size_t st, double x, double y) {
        return (float)((view_sigma ? (*view_sigma)[st] : (double)sigma) * sqrt(-2.0 * log(x)) * cos(2.0 * M_PI * y));
    };
    if (!seed) {
        parallel_sais((unsigned)LF.size(), [&](unsigned st) {
            if (!mask[st]) return true;
            timeval tp; gettimeofday(&tp, nullptr);
            Mt g(tp.tv_sec * 1000 + tp.tv_usec / 1000 + (unsigned long)getpid() + st);
            for (size_t q = 0; q < LF[st].size(); q++) {
                const double x = g.res53(), y = g.res53();
                LF_noisy[st][q] = LF[st][q] + gauss(st, x, y);
            }
            return true;
        });
        return;
    }
    Mt g(strtoul(seed, nullptr, 10));
    vector<double> u;
    for (size_t st = 0; st < LF.size(); st++) {
        if (!mask[st]) continue;
        const size_t n = LF[st].size();
        u.resize(2 * n);
        for (size_t q = 0; q < 2 * n; q++) u[q] = g.res53();
        const unsigned parts = 16;
        parallel_sais(parts, [&](unsigned part) {
            for (size_t q = n * part / parts; q < n * (part + 1) / parts; q++) LF_noisy[st][q] = LF[st][q] + gauss(st, u[2 * q], u[2 * q + 1]);
            return true;
        });
    }
}

/* LFBM5D_SIGMA: unset -> 0 (the argument's sigma), "auto" -> 1 (estimate it), "poisson" -> 2 (Poisson-Gaussian model, estimated),
 * "poisson:<a>,<b>" -> 3 (that model: pg = {a, b}), "poisson-clipped" -> 4 (the clipped Poisson-Gaussian model, estimated),
 * "poisson-clipped:<a>,<b>" -> 5 (that model; a >= 0, b >= 0, a + b > 0: the library checks the accepted domain), anything else -> -1
 * (error, message printed) */
int sigma_mode(double* pg) {
    const char* e = env("LFBM5D_SIGMA");
    if (!e) return 0;
    if (!strcmp(e, "auto")) return 1;
    if (!strcmp(e, "poisson")) return 2;
    if (!strcmp(e, "poisson-clipped")) return 4;
    const bool clipped = !strncmp(e, "poisson-clipped:", 16);
    if (clipped || !strncmp(e, "poisson:", 8)) {
        const char* p = e + (clipped ? 16 : 8);
        char *q = nullptr, *r = nullptr;
        const double a = strtod(p, &q);
        if (q != p && !(clipped && isspace((unsigned char)*p)) && *q == ',' && q[1] && !isspace((unsigned char)q[1])) {
            const double b = strtod(q + 1, &r);
            const bool ok = r != q + 1 && !*r && std::isfinite(a) && std::isfinite(b) && a >= 0.0;
            if (ok && (clipped ? b >= 0.0 && a + b > 0.0 : 0.375 * a * a + b > 0.0)) { pg[0] = a; pg[1] = b; return clipped ? 5 : 3; }
        }
    }
    cout << "LFBM5D_SIGMA must be \"auto\" (estimate sigma from the noisy light field), \"poisson\" (estimate a Poisson-Gaussian noise model "
            "var = a y + b), \"poisson:<a>,<b>\" (that model; a >= 0, 3/8 a^2 + b > 0), \"poisson-clipped\" (estimate that model on data "
            "rounded and clipped to the range of LFBM5D_CLIP_RANGE) or \"poisson-clipped:<a>,<b>\" (that model; a >= 0, b >= 0, a + b > 0), "
            "or unset; got \"" << e << "\"" << endl;
    return -1;
}

/* LFBM5D_CLIP_RANGE: the range of LFBM5D_SIGMA=poisson-clipped, 0..255 when unset; false (message printed) on a malformed value */
bool clip_range_mode(double& lo, double& hi) {
    lo = 0.0; hi = 255.0;
    const char* e = env("LFBM5D_CLIP_RANGE");
    if (!e) return true;
    char* q = nullptr; char* r = nullptr;
    lo = strtod(e, &q);
    bool ok = q != e && *q == ',' && !isspace((unsigned char)*e) && q[1] && !isspace((unsigned char)q[1]);
    if (ok) { hi = strtod(q + 1, &r); ok = r != q + 1 && !*r; }
    if (ok && std::isfinite(lo) && std::isfinite(hi) && lo < hi) return true;
    cout << "LFBM5D_CLIP_RANGE must be the range \"<lo>,<hi>\" with lo < hi that LFBM5D_SIGMA=poisson-clipped assumes the noisy light field was "
            "rounded and clipped to, or unset (0,255); got \"" << e << "\"" << endl;
    return false;
}

/* LFBM5D_SIGMA=poisson-clipped: the line that reports the model and the sigma the filter ran with */
void print_pgclip_model(bool estimated, const double* pg, double lo, double hi, unsigned levels, double f_max, float s) {
    cout << endl << (estimated ? "Estimated" : "Given") << " clipped noise model: a = " << setprecision(8) << pg[0] << ", b = " << pg[1]
         << ", range " << lo << ".." << hi << " (";
    if (estimated) cout << levels << " levels, censored blocks <= " << 100.0 * f_max << " %; ";
    cout << "sigma after stabilisation = " << s << ")" << setprecision(6) << endl;
}

/* LFBM5D_IMPULSE / LFBM5D_IMPULSE_ADD: k < 0 = no repair, add = 0 = no impulses added; false (message printed) on anything else */
bool impulse_mode(double& k, double& add) {
    k = -1.0; add = 0.0;
    if (const char* e = env("LFBM5D_IMPULSE")) {
        char* q = nullptr;
        const double v = strcmp(e, "auto") ? strtod(e, &q) : 8.0;
        if (strcmp(e, "auto") && (q == e || *q || isspace((unsigned char)*e) || !std::isfinite(v) || v < 0.0)) {
            cout << "LFBM5D_IMPULSE must be \"auto\" (impulse repair with the default threshold factor k = 8) or a factor k >= 0, or unset; got \""
                 << e << "\"" << endl;
            return false;
        }
        k = v;
    }
    if (const char* e = env("LFBM5D_IMPULSE_ADD")) {
        char* q = nullptr;
        const double v = strtod(e, &q);
        if (q == e || *q || isspace((unsigned char)*e) || !(v >= 0.0 && v <= 1.0)) {
            cout << "LFBM5D_IMPULSE_ADD must be a fraction 0 <= p <= 1 of the values to replace by 0 or 255, or unset; got \"" << e << "\"" << endl;
            return false;
        }
        add = v;
    }
    return true;
}

/* LFBM5D_CLIP / LFBM5D_CLIP_ADD: on = false when unset (lo..hi = 0..255, for LFBM5D_CLIP_ADD alone); false (message printed) on a
 * malformed value or together with LFBM5D_SIGMA=poisson (smode >= 2) */
bool clip_mode(bool& on, double& lo, double& hi, bool& add, int smode) {
    on = add = false; lo = 0.0; hi = 255.0;
    if (const char* e = env("LFBM5D_CLIP")) {
        if (strcmp(e, "auto")) {
            char* q = nullptr; char* r = nullptr;
            lo = strtod(e, &q);
            bool ok = q != e && *q == ',' && !isspace((unsigned char)*e) && !isspace((unsigned char)q[1]);
            if (ok) { hi = strtod(q + 1, &r); ok = r != q + 1 && !*r; }
            if (!ok || !std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) {
                cout << "LFBM5D_CLIP must be \"auto\" (the noisy light field was clipped to 0..255) or a range \"<lo>,<hi>\" with lo < hi, or unset; got \""
                     << e << "\"" << endl;
                return false;
            }
        }
        if (smode >= 2) {
            cout << "LFBM5D_CLIP cannot be combined with LFBM5D_SIGMA=poisson (Poisson-Gaussian noise combined with clipping is not covered)" << endl;
            return false;
        }
        on = true;
    }
    if (const char* e = env("LFBM5D_CLIP_ADD")) {
        if (strcmp(e, "1")) { cout << "LFBM5D_CLIP_ADD must be \"1\" (round and clip the synthesised noisy light field to the range of LFBM5D_CLIP, 0..255 without it) or unset; got \"" << e << "\"" << endl; return false; }
        add = true;
    }
    return true;
}

/* LFBM5D_CLIP_ADD: what storing the synthesised noisy light field in an integer format of range lo..hi does to it */
void clip_round_LF(vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, double lo, double hi) {
    unsigned long long hit = 0, all = 0;
    for (size_t st = 0; st < LF_noisy.size(); st++) {
        if (!mask[st]) continue;
        for (float& v : LF_noisy[st]) {
            const float r = std::nearbyint(v);
            all++;
            hit += r <= (float)lo || r >= (float)hi;
            v = std::min(std::max(r, (float)lo), (float)hi);
        }
    }
    cout << "Round and clip [range " << lo << ".." << hi << "]: " << hit << " of " << all << " values at the bounds" << endl;
}

/* LFBM5D_CLIP with LFBM5D_SIGMA=auto: replace `sigma` with the clipping-aware estimate on the noisy light field */
bool estimate_sigma_clipped_LF(const vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, unsigned W, unsigned H, unsigned C, double lo,
                               double hi, float& sigma) {
    float est = 0.0f; unsigned levels = 0; double f_max = 0.0;
    if (noise_level_clipped_LF(LF_noisy, mask, W, H, C, lo, hi, est, levels, f_max) != EXIT_SUCCESS) return false;
    cout << endl << "Estimated noise level: sigma = " << setprecision(8) << est << setprecision(6) << " (clipping-aware: " << levels
         << " levels, censored blocks <= " << 100.0 * f_max << " %)" << endl;
    sigma = est;
    return true;
}

void print_declipping(double lo, double hi, float sigma) {
    cout << endl << "Declipping: range " << lo << ".." << hi << ", sigma = " << setprecision(8) << sigma << setprecision(6) << endl;
}

/* LFBM5D_IMPULSE_ADD: salt and pepper on the synthesised noisy light field, one <random> stream through the SAIs in order */
void add_impulses_LF(vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, double p) {
    const char* seed = env("LFBM5D_SEED");
    timeval tp; gettimeofday(&tp, nullptr);
    std::mt19937_64 g(seed ? strtoull(seed, nullptr, 10) + 0x9e3779b97f4a7c15ull : (unsigned long long)(tp.tv_sec * 1000 + tp.tv_usec / 1000 + getpid()));
    std::uniform_real_distribution<double> u(0.0, 1.0);
    unsigned long long hit = 0, all = 0;
    for (size_t st = 0; st < LF_noisy.size(); st++) {
        if (!mask[st]) continue;
        for (float& v : LF_noisy[st]) {
            all++;
            if (u(g) < p) { v = (g() & 1ull) ? 255.0f : 0.0f; hit++; }
        }
    }
    cout << "Add impulses [p = " << p << "]: " << hit << " of " << all << " values replaced by 0 or 255" << endl;
}

/* LFBM5D_IMPULSE: repair the noisy light field in place */
bool repair_impulses_LF(vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, unsigned W, unsigned H, unsigned C, double k) {
    unsigned long long flagged = 0, left = 0, all = 0;
    double T[3] = {0.0, 0.0, 0.0};
    if (impulse_repair_LF(LF_noisy, mask, W, H, C, k, flagged, left, T) != EXIT_SUCCESS) return false;
    for (size_t st = 0; st < mask.size(); st++) if (mask[st]) all += (unsigned long long)W * H * C;
    cout << endl << "Impulse repair: " << flagged << " of " << all << " values flagged (" << 100.0 * (double)flagged / (double)all << " %), " << left
         << " left; thresholds " << T[0] << " " << T[1] << " " << T[2] << endl;
    return true;
}

/* LFBM5D_DEFECTS / LFBM5D_DEFECTS_ITER: dir = NULL: no inpainting; iter < 0: the library's number of steps; false (message printed) on a
 * malformed value */
bool defects_mode(const char*& dir, int& iter) {
    dir = env("LFBM5D_DEFECTS"); iter = -1;
    if (dir && !*dir) { cout << "LFBM5D_DEFECTS must name a directory of defect maps (PNG files named like the SAIs), or be unset" << endl; return false; }
    if (const char* e = env("LFBM5D_DEFECTS_ITER")) {
        char* q = nullptr;
        const long v = strtol(e, &q, 10);
        if (q == e || *q || isspace((unsigned char)*e) || v < 0 || v > 1000) {
            cout << "LFBM5D_DEFECTS_ITER must be a number of refinement steps 0 <= K <= 1000, or unset; got \"" << e << "\"" << endl;
            return false;
        }
        iter = (int)v;
    }
    return true;
}

/* the defect maps of LFBM5D_DEFECTS: one uint8 plane set per non-empty SAI, non-zero = defective */
bool load_defects(const char* dir, const char* name, const char* sep, vector<vector<unsigned char> >& flags, const vector<unsigned>& mask,
                  unsigned ang_major, unsigned aw, unsigned ah, unsigned s0, unsigned t0, unsigned W, unsigned H, unsigned C) {
    flags.assign(aw * ah, vector<unsigned char>());
    const size_t plane = (size_t)W * H;
    for (unsigned s = 0; s < ah; s++)
        for (unsigned t = 0; t < aw; t++) {
            const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
            if (!mask[st]) continue;
            flags[st].assign(plane * C, 0);
            const string p = sai_path(dir, name, sep, s + s0, t + t0);
            if (!ifstream(p)) continue;   /* no file: no defects in this SAI */
            vector<float> img; size_t w, h, c;
            if (!png_read_planar_f32(p, img, w, h, c) || w != W || h != H) {
                cout << "error :: defect map " << p << " is not a png image of the SAIs' size." << endl;
                return false;
            }
            const size_t colours = c >= 3 ? 3 : 1;   /* alpha is dropped */
            for (unsigned ch = 0; ch < C; ch++)
                for (size_t k = 0; k < plane; k++) {
                    bool f;
                    if (colours == 1) f = img[k] != 0.0f;
                    else if (C == 3) f = img[ch * plane + k] != 0.0f;
                    else f = img[k] != 0.0f || img[plane + k] != 0.0f || img[2 * plane + k] != 0.0f;
                    flags[st][ch * plane + k] = f ? 1 : 0;
                }
        }
    return true;
}

/* LFBM5D_DEFECTS: the fill (steps = 0) or the fill and the refinement loop, in place; hard = N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D,
 * tau_5D of the hard-thresholding step.  report: print the line of the header comment, with the steps that are still to come. */
bool inpaint_defects_LF(vector<vector<float> >& LF_noisy, const vector<vector<unsigned char> >& flags, const vector<unsigned>& mask,
                        unsigned ang_major, unsigned aw, unsigned ah, unsigned an, unsigned W, unsigned H, unsigned C, unsigned steps,
                        unsigned steps_to_come, float sigma_noise, float lambda, const unsigned* hard, unsigned cs, bool report) {
    unsigned long long flagged = 0, left = 0, all = 0; unsigned passes = 0;
    if (inpaint_LF(LF_noisy, flags, mask, ang_major, aw, ah, an, W, H, C, (int)steps, 0.0f, 0.0f, sigma_noise, lambda, hard[0], hard[1], hard[2],
                   hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], cs, flagged, left, passes) != EXIT_SUCCESS) return false;
    for (size_t st = 0; st < mask.size(); st++) if (mask[st]) all += (unsigned long long)W * H * C;
    if (report)
        cout << endl << "Defect inpainting: " << flagged << " of " << all << " values flagged (" << 100.0 * (double)flagged / (double)all << " %), "
             << left << " left; " << passes << " fill passes, " << steps_to_come << " refinement steps" << endl;
    return true;
}

/* LFBM5D_MISSING / LFBM5D_MISSING_ITER: missing stays empty when unset, else one entry per SAI (non-zero = to be reconstructed);
 * iter < 0: the library's number of steps; false (message printed) on a malformed value or together with LFBM5D_DEFECTS (unless
 * LFBM5D_REPAIR is set, which repair_mode() has checked by then) */
bool missing_mode(vector<unsigned>& missing, int& iter, unsigned ang_major, unsigned aw, unsigned ah, unsigned s0, unsigned t0) {
    missing.clear(); iter = -1;
    if (const char* e = env("LFBM5D_MISSING_ITER")) {
        char* q = nullptr;
        const long v = strtol(e, &q, 10);
        if (q == e || *q || isspace((unsigned char)*e) || v < 0 || v > 1000) {
            cout << "LFBM5D_MISSING_ITER must be a number of refinement steps 0 <= K <= 1000, or unset; got \"" << e << "\"" << endl;
            return false;
        }
        iter = (int)v;
    }
    const char* e = env("LFBM5D_MISSING");
    if (!e) return true;
    if (env("LFBM5D_DEFECTS") && !env("LFBM5D_REPAIR")) { cout << "LFBM5D_MISSING cannot be combined with LFBM5D_DEFECTS (there is no combined loop): run them one after the other" << endl; return false; }
    missing.assign((size_t)aw * ah, 0u);
    const char* p = e;
    bool ok = *p != 0;
    while (ok) {
        char *q = nullptr, *r = nullptr;
        ok = isdigit((unsigned char)*p) != 0;
        const long s = ok ? strtol(p, &q, 10) : 0;
        ok = ok && *q == '_' && isdigit((unsigned char)q[1]);
        const long t = ok ? strtol(q + 1, &r, 10) : 0;
        ok = ok && s >= (long)s0 && s < (long)(s0 + ah) && t >= (long)t0 && t < (long)(t0 + aw);
        if (!ok) break;
        const unsigned ss = (unsigned)s - s0, tt = (unsigned)t - t0;
        missing[ang_major == LFBM5D_ROWMAJOR ? ss * aw + tt : ss + tt * ah] = 1;
        if (!*r) break;
        ok = *r == ',';
        p = r + 1;
    }
    if (!ok) {
        cout << "LFBM5D_MISSING must be a list <s>_<t>[,<s>_<t>...] of SAIs of the light field, in the indices the file names carry, or unset; got \""
             << e << "\"" << endl;
        return false;
    }
    return true;
}

/* LFBM5D_MISSING: the synthesis (steps = 0) or the synthesis and the refinement loop, in place; hard as for inpaint_defects_LF.  report:
 * print the line of the header comment, with the steps that are still to come. */
bool synthesise_missing_LF(vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, const vector<unsigned>& missing, unsigned ang_major,
                           unsigned aw, unsigned ah, unsigned an, unsigned W, unsigned H, unsigned C, unsigned steps, unsigned steps_to_come,
                           float sigma_noise, float lambda, const unsigned* hard, unsigned cs, bool report, unsigned dsteps,
                           float occl) {
    unsigned done = 0, left = 0, all = 0, n = 0; int dmin = 0, dmax = 0;
    unsigned long long sets[5] = {0, 0, 0, 0, 0};
    if (view_synth_LF(LF_noisy, mask, missing, ang_major, aw, ah, an, W, H, C, -1, -1, -1, (int)steps, 0.0f, 0.0f, sigma_noise, lambda, hard[0],
                      hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], cs, done, left, dmin, dmax, dsteps, occl,
                      sets) != EXIT_SUCCESS)
        return false;
    for (size_t st = 0; st < mask.size(); st++) { if (mask[st]) all++; if (missing[st]) n++; }
    if (report && dsteps == 1)
        cout << endl << "View synthesis: " << n << " of " << all << " SAIs missing, " << left << " left; disparities " << dmin << ".." << dmax << ", "
             << steps_to_come << " refinement steps";
    else if (report)                                                            /* the range is in units of 1 / dsteps: printed in pixels */
        cout << endl << "View synthesis: " << n << " of " << all << " SAIs missing, " << left << " left; disparities " << dmin / (double)dsteps << ".."
             << dmax / (double)dsteps << ", " << steps_to_come << " refinement steps, " << dsteps << " steps per pixel";
    if (report && occl != 0.0f) {
        const unsigned long long total = sets[0] + sets[1] + sets[2] + sets[3] + sets[4];
        char txt[96];                                                           /* its own format: cout's flags are the measures' */
        snprintf(txt, sizeof(txt), ", occlusion ratio %g: %.1f %% of the positions from a half-plane", (double)occl,
                 total ? 100.0 * (double)(total - sets[0]) / (double)total : 0.0);
        cout << txt;
    }
    if (report) cout << endl;
    return true;
}

/* LFBM5D_REPAIR / LFBM5D_REPAIR_ITER: joint = false when unset; iter < 0: the library's number of steps; false (message printed) on a
 * malformed value, LFBM5D_REPAIR_ITER alone, nothing to hand to the job, or a combination the header comment excludes.  Ahead of every
 * other *_mode(): missing_mode() admits LFBM5D_DEFECTS beside LFBM5D_MISSING only under it. */
bool repair_mode(bool& joint, int& iter, int smode) {
    joint = false; iter = -1;
    const char* e = env("LFBM5D_REPAIR");
    const char* it = env("LFBM5D_REPAIR_ITER");
    if (!e) {
        if (it) { cout << "LFBM5D_REPAIR_ITER needs LFBM5D_REPAIR" << endl; return false; }
        return true;
    }
    if (strcmp(e, "joint")) {
        cout << "LFBM5D_REPAIR must be \"joint\" (defects and missing views repaired together by one mask-aware sweep and one loop), or unset; got \""
             << e << "\"" << endl;
        return false;
    }
    if (it) {
        char* q = nullptr;
        const long v = strtol(it, &q, 10);
        if (q == it || *q || isspace((unsigned char)*it) || v < 0 || v > 1000) {
            cout << "LFBM5D_REPAIR_ITER must be a number of refinement steps 0 <= K <= 1000, or unset; got \"" << it << "\"" << endl;
            return false;
        }
        iter = (int)v;
    }
    if (!env("LFBM5D_DEFECTS") && !env("LFBM5D_MISSING") && !env("LFBM5D_DETECT")) {
        cout << "LFBM5D_REPAIR needs LFBM5D_DEFECTS, LFBM5D_MISSING or LFBM5D_DETECT" << endl;
        return false;
    }
    if (const char* d = env("LFBM5D_DISPARITY_STEPS"))
        if (strcmp(d, "1")) { cout << "LFBM5D_REPAIR cannot be combined with LFBM5D_DISPARITY_STEPS other than 1 (the joint sweep takes integer disparities only)" << endl; return false; }
    if (env("LFBM5D_OCCLUSION")) { cout << "LFBM5D_REPAIR cannot be combined with LFBM5D_OCCLUSION (the joint sweep does not reason about occlusions)" << endl; return false; }
    if (smode >= 2) { cout << "LFBM5D_REPAIR cannot be combined with LFBM5D_SIGMA=poisson (the refinement steps assume one sigma)" << endl; return false; }
    if (env("LFBM5D_VIEW_SIGMA")) { cout << "LFBM5D_REPAIR cannot be combined with LFBM5D_VIEW_SIGMA (the refinement steps assume one sigma)" << endl; return false; }
    joint = true;
    return true;
}

/* LFBM5D_REPAIR=joint: the fill (steps = 0) or the fill and the refinement loop, in place; flags and missing may be empty; hard as for
 * inpaint_defects_LF.  report: print the line of the header comment, with the steps that are still to come. */
bool repair_joint_LF(vector<vector<float> >& LF_noisy, const vector<vector<unsigned char> >& flags, const vector<unsigned>& mask,
                     const vector<unsigned>& missing, unsigned ang_major, unsigned aw, unsigned ah, unsigned an, unsigned W, unsigned H, unsigned C,
                     unsigned steps, unsigned steps_to_come, float sigma_noise, float lambda, const unsigned* hard, unsigned cs, bool report) {
    unsigned long long r[6];   /* values, flagged, missing, from other views, from the rim, left */
    int dmin = 0, dmax = 0;
    if (repair_LF(LF_noisy, flags, mask, missing, ang_major, aw, ah, an, W, H, C, -1, -1, -1, -1, (int)steps, 0.0f, 0.0f, sigma_noise, lambda, hard[0],
                  hard[1], hard[2], hard[3], hard[4], hard[5] != 0, hard[6], hard[7], hard[8], cs, r, dmin, dmax) != EXIT_SUCCESS) return false;
    unsigned all = 0;
    for (size_t st = 0; st < mask.size(); st++) if (mask[st]) all++;
    if (report)
        cout << endl << "Joint repair: " << r[1] << " of " << r[0] << " values flagged (" << 100.0 * (double)r[1] / (double)r[0] << " %), " << r[2]
             << " of " << all << " SAIs missing; " << r[3] << " values from other views, " << r[4] << " from the rim, " << r[5]
             << " left; disparities " << dmin << ".." << dmax << ", " << steps_to_come << " refinement steps" << endl;
    return true;
}

/* LFBM5D_EQUALISE / LFBM5D_EQUALISE_ADD: mode 0 when unset, 1 = auto, 2 = flat; add = 0 when unset; false (message printed) on a malformed
 * value, together with LFBM5D_SIGMA=poisson (smode >= 2) or LFBM5D_CLIP, or LFBM5D_EQUALISE_ADD without a ground truth.  Ahead of
 * disparity_steps_mode(), which counts its sweep. */
bool equalise_mode(int& mode, double& add, int smode, bool gt) {
    mode = 0; add = 0.0;
    if (const char* e = env("LFBM5D_EQUALISE")) {
        mode = !strcmp(e, "auto") ? 1 : !strcmp(e, "flat") ? 2 : 0;
        if (!mode) {
            cout << "LFBM5D_EQUALISE must be \"auto\" (equalise the views, give the results their own photometry back) or \"flat\" (leave the "
                    "results equalised), or unset; got \"" << e << "\"" << endl;
            return false;
        }
        if (smode >= 2) {
            cout << "LFBM5D_EQUALISE cannot be combined with LFBM5D_SIGMA=poisson (a gain changes the noise model)" << endl;
            return false;
        }
        if (env("LFBM5D_CLIP")) {
            cout << "LFBM5D_EQUALISE cannot be combined with LFBM5D_CLIP (a gain changes the clipping range)" << endl;
            return false;
        }
    }
    if (const char* e = env("LFBM5D_EQUALISE_ADD")) {
        char* q = nullptr;
        add = strtod(e, &q);
        if (q == e || *q || isspace((unsigned char)*e) || !(add > 0.0) || !(add <= 1.0)) {
            cout << "LFBM5D_EQUALISE_ADD must be the gain of the corner views, 0 < edge <= 1, or unset; got \"" << e << "\"" << endl;
            return false;
        }
        if (!gt) { cout << "LFBM5D_EQUALISE_ADD needs a source light field to synthesise the noisy one from" << endl; return false; }
    }
    return true;
}

/* LFBM5D_VIEW_SIGMA / LFBM5D_VIEW_SIGMA_ADD: mode 0 when unset, 1 = auto, 2 = gains; add = 0 when unset; false (message printed) on a
 * malformed value, a combination the header comment excludes, or LFBM5D_VIEW_SIGMA_ADD without a ground truth */
bool view_sigma_mode(int& mode, double& add, int smode, bool gt) {
    mode = 0; add = 0.0;
    if (const char* e = env("LFBM5D_VIEW_SIGMA")) {
        mode = !strcmp(e, "auto") ? 1 : !strcmp(e, "gains") ? 2 : 0;
        if (!mode) {
            cout << "LFBM5D_VIEW_SIGMA must be \"auto\" (estimate one noise level per view from the noisy light field) or \"gains\" (derive them "
                    "from sigma and the gains of LFBM5D_EQUALISE), or unset; got \"" << e << "\"" << endl;
            return false;
        }
        if (smode >= 2) {
            cout << "LFBM5D_VIEW_SIGMA cannot be combined with LFBM5D_SIGMA=poisson (per-view signal-dependent models are not covered)" << endl;
            return false;
        }
        if (env("LFBM5D_CLIP")) {
            cout << "LFBM5D_VIEW_SIGMA cannot be combined with LFBM5D_CLIP (the clipped estimate and the declipping assume one sigma)" << endl;
            return false;
        }
        if (env("LFBM5D_MISSING") || env("LFBM5D_DEFECTS") || env("LFBM5D_DETECT")) {
            cout << "LFBM5D_VIEW_SIGMA cannot be combined with LFBM5D_MISSING, LFBM5D_DEFECTS or LFBM5D_DETECT (their refinement steps assume one sigma)" << endl;
            return false;
        }
        if (mode == 2 && !env("LFBM5D_EQUALISE")) {
            cout << "LFBM5D_VIEW_SIGMA=gains needs LFBM5D_EQUALISE (the gains it divides out)" << endl;
            return false;
        }
        if (mode == 2 && smode == 1) {
            cout << "LFBM5D_VIEW_SIGMA=gains needs a numeric sigma, not LFBM5D_SIGMA=auto: LFBM5D_VIEW_SIGMA=auto estimates every view's level" << endl;
            return false;
        }
    }
    if (const char* e = env("LFBM5D_VIEW_SIGMA_ADD")) {
        char* q = nullptr;
        add = strtod(e, &q);
        if (q == e || *q || isspace((unsigned char)*e) || !(add > 0.0) || !(add <= 1.0)) {
            cout << "LFBM5D_VIEW_SIGMA_ADD must be the vignette gain of the corner views, 0 < edge <= 1, or unset; got \"" << e << "\"" << endl;
            return false;
        }
        if (!gt) { cout << "LFBM5D_VIEW_SIGMA_ADD needs a source light field to synthesise the noisy one from" << endl; return false; }
        if (smode >= 2) { cout << "LFBM5D_VIEW_SIGMA_ADD cannot be combined with LFBM5D_SIGMA=poisson (the synthesised noise is Gaussian)" << endl; return false; }
    }
    return true;
}

/* taps of LFBM5D_NOISE_CORR=kernel:<file> / LFBM5D_NOISE_CORR_ADD=<file>: one row per line, 1..7 rows of 1..7 numbers, all rows as long */
bool read_taps(const char* var, const char* path, vector<double>& g, unsigned& gh, unsigned& gw) {
    ifstream f(path);
    if (!f) { cout << var << ": cannot read \"" << path << "\"" << endl; return false; }
    g.clear(); gh = gw = 0;
    string line;
    while (getline(f, line)) {
        istringstream ls(line);
        vector<double> row;
        string tok;
        while (ls >> tok) {
            char* end = nullptr;
            const double v = strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end || !std::isfinite(v)) { cout << var << ": \"" << tok << "\" in \"" << path << "\" is not a finite number" << endl; return false; }
            row.push_back(v);
        }
        if (row.empty()) continue;
        if (gh && row.size() != gw) { cout << var << ": the rows of \"" << path << "\" differ in length" << endl; return false; }
        gw = (unsigned)row.size(); gh++;
        g.insert(g.end(), row.begin(), row.end());
    }
    if (gh < 1 || gh > 7 || gw < 1 || gw > 7) { cout << var << ": \"" << path << "\" must hold 1..7 rows of 1..7 taps" << endl; return false; }
    return true;
}

/* LFBM5D_NOISE_CORR / LFBM5D_NOISE_CORR_ADD: mode 0 when unset, 1 = auto, 2 = <file>, 3 = kernel:<file>; acf filled for 2 and 3; add_taps
 * empty when unset; false (message printed) on a malformed value, a combination the header comment excludes, or LFBM5D_NOISE_CORR_ADD
 * without a ground truth */
bool noise_corr_mode(int& mode, vector<double>& acf, vector<double>& add_taps, unsigned& add_h, unsigned& add_w, int smode, bool gt, bool bm3d) {
    mode = 0; add_h = add_w = 0;
    if (const char* e = env("LFBM5D_NOISE_CORR")) {
        if (bm3d) { cout << "LFBM5D_NOISE_CORR is not supported by LFBM3Ddenoising (the per-SAI BM3D flavour has no variance table)" << endl; return false; }
        if (smode != 0) { cout << "LFBM5D_NOISE_CORR cannot be combined with LFBM5D_SIGMA (the command's sigma is the marginal level of the correlated noise)" << endl; return false; }
        for (const char* other : {"LFBM5D_CLIP", "LFBM5D_VIEW_SIGMA", "LFBM5D_REPAIR", "LFBM5D_DEFECTS", "LFBM5D_MISSING", "LFBM5D_DETECT", "LFBM5D_EQUALISE"})
            if (env(other)) { cout << "LFBM5D_NOISE_CORR cannot be combined with " << other << " (their stages assume white noise)" << endl; return false; }
        if (!*e) { cout << "LFBM5D_NOISE_CORR must be \"auto\", a file of 49 numbers or kernel:<file of taps>, or unset; got \"\"" << endl; return false; }
        if (!strcmp(e, "auto")) mode = 1;
        else if (!strncmp(e, "kernel:", 7)) {
            vector<double> g; unsigned gh, gw;
            if (!read_taps("LFBM5D_NOISE_CORR", e + 7, g, gh, gw)) return false;
            acf.assign(49, 0.0);
            if (lfbm5d_corr_from_kernel(g.data(), gh, gw, acf.data())) { cout << "LFBM5D_NOISE_CORR: " << lfbm5d_corr_error() << endl; return false; }
            mode = 3;
        } else {
            ifstream f(e);
            if (!f) { cout << "LFBM5D_NOISE_CORR must be \"auto\", a file of 49 numbers or kernel:<file of taps>, or unset; cannot read \"" << e << "\"" << endl; return false; }
            acf.clear();
            string tok;
            while (f >> tok) {
                char* end = nullptr;
                const double v = strtod(tok.c_str(), &end);
                if (end == tok.c_str() || *end) { cout << "LFBM5D_NOISE_CORR: \"" << tok << "\" in \"" << e << "\" is not a number" << endl; return false; }
                acf.push_back(v);
            }
            if (acf.size() != 49) { cout << "LFBM5D_NOISE_CORR: \"" << e << "\" must hold 49 numbers (the lags -3..3 row-major), it holds " << acf.size() << endl; return false; }
            if (lfbm5d_corr_check(acf.data())) { cout << "LFBM5D_NOISE_CORR: " << lfbm5d_corr_error() << endl; return false; }
            mode = 2;
        }
    }
    if (const char* e = env("LFBM5D_NOISE_CORR_ADD")) {
        if (bm3d) { cout << "LFBM5D_NOISE_CORR_ADD is not supported by LFBM3Ddenoising" << endl; return false; }
        if (!gt) { cout << "LFBM5D_NOISE_CORR_ADD needs a source light field to synthesise the noisy one from" << endl; return false; }
        if (smode >= 2) { cout << "LFBM5D_NOISE_CORR_ADD cannot be combined with LFBM5D_SIGMA=poisson (the synthesised noise is Gaussian)" << endl; return false; }
        if (!read_taps("LFBM5D_NOISE_CORR_ADD", e, add_taps, add_h, add_w)) return false;
        double en = 0.0;
        for (double v : add_taps) en += v * v;
        if (!(en > 0.0)) { cout << "LFBM5D_NOISE_CORR_ADD: the taps are all zero" << endl; return false; }
        for (double& v : add_taps) v /= sqrt(en);
    }
    return true;
}

/* LFBM5D_NOISE_CORR_ADD: the synthesised noise (noisy - clean) of every plane filtered by the unit-energy taps, periodic at the border */
void correlate_noise_LF(const vector<vector<float> >& LF, const vector<unsigned>& mask, vector<vector<float> >& LF_noisy, unsigned W, unsigned H,
                        unsigned C, const vector<double>& g, unsigned gh, unsigned gw) {
    parallel_sais((unsigned)LF.size(), [&](unsigned st) {
        if (!mask[st]) return true;
        vector<double> n((size_t)W * H);
        for (unsigned c = 0; c < C; c++) {
            const size_t o = (size_t)c * W * H;
            for (size_t q = 0; q < n.size(); q++) n[q] = (double)LF_noisy[st][o + q] - (double)LF[st][o + q];
            for (unsigned y = 0; y < H; y++)
                for (unsigned x = 0; x < W; x++) {
                    double z = 0.0;
                    for (unsigned i = 0; i < gh; i++)
                        for (unsigned j = 0; j < gw; j++)
                            z += g[i * gw + j] * n[(size_t)((y + i + H - gh / 2) % H) * W + (x + j + W - gw / 2) % W];
                    LF_noisy[st][o + (size_t)y * W + x] = LF[st][o + (size_t)y * W + x] + (float)z;
                }
        }
        return true;
    });
}

/* LFBM5D_NOISE_CORR: the line that reports the autocorrelation the filter ran with and the variance tables of both steps */
bool print_noise_corr(const vector<double>& acf, int mode, const int* t2, const unsigned* k) {
    float lo[2] = {1.0f, 1.0f}, hi[2] = {1.0f, 1.0f};
    unsigned clamped = 0;
    for (int i = 0; i < 2; i++) {
        vector<float> v((size_t)k[i] * k[i]);
        unsigned cl = 0;
        if (lfbm5d_corr_table(acf.data(), (unsigned)t2[i], k[i], nullptr, v.data(), &cl)) { cout << "LFBM5D_NOISE_CORR: " << lfbm5d_corr_error() << endl; return false; }
        lo[i] = *std::min_element(v.begin(), v.end()); hi[i] = *std::max_element(v.begin(), v.end());
        clamped += cl;
    }
    cout << "Noise correlation: lag-1 " << acf[3 * 7 + 4] << " " << acf[4 * 7 + 3] << ", variance factors " << lo[0] << ".." << hi[0] << " (step 1), "
         << lo[1] << ".." << hi[1] << " (step 2), " << clamped << " clamped; from " << (mode == 1 ? "estimate" : mode == 2 ? "file" : "kernel") << endl;
    return true;
}

/* the smooth vignette of LFBM5D_EQUALISE_ADD and LFBM5D_VIEW_SIGMA_ADD: view (s, t) gets 1 - (1 - edge) rho^2, rho its angular distance from
 * the centre, 1 at the corners */
double vignette_gain(unsigned s, unsigned t, unsigned aw, unsigned ah, double edge) {
    const double cs = (ah - 1) / 2.0, ct = (aw - 1) / 2.0, corner = cs * cs + ct * ct;
    const double rho2 = corner > 0.0 ? ((s - cs) * (s - cs) + (t - ct) * (t - ct)) / corner : 0.0;
    return 1.0 - (1.0 - edge) * rho2;
}

/* LFBM5D_VIEW_SIGMA_ADD: sigma_v = sigma / g_v */
vector<double> vignette_sigmas(float sigma, unsigned ang_major, unsigned aw, unsigned ah, double edge) {
    vector<double> out((size_t)aw * ah, 0.0);
    for (unsigned s = 0; s < ah; s++)
        for (unsigned t = 0; t < aw; t++)
            out[ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah] = (double)sigma / vignette_gain(s, t, aw, ah, edge);
    return out;
}

/* LFBM5D_VIEW_SIGMA: the line that reports the table the filter ran with */
void print_view_sigmas(const vector<double>& table, const vector<unsigned>& mask, const vector<float>& window_sigmas, bool estimated) {
    unsigned n = 0;
    double lo = 0.0, hi = 0.0, sum = 0.0;
    for (size_t st = 0; st < table.size(); st++) {
        if (!mask[st]) continue;
        lo = n ? std::min(lo, table[st]) : table[st]; hi = n ? std::max(hi, table[st]) : table[st];
        sum += table[st] * table[st];
        n++;
    }
    float wlo = 0.0f, whi = 0.0f;
    for (size_t i = 0; i < window_sigmas.size(); i++) {
        wlo = i ? std::min(wlo, window_sigmas[i]) : window_sigmas[i]; whi = i ? std::max(whi, window_sigmas[i]) : window_sigmas[i];
    }
    cout << endl << "Per-view noise levels: " << n << " SAIs, sigma " << lo << ".." << hi << " (pooled " << (n ? sqrt(sum / n) : 0.0) << "), from "
         << (estimated ? "estimate" : "gains") << "; window sigmas " << wlo << ".." << whi << endl;
}

/* LFBM5D_EQUALISE_ADD: view (s, t) times its vignette gain */
void add_vignette_LF(vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, unsigned ang_major, unsigned aw, unsigned ah, double edge) {
    for (unsigned s = 0; s < ah; s++)
        for (unsigned t = 0; t < aw; t++) {
            const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
            if (!mask[st]) continue;
            const float g = (float)vignette_gain(s, t, aw, ah, edge);
            for (float& v : LF_noisy[st]) v = v * g;
        }
    cout << "Vignette [corner views x " << edge << "]" << endl;
}

/* LFBM5D_EQUALISE: the noisy light field equalised in place; `gains` for restore_LF */
bool equalise_noisy_LF(vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, unsigned ang_major, unsigned aw, unsigned ah, unsigned W,
                       unsigned H, unsigned C, unsigned dsteps, vector<double>& gains) {
    vector<unsigned> state;
    unsigned fitted = 0, untested = 0, unfit = 0, rounds = 0, sais = 0;
    double residual = 0.0, gmin = 1.0, gmax = 1.0;
    if (equalise_LF(LF_noisy, mask, LF_noisy, ang_major, aw, ah, W, H, C, -1, -1, -1, -1, -1, -1, -1, -1.0, -1.0, -1.0, gains, state, fitted, untested,
                    unfit, rounds, residual, gmin, gmax, dsteps) != EXIT_SUCCESS) return false;
    for (size_t st = 0; st < mask.size(); st++) sais += mask[st] != 0;
    cout << endl << "Photometric equalisation: " << fitted << " of " << sais << " SAIs fitted, " << untested << " untested, " << unfit << " unfit; gains "
         << gmin << ".." << gmax << "; " << rounds << " sweeps, residual " << residual;
    if (dsteps > 1) cout << ", " << dsteps << " steps per pixel";
    cout << endl;
    return true;
}

/* LFBM5D_EQUALISE=auto: a result of the filter gets every view's own photometry back */
bool restore_LF(vector<vector<float> >& LF_out, const vector<unsigned>& mask, const vector<double>& gains, unsigned aw, unsigned ah, unsigned W,
                unsigned H, unsigned C) {
    return apply_gains_LF(LF_out, mask, gains, true, aw, ah, W, H, C) == EXIT_SUCCESS;
}

/* LFBM5D_DETECT / LFBM5D_DETECT_SAVE: on = false when unset; k < 0 = the library's factor; false (message printed) on a malformed value,
 * LFBM5D_DETECT_SAVE without LFBM5D_DETECT, or together with LFBM5D_DEFECTS / LFBM5D_MISSING */
bool detect_mode(bool& on, double& k, const char*& save) {
    on = false; k = -1.0;
    save = env("LFBM5D_DETECT_SAVE");
    const char* e = env("LFBM5D_DETECT");
    if (!e) {
        if (save) { cout << "LFBM5D_DETECT_SAVE needs LFBM5D_DETECT" << endl; return false; }
        return true;
    }
    if (strcmp(e, "auto")) {
        char* q = nullptr;
        const double v = strtod(e, &q);
        if (q == e || *q || isspace((unsigned char)*e) || !std::isfinite(v) || v < 0.0) {
            cout << "LFBM5D_DETECT must be \"auto\" (consistency check with the library's threshold factor) or a factor k >= 0, or unset; got \""
                 << e << "\"" << endl;
            return false;
        }
        k = v;
    }
    if (save && !*save) { cout << "LFBM5D_DETECT_SAVE must name a directory for the detected maps, or be unset" << endl; return false; }
    if (env("LFBM5D_DEFECTS")) { cout << "LFBM5D_DETECT cannot be combined with LFBM5D_DEFECTS (there is no combined loop of a given and a detected map): run them one after the other" << endl; return false; }
    if (env("LFBM5D_MISSING")) { cout << "LFBM5D_DETECT cannot be combined with LFBM5D_MISSING (there is no combined loop of given and detected SAIs): run them one after the other" << endl; return false; }
    on = true;
    return true;
}

/* LFBM5D_DISPARITY_STEPS: 1 when unset; false (message printed) on anything but 1, 2 or 4, or without a sweep to apply it to.  After
 * missing_mode() and detect_mode(). */
bool disparity_steps_mode(unsigned& dsteps, bool sweeps) {
    dsteps = 1;
    const char* e = env("LFBM5D_DISPARITY_STEPS");
    if (!e) return true;
    if (strcmp(e, "1") && strcmp(e, "2") && strcmp(e, "4")) {
        cout << "LFBM5D_DISPARITY_STEPS must be 1, 2 or 4, or unset; got \"" << e << "\"" << endl;
        return false;
    }
    if (!sweeps) { cout << "LFBM5D_DISPARITY_STEPS needs LFBM5D_MISSING or LFBM5D_DETECT" << endl; return false; }
    dsteps = (unsigned)(e[0] - '0');
    return true;
}

/* LFBM5D_OCCLUSION: 0 (the plain sweep) when unset; false (message printed) on anything but "auto" or a finite ratio >= 1, or without a
 * synthesis to apply it to.  After missing_mode() and detect_mode(). */
bool occlusion_mode(float& occl, bool synthesis) {
    occl = 0.0f;
    const char* e = env("LFBM5D_OCCLUSION");
    if (!e) return true;
    if (!strcmp(e, "auto")) occl = lfbm5d_view_occl_default();
    else {
        char* q = nullptr;
        const float v = strtof(e, &q);
        if (q == e || *q || !(isdigit((unsigned char)*e) || *e == '.') || strpbrk(e, "xXpP") || !std::isfinite(v) || v < 1.0f) {
            cout << "LFBM5D_OCCLUSION must be \"auto\" (the library's ratio) or a finite ratio >= 1, or unset; got \"" << e << "\"" << endl;
            return false;
        }
        occl = v;
    }
    if (!synthesis) { cout << "LFBM5D_OCCLUSION needs LFBM5D_MISSING or LFBM5D_DETECT" << endl; return false; }
    return true;
}

/* LFBM5D_DETECT: the check; `missing` receives the bad SAIs (left empty when there is none), `defects` the flag planes (left empty when
 * nothing is flagged); LFBM5D_DETECT_SAVE: the maps and the list */
bool detect_LF(const vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, double k, const char* save, const char* name, const char* sep,
               unsigned ang_major, unsigned aw, unsigned ah, unsigned s0, unsigned t0, unsigned W, unsigned H, unsigned C, vector<unsigned>& missing,
               vector<vector<unsigned char> >& defects, unsigned dsteps) {
    vector<unsigned> state;
    vector<vector<unsigned char> > flags;
    unsigned long long flagged = 0, nonfinite = 0, all = 0; unsigned bad = 0, untested = 0, rounds = 0, sais = 0;
    double sc[3] = {0.0, 0.0, 0.0};
    if (consist_LF(LF_noisy, mask, vector<unsigned>(), ang_major, aw, ah, W, H, C, -1, -1, -1, -1, -1, k, -1.0, -1.0, flags, state, flagged, nonfinite, bad,
                   untested, rounds, sc, dsteps) != EXIT_SUCCESS) return false;
    ostringstream list, line;
    for (unsigned s = 0; s < ah; s++)
        for (unsigned t = 0; t < aw; t++) {
            const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
            if (!mask[st]) continue;
            sais++; all += (unsigned long long)W * H * C;
            if (state[st] != 2u) continue;
            list << (list.tellp() > 0 ? " " : "") << s + s0 << "_" << t + t0;
            line << (line.tellp() > 0 ? "," : "") << s + s0 << "_" << t + t0;
        }
    const unsigned long long n = flagged + nonfinite;
    cout << endl << "Consistency check: " << bad << " of " << sais << " SAIs bad [" << list.str() << "], " << n << " of " << all << " values flagged ("
         << 100.0 * (double)n / (double)all << " %), " << untested << " SAIs untested; scales " << sc[0] << " " << sc[1] << " " << sc[2] << "; " << rounds
         << " sweeps";
    if (dsteps > 1) cout << ", " << dsteps << " steps per pixel";
    cout << endl;
    if (save) {
        const size_t plane = (size_t)W * H;
        vector<float> img(plane * C);
        for (unsigned s = 0; s < ah; s++)
            for (unsigned t = 0; t < aw; t++) {
                const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
                if (!mask[st]) continue;
                for (size_t i = 0; i < plane * C; i++) img[i] = flags[st][i] ? 255.0f : 0.0f;
                const string p = sai_path(save, name, sep, s + s0, t + t0);
                if (!png_write_planar_f32(p, img.data(), W, H, C)) { cout << "error :: cannot write the detected map " << p << endl; return false; }
            }
        ofstream f(string(save) + "/missing.txt");
        f << line.str() << endl;
        if (!f) { cout << "error :: cannot write " << save << "/missing.txt" << endl; return false; }
    }
    missing.clear(); defects.clear();
    if (bad) { missing.assign(mask.size(), 0u); for (size_t st = 0; st < mask.size(); st++) missing[st] = state[st] == 2u; }
    if (n) defects.swap(flags);
    return true;
}

/* LFBM5D_SIGMA=poisson: the model of the noisy light field */
[[maybe_unused]] bool estimate_pg_LF(const vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, unsigned W, unsigned H, unsigned C, double* pg) {
    return pg_estimate_LF(LF_noisy, mask, W, H, C, pg[0], pg[1]) == EXIT_SUCCESS;
}

void print_pg_model(bool estimated, const double* pg, float s) {
    cout << endl << (estimated ? "Estimated" : "Given") << " noise model: a = " << setprecision(8) << pg[0] << ", b = " << pg[1]
         << " (sigma after stabilisation = " << s << ")" << setprecision(6) << endl;
}

/* LFBM5D_SIGMA=auto: replace `sigma` with the estimate on the noisy light field */
bool estimate_sigma_LF(const vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, unsigned W, unsigned H, unsigned C, float& sigma) {
    float est = 0.0f;
    if (noise_level_LF(LF_noisy, mask, W, H, C, est) != EXIT_SUCCESS) return false;
    cout << endl << "Estimated noise level: sigma = " << setprecision(8) << est << setprecision(6) << " (argument: " << sigma << ")" << endl;
    sigma = est;
    return true;
}

[[maybe_unused]] int tau(const char* s, int which) {
    if (!strcmp(s, "id")) return LFBM5D_ID;
    if (!strcmp(s, "dct")) return LFBM5D_DCT;
    if (which == 2 && !strcmp(s, "bior")) return LFBM5D_BIOR;
    if (which == 4 && !strcmp(s, "sadct")) return LFBM5D_SADCT;
    if (which == 5 && !strcmp(s, "hw")) return LFBM5D_HADAMARD;
    if (which == 5 && !strcmp(s, "haar")) return LFBM5D_HAAR;
    return -1;
}

[[maybe_unused]] void usage(const char* a0) {
    cout << "usage: " << a0 << " LFSourceDir|none SAIName sep awidth aheight sIdxStart tIdxStart aswSizeHard aswSizeWien row|col "
            "sigma lambda LFNoisyDir LFBasicDir LFDenoisedDir LFDiffDir NHard nSimHard nDispHard kHard pHard id|dct|bior id|dct|sadct "
            "hw|haar|dct useSDHard NWien nSimWien nDispWien kWien pWien id|dct|bior id|dct|sadct hw|haar|dct useSDWien "
            "rgb|yuv|ycbcr|opp nbThreads resultsFile" << endl;
}

/* every LFBM5D_* mode of the header comment, as both commands read it */
struct Modes {
    double pg[2] = {0.0, 0.0}; int smode = 0;                                           /* LFBM5D_SIGMA (sigma_mode) */
    int qmode = 0;                                                                      /* LFBM5D_REPORT_SSIM */
    double imp_k = -1.0, imp_add = 0.0;
    bool joint = false; int rep_iter = -1;
    const char* def_dir = nullptr; int def_iter = -1;
    vector<unsigned> missing; int miss_iter = -1;
    bool detect = false; double det_k = -1.0; const char* det_save = nullptr;
    int eq_mode = 0; double eq_add = 0.0;
    int vs_mode = 0; double vs_add = 0.0;
    int nc_mode = 0; vector<double> nc_acf, nc_add; unsigned nc_add_h = 0, nc_add_w = 0;
    unsigned dsteps = 1;
    float occl = 0.0f;
    bool clip_on = false, clip_add = false; double clip_lo = 0.0, clip_hi = 255.0;
    double pc_lo = 0.0, pc_hi = 255.0;                                                  /* LFBM5D_SIGMA=poisson-clipped: its range */
};

/* in the order the commands have always read them: the first bad value's message is the one printed.  bm3d: LFBM3Ddenoising, which
 * refuses LFBM5D_NOISE_CORR.  false: the message is out */
bool read_modes(Modes& m, unsigned ang_major, unsigned aw, unsigned ah, unsigned s0, unsigned t0, bool gt, bool bm3d) {
    return (m.smode = sigma_mode(m.pg)) >= 0 && (m.qmode = cli_quality::ssim_mode()) >= 0 && impulse_mode(m.imp_k, m.imp_add) &&
           repair_mode(m.joint, m.rep_iter, m.smode) && defects_mode(m.def_dir, m.def_iter) &&
           missing_mode(m.missing, m.miss_iter, ang_major, aw, ah, s0, t0) && detect_mode(m.detect, m.det_k, m.det_save) &&
           equalise_mode(m.eq_mode, m.eq_add, m.smode, gt) && view_sigma_mode(m.vs_mode, m.vs_add, m.smode, gt) &&
           noise_corr_mode(m.nc_mode, m.nc_acf, m.nc_add, m.nc_add_h, m.nc_add_w, m.smode, gt, bm3d) &&
           disparity_steps_mode(m.dsteps, m.detect || !m.missing.empty() || m.eq_mode) && occlusion_mode(m.occl, m.detect || !m.missing.empty()) &&
           clip_mode(m.clip_on, m.clip_lo, m.clip_hi, m.clip_add, m.smode) && clip_range_mode(m.pc_lo, m.pc_hi);
}

/* The noisy light field: with a ground truth (gt) the source is loaded, the noise the modes ask for is added and the result is saved;
 * without one it is loaded from its directory.  Then LFBM5D_EQUALISE and LFBM5D_DETECT, which come ahead of every repair.  (LFBM3Ddenoising
 * never has taps to filter the noise with: it refuses the variable.)  false: the message is out */
bool noisy_LF(Modes& m, bool gt, const char* src, const char* d_noisy, const char* name, const char* sep, unsigned ang_major, unsigned aw, unsigned ah,
              unsigned s0, unsigned t0, float sigma, vector<vector<float> >& LF, vector<vector<float> >& LF_noisy, vector<unsigned>& mask, unsigned& W,
              unsigned& H, unsigned& C, vector<double>& eq_gains, vector<vector<unsigned char> >& detected) {
    if (gt) {
        double t = now_s();
        if (load_LF(src, name, sep, LF, mask, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return false;
        cout << "Loading LF elapsed time = " << now_s() - t << "s." << endl;
        LF_noisy.assign(aw * ah, vector<float>((size_t)W * H * C, 0.0f));
        const bool poisson = m.smode == 3 || m.smode == 5;
        if (poisson) cout << endl << "Add noise [Poisson-Gaussian, a = " << m.pg[0] << ", b = " << m.pg[1] << "] ... " << flush;
        else if (m.vs_add > 0.0) cout << endl << "Add noise [sigma = " << sigma << " / vignette, corner views x " << m.vs_add << "] ... " << flush;
        else cout << endl << "Add noise [sigma = " << sigma << "] ... " << flush;
        t = now_s();
        const vector<double> vs_sigmas = m.vs_add > 0.0 ? vignette_sigmas(sigma, ang_major, aw, ah, m.vs_add) : vector<double>();
        add_noise_LF(LF, mask, LF_noisy, sigma, poisson ? m.pg : nullptr, m.vs_add > 0.0 ? &vs_sigmas : nullptr);
        if (!m.nc_add.empty()) correlate_noise_LF(LF, mask, LF_noisy, W, H, C, m.nc_add, m.nc_add_h, m.nc_add_w);
        cout << "done in " << now_s() - t << "s." << endl;
        if (m.eq_add > 0.0) add_vignette_LF(LF_noisy, mask, ang_major, aw, ah, m.eq_add);
        if (m.clip_add) clip_round_LF(LF_noisy, mask, m.clip_lo, m.clip_hi);
        if (m.smode == 5) clip_round_LF(LF_noisy, mask, m.pc_lo, m.pc_hi);   /* the given clipped model: the data are what it describes */
        if (m.imp_add > 0.0) add_impulses_LF(LF_noisy, mask, m.imp_add);
        for (size_t st = 0; st < m.missing.size(); st++) if (m.missing[st]) LF_noisy[st].assign(LF_noisy[st].size(), 0.0f);   /* dropped */
        cout << endl << "Save noisy light field..." << endl;
        if (save_LF(d_noisy, name, sep, LF_noisy, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return false;
    } else if (load_LF(d_noisy, name, sep, LF_noisy, mask, ang_major, aw, ah, s0, t0, W, H, C, m.missing.empty() ? nullptr : &m.missing) != EXIT_SUCCESS)
        return false;
    if (m.eq_mode && !equalise_noisy_LF(LF_noisy, mask, ang_major, aw, ah, W, H, C, m.dsteps, eq_gains)) return false;
    return !m.detect || detect_LF(LF_noisy, mask, m.det_k, m.det_save, name, sep, ang_major, aw, ah, s0, t0, W, H, C, m.missing, detected, m.dsteps);
}

/* what both commands run behind their repairs: LFBM5D_IMPULSE, then the sigma of LFBM5D_SIGMA=auto (est_mask: without the reconstructed SAIs) */
bool settle_noisy_LF(const Modes& m, vector<vector<float> >& LF_noisy, const vector<unsigned>& mask, const vector<unsigned>& est_mask, unsigned W,
                     unsigned H, unsigned C, float& sigma) {
    if (m.imp_k >= 0.0 && !repair_impulses_LF(LF_noisy, mask, W, H, C, m.imp_k)) return false;
    if (m.smode != 1) return true;
    return m.clip_on ? estimate_sigma_clipped_LF(LF_noisy, est_mask, W, H, C, m.clip_lo, m.clip_hi, sigma) : estimate_sigma_LF(LF_noisy, est_mask, W, H, C, sigma);
}

/* PSNR and RMSE (with LFBM5D_REPORT_SSIM: SSIM too) of a light field against the source: the averages into avg, say() prints what the command
 * says about them, the blocks go to the end of the results file.  false: the GPU backend failed (message on stdout) */
struct Quality {
    const vector<vector<float> >& source; const vector<unsigned>& mask; const char* results; unsigned ang_major, aw, ah, W, H, C; int ssim;
    template <class Say> bool report(const char* label, const vector<vector<float> >& LF_x, cli_quality::Avg& avg, Say say) const {
        vector<float> ps, rm; float sp = 0, ar = 0, sr = 0;
        cli_quality::Block qb;
        psnr_LF(source, LF_x, mask, ps, avg.psnr, sp, rm, ar, sr);
        if (ssim && !cli_quality::compute(source, LF_x, mask, W, H, C, avg, qb)) return false;
        say();
        write_psnr(results, label, mask, ang_major, aw, ah, ps, avg.psnr, sp, rm, ar, sr);
        if (ssim) cli_quality::write(results, label, mask, ang_major, aw, ah, qb);
        return true;
    }
};

} // namespace

#ifdef LFBM3D_CLI
int main(int argc, char** argv) {
    cout << "*********************************************************************************************************************" << endl;
    cout << "********************************************              START               ***************************************" << endl;
    cout << "*********************************************************************************************************************" << endl;
    if (argc < 32) {
        cout << "usage: " << argv[0] << " LFSourceDir|none SAIName sep awidth aheight sIdxStart tIdxStart aswSizeHard aswSizeWien row|col "
                "sigma lambda LFNoisyDir LFBasicDir LFDenoisedDir LFDiffDir NHard nHard kHard pHard dct|bior useSDHard "
                "NWien nWien kWien pWien dct|bior useSDWien rgb|yuv|ycbcr|opp nbThreads resultsFile" << endl;
        cout << "Problem while reading parameters from command line !" << endl;
        return EXIT_FAILURE;
    }
    int a = 1;
    const char* src = argv[a++]; const char* name = argv[a++]; const char* sep_in = argv[a++];
    const bool gt = strcmp(src, "none") != 0;
    const char* sep = strcmp(sep_in, "none") ? sep_in : "";
    if (!strcmp(name, "none")) name = "";
    const unsigned aw = atoi(argv[a++]), ah = atoi(argv[a++]), s0 = atoi(argv[a++]), t0 = atoi(argv[a++]);
    a += 2;   /* aswSizeHard, aswSizeWien: parsed by the reference, unused by BM3D */
    const char* maj = argv[a++];
    const unsigned ang_major = !strcmp(maj, "row") ? LFBM5D_ROWMAJOR : !strcmp(maj, "col") ? LFBM5D_COLMAJOR : 0;
    float sigma = (float)atof(argv[a++]);
    const float lambda = (float)atof(argv[a++]);
    const char* d_noisy = argv[a++]; const char* d_basic = argv[a++]; const char* d_den = argv[a++]; const char* d_diff = argv[a++];
    unsigned N[2], n[2], k[2], p[2], sd[2]; int t2[2];
    for (int i = 0; i < 2; i++) {
        N[i] = atoi(argv[a++]); n[i] = atoi(argv[a++]); k[i] = atoi(argv[a++]); p[i] = atoi(argv[a++]);
        const char* t = argv[a++];
        t2[i] = !strcmp(t, "dct") ? LFBM5D_DCT : !strcmp(t, "bior") ? LFBM5D_BIOR : -1;
        sd[i] = atoi(argv[a++]);
        if (t2[i] < 0) { cout << (i ? "tau_2d_wien" : "tau_2d_hard") << " is not known. Choice is :" << endl << " -dct" << endl << " -bior" << endl; return EXIT_FAILURE; }
    }
    const char* csn = argv[a++];
    const int cs = !strcmp(csn, "rgb") ? LFBM5D_RGB : !strcmp(csn, "yuv") ? LFBM5D_YUV : !strcmp(csn, "ycbcr") ? LFBM5D_YCBCR : !strcmp(csn, "opp") ? LFBM5D_OPP : -1;
    const unsigned nb_threads = atoi(argv[a++]);
    const char* results = argv[a++];
    if (!ang_major || cs < 0) { cout << "Problem while reading parameters from command line !" << endl; return EXIT_FAILURE; }
    Modes m;
    if (!read_modes(m, ang_major, aw, ah, s0, t0, gt, true)) return EXIT_FAILURE;
    unsigned pc_levels = 0; double pc_fmax = 0.0;   /* LFBM5D_SIGMA=poisson-clipped: its fit */
    vector<double> eq_gains;

    vector<vector<float> > LF, LF_noisy, LF_basic, LF_den, LF_diff;
    vector<unsigned> mask;
    unsigned W = 0, H = 0, C = 0;
    const unsigned awh = aw * ah;
    vector<vector<unsigned char> > detected;
    if (!noisy_LF(m, gt, src, d_noisy, name, sep, ang_major, aw, ah, s0, t0, sigma, LF, LF_noisy, mask, W, H, C, eq_gains, detected)) return EXIT_FAILURE;
    vector<unsigned> est_mask = mask;   /* the sigma estimate does not look at reconstructed SAIs */
    if (m.joint && (m.def_dir || !detected.empty() || !m.missing.empty())) {   /* one joint fill in place of the two below */
        vector<vector<unsigned char> > defects;
        const unsigned hard[9] = {8, 8, 3, 8, 3, 0, LFBM5D_DCT, LFBM5D_SADCT, LFBM5D_HAAR};
        if (!m.def_dir) defects.swap(detected);
        else if (!load_defects(m.def_dir, name, sep, defects, mask, ang_major, aw, ah, s0, t0, W, H, C)) return EXIT_FAILURE;
        if (!repair_joint_LF(LF_noisy, defects, mask, m.missing, ang_major, aw, ah, 1, W, H, C, 0, 0, 0.0f, lambda, hard, (unsigned)cs, true)) return EXIT_FAILURE;
        cout << "Joint repair: the fill alone (the refinement steps run in LFBM5Ddenoising)" << endl;
        for (size_t st = 0; st < m.missing.size(); st++) if (m.missing[st]) est_mask[st] = 0;
        m.missing.clear(); m.def_dir = nullptr; detected.clear();
    }
    if (!m.missing.empty()) {   /* the synthesis alone, for the same reason as the fill alone below */
        const unsigned hard[9] = {8, 8, 3, 8, 3, 0, LFBM5D_DCT, LFBM5D_SADCT, LFBM5D_HAAR};
        if (!synthesise_missing_LF(LF_noisy, mask, m.missing, ang_major, aw, ah, 1, W, H, C, 0, 0, 0.0f, lambda, hard, (unsigned)cs, true, m.dsteps, m.occl)) return EXIT_FAILURE;
        cout << "View synthesis: the synthesis alone (the refinement steps run in LFBM5Ddenoising)" << endl;
        for (size_t st = 0; st < m.missing.size(); st++) if (m.missing[st]) est_mask[st] = 0;
    }
    if (m.def_dir || !detected.empty()) {   /* the fill alone: the refinement loop needs the 5-D step's parameters, which this command does not have */
        vector<vector<unsigned char> > defects;
        const unsigned hard[9] = {8, 8, 3, 8, 3, 0, LFBM5D_DCT, LFBM5D_SADCT, LFBM5D_HAAR};
        if (!m.def_dir) defects.swap(detected);
        else if (!load_defects(m.def_dir, name, sep, defects, mask, ang_major, aw, ah, s0, t0, W, H, C)) return EXIT_FAILURE;
        if (!inpaint_defects_LF(LF_noisy, defects, mask, ang_major, aw, ah, 1, W, H, C, 0, 0, 0.0f, lambda, hard, (unsigned)cs, true)) return EXIT_FAILURE;
        cout << "Defect inpainting: the fill alone (the refinement steps run in LFBM5Ddenoising)" << endl;
    }
    if (!settle_noisy_LF(m, LF_noisy, mask, est_mask, W, H, C, sigma)) return EXIT_FAILURE;
    LF_basic.assign(awh, vector<float>((size_t)W * H * C, 0.0f));
    LF_den = LF_basic; LF_diff = LF_basic;
    cli_quality::Avg ap_n, ap_b, ap_d;
    const Quality quality = {LF, mask, results, ang_major, aw, ah, W, H, C, m.qmode};
    if (gt && !quality.report("noisy", LF_noisy, ap_n, [&]() { cout << endl << "Average PSNR:" << endl << "- Noisy light field: " << ap_n << endl; }))
        return EXIT_FAILURE;
    cout << endl << " ---> Running LFBM3D filter <--- " << endl << endl;
    const double tb = now_s();
    char sub[] = "SAI";
    if (m.smode >= 4) {   /* clipped Poisson-Gaussian noise: the same between the clipped model's stabiliser and its exact unbiased inverse */
        if (m.smode == 4 && pgclip_estimate_LF(LF_noisy, mask, W, H, C, m.pc_lo, m.pc_hi, m.pg[0], m.pg[1], pc_levels, pc_fmax) != EXIT_SUCCESS) return EXIT_FAILURE;
        vector<vector<float> > LF_t = LF_noisy;
        if (pgclip_forward_LF(m.pg[0], m.pg[1], m.pc_lo, m.pc_hi, LF_t, mask, W, H, C, sigma) != EXIT_SUCCESS) return EXIT_FAILURE;
        print_pgclip_model(m.smode == 4, m.pg, m.pc_lo, m.pc_hi, pc_levels, pc_fmax, sigma);
        if (run_bm3d_LF(sigma, LF_t, mask, LF_basic, LF_den, W, H, C, n[0], n[1], k[0], k[1], N[0], N[1], p[0], p[1], sd[0] != 0, sd[1] != 0,
                        t2[0], t2[1], lambda, cs, nb_threads, sub) != EXIT_SUCCESS) return EXIT_FAILURE;
        if (pgclip_inverse_LF(m.pg[0], m.pg[1], m.pc_lo, m.pc_hi, LF_basic, mask, W, H, C) != EXIT_SUCCESS ||
            pgclip_inverse_LF(m.pg[0], m.pg[1], m.pc_lo, m.pc_hi, LF_den, mask, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    } else
    if (m.smode >= 2) {   /* Poisson-Gaussian noise: stabilise a copy, filter it with the sigma that leaves, invert the results */
        if (m.smode == 2 && !estimate_pg_LF(LF_noisy, mask, W, H, C, m.pg)) return EXIT_FAILURE;
        vector<vector<float> > LF_t = LF_noisy;
        if (pg_forward_LF(m.pg[0], m.pg[1], LF_t, mask, W, H, C, sigma) != EXIT_SUCCESS) return EXIT_FAILURE;
        print_pg_model(m.smode == 2, m.pg, sigma);
        if (run_bm3d_LF(sigma, LF_t, mask, LF_basic, LF_den, W, H, C, n[0], n[1], k[0], k[1], N[0], N[1], p[0], p[1], sd[0] != 0, sd[1] != 0,
                        t2[0], t2[1], lambda, cs, nb_threads, sub) != EXIT_SUCCESS) return EXIT_FAILURE;
        if (pg_inverse_LF(m.pg[0], m.pg[1], LF_basic, mask, W, H, C) != EXIT_SUCCESS || pg_inverse_LF(m.pg[0], m.pg[1], LF_den, mask, W, H, C) != EXIT_SUCCESS)
            return EXIT_FAILURE;
    } else
    if (m.vs_mode) {   /* one noise level per SAI: every SAI is its own "window" */
        vector<double> table;
        if (m.vs_mode == 2 && views_from_gains((double)sigma, eq_gains, C, mask, table) != EXIT_SUCCESS) return EXIT_FAILURE;
        if (bm3d_views_LF(table, LF_noisy, mask, LF_basic, LF_den, W, H, C, n[0], n[1], k[0], k[1], N[0], N[1], p[0], p[1], sd[0] != 0, sd[1] != 0,
                          t2[0], t2[1], lambda, cs) != EXIT_SUCCESS) return EXIT_FAILURE;
        vector<float> each;
        for (size_t st = 0; st < table.size(); st++) if (mask[st]) each.push_back((float)table[st]);
        print_view_sigmas(table, mask, each, m.vs_mode == 1);
    } else
    if (run_bm3d_LF(sigma, LF_noisy, mask, LF_basic, LF_den, W, H, C, n[0], n[1], k[0], k[1], N[0], N[1], p[0], p[1], sd[0] != 0, sd[1] != 0,
                    t2[0], t2[1], lambda, cs, nb_threads, sub) != EXIT_SUCCESS) return EXIT_FAILURE;
    if (m.clip_on) {   /* the filter saw the clipped data; its results go through the inverse of the clipped mean */
        if (declip_LF(sigma, m.clip_lo, m.clip_hi, LF_basic, mask, W, H, C) != EXIT_SUCCESS || declip_LF(sigma, m.clip_lo, m.clip_hi, LF_den, mask, W, H, C) != EXIT_SUCCESS)
            return EXIT_FAILURE;
        print_declipping(m.clip_lo, m.clip_hi, sigma);
    }
    if (m.eq_mode == 1 && !(restore_LF(LF_basic, mask, eq_gains, aw, ah, W, H, C) && restore_LF(LF_den, mask, eq_gains, aw, ah, W, H, C))) return EXIT_FAILURE;
    const double secs = now_s() - tb;
    if (gt && !quality.report("basic", LF_basic, ap_b, []() {})) return EXIT_FAILURE;
    cout << endl << "Save basic light field..." << endl;
    if (save_LF(d_basic, name, sep, LF_basic, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    if (gt) {
        if (!quality.report("denoised", LF_den, ap_d, [&]() {
                cout << endl << "Average PSNR:" << endl << "- Noisy light field: " << ap_n << endl << "- Basic light field: " << ap_b << endl
                     << "- Denoised light field: " << ap_d << endl << endl; }))
            return EXIT_FAILURE;
        diff_LF(LF, LF_den, mask, LF_diff, sigma);
    }
    cout << endl << "Save denoised light field..." << endl;
    if (save_LF(d_den, name, sep, LF_den, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    if (gt) {
        cout << endl << "Save diff light field..." << endl;
        if (save_LF(d_diff, name, sep, LF_diff, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    }
    cout << "Total LFBM3D computing time = " << secs << "s." << endl << endl;
    cout << "*********************************************************************************************************************" << endl;
    cout << "********************************************         THIS IS THE END          ***************************************" << endl;
    cout << "*********************************************************************************************************************" << endl;
    return EXIT_SUCCESS;
}
#else
int main(int argc, char** argv) {
    cout << "*********************************************************************************************************************" << endl;
    cout << "********************************************              START               ***************************************" << endl;
    cout << "*********************************************************************************************************************" << endl;
    if (argc == 4 && !strcmp(argv[1], "--png-roundtrip")) { /* codec self-check (no GPU): read, rewrite */
        vector<float> img; size_t w, h, c;
        if (!png_read_planar_f32(argv[2], img, w, h, c)) { cout << "cannot read " << argv[2] << endl; return EXIT_FAILURE; }
        if (c == 2) c = 1;
        if (c == 4) c = 3;
        return png_write_planar_f32(argv[3], img.data(), w, h, c) ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    if (argc < 38) { usage(argv[0]); cout << "Problem while reading parameters from command line !" << endl; return EXIT_FAILURE; }
    int a = 1;
    const char* src = argv[a++]; const char* name = argv[a++]; const char* sep_in = argv[a++];
    const bool gt = strcmp(src, "none") != 0;
    const char* sep = strcmp(sep_in, "none") ? sep_in : "";
    if (!strcmp(name, "none")) name = "";
    const unsigned aw = atoi(argv[a++]), ah = atoi(argv[a++]), s0 = atoi(argv[a++]), t0 = atoi(argv[a++]);
    const unsigned anH = atoi(argv[a++]), anW = atoi(argv[a++]);
    const char* maj = argv[a++];
    const unsigned ang_major = !strcmp(maj, "row") ? LFBM5D_ROWMAJOR : !strcmp(maj, "col") ? LFBM5D_COLMAJOR : 0;
    float sigma = (float)atof(argv[a++]);
    const float lambda = (float)atof(argv[a++]);
    const char* d_noisy = argv[a++]; const char* d_basic = argv[a++]; const char* d_den = argv[a++]; const char* d_diff = argv[a++];
    unsigned N[2], nSim[2], nDisp[2], k[2], p[2], sd[2]; int t2[2], t4[2], t5[2];
    for (int i = 0; i < 2; i++) {
        N[i] = atoi(argv[a++]); nSim[i] = atoi(argv[a++]); nDisp[i] = atoi(argv[a++]); k[i] = atoi(argv[a++]); p[i] = atoi(argv[a++]);
        t2[i] = tau(argv[a++], 2); t4[i] = tau(argv[a++], 4); t5[i] = tau(argv[a++], 5); sd[i] = atoi(argv[a++]);
        if (t2[i] < 0 || t4[i] < 0 || t5[i] < 0) { cout << "unknown transform name" << endl; usage(argv[0]); return EXIT_FAILURE; }
    }
    const char* csn = argv[a++];
    const int cs = !strcmp(csn, "rgb") ? LFBM5D_RGB : !strcmp(csn, "yuv") ? LFBM5D_YUV : !strcmp(csn, "ycbcr") ? LFBM5D_YCBCR : !strcmp(csn, "opp") ? LFBM5D_OPP : -1;
    const unsigned nb_threads = atoi(argv[a++]);
    const char* results = argv[a++];
    if (!ang_major || cs < 0) { cout << "Problem while reading parameters from command line !" << endl; usage(argv[0]); return EXIT_FAILURE; }
    Modes m;
    if (!read_modes(m, ang_major, aw, ah, s0, t0, gt, false)) return EXIT_FAILURE;
    unsigned pc_levels = 0; double pc_fmax = 0.0;   /* LFBM5D_SIGMA=poisson-clipped: its fit */
    vector<double> eq_gains;

    vector<vector<float> > LF, LF_noisy, LF_basic, LF_den, LF_diff;
    vector<unsigned> mask;
    unsigned W = 0, H = 0, C = 0;
    const unsigned awh = aw * ah;
    vector<vector<unsigned char> > defects;
    if (!noisy_LF(m, gt, src, d_noisy, name, sep, ang_major, aw, ah, s0, t0, sigma, LF, LF_noisy, mask, W, H, C, eq_gains, defects)) return EXIT_FAILURE;
    const unsigned def_hard[9] = {N[0], nSim[0], nDisp[0], k[0], p[0], sd[0], (unsigned)t2[0], (unsigned)t4[0], (unsigned)t5[0]};
    unsigned def_steps = 0;
    vector<unsigned> est_mask = mask;   /* the sigma estimate does not look at reconstructed SAIs */
    unsigned view_steps = 0;
    unsigned rep_steps = 0;
    const bool joint_job = m.joint && (m.def_dir || !defects.empty() || !m.missing.empty());
    if (joint_job) {   /* one joint fill now, one loop behind the sigma estimate, in place of the two stages below */
        lfbm5d_repair_params rp;
        lfbm5d_repair_defaults(&rp);
        rep_steps = m.rep_iter >= 0 ? (unsigned)m.rep_iter : rp.iterations;
        if (m.def_dir && !load_defects(m.def_dir, name, sep, defects, mask, ang_major, aw, ah, s0, t0, W, H, C)) return EXIT_FAILURE;
        if (!repair_joint_LF(LF_noisy, defects, mask, m.missing, ang_major, aw, ah, anH, W, H, C, 0, rep_steps, 0.0f, lambda, def_hard, (unsigned)cs, true))
            return EXIT_FAILURE;
        for (size_t st = 0; st < m.missing.size(); st++) if (m.missing[st]) est_mask[st] = 0;
    }
    const bool have_defects = !joint_job && (m.def_dir || !defects.empty());
    if (!joint_job && !m.missing.empty()) {
        lfbm5d_view_params vp;
        lfbm5d_view_defaults(&vp);
        view_steps = m.smode >= 2 ? 0u : m.miss_iter >= 0 ? (unsigned)m.miss_iter : vp.iterations;
        if (!synthesise_missing_LF(LF_noisy, mask, m.missing, ang_major, aw, ah, anH, W, H, C, 0, view_steps, 0.0f, lambda, def_hard, (unsigned)cs, true, m.dsteps, m.occl))
            return EXIT_FAILURE;
        if (m.smode >= 2) cout << "View synthesis: the synthesis alone (LFBM5D_SIGMA=poisson: the refinement steps assume one sigma)" << endl;
        for (size_t st = 0; st < m.missing.size(); st++) if (m.missing[st]) est_mask[st] = 0;
    }
    if (have_defects) {
        lfbm5d_inpaint_params ip;
        lfbm5d_inpaint_defaults(&ip);
        def_steps = m.smode >= 2 ? 0u : m.def_iter >= 0 ? (unsigned)m.def_iter : ip.iterations;
        if (m.def_dir && !load_defects(m.def_dir, name, sep, defects, mask, ang_major, aw, ah, s0, t0, W, H, C)) return EXIT_FAILURE;
        if (!inpaint_defects_LF(LF_noisy, defects, mask, ang_major, aw, ah, anH, W, H, C, 0, def_steps, 0.0f, lambda, def_hard, (unsigned)cs, true))
            return EXIT_FAILURE;
        if (m.smode >= 2) cout << "Defect inpainting: the fill alone (LFBM5D_SIGMA=poisson: the refinement steps assume one sigma)" << endl;
    }
    if (!settle_noisy_LF(m, LF_noisy, mask, est_mask, W, H, C, sigma)) return EXIT_FAILURE;
    if (rep_steps && !repair_joint_LF(LF_noisy, defects, mask, m.missing, ang_major, aw, ah, anH, W, H, C, rep_steps, rep_steps, sigma, lambda, def_hard,
                                      (unsigned)cs, false)) return EXIT_FAILURE;
    if (view_steps && !synthesise_missing_LF(LF_noisy, mask, m.missing, ang_major, aw, ah, anH, W, H, C, view_steps, view_steps, sigma, lambda, def_hard,
                                             (unsigned)cs, false, m.dsteps, m.occl)) return EXIT_FAILURE;
    if (def_steps && !inpaint_defects_LF(LF_noisy, defects, mask, ang_major, aw, ah, anH, W, H, C, def_steps, def_steps, sigma, lambda, def_hard,
                                         (unsigned)cs, false)) return EXIT_FAILURE;
    LF_basic.assign(awh, vector<float>((size_t)W * H * C, 0.0f));
    LF_den = LF_basic; LF_diff = LF_basic;
    cli_quality::Avg ap_n, ap_b, ap_d;
    const Quality quality = {LF, mask, results, ang_major, aw, ah, W, H, C, m.qmode};
    if (gt && !quality.report("noisy", LF_noisy, ap_n, [&]() { cout << endl << "Average PSNR:" << endl << "- Noisy light field: " << ap_n << endl; }))
        return EXIT_FAILURE;
    /* LFBM5D_ONE_JOB=1 (not in the reference): both steps as one job (run_bm5d, run_bm5d.h) -- the same denoised files and PSNR, one time for
     * both.  The BASIC light field saved and reported in this mode is the one the job returns at its end, inverse(forward(inverse(estimate)))
     * -- what LF_basic holds after run_bm5d_2nd_step's lossy colour round trip (bm5d.cpp:829, :1416) -- where the two-call form saves
     * inverse(estimate) between the calls: the two differ (0.015 dB on the test light field) because the reference's colour matrices are not
     * inverses of each other */
    const char* one_job_s = env("LFBM5D_ONE_JOB");
    const bool one_job = m.smode >= 2 || m.clip_on || m.vs_mode || m.nc_mode || (one_job_s && *one_job_s && *one_job_s != '0');   /* the Poisson-Gaussian, the clipped and the per-view path are one job */
    cout << endl << " ---> Running LFBM5D filter <--- " << endl << endl << (one_job ? "Steps 1 and 2 running as one job..." : "Step 1 running...") << endl;
    const double tb = now_s();
    double t1 = now_s();
    double job = 0.0;
    if (m.smode >= 4) {
        if (denoise_pgclip_LF(m.pg[0], m.pg[1], m.pc_lo, m.pc_hi, m.smode == 4, sigma, pc_levels, pc_fmax, lambda, LF_noisy, mask, LF_basic, LF_den, ang_major, aw,
                              ah, anH, anW, W, H, C, N[0], nSim[0], nDisp[0], k[0], p[0], sd[0] != 0, t2[0], t4[0], t5[0], N[1], nSim[1], nDisp[1], k[1],
                              p[1], sd[1] != 0, t2[1], t4[1], t5[1], cs, nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
        job = now_s() - t1;
        print_pgclip_model(m.smode == 4, m.pg, m.pc_lo, m.pc_hi, pc_levels, pc_fmax, sigma);
    } else if (m.smode >= 2) {
        if (denoise_pg_LF(m.pg[0], m.pg[1], m.smode == 2, sigma, lambda, LF_noisy, mask, LF_basic, LF_den, ang_major, aw, ah, anH, anW, W, H, C, N[0],
                          nSim[0], nDisp[0], k[0], p[0], sd[0] != 0, t2[0], t4[0], t5[0], N[1], nSim[1], nDisp[1], k[1], p[1], sd[1] != 0, t2[1],
                          t4[1], t5[1], cs, nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
        job = now_s() - t1;
        print_pg_model(m.smode == 2, m.pg, sigma);
    } else if (m.clip_on) {
        if (denoise_clipped_LF(sigma, m.clip_lo, m.clip_hi, lambda, LF_noisy, mask, LF_basic, LF_den, ang_major, aw, ah, anH, anW, W, H, C, N[0], nSim[0], nDisp[0],
                               k[0], p[0], sd[0] != 0, t2[0], t4[0], t5[0], N[1], nSim[1], nDisp[1], k[1], p[1], sd[1] != 0, t2[1], t4[1], t5[1], cs,
                               nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
        job = now_s() - t1;
        print_declipping(m.clip_lo, m.clip_hi, sigma);
    } else if (m.vs_mode) {
        vector<double> table; vector<float> window_sigmas;
        if (m.vs_mode == 2 && views_from_gains((double)sigma, eq_gains, C, mask, table) != EXIT_SUCCESS) return EXIT_FAILURE;
        if (denoise_views_LF(table, window_sigmas, lambda, LF_noisy, mask, LF_basic, LF_den, ang_major, aw, ah, anH, anW, W, H, C, N[0], nSim[0],
                             nDisp[0], k[0], p[0], sd[0] != 0, t2[0], t4[0], t5[0], N[1], nSim[1], nDisp[1], k[1], p[1], sd[1] != 0, t2[1], t4[1],
                             t5[1], cs, nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
        job = now_s() - t1;
        print_view_sigmas(table, mask, window_sigmas, m.vs_mode == 1);
    } else if (m.nc_mode) {
        if (m.nc_mode == 1) {   /* the blind shape from the noisy light field; the command's sigma stays the marginal level */
            double s_est = 0.0;
            if (corr_measure_LF(LF_noisy, mask, W, H, C, 0, 0.0, m.nc_acf, s_est) != EXIT_SUCCESS) return EXIT_FAILURE;
        }
        if (denoise_corr_LF(m.nc_acf, sigma, lambda, LF_noisy, mask, LF_basic, LF_den, ang_major, aw, ah, anH, anW, W, H, C, N[0], nSim[0], nDisp[0],
                            k[0], p[0], sd[0] != 0, t2[0], t4[0], t5[0], N[1], nSim[1], nDisp[1], k[1], p[1], sd[1] != 0, t2[1], t4[1], t5[1], cs,
                            nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
        job = now_s() - t1;
        if (!print_noise_corr(m.nc_acf, m.nc_mode, t2, k)) return EXIT_FAILURE;
    } else if (one_job) {
        if (run_bm5d(sigma, lambda, LF_noisy, mask, LF_basic, LF_den, ang_major, aw, ah, anH, anW, W, H, C, N[0], nSim[0], nDisp[0], k[0], p[0],
                     sd[0] != 0, t2[0], t4[0], t5[0], N[1], nSim[1], nDisp[1], k[1], p[1], sd[1] != 0, t2[1], t4[1], t5[1], cs, nb_threads) != EXIT_SUCCESS)
            return EXIT_FAILURE;
        job = now_s() - t1;
    } else
    if (run_bm5d_1st_step(sigma, lambda, LF_noisy, mask, LF_basic, ang_major, aw, ah, anH, W, H, C, N[0], nSim[0], nDisp[0], k[0], p[0],
                          sd[0] != 0, t2[0], t4[0], t5[0], cs, nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
    const double step1 = one_job ? job : now_s() - t1;
    if (one_job) cout << endl << "Steps 1 and 2 done in " << job << " secs." << endl << endl;
    else cout << endl << "Step 1 done in " << step1 << " secs." << endl << endl;
    vector<vector<float> > LF_basic_eq;   /* LFBM5D_EQUALISE=auto: step 2 reads the equalised basic estimate, the file gets the restored one */
    if (m.eq_mode == 1) {
        LF_basic_eq = LF_basic;
        if (!restore_LF(LF_basic, mask, eq_gains, aw, ah, W, H, C)) return EXIT_FAILURE;
        if (one_job && !restore_LF(LF_den, mask, eq_gains, aw, ah, W, H, C)) return EXIT_FAILURE;
    }
    if (gt) {
        if (!quality.report("basic", LF_basic, ap_b, [&]() {
                cout << endl << "Average PSNR:" << endl << "- Noisy light field: " << ap_n << endl << "- Basic light field: " << ap_b << endl; }))
            return EXIT_FAILURE;
        diff_LF(LF, LF_basic, mask, LF_diff, sigma);
    }
    cout << endl << "Save basic light field..." << endl;
    if (save_LF(d_basic, name, sep, LF_basic, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    if (!one_job) cout << endl << endl << "Step 2 running..." << endl;
    t1 = now_s();
    if (m.eq_mode == 1 && !one_job) LF_basic.swap(LF_basic_eq);
    if (!one_job && run_bm5d_2nd_step(sigma, LF_noisy, mask, LF_basic, LF_den, ang_major, aw, ah, anW, W, H, C, N[1], nSim[1], nDisp[1], k[1], p[1],
                          sd[1] != 0, t2[1], t4[1], t5[1], cs, nb_threads) != EXIT_SUCCESS) return EXIT_FAILURE;
    const double step2 = one_job ? 0.0 : now_s() - t1;
    if (!one_job) cout << endl << "Step 2 done in " << step2 << " secs." << endl << endl;
    if (m.eq_mode == 1 && !one_job && !restore_LF(LF_den, mask, eq_gains, aw, ah, W, H, C)) return EXIT_FAILURE;
    if (gt) {
        if (!quality.report("denoised", LF_den, ap_d, [&]() {
                cout << endl << "Average PSNR:" << endl << "- Noisy light field: " << ap_n << endl << "- Basic light field: " << ap_b << endl
                     << "- Denoised light field: " << ap_d << endl << endl; }))
            return EXIT_FAILURE;
        diff_LF(LF, LF_den, mask, LF_diff, sigma);
    }
    cout << endl << "Save denoised light field..." << endl;
    if (save_LF(d_den, name, sep, LF_den, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    if (gt) {
        cout << endl << "Save diff light field..." << endl;
        if (save_LF(d_diff, name, sep, LF_diff, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    }
    cout << "Total LFBM5D computing time = " << step1 + step2 << "s." << endl;
    cout << "Total elapsed time = " << now_s() - tb << "s." << endl << endl;
    cout << "*********************************************************************************************************************" << endl;
    cout << "********************************************         THIS IS THE END          ***************************************" << endl;
    cout << "*********************************************************************************************************************" << endl;
    return EXIT_SUCCESS;
}
#endif
