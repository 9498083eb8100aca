"""ctypes binding of liblfbm5d_hip.so (include/lfbm5d.h) and the reference-named wrappers.

Device buffers are torch CUDA tensors (torch is plumbing for HBM allocations and, in bench.py,
torch.distributed for the rendezvous); the C-ABI itself only sees raw pointers.
"""
import ctypes as C
import os
import subprocess

from typing import NamedTuple, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

# enum ints of the reference (src/bm5d.cpp:36-48)
YUV, YCBCR, OPP, RGB, ID, DCT, SADCT, BIOR, HADAMARD, HAAR = range(10)
ROWMAJOR, COLMAJOR = 11, 12
TAU = {"id": ID, "dct": DCT, "sadct": SADCT, "bior": BIOR, "hw": HADAMARD, "haar": HAAR}
COLOR_SPACE = {"yuv": YUV, "ycbcr": YCBCR, "opp": OPP, "rgb": RGB}
UNIQUE_ID_BYTES = 128
SR_BICUBIC, SR_GAUSSIAN = 0, 1
SR_UP, SR_DOWN = 0, 1
SR_KERNEL = {"bicubic": SR_BICUBIC, "gaussian": SR_GAUSSIAN}


class LfBm5dError(RuntimeError):
    pass


class Params(C.Structure):
    """lfbm5d_params: the parameter tail of run_bm5d_*_step (bm5d.h:11-62)."""
    _fields_ = [("sigma", C.c_float), ("lambda_", C.c_float), ("N", C.c_uint), ("nSim", C.c_uint),
                ("nDisp", C.c_uint), ("k", C.c_uint), ("p", C.c_uint), ("useSD", C.c_uint),
                ("tau_2D", C.c_uint), ("tau_4D", C.c_uint), ("tau_5D", C.c_uint),
                ("color_space", C.c_uint)]


class Bm3dParams(C.Structure):
    """lfbm5d_bm3d_params: one step's parameters of run_bm3d (src/bm3d.h:11-34)."""
    _fields_ = [("sigma", C.c_float), ("lambda3D", C.c_float), ("N", C.c_uint), ("nHW", C.c_uint), ("k", C.c_uint),
                ("p", C.c_uint), ("useSD", C.c_uint), ("tau_2D", C.c_uint), ("color_space", C.c_uint)]


class Stats(C.Structure):
    _fields_ = [("windows", C.c_ulonglong), ("passes", C.c_ulonglong), ("groups", C.c_ulonglong),
                ("stack_patches", C.c_ulonglong), ("sadct_groups", C.c_ulonglong),
                ("algorithmic_bytes", C.c_double), ("ms_bm", C.c_double), ("ms_group", C.c_double),
                ("ms_aggregate", C.c_double), ("ms_other", C.c_double), ("ms_comm", C.c_double),
                ("launches_group", C.c_ulonglong), ("launches_aggregate", C.c_ulonglong),
                ("lane_windows", C.c_ulonglong), ("messages", C.c_ulonglong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AggDebugStruct(C.Structure):
    """lfbm5d_agg_debug: the aggregation launch of a core pass on buffers the caller supplies (include/lfbm5d.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("num", "den", "filt", "wgt", "aggpos", "mask", "proc", "sai")]
                + [(n, C.c_ulonglong) for n in ("filt_sai_stride", "filt_bytes", "lf_stride", "sums_floats", "wgt_floats", "aggpos_words")]
                + [(n, C.c_uint) for n in ("n_refs_total", "ref_begin", "n_groups", "n_ref_rows", "n_ref_cols", "Wb", "Hb", "C", "A", "k",
                                           "N", "pst", "p", "nSim", "nDisp", "irregular", "wchan0", "direct")])


class GroupDebugStruct(C.Structure):
    """lfbm5d_group_debug: the group launch of a core pass on tables and buffers the caller supplies (include/lfbm5d.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("noisy", "basic", "refs", "self_idx", "self_cnt", "best", "shape", "filt", "wgt", "aggpos",
                                           "counters", "mask", "params", "kernels")]
                + [(n, C.c_ulonglong) for n in ("filt_sai_stride", "image_floats", "table_words", "filt_floats", "wgt_floats",
                                                "aggpos_words", "kernels_cap")]
                + [(n, C.c_uint) for n in ("step", "aw", "ah", "Wb", "Hb", "C", "pst", "fill_quirk", "n_refs_total", "ref_begin",
                                           "n_groups", "bm3d")])


WINDOW_OPS = ("color", "color_roundtrip", "symetrize", "crop", "symetrize_multi", "unsymetrize_multi", "estimate", "estimate_multi",
              "estimate_lf", "window_begin", "window_end", "finalize", "output", "count_zeros", "count_denoised", "copy_rect", "copy_rows")
_WINDOW_LF = ("noisy", "basic", "num", "den", "sub", "out", "noisy_dst")   # the light-field side of lfbm5d_window_debug
_WINDOW_W = ("w_noisy", "w_basic", "w_num", "w_den")                        # ... and the window side


class WindowDebugStruct(C.Structure):
    """lfbm5d_window_debug: one launcher of the window-schedule kernels on buffers the caller supplies (include/lfbm5d.h)."""
    _fields_ = ([(n, C.c_void_p) for n in _WINDOW_LF + _WINDOW_W + ("est", "counters", "dmask", "list", "slot_mask")]
                + [(n, C.c_ulonglong) for n in ("lf_stride", "w_stride", "lf_floats", "w_floats", "est_floats", "n")]
                + [(n, C.c_uint) for n in ("op", "W", "H", "C", "N", "k", "off", "cs", "forward", "colour", "n_sai", "n_list", "sW", "sH",
                                           "sx0", "sy0", "dx0", "dy0", "rw", "rh", "counter_words", "dmask_words")])


class NoiseLevelStruct(C.Structure):
    """lfbm5d_noise_level: the blind noise-level estimate (include/lfbm5d.h)."""
    _fields_ = [("sigma", C.c_double), ("sigma_channel", C.c_double * 3), ("components", C.c_uint), ("patch", C.c_uint),
                ("patches", C.c_ulonglong)]


class QualityStruct(C.Structure):
    """lfbm5d_quality: the summary of the quality metrics (include/lfbm5d.h)."""
    _fields_ = [("psnr_mean", C.c_double), ("psnr_std", C.c_double), ("rmse_mean", C.c_double), ("rmse_std", C.c_double),
                ("ssim_mean", C.c_double), ("ssim_std", C.c_double), ("mse", C.c_double), ("count", C.c_uint), ("has_ssim", C.c_uint)]


class SrParams(C.Structure):
    """lfbm5d_sr_params: operators and loop of the super-resolution (include/lfbm5d.h)."""
    _fields_ = [("scale", C.c_uint), ("kernel", C.c_uint), ("blur_sigma", C.c_float), ("iterations", C.c_uint),
                ("sigma_start", C.c_float), ("sigma_end", C.c_float), ("beta", C.c_float), ("close_projection", C.c_uint)]


class PgModelStruct(C.Structure):
    """lfbm5d_pg_model: a, b of var(z | y) = a y + b per stored channel (include/lfbm5d.h)."""
    _fields_ = [("a", C.c_double * 3), ("b", C.c_double * 3)]


class PgEstimateStruct(C.Structure):
    """lfbm5d_pg_estimate: the fitted Poisson-Gaussian models of a light field (include/lfbm5d.h)."""
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("a_channel", C.c_double * 3), ("b_channel", C.c_double * 3),
                ("blocks", C.c_ulonglong), ("skipped", C.c_ulonglong)]


PG_LEVELS, PG_KEYS = 64, 322


class ClipEstimateStruct(C.Structure):
    """lfbm5d_clip_estimate: the clipping-aware noise level of a light field (include/lfbm5d.h)."""
    _fields_ = [("sigma", C.c_double), ("sigma_channel", C.c_double * 3), ("f_max", C.c_double), ("censored", C.c_double),
                ("levels", C.c_uint), ("heavily_clipped", C.c_uint), ("quantised", C.c_uint), ("reserved", C.c_uint),
                ("blocks", C.c_ulonglong), ("skipped", C.c_ulonglong)]


PGCLIP_KNOTS = 4097


class PgclipModelStruct(C.Structure):
    """lfbm5d_pgclip_model: sigma^2(y) = max(a (y - lo) + b, 1/12) on data clipped to lo..hi (include/lfbm5d_pgclip.h)."""
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("lo", C.c_double), ("hi", C.c_double)]


class PgclipEstimateStruct(C.Structure):
    """lfbm5d_pgclip_estimate: the censored fit of the clipped Poisson-Gaussian model (include/lfbm5d_pgclip.h)."""
    _fields_ = [("model", PgclipModelStruct), ("a_channel", C.c_double * 3), ("b_channel", C.c_double * 3), ("f_max", C.c_double),
                ("censored", C.c_double), ("levels", C.c_uint), ("heavily_clipped", C.c_uint), ("quantised", C.c_uint),
                ("reserved", C.c_uint), ("blocks", C.c_ulonglong), ("skipped", C.c_ulonglong)]


class PgclipCurvesStruct(C.Structure):
    """lfbm5d_pgclip_curves: the stabiliser and its exact unbiased inverse as tables (include/lfbm5d_pgclip.h)."""
    _fields_ = [("model", PgclipModelStruct), ("s", C.c_double), ("fwd_x0", C.c_double), ("fwd_dx", C.c_double),
                ("inv_x0", C.c_double), ("inv_dx", C.c_double), ("fwd", C.c_float * PGCLIP_KNOTS), ("inv", C.c_float * PGCLIP_KNOTS)]


class ImpulseParamsStruct(C.Structure):
    """lfbm5d_impulse_params: threshold factor, floor and given thresholds of the impulse repair (include/lfbm5d.h)."""
    _fields_ = [("k", C.c_double), ("min_threshold", C.c_double), ("threshold", C.c_double * 3)]


class ImpulseResultStruct(C.Structure):
    """lfbm5d_impulse_result: scales, thresholds and counts of one impulse repair (include/lfbm5d.h)."""
    _fields_ = [("scale", C.c_double), ("scale_channel", C.c_double * 3), ("threshold", C.c_double * 3),
                ("flagged", C.c_ulonglong * 3), ("repaired", C.c_ulonglong * 3), ("left", C.c_ulonglong * 3),
                ("pixels", C.c_ulonglong), ("skipped", C.c_ulonglong)]


IMPULSE_KEYS = 386
VIEW_STEPS_HIST = 65    # LFBM5D_VIEW_STEPS_HIST: positions per j*, index j* + 32


class InpaintParamsStruct(C.Structure):
    """lfbm5d_inpaint_params: refinement steps and sigma schedule of the defect inpainting (include/lfbm5d.h)."""
    _fields_ = [("iterations", C.c_uint), ("sigma_start", C.c_float), ("sigma_end", C.c_float), ("sigma_noise", C.c_float)]


class InpaintResultStruct(C.Structure):
    """lfbm5d_inpaint_result: counts of one fill (include/lfbm5d.h)."""
    _fields_ = [("flagged", C.c_ulonglong * 3), ("filled", C.c_ulonglong * 3), ("left", C.c_ulonglong * 3), ("pixels", C.c_ulonglong),
                ("passes", C.c_uint), ("launches", C.c_uint)]


INPAINT_PASSES_PER_LAUNCH = 8


class ViewParamsStruct(C.Structure):
    """lfbm5d_view_params: hypotheses, box, sources and the refinement schedule of the view synthesis (include/lfbm5d.h)."""
    _fields_ = [("max_disparity", C.c_uint), ("box_radius", C.c_uint), ("ang_radius", C.c_uint), ("iterations", C.c_uint),
                ("sigma_start", C.c_float), ("sigma_end", C.c_float), ("sigma_noise", C.c_float)]


class ViewResultStruct(C.Structure):
    """lfbm5d_view_result: counts of one synthesis (include/lfbm5d.h)."""
    _fields_ = [("missing", C.c_uint), ("synthesised", C.c_uint), ("left", C.c_uint), ("pixels", C.c_ulonglong),
                ("disparity_hist", C.c_ulonglong * 17)]


class RepairParamsStruct(C.Structure):
    """lfbm5d_repair_params: the mask-aware sweep, min_valid and the refinement schedule of the joint repair (include/lfbm5d_repair.h)."""
    _fields_ = [("max_disparity", C.c_uint), ("box_radius", C.c_uint), ("ang_radius", C.c_uint), ("min_valid", C.c_uint),
                ("iterations", C.c_uint), ("sigma_start", C.c_float), ("sigma_end", C.c_float), ("sigma_noise", C.c_float)]


class RepairResultStruct(C.Structure):
    """lfbm5d_repair_result: counts of one joint fill (include/lfbm5d_repair.h)."""
    _fields_ = [("missing", C.c_uint), ("targets", C.c_uint), ("swept", C.c_uint), ("passes", C.c_uint), ("values", C.c_ulonglong),
                ("flagged", C.c_ulonglong), ("unsound", C.c_ulonglong * 3), ("views", C.c_ulonglong * 3), ("rim", C.c_ulonglong * 3),
                ("left", C.c_ulonglong * 3), ("positions", C.c_ulonglong), ("disparity_hist", C.c_ulonglong * 17)]


class ViewOcclResultStruct(C.Structure):
    """lfbm5d_view_occl_result: positions per set chosen by the occlusion-aware synthesis (include/lfbm5d_occl.h)."""
    _fields_ = [("set_hist", C.c_ulonglong * 5)]


class ConsistParamsStruct(C.Structure):
    """lfbm5d_consist_params: the sweep, the two pixel tests and the bad-SAI decision of the consistency check (include/lfbm5d.h)."""
    _fields_ = [("max_disparity", C.c_uint), ("box_radius", C.c_uint), ("ang_radius", C.c_uint), ("min_sources", C.c_uint),
                ("max_rounds", C.c_uint), ("k", C.c_double), ("min_threshold", C.c_double), ("spread", C.c_double),
                ("sai_factor", C.c_double), ("min_scale", C.c_double)]


class ConsistResultStruct(C.Structure):
    """lfbm5d_consist_result: scales, thresholds and counts of one consistency check (include/lfbm5d.h)."""
    _fields_ = [("scale_channel", C.c_double * 3), ("threshold", C.c_double * 3), ("flagged", (C.c_ulonglong * 2) * 3),
                ("pixels", C.c_ulonglong), ("skipped", C.c_ulonglong), ("bad", C.c_uint), ("untested", C.c_uint), ("tested", C.c_uint),
                ("rounds", C.c_uint)]


CONSIST_EMPTY, CONSIST_TESTED, CONSIST_BAD, CONSIST_UNTESTED, CONSIST_EXCLUDED = 0, 1, 2, 3, 4


class Consist(NamedTuple):
    """Result of Context.consist / consist: the flag planes (uint8 like the input: 0 sound, 1 inconsistent with the other views, 2 not
    finite; a tensor or an array like the input), the state of every SAI (int64 [asize]: 0 empty, 1 tested, 2 bad, 3 untested,
    4 excluded), the disparity planes (int8 [asize][H*W], written for tested SAIs; None unless asked for), the median |residual| per
    stored channel and the float32 thresholds, s_m per SAI (float64 [asize]), the histograms (uint64 [asize][C][386]), the counts per
    stored channel of code 1 and of code 2, the indices of the bad and of the untested SAIs, the sweeps, the values of the tested SAIs
    and how many of them are not finite."""
    flags: object
    state: object
    disparity: object
    scale_channel: tuple
    threshold: tuple
    scale_sai: object
    hist: object
    flagged: tuple
    nonfinite: tuple
    bad: tuple
    untested: tuple
    rounds: int
    pixels: int
    skipped: int

    @property
    def missing(self):
        """uint32 [asize], 1 on the bad SAIs: the `missing` argument of view_synth."""
        return (np.asarray(self.state) == CONSIST_BAD).astype(np.uint32)


class PhotoParamsStruct(C.Structure):
    """lfbm5d_photo_params: the sweep, the admission range, the fit and the rounds of the photometric equalisation
    (include/lfbm5d_photo.h)."""
    _fields_ = [("max_disparity", C.c_uint), ("box_radius", C.c_uint), ("ang_radius", C.c_uint), ("steps", C.c_uint),
                ("min_sources", C.c_uint), ("max_rounds", C.c_uint), ("per_channel", C.c_uint), ("anchor", C.c_uint),
                ("min_count", C.c_ulonglong), ("tol", C.c_double), ("lo", C.c_double), ("hi", C.c_double)]


class PhotoResultStruct(C.Structure):
    """lfbm5d_photo_result: what one photometric equalisation found (include/lfbm5d_photo.h)."""
    _fields_ = [("residual", C.c_double), ("gain_min", C.c_double), ("gain_max", C.c_double), ("admitted", C.c_ulonglong),
                ("skipped_nonfinite", C.c_ulonglong), ("skipped_range", C.c_ulonglong), ("rounds", C.c_uint), ("converged", C.c_uint),
                ("fitted", C.c_uint), ("untested", C.c_uint), ("unfit", C.c_uint)]


PHOTO_KEYS, PHOTO_EDGES, PHOTO_NO_ANCHOR, PHOTO_MAX_SOURCES = 1026, 1025, 0xFFFFFFFF, 24
PHOTO_EMPTY, PHOTO_FITTED, PHOTO_UNTESTED, PHOTO_UNFIT = 0, 1, 2, 3


class Equalise(NamedTuple):
    """Result of Context.equalise / equalise: the equalised light field (a tensor or an array like the input; planes of empty SAIs are
    the input's), the gains G that were divided out (float64 [asize][3]; 1 for empty SAIs and channels that are not stored: hand them
    to apply_gains(..., invert=True) to restore every view's own photometry), the state of every SAI (int64 [asize]: 0 empty,
    1 fitted, 2 untested, 3 unfit in some channel), the last sweep's histograms (uint64 [asize][C][1026]; None unless asked for), the
    sweeps, whether the last sweep's ratios were within tol of 1, that sweep's largest |ratio - 1|, the smallest and the largest gain,
    the numbers of fitted, untested and unfit SAIs, and the values the last sweep counted, found not finite and found out of range."""
    out: object
    gain: np.ndarray
    state: np.ndarray
    hist: object
    rounds: int
    converged: bool
    residual: float
    gain_min: float
    gain_max: float
    fitted: int
    untested: int
    unfit: int
    admitted: int
    skipped_nonfinite: int
    skipped_range: int


class ViewSynth(NamedTuple):
    """Result of Context.view_fill / Context.view_synth / view_synth: the light field with the missing SAIs reconstructed (a tensor or
    an array like the input), the disparity planes (int8 [asize][H*W], written for the synthesised SAIs; None unless asked for), the
    SAIs marked missing, synthesised and left (no source within ang_radius), the positions of the synthesised SAIs and the positions
    per disparity (index d + 8).  With disparity_steps > 1 the disparity planes hold j* = d* in units of 1 / disparity_steps,
    disparity_hist is all zero and steps_hist holds the positions per j* (65 bins, index j* + 32); steps_hist is None otherwise.
    With `occlusion` on, steps_hist is filled for every disparity_steps, set_hist holds the positions per set chosen (0 the full set of
    sources, 1..4 the half-planes dt <= 0, dt >= 0, ds <= 0, ds >= 0) and, with return_sets, sets the uint8 planes [asize][H*W] of it;
    both are None otherwise."""
    out: object
    disparity: object
    missing: int
    synthesised: int
    left: int
    pixels: int
    disparity_hist: tuple
    steps_hist: tuple = None
    set_hist: tuple = None
    sets: object = None


class Repair(NamedTuple):
    """Result of Context.repair_fill / Context.repair / repair: the repaired light field (a tensor or an array like the input), the code
    planes (uint8 like the light field: 0 sound, 1 filled from the other views, 2 filled from the rim of its own plane, 3 left; None
    unless asked for), the disparity planes (int8 [asize][H*W], d* at the unsound positions of the swept targets; None unless asked
    for), the SAIs marked missing, the targets and those of them with a source, the passes of the rim fill, the values of the non-empty
    SAIs, the non-zero flags, the counts per stored channel, the positions the sweep wrote at and those positions per disparity
    (index d + 8)."""
    out: object
    codes: object
    disparity: object
    missing: int
    targets: int
    swept: int
    passes: int
    values: int
    flagged: int
    unsound: tuple
    views: tuple
    rim: tuple
    left: tuple
    positions: int
    disparity_hist: tuple


class Inpaint(NamedTuple):
    """Result of Context.inpaint_fill / Context.inpaint / inpaint: the repaired light field (a tensor or an array like the input), the
    flag plane (uint8, 0 = sound, 1 = flagged and filled, 2 = flagged and left; None unless asked for), the counts per stored channel,
    the values of the non-empty SAIs, the largest pass number that filled something and the launches of the fill kernel."""
    out: object
    flags: object
    flagged: tuple
    filled: tuple
    left: tuple
    pixels: int
    passes: int
    launches: int


class ImpulseRepair(NamedTuple):
    """Result of Context.impulse_repair / impulse_repair: the repaired light field (a tensor or an array like the input), the flag plane
    (uint8, 0 = sound, 1 = flagged and repaired, 2 = flagged and left; None unless asked for), the pooled and per-channel median ROAD
    (0 when every threshold was given, and with given flags), the float32 thresholds applied, the counts per stored channel and per
    (SAI, channel) -- counts_sai int64 [asize][C][3] = flagged, repaired, left -- and the values visited / skipped by the statistics."""
    out: object
    flags: object
    scale: float
    scale_channel: tuple
    threshold: tuple
    flagged: tuple
    repaired: tuple
    left: tuple
    pixels: int
    skipped: int
    counts_sai: np.ndarray


class PgEstimate(NamedTuple):
    """Result of Context.pg_estimate / pg_estimate: the light field's model var(z | y) = a y + b (all non-empty SAIs and channels
    pooled), the per-channel models (NaN where a channel's own fit fails), the 2 x 2 blocks visited and skipped (non-finite), and
    the statistics the fits came from: hist uint64 [C][64][322], sum_m uint64 [C][64]."""
    a: float
    b: float
    a_channel: tuple
    b_channel: tuple
    blocks: int
    skipped: int
    hist: np.ndarray
    sum_m: np.ndarray


class ClipNoiseLevel(NamedTuple):
    """Result of Context.noise_level_clipped / noise_level_clipped / clip_fit: sigma of the whole light field (what to pass as
    `sigma`), per stored channel (NaN where a channel's own fit fails), the levels that counted, the rung f_max of the ladder that was
    used (a level counts while at most that fraction of its blocks holds a censored pixel), the censored fraction of all blocks,
    heavily_clipped (f_max > 0.1: the estimate leans on levels the clipping has touched), quantised (every block holds whole numbers:
    the fit allowed for the rounding) and the 2 x 2 blocks visited and skipped (0 from clip_fit)."""
    sigma: float
    sigma_channel: tuple
    levels: int
    f_max: float
    censored: float
    heavily_clipped: bool
    quantised: bool
    blocks: int
    skipped: int


class PgclipEstimate(NamedTuple):
    """Result of Context.pgclip_estimate / pgclip_estimate / pgclip_fit: the pooled model a, b on the range lo..hi, every stored
    channel's own fit (NaN where it fails), the levels that counted, the rung f_max of the ladder, the censored fraction of all
    blocks, heavily_clipped (f_max > 0.1), quantised, and the 2 x 2 blocks visited and skipped (0 from pgclip_fit)."""
    a: float
    b: float
    lo: float
    hi: float
    a_channel: tuple
    b_channel: tuple
    levels: int
    f_max: float
    censored: float
    heavily_clipped: bool
    quantised: bool
    blocks: int
    skipped: int


class PgclipCurves(NamedTuple):
    """Result of pgclip_curves: the model, s (the filter's sigma on the stabilised data), the tables fwd and inv (float32 [4097]) with
    the first knot and the spacing of each, and the C struct that Context.pgclip_forward / pgclip_inverse hand to the library."""
    a: float
    b: float
    lo: float
    hi: float
    s: float
    fwd: np.ndarray
    fwd_x0: float
    fwd_dx: float
    inv: np.ndarray
    inv_x0: float
    inv_dx: float
    struct: PgclipCurvesStruct


class CorrEstimateStruct(C.Structure):
    """lfbm5d_corr_estimate (include/lfbm5d_corr.h)."""
    _fields_ = [("acf", C.c_double * 49), ("sigma", C.c_double), ("cut", C.c_double), ("blocks", C.c_ulonglong),
                ("selected", C.c_ulonglong), ("block", C.c_uint), ("reserved", C.c_uint)]


class CorrEstimate(NamedTuple):
    """Result of Context.corr_measure / corr_measure (include/lfbm5d_corr.h): the autocorrelation of the noise at the lags -3..3
    (float64 [7][7], 1 at [3][3]), the marginal level of the selected blocks (biased low when fraction < 1), the number of blocks,
    the number selected, the largest score selected and the block size used."""
    acf: np.ndarray
    sigma: float
    blocks: int
    selected: int
    cut: float
    block: int


class NoiseLevel(NamedTuple):
    """Result of Context.noise_level / noise_level: sigma of the whole light field (what to pass as `sigma`), per stored channel
    (grey: [0] only), the size m of the noise subspace, the patches pooled, the eigenvalues of the pooled covariance (ascending)
    and, when asked for, every SAI's own estimate (0 for empty SAIs)."""
    sigma: float
    sigma_channel: tuple
    components: int
    patches: int
    eigen: np.ndarray
    sigma_sai: Optional[np.ndarray]


class Quality(NamedTuple):
    """Result of Context.quality / quality / quality_summary: mean and population standard deviation of PSNR, RMSE and SSIM over the
    non-empty SAIs, the pooled mse, the count of non-empty SAIs, and the per-SAI arrays (float64, 0 for empty SAIs).  The ssim
    fields are None when SSIM was not asked for.  One SAI with mse == 0 makes psnr_mean +inf (IEEE arithmetic, not special-cased)."""
    psnr_mean: float
    psnr_std: float
    rmse_mean: float
    rmse_std: float
    ssim_mean: Optional[float]
    ssim_std: Optional[float]
    mse: float
    count: int
    psnr_sai: np.ndarray
    rmse_sai: np.ndarray
    ssim_sai: Optional[np.ndarray]


def library_path():
    return os.path.join(_HERE, "liblfbm5d_hip.so")


def build_library(force=False):
    """Compile the HIP extension in-tree (hipcc --offload-arch=gfx950; works without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    args = ["make", "-C", src]
    if force:
        subprocess.check_call(args + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return library_path()


_lib = None


def lib():
    """Load the HIP extension.  Fails loudly if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # LFBM5D_HIP_LIB: an alternative build of the same library (kernel A/B experiments, tools/build_variant.sh)
    path = os.environ.get("LFBM5D_HIP_LIB") or library_path()
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  lfbm5d_amd has no CPU fallback.")
    L = C.CDLL(path)
    vp, up, fp = C.c_void_p, C.POINTER(C.c_uint), C.c_void_p
    L.lfbm5d_create.argtypes = [C.POINTER(vp), C.c_int]
    L.lfbm5d_destroy.argtypes = [vp]
    L.lfbm5d_last_error.argtypes = [vp]
    L.lfbm5d_last_error.restype = C.c_char_p
    L.lfbm5d_reset_stats.argtypes = [vp]
    L.lfbm5d_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.lfbm5d_stream.argtypes = [vp]
    L.lfbm5d_stream.restype = vp
    if hasattr(L, "lfbm5d_set_option"):      # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs: they read the environment themselves)
        L.lfbm5d_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.lfbm5d_get_option.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_ulonglong]
    L.lfbm5d_comm_unique_id.argtypes = [vp]
    L.lfbm5d_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    if hasattr(L, "lfbm5d_comm_init_ipc"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        L.lfbm5d_comm_init_ipc.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_double]
    L.lfbm5d_set_shard.argtypes = [vp, C.c_int, C.c_int]
    L.lfbm5d_set_tiles.argtypes = [vp, C.c_int]
    L.lfbm5d_comm_ranks.argtypes = [vp]
    L.lfbm5d_comm_ranks.restype = C.c_int
    L.lfbm5d_comm_selftest.argtypes = [vp, C.c_uint]
    L.lfbm5d_auto_bands.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int]
    L.lfbm5d_auto_bands.restype = C.c_int
    L.lfbm5d_shard_rows.argtypes = [C.c_uint, C.c_int, C.c_int, up, up]
    L.lfbm5d_shard_rows.restype = None
    L.lfbm5d_plan_windows.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, up, up, C.c_uint]
    L.lfbm5d_last_windows.argtypes = [vp, up, C.c_uint]
    L.lfbm5d_plan_graph.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, up, C.c_int, C.c_int, up, up, up, C.c_uint]
    L.lfbm5d_plan_messages.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, up, C.c_int, up, C.c_uint]
    L.lfbm5d_plan_job.argtypes = [C.c_uint, C.c_uint, C.c_uint, up, C.c_int, up, up, C.c_int, C.c_int, up, C.c_uint, up, C.c_uint, up]
    L.lfbm5d_denoise_device.argtypes = [vp, C.POINTER(Params), C.POINTER(Params), fp, up, fp, fp] + [C.c_uint] * 8
    L.lfbm5d_denoise_host.argtypes = [vp, C.POINTER(Params), C.POINTER(Params), fp, up, fp, fp] + [C.c_uint] * 8
    tail = [C.c_uint] * 7
    L.lfbm5d_step1_device.argtypes = [vp, C.POINTER(Params), fp, up, fp] + tail
    L.lfbm5d_step2_device.argtypes = [vp, C.POINTER(Params), fp, up, fp, fp] + tail
    L.lfbm5d_step1_host.argtypes = [vp, C.POINTER(Params), fp, up, fp] + tail
    L.lfbm5d_step2_host.argtypes = [vp, C.POINTER(Params), fp, up, fp, fp] + tail
    # host seam with one pointer per SAI (what the reference's vector<vector<float>> is): arrays of float*
    if hasattr(L, "lfbm5d_denoise_host_sai"):
        L.lfbm5d_step1_host_sai.argtypes = [vp, C.POINTER(Params), fp, up, fp] + tail
        L.lfbm5d_step2_host_sai.argtypes = [vp, C.POINTER(Params), fp, up, fp, fp] + tail
        L.lfbm5d_denoise_host_sai.argtypes = [vp, C.POINTER(Params), C.POINTER(Params), fp, up, fp, fp] + [C.c_uint] * 8
    L.lfbm5d_pass_device.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_uint, C.c_uint, C.c_uint,
                                     C.c_uint, C.c_uint, fp, fp, fp, fp, up, up, C.c_uint, C.c_uint]
    L.lfbm5d_last_bm.argtypes = [vp, up, vp, vp, vp, vp, vp]
    bp = C.POINTER(Bm3dParams)
    L.lfbm5d_bm3d_step_device.argtypes = [vp, C.c_int, bp, C.c_uint, C.c_uint, C.c_uint, fp, fp, fp]
    L.lfbm5d_bm3d_lf_device.argtypes = [vp, bp, bp, fp, up, fp, fp, C.c_uint, C.c_uint, C.c_uint, C.c_uint]
    L.lfbm5d_bm3d_lf_host.argtypes = [vp, bp, bp, fp, up, fp, fp, C.c_uint, C.c_uint, C.c_uint, C.c_uint]
    L.lfbm5d_last_tables.argtypes = [vp, vp, C.c_size_t]
    L.lfbm5d_last_tables.restype = C.c_size_t
    L.lfbm5d_last_weights.argtypes = [vp, vp, C.c_size_t]
    L.lfbm5d_last_weights.restype = C.c_size_t
    if hasattr(L, "lfbm5d_last_group_list"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        L.lfbm5d_last_group_list.argtypes = [vp, up, vp, C.c_uint]
    L.lfbm5d_last_scores.argtypes = [vp, vp, C.c_size_t]
    L.lfbm5d_last_scores.restype = C.c_size_t
    L.lfbm5d_last_scan_version.argtypes = [vp]
    L.lfbm5d_last_scan_version.restype = C.c_int
    if hasattr(L, "lfbm5d_debug_aggregate"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        L.lfbm5d_debug_aggregate.argtypes = [vp, C.POINTER(AggDebugStruct)]
    if hasattr(L, "lfbm5d_debug_group"):
        L.lfbm5d_debug_group.argtypes = [vp, C.POINTER(GroupDebugStruct)]
    if hasattr(L, "lfbm5d_debug_window"):
        L.lfbm5d_debug_window.argtypes = [vp, C.POINTER(WindowDebugStruct)]
        L.lfbm5d_sigma_table.argtypes = [C.c_float, C.c_uint, C.c_uint, fp]
    if hasattr(L, "lfbm5d_noise_level_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        dp, np_ = C.POINTER(C.c_double), C.POINTER(NoiseLevelStruct)
        L.lfbm5d_noise_level_device.argtypes = [vp, fp, up] + [C.c_uint] * 5 + [np_, dp, dp]
        L.lfbm5d_noise_level_host_sai.argtypes = [vp, fp, up] + [C.c_uint] * 5 + [np_, dp, dp]
        L.lfbm5d_noise_level_statistic.argtypes = [C.c_uint, dp, dp, up, dp]
    if hasattr(L, "lfbm5d_quality_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        dp, qp = C.POINTER(C.c_double), C.POINTER(QualityStruct)
        L.lfbm5d_quality_device.argtypes = [vp, fp, fp, up] + [C.c_uint] * 4 + [C.c_double, C.c_int, qp, dp, dp]
        L.lfbm5d_quality_host_sai.argtypes = [vp, fp, fp, up] + [C.c_uint] * 4 + [C.c_double, C.c_int, qp, dp, dp]
        L.lfbm5d_quality_summary.argtypes = [dp, dp, up, C.c_uint, C.c_double, qp]
    if hasattr(L, "lfbm5d_superres_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        sp, pp = C.POINTER(SrParams), C.POINTER(Params)
        L.lfbm5d_sr_defaults.argtypes = [C.c_uint, sp]
        L.lfbm5d_sr_taps.argtypes = [C.c_uint, sp, C.c_uint, vp, vp, up, C.c_uint]
        L.lfbm5d_sr_up_device.argtypes = [vp, sp, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_sr_down_device.argtypes = [vp, sp, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_sr_backproject_device.argtypes = [vp, sp, fp, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_superres_device.argtypes = [vp, sp, pp, fp, up, fp] + [C.c_uint] * 7
        L.lfbm5d_superres_host_sai.argtypes = [vp, sp, pp, fp, up, fp] + [C.c_uint] * 7
    if hasattr(L, "lfbm5d_denoise_pg_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        dp, ullp, mp_, ep = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), C.POINTER(PgModelStruct), C.POINTER(PgEstimateStruct)
        pp = C.POINTER(Params)
        L.lfbm5d_pg_histogram_device.argtypes = [vp, fp, up] + [C.c_uint] * 4 + [ullp, ullp, ullp, ullp]
        L.lfbm5d_pg_fit.argtypes = [ullp, ullp, dp, dp]
        L.lfbm5d_pg_estimate_device.argtypes = [vp, fp, up] + [C.c_uint] * 4 + [ep, ullp, ullp]
        L.lfbm5d_pg_estimate_host_sai.argtypes = [vp, fp, up] + [C.c_uint] * 4 + [ep, ullp, ullp]
        L.lfbm5d_pg_scale.argtypes = [mp_, C.c_uint, dp]
        L.lfbm5d_pg_forward_device.argtypes = [vp, mp_, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_pg_inverse_device.argtypes = [vp, mp_, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_denoise_pg_device.argtypes = [vp, mp_, mp_, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_denoise_pg_host_sai.argtypes = [vp, mp_, mp_, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
    if hasattr(L, "lfbm5d_denoise_clipped_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        ullp, cep, dp, pp = C.POINTER(C.c_ulonglong), C.POINTER(ClipEstimateStruct), C.POINTER(C.c_double), C.POINTER(Params)
        rng = [C.c_double, C.c_double]
        L.lfbm5d_clip_histogram_device.argtypes = [vp, fp, up] + [C.c_uint] * 4 + rng + [ullp] * 6
        L.lfbm5d_clip_fit.argtypes = [ullp, ullp, ullp, ullp, C.c_uint] + rng + [cep]
        L.lfbm5d_noise_level_clipped_device.argtypes = [vp, fp, up] + [C.c_uint] * 4 + rng + [cep]
        L.lfbm5d_noise_level_clipped_host_sai.argtypes = [vp, fp, up] + [C.c_uint] * 4 + rng + [cep]
        L.lfbm5d_declip_device.argtypes = [vp, C.c_double] + rng + [fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_declip_host_sai.argtypes = [vp, C.c_double] + rng + [fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_denoise_clipped_device.argtypes = [vp, C.c_double] + rng + [cep, dp, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_denoise_clipped_host_sai.argtypes = [vp, C.c_double] + rng + [cep, dp, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
    if hasattr(L, "lfbm5d_denoise_pgclip_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        ullp, pp = C.POINTER(C.c_ulonglong), C.POINTER(Params)
        gm, ge, gc = C.POINTER(PgclipModelStruct), C.POINTER(PgclipEstimateStruct), C.POINTER(PgclipCurvesStruct)
        rng = [C.c_double, C.c_double]
        L.lfbm5d_pgclip_fit.argtypes = [ullp, ullp, ullp, ullp, C.c_uint] + rng + [ge]
        L.lfbm5d_pgclip_curves.argtypes = [gm, gc]
        L.lfbm5d_pgclip_curves_error.argtypes = []
        L.lfbm5d_pgclip_curves_error.restype = C.c_char_p
        L.lfbm5d_pgclip_estimate_device.argtypes = [vp, fp, up] + [C.c_uint] * 4 + rng + [ge]
        L.lfbm5d_pgclip_estimate_host_sai.argtypes = [vp, fp, up] + [C.c_uint] * 4 + rng + [ge]
        L.lfbm5d_pgclip_forward_device.argtypes = [vp, gc, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_pgclip_inverse_device.argtypes = [vp, gc, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_denoise_pgclip_device.argtypes = [vp, gm] + rng + [gm, C.POINTER(C.c_double), ge, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_denoise_pgclip_host_sai.argtypes = [vp, gm] + rng + [gm, C.POINTER(C.c_double), ge, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
    if hasattr(L, "lfbm5d_impulse_repair_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        dp, ullp = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
        ip, rp = C.POINTER(ImpulseParamsStruct), C.POINTER(ImpulseResultStruct)
        L.lfbm5d_impulse_defaults.argtypes = [ip]
        L.lfbm5d_impulse_defaults.restype = None
        L.lfbm5d_impulse_histogram_device.argtypes = [vp, fp, up] + [C.c_uint] * 4 + [ullp, ullp, ullp]
        L.lfbm5d_impulse_scale.argtypes = [ullp, dp]
        L.lfbm5d_impulse_repair_device.argtypes = [vp, ip, fp, up, fp, vp] + [C.c_uint] * 4 + [rp, ullp]
        L.lfbm5d_impulse_repair_flags_device.argtypes = [vp, fp, vp, up, fp, vp] + [C.c_uint] * 4 + [rp, ullp]
        L.lfbm5d_impulse_repair_host_sai.argtypes = [vp, ip, fp, vp, up, fp, vp] + [C.c_uint] * 4 + [rp, ullp]
    if hasattr(L, "lfbm5d_inpaint_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        np_, nr, pp = C.POINTER(InpaintParamsStruct), C.POINTER(InpaintResultStruct), C.POINTER(Params)
        L.lfbm5d_inpaint_defaults.argtypes = [np_]
        L.lfbm5d_inpaint_defaults.restype = None
        L.lfbm5d_inpaint_fill_device.argtypes = [vp, fp, vp, up, fp, vp] + [C.c_uint] * 4 + [nr]
        L.lfbm5d_inpaint_project_device.argtypes = [vp, vp, fp, fp, up, fp] + [C.c_uint] * 4
        L.lfbm5d_inpaint_device.argtypes = [vp, np_, pp, fp, vp, up, fp, vp] + [C.c_uint] * 7 + [nr]
        L.lfbm5d_inpaint_host_sai.argtypes = [vp, np_, pp, fp, vp, up, fp, vp] + [C.c_uint] * 7 + [nr]
    if hasattr(L, "lfbm5d_view_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        wp, wr, pp = C.POINTER(ViewParamsStruct), C.POINTER(ViewResultStruct), C.POINTER(Params)
        L.lfbm5d_view_defaults.argtypes = [wp]
        L.lfbm5d_view_defaults.restype = None
        L.lfbm5d_view_fill_device.argtypes = [vp, wp, fp, up, up, fp, vp] + [C.c_uint] * 6 + [wr]
        L.lfbm5d_view_device.argtypes = [vp, wp, pp, fp, up, up, fp, vp] + [C.c_uint] * 7 + [wr]
        L.lfbm5d_view_host_sai.argtypes = [vp, wp, pp, vp, up, up, vp, vp] + [C.c_uint] * 7 + [wr]
    if hasattr(L, "lfbm5d_view_steps_device"):   # the sub-pixel forms: `steps` behind the parameters, the 65-bin histogram at the end
        wp, wr, pp = C.POINTER(ViewParamsStruct), C.POINTER(ViewResultStruct), C.POINTER(Params)
        cp, cr = C.POINTER(ConsistParamsStruct), C.POINTER(ConsistResultStruct)
        ullp, dp = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
        L.lfbm5d_view_fill_steps_device.argtypes = [vp, wp, C.c_uint, fp, up, up, fp, vp] + [C.c_uint] * 6 + [wr, ullp]
        L.lfbm5d_view_steps_device.argtypes = [vp, wp, C.c_uint, pp, fp, up, up, fp, vp] + [C.c_uint] * 7 + [wr, ullp]
        L.lfbm5d_view_steps_host_sai.argtypes = [vp, wp, C.c_uint, pp, vp, up, up, vp, vp] + [C.c_uint] * 7 + [wr, ullp]
        L.lfbm5d_consist_steps_device.argtypes = [vp, cp, C.c_uint, fp, up, up, vp, up, vp, dp, ullp] + [C.c_uint] * 6 + [cr]
        L.lfbm5d_consist_steps_host_sai.argtypes = [vp, cp, C.c_uint, vp, up, up, vp, up, vp, dp, ullp] + [C.c_uint] * 6 + [cr]
    if hasattr(L, "lfbm5d_view_occl_device"):   # the occlusion-aware forms: the ratio behind `steps`, the set planes behind the disparities
        wp, wr, pp = C.POINTER(ViewParamsStruct), C.POINTER(ViewResultStruct), C.POINTER(Params)
        ullp, orp = C.POINTER(C.c_ulonglong), C.POINTER(ViewOcclResultStruct)
        L.lfbm5d_view_occl_default.argtypes = []
        L.lfbm5d_view_occl_default.restype = C.c_float
        L.lfbm5d_view_fill_occl_device.argtypes = [vp, wp, C.c_uint, C.c_float, fp, up, up, fp, vp, vp] + [C.c_uint] * 6 + [wr, ullp, orp]
        L.lfbm5d_view_occl_device.argtypes = [vp, wp, C.c_uint, C.c_float, pp, fp, up, up, fp, vp, vp] + [C.c_uint] * 7 + [wr, ullp, orp]
        L.lfbm5d_view_occl_host_sai.argtypes = [vp, wp, C.c_uint, C.c_float, pp, vp, up, up, vp, vp, vp] + [C.c_uint] * 7 + [wr, ullp, orp]
    if hasattr(L, "lfbm5d_repair_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        jp, jr, pp = C.POINTER(RepairParamsStruct), C.POINTER(RepairResultStruct), C.POINTER(Params)
        L.lfbm5d_repair_defaults.argtypes = [jp]
        L.lfbm5d_repair_defaults.restype = None
        L.lfbm5d_repair_fill_device.argtypes = [vp, jp, fp, vp, up, up, fp, vp, vp] + [C.c_uint] * 6 + [jr]
        L.lfbm5d_repair_device.argtypes = [vp, jp, pp, fp, vp, up, up, fp, vp, vp] + [C.c_uint] * 7 + [jr]
        L.lfbm5d_repair_host_sai.argtypes = [vp, jp, pp, vp, vp, up, up, vp, vp, vp] + [C.c_uint] * 7 + [jr]
    if hasattr(L, "lfbm5d_consist_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        cp, cr = C.POINTER(ConsistParamsStruct), C.POINTER(ConsistResultStruct)
        dp, ullp = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
        L.lfbm5d_consist_defaults.argtypes = [cp]
        L.lfbm5d_consist_defaults.restype = None
        L.lfbm5d_consist_device.argtypes = [vp, cp, fp, up, up, vp, up, vp, dp, ullp] + [C.c_uint] * 6 + [cr]
        L.lfbm5d_consist_host_sai.argtypes = [vp, cp, vp, up, up, vp, up, vp, dp, ullp] + [C.c_uint] * 6 + [cr]
    if hasattr(L, "lfbm5d_photo_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        qp, qr = C.POINTER(PhotoParamsStruct), C.POINTER(PhotoResultStruct)
        dp, ullp = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
        L.lfbm5d_photo_defaults.argtypes = [qp]
        L.lfbm5d_photo_defaults.restype = None
        L.lfbm5d_photo_edges.argtypes = [C.POINTER(C.c_float)]
        L.lfbm5d_photo_edges.restype = None
        L.lfbm5d_photo_ratio.argtypes = [ullp, C.c_ulonglong, dp]
        L.lfbm5d_photo_solve.argtypes = [C.c_uint, dp, up, up, up, C.c_uint, dp]
        L.lfbm5d_photo_device.argtypes = [vp, qp, fp, up, fp, dp, up, ullp] + [C.c_uint] * 6 + [qr]
        L.lfbm5d_photo_host_sai.argtypes = [vp, qp, vp, up, vp, dp, up, ullp] + [C.c_uint] * 6 + [qr]
        L.lfbm5d_photo_apply_device.argtypes = [vp, fp, up, dp, C.c_uint, fp] + [C.c_uint] * 5
        L.lfbm5d_photo_apply_host_sai.argtypes = [vp, vp, up, dp, C.c_uint, vp] + [C.c_uint] * 5
    if hasattr(L, "lfbm5d_denoise_views_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        dp, pp = C.POINTER(C.c_double), C.POINTER(Params)
        L.lfbm5d_views_error.argtypes = []
        L.lfbm5d_views_error.restype = C.c_char_p
        L.lfbm5d_views_window_sigma.argtypes = [dp, up] + [C.c_uint] * 6 + [C.POINTER(C.c_float)]
        L.lfbm5d_views_from_gains.argtypes = [C.c_double, C.POINTER(C.c_float), C.c_uint, up, C.c_uint, dp]
        L.lfbm5d_denoise_views_device.argtypes = [vp, dp, dp, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_denoise_views_host_sai.argtypes = [vp, dp, dp, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_step1_views_device.argtypes = [vp, dp, dp, pp, fp, up, fp] + [C.c_uint] * 7
        L.lfbm5d_step2_views_device.argtypes = [vp, dp, dp, pp, fp, up, fp, fp] + [C.c_uint] * 7
        L.lfbm5d_bm3d_lf_views_device.argtypes = [vp, dp, dp, bp, bp, fp, up, fp, fp] + [C.c_uint] * 4
        L.lfbm5d_last_window_sigmas.argtypes = [vp, C.POINTER(C.c_float), C.c_uint]
    if hasattr(L, "lfbm5d_denoise_corr_device"):   # (absent from older builds loaded through LFBM5D_HIP_LIB for A/B runs)
        dp, pp = C.POINTER(C.c_double), C.POINTER(Params)
        L.lfbm5d_corr_error.argtypes = []
        L.lfbm5d_corr_error.restype = C.c_char_p
        L.lfbm5d_corr_check.argtypes = [dp]
        L.lfbm5d_corr_from_kernel.argtypes = [dp, C.c_uint, C.c_uint, dp]
        L.lfbm5d_corr_table.argtypes = [dp, C.c_uint, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_float), up]
        L.lfbm5d_corr_measure_device.argtypes = [vp, fp, up] + [C.c_uint] * 5 + [C.c_double, C.POINTER(CorrEstimateStruct)]
        L.lfbm5d_corr_measure_host_sai.argtypes = [vp, vp, up] + [C.c_uint] * 5 + [C.c_double, C.POINTER(CorrEstimateStruct)]
        L.lfbm5d_denoise_corr_device.argtypes = [vp, dp, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_denoise_corr_host_sai.argtypes = [vp, dp, pp, pp, fp, up, fp, fp] + [C.c_uint] * 8
        L.lfbm5d_step1_corr_device.argtypes = [vp, dp, pp, fp, up, fp] + [C.c_uint] * 7
        L.lfbm5d_step2_corr_device.argtypes = [vp, dp, pp, fp, up, fp, fp] + [C.c_uint] * 7
        L.lfbm5d_debug_group_corr.argtypes = [vp, C.POINTER(GroupDebugStruct), dp]
    L.lfbm5d_malloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.lfbm5d_free.argtypes = [vp]
    L.lfbm5d_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
    L.lfbm5d_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
    L.lfbm5d_device_count.restype = C.c_int
    _lib = L
    return L


def plan_windows(awidth, aheight, an=1, ang_major=None, mask=None):
    """Window schedule of a step (processed SAI of every window, in order); host only."""
    ang_major = ROWMAJOR if ang_major is None else ang_major
    m = np.ones(awidth * aheight, np.uint32) if mask is None else _u32(mask)
    out = np.zeros(awidth * aheight, np.uint32)
    n = lib().lfbm5d_plan_windows(awidth, aheight, an, ang_major, m.ctypes.data_as(C.POINTER(C.c_uint)),
                                  out.ctypes.data_as(C.POINTER(C.c_uint)), out.size)
    if n < 0:
        raise LfBm5dError("lfbm5d_plan_windows: bad arguments")
    return out[:n].copy()


def plan_graph(awidth, aheight, world, lanes=1, an=1, ang_major=None, mask=None):
    """Graph form of a step (host only): (rank, lane, start slot) of every planned window, as uint32 arrays."""
    ang_major = ROWMAJOR if ang_major is None else ang_major
    m = np.ones(awidth * aheight, np.uint32) if mask is None else _u32(mask)
    mp = m.ctypes.data_as(C.POINTER(C.c_uint))
    n = lib().lfbm5d_plan_graph(awidth, aheight, an, ang_major, mp, world, lanes, None, None, None, 0)
    if n < 0:
        raise LfBm5dError("lfbm5d_plan_graph: bad arguments")
    r, l, t = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    lib().lfbm5d_plan_graph(awidth, aheight, an, ang_major, mp, world, lanes, p(r), p(l), p(t), n)
    return r[:n], l[:n], t[:n]


def plan_messages(awidth, aheight, world, an=1, ang_major=None, mask=None):
    """Messages of the graph form in issue order: rows of (producer window, consumer window, SAI, channel)."""
    ang_major = ROWMAJOR if ang_major is None else ang_major
    m = np.ones(awidth * aheight, np.uint32) if mask is None else _u32(mask)
    mp = m.ctypes.data_as(C.POINTER(C.c_uint))
    n = lib().lfbm5d_plan_messages(awidth, aheight, an, ang_major, mp, world, None, 0)
    if n < 0:
        raise LfBm5dError("lfbm5d_plan_messages: bad arguments")
    out = np.zeros((max(n, 1), 4), np.uint32)
    lib().lfbm5d_plan_messages(awidth, aheight, an, ang_major, mp, world, out.ctypes.data_as(C.POINTER(C.c_uint)), n)
    return out[:n]


def plan_job(awidth, aheight, world, lanes=1, an=(1, 1), cost=None, ang_major=None, mask=None):
    """Graph of a job (len(an) = 1: one step; 2: both steps as lfbm5d_denoise_* runs them), host only.  Returns
    (nodes, msgs, info): nodes[i] = (step slot, window, processed SAI, graph rank, lane, start, issue position, chain) as a
    uint32 array [n, 8]; msgs[j] = (kind, producer node, consumer node | 0xffffffff, receiving rank, SAI, channel) [m, 6];
    info = dict(windows, messages, makespan, centre_ok)."""
    ang_major = ROWMAJOR if ang_major is None else ang_major
    m = np.ones(awidth * aheight, np.uint32) if mask is None else _u32(mask)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    an_a = _u32(list(an))
    cost_a = _u32(list(cost)) if cost is not None else None
    cnt = np.zeros(4, np.uint32)
    n = lib().lfbm5d_plan_job(awidth, aheight, ang_major, p(m), len(an_a), p(an_a), p(cost_a) if cost_a is not None else None,
                              world, lanes, None, 0, None, 0, p(cnt))
    if n < 0:
        raise LfBm5dError("lfbm5d_plan_job: bad arguments")
    nodes = np.zeros((max(int(cnt[0]), 1), 8), np.uint32)
    msgs = np.zeros((max(int(cnt[1]), 1), 6), np.uint32)
    lib().lfbm5d_plan_job(awidth, aheight, ang_major, p(m), len(an_a), p(an_a), p(cost_a) if cost_a is not None else None,
                          world, lanes, p(nodes), int(cnt[0]), p(msgs), int(cnt[1]), p(cnt))
    return nodes[:int(cnt[0])], msgs[:int(cnt[1])], {"windows": int(cnt[0]), "messages": int(cnt[1]), "makespan": int(cnt[2]),
                                                     "centre_ok": bool(cnt[3])}


def auto_bands(awidth, aheight, height, halo, world):
    """Spatial bands S for a two-step job on `world` ranks (lfbm5d_auto_bands, include/lfbm5d.h; tools/scale_model.py): the graph takes the
    ranks it can keep busy (a power of two within 0.8 ceil(a / 3)), bands take the rest, as long as a band stays twice as tall as its
    halo.  1 = the graph alone (bit-identical to one GPU)."""
    return int(lib().lfbm5d_auto_bands(int(awidth), int(aheight), int(height), int(halo), int(world)))


def noise_level_statistic(cov):
    """lfbm5d_noise_level_statistic (host only, no GPU): (sigma, components, eigenvalues ascending) of one symmetric d x d
    covariance, d <= 64."""
    cov = np.ascontiguousarray(cov, np.float64)
    d = cov.shape[0]
    sig, m, lam = C.c_double(), C.c_uint(), np.zeros(d, np.float64)
    dp = C.POINTER(C.c_double)
    if lib().lfbm5d_noise_level_statistic(d, cov.ctypes.data_as(dp), C.byref(sig), C.byref(m), lam.ctypes.data_as(dp)) != 0:
        raise LfBm5dError("lfbm5d_noise_level_statistic: bad arguments (d must be 1..64)")
    return sig.value, m.value, lam


def _quality_result(res, mse, ssim, m, peak):
    """Quality from the summary struct and the per-SAI mse / ssim arrays (psnr and rmse per SAI follow from mse)."""
    pk = 255.0 if peak == 0 else float(peak)
    on = m != 0
    psnr, rmse = np.zeros(m.size, np.float64), np.zeros(m.size, np.float64)
    with np.errstate(divide="ignore"):
        psnr[on] = 10.0 * np.log10(pk * pk / mse[on])
    rmse[on] = np.sqrt(mse[on])
    has = bool(res.has_ssim)
    return Quality(res.psnr_mean, res.psnr_std, res.rmse_mean, res.rmse_std, res.ssim_mean if has else None, res.ssim_std if has else None,
                   res.mse, int(res.count), psnr, rmse, ssim if has else None)


def quality_summary(mse_sai, ssim_sai, mask, peak=255.0):
    """lfbm5d_quality_summary (host only, no GPU): the Quality of per-SAI mse and ssim (or None) under `mask`; entries of empty SAIs
    are ignored (and 0 in the result's arrays)."""
    m = _u32(mask)
    mse = np.ascontiguousarray(mse_sai, np.float64).copy()
    ssim = None if ssim_sai is None else np.ascontiguousarray(ssim_sai, np.float64).copy()
    if mse.size != m.size or (ssim is not None and ssim.size != m.size):
        raise LfBm5dError("lfbm5d_quality_summary: mse, ssim and mask must hold one entry per SAI")
    dp = C.POINTER(C.c_double)
    res = QualityStruct()
    if lib().lfbm5d_quality_summary(mse.ctypes.data_as(dp), ssim.ctypes.data_as(dp) if ssim is not None else None,
                                    m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, float(peak), C.byref(res)) != 0:
        raise LfBm5dError("lfbm5d_quality_summary: bad arguments (no non-empty SAI, or peak negative or not finite)")
    mse[m == 0] = 0.0
    if ssim is not None:
        ssim[m == 0] = 0.0
    return _quality_result(res, mse, ssim, m, peak)


def sigma_table(sigma, chnls, color_space):
    """lfbm5d_sigma_table (host only, no GPU): the noise level of every channel behind the forward colour transform, float32 [chnls]."""
    out = np.zeros(3, np.float32)
    if lib().lfbm5d_sigma_table(float(sigma), int(chnls), int(color_space), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise LfBm5dError("lfbm5d_sigma_table: unknown colour space")
    return out[:chnls]


def pg_fit(hist, sum_m):
    """lfbm5d_pg_fit (host only, no GPU): (a, b) of one histogram hist uint64 [64][322] with sum_m uint64 [64] (include/lfbm5d.h has
    the definition).  Raises when no level is valid."""
    h = np.ascontiguousarray(hist, np.uint64)
    sm = np.ascontiguousarray(sum_m, np.uint64)
    if h.shape != (PG_LEVELS, PG_KEYS) or sm.shape != (PG_LEVELS,):
        raise LfBm5dError("lfbm5d_pg_fit: hist must be [64][322] and sum_m [64]")
    a, b = C.c_double(), C.c_double()
    ullp = C.POINTER(C.c_ulonglong)
    if lib().lfbm5d_pg_fit(h.ctypes.data_as(ullp), sm.ctypes.data_as(ullp), C.byref(a), C.byref(b)) != 0:
        raise LfBm5dError("lfbm5d_pg_fit: no valid level (every level holds fewer than 256 blocks, or its quantile fell into an end bin)")
    return a.value, b.value


def _pgclip_result(res, chnls):
    m = res.model
    return PgclipEstimate(m.a, m.b, m.lo, m.hi, tuple(res.a_channel[:chnls]), tuple(res.b_channel[:chnls]), int(res.levels), res.f_max,
                          res.censored, bool(res.heavily_clipped), bool(res.quantised), int(res.blocks), int(res.skipped))


def pgclip_fit(hist, sum_m, cens, whole, lo=0.0, hi=255.0):
    """lfbm5d_pgclip_fit (host only, no GPU): the PgclipEstimate of the statistics hist uint64 [C][64][322], sum_m and cens uint64
    [C][64] and whole uint64 [C] of Context.clip_histogram.  Raises when fewer than 4 levels are populated or the range is bad."""
    h, sm = np.ascontiguousarray(hist, np.uint64), np.ascontiguousarray(sum_m, np.uint64)
    cz, wh = np.ascontiguousarray(cens, np.uint64), np.ascontiguousarray(whole, np.uint64)
    if h.ndim != 3 or h.shape[0] not in (1, 3) or h.shape[1:] != (PG_LEVELS, PG_KEYS) or sm.shape != h.shape[:2] or cz.shape != h.shape[:2] \
            or wh.shape != h.shape[:1]:
        raise LfBm5dError("lfbm5d_pgclip_fit: hist must be [C][64][322], sum_m and cens [C][64], whole [C], C = 1 or 3")
    ullp = C.POINTER(C.c_ulonglong)
    res = PgclipEstimateStruct()
    if lib().lfbm5d_pgclip_fit(h.ctypes.data_as(ullp), sm.ctypes.data_as(ullp), cz.ctypes.data_as(ullp), wh.ctypes.data_as(ullp), h.shape[0],
                               float(lo), float(hi), C.byref(res)) != 0:
        raise LfBm5dError("lfbm5d_pgclip_fit: fewer than 4 levels are populated (256 blocks, a quantile outside the end bins), or the "
                          "range is bad (lo < hi, both finite)")
    return _pgclip_result(res, h.shape[0])


def pgclip_curves(a, b, lo=0.0, hi=255.0):
    """lfbm5d_pgclip_curves (host only, no GPU): the PgclipCurves of the model sigma^2(y) = max(a (y - lo) + b, 1/12) on lo..hi.  Raises
    on an invalid model and on one outside the accepted domain (a^2 <= 0.5 b, a <= 5: beyond it denoise_pg is the tool)."""
    m = PgclipModelStruct(float(a), float(b), float(lo), float(hi))
    cv = PgclipCurvesStruct()
    L = lib()
    if L.lfbm5d_pgclip_curves(C.byref(m), C.byref(cv)) != 0:
        raise LfBm5dError(L.lfbm5d_pgclip_curves_error().decode())
    return PgclipCurves(m.a, m.b, m.lo, m.hi, cv.s, np.ctypeslib.as_array(cv.fwd).copy(), cv.fwd_x0, cv.fwd_dx,
                        np.ctypeslib.as_array(cv.inv).copy(), cv.inv_x0, cv.inv_dx, cv)


def _clip_result(res, chnls):
    return ClipNoiseLevel(res.sigma, tuple(res.sigma_channel[:chnls]), int(res.levels), res.f_max, res.censored, bool(res.heavily_clipped),
                          bool(res.quantised), int(res.blocks), int(res.skipped))


def clip_fit(hist, sum_m, cens, whole, lo=0.0, hi=255.0):
    """lfbm5d_clip_fit (host only, no GPU): the ClipNoiseLevel of the statistics hist uint64 [C][64][322], cens uint64 [C][64] and whole
    uint64 [C] of Context.clip_histogram (sum_m [C][64] belongs to them and is not read; it may be None).  Raises when fewer than 4
    levels are populated (include/lfbm5d.h has the definition)."""
    h = np.ascontiguousarray(hist, np.uint64)
    cz = np.ascontiguousarray(cens, np.uint64)
    wh = np.ascontiguousarray(whole, np.uint64).reshape(-1)
    sm = None if sum_m is None else np.ascontiguousarray(sum_m, np.uint64)
    if h.ndim != 3 or h.shape[0] not in (1, 3) or h.shape[1:] != (PG_LEVELS, PG_KEYS) or cz.shape != h.shape[:2] or wh.shape != h.shape[:1] \
            or (sm is not None and sm.shape != h.shape[:2]):
        raise LfBm5dError("lfbm5d_clip_fit: hist must be [C][64][322], sum_m and cens [C][64], whole [C], C = 1 or 3")
    ullp = C.POINTER(C.c_ulonglong)
    res = ClipEstimateStruct()
    if lib().lfbm5d_clip_fit(h.ctypes.data_as(ullp), sm.ctypes.data_as(ullp) if sm is not None else None, cz.ctypes.data_as(ullp),
                             wh.ctypes.data_as(ullp), h.shape[0], float(lo), float(hi), C.byref(res)) != 0:
        raise LfBm5dError("lfbm5d_clip_fit: fewer than 4 levels are populated (256 blocks, a quantile outside the end bins), or the range "
                          "is bad (lo < hi, both finite)")
    return _clip_result(res, h.shape[0])


def pg_model(a, b, chnls=3):
    """lfbm5d_pg_model from scalars (the same model for every channel) or per-channel sequences."""
    a = [float(a)] * chnls if np.isscalar(a) else [float(v) for v in a]
    b = [float(b)] * chnls if np.isscalar(b) else [float(v) for v in b]
    if len(a) != chnls or len(b) != chnls or chnls not in (1, 3):
        raise LfBm5dError("a Poisson-Gaussian model holds one (a, b) per stored channel, 1 or 3 of them")
    m = PgModelStruct()
    for i in range(3):
        j = i if chnls == 3 else 0
        m.a[i], m.b[i] = a[j], b[j]
    return m


def _as_pg_model(model, chnls):
    if model is None or isinstance(model, PgModelStruct):
        return model
    if isinstance(model, PgEstimate):
        return pg_model(model.a, model.b, chnls)
    return pg_model(model[0], model[1], chnls)


def pg_scale(model, chnls=3):
    """lfbm5d_pg_scale (host only, no GPU): the sigma of the light field after the forward transform of `model` (a PgModelStruct, a
    PgEstimate or a pair (a, b) of scalars or per-channel sequences).  Raises on a rejected model."""
    s = C.c_double()
    try:
        m = _as_pg_model(model, chnls)
    except (TypeError, ValueError) as e:
        raise LfBm5dError(f"lfbm5d_pg_scale: {e}")
    if m is None or lib().lfbm5d_pg_scale(C.byref(m), int(chnls), C.byref(s)) != 0:
        raise LfBm5dError("lfbm5d_pg_scale: bad model (every channel needs a >= 0 and 3/8 a^2 + b > 0, finite; chnls 1 or 3)")
    return s.value


def impulse_scale(hist):
    """lfbm5d_impulse_scale (host only, no GPU): the 0.5 quantile of one ROAD histogram hist uint64 [386], interpolated inside its bin
    (include/lfbm5d.h has the definition).  Raises LfBm5dError on an empty histogram."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.shape != (IMPULSE_KEYS,):
        raise LfBm5dError("lfbm5d_impulse_scale: hist must be [386]")
    s = C.c_double()
    if lib().lfbm5d_impulse_scale(h.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(s)) != 0:
        raise LfBm5dError("lfbm5d_impulse_scale: the histogram is empty")
    return s.value


def impulse_params(k=8.0, min_threshold=0.0, threshold=None):
    """lfbm5d_impulse_params from the defaults of the library; threshold: a scalar (every channel) or a per-channel sequence."""
    P = ImpulseParamsStruct()
    lib().lfbm5d_impulse_defaults(C.byref(P))
    P.k, P.min_threshold = float(k), float(min_threshold)
    if threshold is not None:
        t = np.atleast_1d(np.asarray(threshold, np.float64))
        if t.size not in (1, 3):
            raise LfBm5dError("impulse repair: threshold must be a scalar or hold one value per channel")
        for c in range(3):
            P.threshold[c] = float(t[c if t.size == 3 else 0])
    return P


def inpaint_params(iterations=None, sigma_start=None, sigma_end=None, sigma_noise=None):
    """lfbm5d_inpaint_params from the defaults of the library (lfbm5d_inpaint_defaults); None keeps a default."""
    P = InpaintParamsStruct()
    lib().lfbm5d_inpaint_defaults(C.byref(P))
    if iterations is not None:
        P.iterations = int(iterations)
    if sigma_start is not None:
        P.sigma_start = float(sigma_start)
    if sigma_end is not None:
        P.sigma_end = float(sigma_end)
    if sigma_noise is not None:
        P.sigma_noise = float(sigma_noise)
    return P


def view_params(max_disparity=None, box_radius=None, ang_radius=None, iterations=None, sigma_start=None, sigma_end=None,
                sigma_noise=None):
    """lfbm5d_view_params from the defaults of the library (lfbm5d_view_defaults, host only); None keeps a default."""
    P = ViewParamsStruct()
    lib().lfbm5d_view_defaults(C.byref(P))
    for name, v in (("max_disparity", max_disparity), ("box_radius", box_radius), ("ang_radius", ang_radius), ("iterations", iterations)):
        if v is not None:
            setattr(P, name, int(v))
    for name, v in (("sigma_start", sigma_start), ("sigma_end", sigma_end), ("sigma_noise", sigma_noise)):
        if v is not None:
            setattr(P, name, float(v))
    return P


def repair_params(max_disparity=None, box_radius=None, ang_radius=None, min_valid=None, iterations=None, sigma_start=None, sigma_end=None,
                  sigma_noise=None):
    """lfbm5d_repair_params from the defaults of the library (lfbm5d_repair_defaults, host only); None keeps a default."""
    P = RepairParamsStruct()
    lib().lfbm5d_repair_defaults(C.byref(P))
    for name, v in (("max_disparity", max_disparity), ("box_radius", box_radius), ("ang_radius", ang_radius), ("min_valid", min_valid),
                    ("iterations", iterations)):
        if v is not None:
            setattr(P, name, int(v))
    for name, v in (("sigma_start", sigma_start), ("sigma_end", sigma_end), ("sigma_noise", sigma_noise)):
        if v is not None:
            setattr(P, name, float(v))
    return P


def consist_params(max_disparity=None, box_radius=None, ang_radius=None, min_sources=None, max_rounds=None, k=None, min_threshold=None,
                   spread=None, sai_factor=None, min_scale=None):
    """lfbm5d_consist_params from the defaults of the library (lfbm5d_consist_defaults, host only); None keeps a default."""
    P = ConsistParamsStruct()
    lib().lfbm5d_consist_defaults(C.byref(P))
    for name, v in (("max_disparity", max_disparity), ("box_radius", box_radius), ("ang_radius", ang_radius), ("min_sources", min_sources),
                    ("max_rounds", max_rounds)):
        if v is not None:
            setattr(P, name, int(v))
    for name, v in (("k", k), ("min_threshold", min_threshold), ("spread", spread), ("sai_factor", sai_factor), ("min_scale", min_scale)):
        if v is not None:
            setattr(P, name, float(v))
    return P


def photo_params(max_disparity=None, box_radius=None, ang_radius=None, steps=None, min_sources=None, max_rounds=None, per_channel=None,
                 anchor=None, min_count=None, tol=None, lo=None, hi=None):
    """lfbm5d_photo_params from the defaults of the library (lfbm5d_photo_defaults, host only); None keeps a default (anchor: none)."""
    P = PhotoParamsStruct()
    lib().lfbm5d_photo_defaults(C.byref(P))
    for name, v in (("max_disparity", max_disparity), ("box_radius", box_radius), ("ang_radius", ang_radius), ("steps", steps),
                    ("min_sources", min_sources), ("max_rounds", max_rounds), ("per_channel", per_channel), ("anchor", anchor),
                    ("min_count", min_count)):
        if v is not None:
            setattr(P, name, int(v))
    for name, v in (("tol", tol), ("lo", lo), ("hi", hi)):
        if v is not None:
            setattr(P, name, float(v))
    return P


def photo_edges():
    """lfbm5d_photo_edges (host only): the 1025 edges of the ratio keys, float32, 256 per octave over 1/4..4."""
    e = np.zeros(PHOTO_EDGES, np.float32)
    lib().lfbm5d_photo_edges(e.ctypes.data_as(C.POINTER(C.c_float)))
    return e


def photo_ratio(hist, min_count=1):
    """lfbm5d_photo_ratio (host only, no GPU): (r, fitted) of one ratio histogram hist uint64 [1026]: the median ratio interpolated
    inside its key; (1.0, False) when the histogram holds fewer than min_count values or its median lies in an end key."""
    h = np.ascontiguousarray(np.asarray(hist, np.uint64).reshape(-1))
    if h.size != PHOTO_KEYS:
        raise LfBm5dError("lfbm5d_photo_ratio: hist must be [1026]")
    r = C.c_double(0.0)
    rc = lib().lfbm5d_photo_ratio(h.ctypes.data_as(C.POINTER(C.c_ulonglong)), int(min_count), C.byref(r))
    return r.value, rc == 0


def photo_solve(r, neighbours, fitted, anchor=None):
    """lfbm5d_photo_solve (host only, no GPU): the gains g float64 [asize] from the ratios r [asize], neighbours[m] the source SAIs of
    m in order (looked at for fitted m only), fitted [asize]; anchor: the SAI whose gain stays 1 (None: the lower median is 1)."""
    r = np.ascontiguousarray(np.asarray(r, np.float64).reshape(-1))
    A = r.size
    fit = _u32(np.asarray(fitted).reshape(-1) != 0)
    n_src, src = np.zeros(A, np.uint32), np.zeros((A, PHOTO_MAX_SOURCES), np.uint32)
    for m in range(A):
        if not fit[m]:
            continue
        q = [int(v) for v in neighbours[m]]
        if not 1 <= len(q) <= PHOTO_MAX_SOURCES:
            raise LfBm5dError("lfbm5d_photo_solve: a fitted SAI needs 1..24 sources")
        n_src[m] = len(q)
        src[m, :len(q)] = q
    g = np.zeros(A, np.float64)
    up, dp = C.POINTER(C.c_uint), C.POINTER(C.c_double)
    if lib().lfbm5d_photo_solve(A, r.ctypes.data_as(dp), n_src.ctypes.data_as(up), src.ctypes.data_as(up), fit.ctypes.data_as(up),
                                PHOTO_NO_ANCHOR if anchor is None else int(anchor), g.ctypes.data_as(dp)) != 0:
        raise LfBm5dError("lfbm5d_photo_solve: fitted needs [asize] entries, every source and the anchor an index below asize")
    return g


def window_sigma(sigma_sai, awidth, aheight, ps, pt, an=1, ang_major=None, mask=None):
    """The sigma of the angular window of half size `an` around SAI (ps, pt) under the view table `sigma_sai` [aheight * awidth], one noise
    level per SAI (lfbm5d_views_window_sigma, include/lfbm5d_views.h): the table's value if the window's non-empty SAIs share one, else
    the root mean square of theirs.  Host only, needs no GPU.  Returns a numpy float32."""
    t = np.ascontiguousarray(np.asarray(sigma_sai, dtype=np.float64).reshape(-1))
    if t.size != int(awidth) * int(aheight):
        raise LfBm5dError("window_sigma: the view table needs one value per SAI")
    m = None if mask is None else _u32(mask)
    out = C.c_float()
    if lib().lfbm5d_views_window_sigma(t.ctypes.data_as(C.POINTER(C.c_double)), None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint)),
                                       ROWMAJOR if ang_major is None else ang_major, int(awidth), int(aheight), int(ps), int(pt), int(an),
                                       C.byref(out)) != 0:
        raise LfBm5dError(lib().lfbm5d_views_error().decode())
    return np.float32(out.value)


def views_from_gains(sigma, gain, mask=None):
    """The view table photometric equalisation leaves behind: sigma_v = sigma sqrt(mean_c g[v][c]^-2) for the gains `gain` [asize] or
    [asize][C] it divided out (lfbm5d_views_from_gains, include/lfbm5d_views.h; Equalise.gain holds them).  Host only, needs no GPU.
    Returns float64 [asize], 0 for empty SAIs."""
    g = np.asarray(gain, dtype=np.float64)
    if g.ndim == 1:
        g = g[:, None]
    if g.ndim != 2 or not 1 <= g.shape[1] <= 3:
        raise LfBm5dError("views_from_gains: gains must be [asize] or [asize][C] with C = 1..3")
    g = np.ascontiguousarray(g.astype(np.float32))
    m = None if mask is None else _u32(mask)
    if m is not None and m.size != g.shape[0]:
        raise LfBm5dError("views_from_gains: the mask needs one value per SAI")
    out = np.zeros(max(g.shape[0], 1), np.float64)
    if lib().lfbm5d_views_from_gains(float(sigma), g.ctypes.data_as(C.POINTER(C.c_float)), g.shape[1],
                                     None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint)), g.shape[0],
                                     out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise LfBm5dError(lib().lfbm5d_views_error().decode())
    return out[:g.shape[0]]


CORR_WHITE = np.zeros((7, 7), np.float64)
CORR_WHITE[3, 3] = 1.0
CORR_WHITE.setflags(write=False)


def _acf49(acf):
    a = np.ascontiguousarray(np.asarray(acf, dtype=np.float64).reshape(-1))
    if a.size != 49:
        raise LfBm5dError("an autocorrelation holds 7 x 7 values (lags -3..3)")
    return a


def corr_from_kernel(taps):
    """The autocorrelation [7][7] of white noise filtered by `taps` (up to 7 x 7; a demosaicking or resampling kernel), 1 at lag 0
    (lfbm5d_corr_from_kernel, include/lfbm5d_corr.h).  Host only, needs no GPU."""
    g = np.ascontiguousarray(np.atleast_2d(np.asarray(taps, dtype=np.float64)))
    if g.ndim != 2:
        raise LfBm5dError("corr_from_kernel: the taps are a 2-D array of up to 7 x 7 values")
    out = np.zeros(49, np.float64)
    dp = C.POINTER(C.c_double)
    if lib().lfbm5d_corr_from_kernel(g.ctypes.data_as(dp), g.shape[0], g.shape[1], out.ctypes.data_as(dp)) != 0:
        raise LfBm5dError(lib().lfbm5d_corr_error().decode())
    return out.reshape(7, 7)


def corr_table(acf, tau_2D, k):
    """(s, v, clamped): the variance factor v [k*k] of every coefficient of the 2-D transform tau_2D (ID, DCT, BIOR or their names) on
    k x k patches under noise of autocorrelation `acf`, s = sqrt(v), both float32 as the kernels take them, and the number of
    entries raised to the floor 1 / 64 (lfbm5d_corr_table, include/lfbm5d_corr.h).  Host only, needs no GPU."""
    a = _acf49(acf)
    k = int(k)
    n = k * k if 2 <= k <= 32 else 1
    s, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    cl = C.c_uint(0)
    tau = TAU[tau_2D] if isinstance(tau_2D, str) else int(tau_2D)
    fp = C.POINTER(C.c_float)
    if lib().lfbm5d_corr_table(a.ctypes.data_as(C.POINTER(C.c_double)), tau, k, s.ctypes.data_as(fp), v.ctypes.data_as(fp), C.byref(cl)) != 0:
        raise LfBm5dError(lib().lfbm5d_corr_error().decode())
    return s, v, int(cl.value)


def sr_defaults(scale, /, **changes):
    """lfbm5d_sr_defaults (host only): the SrParams the library starts from for `scale`; keyword arguments replace fields
    (kernel may be "bicubic" / "gaussian")."""
    sr = SrParams()
    if lib().lfbm5d_sr_defaults(int(scale), C.byref(sr)) != 0:
        raise LfBm5dError("lfbm5d_sr_defaults: scale must be 2, 3 or 4")
    for k, v in changes.items():
        if k == "kernel" and isinstance(v, str):
            v = SR_KERNEL[v]
        if k not in dict(SrParams._fields_):
            raise LfBm5dError(f"SrParams has no field {k}")
        setattr(sr, k, v)
    return sr


def sr_taps(op, sr, n_in):
    """lfbm5d_sr_taps (host only, no GPU): (first int32 [n_out], w float32 [n_out][T]) of the 1-D operator `op` (SR_UP / SR_DOWN or
    "up" / "down") for n_in input samples."""
    op = {"up": SR_UP, "down": SR_DOWN}.get(op, op)
    T = C.c_uint(0)
    if lib().lfbm5d_sr_taps(int(op), C.byref(sr), int(n_in), None, None, C.byref(T), 0) != 0:
        raise LfBm5dError("lfbm5d_sr_taps: rejected parameters (scale, kernel, blur_sigma, n_in)")
    n_out = int(n_in) * sr.scale if op == SR_UP else int(n_in) // sr.scale
    first, w = np.zeros(n_out, np.int32), np.zeros((n_out, T.value), np.float32)
    if lib().lfbm5d_sr_taps(int(op), C.byref(sr), int(n_in), first.ctypes.data, w.ctypes.data, C.byref(T), w.size) != 0:
        raise LfBm5dError("lfbm5d_sr_taps failed")
    return first, w


def shard_rows(n_rows, rank, world):
    b, e = C.c_uint(), C.c_uint()
    lib().lfbm5d_shard_rows(n_rows, rank, world, C.byref(b), C.byref(e))
    return b.value, e.value


def make_params(sigma, lam, N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D, useSD=0, color_space=OPP):
    t = lambda v: TAU[v] if isinstance(v, str) else int(v)
    cs = COLOR_SPACE[color_space] if isinstance(color_space, str) else int(color_space)
    return Params(float(sigma), float(lam), int(N), int(nSim), int(nDisp), int(k), int(p),
                  int(bool(useSD)), t(tau_2D), t(tau_4D), t(tau_5D), cs)


def make_bm3d_params(sigma, lam, N, nHW, k, p, tau_2D, useSD=0, color_space=OPP):
    cs = COLOR_SPACE[color_space] if isinstance(color_space, str) else int(color_space)
    return Bm3dParams(float(sigma), float(lam), int(N), int(nHW), int(k), int(p), int(bool(useSD)),
                      TAU[tau_2D] if isinstance(tau_2D, str) else int(tau_2D), cs)


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


# what a plane's element type is called in the two messages below: float32 values, uint8 flags, int8 disparities
_PLANES = {np.float32: ("device entry points need contiguous float32 CUDA tensors",
                        "per-SAI host buffers must be contiguous float32 numpy arrays"),
           np.uint8: ("flag planes on the device must be contiguous uint8 CUDA tensors",
                      "per-SAI host flag planes must be contiguous uint8 numpy arrays"),
           np.int8: ("disparity planes on the device must be contiguous int8 CUDA tensors",
                     "per-SAI host disparity planes must be contiguous int8 numpy arrays")}


def _dev_ptr(t, dtype=np.float32):
    """Raw device pointer of a contiguous CUDA tensor of `dtype` (np.float32: values, np.uint8: flag planes, np.int8: disparity
    planes).  The library launches on the context's own stream and knows nothing about torch's: work torch has queued on the tensor's
    device (a zero-fill, a copy) must have finished before the library reads the buffer, so the current torch stream is drained here
    (include/lfbm5d.h: "buffers are ready on entry, results complete on return")."""
    import torch
    dtype = np.dtype(dtype).type
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, np.dtype(dtype).name) and t.is_contiguous()):
        raise LfBm5dError(_PLANES[dtype][0])
    torch.cuda.current_stream(t.device).synchronize()
    return C.c_void_p(t.data_ptr())


def _sai_ptrs(arrays, mask, dtype=np.float32):
    """dtype*[asize] over a list of per-SAI arrays of `dtype` (entries of empty SAIs may be None)."""
    dtype = np.dtype(dtype).type
    out = (C.c_void_p * len(arrays))()
    for i, a in enumerate(arrays):
        if a is None or not mask[i]:
            continue
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous):
            raise LfBm5dError(_PLANES[dtype][1])
        out[i] = a.ctypes.data
    return out


# The library's run-time options (lfbm5d_amd/csrc/lfbm5d_options.h) and the environment variables they came from: the library
# reads the environment ONCE, at lfbm5d_create; afterwards options change through lfbm5d_set_option.  This Python mirror keeps
# the old convenience -- os.environ["LFBM5D_LANES"] = "3" between two calls on one Context takes effect -- by handing changed
# variables to lfbm5d_set_option before every library call (Context._h).
OPTION_ENV = ("LFBM5D_LANES", "LFBM5D_EMULATE_WORLD", "LFBM5D_MAX_WINDOWS", "LFBM5D_FUSED", "LFBM5D_STEP_SHARDING",
              "LFBM5D_DATA_DRIVEN_SCHEDULE", "LFBM5D_HOST_BLOCKING", "LFBM5D_BAND_MB", "LFBM5D_BM3D_LANES", "LFBM5D_SCAN_LDS_CAP",
              "LFBM5D_FORCE_REDO", "LFBM5D_SPATIAL_BANDS", "LFBM5D_BAND_HALO", "LFBM5D_SCAN_V1", "LFBM5D_SCAN_ANY", "LFBM5D_SCAN_FULL_TABLES", "LFBM5D_DCT8W_V2",
              "LFBM5D_GROUP_GENERIC", "LFBM5D_NO_SA_KERNELS", "LFBM5D_NO_SLAB_KERNEL", "LFBM5D_WIDE_NOSPLIT", "LFBM5D_AGG_64BIT",
              "LFBM5D_AGG_SCALAR_SCAN", "LFBM5D_SUBSET_LIST_HOST", "LFBM5D_SUBSET_SCAN_V1", "LFBM5D_FILT_GROUP_MAJOR",
              "LFBM5D_HT_REF_ORDER", "LFBM5D_WINDOW_SUMS_PADDED", "LFBM5D_SELECT_PREFILL")
# ... of these, the ones whose empty value means "off" (the others keep rounds 1-5's reading: present = set)
OPTION_ENV_EMPTY_OFF = ("LFBM5D_WINDOW_SUMS_PADDED",)


class Context:
    """lfbm5d_ctx: one per process / GPU."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        if self._L.lfbm5d_create(C.byref(h), int(device)) != 0:
            raise LfBm5dError(self._L.lfbm5d_last_error(None).decode())
        self._handle = h
        self._env_seen = {k: os.environ.get(k) for k in OPTION_ENV}   # what lfbm5d_create has just read
        self.device = int(device)

    @property
    def _h(self):
        """The context handle, with the options brought up to date with the environment (see OPTION_ENV)."""
        h = self._handle
        if h and hasattr(self._L, "lfbm5d_set_option"):
            for k in OPTION_ENV:
                v = os.environ.get(k)
                if v != self._env_seen[k]:
                    self._env_seen[k] = v
                    # a variable that is present but empty counted as "set" for the presence flags
                    if not v and k in OPTION_ENV_EMPTY_OFF:
                        v = None
                    self._L.lfbm5d_set_option(h, k.encode(), None if v is None else (v or "1").encode())
        return h

    def set_option(self, key, value):
        """lfbm5d_set_option: `key` as in lfbm5d_options.h ("lanes", "step_sharding", ...; the old variable names work too); None
        resets it to its default."""
        if self._L.lfbm5d_set_option(self._handle, key.encode(), None if value is None else str(value).encode()) != 0:
            raise LfBm5dError(self._L.lfbm5d_last_error(self._handle).decode())

    def get_option(self, key):
        buf = C.create_string_buffer(64)
        if self._L.lfbm5d_get_option(self._handle, key.encode(), buf, 64) != 0:
            raise LfBm5dError(self._L.lfbm5d_last_error(self._handle).decode())
        return buf.value.decode()

    def close(self):
        if getattr(self, "_handle", None):
            self._L.lfbm5d_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise LfBm5dError(self._L.lfbm5d_last_error(self._h).decode())

    # ---- multi-GPU ----
    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
        if lib().lfbm5d_comm_unique_id(buf) != 0:
            raise LfBm5dError("ncclGetUniqueId failed")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._ck(self._L.lfbm5d_comm_init(self._h, buf, rank, world))

    def comm_init_ipc(self, rank, world, rendezvous_dir, timeout_s=30.0):
        """Tests only: this process is rank `rank` of `world` processes sharing ONE GPU; the window graph's messages travel through
        IPC-mapped device buffers instead of RCCL (include/lfbm5d.h)."""
        self._ck(self._L.lfbm5d_comm_init_ipc(self._h, rank, world, os.fsencode(rendezvous_dir), float(timeout_s)))

    def comm_selftest(self, n=1 << 20):
        """All-reduce n floats through RCCL on the context's stream and check the sums."""
        self._ck(self._L.lfbm5d_comm_selftest(self._h, n))

    def comm_ranks(self):
        """Ranks of the RCCL communicator as RCCL counts them (0: none)."""
        return int(self._L.lfbm5d_comm_ranks(self._h))

    def set_shard(self, rank, world):
        self._ck(self._L.lfbm5d_set_shard(self._h, rank, world))

    def set_tiles(self, nb_tiles):
        """The reference's tile mode (run_bm5d_* with nb_threads > 1) for whole steps; 0 / 1 switches it off."""
        self._ck(self._L.lfbm5d_set_tiles(self._h, int(nb_tiles)))

    # ---- stats ----
    def reset_stats(self):
        self._L.lfbm5d_reset_stats(self._h)

    def stats(self):
        s = Stats()
        self._L.lfbm5d_get_stats(self._h, C.byref(s))
        return s

    def stream(self):
        return self._L.lfbm5d_stream(self._h)

    # ---- outer seam ----
    def step1(self, P, noisy, mask, basic, ang_major, awidth, aheight, an, W, H, Cc):
        """run_bm5d_1st_step on device tensors (torch CUDA) or host arrays (numpy float32)."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        tail = (ang_major, awidth, aheight, an, W, H, Cc)
        if isinstance(noisy, (list, tuple)):   # one float32 array per SAI, like the reference's vector<vector<float>>
            self._ck(self._L.lfbm5d_step1_host_sai(self._h, C.byref(P), _sai_ptrs(noisy, m), mp, _sai_ptrs(basic, m), *tail))
        elif isinstance(noisy, np.ndarray):
            self._ck(self._L.lfbm5d_step1_host(self._h, C.byref(P), noisy.ctypes.data_as(C.c_void_p), mp,
                                               basic.ctypes.data_as(C.c_void_p), *tail))
        else:
            self._ck(self._L.lfbm5d_step1_device(self._h, C.byref(P), _dev_ptr(noisy), mp, _dev_ptr(basic), *tail))

    def step2(self, P, noisy, mask, basic, denoised, ang_major, awidth, aheight, an, W, H, Cc):
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        tail = (ang_major, awidth, aheight, an, W, H, Cc)
        if isinstance(noisy, (list, tuple)):
            self._ck(self._L.lfbm5d_step2_host_sai(self._h, C.byref(P), _sai_ptrs(noisy, m), mp, _sai_ptrs(basic, m), _sai_ptrs(denoised, m), *tail))
        elif isinstance(noisy, np.ndarray):
            self._ck(self._L.lfbm5d_step2_host(self._h, C.byref(P), noisy.ctypes.data_as(C.c_void_p), mp,
                                               basic.ctypes.data_as(C.c_void_p),
                                               denoised.ctypes.data_as(C.c_void_p), *tail))
        else:
            self._ck(self._L.lfbm5d_step2_device(self._h, C.byref(P), _dev_ptr(noisy), mp, _dev_ptr(basic),
                                                 _dev_ptr(denoised), *tail))

    def denoise(self, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, Cc):
        """run_bm5d_1st_step + run_bm5d_2nd_step as one job (lfbm5d_denoise_*): bit-identical to step1() followed by step2()."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        tail = (ang_major, awidth, aheight, an1, an2, W, H, Cc)
        if isinstance(noisy, (list, tuple)):
            self._ck(self._L.lfbm5d_denoise_host_sai(self._h, C.byref(P1), C.byref(P2), _sai_ptrs(noisy, m), mp, _sai_ptrs(basic, m),
                                                     _sai_ptrs(denoised, m), *tail))
        elif isinstance(noisy, np.ndarray):
            self._ck(self._L.lfbm5d_denoise_host(self._h, C.byref(P1), C.byref(P2), noisy.ctypes.data_as(C.c_void_p), mp,
                                                 basic.ctypes.data_as(C.c_void_p), denoised.ctypes.data_as(C.c_void_p), *tail))
        else:
            self._ck(self._L.lfbm5d_denoise_device(self._h, C.byref(P1), C.byref(P2), _dev_ptr(noisy), mp, _dev_ptr(basic),
                                                   _dev_ptr(denoised), *tail))

    # ---- per-view noise levels (include/lfbm5d_views.h) ----
    @staticmethod
    def _view_table(sigma_sai, asize):
        """(the table or NULL, the buffer the applied table is written to) of a *_views_* call."""
        dp = C.POINTER(C.c_double)
        used = np.zeros(max(asize, 1), np.float64)
        if sigma_sai is None:
            return None, None, used
        t = np.ascontiguousarray(np.asarray(sigma_sai, dtype=np.float64).reshape(-1))
        if t.size != asize:
            raise LfBm5dError("the view table needs one value per SAI")
        return t, t.ctypes.data_as(dp), used

    def denoise_views(self, sigma_sai, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, Cc):
        """denoise() with one noise level per SAI (lfbm5d_denoise_views_*): every angular window runs with its window sigma
        (window_sigma(); P1.sigma / P2.sigma are ignored).  sigma_sai: [asize] in the units of sigma, or None: the per-SAI estimate
        noise_level(..., per_sai=True) of `noisy` is taken first.  CUDA float32 tensors (device form), or float32 numpy arrays /
        lists of per-SAI arrays (host form, in / out like denoise(); bit-identical).  Returns the table that was applied, float64
        [asize] (0 for empty SAIs)."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        t, tp, used = self._view_table(sigma_sai, m.size)
        head = (self._h, tp, used.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P1), C.byref(P2))
        tail = (ang_major, awidth, aheight, an1, an2, int(W), int(H), int(Cc))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            n, b, d = (self._host_sais(x) for x in (noisy, basic, denoised))
            self._ck(self._L.lfbm5d_denoise_views_host_sai(*head, _sai_ptrs(n, m), mp, _sai_ptrs(b, m), _sai_ptrs(d, m), *tail))
        else:
            self._ck(self._L.lfbm5d_denoise_views_device(*head, _dev_ptr(noisy), mp, _dev_ptr(basic), _dev_ptr(denoised), *tail))
        return used[:m.size]

    def step1_views(self, sigma_sai, P, noisy, mask, basic, ang_major, awidth, aheight, an, W, H, Cc):
        """step1() with a view table (lfbm5d_step1_views_device; CUDA tensors): see denoise_views().  Returns the table applied."""
        m = _u32(mask)
        t, tp, used = self._view_table(sigma_sai, m.size)
        self._ck(self._L.lfbm5d_step1_views_device(self._h, tp, used.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P), _dev_ptr(noisy),
                                                   m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(basic), ang_major, awidth, aheight, an,
                                                   int(W), int(H), int(Cc)))
        return used[:m.size]

    def step2_views(self, sigma_sai, P, noisy, mask, basic, denoised, ang_major, awidth, aheight, an, W, H, Cc):
        """step2() with a view table (lfbm5d_step2_views_device; CUDA tensors): see denoise_views().  Returns the table applied."""
        m = _u32(mask)
        t, tp, used = self._view_table(sigma_sai, m.size)
        self._ck(self._L.lfbm5d_step2_views_device(self._h, tp, used.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P), _dev_ptr(noisy),
                                                   m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(basic), _dev_ptr(denoised), ang_major,
                                                   awidth, aheight, an, int(W), int(H), int(Cc)))
        return used[:m.size]

    # ---- spatially correlated noise (include/lfbm5d_corr.h) ----
    def corr_measure(self, LF, LF_SAI_mask, width, height, chnls, block=16, fraction=None):
        """The autocorrelation of the noise at the lags -3..3 from the block autocovariance of `LF` (lfbm5d_corr_measure_*).
        fraction = 1 on a flat-field or dark-frame light field (or the difference of two captures): the calibration.  A small
        fraction (None: the default, 0.1) on the noisy light field itself: the blind estimate from its flattest blocks; its sigma is
        biased low.  LF: a CUDA float32 tensor [asize][C*H*W] (device form, read only), a float32 numpy array of that shape or a
        list of per-SAI float32 arrays (host form, staged through HBM; bit-identical).  Returns a CorrEstimate."""
        m = _u32(LF_SAI_mask)
        res = CorrEstimateStruct()
        tail = (m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width), int(height), int(chnls), int(block),
                0.0 if fraction is None else float(fraction), C.byref(res))
        if fraction is not None and float(fraction) == 0.0:
            raise LfBm5dError("corr_measure: fraction must be in (0, 1] (None = the default)")
        if isinstance(LF, (list, tuple, np.ndarray)):
            self._ck(self._L.lfbm5d_corr_measure_host_sai(self._h, _sai_ptrs(self._host_sais(LF), m), *tail))
        else:
            self._ck(self._L.lfbm5d_corr_measure_device(self._h, _dev_ptr(LF), *tail))
        return CorrEstimate(np.array(res.acf, np.float64).reshape(7, 7), float(res.sigma), int(res.blocks), int(res.selected),
                            float(res.cut), int(res.block))

    def denoise_corr(self, acf, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, Cc):
        """denoise() under noise of autocorrelation `acf` [7][7] (lfbm5d_denoise_corr_*): every 2-D coefficient is thresholded and
        Wiener-shrunk with its own variance factor (corr_table); P1.sigma / P2.sigma stay the marginal level.  General group kernels
        only; with the white autocorrelation bit-identical to denoise() under option group_generic.  CUDA float32 tensors (device
        form), or float32 numpy arrays / lists of per-SAI arrays (host form, in / out like denoise(); bit-identical)."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        a = _acf49(acf)
        head = (self._h, a.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P1), C.byref(P2))
        tail = (ang_major, awidth, aheight, an1, an2, int(W), int(H), int(Cc))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            n, b, d = (self._host_sais(x) for x in (noisy, basic, denoised))
            self._ck(self._L.lfbm5d_denoise_corr_host_sai(*head, _sai_ptrs(n, m), mp, _sai_ptrs(b, m), _sai_ptrs(d, m), *tail))
        else:
            self._ck(self._L.lfbm5d_denoise_corr_device(*head, _dev_ptr(noisy), mp, _dev_ptr(basic), _dev_ptr(denoised), *tail))

    def step1_corr(self, acf, P, noisy, mask, basic, ang_major, awidth, aheight, an, W, H, Cc):
        """step1() under noise of autocorrelation `acf` (lfbm5d_step1_corr_device; CUDA tensors): see denoise_corr()."""
        m = _u32(mask)
        a = _acf49(acf)
        self._ck(self._L.lfbm5d_step1_corr_device(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P), _dev_ptr(noisy),
                                                  m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(basic), ang_major, awidth, aheight, an,
                                                  int(W), int(H), int(Cc)))

    def step2_corr(self, acf, P, noisy, mask, basic, denoised, ang_major, awidth, aheight, an, W, H, Cc):
        """step2() under noise of autocorrelation `acf` (lfbm5d_step2_corr_device; CUDA tensors): see denoise_corr()."""
        m = _u32(mask)
        a = _acf49(acf)
        self._ck(self._L.lfbm5d_step2_corr_device(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P), _dev_ptr(noisy),
                                                  m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(basic), _dev_ptr(denoised), ang_major,
                                                  awidth, aheight, an, int(W), int(H), int(Cc)))

    def debug_group_corr(self, acf, *args, **kw):
        """lfbm5d_debug_group_corr: debug_group() with the variance table of `acf` -- the general kernels' table forms alone."""
        return self.debug_group(*args, _acf=_acf49(acf), **kw)

    def bm3d_lf_views(self, sigma_sai, hard, wien, noisy, mask, basic, denoised, W, H, Cc):
        """bm3d_lf() with a view table (lfbm5d_bm3d_lf_views_device; CUDA tensors): SAI v is filtered with sigma_sai[v] in both steps
        (hard.sigma / wien.sigma are ignored).  Returns the table applied."""
        m = _u32(mask)
        t, tp, used = self._view_table(sigma_sai, m.size)
        self._ck(self._L.lfbm5d_bm3d_lf_views_device(self._h, tp, used.ctypes.data_as(C.POINTER(C.c_double)), C.byref(hard), C.byref(wien),
                                                     _dev_ptr(noisy), m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(basic),
                                                     _dev_ptr(denoised), m.size, int(W), int(H), int(Cc)))
        return used[:m.size]

    def last_window_sigmas(self):
        """The sigma applied to every window of the last step / denoise job, in the order of last_windows() (float32)."""
        n = self._L.lfbm5d_last_window_sigmas(self._h, None, 0)
        out = np.zeros(max(n, 1), np.float32)
        self._L.lfbm5d_last_window_sigmas(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
        return out[:max(n, 0)].copy()

    # ---- inner seam ----
    def core_pass(self, step, P, aw, ah, Wb, Hb, Cc, noisy, basic, num, den, mask, procSAI, cst, pst):
        """bm5d_1st_step / bm5d_2nd_step on a padded window held in CUDA tensors."""
        m, pr = _u32(mask), _u32(procSAI)
        self._ck(self._L.lfbm5d_pass_device(
            self._h, step, C.byref(P), aw, ah, Wb, Hb, Cc, _dev_ptr(noisy),
            _dev_ptr(basic) if basic is not None else None, _dev_ptr(num), _dev_ptr(den),
            m.ctypes.data_as(C.POINTER(C.c_uint)), pr.ctypes.data_as(C.POINTER(C.c_uint)), cst, pst))

    # ---- per-SAI BM3D (LFBM3Ddenoising) ----
    def bm3d_step(self, step, P, Wb, Hb, Cc, noisy, basic, out):
        """bm3d_1st_step / bm3d_2nd_step on a mirror-padded image held in CUDA tensors; out = num / den."""
        self._ck(self._L.lfbm5d_bm3d_step_device(self._h, step, C.byref(P), Wb, Hb, Cc, _dev_ptr(noisy),
                                                 _dev_ptr(basic) if basic is not None else None, _dev_ptr(out)))

    def bm3d_lf(self, hard, wien, noisy, mask, basic, denoised, W, H, Cc):
        """run_bm3d_LF on device tensors (torch CUDA) or host arrays (numpy float32), [asize][C*H*W]."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        if isinstance(noisy, np.ndarray):
            self._ck(self._L.lfbm5d_bm3d_lf_host(self._h, C.byref(hard), C.byref(wien), noisy.ctypes.data_as(C.c_void_p), mp,
                                                 basic.ctypes.data_as(C.c_void_p), denoised.ctypes.data_as(C.c_void_p),
                                                 m.size, W, H, Cc))
        else:
            self._ck(self._L.lfbm5d_bm3d_lf_device(self._h, C.byref(hard), C.byref(wien), _dev_ptr(noisy), mp, _dev_ptr(basic),
                                                   _dev_ptr(denoised), m.size, W, H, Cc))

    # ---- blind noise level ----
    def noise_level(self, LF, LF_SAI_mask, width, height, chnls, patch=8, per_sai=False):
        """Estimate the standard deviation of additive white Gaussian noise (lfbm5d_noise_level_*, include/lfbm5d.h) in the units
        of `sigma`.  LF: a CUDA float32 tensor [asize][C*H*W] (device form, read only), a float32 numpy array of that shape or a
        list of per-SAI float32 arrays (host form, staged through HBM; bit-identical).  Returns a NoiseLevel."""
        m = _u32(LF_SAI_mask)
        asize, C_ = m.size, int(chnls)
        res = NoiseLevelStruct()
        d = int(patch) * int(patch) if 4 <= int(patch) <= 8 else 64
        eig = np.zeros(d, np.float64)
        sai = np.zeros(max(asize, 1), np.float64) if per_sai else None
        dp = C.POINTER(C.c_double)
        tail = (m.ctypes.data_as(C.POINTER(C.c_uint)), asize, int(width), int(height), C_, int(patch), C.byref(res),
                sai.ctypes.data_as(dp) if per_sai else None, eig.ctypes.data_as(dp))
        if isinstance(LF, (list, tuple)) or isinstance(LF, np.ndarray):
            arrays = list(LF) if isinstance(LF, (list, tuple)) else [np.ascontiguousarray(a) for a in LF]
            if isinstance(LF, np.ndarray) and LF.dtype != np.float32:
                raise LfBm5dError("host light fields must be float32")
            self._ck(self._L.lfbm5d_noise_level_host_sai(self._h, _sai_ptrs(arrays, m), *tail))
        else:
            self._ck(self._L.lfbm5d_noise_level_device(self._h, _dev_ptr(LF), *tail))
        return NoiseLevel(res.sigma, tuple(res.sigma_channel[:C_]), int(res.components), int(res.patches), eig[:int(res.patch) ** 2],
                          sai[:asize] if per_sai else None)

    # ---- quality metrics ----
    def quality(self, ref, test, mask, width, height, chnls, peak=255.0, ssim=True):
        """PSNR, RMSE and (ssim=True) SSIM of `test` against `ref`, per SAI and summarised (lfbm5d_quality_*, include/lfbm5d.h).  ref /
        test: CUDA float32 tensors [asize][C*H*W] (device form, read only), or float32 numpy arrays of that shape / lists of per-SAI
        float32 arrays (host form, staged through HBM; bit-identical).  Returns a Quality."""
        m = _u32(mask)
        asize = m.size
        res = QualityStruct()
        mse, ss = np.zeros(max(asize, 1), np.float64), np.zeros(max(asize, 1), np.float64)
        dp = C.POINTER(C.c_double)
        tail = (m.ctypes.data_as(C.POINTER(C.c_uint)), asize, int(width), int(height), int(chnls), float(peak), 1 if ssim else 0,
                C.byref(res), mse.ctypes.data_as(dp), ss.ctypes.data_as(dp))
        host = [isinstance(x, (list, tuple, np.ndarray)) for x in (ref, test)]
        if host[0] != host[1]:
            raise LfBm5dError("quality: ref and test must both be device tensors or both be host arrays")
        if host[0]:
            arrays = []
            for x in (ref, test):
                if isinstance(x, np.ndarray) and x.dtype != np.float32:
                    raise LfBm5dError("host light fields must be float32")
                arrays.append(list(x) if isinstance(x, (list, tuple)) else [np.ascontiguousarray(a) for a in x])
            self._ck(self._L.lfbm5d_quality_host_sai(self._h, _sai_ptrs(arrays[0], m), _sai_ptrs(arrays[1], m), *tail))
        else:
            self._ck(self._L.lfbm5d_quality_device(self._h, _dev_ptr(ref), _dev_ptr(test), *tail))
        return _quality_result(res, mse[:asize], ss[:asize], m, peak)

    # ---- Poisson-Gaussian noise ----
    @staticmethod
    def _host_sais(LF):
        if isinstance(LF, np.ndarray) and LF.dtype != np.float32:
            raise LfBm5dError("host light fields must be float32")
        return list(LF) if isinstance(LF, (list, tuple)) else [np.ascontiguousarray(a) for a in LF]

    # ---- what impulse_repair, inpaint, view_synth and consist share: results to write into, host form or device form ----
    def _host_out(self, arrays, out, m=None, img=0):
        """(out, its per-SAI list): a missing `out` is a copy of the input (img: zeros of that size for a non-empty SAI without one)."""
        if out is None:
            out = [(np.zeros(img, np.float32) if img and m[i] else None) if a is None else np.array(a, np.float32, copy=True)
                   for i, a in enumerate(arrays)]
        return out, self._host_sais(out)

    @staticmethod
    def _host_planes(arrays, given, wanted, dtype, n=None):
        """Optional per-SAI output planes of the host form (flags, disparities): `given`, fresh zeros when only `wanted`, else None.
        n: values per plane (default: shaped like the SAI's array, None where there is none)."""
        if given is not None:
            return list(given)
        if not wanted:
            return None
        return [np.zeros(n, dtype) if n is not None else None if a is None else np.zeros(np.shape(a), dtype) for a in arrays]

    @staticmethod
    def _stacked(noisy, x, like_input=True):
        """A per-SAI list back in the form of a numpy input: one array (like_input: of the input's shape); anything else as it is."""
        if not isinstance(noisy, np.ndarray) or x is None or isinstance(x, np.ndarray):
            return x
        return np.stack(x).reshape(noisy.shape) if like_input else np.stack(x)

    @staticmethod
    def _dev_out(noisy, out, m=None):
        """A missing `out` of the device form: a copy of the input (m: uninitialised when no SAI is empty, every plane is written)."""
        import torch
        if out is not None:
            return out
        return torch.empty_like(noisy) if m is not None and m.all() else noisy.clone()

    @staticmethod
    def _dev_planes(noisy, given, wanted, shape, dtype):
        """Optional output planes of the device form (uint8 flags, int8 disparities): `given`, fresh zeros when only `wanted`, else None."""
        import torch
        if given is None and wanted:
            return torch.zeros(shape, dtype=dtype, device=noisy.device)
        return given

    def pg_histogram(self, LF, LF_SAI_mask, width, height, chnls):
        """The block statistics of lfbm5d_pg_histogram_device on a CUDA float32 tensor [asize][C*H*W]: (hist uint64 [C][64][322],
        sum_m uint64 [C][64], blocks, skipped)."""
        m = _u32(LF_SAI_mask)
        C_ = int(chnls)
        hist, sm = np.zeros((max(C_, 1), PG_LEVELS, PG_KEYS), np.uint64), np.zeros((max(C_, 1), PG_LEVELS), np.uint64)
        blocks, skipped = C.c_ulonglong(), C.c_ulonglong()
        ullp = C.POINTER(C.c_ulonglong)
        self._ck(self._L.lfbm5d_pg_histogram_device(self._h, _dev_ptr(LF), m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width),
                                                    int(height), C_, hist.ctypes.data_as(ullp), sm.ctypes.data_as(ullp),
                                                    C.byref(blocks), C.byref(skipped)))
        return hist, sm, blocks.value, skipped.value

    def pg_estimate(self, LF, LF_SAI_mask, width, height, chnls):
        """Estimate the Poisson-Gaussian model var(z | y) = a y + b of a noisy light field (lfbm5d_pg_estimate_*, include/lfbm5d.h).
        LF: a CUDA float32 tensor [asize][C*H*W] (device form, read only), a float32 numpy array of that shape or a list of per-SAI
        float32 arrays (host form, staged through HBM; identical results).  Returns a PgEstimate."""
        m = _u32(LF_SAI_mask)
        C_ = int(chnls)
        res = PgEstimateStruct()
        hist, sm = np.zeros((max(C_, 1), PG_LEVELS, PG_KEYS), np.uint64), np.zeros((max(C_, 1), PG_LEVELS), np.uint64)
        ullp = C.POINTER(C.c_ulonglong)
        tail = (m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width), int(height), C_, C.byref(res), hist.ctypes.data_as(ullp),
                sm.ctypes.data_as(ullp))
        if isinstance(LF, (list, tuple, np.ndarray)):
            self._ck(self._L.lfbm5d_pg_estimate_host_sai(self._h, _sai_ptrs(self._host_sais(LF), m), *tail))
        else:
            self._ck(self._L.lfbm5d_pg_estimate_device(self._h, _dev_ptr(LF), *tail))
        return PgEstimate(res.a, res.b, tuple(res.a_channel[:C_]), tuple(res.b_channel[:C_]), int(res.blocks), int(res.skipped), hist, sm)

    def pg_forward(self, model, LF, mask, out, width, height, chnls):
        """out = generalised Anscombe transform of LF under `model` (lfbm5d_pg_forward_device): CUDA float32 tensors [asize][C*H*W];
        out may be LF.  Returns the sigma of `out` (pg_scale)."""
        mdl = _as_pg_model(model, int(chnls))
        m = _u32(mask)
        self._ck(self._L.lfbm5d_pg_forward_device(self._h, C.byref(mdl), _dev_ptr(LF), m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(out),
                                                  m.size, int(width), int(height), int(chnls)))
        return pg_scale(mdl, chnls)

    def pg_inverse(self, model, LF, mask, out, width, height, chnls):
        """out = exact unbiased inverse of pg_forward (lfbm5d_pg_inverse_device); out may be LF."""
        mdl = _as_pg_model(model, int(chnls))
        m = _u32(mask)
        self._ck(self._L.lfbm5d_pg_inverse_device(self._h, C.byref(mdl), _dev_ptr(LF), m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(out),
                                                  m.size, int(width), int(height), int(chnls)))

    def denoise_pg(self, model, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, Cc):
        """The two-step job under Poisson-Gaussian noise (lfbm5d_denoise_pg_*): forward transform, denoise() with sigma = the model's
        scale (P1.sigma / P2.sigma are ignored), inverse transform.  model: a PgModelStruct, a PgEstimate, a pair (a, b), or None =
        estimate the pooled model from `noisy`.  noisy is only read.  CUDA float32 tensors (device form), or float32 numpy arrays /
        lists of per-SAI arrays (host form; bit-identical).  Returns the model that was used (PgModelStruct)."""
        mdl = _as_pg_model(model, int(Cc))
        used = PgModelStruct()
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        head = (self._h, C.byref(mdl) if mdl is not None else None, C.byref(used), C.byref(P1), C.byref(P2))
        tail = (ang_major, awidth, aheight, an1, an2, int(W), int(H), int(Cc))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            n, b, d = (self._host_sais(x) for x in (noisy, basic, denoised))
            self._ck(self._L.lfbm5d_denoise_pg_host_sai(*head, _sai_ptrs(n, m), mp, _sai_ptrs(b, m), _sai_ptrs(d, m), *tail))
        else:
            self._ck(self._L.lfbm5d_denoise_pg_device(*head, _dev_ptr(noisy), mp, _dev_ptr(basic), _dev_ptr(denoised), *tail))
        return used

    # ---- clipped data ----
    def clip_histogram(self, LF, LF_SAI_mask, width, height, chnls, lo=0.0, hi=255.0):
        """The block statistics of lfbm5d_clip_histogram_device on a CUDA float32 tensor [asize][C*H*W]: (hist uint64 [C][64][322],
        sum_m uint64 [C][64], cens uint64 [C][64], whole uint64 [C], blocks, skipped)."""
        m = _u32(LF_SAI_mask)
        C_ = int(chnls)
        n = max(C_, 1)
        hist, sm, cens = np.zeros((n, PG_LEVELS, PG_KEYS), np.uint64), np.zeros((n, PG_LEVELS), np.uint64), np.zeros((n, PG_LEVELS), np.uint64)
        whole = np.zeros(n, np.uint64)
        blocks, skipped = C.c_ulonglong(), C.c_ulonglong()
        ullp = C.POINTER(C.c_ulonglong)
        self._ck(self._L.lfbm5d_clip_histogram_device(self._h, _dev_ptr(LF), m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width),
                                                      int(height), C_, float(lo), float(hi), hist.ctypes.data_as(ullp),
                                                      sm.ctypes.data_as(ullp), cens.ctypes.data_as(ullp), whole.ctypes.data_as(ullp),
                                                      C.byref(blocks), C.byref(skipped)))
        return hist, sm, cens, whole, blocks.value, skipped.value

    clip_fit = staticmethod(clip_fit)

    def noise_level_clipped(self, LF, LF_SAI_mask, width, height, chnls, lo=0.0, hi=255.0):
        """The noise sigma of a light field whose values were clipped to lo..hi (8-bit files: 0..255), from the levels the clipping left
        alone (lfbm5d_noise_level_clipped_*, include/lfbm5d.h).  LF: a CUDA float32 tensor [asize][C*H*W] (device form, read only), a
        float32 numpy array of that shape or a list of per-SAI float32 arrays (host form, staged through HBM; identical results).
        Returns a ClipNoiseLevel."""
        m = _u32(LF_SAI_mask)
        C_ = int(chnls)
        res = ClipEstimateStruct()
        tail = (m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width), int(height), C_, float(lo), float(hi), C.byref(res))
        if isinstance(LF, (list, tuple, np.ndarray)):
            self._ck(self._L.lfbm5d_noise_level_clipped_host_sai(self._h, _sai_ptrs(self._host_sais(LF), m), *tail))
        else:
            self._ck(self._L.lfbm5d_noise_level_clipped_device(self._h, _dev_ptr(LF), *tail))
        return _clip_result(res, C_)

    def declip(self, sigma, LF, mask, out, width, height, chnls, lo=0.0, hi=255.0):
        """out = clamp(E^-1(LF), lo, hi), the inverse of the mean of a value clipped to lo..hi under noise of `sigma`
        (lfbm5d_declip_*): what takes a denoised clipped light field back to the unclipped signal.  CUDA float32 tensors
        [asize][C*H*W] (device form), or float32 numpy arrays / lists of per-SAI arrays (host form; bit-identical); out may be LF."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        head = (self._h, float(sigma), float(lo), float(hi))
        tail = (m.size, int(width), int(height), int(chnls))
        if isinstance(LF, (list, tuple, np.ndarray)):
            self._ck(self._L.lfbm5d_declip_host_sai(*head, _sai_ptrs(self._host_sais(LF), m), mp, _sai_ptrs(self._host_sais(out), m), *tail))
        else:
            self._ck(self._L.lfbm5d_declip_device(*head, _dev_ptr(LF), mp, _dev_ptr(out), *tail))

    def denoise_clipped(self, sigma, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, Cc, lo=0.0, hi=255.0):
        """The two-step job on data clipped to lo..hi (lfbm5d_denoise_clipped_*): sigma None (or <= 0): noise_level_clipped() of `noisy`
        first; denoise() with that sigma (P1.sigma / P2.sigma are ignored); declip() of basic and denoised in place.  CUDA float32
        tensors (device form: noisy is left as denoise() leaves it), or float32 numpy arrays / lists of per-SAI arrays (host form:
        noisy is only read; bit-identical).  Returns (the sigma that was applied, the ClipNoiseLevel or None when sigma was given)."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        res, used = ClipEstimateStruct(), C.c_double()
        sig = 0.0 if sigma is None else float(sigma)
        head = (self._h, sig, float(lo), float(hi), C.byref(res), C.byref(used), C.byref(P1), C.byref(P2))
        tail = (ang_major, awidth, aheight, an1, an2, int(W), int(H), int(Cc))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            n, b, d = (self._host_sais(x) for x in (noisy, basic, denoised))
            self._ck(self._L.lfbm5d_denoise_clipped_host_sai(*head, _sai_ptrs(n, m), mp, _sai_ptrs(b, m), _sai_ptrs(d, m), *tail))
        else:
            self._ck(self._L.lfbm5d_denoise_clipped_device(*head, _dev_ptr(noisy), mp, _dev_ptr(basic), _dev_ptr(denoised), *tail))
        return used.value, (_clip_result(res, int(Cc)) if sig <= 0.0 else None)

    # ---- clipped Poisson-Gaussian noise ----
    pgclip_fit = staticmethod(pgclip_fit)
    pgclip_curves = staticmethod(pgclip_curves)

    def pgclip_estimate(self, LF, LF_SAI_mask, width, height, chnls, lo=0.0, hi=255.0):
        """The model sigma^2(y) = a (y - lo) + b of a light field whose values were rounded and clipped to lo..hi, from the levels the
        clipping left alone (lfbm5d_pgclip_estimate_*, include/lfbm5d_pgclip.h).  LF: a CUDA float32 tensor [asize][C*H*W] (device
        form, read only), a float32 numpy array of that shape or a list of per-SAI float32 arrays (host form, staged through HBM;
        identical results).  Returns a PgclipEstimate."""
        m = _u32(LF_SAI_mask)
        C_ = int(chnls)
        res = PgclipEstimateStruct()
        tail = (m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width), int(height), C_, float(lo), float(hi), C.byref(res))
        if isinstance(LF, (list, tuple, np.ndarray)):
            self._ck(self._L.lfbm5d_pgclip_estimate_host_sai(self._h, _sai_ptrs(self._host_sais(LF), m), *tail))
        else:
            self._ck(self._L.lfbm5d_pgclip_estimate_device(self._h, _dev_ptr(LF), *tail))
        return _pgclip_result(res, C_)

    def _pgclip_map(self, fn, curves, LF, mask, out, width, height, chnls):
        m = _u32(mask)
        cv = curves.struct if isinstance(curves, PgclipCurves) else curves
        tail = (m.size, int(width), int(height), int(chnls))
        if isinstance(LF, (list, tuple, np.ndarray)):   # host form: staged through HBM by torch, the result copied back into `out`
            import torch
            arrays, outs = self._host_sais(LF), self._host_sais(out)
            src = np.zeros((m.size, int(chnls) * int(width) * int(height)), np.float32)
            for st in range(m.size):
                if m[st]:
                    src[st] = np.asarray(arrays[st], np.float32).reshape(-1)
            d = torch.from_numpy(src).to(f"cuda:{self.device}")
            self._ck(fn(self._h, C.byref(cv), _dev_ptr(d), m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(d), *tail))
            res = d.cpu().numpy()
            for st in range(m.size):
                if m[st]:
                    outs[st].reshape(-1)[:] = res[st]
        else:
            self._ck(fn(self._h, C.byref(cv), _dev_ptr(LF), m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(out), *tail))

    def pgclip_forward(self, curves, LF, mask, out, width, height, chnls):
        """out = the stabiliser F of pgclip_curves() applied to LF by table look-up (lfbm5d_pgclip_forward_device): CUDA float32
        tensors [asize][C*H*W], or float32 numpy arrays / lists of per-SAI arrays (staged through HBM; bit-identical); out may be LF.
        Planes of empty SAIs are not touched."""
        self._pgclip_map(self._L.lfbm5d_pgclip_forward_device, curves, LF, mask, out, width, height, chnls)

    def pgclip_inverse(self, curves, LF, mask, out, width, height, chnls):
        """out = the exact unbiased inverse G^-1 of pgclip_curves() applied to LF (lfbm5d_pgclip_inverse_device): it undoes the
        stabiliser and the clipping bias in one step; the output lies in lo..hi.  Arguments as for pgclip_forward."""
        self._pgclip_map(self._L.lfbm5d_pgclip_inverse_device, curves, LF, mask, out, width, height, chnls)

    def denoise_pgclip(self, model, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, Cc, lo=0.0, hi=255.0):
        """The two-step job on Poisson-Gaussian data clipped to lo..hi (lfbm5d_denoise_pgclip_*): model None: pgclip_estimate() of
        `noisy` first, else (a, b) or a PgclipEstimate; pgclip_curves(); pgclip_forward() into a scratch light field; denoise() with
        sigma = s (P1.sigma / P2.sigma are ignored); pgclip_inverse() of basic and denoised in place.  CUDA float32 tensors (noisy is
        only read), or float32 numpy arrays / lists of per-SAI arrays (host form; bit-identical).  Returns (the PgclipEstimate of the
        model that was applied -- the fit's when it was estimated -- , s)."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        used, res, s = PgclipModelStruct(), PgclipEstimateStruct(), C.c_double()
        given = None
        if model is not None:
            a, b = (model.a, model.b) if hasattr(model, "a") else model
            given = PgclipModelStruct(float(a), float(b), float(lo), float(hi))
        head = (self._h, C.byref(given) if given is not None else None, float(lo), float(hi), C.byref(used), C.byref(s), C.byref(res), C.byref(P1),
                C.byref(P2))
        tail = (ang_major, awidth, aheight, an1, an2, int(W), int(H), int(Cc))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            n, b_, d = (self._host_sais(x) for x in (noisy, basic, denoised))
            self._ck(self._L.lfbm5d_denoise_pgclip_host_sai(*head, _sai_ptrs(n, m), mp, _sai_ptrs(b_, m), _sai_ptrs(d, m), *tail))
        else:
            self._ck(self._L.lfbm5d_denoise_pgclip_device(*head, _dev_ptr(noisy), mp, _dev_ptr(basic), _dev_ptr(denoised), *tail))
        if given is None:
            est = _pgclip_result(res, int(Cc))
        else:
            est = PgclipEstimate(used.a, used.b, used.lo, used.hi, (), (), 0, 0.0, 0.0, False, False, 0, 0)
        return est, s.value

    # ---- impulse repair ----
    def impulse_histogram(self, LF, LF_SAI_mask, width, height, chnls):
        """The ROAD histogram of lfbm5d_impulse_histogram_device on a CUDA float32 tensor [asize][C*H*W]: (hist uint64 [C][386], pixels,
        skipped)."""
        m = _u32(LF_SAI_mask)
        C_ = int(chnls)
        hist = np.zeros((max(C_, 1), IMPULSE_KEYS), np.uint64)
        pixels, skipped = C.c_ulonglong(), C.c_ulonglong()
        self._ck(self._L.lfbm5d_impulse_histogram_device(self._h, _dev_ptr(LF), m.ctypes.data_as(C.POINTER(C.c_uint)), m.size, int(width),
                                                         int(height), C_, hist.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                                         C.byref(pixels), C.byref(skipped)))
        return hist, pixels.value, skipped.value

    def impulse_repair(self, noisy, mask, width, height, chnls, k=8.0, threshold=None, flags=None, return_flags=False, min_threshold=0.0,
                       out=None, flags_out=None):
        """Impulse repair (lfbm5d_impulse_repair_*, include/lfbm5d.h): pixels that are not finite, or whose rank-ordered absolute
        difference exceeds max(k x the channel's median, min_threshold) -- or `threshold`, a scalar or per-channel sequence, outright --
        while no neighbour lies on one side of them, are replaced by the lower median of their sound neighbours.  flags (uint8, like
        noisy, non-zero = defective): repair exactly those instead; no detection.  noisy: a CUDA float32 tensor [asize][C*H*W] (device
        form; out / flags_out: optional tensors to write into, distinct from the inputs) or a float32 numpy array of that shape / a list
        of per-SAI arrays (host form, staged through HBM; identical results).  noisy is only read; planes of empty SAIs of the result
        are copies of the input's (of `out` when given: untouched).  Returns an ImpulseRepair."""
        m = _u32(mask)
        asize, C_ = m.size, int(chnls)
        P = impulse_params(k, min_threshold, threshold)
        res = ImpulseResultStruct()
        cs = np.zeros((max(asize, 1), max(C_, 1), 3), np.uint64)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        tail = (asize, int(width), int(height), C_, C.byref(res), cs.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            arrays = self._host_sais(noisy)
            out, outs = self._host_out(arrays, out)
            fin = None
            if flags is not None:
                fin = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in flags]
            fo = self._host_planes(arrays, flags_out, return_flags, np.uint8)
            self._ck(self._L.lfbm5d_impulse_repair_host_sai(self._h, C.byref(P), _sai_ptrs(arrays, m), None if fin is None else _sai_ptrs(fin, m, np.uint8),
                                                            mp, _sai_ptrs(outs, m), None if fo is None else _sai_ptrs(fo, m, np.uint8), *tail))
            out, fo = self._stacked(noisy, out), self._stacked(noisy, fo)
        else:
            import torch
            out = self._dev_out(noisy, out, m)
            fo = self._dev_planes(noisy, flags_out, return_flags, noisy.shape, torch.uint8)
            fop = None if fo is None else _dev_ptr(fo, np.uint8)
            if flags is None:
                self._ck(self._L.lfbm5d_impulse_repair_device(self._h, C.byref(P), _dev_ptr(noisy), mp, _dev_ptr(out), fop, *tail))
            else:
                self._ck(self._L.lfbm5d_impulse_repair_flags_device(self._h, _dev_ptr(noisy), _dev_ptr(flags, np.uint8), mp, _dev_ptr(out), fop, *tail))
        return ImpulseRepair(out, fo, res.scale, tuple(res.scale_channel[:C_]), tuple(res.threshold[:C_]), tuple(res.flagged[:C_]),
                             tuple(res.repaired[:C_]), tuple(res.left[:C_]), int(res.pixels), int(res.skipped),
                             cs[:asize, :C_].astype(np.int64))

    # ---- defect inpainting ----
    @staticmethod
    def _inpaint_result(out, fo, res, C_):
        return Inpaint(out, fo, tuple(res.flagged[:C_]), tuple(res.filled[:C_]), tuple(res.left[:C_]), int(res.pixels), int(res.passes),
                       int(res.launches))

    def inpaint_fill(self, noisy, flags, mask, width, height, chnls, return_flags=False, out=None, flags_out=None):
        """The onion-peel fill of lfbm5d_inpaint_fill_device on CUDA tensors: noisy float32 [asize][C*H*W], flags uint8 of that shape
        (non-zero = defective; a value that is not finite is flagged too).  Both are only read; out / flags_out: optional tensors to
        write into, distinct from the inputs; planes of empty SAIs of a fresh result are copies of the input's.  Returns an Inpaint."""
        import torch
        m = _u32(mask)
        C_ = int(chnls)
        res = InpaintResultStruct()
        out = self._dev_out(noisy, out, m)
        fo = self._dev_planes(noisy, flags_out, return_flags, noisy.shape, torch.uint8)
        self._ck(self._L.lfbm5d_inpaint_fill_device(self._h, _dev_ptr(noisy), _dev_ptr(flags, np.uint8), m.ctypes.data_as(C.POINTER(C.c_uint)),
                                                    _dev_ptr(out), None if fo is None else _dev_ptr(fo, np.uint8), m.size, int(width), int(height),
                                                    C_, C.byref(res)))
        return self._inpaint_result(out, fo, res, C_)

    def inpaint_project(self, flags, x, y, mask, out, width, height, chnls):
        """out = flags ? x : y on the non-empty SAIs (lfbm5d_inpaint_project_device); CUDA tensors, out may be x or y."""
        m = _u32(mask)
        self._ck(self._L.lfbm5d_inpaint_project_device(self._h, _dev_ptr(flags, np.uint8), _dev_ptr(x), _dev_ptr(y),
                                                       m.ctypes.data_as(C.POINTER(C.c_uint)), _dev_ptr(out), m.size, int(width), int(height),
                                                       int(chnls)))

    def inpaint(self, noisy, flags, mask, P, ang_major, awidth, aheight, an, width, height, chnls, iterations=None, sigma_start=None,
                sigma_end=None, sigma_noise=None, return_flags=False, out=None, flags_out=None):
        """Defect inpainting (lfbm5d_inpaint_*, include/lfbm5d.h): the values `flags` names (uint8 like noisy, non-zero = defective) and
        every value that is not finite are filled from their rim inwards, then refined by `iterations` hard-thresholding steps (P, its
        sigma replaced by the schedule sigma_start -> sigma_end, not below sigma_noise) with the sound data put back after every step;
        iterations = 0 is the fill alone, None the library's defaults.  noisy: a CUDA float32 tensor [asize][C*H*W] with a uint8 CUDA
        tensor of flags (device form), or float32 / uint8 numpy arrays of that shape or lists of per-SAI arrays (host form, staged
        through HBM; identical results).  The inputs are only read.  Returns an Inpaint."""
        m = _u32(mask)
        asize, C_ = m.size, int(chnls)
        ip = inpaint_params(iterations, sigma_start, sigma_end, sigma_noise)
        res = InpaintResultStruct()
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        tail = (ang_major, awidth, aheight, an, int(width), int(height), C_, C.byref(res))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            arrays = self._host_sais(noisy)
            out, outs = self._host_out(arrays, out)
            fin = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in flags]
            fo = self._host_planes(arrays, flags_out, return_flags, np.uint8)
            self._ck(self._L.lfbm5d_inpaint_host_sai(self._h, C.byref(ip), C.byref(P), _sai_ptrs(arrays, m), _sai_ptrs(fin, m, np.uint8), mp,
                                                     _sai_ptrs(outs, m), None if fo is None else _sai_ptrs(fo, m, np.uint8), *tail))
            out, fo = self._stacked(noisy, out), self._stacked(noisy, fo)
        else:
            import torch
            out = self._dev_out(noisy, out, m)
            fo = self._dev_planes(noisy, flags_out, return_flags, noisy.shape, torch.uint8)
            self._ck(self._L.lfbm5d_inpaint_device(self._h, C.byref(ip), C.byref(P), _dev_ptr(noisy), _dev_ptr(flags, np.uint8), mp, _dev_ptr(out),
                                                   None if fo is None else _dev_ptr(fo, np.uint8), *tail))
        return self._inpaint_result(out, fo, res, C_)

    # ---- view synthesis ----
    @staticmethod
    def _view_result(out, disp, res, steps_hist=None, occl=None, sets=None):
        return ViewSynth(out, disp, int(res.missing), int(res.synthesised), int(res.left), int(res.pixels), tuple(res.disparity_hist),
                         None if steps_hist is None else tuple(int(v) for v in steps_hist),
                         None if occl is None else tuple(int(v) for v in occl.set_hist), sets)

    @staticmethod
    def _occlusion(occlusion, return_sets=False, sets_out=None):
        """The occl_ratio of `occlusion`: None or False -> 0 (off), True -> the library's default, a number -> itself (the library
        checks its range).  Set planes without occlusion are an error."""
        if occlusion is None or occlusion is False:
            ratio = 0.0
        elif occlusion is True:
            ratio = float(lib().lfbm5d_view_occl_default())
        elif isinstance(occlusion, (int, float, np.integer, np.floating)):
            ratio = float(occlusion)
        else:
            raise LfBm5dError(f"occlusion must be None, True or a ratio, not {type(occlusion).__name__}")
        if ratio == 0.0 and (return_sets or sets_out is not None):
            raise LfBm5dError("return_sets and sets_out need occlusion (the plain sweep chooses no set)")
        return ratio

    @staticmethod
    def _steps(disparity_steps):
        """(steps, the 65-bin histogram to fill or None, its pointer): the integer forms serve disparity_steps = 1."""
        steps = int(disparity_steps)
        if steps == 1:
            return 1, None, None
        hist = np.zeros(VIEW_STEPS_HIST, np.uint64)
        return steps, hist, hist.ctypes.data_as(C.POINTER(C.c_ulonglong))

    def view_fill(self, noisy, mask, missing, ang_major, awidth, aheight, width, height, chnls, max_disparity=None, box_radius=None,
                  ang_radius=None, return_disparity=False, out=None, disparity_out=None, disparity_steps=1, occlusion=None,
                  return_sets=False, sets_out=None):
        """The plane-sweep synthesis of lfbm5d_view_fill_device on CUDA tensors: noisy float32 [asize][C*H*W] (only read; the planes of
        the SAIs `missing` marks are never read).  out / disparity_out (int8 [asize][H*W]): optional tensors to write into, distinct
        from the input; only the planes of the synthesised SAIs are written, a fresh `out` is a copy of the input elsewhere.
        disparity_steps = 1, 2 or 4 hypotheses per pixel (lfbm5d_view_fill_steps_device; sources are interpolated bilinearly): the
        result's `disparity` is in units of 1 / disparity_steps, and above 1 its steps_hist is the histogram.  occlusion: None (off),
        True (the library's ratio) or a ratio >= 1: the occlusion-aware sweep of lfbm5d_view_fill_occl_device (include/lfbm5d_occl.h);
        the result gains set_hist and, with return_sets or sets_out (uint8 [asize][H*W]), sets.  Returns a ViewSynth."""
        ratio = self._occlusion(occlusion, return_sets, sets_out)
        steps, sh, shp = self._steps(disparity_steps)
        m, ms = _u32(mask), _u32(missing)
        vp = view_params(max_disparity, box_radius, ang_radius)
        res = ViewResultStruct()
        import torch
        out = self._dev_out(noisy, out)
        dp = self._dev_planes(noisy, disparity_out, return_disparity, (m.size, int(width) * int(height)), torch.int8)
        up = C.POINTER(C.c_uint)
        args = (_dev_ptr(noisy), m.ctypes.data_as(up), ms.ctypes.data_as(up), _dev_ptr(out), None if dp is None else _dev_ptr(dp, np.int8),
                ang_major, awidth, aheight, int(width), int(height), int(chnls), C.byref(res))
        if ratio != 0.0:
            sh = np.zeros(VIEW_STEPS_HIST, np.uint64)
            sp = self._dev_planes(noisy, sets_out, return_sets, (m.size, int(width) * int(height)), torch.uint8)
            occl = ViewOcclResultStruct()
            self._ck(self._L.lfbm5d_view_fill_occl_device(self._h, C.byref(vp), steps, ratio, *args[:5], None if sp is None else _dev_ptr(sp, np.uint8),
                                                          *args[5:], sh.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(occl)))
            return self._view_result(out, dp, res, sh, occl, sp)
        if steps == 1:
            self._ck(self._L.lfbm5d_view_fill_device(self._h, C.byref(vp), *args))
        else:
            self._ck(self._L.lfbm5d_view_fill_steps_device(self._h, C.byref(vp), steps, *args, shp))
        return self._view_result(out, dp, res, sh)

    def view_synth(self, noisy, mask, missing, P, ang_major, awidth, aheight, an, width, height, chnls, max_disparity=None,
                   box_radius=None, ang_radius=None, iterations=None, sigma_start=None, sigma_end=None, sigma_noise=None,
                   return_disparity=False, out=None, disparity_out=None, disparity_steps=1, occlusion=None, return_sets=False,
                   sets_out=None):
        """View synthesis (lfbm5d_view_*, include/lfbm5d.h): the SAIs `missing` marks (non-zero; they must be non-empty in `mask`) are
        synthesised from their sound angular neighbours by a plane sweep over the integer disparities -max_disparity..max_disparity
        and refined by `iterations` hard-thresholding steps (P, its sigma replaced by the schedule sigma_start -> sigma_end, not below
        sigma_noise) with the sound SAIs put back after every step; iterations = 0 is the synthesis alone, None the library's
        defaults.  noisy: a CUDA float32 tensor [asize][C*H*W] (device form), or a float32 numpy array of that shape or a list of
        per-SAI arrays, None allowed for missing SAIs (host form, staged through HBM; identical results).  The input is only read.
        return_disparity: the int8 planes [asize][H*W] of d*.  disparity_steps = 1, 2 or 4 hypotheses per pixel (the *_steps_* forms;
        sources are interpolated bilinearly): `disparity` is in units of 1 / disparity_steps, and above 1 the result's steps_hist is
        the histogram.  occlusion: None (off), True (the library's ratio) or a ratio >= 1: the occlusion-aware sweep of the
        lfbm5d_view_occl_* forms (include/lfbm5d_occl.h); the result gains set_hist and, with return_sets or sets_out (uint8
        [asize][H*W]; a list of per-SAI planes in the host form), sets.  Returns a ViewSynth."""
        ratio = self._occlusion(occlusion, return_sets, sets_out)
        m, ms = _u32(mask), _u32(missing)
        steps, sh, shp = self._steps(disparity_steps)
        occl = sp = None
        if ratio != 0.0:
            sh, occl = np.zeros(VIEW_STEPS_HIST, np.uint64), ViewOcclResultStruct()
            tail_occl = (sh.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(occl))
        asize = m.size
        vp = view_params(max_disparity, box_radius, ang_radius, iterations, sigma_start, sigma_end, sigma_noise)
        res = ViewResultStruct()
        up = C.POINTER(C.c_uint)
        mp, msp = m.ctypes.data_as(up), ms.ctypes.data_as(up)
        tail = (ang_major, awidth, aheight, an, int(width), int(height), int(chnls), C.byref(res))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            arrays = self._host_sais(noisy)
            out, outs = self._host_out(arrays, out, m, int(chnls) * int(width) * int(height))
            dp = self._host_planes(arrays, disparity_out, return_disparity, np.int8, int(width) * int(height))
            args = (C.byref(P), _sai_ptrs(arrays, m), mp, msp, _sai_ptrs(outs, m), None if dp is None else _sai_ptrs(dp, m, np.int8), *tail)
            if ratio != 0.0:
                sp = self._host_planes(arrays, sets_out, return_sets, np.uint8, int(width) * int(height))
                self._ck(self._L.lfbm5d_view_occl_host_sai(self._h, C.byref(vp), steps, ratio, *args[:6],
                                                           None if sp is None else _sai_ptrs(sp, m, np.uint8), *tail, *tail_occl))
                sp = self._stacked(noisy, sp, False)
            elif steps == 1:
                self._ck(self._L.lfbm5d_view_host_sai(self._h, C.byref(vp), *args))
            else:
                self._ck(self._L.lfbm5d_view_steps_host_sai(self._h, C.byref(vp), steps, *args, shp))
            out, dp = self._stacked(noisy, out), self._stacked(noisy, dp, False)
        else:
            import torch
            out = self._dev_out(noisy, out)
            dp = self._dev_planes(noisy, disparity_out, return_disparity, (asize, int(width) * int(height)), torch.int8)
            args = (C.byref(P), _dev_ptr(noisy), mp, msp, _dev_ptr(out), None if dp is None else _dev_ptr(dp, np.int8), *tail)
            if ratio != 0.0:
                sp = self._dev_planes(noisy, sets_out, return_sets, (asize, int(width) * int(height)), torch.uint8)
                self._ck(self._L.lfbm5d_view_occl_device(self._h, C.byref(vp), steps, ratio, *args[:6], None if sp is None else _dev_ptr(sp, np.uint8),
                                                         *tail, *tail_occl))
            elif steps == 1:
                self._ck(self._L.lfbm5d_view_device(self._h, C.byref(vp), *args))
            else:
                self._ck(self._L.lfbm5d_view_steps_device(self._h, C.byref(vp), steps, *args, shp))
        return self._view_result(out, dp, res, sh, occl, sp)

    # ---- joint repair ----
    @staticmethod
    def _repair_result(out, codes, disp, res, C_):
        return Repair(out, codes, disp, int(res.missing), int(res.targets), int(res.swept), int(res.passes), int(res.values), int(res.flagged),
                      tuple(res.unsound[:C_]), tuple(res.views[:C_]), tuple(res.rim[:C_]), tuple(res.left[:C_]), int(res.positions),
                      tuple(res.disparity_hist))

    def repair_fill(self, noisy, flags, missing, mask, ang_major, awidth, aheight, width, height, chnls, max_disparity=None, box_radius=None,
                    ang_radius=None, min_valid=None, return_codes=False, return_disparity=False, out=None, codes_out=None,
                    disparity_out=None):
        """The joint fill of lfbm5d_repair_fill_device on CUDA tensors (include/lfbm5d_repair.h): noisy float32 [asize][C*H*W], flags
        uint8 of that shape (non-zero = defective) or None, missing [asize] (non-zero = the whole SAI) or None.  The inputs are only
        read; out / codes_out / disparity_out (int8 [asize][H*W]): optional tensors to write into, distinct from the inputs; planes of
        empty SAIs of a fresh result are copies of the input's.  Returns a Repair."""
        import torch
        m = _u32(mask)
        ms = None if missing is None else _u32(missing)
        C_ = int(chnls)
        rp = repair_params(max_disparity, box_radius, ang_radius, min_valid)
        res = RepairResultStruct()
        out = self._dev_out(noisy, out, m)
        co = self._dev_planes(noisy, codes_out, return_codes, noisy.shape, torch.uint8)
        dp = self._dev_planes(noisy, disparity_out, return_disparity, (m.size, int(width) * int(height)), torch.int8)
        up = C.POINTER(C.c_uint)
        rc = self._L.lfbm5d_repair_fill_device(self._h, C.byref(rp), _dev_ptr(noisy), None if flags is None else _dev_ptr(flags, np.uint8),
                                               m.ctypes.data_as(up), None if ms is None else ms.ctypes.data_as(up), _dev_ptr(out),
                                               None if co is None else _dev_ptr(co, np.uint8), None if dp is None else _dev_ptr(dp, np.int8),
                                               ang_major, awidth, aheight, int(width), int(height), C_, C.byref(res))
        self._ck(rc)
        return self._repair_result(out, co, dp, res, C_)

    def repair(self, noisy, flags, missing, mask, P, ang_major, awidth, aheight, an, width, height, chnls, max_disparity=None,
               box_radius=None, ang_radius=None, min_valid=None, iterations=None, sigma_start=None, sigma_end=None, sigma_noise=None,
               return_codes=False, return_disparity=False, out=None, codes_out=None, disparity_out=None):
        """Joint repair (lfbm5d_repair_*, include/lfbm5d_repair.h): the values `flags` names (uint8 like noisy, non-zero = defective; or
        None), every value that is not finite and every value of the SAIs `missing` marks (or None) are filled from the other views by a
        plane sweep that skips unsound source values, what it cannot reach from the rim of its own plane, and the fill is refined by
        `iterations` hard-thresholding steps (P, its sigma replaced by the schedule sigma_start -> sigma_end, not below sigma_noise) with
        the sound values put back after every step; iterations = 0 is the fill alone, None the library's defaults.  noisy: a CUDA float32
        tensor [asize][C*H*W] with a uint8 CUDA tensor of flags (device form), or float32 / uint8 numpy arrays of that shape or lists of
        per-SAI arrays (host form, staged through HBM; identical results).  The inputs are only read.  Returns a Repair."""
        m = _u32(mask)
        ms = None if missing is None else _u32(missing)
        asize, C_ = m.size, int(chnls)
        rp = repair_params(max_disparity, box_radius, ang_radius, min_valid, iterations, sigma_start, sigma_end, sigma_noise)
        res = RepairResultStruct()
        up = C.POINTER(C.c_uint)
        mp, msp = m.ctypes.data_as(up), None if ms is None else ms.ctypes.data_as(up)
        tail = (ang_major, awidth, aheight, an, int(width), int(height), C_, C.byref(res))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            arrays = self._host_sais(noisy)
            out, outs = self._host_out(arrays, out)
            fin = None if flags is None else [None if a is None else np.ascontiguousarray(a, np.uint8) for a in flags]
            co = self._host_planes(arrays, codes_out, return_codes, np.uint8)
            dp = self._host_planes(arrays, disparity_out, return_disparity, np.int8, int(width) * int(height))
            rc = self._L.lfbm5d_repair_host_sai(self._h, C.byref(rp), C.byref(P), _sai_ptrs(arrays, m),
                                                None if fin is None else _sai_ptrs(fin, m, np.uint8), mp, msp, _sai_ptrs(outs, m),
                                                None if co is None else _sai_ptrs(co, m, np.uint8),
                                                None if dp is None else _sai_ptrs(dp, m, np.int8), *tail)
            self._ck(rc)
            out, co, dp = self._stacked(noisy, out), self._stacked(noisy, co), self._stacked(noisy, dp, False)
        else:
            import torch
            out = self._dev_out(noisy, out, m)
            co = self._dev_planes(noisy, codes_out, return_codes, noisy.shape, torch.uint8)
            dp = self._dev_planes(noisy, disparity_out, return_disparity, (asize, int(width) * int(height)), torch.int8)
            rc = self._L.lfbm5d_repair_device(self._h, C.byref(rp), C.byref(P), _dev_ptr(noisy), None if flags is None else _dev_ptr(flags, np.uint8),
                                              mp, msp, _dev_ptr(out), None if co is None else _dev_ptr(co, np.uint8),
                                              None if dp is None else _dev_ptr(dp, np.int8), *tail)
            self._ck(rc)
        return self._repair_result(out, co, dp, res, C_)

    # ---- consistency check ----
    def consist(self, noisy, mask, ang_major, awidth, aheight, width, height, chnls, exclude=None, return_disparity=False,
                flags_out=None, disparity_out=None, fill_nonfinite=True, disparity_steps=1, **params):
        """Consistency check (lfbm5d_consist_*, include/lfbm5d.h): every usable SAI is predicted from its angular neighbours by the view
        synthesis' plane sweep with the SAI itself left out; a value is flagged when its residual exceeds k x the light field's median
        residual and spread x the sources' own disagreement, an SAI is bad when its median residual stands out among its neighbours'.
        noisy: a CUDA float32 tensor [asize][C*H*W] (device form), or a float32 numpy array of that shape or a list of per-SAI arrays
        (host form, staged through HBM; identical results).  The input is only read.  exclude: SAIs known bad (non-zero), neither
        tested nor used.  params: the fields of consist_params.  fill_nonfinite: when the input holds a value that is not finite, the
        check runs on a copy with those values filled (inpaint_fill under an empty map) and they are reported with code 2 on top of
        the library's flags (the counts are the library's).  disparity_steps = 1, 2 or 4 hypotheses per pixel in the sweep (the
        *_steps_* forms): `disparity` is in units of 1 / disparity_steps.  Returns a Consist, whose flags go to inpaint(...) as the map
        and whose .missing goes to view_synth(...)."""
        m = _u32(mask)
        steps = int(disparity_steps)
        asize, C_, W_, H_ = m.size, int(chnls), int(width), int(height)
        P = consist_params(**params)
        res = ConsistResultStruct()
        up = C.POINTER(C.c_uint)
        ex = None if exclude is None else _u32(exclude)
        state = np.zeros(asize, np.uint32)
        ssai = np.zeros(asize, np.float64)
        hist = np.zeros((asize, max(C_, 1), IMPULSE_KEYS), np.uint64)
        head = (self._h, C.byref(P)) if steps == 1 else (self._h, C.byref(P), steps)
        host_sai = self._L.lfbm5d_consist_host_sai if steps == 1 else self._L.lfbm5d_consist_steps_host_sai
        device = self._L.lfbm5d_consist_device if steps == 1 else self._L.lfbm5d_consist_steps_device
        mid = (m.ctypes.data_as(up), None if ex is None else ex.ctypes.data_as(up))
        tail = (ssai.ctypes.data_as(C.POINTER(C.c_double)), hist.ctypes.data_as(C.POINTER(C.c_ulonglong)), ang_major, awidth, aheight,
                W_, H_, C_, C.byref(res))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            arrays = self._host_sais(noisy)
            live = [i for i in range(asize) if m[i] and arrays[i] is not None]
            holes = {i: ~np.isfinite(arrays[i]) for i in live} if fill_nonfinite else {}
            holes = {i: h for i, h in holes.items() if h.any()}
            if holes:
                import torch
                full = np.zeros((asize, C_ * W_ * H_), np.float32)
                for i in live:
                    full[i] = np.asarray(arrays[i]).reshape(-1)
                d = torch.from_numpy(full).cuda()
                filled = self.inpaint_fill(d, torch.zeros(d.shape, dtype=torch.uint8, device=d.device), m, W_, H_, C_).out.cpu().numpy()
                arrays = [np.ascontiguousarray(filled[i].reshape(np.shape(arrays[i]))) if i in holes else arrays[i] for i in range(asize)]
            fo = self._host_planes(arrays, flags_out, True, np.uint8)
            dp = self._host_planes(arrays, disparity_out, return_disparity, np.int8, W_ * H_)
            self._ck(host_sai(*head, _sai_ptrs(arrays, m), *mid, _sai_ptrs(fo, m, np.uint8), state.ctypes.data_as(up),
                              None if dp is None else _sai_ptrs(dp, m, np.int8), *tail))
            for i, h in holes.items():
                fo[i][h] = 2
            fo, dp = self._stacked(noisy, fo), self._stacked(noisy, dp, False)
        else:
            import torch
            src, hole = noisy, None
            live = torch.from_numpy(m != 0).to(noisy.device)
            if fill_nonfinite and not bool(torch.isfinite(noisy[live]).all().item()):
                hole = ~torch.isfinite(noisy)
                hole[~live] = False
                src = self.inpaint_fill(noisy, torch.zeros(noisy.shape, dtype=torch.uint8, device=noisy.device), m, W_, H_, C_).out
            fo = self._dev_planes(noisy, flags_out, True, noisy.shape, torch.uint8)
            dp = self._dev_planes(noisy, disparity_out, return_disparity, (asize, W_ * H_), torch.int8)
            self._ck(device(*head, _dev_ptr(src), *mid, _dev_ptr(fo, np.uint8), state.ctypes.data_as(up),
                            None if dp is None else _dev_ptr(dp, np.int8), *tail))
            if hole is not None:
                fo[hole] = 2
        st = state.astype(np.int64)
        return Consist(fo, st, dp, tuple(res.scale_channel[:C_]), tuple(res.threshold[:C_]), ssai, hist[:, :C_],
                       tuple(int(res.flagged[c][0]) for c in range(C_)), tuple(int(res.flagged[c][1]) for c in range(C_)),
                       tuple(int(i) for i in np.nonzero(st == CONSIST_BAD)[0]), tuple(int(i) for i in np.nonzero(st == CONSIST_UNTESTED)[0]),
                       int(res.rounds), int(res.pixels), int(res.skipped))

    # ---- photometric equalisation ----
    def equalise(self, noisy, mask, ang_major, awidth, aheight, width, height, chnls, return_hist=False, out=None, **params):
        """Photometric equalisation (lfbm5d_photo_*, include/lfbm5d_photo.h): every SAI with enough neighbours is predicted from them
        by the view synthesis' plane sweep with the SAI itself left out, the median ratio of its values to the prediction gives one
        gain per SAI and stored channel, and the gains are divided out; sweep, fit and correction repeat until the ratios are within
        tol of 1.  noisy: a CUDA float32 tensor [asize][C*H*W] (device form), or a float32 numpy array of that shape or a list of
        per-SAI arrays (host form, staged through HBM; identical results).  The input is only read.  params: the fields of
        photo_params.  Returns an Equalise."""
        m = _u32(mask)
        asize, C_, W_, H_ = m.size, int(chnls), int(width), int(height)
        P = photo_params(**params)
        res = PhotoResultStruct()
        up = C.POINTER(C.c_uint)
        gain, state = np.ones((asize, 3), np.float64), np.zeros(asize, np.uint32)
        hist = np.zeros((asize, max(C_, 1), PHOTO_KEYS), np.uint64) if return_hist else None
        tail = (gain.ctypes.data_as(C.POINTER(C.c_double)), state.ctypes.data_as(up),
                None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_ulonglong)), ang_major, awidth, aheight, W_, H_, C_, C.byref(res))
        if isinstance(noisy, (list, tuple, np.ndarray)):
            arrays = self._host_sais(noisy)
            o, olist = self._host_out(arrays, out)
            self._ck(self._L.lfbm5d_photo_host_sai(self._h, C.byref(P), _sai_ptrs(arrays, m), m.ctypes.data_as(up), _sai_ptrs(olist, m), *tail))
            o = self._stacked(noisy, o)
        else:
            o = self._dev_out(noisy, out, m)
            self._ck(self._L.lfbm5d_photo_device(self._h, C.byref(P), _dev_ptr(noisy), m.ctypes.data_as(up), _dev_ptr(o), *tail))
        return Equalise(o, gain, state.astype(np.int64), hist, int(res.rounds), bool(res.converged), float(res.residual),
                        float(res.gain_min), float(res.gain_max), int(res.fitted), int(res.untested), int(res.unfit), int(res.admitted),
                        int(res.skipped_nonfinite), int(res.skipped_range))

    def apply_gains(self, lf, gain, invert=False, *, chnls, mask=None, out=None):
        """lfbm5d_photo_apply_*: out = lf (float)(invert ? G : 1 / G) per SAI and stored channel, G = gain float64 [asize][3] (an
        Equalise's .gain).  lf as for equalise, [asize][chnls*H*W].  out: where to write (device form: may be lf itself, the default is
        a fresh tensor; host form: a list of per-SAI arrays, the default is fresh arrays).  invert=True after denoising gives every
        view its own photometry back."""
        g = np.ascontiguousarray(np.asarray(gain, np.float64).reshape(-1, 3))
        asize, C_ = g.shape[0], int(chnls)
        m = np.ones(asize, np.uint32) if mask is None else _u32(mask)
        host = isinstance(lf, (list, tuple, np.ndarray))
        arrays = self._host_sais(lf) if host else None
        img = next((int(np.size(a)) for a in arrays if a is not None), 0) if host else int(lf.shape[1])
        if len(arrays if host else lf) != asize or C_ < 1 or img % C_:
            raise LfBm5dError("apply_gains: lf must be [asize][chnls*H*W] and gain [asize][3]")
        up, dp = C.POINTER(C.c_uint), C.POINTER(C.c_double)
        tail = (asize, 1, img // C_, 1, C_)          # only the products awidth x aheight and W x H matter
        if host:
            o, olist = self._host_out(arrays, out)
            self._ck(self._L.lfbm5d_photo_apply_host_sai(self._h, _sai_ptrs(arrays, m), m.ctypes.data_as(up), g.ctypes.data_as(dp),
                                                         int(bool(invert)), _sai_ptrs(olist, m), *tail))
            return self._stacked(lf, o)
        o = self._dev_out(lf, out)
        self._ck(self._L.lfbm5d_photo_apply_device(self._h, _dev_ptr(lf), m.ctypes.data_as(up), g.ctypes.data_as(dp), int(bool(invert)),
                                                   _dev_ptr(o), *tail))
        return o

    # ---- super-resolution ----
    def _sr_tail(self, mask, w, h, Cc):
        m = _u32(mask)
        return m, m.ctypes.data_as(C.POINTER(C.c_uint)), (m.size, int(w), int(h), int(Cc))

    def sr_up(self, sr, low, mask, high, w, h, Cc):
        """high = U low (lfbm5d_sr_up_device): CUDA float32 tensors [asize][C*h*w] -> [asize][C*sh*sw]; w, h = the low-resolution size."""
        m, mp, tail = self._sr_tail(mask, w, h, Cc)
        self._ck(self._L.lfbm5d_sr_up_device(self._h, C.byref(sr), _dev_ptr(low), mp, _dev_ptr(high), *tail))

    def sr_down(self, sr, high, mask, low, w, h, Cc):
        """low = D high (lfbm5d_sr_down_device)."""
        m, mp, tail = self._sr_tail(mask, w, h, Cc)
        self._ck(self._L.lfbm5d_sr_down_device(self._h, C.byref(sr), _dev_ptr(high), mp, _dev_ptr(low), *tail))

    def sr_backproject(self, sr, low_y, high_x, mask, high_z, w, h, Cc):
        """high_z = high_x + beta U (low_y - D high_x) in two launches (lfbm5d_sr_backproject_device); high_z may be high_x."""
        m, mp, tail = self._sr_tail(mask, w, h, Cc)
        self._ck(self._L.lfbm5d_sr_backproject_device(self._h, C.byref(sr), _dev_ptr(low_y), _dev_ptr(high_x), mp, _dev_ptr(high_z), *tail))

    def superres(self, sr, P, low, mask, high, ang_major, awidth, aheight, an, w, h, Cc):
        """Super-resolve `low` into `high` (lfbm5d_superres_*, include/lfbm5d.h): CUDA float32 tensors (device form), or float32 numpy
        arrays / lists of per-SAI arrays (host form, staged through HBM; bit-identical).  P: the hard-thresholding parameters (sigma
        ignored); w, h: the low-resolution size."""
        m = _u32(mask)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint))
        tail = (ang_major, awidth, aheight, an, int(w), int(h), int(Cc))
        if isinstance(low, (list, tuple, np.ndarray)):
            lo = list(low) if isinstance(low, (list, tuple)) else [a for a in low]
            hi = list(high) if isinstance(high, (list, tuple)) else [a for a in high]
            self._ck(self._L.lfbm5d_superres_host_sai(self._h, C.byref(sr), C.byref(P), _sai_ptrs(lo, m), mp, _sai_ptrs(hi, m), *tail))
        else:
            self._ck(self._L.lfbm5d_superres_device(self._h, C.byref(sr), C.byref(P), _dev_ptr(low), mp, _dev_ptr(high), *tail))

    def last_windows(self):
        """Processed SAI of every window the last step call ran, in order."""
        n = self._L.lfbm5d_last_windows(self._h, None, 0)
        out = np.zeros(max(n, 1), np.uint32)
        self._L.lfbm5d_last_windows(self._h, out.ctypes.data_as(C.POINTER(C.c_uint)), out.size)
        return out[:max(n, 0)].copy()

    def last_bm(self, N, A, plane):
        """Block-matching tables of the last pass, as numpy arrays."""
        n = C.c_uint()
        self._ck(self._L.lfbm5d_last_bm(self._h, C.byref(n), None, None, None, None, None))
        R = n.value
        refs = np.zeros(R, np.uint32)
        idx = np.zeros((R, max(N, 1)), np.uint32)
        cnt = np.zeros(R, np.uint32)
        best = np.zeros((A, plane), np.uint32)
        shape = np.zeros((A, plane), np.uint8)
        self._ck(self._L.lfbm5d_last_bm(self._h, C.byref(n), refs.ctypes.data, idx.ctypes.data, cnt.ctypes.data,
                                        best.ctypes.data, shape.ctypes.data))
        return refs, idx, cnt, best, shape


    def last_tables(self, n_floats=None):
        """Raw disparity distance tables of the last pass (flat float32 array)."""
        have = self._L.lfbm5d_last_tables(self._h, None, 0)
        n = have if n_floats is None else min(have, int(n_floats))
        out = np.zeros(n, np.float32)
        got = self._L.lfbm5d_last_tables(self._h, out.ctypes.data, n)
        return out[:got]

    def last_scores(self, n_floats=None):
        """Candidate scores of the self-similarity search of the last pass (flat float32 array)."""
        have = self._L.lfbm5d_last_scores(self._h, None, 0)
        n = have if n_floats is None else min(have, int(n_floats))
        out = np.zeros(n, np.float32)
        got = self._L.lfbm5d_last_scores(self._h, out.ctypes.data, n)
        return out[:got]

    def last_weights(self, n_groups, C_):
        """Aggregation weights of the groups of the last pass, [group][channel]."""
        out = np.zeros(n_groups * C_, np.float32)
        got = self._L.lfbm5d_last_weights(self._h, out.ctypes.data, out.size)
        assert got == out.size
        return out.reshape(n_groups, C_)

    def last_group_list(self):
        """The list of the last group launch (lfbm5d_last_group_list): uint32 entries group | channel mask << 29, mask 7 for a
        group of a shape that is not the whole window, one channel bit for a guard-band (group, channel) of the fast chain."""
        n = C.c_uint(0)
        if self._L.lfbm5d_last_group_list(self._h, C.byref(n), None, 0) != 0:
            raise LfBm5dError("lfbm5d_last_group_list failed")
        out = np.zeros(max(1, n.value), np.uint32)
        if self._L.lfbm5d_last_group_list(self._h, C.byref(n), out.ctypes.data, out.size) != 0:
            raise LfBm5dError("lfbm5d_last_group_list failed")
        return out[:min(n.value, out.size)]

    def last_scan_version(self):
        return int(self._L.lfbm5d_last_scan_version(self._h))

    def debug_aggregate(self, num, den, filt, wgt, aggpos, mask, proc, *, n_refs_total, ref_begin, n_groups, n_ref_rows, n_ref_cols,
                        Wb, Hb, C_, A, k, N, pst, p, nSim, nDisp, filt_sai_stride=0, filt_bytes=None, irregular=0, wchan0=0,
                        direct=0, lf_stride=0, sai=None):
        """lfbm5d_debug_aggregate: the aggregation launch alone.  num, den, filt, wgt: float32 CUDA tensors, aggpos: an int32 CUDA
        tensor holding the uint32 words; num and den are added to in place.  mask, proc, sai: sequences of A integers.  A None entry
        among the tensors goes to the library as a NULL pointer (which it refuses)."""
        import torch

        def ptr(t, dtype):
            if t is None:
                return None, 0
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
                raise LfBm5dError("debug_aggregate takes contiguous CUDA tensors: float32 values, int32 positions")
            torch.cuda.current_stream(t.device).synchronize()
            return t.data_ptr(), t.numel()

        a = AggDebugStruct()
        (a.num, n_num), (a.den, n_den) = ptr(num, torch.float32), ptr(den, torch.float32)
        a.filt, n_filt = ptr(filt, torch.float32)
        a.wgt, a.wgt_floats = ptr(wgt, torch.float32)
        a.aggpos, a.aggpos_words = ptr(aggpos, torch.int32)
        a.sums_floats = min(n_num, n_den)
        a.filt_bytes = 4 * n_filt if filt_bytes is None else min(int(filt_bytes), 4 * n_filt)
        keep = [None if x is None else _u32(x) for x in (mask, proc, sai)]
        a.mask, a.proc, a.sai = [None if x is None else x.ctypes.data for x in keep]
        if any(x is not None and x.size < A for x in keep):
            raise LfBm5dError("debug_aggregate: mask, proc and sai hold one entry per SAI slot")
        a.filt_sai_stride, a.lf_stride = int(filt_sai_stride), int(lf_stride)
        a.n_refs_total, a.ref_begin, a.n_groups, a.n_ref_rows, a.n_ref_cols = n_refs_total, ref_begin, n_groups, n_ref_rows, n_ref_cols
        a.Wb, a.Hb, a.C, a.A, a.k, a.N, a.pst, a.p, a.nSim, a.nDisp = Wb, Hb, C_, A, k, N, pst, p, nSim, nDisp
        a.irregular, a.wchan0, a.direct = int(irregular), int(wchan0), int(direct)
        self._ck(self._L.lfbm5d_debug_aggregate(self._h, C.byref(a)))

    def debug_group(self, step, P, aw, ah, Wb, Hb, C_, noisy, basic, refs, self_idx, self_cnt, best, shape, filt, wgt, aggpos, mask, pst,
                    *, fill_quirk=1, n_refs_total, ref_begin=0, n_groups=None, filt_sai_stride=0, filt_floats=None, bm3d=0, null=(), _acf=None):
        """lfbm5d_debug_group: the group launch alone.  noisy, basic, filt, wgt: float32 CUDA tensors; refs, self_idx, self_cnt, best,
        aggpos: int32 CUDA tensors holding the uint32 words; shape: a uint8 CUDA tensor; mask: a sequence of A integers; P: Params.
        filt, wgt and aggpos are written.  A None tensor goes to the library as a NULL pointer (which it refuses, `basic` in step 1
        apart).  null: names of further fields of the struct to hand over as NULL (the refusal tests).  Returns (kernel text, sum of
        the stack sizes, shape-adaptive groups)."""
        import torch

        def ptr(t, dtype):
            if t is None:
                return None, 0
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
                raise LfBm5dError("debug_group takes contiguous CUDA tensors: float32 values, int32 tables, uint8 shapes")
            torch.cuda.current_stream(t.device).synchronize()
            return t.data_ptr(), t.numel()

        a = GroupDebugStruct()
        a.noisy, n_noisy = ptr(noisy, torch.float32)
        a.basic, n_basic = ptr(basic, torch.float32)
        a.image_floats = n_noisy if basic is None else min(n_noisy, n_basic)
        a.refs, n_refs = ptr(refs, torch.int32)
        a.self_idx, n_idx = ptr(self_idx, torch.int32)
        a.self_cnt, n_cnt = ptr(self_cnt, torch.int32)
        a.best, n_best = ptr(best, torch.int32)
        a.shape, n_shape = ptr(shape, torch.uint8)
        a.table_words = min(n_best, n_shape)
        a.filt, n_filt = ptr(filt, torch.float32)
        a.filt_floats = n_filt if filt_floats is None else min(int(filt_floats), n_filt)
        a.wgt, a.wgt_floats = ptr(wgt, torch.float32)
        a.aggpos, a.aggpos_words = ptr(aggpos, torch.int32)
        N = max(1, int(P.N))
        if any(t is not None and n < need for t, n, need in ((refs, n_refs, n_refs_total), (self_cnt, n_cnt, n_refs_total),
                                                             (self_idx, n_idx, n_refs_total * N))):
            raise LfBm5dError("debug_group: refs, self_cnt and self_idx hold n_refs_total (x N) entries")
        counters = (C.c_ulonglong * 2)(0, 0)
        a.counters = C.addressof(counters)
        keep = None if mask is None else _u32(mask)
        if keep is not None and keep.size < aw * ah:
            raise LfBm5dError("debug_group: mask holds one entry per SAI slot")
        a.mask = None if keep is None else keep.ctypes.data
        a.params = None if P is None else C.addressof(P)
        text = C.create_string_buffer(512)
        a.kernels, a.kernels_cap = C.addressof(text), 512
        a.filt_sai_stride = int(filt_sai_stride)
        a.step, a.aw, a.ah, a.Wb, a.Hb, a.C, a.pst, a.fill_quirk = step, aw, ah, Wb, Hb, C_, pst, int(fill_quirk)
        a.n_refs_total, a.ref_begin = n_refs_total, ref_begin
        a.n_groups = n_refs_total - ref_begin if n_groups is None else n_groups
        a.bm3d = int(bm3d)
        for name in null:
            setattr(a, name, None)
        if _acf is not None:   # (debug_group_corr)
            self._ck(self._L.lfbm5d_debug_group_corr(self._h, C.byref(a), _acf.ctypes.data_as(C.POINTER(C.c_double))))
        else:
            self._ck(self._L.lfbm5d_debug_group(self._h, C.byref(a)))
        return text.value.decode(), int(counters[0]), int(counters[1])

    def debug_window(self, op, *, list=None, slot_mask=None, **f):
        """lfbm5d_debug_window: one launcher of the window-schedule kernels alone.  op: a name of WINDOW_OPS.  The buffers go by the
        names of lfbm5d_window_debug (include/lfbm5d.h has the table of what each op reads): float32 CUDA tensors, `counters` and
        `dmask` int32 CUDA tensors holding the uint32 words; a None buffer goes to the library as a NULL pointer.  list, slot_mask:
        sequences of integers.  Everything else (W, H, C, N, k, off, cs, forward, colour, n_sai, n, strides, rectangle) by keyword;
        the sizes the library checks the geometry against are taken from the tensors (the smallest of each side), unless given."""
        import torch

        a = WindowDebugStruct()
        a.op = WINDOW_OPS.index(op)
        sizes = {"lf_floats": [], "w_floats": []}
        for name in _WINDOW_LF + _WINDOW_W + ("est", "counters", "dmask"):
            t = f.pop(name, None)
            if t is None:
                continue
            dtype = torch.int32 if name in ("counters", "dmask") else torch.float32
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
                raise LfBm5dError("debug_window takes contiguous CUDA tensors: float32 values, int32 counters and masks")
            torch.cuda.current_stream(t.device).synchronize()
            setattr(a, name, t.data_ptr())
            if name in _WINDOW_LF:
                sizes["lf_floats"].append(t.numel())
            elif name in _WINDOW_W:
                sizes["w_floats"].append(t.numel())
            else:
                setattr(a, {"est": "est_floats", "counters": "counter_words", "dmask": "dmask_words"}[name], t.numel())
        for key, v in sizes.items():
            setattr(a, key, min(v) if v else 0)
        keep = [None if x is None else _u32(x) for x in (list, slot_mask)]
        a.list, a.slot_mask = [None if x is None else x.ctypes.data for x in keep]
        n_list = f.pop("n_list", None)
        a.n_list = max((x.size for x in keep if x is not None), default=0) if n_list is None else int(n_list)
        if any(x is not None and x.size < a.n_list for x in keep):
            raise LfBm5dError("debug_window: list and slot_mask hold n_list entries")
        for key, v in f.items():
            if key not in dict(WindowDebugStruct._fields_) or key in ("list", "slot_mask", "op"):
                raise LfBm5dError("debug_window: unknown field " + key)
            setattr(a, key, int(v))
        self._ck(self._L.lfbm5d_debug_window(self._h, C.byref(a)))


_default_ctx = None


def _ctx():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def run_bm5d_1st_step(sigma, lambdaHard5D, LF_noisy, LF_SAI_mask, LF_basic, ang_major, awidth, aheight,
                      anHard, width, height, chnls, NHard, nSim, nDisp, kHard, pHard, useSD, tau_2D, tau_4D,
                      tau_5D, color_space, nb_threads=1, ctx=None):
    """Same argument list as the reference's run_bm5d_1st_step (src/bm5d.h:11-35).  LF_noisy is
    mutated in place and LF_basic filled, like the reference; nb_threads is accepted and ignored
    (the GPU path always has the untiled, nb_threads == 1 semantics).  Returns 0 (EXIT_SUCCESS)
    or raises LfBm5dError with the library's message."""
    P = make_params(sigma, lambdaHard5D, NHard, nSim, nDisp, kHard, pHard, tau_2D, tau_4D, tau_5D, useSD, color_space)
    (ctx or _ctx()).step1(P, LF_noisy, LF_SAI_mask, LF_basic, ang_major, awidth, aheight, anHard, width, height, chnls)
    return 0


def run_bm5d_2nd_step(sigma, LF_noisy, LF_SAI_mask, LF_basic, LF_denoised, ang_major, awidth, aheight,
                      anWien, width, height, chnls, NWien, nSim, nDisp, kWien, pWien, useSD, tau_2D, tau_4D,
                      tau_5D, color_space, nb_threads=1, ctx=None):
    """Same argument list as the reference's run_bm5d_2nd_step (src/bm5d.h:38-62)."""
    P = make_params(sigma, 0.0, NWien, nSim, nDisp, kWien, pWien, tau_2D, tau_4D, tau_5D, useSD, color_space)
    (ctx or _ctx()).step2(P, LF_noisy, LF_SAI_mask, LF_basic, LF_denoised, ang_major, awidth, aheight, anWien,
                          width, height, chnls)
    return 0


def run_bm3d_LF(sigma, LF_noisy, LF_SAI_mask, LF_basic, LF_denoised, width, height, chnls, nHard, nWien, kHard, kWien,
                NHard, NWien, pHard, pWien, useSD_h, useSD_w, tau_2D_hard, tau_2D_wien, lambdaHard3D, color_space,
                nb_threads=1, sub_img_name="SAI", ctx=None):
    """Same argument list as the reference's run_bm3d_LF (src/bm3d_LF.h:10-35): BM3D on every SAI of the mask.
    nb_threads is accepted and ignored (untiled, nb_threads == 1 semantics)."""
    hard = make_bm3d_params(sigma, lambdaHard3D, NHard, nHard, kHard, pHard, tau_2D_hard, useSD_h, color_space)
    wien = make_bm3d_params(sigma, lambdaHard3D, NWien, nWien, kWien, pWien, tau_2D_wien, useSD_w, color_space)
    (ctx or _ctx()).bm3d_lf(hard, wien, LF_noisy, LF_SAI_mask, LF_basic, LF_denoised, width, height, chnls)
    return 0


def noise_level(LF, LF_SAI_mask, width, height, chnls, patch=8, per_sai=False, ctx=None):
    """Context.noise_level on the default context (device 0): the blind estimate of the light field's noise sigma."""
    return (ctx or _ctx()).noise_level(LF, LF_SAI_mask, width, height, chnls, patch, per_sai)


def quality(ref, test, mask, width, height, chnls, peak=255.0, ssim=True, ctx=None):
    """Context.quality on the default context (device 0): per-SAI PSNR, RMSE and SSIM of `test` against `ref` and their summary."""
    return (ctx or _ctx()).quality(ref, test, mask, width, height, chnls, peak, ssim)


def pg_estimate(LF, LF_SAI_mask, width, height, chnls, ctx=None):
    """Context.pg_estimate on the default context (device 0): the Poisson-Gaussian noise model of a noisy light field."""
    return (ctx or _ctx()).pg_estimate(LF, LF_SAI_mask, width, height, chnls)


def impulse_repair(noisy, mask, width, height, chnls, k=8.0, threshold=None, flags=None, return_flags=False, ctx=None, **more):
    """Context.impulse_repair on the default context (device 0): detection and repair of impulses ahead of the denoiser."""
    return (ctx or _ctx()).impulse_repair(noisy, mask, width, height, chnls, k=k, threshold=threshold, flags=flags,
                                          return_flags=return_flags, **more)


def inpaint(noisy, flags, mask, P, ang_major, awidth, aheight, an, width, height, chnls, ctx=None, **more):
    """Context.inpaint on the default context (device 0): defect inpainting under a given map, refined by the hard-thresholding step."""
    return (ctx or _ctx()).inpaint(noisy, flags, mask, P, ang_major, awidth, aheight, an, width, height, chnls, **more)


def view_occl_default():
    """The occlusion ratio the library ships (lfbm5d_view_occl_default, host only): what occlusion=True means."""
    return float(lib().lfbm5d_view_occl_default())


def view_synth(noisy, mask, missing, P, ang_major, awidth, aheight, an, width, height, chnls, ctx=None, **more):
    """Context.view_synth on the default context (device 0): missing SAIs synthesised from their angular neighbours, refined by the
    hard-thresholding step."""
    return (ctx or _ctx()).view_synth(noisy, mask, missing, P, ang_major, awidth, aheight, an, width, height, chnls, **more)


def repair(noisy, flags, missing, mask, P, ang_major, awidth, aheight, an, width, height, chnls, ctx=None, **more):
    """Context.repair on the default context (device 0): defective values and missing SAIs repaired together by a mask-aware plane
    sweep, refined by the hard-thresholding step."""
    return (ctx or _ctx()).repair(noisy, flags, missing, mask, P, ang_major, awidth, aheight, an, width, height, chnls, **more)


def consist(noisy, mask, ang_major, awidth, aheight, width, height, chnls, ctx=None, **more):
    """Context.consist on the default context (device 0): defective values and bad SAIs found by cross-view consistency."""
    return (ctx or _ctx()).consist(noisy, mask, ang_major, awidth, aheight, width, height, chnls, **more)


def equalise(noisy, mask, ang_major, awidth, aheight, width, height, chnls, return_hist=False, ctx=None, **params):
    """Context.equalise on the default context (device 0): per-view gains estimated from the other views and divided out."""
    return (ctx or _ctx()).equalise(noisy, mask, ang_major, awidth, aheight, width, height, chnls, return_hist=return_hist, **params)


def denoise_views(sigma_sai, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls, ctx=None):
    """Context.denoise_views on the process-wide context (or `ctx`): the two-step job with one noise level per SAI."""
    return (ctx or _ctx()).denoise_views(sigma_sai, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls)


def corr_measure(LF, LF_SAI_mask, width, height, chnls, block=16, fraction=None, ctx=None):
    """Context.corr_measure on the process-wide context (or `ctx`): the autocorrelation of the noise, measured on the GPU."""
    return (ctx or _ctx()).corr_measure(LF, LF_SAI_mask, width, height, chnls, block, fraction)


def denoise_corr(acf, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls, ctx=None):
    """Context.denoise_corr on the process-wide context (or `ctx`): the two-step job under spatially correlated noise."""
    return (ctx or _ctx()).denoise_corr(acf, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls)


def denoise_pg(model, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls, ctx=None):
    """Context.denoise_pg on the default context (device 0); returns the model that was used."""
    return (ctx or _ctx()).denoise_pg(model, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls)


def noise_level_clipped(LF, LF_SAI_mask, width, height, chnls, lo=0.0, hi=255.0, ctx=None):
    """Context.noise_level_clipped on the default context (device 0): the noise sigma of a light field clipped to lo..hi."""
    return (ctx or _ctx()).noise_level_clipped(LF, LF_SAI_mask, width, height, chnls, lo, hi)


def pgclip_estimate(LF, LF_SAI_mask, width, height, chnls, lo=0.0, hi=255.0, ctx=None):
    """Context.pgclip_estimate on the default context (device 0): the clipped Poisson-Gaussian model of a light field."""
    return (ctx or _ctx()).pgclip_estimate(LF, LF_SAI_mask, width, height, chnls, lo, hi)


def denoise_pgclip(model, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls, lo=0.0, hi=255.0,
                   ctx=None):
    """Context.denoise_pgclip on the default context (device 0); returns (the model applied as a PgclipEstimate, s)."""
    return (ctx or _ctx()).denoise_pgclip(model, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls,
                                          lo, hi)


def denoise_clipped(sigma, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls, lo=0.0, hi=255.0,
                    ctx=None):
    """Context.denoise_clipped on the default context (device 0); returns (sigma applied, the estimate or None)."""
    return (ctx or _ctx()).denoise_clipped(sigma, P1, P2, noisy, mask, basic, denoised, ang_major, awidth, aheight, an1, an2, W, H, chnls,
                                           lo, hi)


def superres(sr, P, low, mask, high, ang_major, awidth, aheight, an, w, h, chnls, ctx=None):
    """Context.superres on the default context (device 0)."""
    (ctx or _ctx()).superres(sr, P, low, mask, high, ang_major, awidth, aheight, an, w, h, chnls)
    return 0


_TAU = {"id": 4, "dct": 5, "sadct": 6, "bior": 7, "hw": 8, "hadamard": 8, "haar": 9}
_CS = {"yuv": 0, "ycbcr": 1, "opp": 2, "rgb": 3}


def dropin_probe(noisy, mask, awidth, aheight, width, height, chnls, sigma, lambda_, hard, wien, color_space="opp", ang_major=ROWMAJOR,
                 an=(1, 1), one_job=False, reps=1):
    """Time the reference's own interval through the C++ drop-in (liblfbm5d_dropin.so: run_bm5d_1st_step + run_bm5d_2nd_step on
    vector<vector<float>> light fields, main.cpp:189-201 + :241-247; one_job: run_bm5d).  hard / wien = (N, nSim, nDisp, k, p,
    tau_2D, tau_4D, tau_5D[, useSD]).  Returns (ms [reps][2], noisy, basic, denoised) -- the light fields as the calls leave them."""
    path = os.path.join(os.path.dirname(library_path()), "liblfbm5d_dropin.so")
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    D = C.CDLL(path)
    D.lfbm5d_dropin_probe.argtypes = ([C.c_int] + [C.c_void_p] * 5 + [C.c_uint] * 8 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_uint,
                                      C.c_int, C.c_void_p])

    def pk(t):
        t = tuple(t)
        v = [t[0], t[1], t[2], t[3], t[4], int(t[8]) if len(t) > 8 else 0, _TAU[t[5]], _TAU[t[6]], _TAU[t[7]]]
        return np.array(v, np.uint32)
    noisy = np.ascontiguousarray(noisy, np.float32)
    m = _u32(mask)
    n_out, b_out, d_out = np.zeros_like(noisy), np.zeros_like(noisy), np.zeros_like(noisy)
    ms = np.zeros((reps, 2), np.float64)
    h, w = pk(hard), pk(wien)
    rc = D.lfbm5d_dropin_probe(1 if one_job else 0, noisy.ctypes.data, m.ctypes.data, n_out.ctypes.data, b_out.ctypes.data, d_out.ctypes.data,
                               ang_major, awidth, aheight, an[0], an[1], width, height, chnls, sigma, lambda_, h.ctypes.data, w.ctypes.data,
                               _CS[color_space] if isinstance(color_space, str) else int(color_space), reps, ms.ctypes.data)
    if rc != 0:
        raise LfBm5dError("drop-in probe failed (message on stdout)")
    return ms, n_out, b_out, d_out


def denoise_views_probe(noisy, mask, sigma_sai, awidth, aheight, width, height, chnls, lambda_, hard, wien, color_space="opp",
                        ang_major=ROWMAJOR, an=(1, 1)):
    """denoise_views_LF of the C++ drop-in (run_bm5d.h) on vector<vector<float>> light fields built from `noisy` [asize][C*H*W] (float32
    numpy): (noisy, basic, denoised as the call leaves them, the table applied, the window sigmas).  sigma_sai None: the estimate.
    hard / wien = (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D) with transform names, as in dropin_probe."""
    import ctypes
    D = ctypes.CDLL(os.path.join(_HERE, "liblfbm5d_dropin.so"))
    dp = C.POINTER(C.c_double)
    D.lfbm5d_denoise_views_probe.argtypes = ([C.c_void_p] * 2 + [dp, dp] + [C.c_void_p] * 3 + [C.c_uint] * 8 + [C.c_float, C.c_void_p, C.c_void_p,
                                             C.c_uint, C.c_void_p, C.c_uint, C.POINTER(C.c_uint)])

    def pk(t):
        N, nSim, nDisp, k, p, t2, t4, t5 = t
        return np.array([N, nSim, nDisp, k, p, 0, TAU[t2], TAU[t4], TAU[t5]], np.uint32)
    noisy = np.ascontiguousarray(noisy, dtype=np.float32)
    m = _u32(mask)
    asize = m.size
    t = None if sigma_sai is None else np.ascontiguousarray(np.asarray(sigma_sai, np.float64).reshape(-1))
    used = np.zeros(max(asize, 1), np.float64)
    outs = [np.zeros_like(noisy) for _ in range(3)]
    h, w = pk(hard), pk(wien)
    win = np.zeros(4 * asize + 8, np.float32)
    n_win = C.c_uint()
    rc = D.lfbm5d_denoise_views_probe(noisy.ctypes.data, m.ctypes.data, None if t is None else t.ctypes.data_as(dp), used.ctypes.data_as(dp),
                                      outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, ang_major, awidth, aheight, an[0], an[1],
                                      width, height, chnls, float(lambda_), h.ctypes.data, w.ctypes.data, COLOR_SPACE[color_space],
                                      win.ctypes.data, win.size, C.byref(n_win))
    if rc != 0:
        raise LfBm5dError("denoise_views_LF failed (its message is on stdout)")
    return outs[0], outs[1], outs[2], used[:asize], win[:min(n_win.value, win.size)].copy()


def superres_probe(low, mask, awidth, aheight, width, height, chnls, sr, lambda_, hard, color_space="opp", ang_major=ROWMAJOR, an=1):
    """The C++ drop-in's superres_LF (liblfbm5d_dropin.so, run_bm5d.h) on vector<vector<float>> light fields built from `low`
    [asize][chnls*height*width]; hard = (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D[, useSD]).  Returns the high-resolution light field."""
    path = os.path.join(os.path.dirname(library_path()), "liblfbm5d_dropin.so")
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    D = C.CDLL(path)
    D.lfbm5d_superres_probe.argtypes = [C.c_void_p] * 3 + [C.c_uint] * 7 + [C.c_void_p] * 3 + [C.c_uint]
    t = tuple(hard)
    hv = np.array([t[0], t[1], t[2], t[3], t[4], int(t[8]) if len(t) > 8 else 0, _TAU[t[5]], _TAU[t[6]], _TAU[t[7]]], np.uint32)
    low = np.ascontiguousarray(low, np.float32)
    m = _u32(mask)
    out = np.zeros((low.shape[0], low[0].size * sr.scale * sr.scale), np.float32)
    su = np.array([sr.scale, sr.kernel, sr.iterations], np.uint32)
    sf = np.array([sr.blur_sigma, sr.sigma_start, sr.sigma_end, lambda_], np.float32)
    rc = D.lfbm5d_superres_probe(low.ctypes.data, m.ctypes.data, out.ctypes.data, ang_major, awidth, aheight, an, width, height, chnls,
                                 su.ctypes.data, sf.ctypes.data, hv.ctypes.data, _CS[color_space] if isinstance(color_space, str) else int(color_space))
    if rc != 0:
        raise LfBm5dError("superres_LF failed (message on stdout)")
    return out



def inpaint_probe(noisy, flags, mask, awidth, aheight, width, height, chnls, lambda_, hard, iterations=-1, sigma_start=0.0, sigma_end=0.0,
                  sigma_noise=0.0, color_space="opp", ang_major=ROWMAJOR, an=1):
    """The C++ drop-in's inpaint_LF (liblfbm5d_dropin.so, run_bm5d.h) on vector<vector<float>> light fields built from `noisy` and `flags`
    [asize][chnls*height*width]; hard = (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D[, useSD]).  Returns (the repaired light field,
    flagged, left, passes)."""
    path = os.path.join(os.path.dirname(library_path()), "liblfbm5d_dropin.so")
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    D = C.CDLL(path)
    D.lfbm5d_inpaint_probe.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 7 + [C.c_int] + [C.c_void_p] * 2 + [C.c_uint, C.c_void_p]
    t = tuple(hard)
    hv = np.array([t[0], t[1], t[2], t[3], t[4], int(t[8]) if len(t) > 8 else 0, _TAU[t[5]], _TAU[t[6]], _TAU[t[7]]], np.uint32)
    noisy = np.ascontiguousarray(noisy, np.float32)
    fl = np.ascontiguousarray(flags, np.uint8)
    m = _u32(mask)
    out = noisy.copy()
    ipf = np.array([sigma_start, sigma_end, sigma_noise, lambda_], np.float32)
    counts = np.zeros(3, np.uint64)
    rc = D.lfbm5d_inpaint_probe(noisy.ctypes.data, fl.ctypes.data, m.ctypes.data, out.ctypes.data, ang_major, awidth, aheight, an, width, height,
                                chnls, int(iterations), ipf.ctypes.data, hv.ctypes.data,
                                _CS[color_space] if isinstance(color_space, str) else int(color_space), counts.ctypes.data)
    if rc != 0:
        raise LfBm5dError("inpaint_LF failed (message on stdout)")
    return out, int(counts[0]), int(counts[1]), int(counts[2])


def view_synth_probe(noisy, mask, missing, awidth, aheight, width, height, chnls, lambda_, hard, max_disparity=-1, box_radius=-1, ang_radius=-1,
                     iterations=-1, sigma_start=0.0, sigma_end=0.0, sigma_noise=0.0, color_space="opp", ang_major=ROWMAJOR, an=1, disparity_steps=1,
                     occl_ratio=0.0):
    """The C++ drop-in's view_synth_LF (liblfbm5d_dropin.so, run_bm5d.h) on a vector<vector<float>> light field built from `noisy`
    [asize][chnls*height*width] (the vectors of missing SAIs are left empty); hard = (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D[, useSD]).
    disparity_steps: view_synth_LF's trailing argument (dmin and dmax are then in units of 1 / disparity_steps).  occl_ratio: the one
    behind it; a sixth value is then returned, the positions per set chosen (5 counters).
    Returns (the completed light field, synthesised, left, dmin, dmax)."""
    path = os.path.join(os.path.dirname(library_path()), "liblfbm5d_dropin.so")
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    D = C.CDLL(path)
    D.lfbm5d_view_synth_probe.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 7 + [C.c_void_p] * 3 + [C.c_uint, C.c_void_p]
    t = tuple(hard)
    hv = np.array([t[0], t[1], t[2], t[3], t[4], int(t[8]) if len(t) > 8 else 0, _TAU[t[5]], _TAU[t[6]], _TAU[t[7]]], np.uint32)
    noisy = np.ascontiguousarray(noisy, np.float32)
    m, ms = _u32(mask), _u32(missing)
    out = noisy.copy()
    vpi = np.array([max_disparity, box_radius, ang_radius, iterations], np.int32)
    vpf = np.array([sigma_start, sigma_end, sigma_noise, lambda_], np.float32)
    counts = np.zeros(4, np.int32)
    D.lfbm5d_view_synth_steps_probe.argtypes = D.lfbm5d_view_synth_probe.argtypes + [C.c_uint]
    args = (noisy.ctypes.data, m.ctypes.data, ms.ctypes.data, out.ctypes.data, ang_major, awidth, aheight, an, width, height, chnls,
            vpi.ctypes.data, vpf.ctypes.data, hv.ctypes.data, _CS[color_space] if isinstance(color_space, str) else int(color_space),
            counts.ctypes.data)
    sets = np.zeros(5, np.uint64)
    if float(occl_ratio) != 0.0:
        D.lfbm5d_view_synth_occl_probe.argtypes = D.lfbm5d_view_synth_steps_probe.argtypes + [C.c_float, C.c_void_p]
        rc = D.lfbm5d_view_synth_occl_probe(*args, int(disparity_steps), float(occl_ratio), sets.ctypes.data)
    else:
        rc = D.lfbm5d_view_synth_probe(*args) if int(disparity_steps) == 1 else D.lfbm5d_view_synth_steps_probe(*args, int(disparity_steps))
    if rc != 0:
        raise LfBm5dError("view_synth_LF failed (message on stdout)")
    res = (out, int(counts[0]), int(counts[1]), int(counts[2]), int(counts[3]))
    return res + (tuple(int(v) for v in sets),) if float(occl_ratio) != 0.0 else res


def consist_probe(noisy, mask, awidth, aheight, width, height, chnls, exclude=None, max_disparity=-1, box_radius=-1, ang_radius=-1,
                  min_sources=-1, max_rounds=-1, k=-1.0, spread=-1.0, sai_factor=-1.0, ang_major=ROWMAJOR, disparity_steps=1):
    """The C++ drop-in's consist_LF (liblfbm5d_dropin.so, run_bm5d.h) on a vector<vector<float>> light field built from `noisy`
    [asize][chnls*height*width]; disparity_steps: its trailing argument.  Returns (flags uint8 like noisy, state int64 [asize], flagged, nonfinite, bad, untested, rounds,
    the three channel scales)."""
    path = os.path.join(os.path.dirname(library_path()), "liblfbm5d_dropin.so")
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    D = C.CDLL(path)
    D.lfbm5d_consist_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint] * 6 + [C.c_void_p] * 4
    noisy = np.ascontiguousarray(noisy, np.float32)
    m = _u32(mask)
    ex = None if exclude is None else _u32(exclude)
    flags = np.zeros(noisy.shape, np.uint8)
    state = np.zeros(m.size, np.uint32)
    cpi = np.array([max_disparity, box_radius, ang_radius, min_sources, max_rounds], np.int32)
    cpd = np.array([k, spread, sai_factor], np.float64)
    counts, scales = np.zeros(5, np.uint64), np.zeros(3, np.float64)
    D.lfbm5d_consist_steps_probe.argtypes = D.lfbm5d_consist_probe.argtypes + [C.c_uint]
    args = (noisy.ctypes.data, m.ctypes.data, None if ex is None else ex.ctypes.data, flags.ctypes.data, state.ctypes.data, ang_major, awidth,
            aheight, width, height, chnls, cpi.ctypes.data, cpd.ctypes.data, counts.ctypes.data, scales.ctypes.data)
    rc = D.lfbm5d_consist_probe(*args) if int(disparity_steps) == 1 else D.lfbm5d_consist_steps_probe(*args, int(disparity_steps))
    if rc != 0:
        raise LfBm5dError("consist_LF failed (message on stdout)")
    return (flags, state.astype(np.int64)) + tuple(int(v) for v in counts) + (tuple(scales),)


def equalise_probe(noisy, mask, awidth, aheight, width, height, chnls, max_disparity=-1, box_radius=-1, ang_radius=-1, min_sources=-1,
                   max_rounds=-1, per_channel=-1, anchor=-1, tol=-1.0, lo=-1.0, hi=-1.0, ang_major=ROWMAJOR, disparity_steps=1, restore=False):
    """The C++ drop-in's equalise_LF (liblfbm5d_dropin.so, run_bm5d.h) on a vector<vector<float>> light field built from `noisy`
    [asize][chnls*height*width]; restore: apply_gains_LF(invert) on its output afterwards.  Negative parameters keep the library's
    defaults.  Returns (out float32 like noisy, planes of empty SAIs zero; gain float64 [asize][3]; state; fitted, untested, unfit,
    rounds; residual, gain_min, gain_max)."""
    D = C.CDLL(os.path.join(_HERE, "liblfbm5d_dropin.so"))
    D.lfbm5d_equalise_probe.argtypes = [C.c_void_p] * 3 + [C.c_uint] * 6 + [C.c_void_p] * 6 + [C.c_int]
    x = np.ascontiguousarray(noisy, np.float32)
    m = _u32(mask)
    out = np.zeros_like(x)
    gain, state = np.zeros((m.size, 3), np.float64), np.zeros(m.size, np.uint32)
    ppi = np.array([max_disparity, box_radius, ang_radius, min_sources, max_rounds, per_channel, anchor, disparity_steps], np.int32)
    ppd = np.array([tol, lo, hi], np.float64)
    counts, figures = np.zeros(4, np.uint32), np.zeros(3, np.float64)
    if D.lfbm5d_equalise_probe(x.ctypes.data, m.ctypes.data, out.ctypes.data, ang_major, awidth, aheight, width, height, chnls, ppi.ctypes.data,
                               ppd.ctypes.data, gain.ctypes.data, state.ctypes.data, counts.ctypes.data, figures.ctypes.data, int(bool(restore))) != 0:
        raise LfBm5dError("equalise_LF failed (message on stdout)")
    return (out, gain, state.astype(np.int64), *(int(v) for v in counts), *(float(v) for v in figures))


def repair_probe(noisy, flags, mask, missing, awidth, aheight, width, height, chnls, lambda_, hard, max_disparity=-1, box_radius=-1,
                 ang_radius=-1, min_valid=-1, iterations=-1, sigma_start=0.0, sigma_end=0.0, sigma_noise=0.0, color_space="opp",
                 ang_major=ROWMAJOR, an=1):
    """The C++ drop-in's repair_LF (liblfbm5d_dropin.so, run_bm5d.h) on vector<vector<float>> light fields built from `noisy` and `flags`
    [asize][chnls*height*width] (flags or missing None: an empty vector); hard = (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D[, useSD]).
    Returns (the repaired light field, counts = (values, flagged, missing, from other views, from the rim, left), dmin, dmax)."""
    path = os.path.join(os.path.dirname(library_path()), "liblfbm5d_dropin.so")
    if not os.path.exists(path):
        raise LfBm5dError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    D = C.CDLL(path)
    D.lfbm5d_repair_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint] * 7 + [C.c_void_p] * 3 + [C.c_uint, C.c_void_p, C.c_void_p]
    t = tuple(hard)
    hv = np.array([t[0], t[1], t[2], t[3], t[4], int(t[8]) if len(t) > 8 else 0, _TAU[t[5]], _TAU[t[6]], _TAU[t[7]]], np.uint32)
    noisy = np.ascontiguousarray(noisy, np.float32)
    fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
    m, ms = _u32(mask), None if missing is None else _u32(missing)
    out = noisy.copy()
    rpi = np.array([max_disparity, box_radius, ang_radius, min_valid, iterations], np.int32)
    rpf = np.array([sigma_start, sigma_end, sigma_noise, lambda_], np.float32)
    res, rng = np.zeros(6, np.uint64), np.zeros(2, np.int32)
    rc = D.lfbm5d_repair_probe(noisy.ctypes.data, None if fl is None else fl.ctypes.data, m.ctypes.data, None if ms is None else ms.ctypes.data,
                               out.ctypes.data, ang_major, awidth, aheight, an, width, height, chnls, rpi.ctypes.data, rpf.ctypes.data,
                               hv.ctypes.data, _CS[color_space] if isinstance(color_space, str) else int(color_space),
                               res.ctypes.data, rng.ctypes.data)
    if rc != 0:
        raise LfBm5dError("repair_LF failed (message on stdout)")
    return out, tuple(int(v) for v in res), int(rng[0]), int(rng[1])
