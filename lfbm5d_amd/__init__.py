"""lfbm5d_amd -- MI355X-native LFBM5D denoising core.

Host-side mirror of the reference's operator interface for the hot path
(`run_bm5d_1st_step` / `run_bm5d_2nd_step`, src/bm5d.h:11-62, and the inner `bm5d_1st_step` /
`bm5d_2nd_step`, src/bm5d_core_processing.h:6-80) over the C-ABI of include/lfbm5d.h.  All compute
runs in liblfbm5d_hip.so (hand-written HIP for gfx950); there is no CPU fallback: importing works
anywhere, creating a context without a GPU raises.
"""
from .core import (Context, Params, Bm3dParams, Stats, run_bm5d_1st_step, run_bm5d_2nd_step, run_bm3d_LF, shard_rows,
                   YUV, YCBCR, OPP, RGB, ID, DCT, SADCT, BIOR, HADAMARD, HAAR, ROWMAJOR, COLMAJOR,
                   TAU, COLOR_SPACE, LfBm5dError, library_path, build_library, NoiseLevel, noise_level,
                   noise_level_statistic, Quality, quality, quality_summary, SrParams, sr_defaults, sr_taps, superres,
                   SR_BICUBIC, SR_GAUSSIAN, SR_UP, SR_DOWN, PgModelStruct, PgEstimate, pg_model, pg_fit, pg_scale, pg_estimate,
                   denoise_pg, ImpulseParamsStruct, ImpulseResultStruct, ImpulseRepair, impulse_params, impulse_scale, impulse_repair,
                   InpaintParamsStruct, InpaintResultStruct, Inpaint, inpaint_params, inpaint,
                   ViewParamsStruct, ViewResultStruct, ViewOcclResultStruct, ViewSynth, view_params, view_synth, view_occl_default,
                   ConsistParamsStruct, ConsistResultStruct, Consist, consist_params, consist,
                   RepairParamsStruct, RepairResultStruct, Repair, repair_params, repair,
                   PhotoParamsStruct, PhotoResultStruct, Equalise, photo_params, photo_edges, photo_ratio, photo_solve, equalise,
                   ClipEstimateStruct, ClipNoiseLevel, clip_fit, noise_level_clipped, denoise_clipped,
                   PgclipModelStruct, PgclipEstimateStruct, PgclipCurvesStruct, PgclipEstimate, PgclipCurves, pgclip_fit, pgclip_curves,
                   pgclip_estimate, denoise_pgclip, denoise_views, window_sigma, views_from_gains,
                   CorrEstimateStruct, CorrEstimate, CORR_WHITE, corr_measure, corr_from_kernel, corr_table, denoise_corr)
from .synth import add_view_noise, add_correlated_noise

__all__ = ["Context", "Params", "Bm3dParams", "Stats", "run_bm5d_1st_step", "run_bm5d_2nd_step", "run_bm3d_LF", "shard_rows",
           "YUV", "YCBCR", "OPP", "RGB", "ID", "DCT", "SADCT", "BIOR", "HADAMARD", "HAAR",
           "ROWMAJOR", "COLMAJOR", "TAU", "COLOR_SPACE", "LfBm5dError", "library_path",
           "build_library", "NoiseLevel", "noise_level", "noise_level_statistic", "Quality", "quality", "quality_summary",
           "SrParams", "sr_defaults", "sr_taps", "superres", "SR_BICUBIC", "SR_GAUSSIAN", "SR_UP", "SR_DOWN",
           "PgModelStruct", "PgEstimate", "pg_model", "pg_fit", "pg_scale", "pg_estimate", "denoise_pg",
           "ImpulseParamsStruct", "ImpulseResultStruct", "ImpulseRepair", "impulse_params", "impulse_scale", "impulse_repair",
           "InpaintParamsStruct", "InpaintResultStruct", "Inpaint", "inpaint_params", "inpaint",
           "ViewParamsStruct", "ViewResultStruct", "ViewOcclResultStruct", "ViewSynth", "view_params", "view_synth", "view_occl_default",
           "ConsistParamsStruct", "ConsistResultStruct", "Consist", "consist_params", "consist",
           "RepairParamsStruct", "RepairResultStruct", "Repair", "repair_params", "repair",
           "PhotoParamsStruct", "PhotoResultStruct", "Equalise", "photo_params", "photo_edges", "photo_ratio", "photo_solve", "equalise",
           "ClipEstimateStruct", "ClipNoiseLevel", "clip_fit", "noise_level_clipped", "denoise_clipped",
           "PgclipModelStruct", "PgclipEstimateStruct", "PgclipCurvesStruct", "PgclipEstimate", "PgclipCurves", "pgclip_fit", "pgclip_curves",
           "pgclip_estimate", "denoise_pgclip", "denoise_views", "window_sigma", "views_from_gains", "add_view_noise",
           "CorrEstimateStruct", "CorrEstimate", "CORR_WHITE", "corr_measure", "corr_from_kernel", "corr_table", "denoise_corr",
           "add_correlated_noise"]
