/*
 * lfbm5d_ctx.h -- what the host side of the library shares between its translation units (round 6: lfbm5d_api.hip, 2 500 lines,
 * was split along its seams):
 *   lfbm5d_pass.hip    one core pass (bm5d_1st_step / bm5d_2nd_step) as a sequence of kernels: geometry, tables, block matching,
 *                      group stage, aggregation; counters and event times
 *   lfbm5d_graph.hip   a job's windows as a dependency graph on lanes and ranks: run_graph, the RCCL and IPC transports, the
 *                      streamed host seam
 *   lfbm5d_steps.hip   run_bm5d_1st_step / run_bm5d_2nd_step / both as one job on device buffers: schedule forms, tile mode
 *   lfbm5d_api.hip     the C-ABI of include/lfbm5d.h: context, options, communicators, host entry points, BM3D, inspection
 *   lfbm5d_side.h      the host frame of the side stages (lfbm5d_noise / quality / resample / pg / impulse / inpaint / view / consist / photo / repair.hip):
 *                      SAI list, argument checks, staging of per-SAI host planes, the refinement loop, the sweep's source rows
 *   lfbm5d_side_values.h   what those stages share per value, host-and-device and free of HIP headers: tile, mirror, bit tests, key
 *                      layout, thresholds, the loop's sigma schedule
 * Internal: nothing here is part of the ABI.
 */
#ifndef LFBM5D_CTX_H
#define LFBM5D_CTX_H

#include "../../include/lfbm5d.h"
#include "lfbm5d_kernels.h"
#include "lfbm5d_plan.h"
#include "lfbm5d_options.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <fstream>
#include <thread>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>


namespace lfbm5d_host {

using namespace lfbm5d;



constexpr double kSqrt2 = 1.414213562373095;     /* core:33 */
constexpr double kSqrt2Inv = 0.7071067811865475; /* core:34 */
constexpr double kPi = 3.14159265358979323846;

struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PassEvents { hipEvent_t e[5]; bool comm; };

struct GeomCache {
    DevBuf refs, rslot, tb, scan_wgs;
    std::vector<Scan2Wg> scan_plan; unsigned scan_key[8] = {0, 0, 0, 0, 0, 0, 0, 0}; size_t scan_lds = 0;
    unsigned scan_nwg_slot = 0; int scan_version = 0;
    std::vector<unsigned> last_refs_host;
    unsigned grid_key[5] = {0, 0, 0, 0, 0};      /* cached reference grid */
    unsigned rslot_key[5] = {0, 0, 0, 0, 0};     /* geometry rslot / n_ref_rows / n_ref_cols were built for (survives a subset pass, which replaces refs) */
    unsigned tb_key[3] = {0, 0, 0};
    unsigned n_ref_rows = 0, n_ref_cols = 0;
};

} /* namespace lfbm5d_host */

using lfbm5d_host::DevBuf; using lfbm5d_host::PassEvents; using lfbm5d_host::GeomCache; using lfbm5d::Options;


/* window lanes of the graph form when LFBM5D_LANES does not say (same-box sweep at the headline workload, round 4: one lane 194,
 * two 220, three 211, four 210, five / six 215 SAI-MP/s -- the table kernel fills the register files of the CUs it runs on, so
 * a third window mostly queues) */
constexpr int kDefaultLanes = 2;
constexpr size_t kEstLead = 64;   /* floats of slack in front of the estimate planes */

/* The caller's light fields of a *_host entry point: one host pointer per SAI (ignored for empty SAIs).  `basic` is an input of
 * run_bm5d_2nd_step only; `out` is the denoised light field of the second step (unused by the first, whose result is `basic`). */
struct HostIO {
    float* const* noisy = nullptr;
    float* const* basic = nullptr;
    float* const* out = nullptr;
};

struct lfbm5d_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int rank = 0, world = 1;
    int tiles = 1;                         /* > 1: the reference's OpenMP tile mode (lfbm5d_set_tiles) */
    ncclComm_t comm = nullptr;
    ncclComm_t comm2 = nullptr;            /* second channel of the window-graph exchange (ncclCommSplit of comm) */
    hipStream_t cs[2] = {nullptr, nullptr}; /* exchange streams, one per channel */
    /* sharding actually applied inside a core pass: rows of reference patches over pass_world ranks (direct
     * lfbm5d_pass_device calls use rank/world; whole steps on several GPUs shard by WINDOWS instead and run
     * every pass unsharded) */
    int pass_rank = 0, pass_world = 1;
    bool pass_reduce = false;
    std::vector<unsigned> last_windows;   /* processed SAI of every window of the last step, in order */
    /* per-view noise levels (include/lfbm5d_views.h): the view table of the job that is running (empty: none; set and cleared by the
     * lfbm5d_*_views_* entry points, lfbm5d_views.hip), and the sigma applied to every window of last_windows */
    struct ViewSigmas { std::vector<double> table; std::vector<float> last; } views;
    lfbm5d_stats stats;
    /* per-pass work buffers (grow only) */
    DevBuf t_noisy, t_basic, t_tnum, t_tden, und_num, und_den;   /* tile mode: one tile of the window, the tiles' interiors */
    DevBuf scan_lcol;                      /* second-generation scan: hand-off columns */
    DevBuf sub_flags, sub_cnt;             /* subset passes: the device-side reference list's scratch and count */
    int last_scan_version = 0;
    /* what a pass derives from its geometry alone (reference grid, transform tables, the table kernel's workgroup list):
     * cached, one set per step slot so that the windows of both steps of a two-step job can alternate on a lane without
     * re-uploading (and without the stream synchronisation an upload from a stack object needs) */
    GeomCache gc[2]; int gslot = 0;
    bool est_ready = false;                /* the caller of pass_impl has formed the matching estimate in `est` already (graph form) */
    /* direct sums (graph form, single-pass windows): the next pass_impl on this context aggregates straight into the light field's
     * num / den (AggArgs::direct) and reads nothing of its d_num / d_den arguments; consumed by that call like est_ready */
    struct DirectSums { bool on = false; float* num = nullptr; float* den = nullptr; size_t lf_stride = 0; lfbm5d::SaiList sai; } direct;
    DevBuf est, refmap, scores, tables, self_idx, self_cnt, best, shape, filt, wgt, aggpos, gpos, gofs, gok, sa_list, gshape, counters, small, t_num, t_den, d_mask;
    /* step-level buffers (g_num2 / g_den2 / n2: second step of a two-step job; e_basic: an emulated rank's own basic estimate) */
    DevBuf g_num, g_den, g_num2, g_den2, n2, e_basic, w_noisy, w_basic, w_num, w_den, h2d_noisy, h2d_basic, h2d_out, d_own, gscratch;
    /* streamed host seam (lfbm5d_*_host): the caller's light fields as host pointers per SAI, set for the duration of a job; the
     * job's inputs as they arrived (what a redo of the job starts from: the streamed outputs overwrite the caller's copies SAI by
     * SAI); the streams the uploads / downloads go through */
    /* second transport of the window-graph exchange, for tests: the ranks are PROCESSES ON ONE GPU (RCCL refuses that), a message is a
     * device copy out of the peer's buffers (hipIpcMemHandle) gated by words in mapped device memory; same graph, issue order, event
     * gating and abort path as the RCCL form (lfbm5d_comm_init_ipc) */
    bool ipc = false;
    std::string ipc_dir; double ipc_timeout_s = 30.0; unsigned ipc_epoch = 0;
    std::string ipc_tag;   /* prefix of the rendezvous names: "" for the whole world, "b<band>." while a band's team runs its job (spatial bands) */
    DevBuf ipc_flags, ipc_out;
    struct IpcPeer { unsigned char handle[7][64]; void* ptr[7]; };   /* flags, g_num[0..1], g_den[0..1], basic, out -- as this process maps them */
    std::vector<IpcPeer> ipc_peers;
    DevBuf pristine, pristine_b;
    /* spatial bands (option spatial_bands, lfbm5d_steps.hip): a band's crop of the three light fields, the input as it arrived (emulated
     * ranks), the all-gather's buffers; the communicators of this rank's team (split from comm once per band count) */
    DevBuf band_noisy, band_basic, band_out, band_src, band_pack, band_gather;
    ncclComm_t team_comm = nullptr, team_comm2 = nullptr; int team_S = 0;
    /* run-time options (lfbm5d_options.h): filled from the environment once at lfbm5d_create, changed by lfbm5d_set_option; lane contexts
     * point at their parent's */
    Options opt_store; Options* opt = &opt_store;
    hipStream_t io_in = nullptr, io_out = nullptr;
    unsigned* h_small = nullptr; /* pinned, 64 uints */
    /* what the side stages share (lfbm5d_side.h): the non-empty SAIs of the last mask on the device and on the host (sai_list), the
     * scratch light field a step or a job is handed as its input (scratch_lf: the refinement loop, the inpainting fill's second value plane,
     * the Poisson-Gaussian job's stabilised light field) */
    struct SideBufs { DevBuf sai, lf; std::vector<unsigned> sai_host; } side;
    /* noise-level estimate (lfbm5d_noise.hip): bulk partial sums, lag cells, centred scatters, pooled covariances */
    struct NoiseBufs { DevBuf part, cells, m, pool; } noise;
    /* quality metrics (lfbm5d_quality.hip): the workgroups' partial sums, the two sums of every SAI */
    struct QualityBufs { DevBuf part, out; } quality;
    /* super-resolution (lfbm5d_resample.hip): the tap tables of U and D for the geometry in `key` (host copy, word offsets of first / w of
     * Ux, Uy, Dx, Dy, their tap counts), the back-projection's low-resolution residual */
    struct SrBufs {
        DevBuf tab, lo;
        std::vector<unsigned> host;
        unsigned key[5] = {0, 0, 0, 0, 0}; size_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned T[4] = {0, 0, 0, 0};
    } sr;
    /* Poisson-Gaussian noise (lfbm5d_pg.hip): the statistics kernel's counters */
    struct PgBufs { DevBuf stats; } pg;
    /* clipping-aware estimate (lfbm5d_clip.hip): the statistics kernel's counters */
    struct ClipBufs { DevBuf stats; } clip;
    /* clipped Poisson-Gaussian stage (lfbm5d_pgclip.hip): the forward and the inverse table */
    struct PgclipBufs { DevBuf tables; } pgclip;
    /* impulse repair (lfbm5d_impulse.hip): the kernels' counters, the host form's flag planes (in, out) */
    struct ImpulseBufs { DevBuf stats, flags; } imp;
    /* defect inpainting (lfbm5d_inpaint.hip): the fill's counters, its state planes, the host form's flag planes (in, out) */
    struct InpaintBufs { DevBuf stats, state[2], flags; } inp;
    /* view synthesis (lfbm5d_view.hip): the source lists, the disparity and set histograms, the host form's disparity and set planes */
    struct ViewBufs { DevBuf table, stats, disp, set; } view;
    /* consistency check (lfbm5d_consist.hip): the leave-one-out source lists, histograms and counters, the prediction light field, the
     * sweep's disparity planes, the host form's flag and disparity planes */
    struct ConsistBufs { DevBuf table, stats, pred, disp, flags; } consist;
    /* photometric equalisation (lfbm5d_photo.hip): the apply kernel's planes and factors (and the host vectors they are copied from),
     * the leave-one-out source lists, histograms and counters, the prediction light field, the sweep's disparity planes, the host
     * form's output light field */
    struct PhotoBufs { DevBuf table, sweep_table, stats, pred, disp, x; std::vector<unsigned> planes_host; std::vector<float> factors_host; } photo;
    /* joint repair (lfbm5d_repair.hip): the validity planes, the sweep's copy of the input and the flags of what is still unsound, the
     * unsound positions per tile, the source lists with the float tables and the missing list, the counters, the code planes when the
     * caller wants none, the host form's flag, code and disparity planes */
    struct RepairBufs { DevBuf valid, mid, rem, tiles, table, stats, codes, host; } repair;
    /* correlated noise (include/lfbm5d_corr.h, lfbm5d_corr.hip).  The variance tables of the job that is running, one per step
     * ([2][k*k] floats each: s, then v; `n` of them, found by the pass's tau_2D and k), set and cleared by the lfbm5d_*_corr_* entry
     * points like views.table; lane contexts point at their parent's.  The measurement's per-block lag sums, scores and chunk sums. */
    struct CorrTables { unsigned n = 0, tau2[2] = {0, 0}, k[2] = {0, 0}; size_t off[2] = {0, 0}; DevBuf dev; };
    CorrTables corr_store; CorrTables* corr = &corr_store;
    struct CorrBufs { DevBuf lags, score, part; } corrm;
    /* window lanes (run_graph; the per-SAI BM3D steps): extra contexts on the same device, each with its own stream, window
     * buffers and per-pass work buffers; owned by this context */
    std::vector<lfbm5d_ctx*> lanes;
    unsigned* h_counts = nullptr; size_t h_counts_cap = 0;   /* pinned: coverage count of every window of a step */
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    std::vector<PassEvents> pending;
    /* last pass (inspection) */
    unsigned last_n_refs = 0, last_N = 0, last_A = 0; size_t last_plane = 0; int last_gslot = 0;   /* geometry slot of that pass */
    /* ... whose score table was not filled in front of the table kernel (pass_impl): lfbm5d_last_scores writes `fill` into the
     * entries that kernel left out before it copies the table (launch_scores_patch), once */
    struct UnfilledScores { bool pending = false; unsigned n_rows = 0, n_cols = 0, W = 0, nSim = 0, nHW = 0, p = 0, last_r = 0, last_c = 0; float fill = 0; } unfilled;
    /* lfbm5d_debug_aggregate: the transform tables (build_tables) of patch size `k`, apart from the passes' cached ones */
    struct DebugAgg { DevBuf tb; unsigned k = 0; } dbg_agg;
    /* lfbm5d_debug_group: likewise, for patch size and window key[0..2] */
    struct DebugGroup { DevBuf tb; unsigned key[3] = {0, 0, 0}; } dbg_group;
};

namespace lfbm5d_host {


#define HIPCK(ctx, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

inline int fail(lfbm5d_ctx* c, const std::string& m) { c->err = m; return 1; }

/* lfbm5d_pass.hip */
lfbm5d_ctx* new_ctx(int device, std::string& err);
hipEvent_t get_event(lfbm5d_ctx* c);
void drain_events(lfbm5d_ctx* c);
int sigma_table(float sigma, unsigned C, unsigned cs, float* out);
void ind_init(std::vector<unsigned>& v, unsigned max_size, unsigned N, unsigned step);
void build_tables(GroupTables& t, unsigned k, unsigned aw, unsigned ah);
bool is_pow2(unsigned n);
int validate(lfbm5d_ctx* c, int step, const lfbm5d_params* P, unsigned aw, unsigned ah, unsigned C, bool bm3d = false);
/* images that are mirror-padded by nHW pixels must be at least that wide and high */
int check_padding(lfbm5d_ctx* c, unsigned W, unsigned H, unsigned nHW);
/* the part of GroupArgs that follows from the pass's parameters (thresholds, lambda rule, sigma table, options, scratch) */
int group_args_of_pass(lfbm5d_ctx* c, lfbm5d::GroupArgs& ga, const lfbm5d_params* P);
/* the variance table (include/lfbm5d_corr.h) launch_group takes with these arguments; NULL when the running job has none */
const float* corr_table_of_pass(lfbm5d_ctx* c, const lfbm5d::GroupArgs& ga);
int fold_counters(lfbm5d_ctx* c, const lfbm5d_params* P, unsigned A, unsigned C, int step, int slot = 0);
/* A lane's (or an emulated rank's) counters and event times into the job's context: every field a pass adds to.  Not added:
 * windows, messages, lane_windows -- the job counts those on its own context as it enqueues, a lane's are zero; ms_comm -- the
 * job's exchange is timed on its own stream, a lane's pass is never sharded; ms_other -- nothing accumulates it. */
inline void add_stats(lfbm5d_stats& dst, const lfbm5d_stats& src) {
    static_assert(sizeof(lfbm5d_stats) == 15 * 8, "lfbm5d_stats has a new field: add it below or name it above");
    dst.passes += src.passes; dst.groups += src.groups; dst.stack_patches += src.stack_patches; dst.sadct_groups += src.sadct_groups;
    dst.algorithmic_bytes += src.algorithmic_bytes;
    dst.ms_bm += src.ms_bm; dst.ms_group += src.ms_group; dst.ms_aggregate += src.ms_aggregate;
    dst.launches_group += src.launches_group; dst.launches_aggregate += src.launches_aggregate;
}
/* lfbm5d_pass.hip */
int pass_impl(lfbm5d_ctx* c, int step, const lfbm5d_params* P, unsigned aw, unsigned ah, unsigned Wb,
              unsigned Hb, unsigned C, const float* d_noisy, const float* d_basic, float* d_num,
              float* d_den, const unsigned* h_mask, const unsigned* h_proc, unsigned cst, unsigned pst,
              bool bm3d = false);
/* lfbm5d_graph.hip */
int io_upload_all(lfbm5d_ctx* c, const HostIO* io, const unsigned* h_mask, unsigned asize, size_t img, float* d_noisy, float* d_basic_in);
int io_download_all(lfbm5d_ctx* c, const HostIO* io, const unsigned* h_mask, unsigned asize, size_t img, const float* d_noisy,
                    const float* d_basic, const float* d_out);
constexpr unsigned kIpcMaxMsgs = 4096;   /* gating words: ready[kIpcMaxMsgs], taken[kIpcMaxMsgs], error */
int auto_bands(unsigned awidth, unsigned aheight, unsigned height, unsigned halo, int world);   /* lfbm5d_steps.hip: lfbm5d_auto_bands */
int ipc_allgather(lfbm5d_ctx* c, const char* tag, int mine, std::vector<int>& all);
bool ipc_put(const std::string& dir, const std::string& name, const void* data, size_t bytes);
bool ipc_get(const std::string& dir, const std::string& name, void* data, size_t bytes, double timeout_s);
/* lfbm5d_steps.hip */
int run_step(lfbm5d_ctx* c, int step, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask,
             float* d_basic, float* d_out, unsigned ang_major, unsigned awidth, unsigned aheight,
             unsigned an, unsigned W, unsigned H, unsigned C, const HostIO* io = nullptr);
int run_denoise(lfbm5d_ctx* c, const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy, const unsigned* h_mask, float* d_basic,
                float* d_out, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H,
                unsigned C, const HostIO* io = nullptr);

/* lfbm5d_view.hip: the plane sweep on the context's stream with a caller-built table (d_table: kViewTabStride ints per SAI to synthesise:
 * its index, n, n x (source index, ds, dt); n_sai rows).  steps = 1: k_view_sweep, d_cnt [17] (index d* + 8) is accumulated into;
 * steps = 2 or 4: k_view_sweep_subpel, d_cnt [65] (index j* + 32), max_sources = the largest n of the table (it picks the instantiation).
 * Enqueues only. */
constexpr int kViewTabStride = 2 + 3 * 24;
int view_sweep_launch(lfbm5d_ctx* c, const int* d_table, unsigned n_sai, const float* d_in, float* d_out, signed char* d_disp, unsigned W,
                      unsigned H, unsigned C, int D, int r, unsigned long long* d_cnt, unsigned steps, unsigned max_sources);

} /* namespace lfbm5d_host */
#endif
