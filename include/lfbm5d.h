/*
 * lfbm5d.h -- C-ABI of the MI355X-native LFBM5D denoising core (liblfbm5d_hip.so).
 *
 * The reference (V-Sense/LFBM5D) has no FFI layer; its seam for this path is two pairs of C++ free
 * functions with std::vector arguments:
 *   outer seam  run_bm5d_1st_step  src/bm5d.h:11-35   (called from src/main.cpp:195)
 *               run_bm5d_2nd_step  src/bm5d.h:38-62   (called from src/main.cpp:242)
 *   inner seam  bm5d_1st_step      src/bm5d_core_processing.h:6-42  (called from bm5d.cpp:351)
 *               bm5d_2nd_step      src/bm5d_core_processing.h:44-80 (called from bm5d.cpp:1050)
 * Every entry point below names the reference function it replaces.  Plain pointers, sizes and POD
 * structs only; return value 0 = success, 1 = failure (EXIT_SUCCESS / EXIT_FAILURE like the
 * reference), message via lfbm5d_last_error().  No C++ types, no exceptions cross this boundary.
 * One host thread per context.  All compute runs on the GPU: there is no CPU fallback, creation
 * fails when no HIP device is present.
 *
 * Stream contract: every context launches on a stream of its own (lfbm5d_stream) and is unaware of the
 * caller's streams.  Device buffers handed to an entry point must be READY on entry (whatever the caller
 * queued on them -- fills, copies, kernels -- has completed or the caller's stream has been synchronised);
 * every entry point returns with its results COMPLETE (it synchronises its stream before returning).
 * Several contexts may share a GPU and run concurrently from different host threads.
 *
 * Light-field layout (same as the reference, utilities_LF.cpp:140-146): asize = awidth*aheight
 * sub-aperture images (SAIs), each C planes of H*W float32 (planar, values nominally 0..255),
 * SAI index st = s*awidth + t (ang_major = LFBM5D_ROWMAJOR) or s + t*aheight (LFBM5D_COLMAJOR);
 * buffers are [asize][C*H*W] contiguous.
 */
#ifndef LFBM5D_H
#define LFBM5D_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum ints of the reference (src/bm5d.cpp:36-48) */
#define LFBM5D_YUV       0
#define LFBM5D_YCBCR     1
#define LFBM5D_OPP       2
#define LFBM5D_RGB       3
#define LFBM5D_ID        4
#define LFBM5D_DCT       5
#define LFBM5D_SADCT     6
#define LFBM5D_BIOR      7
#define LFBM5D_HADAMARD  8
#define LFBM5D_HAAR      9
#define LFBM5D_ROWMAJOR  11
#define LFBM5D_COLMAJOR  12

typedef struct lfbm5d_ctx lfbm5d_ctx;

/* The parameter tail of run_bm5d_1st_step / run_bm5d_2nd_step (bm5d.h:11-62). */
typedef struct {
    float    sigma;        /* sigma                                   */
    float    lambda;       /* lambdaHard5D (ignored by step 2)        */
    unsigned N;            /* NHard / NWien                           */
    unsigned nSim;         /* nSim                                    */
    unsigned nDisp;        /* nDisp                                   */
    unsigned k;            /* kHard / kWien                           */
    unsigned p;            /* pHard / pWien                           */
    unsigned useSD;        /* useSD                                   */
    unsigned tau_2D;       /* LFBM5D_ID | _DCT | _BIOR                */
    unsigned tau_4D;       /* LFBM5D_ID | _DCT | _SADCT               */
    unsigned tau_5D;       /* LFBM5D_HADAMARD | _HAAR | _DCT          */
    unsigned color_space;  /* LFBM5D_YUV | _YCBCR | _OPP | _RGB       */
} lfbm5d_params;

/* Counters and HIP-event timings accumulated since the last lfbm5d_reset_stats(). */
typedef struct {
    unsigned long long windows;        /* angular search windows visited                      */
    unsigned long long passes;         /* core passes (bm5d_*_step calls)                     */
    unsigned long long groups;         /* 5-D groups processed on this rank                   */
    unsigned long long stack_patches;  /* sum of nSx_r over those groups                      */
    unsigned long long sadct_groups;   /* groups that used the shape-adaptive 4-D transform   */
    double algorithmic_bytes;          /* sum_groups (4*S + 16) B * nSx*A*k^2*C  */
    double ms_bm;                      /* block-matching kernels, HIP-event time              */
    double ms_group;                   /* 5-D transform + shrink kernel                       */
    double ms_aggregate;               /* aggregation kernel                                  */
    double ms_other;                   /* padding / estimate / reductions / colour            */
    double ms_comm;                    /* RCCL all-reduce                                     */
    unsigned long long launches_group; /* launches of the transform kernel                    */
    unsigned long long launches_aggregate;
    unsigned long long lane_windows;   /* windows that ran on a lane other than the first (pipelined steps) */
    unsigned long long messages;       /* SAI messages (num + den of one SAI) exchanged between ranks, graph form   */
} lfbm5d_stats;

/* ---- context ---- */
/* Binds HIP device `device` (index within the visible devices), creates the stream the whole path
 * runs on.  Fails (returns 1, *out = NULL) when no HIP device is available. */
int  lfbm5d_create(lfbm5d_ctx** out, int device);
void lfbm5d_destroy(lfbm5d_ctx* ctx);
const char* lfbm5d_last_error(const lfbm5d_ctx* ctx); /* ctx may be NULL: creation errors */
void lfbm5d_reset_stats(lfbm5d_ctx* ctx);
void lfbm5d_get_stats(const lfbm5d_ctx* ctx, lfbm5d_stats* out);
/* The HIP stream (hipStream_t) the context launches on, for callers that time with events. */
void* lfbm5d_stream(lfbm5d_ctx* ctx);

/* ---- run-time options (round 6; lfbm5d_amd/csrc/lfbm5d_options.h has the list) ----
 * Every knob of the library is a per-context option.  lfbm5d_create fills them ONCE from the environment (LFBM5D_LANES=3 exported
 * before the context exists still means three window lanes); afterwards they change only through lfbm5d_set_option -- no entry
 * point reads the environment, so two contexts of one process can run different settings.  Keys: "lanes" (window lanes of the
 * graph form, 1..8, default 2), "fused" (0: lfbm5d_denoise_* runs the two calls), "step_sharding" ("rows" / "blocks" / 0),
 * "max_windows", "emulate_world", "data_driven_schedule", "host_blocking", "band_mb", "bm3d_lanes", "spatial_bands" / "band_halo"
 * (several ranks, lfbm5d_denoise_*: teams of ranks denoise horizontal bands of every SAI, see the multi-GPU notes below); test hooks that select
 * between implementations of the same arithmetic ("scan_v1", "scan_any", "scan_full_tables", "dct8w_v2", "group_generic",
 * "no_sa_kernels", "no_slab_kernel", "wide_nosplit", "agg_64bit", "agg_scalar_scan", "subset_list_host", "subset_scan_v1", "filt_group_major",
 * "force_redo"); "scan_lds_cap" is accepted and has no effect (it belonged to a timing experiment).  The old variable names ("LFBM5D_LANES" ...) are accepted as keys.  Values are spelled as the
 * environment spelled them (integers; "rows" / "blocks"; flags: anything but "0" is on); value NULL or "" restores the default.
 * Unknown key: returns 1.  lfbm5d_get_option writes the current value as text (size: bytes of `value`). */
int lfbm5d_set_option(lfbm5d_ctx* ctx, const char* key, const char* value);
int lfbm5d_get_option(lfbm5d_ctx* ctx, const char* key, char* value, unsigned long long size);

/* ---- multi-GPU: one process per GPU, every rank holds the whole (read-only) light field.
 * Whole steps (lfbm5d_step*) and the two-step job (lfbm5d_denoise_*): the windows of the reference's schedule
 * (bm5d.cpp:165-407; a pure function of the SAI mask, see lfbm5d_plan_windows) form a dependency graph -- a window has to
 * wait exactly for the previous window of its step that touched each of its SAIs, because windows interact only through
 * num / den of shared SAIs (the running estimate block matching reads, the sums aggregation adds to); in the two-step job a
 * window of the second step also waits for the last first-step window on each of its SAIs, behind which that SAI's basic
 * estimate is final.  Every window has an owner rank, chosen along a simulated execution (a window follows the rank of the
 * windows of its row of SAIs while that rank is free; lfbm5d_plan_graph / lfbm5d_plan_job return the assignment -- a pure
 * function of the mask, the steps and the rank count); what a window needs from a window of another rank travels as one
 * RCCL send / recv per SAI (num and den of that SAI, or its basic estimate; xGMI point-to-point); at the end every SAI's
 * outputs are formed on the rank that holds them and broadcast.  Every window sees exactly the sums the single-GPU order shows
 * it: the result is BIT-IDENTICAL to one GPU for any rank count (lfbm5d_plan_job exposes owners, issue order and the
 * message list).  The reference's backward raster leaves a wavefront -- a row of windows may run two windows behind the row
 * before it -- so the speed-up is bounded by the graph's critical path: 22 of 64 window slots for ONE step of a 17x17 light
 * field (2.9x however many ranks), 27 of 128 window times for the two-step job (4.75x at eight ranks): use lfbm5d_denoise_*.
 * Environment LFBM5D_STEP_SHARDING selects the alternatives: "rows" = single-GPU window order with every core pass
 * row-sharded as below (exact, two all-reduces per pass; also what greyscale light fields need); "blocks" = round 1's
 * contiguous blocks of windows per rank + ONE all-reduce per step, which scales with the rank count but is NOT the
 * reference's result (a rank's block matching only sees its own earlier windows: -0.01 / -0.03 / -0.07 dB at 2 / 4 / 8 ranks).
 * Option "spatial_bands" = S > 1 (lfbm5d_denoise_* only; "0" = S from lfbm5d_auto_bands) adds a level above the graph for rank counts beyond what the graph keeps
 * busy: S teams of world / S ranks (rank = band * team size + team rank), team b runs the whole two-step job on rows
 * [b H / S, (b + 1) H / S) of every SAI plus "band_halo" rows on either side (default nSim + nDisp + k of the wider step) as a
 * light field of its own -- the same window graph, on a communicator split off for the team -- and ONE all-gather stitches the
 * three light fields.  NOT bit-identical to one GPU (a band's distance tables start their float recurrences at its first row, near
 * ties fall differently); PSNR within 1e-3 dB on 512 x 512 SAIs, a tenth of the +-0.01 dB the reference's own tile mode is held to.
 * Single core passes (lfbm5d_pass_device): the reference patches are sharded by rows over the ranks and
 * the window's num/den all-reduced.
 * Replaces the reference's only parallelism, the OpenMP tile loop + undivide_LF merge
 * (bm5d.cpp:411-708, utilities_LF.cpp:438-515), without its tile-border quality loss. ---- */
#define LFBM5D_UNIQUE_ID_BYTES 128
int lfbm5d_comm_unique_id(void* id_out /* LFBM5D_UNIQUE_ID_BYTES */);
/* (whole steps / jobs on several ranks run window lanes and two exchange streams at once: set GPU_MAX_HW_QUEUES >= 8 in the
 * environment BEFORE the HIP runtime initialises -- ROCm maps streams onto 4 hardware queues by default, and a send that
 * waits for its peer must not sit in front of a compute stream on the same queue; bench.py does it for itself) */
int lfbm5d_comm_init(lfbm5d_ctx* ctx, const void* id, int rank, int world);
/* TESTS ONLY -- the exchange of the window graph between PROCESSES THAT SHARE ONE GPU.  RCCL refuses several ranks on one device, so
 * the multi-rank form could never run between real processes on a one-GPU box; this second transport plays every message of the
 * graph with the same issue order, event gating, channels and abort path as the RCCL form (lfbm5d_api.hip, run_graph), only the
 * bytes move differently: the receiver's exchange stream waits for a word the sender publishes behind its window (device memory
 * both processes map through hipIpcMemHandle), copies the SAI out of the sender's buffers and publishes "taken".  Rendezvous
 * (handles, the completion vote, the closing barriers) goes through small files in `rendezvous_dir`, which must be empty and
 * visible to all ranks.  A peer that dies ends the job with return value 1 after `timeout_s` (<= 0: 30 s), never with a hung GPU.
 * After this call lfbm5d_step*_device / lfbm5d_denoise_device run as rank `rank` of `world`; results are bit-identical to one rank. */
int lfbm5d_comm_init_ipc(lfbm5d_ctx* ctx, int rank, int world, const char* rendezvous_dir, double timeout_s);
/* Diagnostics: all-reduce n floats on the context's stream through the context's communicator (or a
 * one-rank communicator created for the call) and verify the sums.  Returns 0 when RCCL works here. */
int lfbm5d_comm_selftest(lfbm5d_ctx* ctx, unsigned n);
/* Ranks of the context's RCCL communicator as RCCL itself counts them (ncclCommCount): 0 without a communicator, -1 on
 * error.  bench.py prints it so that a multi-GPU record shows the ranks that took part. */
int lfbm5d_comm_ranks(const lfbm5d_ctx* ctx);
/* Shard without a communicator (tests): this rank only processes its rows; no reduction. */
int lfbm5d_set_shard(lfbm5d_ctx* ctx, int rank, int world);
/* The reference's OpenMP tile mode for whole steps (bm5d.cpp:411-708, run_bm5d_* with nb_threads > 1): every window pass
 * runs tile by tile (sub_divide, utilities.cpp:312-395) and keeps the tiles' interiors only (undivide_LF,
 * utilities_LF.cpp:438-515).  nb_tiles is floored to a power of two like main.cpp:101-102 does with nbThreads; 0 / 1 =
 * off (the default: the untiled result, which is what nb_threads == 1 gives and about 0.5 dB better).  A compatibility
 * mode for reproducing a tiled reference run; one GPU, one window after the other.  Returns 0. */
int lfbm5d_set_tiles(lfbm5d_ctx* ctx, int nb_tiles);
/* Row range [begin,end) of n_rows reference-patch rows owned by `rank` of `world`. */
void lfbm5d_shard_rows(unsigned n_rows, int rank, int world, unsigned* begin, unsigned* end);
/* Spatial bands S for a two-step job on `world` ranks (option "spatial_bands"; host only): the window graph of an a x a light field
 * (a = the smaller angular side) keeps about 0.8 ceil(a / 3) ranks busy, so the graph takes the largest power of two of ranks within
 * that and bands take the rest -- while S divides `world` and a band (height / S rows) stays twice as tall as `halo` (0: 40, the
 * README parameters' nSim + nDisp + k).  1 = the graph alone.  Option value "0" applies this rule inside lfbm5d_denoise_*. */
int lfbm5d_auto_bands(unsigned awidth, unsigned aheight, unsigned height, unsigned halo, int world);
/* The window schedule of a step as the processed SAI (index in `ang_major` order) of each window, in
 * order: the centre SAI first, then always the last SAI not covered yet (bm5d.cpp:187-213 -- all
 * candidates tie on the zero-weight count because a window always finishes all of its SAIs).  Host
 * only, needs no GPU.  Returns the number of windows (-1 on bad arguments); writes min(n, cap) entries. */
int lfbm5d_plan_windows(unsigned awidth, unsigned aheight, unsigned an, unsigned ang_major, const unsigned* mask,
                        unsigned* out_sai, unsigned cap);
/* The graph form of a step for `world` ranks with `lanes` lanes each (host only, needs no GPU): owner rank, lane and
 * unit-time start slot of every window of lfbm5d_plan_windows' sequence in the simulated execution whose start order
 * (ties: the earlier window) is the ISSUE ORDER every rank enqueues in.  Returns the number of windows (-1 on bad
 * arguments); writes min(n, cap) entries to each non-NULL array. */
int lfbm5d_plan_graph(unsigned awidth, unsigned aheight, unsigned an, unsigned ang_major, const unsigned* mask, int world, int lanes,
                      unsigned* out_rank, unsigned* out_lane, unsigned* out_start, unsigned cap);
/* The messages of that graph in the order every rank issues them (by the producer's place in the issue order, then SAI
 * slot): out[4 i] = {producer window, consumer window, SAI, channel}; the producer's rank sends num and den of the SAI to the
 * consumer's rank once the producer window is done.
 * Returns the number of messages (-1 on bad arguments); writes min(n, cap) quadruples. */
int lfbm5d_plan_messages(unsigned awidth, unsigned aheight, unsigned an, unsigned ang_major, const unsigned* mask, int world,
                         unsigned* out, unsigned cap);
/* The graph of a JOB -- one step (n_steps = 1) or run_bm5d_1st_step + run_bm5d_2nd_step back to back (n_steps = 2, what
 * lfbm5d_denoise_* executes) -- for `world` graph ranks with `lanes` lanes each (host only, needs no GPU).  an[n_steps] =
 * half size of every step's angular search window; cost[n_steps] = relative cost of a window pass of every step in the
 * scheduling model (NULL: 10 / 9 for two steps, 1 for one).  In a two-step job a window of the second step waits, per SAI, for
 * the LAST window of the first step touching that SAI (the SAI's basic estimate is final then), so the second step's wavefront
 * follows the first's: 128 windows with a critical path of about 28 on a 17x17 light field instead of 2 x 22.
 *   out_nodes  8 unsigned per window, step 0's windows in plan order, then step 1's:
 *              {step slot, index in the step's sequence, processed SAI, graph rank, lane, start time (cost units) of the simulated
 *               execution, position in the ISSUE ORDER every rank walks, chain}
 *   out_msgs   6 unsigned per message, in issue order: {kind, producer node, consumer node (kind 0) or 0xffffffff, receiving graph
 *              rank, SAI, channel}; kind 0 = num and den of the SAI from the producer's rank to its next toucher's, kind 1 = the
 *              basic estimate of the SAI, finalised behind the producer node, to a rank whose second-step windows read it
 *   out_counts {windows, messages, makespan of the simulated execution in cost units, 1 if every window centre is non-empty}
 * Returns the number of windows (-1 on bad arguments); writes min(n, cap) entries to each non-NULL array. */
int lfbm5d_plan_job(unsigned awidth, unsigned aheight, unsigned ang_major, const unsigned* mask, int n_steps, const unsigned* an,
                    const unsigned* cost, int world, int lanes, unsigned* out_nodes, unsigned node_cap, unsigned* out_msgs,
                    unsigned msg_cap, unsigned* out_counts);
/* The windows the last lfbm5d_step* / lfbm5d_denoise_* call on this context actually ran (same encoding; a two-step job: the
 * first step's windows, then the second's). */
int lfbm5d_last_windows(const lfbm5d_ctx* ctx, unsigned* out_sai, unsigned cap);

/* ---- outer seam, device-resident: LF buffers already in HBM ----
 * lfbm5d_step1_device == run_bm5d_1st_step (bm5d.h:11-35, nb_threads == 1 semantics):
 *   d_noisy  [asize][C*H*W]  in/out: colour-transformed at entry and back at exit, exactly like the
 *                            reference mutates LF_noisy (bm5d.cpp:133, :713)
 *   h_mask   [asize] host    LF_SAI_mask (0 = empty SAI)
 *   d_basic  [asize][C*H*W]  out: basic estimate (RGB)
 * lfbm5d_step2_device == run_bm5d_2nd_step (bm5d.h:38-62): d_basic is in/out (bm5d.cpp:829,:1416),
 *   d_denoised is the output. */
int lfbm5d_step1_device(lfbm5d_ctx* ctx, const lfbm5d_params* P, float* d_noisy,
                        const unsigned* h_mask, float* d_basic, unsigned ang_major,
                        unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H,
                        unsigned C);
int lfbm5d_step2_device(lfbm5d_ctx* ctx, const lfbm5d_params* P, float* d_noisy,
                        const unsigned* h_mask, float* d_basic, float* d_denoised,
                        unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                        unsigned W, unsigned H, unsigned C);

/* Both steps as ONE job == run_bm5d_1st_step followed by run_bm5d_2nd_step (main.cpp:195, :242), bit-identical to
 * lfbm5d_step1_device + lfbm5d_step2_device: the windows of both steps form one dependency graph (lfbm5d_plan_job) and what the
 * reference does between the two calls (final estimate, inverse and forward colour transform: bm5d.cpp:405, :711-714, :827-830)
 * happens SAI by SAI as soon as a SAI's basic estimate is final.  On one GPU that closes the gap between the steps; on several
 * it is what lets all ranks work (the second step's wavefront follows the first's).  P1 / an1 = the hard-thresholding step's
 * parameters, P2 / an2 = the Wiener step's.  d_noisy in/out, d_basic and d_denoised out, exactly as the two calls leave them.
 * Light fields outside the graph form (greyscale, an empty SAI at a window centre, tile mode, LFBM5D_STEP_SHARDING,
 * LFBM5D_DATA_DRIVEN_SCHEDULE, LFBM5D_FUSED=0) run the two calls one after the other. */
int lfbm5d_denoise_device(lfbm5d_ctx* ctx, const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy,
                          const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned ang_major,
                          unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C);

/* ---- outer seam, host buffers (what the run_bm5d_* wrappers of the drop-in call): same
 * semantics, the library stages through HBM (PCIe-inclusive).
 * ERRORS: the host forms write their in / out buffers (h_noisy, h_basic, h_denoised) while the job runs -- the streamed form
 * delivers a SAI's outputs as soon as the last window on it has run.  After a NON-ZERO return the contents of every in / out
 * buffer of the call are UNDEFINED (partly inputs, partly colour-round-tripped outputs): a caller that wants to retry keeps its
 * own copy of the inputs.  (The reference has the same contract: run_bm5d_* transform LF_noisy in place before anything can
 * fail, bm5d.cpp:133.) ---- */
int lfbm5d_step1_host(lfbm5d_ctx* ctx, const lfbm5d_params* P, float* h_noisy,
                      const unsigned* h_mask, float* h_basic, unsigned ang_major, unsigned awidth,
                      unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C);
int lfbm5d_step2_host(lfbm5d_ctx* ctx, const lfbm5d_params* P, float* h_noisy,
                      const unsigned* h_mask, float* h_basic, float* h_denoised,
                      unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                      unsigned W, unsigned H, unsigned C);

int lfbm5d_denoise_host(lfbm5d_ctx* ctx, const lfbm5d_params* P1, const lfbm5d_params* P2, float* h_noisy,
                        const unsigned* h_mask, float* h_basic, float* h_denoised, unsigned ang_major,
                        unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C);

/* The same with the caller's light fields as ONE HOST POINTER PER SAI -- h_x[st] = &LF_x[st][0], C*H*W floats each, exactly the
 * reference's vector<vector<float>> (src/bm5d.h:11-62) without a flat copy; entries of empty SAIs are ignored (may be NULL).
 * The flat forms above are these with pointers into one buffer.  On one rank with the window graph (colour light fields) the
 * SAIs are STREAMED: a SAI goes up when the first window that needs it is enqueued (forward colour transform behind the copy),
 * its outputs come down as soon as the last window on it has run, while the other windows compute -- the interval the reference
 * times (main.cpp:189-201, :241-247) then costs a few per cent more than device-resident buffers instead of the 20 % four
 * blocking copies of the light field cost.  Pageable memory is fine.  Everything else about the call (in / out arguments, result
 * bit-identical to the device form) is unchanged; LFBM5D_HOST_BLOCKING=1 selects the upload-all / download-all form. */
int lfbm5d_step1_host_sai(lfbm5d_ctx* ctx, const lfbm5d_params* P, float* const* h_noisy, const unsigned* h_mask,
                          float* const* h_basic, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                          unsigned W, unsigned H, unsigned C);
int lfbm5d_step2_host_sai(lfbm5d_ctx* ctx, const lfbm5d_params* P, float* const* h_noisy, const unsigned* h_mask,
                          float* const* h_basic, float* const* h_denoised, unsigned ang_major, unsigned awidth,
                          unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C);
int lfbm5d_denoise_host_sai(lfbm5d_ctx* ctx, const lfbm5d_params* P1, const lfbm5d_params* P2, float* const* h_noisy,
                            const unsigned* h_mask, float* const* h_basic, float* const* h_denoised, unsigned ang_major,
                            unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C);

/* ---- inner seam: one core pass on a mirror-padded angular window, device pointers ----
 * == bm5d_1st_step (step = 1) / bm5d_2nd_step (step = 2) (bm5d_core_processing.h:6-80).
 * Buffers are [A][C*Wb*Hb], A = aw*ah; d_basic may be NULL for step 1; d_num / d_den are
 * accumulated into.  h_mask / h_procSAI are host arrays of A entries (LF_SAI_mask, procSAI). */
int lfbm5d_pass_device(lfbm5d_ctx* ctx, int step, const lfbm5d_params* P, unsigned aw,
                       unsigned ah, unsigned Wb, unsigned Hb, unsigned C, const float* d_noisy,
                       const float* d_basic, float* d_num, float* d_den, const unsigned* h_mask,
                       const unsigned* h_procSAI, unsigned cst, unsigned pst);

/* ---- per-SAI BM3D: the reference's comparison tool LFBM3Ddenoising, on the same kernels ----
 * One step's parameters of run_bm3d (src/bm3d.h:11-34). */
typedef struct {
    float    sigma;        /* sigma                                   */
    float    lambda3D;     /* lambdaHard3D (ignored by step 2)        */
    unsigned N;            /* NHard / NWien: power of two, 2..32      */
    unsigned nHW;          /* nHard / nWien: half search window       */
    unsigned k;            /* kHard / kWien                           */
    unsigned p;            /* pHard / pWien                           */
    unsigned useSD;        /* useSD_h / useSD_w                       */
    unsigned tau_2D;       /* LFBM5D_DCT | LFBM5D_BIOR                */
    unsigned color_space;  /* LFBM5D_YUV | _YCBCR | _OPP | _RGB       */
} lfbm5d_bm3d_params;
/* == bm3d_1st_step (step = 1, src/bm3d.h:37-55) / bm3d_2nd_step (step = 2, src/bm3d.h:58-76) on a mirror-padded,
 * colour-transformed image [C][Hb][Wb] in HBM; d_basic may be NULL for step 1.  d_out [C][Hb][Wb] receives
 * numerator / denominator (pixels no patch reached keep the step's input image). */
int lfbm5d_bm3d_step_device(lfbm5d_ctx* ctx, int step, const lfbm5d_bm3d_params* P, unsigned Wb, unsigned Hb,
                            unsigned C, const float* d_noisy, const float* d_basic, float* d_out);
/* == run_bm3d_LF (src/bm3d_LF.h:10-35; run_bm3d src/bm3d.h:11-34 with nb_threads == 1 for every SAI of the mask).
 * Buffers [asize][C*H*W]; d_noisy is colour-transformed at entry and back at exit like the reference mutates
 * LF_noisy (bm3d.cpp:115, :290); d_basic and d_denoised are outputs (RGB).  nHard != nWien reproduces the reference's
 * crop of the second step at offset nWien of the nHard-padded image (bm3d.cpp:181-189: a shifted picture); nWien <= nHard
 * (beyond that the reference itself returns 0 / 0 in the border). */
int lfbm5d_bm3d_lf_device(lfbm5d_ctx* ctx, const lfbm5d_bm3d_params* hard, const lfbm5d_bm3d_params* wien,
                          float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised,
                          unsigned asize, unsigned W, unsigned H, unsigned C);
int lfbm5d_bm3d_lf_host(lfbm5d_ctx* ctx, const lfbm5d_bm3d_params* hard, const lfbm5d_bm3d_params* wien,
                        float* h_noisy, const unsigned* h_mask, float* h_basic, float* h_denoised,
                        unsigned asize, unsigned W, unsigned H, unsigned C);

/* ---- blind noise level: the `sigma` every entry point above needs, estimated from the noisy light field itself ----
 * Not in the reference, whose README asks the caller of `LFSourceDir = none` for "an estimated value of the noise level" without
 * providing one (its estimate_sigma, utilities.cpp:633, only scales a given sigma per channel of the colour space).  The PCA statistic
 * of Chen, Zhu & Heng (ICCV 2015) pooled over the SAIs: for every non-empty SAI a and channel c (as stored: no colour transform) the
 * n_ac = (H-r+1)(W-r+1) overlapping r x r patches at stride 1, as vectors x of d = r*r values in row-major order, give s_ac = sum x,
 * S_ac = sum x x^T and M_ac = S_ac - s_ac s_ac^T / n_ac; Cov = sum M_ac / sum n_ac over (a, c) for the light field, over a for a
 * channel, over c for a SAI.  With the eigenvalues of Cov ascending, lambda_1 <= ... <= lambda_d, the statistic takes the first
 * m = d, d-1, ..., 1 at which as many of lambda_1..m lie above their mean mu_m as below it, and returns sqrt(max(mu_m, 0)) and m
 * (the size of the noise subspace found).  Units: grey levels of the channels as stored, i.e. lfbm5d_params.sigma.
 * The statistic assumes additive white Gaussian noise: under signal-dependent (Poisson-Gaussian) noise it returns roughly the level of
 * the darkest regions (lfbm5d_pg_* below model that case), spatially correlated noise (e.g. demosaicked raw data) is outside it, and
 * values clipped to 0..255 (8-bit files) bias it low at large sigma.
 * The patch sums run on the GPU in double, every sum in a fixed order: repeated calls, and the device and host forms, return the
 * same bits; only the pooled d x d matrices leave the device; the eigenvalues are found on the host (double).  One GPU. */
typedef struct {
    double   sigma;             /* all non-empty SAIs and channels pooled: the value to pass as lfbm5d_params.sigma */
    double   sigma_channel[3];  /* per stored channel, all SAIs pooled (grey: [0] only, rest 0)                      */
    unsigned components;        /* m of the light-field estimate                                                    */
    unsigned patch;             /* r used                                                                           */
    unsigned long long patches; /* sum of n_ac                                                                      */
} lfbm5d_noise_level;
/* d_lf [asize][C*H*W] in HBM, read only; h_mask [asize] (0 = empty SAI); C = 1 or 3; patch r = 4..8 (0 = 8); W, H >= 2 r.
 * h_sigma_sai [asize] or NULL: the estimate of every SAI on its own (0 for empty SAIs); h_eigen [r*r] or NULL: the eigenvalues of the
 * light field's covariance, ascending.  Returns 1 with a message on a rejected input (C, patch, W / H, a mask without a non-empty
 * SAI, a NULL buffer that is required). */
int lfbm5d_noise_level_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                              unsigned C, unsigned patch, lfbm5d_noise_level* out, double* h_sigma_sai, double* h_eigen);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM: bit-identical results. */
int lfbm5d_noise_level_host_sai(lfbm5d_ctx* ctx, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W,
                                unsigned H, unsigned C, unsigned patch, lfbm5d_noise_level* out, double* h_sigma_sai, double* h_eigen);
/* Host only, needs no GPU: the statistic above on one covariance, cov row-major d x d symmetric, 1 <= d <= 64; h_eigen [d] or NULL
 * receives the eigenvalues ascending.  Returns 1 on bad arguments (no message: there is no context). */
int lfbm5d_noise_level_statistic(unsigned d, const double* cov, double* sigma, unsigned* components, double* h_eigen);

/* ---- light-field super-resolution: the scheme of SR-LFBM5D (Alain & Smolic, ICIP 2018; the reference's README points to its "SR
 * branch") with the operators below -- NOT that branch's output, whose blur models and stopping rule are not reproduced.  Iterative
 * back-projection regularised by the hard-thresholding step: with y the low-resolution light field (w x h per SAI), s = scale and
 * W = s w, H = s h,
 *   x_0 = U y;   for k = 1..K:  z = x_{k-1} + beta U (y - D x_{k-1}),  x_k = basic estimate of lfbm5d_step1_device on z with
 *   P.sigma = sigma_k = sigma_start (sigma_end / sigma_start)^((k-1)/(K-1)) (double; K = 1: sigma_start);
 *   close_projection != 0:  out = x_K + beta U (y - D x_K), else out = x_K.
 * The step runs exactly as lfbm5d_step1_device runs it (colour space, window graph, lanes, every option).  One GPU.
 * Operators: separable; a 1-D operator from n_in to n_out samples is a tap table first[n_out] (signed), w[n_out][T], built in double
 * and rounded to float:  out[X] = sum_{t<T} w[X][t] in[clamp(first[X]+t, 0, n_in-1)], t ascending, float32 (clamped at read time,
 * weights not merged); 2-D: rows' table * plane * columns' table^T, horizontal pass first.  keys = the Keys cubic with a = -0.5.
 *   U  (LFBM5D_SR_UP, n_out = s n_in): u = (X+0.5)/s - 0.5, first = floor(u) - 1, T = 4, w_t = keys(u - (first+t)).
 *   D  (LFBM5D_SR_DOWN, n_out = n_in / s, n_in a multiple of s): u = (x+0.5) s - 0.5;
 *      LFBM5D_SR_BICUBIC  (antialiased): taps j in [ceil(u-2s), floor(u+2s)], w_j = keys((u-j)/s);
 *      LFBM5D_SR_GAUSSIAN (blur_sigma in (0, 5]): R = ceil(3 blur_sigma), taps j in [ceil(u-R), floor(u+R)], w_j = exp(-(u-j)^2 / (2 blur_sigma^2));
 *      both normalised to sum 1 in double; T = the largest tap count (<= 32), shorter rows padded with zero weights.
 * No atomics, fixed summation order: repeated calls return the same bits.  Planes of empty SAIs are neither read nor written. */
#define LFBM5D_SR_BICUBIC  0
#define LFBM5D_SR_GAUSSIAN 1
#define LFBM5D_SR_UP       0
#define LFBM5D_SR_DOWN     1
typedef struct {
    unsigned scale;             /* 2, 3 or 4                                                         */
    unsigned kernel;            /* of D: LFBM5D_SR_BICUBIC | LFBM5D_SR_GAUSSIAN                      */
    float    blur_sigma;        /* of the Gaussian D, in high-resolution pixels (bicubic: ignored)   */
    unsigned iterations;        /* K >= 1                                                            */
    float    sigma_start;       /* sigma_1 > 0                                                       */
    float    sigma_end;         /* sigma_K, 0 < sigma_end <= sigma_start                             */
    float    beta;              /* back-projection step, (0, 2]                                      */
    unsigned close_projection;  /* != 0: one more back-projection behind the last filtered iterate   */
} lfbm5d_sr_params;
/* Host only: K = 12, sigma_start = 15 s, sigma_end = 2 s, beta = 1, bicubic D (blur_sigma = 0.4 s for callers that switch to the Gaussian),
 * closing projection on -- the best of a sweep on ONE light field (profiles/sr_defaults.txt), not optimal beyond it.  Returns 1 on a
 * scale outside 2..4. */
int lfbm5d_sr_defaults(unsigned scale, lfbm5d_sr_params* out);
/* Host only, needs no GPU: the tap table of one 1-D operator for n_in input samples.  *T receives the taps per output sample; first
 * [n_out] and w [n_out * T] are filled when both are given and `cap` (floats w can hold) >= n_out * T; both NULL = query T.  Returns
 * 1 (no message: there is no context) on rejected parameters (scale, kernel, blur_sigma), n_in = 0, n_in no multiple of s for D, or a
 * table that does not fit. */
int lfbm5d_sr_taps(unsigned op, const lfbm5d_sr_params* sr, unsigned n_in, int* first, float* w, unsigned* T, unsigned cap);
/* Device buffers: d_low [asize][C*h*w], d_high [asize][C*H*W]; h_mask [asize] host (0 = empty SAI); C = 1 or 3; w, h = the LOW-resolution
 * size.  up: d_high = U d_low.  down: d_low = D d_high.  backproject: d_high_z = d_high_x + beta U (d_low_y - D d_high_x) in exactly two
 * launches (d_high_z may be d_high_x).  Rejected inputs (see lfbm5d_sr_params; a NULL buffer; a mask without a non-empty SAI) return 1
 * with a message. */
int lfbm5d_sr_up_device(lfbm5d_ctx* ctx, const lfbm5d_sr_params* sr, const float* d_low, const unsigned* h_mask, float* d_high,
                        unsigned asize, unsigned w, unsigned h, unsigned C);
int lfbm5d_sr_down_device(lfbm5d_ctx* ctx, const lfbm5d_sr_params* sr, const float* d_high, const unsigned* h_mask, float* d_low,
                          unsigned asize, unsigned w, unsigned h, unsigned C);
int lfbm5d_sr_backproject_device(lfbm5d_ctx* ctx, const lfbm5d_sr_params* sr, const float* d_low_y, const float* d_high_x,
                                 const unsigned* h_mask, float* d_high_z, unsigned asize, unsigned w, unsigned h, unsigned C);
/* The loop above.  P = the hard-thresholding parameters (P->sigma is ignored), an = half size of its angular search window; d_low is only
 * read, d_high receives the result.  Scratch (one high- and one low-resolution light field) belongs to the context and is reused.
 * Contexts with a communicator return 1. */
int lfbm5d_superres_device(lfbm5d_ctx* ctx, const lfbm5d_sr_params* sr, const lfbm5d_params* P, const float* d_low, const unsigned* h_mask,
                           float* d_high, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned w, unsigned h,
                           unsigned C);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form. */
int lfbm5d_superres_host_sai(lfbm5d_ctx* ctx, const lfbm5d_sr_params* sr, const lfbm5d_params* P, const float* const* h_low,
                             const unsigned* h_mask, float* const* h_high, unsigned ang_major, unsigned awidth, unsigned aheight,
                             unsigned an, unsigned w, unsigned h, unsigned C);

/* ---- quality of a light field against a reference: per-SAI PSNR, RMSE and SSIM, with the light fields resident in HBM ----
 * ref and test are [asize][C*H*W] float32; channels are compared as stored (no colour transform); peak > 0 is the value range
 * (0 = 255).  For every non-empty SAI, in double:
 *   mse  = mean over all C*H*W values of (ref - test)^2;  rmse = sqrt(mse);  psnr = 10 log10(peak^2 / mse) (+inf when mse == 0)
 *          -- the reference's compute_psnr / compute_psnr_LF (utilities_LF.cpp:639-692), which accumulate in float;
 *   ssim = Wang, Bovik, Sheikh & Simoncelli (2004): window w = g g^T, 11 x 11, g_i = exp(-(i-5)^2 / (2 1.5^2)) normalised to sum 1;
 *          per channel plane every valid window position, (H-10) x (W-10) of them, no padding; with mu_a = sum w a, mu_b,
 *          s_a = sum w a^2 - mu_a^2, s_b, s_ab = sum w a b - mu_a mu_b, C1 = (0.01 peak)^2, C2 = (0.03 peak)^2 the map is
 *          (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_a + s_b + C2)); the SAI's SSIM is the mean of the map over
 *          channels and positions.  Needs W, H >= 11.
 * The summary follows compute_psnr_LF: mean and population standard deviation (divide by the count) of psnr, rmse and ssim over
 * the non-empty SAIs, the pooled mse over all values of all non-empty SAIs, and the count.  Non-finite entries follow IEEE
 * arithmetic and are not special-cased: ONE SAI with mse == 0 makes psnr_mean +inf (and psnr_std NaN).  Entries of empty SAIs in
 * the per-SAI arrays are 0.
 * Every sum runs on the GPU in double and in a fixed order (no atomics): repeated calls, the device and host forms, and want_ssim
 * on / off (for mse) return the same bits; only two doubles per SAI leave the device.  The inputs are only read; planes of empty
 * SAIs are neither read nor written.  One GPU; works on any context. */
typedef struct {
    double   psnr_mean, psnr_std;   /* over the non-empty SAIs                                  */
    double   rmse_mean, rmse_std;
    double   ssim_mean, ssim_std;   /* 0 when SSIM was not asked for                            */
    double   mse;                   /* pooled over all values of all non-empty SAIs             */
    unsigned count;                 /* non-empty SAIs                                           */
    unsigned has_ssim;              /* != 0: ssim_mean / ssim_std are filled                    */
} lfbm5d_quality;
/* d_ref, d_test [asize][C*H*W] in HBM, read only; h_mask [asize] (0 = empty SAI); C = 1 or 3; want_ssim != 0: SSIM too, in the same
 * pass over the light fields.  h_mse_sai / h_ssim_sai [asize] or NULL: the per-SAI values (psnr and rmse follow from mse as above;
 * h_ssim_sai is zero-filled without want_ssim).  Returns 1 with a message on a rejected input: a NULL required buffer, C not 1 or
 * 3, a mask without a non-empty SAI, peak < 0 or not finite, W or H below 11 with want_ssim (or 0 at all). */
int lfbm5d_quality_device(lfbm5d_ctx* ctx, const float* d_ref, const float* d_test, const unsigned* h_mask, unsigned asize, unsigned W,
                          unsigned H, unsigned C, double peak, int want_ssim, lfbm5d_quality* out, double* h_mse_sai, double* h_ssim_sai);
/* The same on host light fields, one pointer per SAI for each (NULL allowed for empty SAIs, rejected for non-empty ones), staged
 * through HBM: bit-identical results. */
int lfbm5d_quality_host_sai(lfbm5d_ctx* ctx, const float* const* h_ref, const float* const* h_test, const unsigned* h_mask, unsigned asize,
                            unsigned W, unsigned H, unsigned C, double peak, int want_ssim, lfbm5d_quality* out, double* h_mse_sai,
                            double* h_ssim_sai);
/* Host only, needs no GPU: the summary above from per-SAI mse [asize] and ssim [asize] (or NULL: no SSIM); entries of empty SAIs are
 * ignored.  The device forms call it.  Returns 1 on bad arguments (NULL mse / mask / out, no non-empty SAI, peak < 0 or not finite;
 * no message: there is no context). */
int lfbm5d_quality_summary(const double* h_mse_sai, const double* h_ssim_sai, const unsigned* h_mask, unsigned asize, double peak,
                           lfbm5d_quality* out);

/* ---- signal-dependent noise: Poisson-Gaussian model var(z | y) = a y + b, its estimate, and denoising through a variance-stabilising
 * transform ----
 * Not in the reference.  Every entry point above assumes additive white Gaussian noise of one sigma; the noise of a real capture
 * (lenslet cameras, low light: the LFSourceDir = none case) grows with the intensity.  The remedy here leaves the filter alone:
 * estimate (a, b), apply the generalised Anscombe transform (the noise becomes white Gaussian of a known sigma s), run the two-step job,
 * return through the exact unbiased inverse (Makitalo & Foi, IEEE TIP 2013, closed-form approximation).  Light fields are [asize][C*H*W]
 * float32, nominally 0..255, channels as stored (no colour transform); planes of empty SAIs are neither read nor written.  One GPU:
 * contexts with a communicator or a shard return 1.
 * Limits: the level bins and the scale s assume the 0..255 range; values clipped to 0..255 (8-bit files) lose part of their noise
 * near black and white, which biases the dark and bright levels of the estimate; spatially correlated noise is outside the model.  At
 * a <~ 1 (on the 0..255 scale) the path does not beat lfbm5d_denoise_* with a well-chosen single sigma (about 0.1-0.2 dB below the
 * best one); the gain is at strong dependence, a >~ 4 (DESIGN.md 3f has the figures).
 *
 * Statistics (GPU, integers: independent of any summation order, equal to the model of tests/pg_model.py bit for bit).  L = 64 levels,
 * E_MIN = -12, E_MAX = 8, Q = (E_MAX - E_MIN) 16 + 2 = 322 keys.  A block exists for every non-empty SAI, every channel plane I and every
 * i < floor(H/2), j < floor(W/2) (odd W / H leave the last column / row unused): p00 = I[2i][2j], p01 = I[2i][2j+1], p10 = I[2i+1][2j],
 * p11 = I[2i+1][2j+1]; in float32, in exactly this order,
 *   m = ((p00 + p01) + (p10 + p11)) * 0.25f,    d = ((p00 - p01) - (p10 - p11)) * 0.5f
 * (var d = the mean of the four pixels' noise variances = a mean(y) + b, plus a signal term the quantile below is robust to).  A block
 * with non-finite m or d is skipped and counted.  mc = min(max(m, 0), 255); lev = min(63, (int)(mc * (float)(64.0/255.0)));
 * key = clamp((bits(|d|) >> 19) - ((E_MIN + 127) << 4) + 1, 0, Q - 1): 16 bins per octave from the exponent and the top four mantissa
 * bits; key 0 is [0, 2^-12), the lower edge e[k] of key k >= 1 is the float whose bits are (k - 1 + 1840) << 19, key 321 collects
 * everything >= 2^8.  hist[c][lev][key] += 1, sum[c][lev] += (uint64) rint(mc * 256.0f).
 * Fit (host, double) of one histogram h[64][322] with sum[64]: a level with n = sum_k h[l][k] < 256 is skipped; T = 0.25 n, k* = the
 * first k whose cumulative count is >= T (k* = 0 or 321: level skipped); Qv = e[k*] + (e[k*+1] - e[k*]) (T - cum[k*-1]) / h[l][k*];
 * v = (Qv / 0.31863936396437514)^2 (the 0.25 quantile of |N(0,1)|); x = sum[l] / (256 n); w = n / v^2.  Weighted least squares
 * v = a x + b over the valid levels in level order; fewer than two valid levels or a determinant <= 1e-12 Sw Swxx: a = 0, b = Swv / Sw;
 * a < 0: a = 0, b = Swv / Sw; otherwise b < 0: b = 0, a = Swxv / Swxx; no valid level: the fit fails.  The light field's model is the
 * fit of the channels' histograms added together, a channel's model the fit of its own histogram.
 * Transform.  A model is a_c >= 0, b_c per stored channel with c_c = 3/8 a_c^2 + b_c > 0 (anything else is rejected); the common scale
 * s = mean over the channels of (sqrt(255 a_c + c_c) + sqrt(c_c)) / 2: after the forward transform every channel has noise standard
 * deviation s and roughly the 0..255 range the filter's parameters are tuned for; a = 0 gives s = sqrt(b) and the identity.  In
 * double, rounded once to float:
 *   forward  w = a z + c (w < 0: w = 0, z = -c / a);  t = s 2z / (sqrt(w) + sqrt(c))      [= s (f(z) - f(0)), f(z) = (2/a) sqrt(a z + c)]
 *   inverse  u = t / s;  q = a u + 2 sqrt(c);  q <= 0 -> 0;  g = a / q;  g > 0.816496580927726 -> 0;  else
 *            y = a u^2 / 4 + u sqrt(c) + a / 4 + a (K1 g - 1.375 g^2 + K3 g^3), K1 = 0.30618621784789724, K3 = 0.7654655446197431;
 *            the output is max(y, 0). */
#define LFBM5D_PG_LEVELS 64
#define LFBM5D_PG_KEYS   322
typedef struct {
    double a[3];   /* per stored channel (grey: [0] only) */
    double b[3];
} lfbm5d_pg_model;
typedef struct {
    double a, b;                         /* the light field's model: every non-empty SAI and channel pooled                   */
    double a_channel[3], b_channel[3];   /* per stored channel (NaN for a channel whose own fit fails; grey: [0] only, rest 0) */
    unsigned long long blocks;           /* 2 x 2 blocks visited                                                              */
    unsigned long long skipped;          /* of those, skipped for a non-finite m or d                                         */
} lfbm5d_pg_estimate;
/* d_lf [asize][C*H*W] in HBM, read only; h_mask [asize] (0 = empty SAI); C = 1 or 3; W, H >= 2.  h_hist [C][64][322], h_sum [C][64]
 * (host) receive the counts; blocks / skipped may be NULL.  Returns 1 with a message on a rejected input (a NULL required buffer, C, W /
 * H, a mask without a non-empty SAI). */
int lfbm5d_pg_histogram_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                               unsigned long long* h_hist, unsigned long long* h_sum, unsigned long long* blocks, unsigned long long* skipped);
/* Host only, needs no GPU: the fit above of one histogram hist [64][322], sum [64].  Returns 1 when no level is valid (or on a NULL
 * pointer; no message: there is no context). */
int lfbm5d_pg_fit(const unsigned long long* hist, const unsigned long long* sum, double* a, double* b);
/* Histogram + fits.  h_hist / h_sum as above or NULL.  Returns 1 with a message when the pooled fit fails (too few blocks). */
int lfbm5d_pg_estimate_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H, unsigned C,
                              lfbm5d_pg_estimate* out, unsigned long long* h_hist, unsigned long long* h_sum);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM: identical results. */
int lfbm5d_pg_estimate_host_sai(lfbm5d_ctx* ctx, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                unsigned C, lfbm5d_pg_estimate* out, unsigned long long* h_hist, unsigned long long* h_sum);
/* Host only, needs no GPU: the common scale s of a model for C = 1 or 3 channels -- the sigma of the transformed light field.  Returns 1
 * on a rejected model (a < 0, 3/8 a^2 + b <= 0, anything not finite) or C. */
int lfbm5d_pg_scale(const lfbm5d_pg_model* model, unsigned C, double* s);
/* d_out = forward / inverse transform of d_in, both [asize][C*H*W] in HBM; d_out may be d_in. */
int lfbm5d_pg_forward_device(lfbm5d_ctx* ctx, const lfbm5d_pg_model* model, const float* d_in, const unsigned* h_mask, float* d_out,
                             unsigned asize, unsigned W, unsigned H, unsigned C);
int lfbm5d_pg_inverse_device(lfbm5d_ctx* ctx, const lfbm5d_pg_model* model, const float* d_in, const unsigned* h_mask, float* d_out,
                             unsigned asize, unsigned W, unsigned H, unsigned C);
/* The job: (1) forward transform of d_noisy -- which is only read -- into a light field of scratch the context owns, (2)
 * lfbm5d_denoise_device on it with P1->sigma = P2->sigma = (float)s (the sigmas passed are ignored; every option and fallback of that
 * call applies), (3) inverse transform in place on d_basic and d_denoised.  Bit-identical to the three calls made by hand.  model NULL:
 * the pooled model (a, b for every channel) is estimated from d_noisy first; `used` (may be NULL) receives the model that was applied. */
int lfbm5d_denoise_pg_device(lfbm5d_ctx* ctx, const lfbm5d_pg_model* model, lfbm5d_pg_model* used, const lfbm5d_params* P1,
                             const lfbm5d_params* P2, const float* d_noisy, const unsigned* h_mask, float* d_basic, float* d_denoised,
                             unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H,
                             unsigned C);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form.  h_noisy is only read. */
int lfbm5d_denoise_pg_host_sai(lfbm5d_ctx* ctx, const lfbm5d_pg_model* model, lfbm5d_pg_model* used, const lfbm5d_params* P1,
                               const lfbm5d_params* P2, const float* const* h_noisy, const unsigned* h_mask, float* const* h_basic,
                               float* const* h_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2,
                               unsigned W, unsigned H, unsigned C);

/* ---- data clipped to a known range: the noise level from the blocks the clipping left alone, and the inverse of the clipped mean ----
 * Not in the reference.  A light field read from 8-bit files has been rounded and clipped to 0..255 (the LFSourceDir = none case).  Near
 * black and white the clipping removes part of the noise, which biases the blind estimates above low, and it moves the mean: a filter
 * estimates E[clip(y + sigma n)], not y -- at y = lo that is sigma phi(0) = 0.4 sigma too bright, and as much too dark at hi.  Both have
 * a pointwise remedy that leaves the filter alone.  Light fields are [asize][C*H*W] float32, channels as stored; planes of empty SAIs are
 * neither read nor written; C = 1 or 3; W, H >= 2.  One GPU: contexts with a communicator or a shard return 1.
 * Range: lo < hi, both finite (and still different, with a finite 255 / (hi - lo), as floats); a value p is censored when p <= lo or
 * p >= hi (compared as floats).
 * Limits: near the bounds the noise's standard deviation is smaller than sigma and the filter is not told (Foi 2009's variance-stabilised
 * form is not built); the inverse's slope reaches 2 at the bounds, so it doubles the residual error there; one sigma for all channels
 * and SAIs; Poisson-Gaussian noise combined with clipping is not covered here (lfbm5d_pgclip.h is the stage for it); one GPU.
 *
 * Statistics (GPU, integers: independent of any order, equal to tests/clip_model.py bit for bit).  s = (float)(255 / (hi - lo)); every
 * pixel becomes p' = (p - (float)lo) * s in float32 (no fused multiply-add; exact at 0..255: p' = p); m, d, the 64 levels and the 322
 * keys of |d| of every 2 x 2 block, hist[c][lev][key] and sum[c][lev] are those of the Poisson-Gaussian statistics above on p'.
 * cens[c][lev] counts the (unskipped) blocks with at least one censored pixel, whole[c] those whose four pixels are whole numbers
 * (p == rint(p)).  At the default range hist and sum equal lfbm5d_pg_histogram_device's.
 * Fit (host, double) of one histogram h[64][322] with cens[64] and whole.  When whole equals the histogram's total the data are quantised:
 * every d is a multiple of delta = s / 2, a count stands for the continuous values within delta / 2 of its d, and the keys' edges fall on
 * multiples of delta -- read as they are, the edges bias the quantile by delta / 2 (0.8 in sigma at 0..255).  So edge e[k], k >= 1, is
 * replaced by ceil(e[k] / delta) delta - delta / 2; otherwise delta = 0 and the edges stay.  A level's n, T, k*, Qv are those of
 * lfbm5d_pg_fit on these edges; v = (Qv / 0.31863936396437514)^2 - delta^2 / 3 (the rounding's own variance); the level is populated when
 * n >= 256, 0 < k* < 321 and v > 0.  A populated level counts under f_max when cens[l] <= f_max n; sigma'^2 = sum w v / sum w over the
 * levels that count, w = n / v^2, in level order (lfbm5d_pg_fit's a = 0 branch); sigma = sigma' / s.  f_max runs down the ladder 0.05,
 * 0.1, 0.2, 0.4, 1 until at least 4 levels count; fewer than 4 populated levels: the fit fails.  heavily_clipped = f_max > 0.1.  The
 * light field's sigma is the fit of the channels' counts added together, a channel's sigma the fit (with its own ladder) of its own.
 * Map.  For sigma > 0, a = (lo - y) / sigma, b = (hi - y) / sigma:
 *   E(y) = lo Phi(a) + hi (1 - Phi(b)) + y (Phi(b) - Phi(a)) + sigma (phi(a) - phi(b)),
 * strictly increasing with slope Phi(b) - Phi(a).  Declipping is out = clamp(E^-1(in), lo, hi): in <= E(lo) gives lo, in >= E(hi) gives
 * hi, a non-finite value passes through; evaluated by Newton steps on E from the start value in, four in float and then two in double, which
 * leave |E(out) - in| below 1e-11 (the identity where in is more than 9 sigma from both bounds), rounded once to float.  The result is non-decreasing in `in` and the same bits on every call. */
#define LFBM5D_CLIP_LEVELS 64
#define LFBM5D_CLIP_KEYS   322
typedef struct {
    double sigma;                /* the light field's noise level: every non-empty SAI and channel pooled               */
    double sigma_channel[3];     /* per stored channel (NaN for a channel whose own fit fails; grey: [0] only, rest 0)  */
    double f_max;                /* the rung of the ladder that was used                                                */
    double censored;             /* blocks with a censored pixel / blocks counted, all levels                           */
    unsigned levels;             /* levels that counted                                                                 */
    unsigned heavily_clipped;    /* 1 when f_max > 0.1: the estimate leans on levels the clipping has touched           */
    unsigned quantised;          /* 1 when every block counted holds whole numbers: the fit used delta = s / 2          */
    unsigned reserved;
    unsigned long long blocks;   /* 2 x 2 blocks visited (0 from lfbm5d_clip_fit)                                       */
    unsigned long long skipped;  /* of those, skipped for a non-finite m or d                                           */
} lfbm5d_clip_estimate;
/* d_lf [asize][C*H*W] in HBM, read only; h_hist [C][64][322], h_sum [C][64], h_cens [C][64], h_whole [C] (host) receive the counts;
 * blocks / skipped may be NULL.  Returns 1 with a message on a rejected input. */
int lfbm5d_clip_histogram_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                 unsigned C, double lo, double hi, unsigned long long* h_hist, unsigned long long* h_sum,
                                 unsigned long long* h_cens, unsigned long long* h_whole, unsigned long long* blocks,
                                 unsigned long long* skipped);
/* Host only, needs no GPU: the fit above of hist [C][64][322], cens [C][64], whole [C] (sum [C][64], the level means, belongs to the
 * statistics and is not read: the fit has no slope; it may be NULL).  Returns 1 when fewer than 4 levels are populated (or on a NULL
 * pointer, C or a bad range; no message: there is no context). */
int lfbm5d_clip_fit(const unsigned long long* hist, const unsigned long long* sum, const unsigned long long* cens,
                    const unsigned long long* whole, unsigned C, double lo, double hi, lfbm5d_clip_estimate* out);
/* Statistics + fit.  Returns 1 with a message when the fit fails. */
int lfbm5d_noise_level_clipped_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                      unsigned C, double lo, double hi, lfbm5d_clip_estimate* out);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM: identical results. */
int lfbm5d_noise_level_clipped_host_sai(lfbm5d_ctx* ctx, const float* const* h_lf, const unsigned* h_mask, unsigned asize, unsigned W,
                                        unsigned H, unsigned C, double lo, double hi, lfbm5d_clip_estimate* out);
/* d_out = declipped d_in, both [asize][C*H*W] in HBM; d_out may be d_in.  sigma must be finite and positive. */
int lfbm5d_declip_device(lfbm5d_ctx* ctx, double sigma, double lo, double hi, const float* d_in, const unsigned* h_mask, float* d_out,
                         unsigned asize, unsigned W, unsigned H, unsigned C);
int lfbm5d_declip_host_sai(lfbm5d_ctx* ctx, double sigma, double lo, double hi, const float* const* h_in, const unsigned* h_mask,
                           float* const* h_out, unsigned asize, unsigned W, unsigned H, unsigned C);
/* The job: sigma <= 0: lfbm5d_noise_level_clipped_device on d_noisy first (`est`, may be NULL, receives it; zeros when sigma was
 * given); lfbm5d_denoise_device on the clipped data with P1->sigma = P2->sigma = (float)sigma (the sigmas passed are ignored; d_noisy
 * in/out exactly as that call leaves it; the basic estimate between the steps stays in the clipped domain: it is the Wiener pilot of the
 * clipped noisy data); lfbm5d_declip_device in place on d_basic and d_denoised.  Bit-identical to those calls made by hand.
 * `sigma_used` (may be NULL) receives the sigma that was applied.  A sigma that is not finite is rejected. */
int lfbm5d_denoise_clipped_device(lfbm5d_ctx* ctx, double sigma, double lo, double hi, lfbm5d_clip_estimate* est, double* sigma_used,
                                  const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy, const unsigned* h_mask, float* d_basic,
                                  float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1, unsigned an2,
                                  unsigned W, unsigned H, unsigned C);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form.  h_noisy is only read. */
int lfbm5d_denoise_clipped_host_sai(lfbm5d_ctx* ctx, double sigma, double lo, double hi, lfbm5d_clip_estimate* est, double* sigma_used,
                                    const lfbm5d_params* P1, const lfbm5d_params* P2, const float* const* h_noisy, const unsigned* h_mask,
                                    float* const* h_basic, float* const* h_denoised, unsigned ang_major, unsigned awidth,
                                    unsigned aheight, unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C);

/* ---- impulse-noise repair: outlier detection and replacement ahead of the denoiser ----
 * Not in the reference (its authors run such a stage in front of it: README [4]).  The estimators above and the filter assume that every
 * pixel carries Gaussian-like noise; hot and dead pixels, salt and pepper and drop-outs written as 0, 255 or NaN count as noise for the
 * blind sigma, as structure for the block matching, and survive the hard threshold.  This stage finds and replaces them; it is opt-in.
 * Light fields are [asize][C*H*W] float32, channels as stored; h_mask marks empty SAIs, whose planes are neither read nor written; C = 1 or
 * 3; W, H >= 2.  One GPU: contexts with a communicator or a shard return 1.  Everything below is stated in float32 operations without a
 * product, integer counts and order statistics: the GPU equals the numpy model of tests/impulse_model.py bit for bit.
 * Limits: an impulse smeared by demosaicking into a blob, or a cluster that fills a 3 x 3, is not found (its neighbours agree with it);
 * detection here is spatial only (the cross-SAI test is the consistency check below, lfbm5d_consist_*); on nearly noise-free, textured data about 0.4 % of the sound values are touched
 * (DESIGN.md 3g has the table); k = 8 is the cheapest row of that table on sound data, a default and not a law.
 *
 * Neighbours.  For a pixel c of a plane I the neighbours q are the eight positions of the 3 x 3 around it; coordinates outside the plane
 * are mirrored without repeating the edge (-1 -> 1, W -> W - 2), so every neighbour is another real pixel, at the corners too (a pixel
 * may appear twice).
 * ROAD (rank-ordered absolute differences, Garnett et al., IEEE TIP 2005), float32: d_q = |c - q|; a non-finite q or c gives d_q = +inf;
 * with d sorted ascending R = ((d0 + d1) + d2) + d3.
 * Extremeness.  lt = the finite neighbours q < c, gt = the finite neighbours q > c; the pixel is extreme when min(lt, gt) = 0 (not a
 * strict test: two adjacent impulses of one value both qualify).  Without it texture, whose R is large, is flagged 10-70 times as often.
 * Scale.  Per channel a histogram of R over every pixel of every non-empty SAI: E_MIN = -12, E_MAX = 12, Q = (E_MAX - E_MIN) 16 + 2 = 386
 * keys, key = clamp((bits(R) >> 19) - ((E_MIN + 127) << 4) + 1, 0, Q - 1): key 0 is [0, 2^-12), the lower edge e[k] of key k >= 1 is the
 * float whose bits are (k - 1 + 1840) << 19, key 385 collects everything >= 2^12 (R reaches 1020 on 0..255 data).  A non-finite R is
 * skipped and counted.  scale = the 0.5 quantile: n = sum_k h[k], T = 0.5 n, k* = the first k whose cumulative count is >= T,
 * scale = e[k*] + (e[k*+1] - e[k*]) (T - cum[k*-1]) / h[k*] in double (k* = 385 has no upper edge: scale = e[385]); n = 0 fails.  A
 * channel's scale comes from its own histogram, the pooled scale from the channels' histograms added; inside the repair an empty
 * histogram counts as scale 0.
 * Threshold.  T_c = (float) max(k scale_c, min_threshold); a caller-given threshold[c] > 0 replaces it: T_c = (float) threshold[c]; when
 * every channel's is given the statistics pass is skipped (scales 0, skipped 0).
 * Flag.  A pixel is flagged when c is not finite, or when R > T_c and the pixel is extreme.
 * Repair.  The unflagged finite neighbours of a flagged pixel, n of them, sorted ascending (-0 before +0): the pixel becomes element
 * (n - 1) / 2, the lower median -- always an existing pixel value, no arithmetic; n = 0: the pixel is left as it is.  Unflagged pixels are
 * copied unchanged.  Flag plane (optional, uint8 [asize][C*H*W]): 0 = sound, 1 = flagged and repaired, 2 = flagged and left. */
#define LFBM5D_IMPULSE_KEYS 386
typedef struct {
    double k;              /* threshold = k x the channel's median ROAD; >= 0                       */
    double min_threshold;  /* floor of that threshold; >= 0                                         */
    double threshold[3];   /* > 0: this channel's threshold outright (grey: [0] only)               */
} lfbm5d_impulse_params;
typedef struct {
    double scale;                  /* median ROAD of all channels pooled (0 when the statistics pass did not run) */
    double scale_channel[3];       /* per stored channel                                                          */
    double threshold[3];           /* the float32 thresholds that were applied                                    */
    unsigned long long flagged[3]; /* per stored channel: repaired + left                                         */
    unsigned long long repaired[3];
    unsigned long long left[3];    /* flagged pixels without a sound neighbour, left as they were                 */
    unsigned long long pixels;     /* values of the non-empty SAIs                                                */
    unsigned long long skipped;    /* of those, the statistics pass skipped for a non-finite R                    */
} lfbm5d_impulse_result;
/* Host only: k = 8, min_threshold = 0, no given threshold. */
void lfbm5d_impulse_defaults(lfbm5d_impulse_params* out);
/* d_lf [asize][C*H*W] in HBM, read only; h_hist [C][386] (host) receives the counts; pixels / skipped may be NULL.  Returns 1 with a
 * message on a rejected input (a NULL required buffer, C, W / H, a mask without a non-empty SAI, a context with a communicator or shard). */
int lfbm5d_impulse_histogram_device(lfbm5d_ctx* ctx, const float* d_lf, const unsigned* h_mask, unsigned asize, unsigned W, unsigned H,
                                    unsigned C, unsigned long long* h_hist, unsigned long long* pixels, unsigned long long* skipped);
/* Host only, needs no GPU: the scale above of one histogram hist [386].  Returns 1 on an empty histogram (or a NULL pointer; no message:
 * there is no context). */
int lfbm5d_impulse_scale(const unsigned long long* hist, double* scale);
/* Detect and repair: d_out = repaired d_in, both [asize][C*H*W] in HBM.  d_out must not overlap d_in (neighbours are read across tile
 * edges): that returns 1 with a message.  d_flags (uint8 [asize][C*H*W] in HBM) or NULL; out or NULL; h_counts_sai (host,
 * [asize][C][3] = flagged, repaired, left; zeros for empty SAIs) or NULL.  Integer atomics only: repeated calls return the same bits. */
int lfbm5d_impulse_repair_device(lfbm5d_ctx* ctx, const lfbm5d_impulse_params* params, const float* d_in, const unsigned* h_mask, float* d_out,
                                 unsigned char* d_flags, unsigned asize, unsigned W, unsigned H, unsigned C, lfbm5d_impulse_result* out,
                                 unsigned long long* h_counts_sai);
/* Repair under the caller's flags (a camera's fixed defect map): d_flags_in uint8 [asize][C*H*W] in HBM, non-zero = defective; no
 * detection, no statistics (scales and thresholds of `out` are 0); an unflagged non-finite pixel is copied like any other and is no
 * candidate for a neighbour's repair.  d_flags (the codes above) or NULL; it must not overlap d_flags_in. */
int lfbm5d_impulse_repair_flags_device(lfbm5d_ctx* ctx, const float* d_in, const unsigned char* d_flags_in, const unsigned* h_mask,
                                       float* d_out, unsigned char* d_flags, unsigned asize, unsigned W, unsigned H, unsigned C,
                                       lfbm5d_impulse_result* out, unsigned long long* h_counts_sai);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies: identical
 * results.  h_flags_in NULL: detect and repair (params required); otherwise the given-flags form (params ignored).  h_flags or NULL.
 * h_out[st] may be h_in[st]: the staging buffers are distinct. */
int lfbm5d_impulse_repair_host_sai(lfbm5d_ctx* ctx, const lfbm5d_impulse_params* params, const float* const* h_in,
                                   const unsigned char* const* h_flags_in, const unsigned* h_mask, float* const* h_out,
                                   unsigned char* const* h_flags, unsigned asize, unsigned W, unsigned H, unsigned C,
                                   lfbm5d_impulse_result* out, unsigned long long* h_counts_sai);

/* ---- defect inpainting: region fill under a defect map, refined by the hard-thresholding step ----
 * Not in the reference.  The impulse repair above sees a 3 x 3: a dead column pair, a dust shadow on the microlens array, a hot cluster,
 * a hole of non-finite values left by rectification or a region the user masks out is larger than that, is structure to the block
 * matching and survives the threshold.  This stage fills such regions from their rim inwards and then refines the fill with what the
 * other sub-aperture images show of it: super-resolution's loop (above) with a mask as the operator.  Opt-in.
 * Data.  Light fields are [asize][C*H*W] float32, channels as stored; h_mask marks empty SAIs, whose planes are neither read nor written;
 * C = 1 or 3; W, H >= 2.  Flags: uint8 [asize][C*H*W], non-zero = defective.  A value that is not finite counts as flagged whether or not
 * the map names it: nothing non-finite reaches the filter.  One GPU: contexts with a communicator or a shard return 1.
 * Fill (onion peel), per channel plane, in passes.  Neighbours are the eight positions of the 3 x 3, mirrored without repeating the edge
 * (-1 -> 1, W -> W - 2) exactly as in the impulse repair; a mirrored neighbour may appear twice and then counts twice.  In pass t every
 * value that was flagged before the pass and has n >= 1 unflagged neighbours becomes s r[n] (float32): s starts at +0.0f and adds the
 * unflagged neighbours in raster order of the 3 x 3 (rows outer, centre skipped); r[n] = (float)(1.0 / n) is a table.  From pass t + 1 on
 * the value counts as sound (Jacobi: a pass reads only the state before it).  Passes repeat until nothing is flagged or a pass fills
 * nothing; the second case is a plane without one sound value, whose values stay as they are.  Unflagged values are copied unchanged.
 * Flag plane (optional): 0 = sound, 1 = flagged and filled, 2 = flagged and left.  Sums in a fixed order, one product, integer counts: the
 * GPU equals the numpy model of tests/inpaint_model.py bit for bit, and the result does not depend on how the passes fall into launches
 * (LFBM5D_INPAINT_PASSES_PER_LAUNCH of them run in one; a region deeper than that takes another launch).
 * Projection.  out = flag ? x : y, elementwise.
 * Loop.  x_0 = fill(y, f); for k = 1..K: b = the basic estimate of lfbm5d_step1_device on a scratch copy of x_{k-1} with
 * P.sigma = max(tau_k, sigma_noise), tau_k = sigma_start (sigma_end / sigma_start)^((k-1)/(K-1)) (double; K = 1: sigma_start);
 * x_k = f ? b : y; the result is x_K, and K = 0 is the fill alone.  f is "flagged" as above (the map or a non-finite value).  The step
 * runs exactly as lfbm5d_step1_device runs it (colour space, window graph, lanes, every option); every step filters the whole light field,
 * not only the windows that hold defects.  K >= 1 with a value left (a plane without one sound value) returns 1 with a message: such a
 * plane belongs to an SAI that should have been masked as empty.
 * Limits: the map is given (it comes from the consistency check below, lfbm5d_consist_*, or from the impulse repair: the code-2 values of
 * its flag plane can be passed on as a map); blobs are not detected here; a whole missing SAI is reconstructed by the view synthesis below, not here; the defaults are the best of a sweep on one light field
 * (profiles/inpaint_defaults.txt) and claim nothing beyond it. */
#define LFBM5D_INPAINT_PASSES_PER_LAUNCH 8
typedef struct {
    unsigned iterations;   /* K refinement steps; 0 = the fill alone                                                  */
    float sigma_start;     /* tau_1 > 0                                                                               */
    float sigma_end;       /* tau_K, 0 < sigma_end <= sigma_start                                                     */
    float sigma_noise;     /* the noise level of the sound data: a floor under the schedule; >= 0                     */
} lfbm5d_inpaint_params;
typedef struct {
    unsigned long long flagged[3]; /* per stored channel: filled + left                                               */
    unsigned long long filled[3];
    unsigned long long left[3];    /* flagged values of planes without one sound value, left as they were             */
    unsigned long long pixels;     /* values of the non-empty SAIs                                                    */
    unsigned passes;               /* the largest pass number that filled something (the depth of the deepest region) */
    unsigned launches;             /* launches of the fill kernel                                                     */
} lfbm5d_inpaint_result;
/* Host only: K = 8, sigma 30 -> 5, sigma_noise = 0 (the best of the sweep in profiles/inpaint_defaults.txt). */
void lfbm5d_inpaint_defaults(lfbm5d_inpaint_params* out);
/* The fill alone: d_out = filled d_in under d_flags_in, all in HBM; d_in and d_flags_in are only read.  d_out must not overlap d_in, and
 * d_flags (the codes above, or NULL) must not overlap d_flags_in (neighbours are read across tile edges): 1 with a message, as for a NULL
 * required buffer, C, W / H, a mask without a non-empty SAI and a context with a communicator or shard.  out or NULL.  Integer atomics
 * only: repeated calls return the same bits. */
int lfbm5d_inpaint_fill_device(lfbm5d_ctx* ctx, const float* d_in, const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out,
                               unsigned char* d_flags, unsigned asize, unsigned W, unsigned H, unsigned C, lfbm5d_inpaint_result* out);
/* The projection: d_out = d_flags ? d_x : d_y on the non-empty SAIs.  d_out may be d_x or d_y. */
int lfbm5d_inpaint_project_device(lfbm5d_ctx* ctx, const unsigned char* d_flags, const float* d_x, const float* d_y, const unsigned* h_mask,
                                  float* d_out, unsigned asize, unsigned W, unsigned H, unsigned C);
/* The loop: d_out = x_K.  P = the hard-thresholding step's parameters (its sigma is replaced step by step), an = its angular search
 * window; buffers as for the fill; d_flags receives the fill's codes.  `out` (or NULL) is filled in before a K >= 1 call fails for
 * values left. */
int lfbm5d_inpaint_device(lfbm5d_ctx* ctx, const lfbm5d_inpaint_params* params, const lfbm5d_params* P, const float* d_in,
                          const unsigned char* d_flags_in, const unsigned* h_mask, float* d_out, unsigned char* d_flags, unsigned ang_major,
                          unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_inpaint_result* out);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form.  h_flags or NULL.  h_out[st] may be h_in[st]: the staging buffers are distinct. */
int lfbm5d_inpaint_host_sai(lfbm5d_ctx* ctx, const lfbm5d_inpaint_params* params, const lfbm5d_params* P, const float* const* h_in,
                            const unsigned char* const* h_flags_in, const unsigned* h_mask, float* const* h_out,
                            unsigned char* const* h_flags, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W,
                            unsigned H, unsigned C, lfbm5d_inpaint_result* out);

/* ---- view synthesis: whole missing sub-aperture images from their angular neighbours, refined by the hard-thresholding step ----
 * Not in the reference.  The stages above repair values; an SAI that is lost, corrupt or too dark, a failed member of a camera array, or the
 * views an angular up-sampling asks for (3 x 3 in, 5 x 5 out) have no sound value at all.  A point seen at x in SAI (s, t) is seen at
 * x + d (ds, dt) in SAI (s + ds, t + dt) with one scalar disparity d: a plane sweep over d synthesises the view from its sound
 * neighbours, and the loop of the defect inpainting refines it.  d is an integer in the forms below and a multiple of 1 / steps in
 * the *_steps_* forms ("Sub-pixel disparities").  Opt-in.
 * Data.  Light fields are [asize][C*H*W] float32, channels as stored; C = 1 or 3; W, H >= 2.  h_mask marks non-empty SAIs as everywhere;
 * h_missing is unsigned [asize], non-zero = to be reconstructed.  A missing SAI must be non-empty in h_mask (the filter processes it).  The
 * planes of a missing SAI in d_in are never read.  (s, t) of index st: ROWMAJOR st = s awidth + t, COLMAJOR st = s + t aheight; s moves along
 * image rows (y), t along columns (x).  One GPU: contexts with a communicator or a shard return 1.  Source values are assumed finite (the
 * impulse and defect stages run ahead of this one).
 * Sources of a missing SAI m: the SAIs q that are non-empty, not missing, with max(|s_q - s_m|, |t_q - t_m|) <= ang_radius, in increasing
 * index order; n of them.  n = 0: the SAI is left (its planes of d_out are not written; counted in `left`).
 * Warp, for a hypothesis d: w_{q,d}(c, y, x) = I_q(c, rho_H(y - d (s_q - s_m)), rho_W(x - d (t_q - t_m))); rho_n is the reflection of
 * period 2n - 2 that does not repeat the edge (-1 -> 1, n -> n - 2), for any argument (a shift can exceed a narrow plane).
 * Mean: mu_d = (((+0.0f + w_1) + w_2) + ... + w_n) r[n], r[n] = (float)(1.0 / n) from a table; float32.
 * Error: e_d(y, x) = sum_c sum_q (w_{q,d} - mu_d)^2 from +0.0f, c outer, q inner; every difference, product and sum rounded on its own
 * (no fused multiply-add).
 * Box: h_d(y, x) = sum_{k=-r..r} e_d(y, rho_W(x + k)), E_d(y, x) = sum_{k=-r..r} h_d(rho_H(y + k), x), both from +0.0f in that order.
 * Decision: hypotheses in the order 0, -1, +1, -2, +2, ..., -D, +D; one replaces the best so far only if E_d < E_best (ties keep the
 * smaller |d|; n = 1 gives E = 0 everywhere: d = 0, a copy of the source).  The view is mu_{d*} for all C channels.
 * d_disp (optional): int8 [asize][H*W], d* of the synthesised SAIs; other planes are not written.
 * Sums in a fixed order, integer counts: the GPU equals the numpy model of tests/view_model.py bit for bit, values and disparities, and
 * repeated calls return the same bits.
 * Loop.  f = every value of the synthesised SAIs; x_0 = the input with those SAIs replaced; for k = 1..K: b = the basic estimate of
 * lfbm5d_step1_device on a scratch copy of x_{k-1} with P.sigma = max(tau_k, sigma_noise), tau_k on the schedule of the defect inpainting;
 * x_k = f ? b : y.  K = 0 is the synthesis alone.  K >= 1 with an SAI left returns 1 with a message, after `out` is filled in.
 * Sub-pixel disparities (the *_steps_* forms, include/lfbm5d_steps.h, with steps = Q in {1, 2, 4}; lenslet cameras, dense arrays and an
 * angular up-sampling move a fraction of a pixel per view).  Everything above stands but the hypotheses and the warp.
 * Hypotheses: j in the order 0, -1, +1, ..., -DQ, +DQ, d = j / Q; one replaces the best so far only if E_j < E_best (ties keep the
 * smaller |j|).
 * Warp of source q with (ds, dt) = (s_q - s_m, t_q - t_m) at (y, x): ny = Q y - j ds, iy = floor(ny / Q) (floor also for negative ny),
 * py = ny - Q iy (0 <= py < Q); nx, ix, px the same from x and dt.  py and px depend on (j, ds, dt) alone.  wy = (float)py / Q,
 * wx = (float)px / Q, both exact.  lerp(a, b, p, w) = a when p = 0, else a + w (b - a): a difference, a product and a sum in that
 * order, each rounded on its own.  With I the source plane: v00 = I(rho_H(iy), rho_W(ix)), v01 = I(rho_H(iy), rho_W(ix + 1)),
 * v10 = I(rho_H(iy + 1), rho_W(ix)), v11 = I(rho_H(iy + 1), rho_W(ix + 1)); top = lerp(v00, v01, px, wx), bot = lerp(v10, v11, px, wx),
 * w_{q,j} = lerp(top, bot, py, wy); with py = 0 bot is neither needed nor read.  rho is applied to every index on its own, so any
 * shift in any plane of W, H >= 2 is defined.
 * Hence a hypothesis with j a multiple of Q warps exactly as the integer sweep at d = j / Q, in bits, and steps = 1 is the integer
 * sweep: the forms without steps are the steps = 1 calls of the *_steps_* forms.
 * Outputs: d_disp holds j* (d* in units of 1 / Q, |j*| <= 32); the histogram has LFBM5D_VIEW_STEPS_HIST = 65 bins, index j* + 32 for
 * every Q (h_hist_steps); disparity_hist[17] of the result is filled for steps = 1 and all zero otherwise.
 * The GPU equals the numpy model of tests/subpel_model.py bit for bit, values and j*.
 * Limits: bilinear interpolation softens the synthesised view; on noisy sources interpolation lowers the noise of a warped source, so
 * the cost leans towards fractional hypotheses (profiles/view_subpel.txt); Q <= 4; occlusions are not modelled by these forms (the *_occl_* forms of include/lfbm5d_occl.h choose among
 * the full set of sources and four half-planes of them, nothing finer); one scalar d per pixel; sources only within ang_radius; which SAIs are bad is
 * not decided here (the consistency check below does that); one GPU; every step of
 * the loop filters the whole light field; the defaults are the best row of a sweep on one light field (profiles/view_defaults.txt). */
typedef struct {
    unsigned max_disparity; /* D, 0..8: hypotheses -D..D                                                               */
    unsigned box_radius;    /* r, 0..7: the (2r + 1)^2 aggregation box                                                 */
    unsigned ang_radius;    /* 1 or 2: how far (Chebyshev, in views) a source may be                                   */
    unsigned iterations;    /* K refinement steps; 0 = the synthesis alone                                             */
    float sigma_start;      /* tau_1 > 0                                                                               */
    float sigma_end;        /* tau_K, 0 < sigma_end <= sigma_start                                                     */
    float sigma_noise;      /* the noise level of the sound SAIs: a floor under the schedule; >= 0                     */
} lfbm5d_view_params;
typedef struct {
    unsigned missing;       /* SAIs marked missing: synthesised + left                                                 */
    unsigned synthesised;
    unsigned left;          /* missing SAIs without a source, not written                                              */
    unsigned long long pixels;             /* positions of the synthesised SAIs (synthesised * W * H)                  */
    unsigned long long disparity_hist[17]; /* positions per d*, index d + 8                                            */
} lfbm5d_view_result;
/* Host only: D = 4, r = 3, ang_radius = 1, K = 4, sigma 30 -> 5, sigma_noise = 0 (the best row of the sweep in
 * profiles/view_defaults.txt). */
void lfbm5d_view_defaults(lfbm5d_view_params* out);
/* The synthesis alone: the planes of the synthesised SAIs of d_out (and of d_disp, or NULL) are written, nothing else; d_in is only read.
 * 1 with a message: a NULL required buffer, C, W / H, max_disparity, box_radius, ang_radius, ang_major, a missing SAI masked empty, no
 * missing SAI, d_out overlapping d_in, a context with a communicator or shard.  The loop's fields of params are not looked at.  out or
 * NULL.  Integer atomics only: repeated calls return the same bits. */
int lfbm5d_view_fill_device(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, const float* d_in, const unsigned* h_mask,
                            const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major, unsigned awidth,
                            unsigned aheight, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out);
/* The loop: d_out = x_K on every non-empty SAI (the sound SAIs are copies of d_in's; an SAI that is left is not written).  P = the
 * hard-thresholding step's parameters (its sigma is replaced step by step), an = its angular search window. */
int lfbm5d_view_device(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, const lfbm5d_params* P, const float* d_in, const unsigned* h_mask,
                       const unsigned* h_missing, float* d_out, signed char* d_disp, unsigned ang_major, unsigned awidth, unsigned aheight,
                       unsigned an, unsigned W, unsigned H, unsigned C, lfbm5d_view_result* out);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs, and in h_in for missing ones), staged through HBM with
 * blocking copies: bit-identical to the device form.  h_disp or NULL: one int8 plane per missing SAI.  h_out[st] may be h_in[st]. */
int lfbm5d_view_host_sai(lfbm5d_ctx* ctx, const lfbm5d_view_params* params, const lfbm5d_params* P, const float* const* h_in,
                         const unsigned* h_mask, const unsigned* h_missing, float* const* h_out, signed char* const* h_disp,
                         unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C,
                         lfbm5d_view_result* out);

/* ---- consistency check: defective values and bad sub-aperture images found by what the other views say ----
 * Not in the reference.  The three stages above repair what they are told about (a defect map, a list of missing SAIs) or what a 3 x 3
 * shows (single-pixel impulses).  A light field says more: a sound value is predicted by its angular neighbours, a defective one is
 * not.  This stage predicts every SAI from its neighbours with the view synthesis' plane sweep, the SAI itself left out, and tests the
 * residual.  Its flag planes can be handed to lfbm5d_inpaint_* as the map, its bad SAIs to lfbm5d_view_* as the missing list.  Opt-in.
 * Data.  As for the view synthesis: [asize][C*H*W] float32, h_mask, (s, t) by ang_major, C = 1 or 3, W, H >= 2.  h_exclude (optional,
 * unsigned [asize], non-zero = known bad): neither tested nor used as a source.  One GPU: contexts with a communicator or a shard
 * return 1.
 * Tested SAIs.  An SAI m is tested if it is non-empty and not excluded.  Its sources are the view synthesis' sources with "missing" =
 * the exclude set and m: every other usable SAI within ang_radius, in increasing index order, n of them.  n < min_sources (>= 2): the
 * SAI is untested (reported; its flag plane is all 0).
 * Prediction.  Exactly the view synthesis' sweep at (max_disparity, box_radius): d*(y, x) and mu = mu_{d*}(c, y, x).  The tested SAI
 * does not take part, so a defect in it cannot steer d*.
 * Residual and spread, float32, every operation rounded on its own (no fused multiply-add): rho = I_m - mu; a = |rho|;
 * v = sum_q (w_{q,d*} - mu)^2 from +0.0f in source order, per channel.
 * Scale.  Per tested SAI and channel a histogram of a with the impulse repair's keys (LFBM5D_IMPULSE_KEYS, the same key function; a NaN
 * a, from a non-finite source, lands in the last key); a value whose I_m is not finite is skipped and counted.  Medians by
 * lfbm5d_impulse_scale: scale_c of the channel's histogram pooled over the tested SAIs, s_m of SAI m's histogram pooled over channels.
 * Pixel decision.  T_c = (float) max(k scale_c, min_threshold); g = (float)(spread^2), formed in double.  Code 2: I_m is not finite.
 * Code 1: a > T_c and (rho rho) (float)(n - 1) > g v.  The second test keeps depth edges and occlusions out (there the sources
 * disagree among themselves) and rejects the shadow a neighbour's defect delta throws on m: then rho = -delta / n and
 * v = delta^2 (n - 1) / n, the ratio of the two sides is 1 / (n spread^2), so no spread >= 1 flags it.
 * Bad-SAI decision, on the host in double.  ref = the lower median of s_m over the tested SAIs with a non-empty histogram; m exceeds
 * when s_m > sai_factor max(ref, min_scale); m is bad when it exceeds and no tested neighbour q within ang_radius exceeds with
 * s_q > s_m, or with s_q = s_m and q < m (a bad view raises its neighbours' residuals by about delta / n: only the local maximum is
 * bad).  A tested SAI whose histogram is empty (nothing finite) is bad.  sai_factor = 0 switches the decision off.
 * Rounds.  Sweep and statistics run with the current exclude set; new bad SAIs join it and the round repeats; at most max_rounds
 * decisions are made; if the last allowed decision still found one, one more sweep runs without a decision.  Flags, scales, histograms
 * and d* come from the final sweep; `rounds` counts the sweeps.
 * Non-finite source values: decisions within max_disparity ang_radius + box_radius of one are deterministic (comparisons with a NaN are
 * false) but meaningless; fill such values first (lfbm5d_inpaint_fill_device under an empty map), as the Python wrapper does.
 * Sums in a fixed order, integer atomics, quantiles on integer histograms: the GPU equals the numpy model of tests/consist_model.py bit
 * for bit in every integer and float it returns, and repeated calls return the same bits.
 * Sub-pixel disparities (the *_steps_* forms, include/lfbm5d_steps.h): the prediction is the view synthesis' sweep with steps
 * hypotheses per pixel, d_disp holds j*, and the spread v uses the interpolated warp w_{q,j*} of that section; residual, histograms,
 * decisions and everything else are unchanged given the prediction.  The GPU equals tests/subpel_model.py bit for bit.
 * Limits: the view synthesis' (interpolation, Q <= 4, no occlusion reasoning: the check's sweep is the plain one, not lfbm5d_occl.h's); a defect at the same position with zero disparity in
 * every view is consistent, hence invisible; one noise level for the whole field (no per-SAI noise model); one GPU; the defaults are
 * one row of a sweep on one light field (profiles/consist_defaults.txt). */
typedef struct {
    unsigned max_disparity; /* D, 0..8, and                                                                            */
    unsigned box_radius;    /* r, 0..7, and                                                                            */
    unsigned ang_radius;    /* 1 or 2: the sweep's, as in lfbm5d_view_params                                           */
    unsigned min_sources;   /* 2..24: an SAI with fewer sources is untested                                            */
    unsigned max_rounds;    /* 1..64: bad-SAI decisions at most                                                        */
    double k;               /* threshold = k x the channel's median |residual|; >= 0                                   */
    double min_threshold;   /* floor of that threshold; >= 0                                                           */
    double spread;          /* the residual must exceed spread x the sources' standard deviation; >= 0                 */
    double sai_factor;      /* an SAI exceeds at sai_factor x the median SAI scale; 0 = no bad-SAI decision            */
    double min_scale;       /* floor under that median; >= 0                                                           */
} lfbm5d_consist_params;
typedef struct {
    double scale_channel[3];          /* median |residual| per stored channel over the tested SAIs (0: nothing finite)  */
    double threshold[3];              /* the float32 thresholds that were applied                                       */
    unsigned long long flagged[3][2]; /* per stored channel: values with code 1, with code 2                            */
    unsigned long long pixels;        /* values of the tested SAIs                                                      */
    unsigned long long skipped;       /* of those, not finite (code 2)                                                  */
    unsigned bad;                     /* SAIs found bad                                                                 */
    unsigned untested;                /* SAIs with fewer than min_sources sources                                       */
    unsigned tested;
    unsigned rounds;                  /* sweeps                                                                         */
} lfbm5d_consist_result;
/* Host only: D = 4, r = 3, ang_radius = 1 (the view synthesis'), min_sources = 3, max_rounds = 3, k = 8, min_threshold = 0, spread = 4,
 * sai_factor = 1.5, min_scale = 0.5 (the row picked by the sweep in profiles/consist_defaults.txt, which rests on one light field). */
void lfbm5d_consist_defaults(lfbm5d_consist_params* out);
/* d_in is only read.  d_flags: uint8 [asize][C*H*W] in HBM, fully written for non-empty SAIs (0 for untested, bad and excluded ones),
 * untouched for empty ones.  h_state [asize] (host): 0 empty, 1 tested, 2 bad, 3 untested, 4 excluded.  Optional (NULL): h_exclude;
 * d_disp int8 [asize][H*W] in HBM, d* of the tested SAIs (other planes are not written); h_scale_sai [asize] (host), s_m of the tested
 * SAIs and, for a bad one, the s_m it was judged by (0 otherwise); h_hist [asize][C][386] (host); out.  1 with a message: a NULL
 * required buffer, C, W / H, ang_major, awidth / aheight, each parameter out of range, a mask without a non-empty SAI, a light field
 * too large, a context with a communicator or shard. */
int lfbm5d_consist_device(lfbm5d_ctx* ctx, const lfbm5d_consist_params* params, const float* d_in, const unsigned* h_mask,
                          const unsigned* h_exclude, unsigned char* d_flags, unsigned* h_state, signed char* d_disp, double* h_scale_sai,
                          unsigned long long* h_hist, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned W, unsigned H,
                          unsigned C, lfbm5d_consist_result* out);
/* The same on host light fields, one pointer per SAI (NULL allowed for empty SAIs), staged through HBM with blocking copies:
 * bit-identical to the device form.  h_flags: one uint8 plane set per non-empty SAI; h_disp or NULL: one int8 plane per non-empty SAI,
 * written for tested ones. */
int lfbm5d_consist_host_sai(lfbm5d_ctx* ctx, const lfbm5d_consist_params* params, const float* const* h_in, const unsigned* h_mask,
                            const unsigned* h_exclude, unsigned char* const* h_flags, unsigned* h_state, signed char* const* h_disp,
                            double* h_scale_sai, unsigned long long* h_hist, unsigned ang_major, unsigned awidth, unsigned aheight,
                            unsigned W, unsigned H, unsigned C, lfbm5d_consist_result* out);

/* ---- inspection of the last pass's block matching (parity tests) ----
 * n_refs reference patches in raster order; h_refs[n_refs] flat index i*Wb+j;
 * h_self_idx[n_refs*N], h_self_cnt[n_refs] (precompute_BM, core:3301);
 * h_best[A*Wb*Hb] / h_shape[A*Wb*Hb] (precompute_BM_stereo, core:3479; entry st == pst unused).
 * Any output pointer may be NULL.  Returns the number of reference patches via n_refs. */
int lfbm5d_last_bm(lfbm5d_ctx* ctx, unsigned* n_refs, unsigned* h_refs, unsigned* h_self_idx,
                   unsigned* h_self_cnt, unsigned* h_best, unsigned char* h_shape);

/* Raw disparity distance tables of the last pass (the scratch precompute_BM_stereo's sum_table plays in the
 * reference, core:3513-3574), in the layout of the kernel generation that ran (lfbm5d_last_scan_version below): copies min(n_floats, size) floats and
 * returns the count; h_tables == NULL returns the buffer's size in floats.  For the bit-reproducibility tests. */
size_t lfbm5d_last_tables(lfbm5d_ctx* ctx, float* h_tables, size_t n_floats);
/* Candidate scores of the self-similarity search of the last pass, [reference patch][(2 nSim+1)^2] in the scan order of
 * core:3407-3420 (entries no table covers keep 2 * threshold): same calling convention. */
size_t lfbm5d_last_scores(lfbm5d_ctx* ctx, float* h_scores, size_t n_floats);
/* Aggregation weights of the groups of the last pass, [reference patch][channel] (core:413-421: 1 / (sigma_c^2 * retained
 * coefficients) in the hard-threshold step): same calling convention.  Lets a test compare survivor counts group by group. */
size_t lfbm5d_last_weights(lfbm5d_ctx* ctx, float* h_w, size_t n_floats);
/* The group list of the last group launch: the (group, channel) pairs the ordinary kernels of a 3x3 window left to the list
 * launch behind them.  Each entry is group | channel mask << 29: mask 7 for a group whose angular shape is not the whole window
 * (every channel; listed by the shape pre-pass), a single channel bit for a (group, channel) in which a wave of the fast
 * hard-thresholding chain came within the guard band of a threshold.  *n = number of entries (any order); copies min(*n, cap)
 * of them to out (may be NULL).  Returns 0, or -1 on a bad context or a failed copy.  For the tests of the guard band. */
int lfbm5d_last_group_list(lfbm5d_ctx* ctx, unsigned* n, unsigned* out, unsigned cap);
/* Which generation of the table kernel the last pass used, i.e. what lfbm5d_last_tables returns:
 *   3 = ring-sharing workgroups, combined form (the default): the disparity tables never reach memory; the buffer holds
 *       [slot][workgroup of the slot][strip][chunk of 8 steps][lane * 8 + step] pairs of (smallest value of the workgroup's tables,
 *       its place in the reference's scan order), 8 bytes each, then per table an edge array [rows][strips] (table column 0 and the
 *       row-0 entry of every strip's first column) -- lfbm5d_kernels.h, stereo_part_stride / stereo_edge_stride;
 *   2 = ring-sharing workgroups with full tables (LFBM5D_SCAN_FULL_TABLES=1), [slot][(2 nDisp+1)^2]{[strip][Q / 4][lane][Q % 4],
 *       column 0}, lfbm5d_kernels.h stereo_table_stride2;
 *   1 = one wave per table (12x12 patches, irregular reference lists, estimates of 2 GiB and more, LFBM5D_SCAN_V1=1), skewed
 *       layout [slot][(2 nDisp+1)^2][strip][table row + lane][64], stereo_table_stride. */
int lfbm5d_last_scan_version(const lfbm5d_ctx* ctx);

/* The aggregation launch of a core pass (core:484-528) alone, on buffers the caller supplies: what a pass hands its aggregation
 * kernel, spelled out.  For the tests that predict num / den bit for bit (tests/agg_model.py).  Device pointers unless marked host. */
typedef struct lfbm5d_agg_debug {
    float* num;                 /* [A][C][Hb][Wb] sums of the padded window, added to in place; direct form: [SAI][C][H][W], lf_stride apart */
    float* den;
    const float* filt;          /* filtered patches of the launch's groups: [g - ref_begin][N][A][C][k*k], or SAI-major [A][g - ref_begin][N][C][k*k] */
    const float* wgt;           /* [n_refs_total][C] group weights */
    const unsigned* aggpos;     /* [A][n_refs_total][N] (row << 16) | column of every patch in the padded window, 0xffffffff: absent; 16-byte aligned */
    const unsigned* mask;       /* host, [A]: non-zero = the SAI of this slot is there */
    const unsigned* proc;       /* host, [A]: non-zero = already processed (skipped) */
    const unsigned* sai;        /* host, [A]: direct form, slot -> SAI of the light field (else unused, may be NULL) */
    unsigned long long filt_sai_stride;   /* 0: group-major; > 0: SAI-major, floats per SAI */
    unsigned long long filt_bytes;        /* size of filt */
    unsigned long long lf_stride;         /* direct form: floats per SAI of num / den */
    unsigned long long sums_floats;       /* size of num and of den, */
    unsigned long long wgt_floats;        /* ... of wgt */
    unsigned long long aggpos_words;      /* ... and of aggpos: the geometry below is checked against them */
    unsigned n_refs_total;      /* reference patches of the pass (regular grid: n_ref_rows * n_ref_cols) */
    unsigned ref_begin, n_groups;   /* the launch's groups: whole rows of the regular grid, any slice of an irregular list */
    unsigned n_ref_rows, n_ref_cols;
    unsigned Wb, Hb, C, A, k, N, pst, p, nSim, nDisp;
    unsigned irregular;         /* the reference list is not the regular grid (nHW + i p, forced last index) */
    unsigned wchan0;            /* every channel takes channel 0's weight */
    unsigned direct;            /* tiles over the interior only, num / den are the light field's */
} lfbm5d_agg_debug;
/* Checks the arguments against what the kernel assumes (message via lfbm5d_last_error, nothing launched), then runs the launch on
 * the context's stream with the context's options (agg_64bit, agg_scalar_scan) and the Kaiser window of patch size k, and waits. */
int lfbm5d_debug_aggregate(lfbm5d_ctx* ctx, const lfbm5d_agg_debug* args);

/* The group launch of a core pass (core:277-481 / :1054-1282) alone: gather, transforms, shrinkage, inverses and group weights on
 * block-matching tables the caller supplies.  For the tests that compare every filtered patch with a model of the chain
 * (tests/group_model.py).  Device pointers unless marked host. */
typedef struct lfbm5d_group_debug {
    const float* noisy;         /* [A][C][Hb][Wb] the padded window */
    const float* basic;         /* the same of the pilot: step 2 only (else unused, may be NULL) */
    const unsigned* refs;       /* [n_refs_total] reference patches, flat positions i * Wb + j */
    const unsigned* self_idx;   /* [n_refs_total][N] the stack of every reference patch in the processed SAI */
    const unsigned* self_cnt;   /* [n_refs_total] its size: a power of two in 1..N (bm3d: 2..N, the selection stores a single match twice) */
    const unsigned* best;       /* [A][Wb*Hb] disparity match of every position (entry pst unused) */
    const unsigned char* shape; /* [A][Wb*Hb] non-zero: the SAI belongs to the angular shape of the reference patch at this position */
    float* filt;                /* out: the launch's groups [g - ref_begin][N][A][C][k*k], or SAI-major [A][g - ref_begin][N][C][k*k] */
    float* wgt;                 /* out: [n_refs_total][C], the launch's rows are written */
    unsigned* aggpos;           /* out: [A][n_refs_total][N], (row << 16) | column or 0xffffffff */
    unsigned long long* counters;   /* host, out: [2] what the launch counted: sum of the stack sizes, shape-adaptive groups */
    const unsigned* mask;       /* host, [A]: non-zero = the SAI of this slot is there */
    const lfbm5d_params* params;   /* host: the pass's parameters (sigma, lambda, N, k, useSD, transforms, colour space) */
    char* kernels;              /* host, out (may be NULL): the kernels launched, in order, names joined by '+' */
    unsigned long long filt_sai_stride;   /* 0: group-major; > 0: SAI-major, floats per SAI (general kernels only) */
    unsigned long long image_floats;      /* size of noisy (and basic), */
    unsigned long long table_words;       /* ... of best and of shape (entries), */
    unsigned long long filt_floats;       /* ... of filt, */
    unsigned long long wgt_floats;        /* ... of wgt */
    unsigned long long aggpos_words;      /* ... and of aggpos: the geometry below is checked against them */
    unsigned long long kernels_cap;       /* bytes behind `kernels` (the text is cut to fit, always terminated) */
    unsigned step;              /* 1: hard thresholding, 2: Wiener */
    unsigned aw, ah;            /* the angular window, A = aw * ah */
    unsigned Wb, Hb, C, pst;
    unsigned fill_quirk;        /* 1 as in a centre pass: patches at columns >= Wb - k read as zeros; 0 as in a subset pass */
    unsigned n_refs_total;
    unsigned ref_begin, n_groups;   /* the launch's groups */
    unsigned bm3d;              /* the per-SAI BM3D arithmetic (A = 1) */
} lfbm5d_group_debug;
/* Checks the arguments and the tables against what the kernels assume (message via lfbm5d_last_error, nothing launched), then runs
 * launch_group as a pass does -- same thresholds, lambda rule, sigma table, scratch and options of the context -- on the context's
 * stream, and waits.  The group list of the launch is read with lfbm5d_last_group_list. */
int lfbm5d_debug_group(lfbm5d_ctx* ctx, const lfbm5d_group_debug* args);

/* The kernels of the window schedule (lfbm5d_window.hip) alone, one launcher per call, on buffers the caller supplies: colour
 * transforms, mirror padding and cropping, estimates, coverage counts, the two ends of a window, the per-SAI finalisation and
 * output kernels, the tile and band copies.  For the tests that predict every one of them bit for bit (tests/window_model.py).
 * `op` selects the launcher; the table says which fields it reads (everything else is ignored):
 *   COLOR             noisy in place, [n_sai][lf_stride] holding [3][H][W]; dmask (may be NULL); cs; forward
 *   COLOR_ROUNDTRIP   noisy -> out (out == noisy allowed), likewise
 *   SYMETRIZE         noisy [C][H][W] -> w_noisy [C][H + 2 N][W + 2 N]
 *   CROP              w_noisy [C][H + 2 N][W + 2 N] -> out [C][H][W], the crop at (off, off); off == N: unsymetrize
 *   SYMETRIZE_MULTI   noisy [SAI][lf_stride] -> w_noisy [slot][w_stride], slot i <- SAI list[i]
 *   UNSYMETRIZE_MULTI w_noisy [slot][w_stride] -> out [SAI][lf_stride], SAI list[i] <- slot i
 *   ESTIMATE          est[i] = den[i] ? num[i] / den[i] : sub[i] on n elements
 *   ESTIMATE_MULTI    w_num, w_den, w_noisy (the substitute) [slot][C][n] -> est [slot][n], channel 0 of the slots of slot_mask
 *   ESTIMATE_LF       num, den, sub -> out, [n_sai][n]; dmask (may be NULL)
 *   WINDOW_BEGIN      noisy, basic (may be NULL), num, den [SAI][lf_stride] -> w_noisy, w_basic, w_num, w_den [slot][w_stride] and
 *                     est [slot][(H + 2 N)(W + 2 N)]; counters[0 .. 32) cleared; direct form: w_num == w_den == NULL
 *   WINDOW_END        w_num, w_den -> num, den (of SAI list[i]), the coverage count added to counters[0 .. 32); patch side k;
 *                     direct form (w_num == w_den == NULL): the count alone, from den
 *   FINALIZE          num, den, sub -> basic, the SAIs list[0 .. n_list) of [SAI][lf_stride] holding [3][H][W]; cs; colour
 *   OUTPUT            num, den, sub -> out; basic in place (may be NULL); noisy -> noisy_dst; likewise (sub == basic, noisy == noisy_dst allowed)
 *   COUNT_ZEROS       den [n_sai][n]: counters[i] += exact zeros of segment i
 *   COUNT_DENOISED    w_den [slot][w_stride] holding [C][H + 2 N][W + 2 N], the slots of slot_mask: counters[0] += the coverage count; k
 *   COPY_RECT         w_noisy (slots w_stride apart, [C][sH][sW]) -> out (slots lf_stride apart, [C][H][W]): the rw x rh rectangle at
 *                     (sx0, sy0) to (dx0, dy0), the slots of slot_mask
 *   COPY_ROWS         w_noisy (n_sai planes of sH rows of W) rows [sy0, sy0 + rh) -> out (planes of H rows) rows dy0 ...
 * Device pointers unless marked host. */
enum lfbm5d_window_op {
    LFBM5D_WOP_COLOR = 0, LFBM5D_WOP_COLOR_ROUNDTRIP = 1, LFBM5D_WOP_SYMETRIZE = 2, LFBM5D_WOP_CROP = 3, LFBM5D_WOP_SYMETRIZE_MULTI = 4,
    LFBM5D_WOP_UNSYMETRIZE_MULTI = 5, LFBM5D_WOP_ESTIMATE = 6, LFBM5D_WOP_ESTIMATE_MULTI = 7, LFBM5D_WOP_ESTIMATE_LF = 8,
    LFBM5D_WOP_WINDOW_BEGIN = 9, LFBM5D_WOP_WINDOW_END = 10, LFBM5D_WOP_FINALIZE = 11, LFBM5D_WOP_OUTPUT = 12, LFBM5D_WOP_COUNT_ZEROS = 13,
    LFBM5D_WOP_COUNT_DENOISED = 14, LFBM5D_WOP_COPY_RECT = 15, LFBM5D_WOP_COPY_ROWS = 16
};
typedef struct lfbm5d_window_debug {
    float* noisy;               /* the light-field side: lf_stride floats per SAI, lf_floats each */
    float* basic;
    float* num;
    float* den;
    float* sub;
    float* out;
    float* noisy_dst;
    float* w_noisy;             /* the window side: w_stride floats per slot, w_floats each */
    float* w_basic;
    float* w_num;
    float* w_den;
    float* est;                 /* est_floats */
    unsigned* counters;         /* counter_words */
    const unsigned* dmask;      /* [n_sai] SAI mask on the device (0 = skip), dmask_words; NULL: every SAI */
    const unsigned* list;       /* host, [n_list]: slot -> SAI of the light field, 0xffffffff: empty slot */
    const unsigned* slot_mask;  /* host, [n_list]: non-zero = the slot is there */
    unsigned long long lf_stride;
    unsigned long long w_stride;
    unsigned long long lf_floats;
    unsigned long long w_floats;
    unsigned long long est_floats;
    unsigned long long n;       /* elements (ESTIMATE), per slot (ESTIMATE_MULTI), per segment (ESTIMATE_LF, COUNT_ZEROS) */
    unsigned op;
    unsigned W, H, C, N, k, off;
    unsigned cs, forward, colour;
    unsigned n_sai;             /* SAIs, segments or planes of the ops without a list */
    unsigned n_list;            /* entries of list / slot_mask */
    unsigned sW, sH, sx0, sy0, dx0, dy0, rw, rh;
    unsigned counter_words, dmask_words;
} lfbm5d_window_debug;
/* Checks the arguments against what the kernels take for granted (message via lfbm5d_last_error, nothing launched): pointers, C,
 * sizes of 0, the colour space, N <= W and N <= H where the op mirrors, k <= W and k <= H where it counts, at most 289 slots, list entries inside the
 * light field the buffer sizes imply, strides of at least one image, every buffer against the geometry, rectangles and row ranges
 * inside their images.  Then runs the one launcher on the context's stream, and waits. */
int lfbm5d_debug_window(lfbm5d_ctx* ctx, const lfbm5d_window_debug* args);

/* The noise level of every channel behind the forward colour transform (utilities.cpp:633-684), as the passes take it: out[0 .. C).
 * Host only, no context.  Returns non-zero for an unknown colour space. */
int lfbm5d_sigma_table(float sigma, unsigned C, unsigned color_space, float* out);

/* ---- device memory helpers so hosts without a HIP binding (ctypes, cgo, JNI) can stage data ---- */
int lfbm5d_malloc(void** dptr, size_t bytes);
int lfbm5d_free(void* dptr);
int lfbm5d_memcpy_h2d(void* dst, const void* src, size_t bytes);
int lfbm5d_memcpy_d2h(void* dst, const void* src, size_t bytes);
int lfbm5d_device_count(void);

/* ---- the sub-pixel forms of the view synthesis and the consistency check (lfbm5d_*_steps_*) ---- */
#include "lfbm5d_steps.h"
/* ---- the occlusion-aware forms of the view synthesis (lfbm5d_view_*_occl_*) ---- */
#include "lfbm5d_occl.h"
/* ---- photometric equalisation: per-view gains estimated and divided out (lfbm5d_photo_*) ---- */
#include "lfbm5d_photo.h"
/* ---- clipped Poisson-Gaussian noise: censored fit, stabiliser and exact unbiased inverse (lfbm5d_pgclip_*) ---- */
#include "lfbm5d_pgclip.h"
/* ---- per-view noise levels: one sigma per SAI, one sigma per angular window (lfbm5d_views_*, lfbm5d_*_views_*) ---- */
#include "lfbm5d_views.h"
/* ---- joint repair of defects and missing views by a mask-aware plane sweep (lfbm5d_repair_*) ---- */
#include "lfbm5d_repair.h"
/* ---- spatially correlated noise: autocorrelation, GPU measurement, per-coefficient variance table (lfbm5d_corr_*, lfbm5d_*_corr_*) ---- */
#include "lfbm5d_corr.h"

#ifdef __cplusplus
}
#endif
#endif
