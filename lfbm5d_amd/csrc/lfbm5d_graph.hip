/*
 * lfbm5d_graph.hip -- a job's windows as a dependency graph (lfbm5d_plan.h) executed on lanes and ranks: run_graph with its RCCL
 * and IPC transports and the streamed host seam.  Split from lfbm5d_api.hip in round 6 (lfbm5d_ctx.h).
 */
#include "lfbm5d_graph.h"

namespace lfbm5d_host {

/* ------------------------------------------------------------------------------------------ */
/* The window graph: one step, or both steps of a denoise, executed as a dependency graph     */
/* ------------------------------------------------------------------------------------------ */

/* A JOB: run_bm5d_1st_step, run_bm5d_2nd_step, or the two back to back (lfbm5d_denoise_device).  The graph (lfbm5d_plan.h) is
 * executed on LANES -- a lane = a context of its own: stream, window buffers, per-pass work buffers -- with HIP events for the
 * dependencies between lanes; on several GPUs every rank runs the windows it owns and what a window needs from a
 * window of another rank arrives as point-to-point messages (RCCL send / recv over xGMI).  Either way every window sees exactly
 * the num / den (and, in the second step of a two-step job, the basic estimate) the window-after-window order of the
 * reference would show it: the result is bit-identical to one lane on one GPU.
 *
 * The reference decides after every pass whether the window is complete (coverage count, bm5d.cpp:370-382); for colour light
 * fields one centre pass always suffices.  The graph form assumes that, copies every window's
 * count to pinned memory and checks them all at the end (*complete). */
/* the blocking form of the host seam (jobs outside the single-rank window graph): every SAI of the caller's light field(s) up
 * before the job, every output down after it */
int io_upload_all(lfbm5d_ctx* c, const HostIO* io, const unsigned* h_mask, unsigned asize, size_t img, float* d_noisy, float* d_basic_in) {
    for (unsigned st = 0; st < asize; st++) {
        if (!h_mask[st]) continue;
        HIPCK(c, hipMemcpyAsync(d_noisy + (size_t)st * img, io->noisy[st], img * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (d_basic_in) HIPCK(c, hipMemcpyAsync(d_basic_in + (size_t)st * img, io->basic[st], img * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}
/* one SAI of the job's light fields down to the caller's (d_basic / d_out: nullptr = the job has none) */
static int io_download(lfbm5d_ctx* c, const HostIO* io, unsigned st, size_t img, const float* d_noisy, const float* d_basic, const float* d_out, hipStream_t xs) {
    HIPCK(c, hipMemcpyAsync(io->noisy[st], d_noisy + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToHost, xs));
    if (d_basic) HIPCK(c, hipMemcpyAsync(io->basic[st], d_basic + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToHost, xs));
    if (d_out) HIPCK(c, hipMemcpyAsync(io->out[st], d_out + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToHost, xs));
    return 0;
}
int io_download_all(lfbm5d_ctx* c, const HostIO* io, const unsigned* h_mask, unsigned asize, size_t img, const float* d_noisy,
                    const float* d_basic, const float* d_out) {
    for (unsigned st = 0; st < asize; st++)
        if (h_mask[st] && io_download(c, io, st, img, d_noisy, d_basic, d_out, c->stream)) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* ---- rendezvous of the two-processes-on-one-GPU transport: small files in a directory both processes see ---- */
bool ipc_put(const std::string& dir, const std::string& name, const void* data, size_t bytes) {
    const std::string tmp = dir + "/." + name + ".tmp", fin = dir + "/" + name;
    { std::ofstream f(tmp, std::ios::binary); if (!f) return false; f.write(reinterpret_cast<const char*>(data), (std::streamsize)bytes); if (!f) return false; }
    return std::rename(tmp.c_str(), fin.c_str()) == 0;
}
bool ipc_get(const std::string& dir, const std::string& name, void* data, size_t bytes, double timeout_s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        std::ifstream f(dir + "/" + name, std::ios::binary);
        if (f) { f.read(reinterpret_cast<char*>(data), (std::streamsize)bytes); if (f.gcount() == (std::streamsize)bytes) return true; }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return false;
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
}
/* every rank publishes `mine`, returns everybody's (a barrier when nobody reads the values) */
int ipc_allgather(lfbm5d_ctx* c, const char* tag, int mine, std::vector<int>& all) {
    const std::string base = c->ipc_tag + tag + "." + std::to_string(c->ipc_epoch) + ".";
    if (!ipc_put(c->ipc_dir, base + std::to_string(c->rank), &mine, sizeof(int))) return fail(c, "ipc transport: cannot write to the rendezvous directory");
    all.assign((size_t)c->world, 0);
    for (int r = 0; r < c->world; r++)
        if (!ipc_get(c->ipc_dir, base + std::to_string(r), &all[(size_t)r], sizeof(int), c->ipc_timeout_s))
            return fail(c, "ipc transport: rank " + std::to_string(r) + " did not reach '" + tag + "' within the watchdog (peer gone?)");
    return 0;
}
/* publish this rank's buffers, map every peer's (re-opened only when a peer's allocation changed) */
int ipc_exchange_handles(lfbm5d_ctx* c, void* const (&mine)[7]) {
    lfbm5d_ctx::IpcPeer me;
    std::memset(&me, 0, sizeof(me));
    for (int i = 0; i < 7; i++)
        if (mine[i]) {
            hipIpcMemHandle_t h;
            HIPCK(c, hipIpcGetMemHandle(&h, mine[i]));
            static_assert(sizeof(h) <= 64, "handle size");
            std::memcpy(me.handle[i], &h, sizeof(h));
        }
    const std::string base = c->ipc_tag + "handles." + std::to_string(c->ipc_epoch) + ".";
    if (!ipc_put(c->ipc_dir, base + std::to_string(c->rank), me.handle, sizeof(me.handle))) return fail(c, "ipc transport: cannot write to the rendezvous directory");
    c->ipc_peers.resize((size_t)c->world);
    for (int r = 0; r < c->world; r++) {
        if (r == c->rank) continue;
        unsigned char hs[7][64];
        if (!ipc_get(c->ipc_dir, base + std::to_string(r), hs, sizeof(hs), c->ipc_timeout_s))
            return fail(c, "ipc transport: rank " + std::to_string(r) + " did not publish its buffers within the watchdog (peer gone?)");
        lfbm5d_ctx::IpcPeer& P = c->ipc_peers[(size_t)r];
        static const unsigned char zero[64] = {0};
        for (int i = 0; i < 7; i++) {
            if (P.ptr[i] && std::memcmp(P.handle[i], hs[i], 64) == 0) continue;
            if (P.ptr[i]) { (void)hipIpcCloseMemHandle(P.ptr[i]); P.ptr[i] = nullptr; }
            std::memcpy(P.handle[i], hs[i], 64);
            if (std::memcmp(hs[i], zero, 64) == 0) continue;
            hipIpcMemHandle_t h;
            std::memcpy(&h, hs[i], sizeof(h));
            HIPCK(c, hipIpcOpenMemHandle(&P.ptr[i], h, hipIpcMemLazyEnablePeerAccess));
        }
    }
    return 0;
}

int lane_buffers(lfbm5d_ctx* c, lfbm5d_ctx* x, size_t win_floats, bool with_basic, bool with_sums, unsigned asize, Lane& L) {
    HIPCK(c, x->w_noisy.reserve(win_floats * sizeof(float)));
    if (with_basic) HIPCK(c, x->w_basic.reserve(win_floats * sizeof(float)));
    if (with_sums) {
        HIPCK(c, x->w_num.reserve(win_floats * sizeof(float)));
        HIPCK(c, x->w_den.reserve(win_floats * sizeof(float)));
    }
    HIPCK(c, x->small.reserve((asize + 8 + kWinCounters) * sizeof(unsigned)));
    L.x = x; L.w_noisy = x->w_noisy.as<float>(); L.w_basic = x->w_basic.as<float>();
    L.w_num = with_sums ? x->w_num.as<float>() : nullptr; L.w_den = with_sums ? x->w_den.as<float>() : nullptr; L.d_small = x->small.as<unsigned>();
    return 0;
}

int zeroed_sums(lfbm5d_ctx* c, lfbm5d_ctx* x, int n_slots, size_t floats, hipStream_t xs, float* g_num[2], float* g_den[2]) {
    DevBuf* nb[2] = {&x->g_num, &x->g_num2}; DevBuf* db[2] = {&x->g_den, &x->g_den2};
    for (int sl = 0; sl < n_slots; sl++) {
        HIPCK(c, nb[sl]->reserve(floats * sizeof(float)));
        HIPCK(c, db[sl]->reserve(floats * sizeof(float)));
        g_num[sl] = nb[sl]->as<float>(); g_den[sl] = db[sl]->as<float>();
        HIPCK(c, hipMemsetAsync(g_num[sl], 0, floats * sizeof(float), xs));
        HIPCK(c, hipMemsetAsync(g_den[sl], 0, floats * sizeof(float), xs));
    }
    return 0;
}

void abort_comms(lfbm5d_ctx* c, const char* what) {
    if (c->comm2) { (void)ncclCommAbort(c->comm2); c->comm2 = nullptr; }
    if (c->comm) { (void)ncclCommAbort(c->comm); c->comm = nullptr; }
    c->err += std::string(" (") + what + " aborted: the RCCL communicators of this context were torn down, call lfbm5d_comm_init again)";
}
void close_ipc_peers(lfbm5d_ctx* c) {
    for (lfbm5d_ctx::IpcPeer& P : c->ipc_peers) for (void*& q : P.ptr) if (q) { (void)hipIpcCloseMemHandle(q); q = nullptr; }
}

namespace {

/* Two-step jobs: a SAI no window of the first step touches (LFBM5D_MAX_WINDOWS) keeps the first step's input as its basic
 * estimate (bm5d.cpp:405 with den == 0), i.e. what the second step reads as noisy. */
int input_as_basic(lfbm5d_ctx* c, const GraphJob& J, const std::vector<unsigned>& sais, float* basic, size_t img, hipStream_t xs) {
    for (unsigned st : sais)
        HIPCK(c, hipMemcpyAsync(basic + (size_t)st * img, J.noisy[1] + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
    return 0;
}

/* The streamed host seam of a single-rank job (io != nullptr): the caller's SAIs come up as the windows first use them and every
 * SAI's outputs leave behind the window that makes them final.  With the seam on there is one rank: the job's sums and basic
 * estimate are the ones the windows work on. */
struct HostSeam {
    lfbm5d_ctx* const c; const GraphJob& J; const plan::Graph& G; const size_t img; const unsigned WH; const bool two, colour;
    const int Ls;                                   /* the slot whose sums are the job's result */
    const HostIO* io = nullptr;
    bool basic_in = false;                          /* run_bm5d_2nd_step alone: LF_basic is an input */
    std::vector<char> up;                           /* per SAI: uploaded */
    std::vector<hipEvent_t> ev_up, ev_out;          /* per SAI: its upload; per node: its outputs formed */
    std::vector<std::vector<unsigned>> outs;        /* per node: the SAIs whose outputs are final behind it */
    std::vector<unsigned> out_nodes;

    /* one SAI of the caller's light field(s) into HBM and into the form the windows read: what run_bm5d_* does to the whole light
     * field at entry (bm5d.cpp:133, :827-830), per SAI; the copy is from pageable memory, i.e. it returns when the data has left */
    int upload(unsigned st) {
        hipStream_t xs = c->io_in;
        const size_t off = (size_t)st * img;
        float* const dn = J.d_noisy + off;
        HIPCK(c, hipMemcpyAsync(dn, io->noisy[st], img * sizeof(float), hipMemcpyHostToDevice, xs));
        HIPCK(c, hipMemcpyAsync(J.pristine + off, dn, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
        if (basic_in) {
            HIPCK(c, hipMemcpyAsync(J.d_basic + off, io->basic[st], img * sizeof(float), hipMemcpyHostToDevice, xs));
            HIPCK(c, hipMemcpyAsync(J.pristine_b + off, J.d_basic + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
        }
        if (colour) {
            HIPCK(c, launch_color_lf(xs, dn, img, 1, J.d_mask + st, J.color_space, WH, 1));
            if (basic_in) HIPCK(c, launch_color_lf(xs, J.d_basic + off, img, 1, J.d_mask + st, J.color_space, WH, 1));
            if (two) HIPCK(c, launch_color_roundtrip_lf(xs, dn, const_cast<float*>(J.noisy[1]) + off, img, 1, J.d_mask + st, J.color_space, WH));
        }
        if (two && G.last_touch[0][st] < 0 && input_as_basic(c, J, {st}, J.d_basic, img, xs)) return 1;
        ev_up[st] = get_event(c);
        HIPCK(c, hipEventRecord(ev_up[st], xs));
        up[st] = 1;
        return 0;
    }
    /* the outputs of these SAIs in the form the caller gets them, kBigA SAIs to a launch */
    int form_outputs(hipStream_t xs, const std::vector<unsigned>& sais) {
        for (size_t o0 = 0; o0 < sais.size(); o0 += (size_t)kBigA) {
            SaiList ol; ol.n = 0;
            for (size_t q = o0; q < sais.size() && ol.n < (unsigned)kBigA; q++) ol.st[ol.n++] = sais[q];
            HIPCK(c, launch_output_multi(xs, J.g_num[Ls], J.g_den[Ls], J.step[Ls] == 1 ? J.noisy[Ls] : J.d_basic, J.d_out,
                                         J.step[Ls] == 2 ? J.d_basic : nullptr, J.noisy[Ls], J.d_noisy, img, ol, J.color_space, WH, colour ? 1 : 0));
        }
        return 0;
    }
    int download(unsigned st) {   /* (a first step's result is what the caller knows as `basic`) */
        const bool second = J.step[Ls] == 2;
        return io_download(c, io, st, img, J.d_noisy, second ? J.d_basic : J.d_out, second ? J.d_out : nullptr, c->io_out);
    }
};

/* An error return in the middle of the graph (a failed HIP call, an RCCL call that reports an error) would leave this
 * rank's queued sends / receives waiting for peers that will never get their counterparts -- and the peers waiting for this
 * rank.  With real ranks the way out is to abort the communicators: RCCL then fails the pending operations here, the peers
 * see the failure through their own RCCL error paths (or their caller's watchdog -- bench.py has one), and every later call
 * on this context reports that the communicator is gone instead of hanging.  Disarmed when the graph has run through. */
struct AbortCommsOnError {
    lfbm5d_ctx* c; bool armed;
    ~AbortCommsOnError() { if (armed) { abort_comms(c, "multi-GPU step"); (void)hipDeviceSynchronize(); } }
};
/* The IPC transport has no communicator to abort: its gating kernels end by their own watchdog.  After an error the ranks may
 * have stopped at different points of the issue order (and of the rendezvous epochs), so the transport of this context is
 * closed: the next job fails at once instead of waiting for peers that are out of step. */
struct CloseIpcOnError {
    lfbm5d_ctx* c; bool armed;
    ~CloseIpcOnError() {
        if (!armed) return;
        (void)hipDeviceSynchronize();
        close_ipc_peers(c);
        c->ipc = false;
        c->err += " (multi-process step aborted: the IPC transport of this context was closed, call lfbm5d_comm_init_ipc again)";
    }
};
/* ... and where no RCCL operation can be pending (one rank, emulated ranks, the IPC transport) an error return must not leave
 * kernels of other lanes running on the caller's buffers (which the caller is free to release once the call has failed): wait
 * for whatever has been enqueued.  With real RCCL ranks the synchronisation belongs behind the abort (AbortCommsOnError does it): in
 * front of it, it would wait for sends / receives whose peers never post their counterparts. */
struct DrainOnError { bool armed; ~DrainOnError() { if (armed) (void)hipDeviceSynchronize(); } };

struct Geo { unsigned asw, Aw, nHW, wb, hb; size_t imgb; };   /* geometry of a step slot's windows */
struct RankState { int rank; lfbm5d_ctx* x; float* g_num[2]; float* g_den[2]; float* basic; std::vector<Lane> lanes; };

/* The state of one job of the window graph; run_graph below calls its phases in order. */
struct GraphRun {
    lfbm5d_ctx* const c; const GraphJob& J; const plan::Graph& G; const unsigned* const h_mask; const plan::Grid grid;   /* run_graph's arguments */
    const unsigned W, H, C; const int nranks; const bool emulate;
    const unsigned asize = grid.size(); const size_t img = (size_t)C * W * H; const hipStream_t s = c->stream;
    const size_t NN = G.nodes.size(); const bool two = J.n_steps == 2;
    const int Ls = J.n_steps - 1;                       /* the slot whose sums are the job's result */
    Geo geo[2];
    /* Every window of the graph has exactly one pass, and the next window on its SAIs pads again from the light field: the mirror ring
     * of a window's sums is never read.  So the aggregation works straight on the light field's num / den (AggArgs::direct), tiles over
     * the interior only, and a window has no padded sums at all -- no copies in k_window_begin, no copy back in k_window_end, which is
     * left with the coverage count.  Same sums, bit for bit.  Option window_sums_padded restores the padded copies (tests, A/B runs). */
    const bool direct = !c->opt->window_sums_padded;
    bool ipc = false;                                   /* ranks = processes on this GPU */
    AbortCommsOnError abort_guard{c, false}; CloseIpcOnError ipc_guard{c, false}; DrainOnError drain_guard{false};   /* (destroyed in reverse order) */
    std::vector<RankState> states;                      /* the ranks that live here: this one, or every emulated one */
    std::vector<unsigned> untouched;                    /* two-step jobs: SAIs without a first-step window (input_as_basic) */
    HostSeam seam{c, J, G, img, W * H, two, C == 3 && J.color_space != LFBM5D_RGB, Ls};
    unsigned* ipc_own = nullptr;                        /* this process's gating words */
    std::vector<size_t> ipc_sent;                       /* messages this rank sent: their "taken" words are waited for before the drain */
    std::vector<hipEvent_t> done, arrived;              /* per node: enqueued here and done; per message: it has reached its consumer's rank */
    std::vector<std::vector<int>> sum_xfer, basic_xfer; /* message of (producer node, SAI slot) / of (reader rank, SAI) */
    std::vector<unsigned> n_in;                         /* per node: the SAIs of its window once it is enqueued here (0: another rank's) */
    ncclComm_t comms[2] = {c->comm, c->comm2 ? c->comm2 : c->comm};
    /* the job's transport: message_emulated | message_ipc | message_rccl */
    int (GraphRun::*message)(size_t, const plan::Xfer&, int, int, int, RankState*, RankState*, size_t) = nullptr;
    size_t xi = 0, n_msgs = 0;                          /* next message of the issue order; messages this rank took part in */
    int complete = 1;

    RankState* local(int r) { return emulate ? &states[(size_t)r] : (r == c->rank ? &states[0] : nullptr); }
    float* ipc_peer(int r, int slot) const { return reinterpret_cast<float*>(c->ipc_peers[(size_t)r].ptr[slot]); }

    /* ---- set-up: lanes, guards, rank states, the transport's buffers, the message maps ---- */
    int setup() {
        size_t win_floats = 0;
        for (int sl = 0; sl < J.n_steps; sl++) {
            Geo& g = geo[sl];
            g.asw = 2 * J.an[sl] + 1; g.Aw = g.asw * g.asw; g.nHW = J.P[sl]->nSim + J.P[sl]->nDisp;
            g.wb = W + 2 * g.nHW; g.hb = H + 2 * g.nHW; g.imgb = (size_t)C * g.wb * g.hb;
            win_floats = std::max(win_floats, g.Aw * g.imgb);
        }
        const bool any_step2 = J.step[0] == 2 || (two && J.step[1] == 2);
        /* lanes the schedule actually uses (a 3x3 light field is one window: no extra lane, no extra buffers) */
        int lanes_used = 1;
        for (const plan::Node& nd : G.nodes) lanes_used = std::max(lanes_used, nd.lane + 1);
        const int lanes_per_rank = emulate ? 1 : lanes_used;
        const size_t need_ctx = emulate ? (size_t)nranks - 1 : (size_t)lanes_used - 1;
        while (c->lanes.size() < need_ctx) {
            std::string e;
            lfbm5d_ctx* x = new_ctx(c->device, e);
            if (!x) return fail(c, "lane context: " + e);
            x->opt = c->opt; x->corr = c->corr;
            c->lanes.push_back(x);
        }
        ipc = c->ipc && nranks > 1 && !emulate;
        abort_guard.armed = nranks > 1 && !emulate && !ipc;
        ipc_guard.armed = ipc;
        drain_guard.armed = nranks == 1 || emulate || ipc;
        message = emulate ? &GraphRun::message_emulated : ipc ? &GraphRun::message_ipc : &GraphRun::message_rccl;

        states.resize(emulate ? (size_t)nranks : 1);
        /* the streamed host seam runs on one rank (several ranks: the caller uploads first and downloads at the end) */
        const HostIO* const io = (nranks == 1 && !emulate) ? J.io : nullptr;
        if (ipc && G.xfers.size() > kIpcMaxMsgs) return fail(c, "ipc transport: too many messages");
        if (ipc) c->ipc_epoch += 1;
        if (two) for (unsigned st = 0; st < asize; st++) if (h_mask[st] && G.last_touch[0][st] < 0) untouched.push_back(st);
        if (!io && input_as_basic(c, J, untouched, J.d_basic, img, s)) return 1;   /* (streamed: per SAI behind its upload) */
        hipEvent_t ev_setup = get_event(c);
        HIPCK(c, hipEventRecord(ev_setup, s));   /* the caller's colour transforms and zeroed sums */
        if (io) {   /* the seam's streams; which window makes which SAIs' outputs final */
            seam.io = io; seam.basic_in = !two && J.step[0] == 2;
            seam.up.assign(asize, 0); seam.ev_up.assign(asize, nullptr); seam.outs.assign(NN, {}); seam.ev_out.assign(NN, nullptr);
            if (!c->io_in) HIPCK(c, hipStreamCreateWithFlags(&c->io_in, hipStreamNonBlocking));
            if (!c->io_out) HIPCK(c, hipStreamCreateWithFlags(&c->io_out, hipStreamNonBlocking));
            HIPCK(c, hipStreamWaitEvent(c->io_in, ev_setup, 0));
            for (unsigned st = 0; st < asize; st++)
                if (h_mask[st] && G.last_touch[Ls][st] >= 0) seam.outs[(size_t)G.last_touch[Ls][st]].push_back(st);
        }
        for (size_t r = 0; r < states.size(); r++) {
            RankState& S = states[r];
            S.rank = emulate ? (int)r : c->rank;
            S.x = r == 0 ? c : c->lanes[r - 1];
            for (int sl = 0; sl < 2; sl++) { S.g_num[sl] = J.g_num[sl]; S.g_den[sl] = J.g_den[sl]; }
            S.basic = J.d_basic;
            if (r > 0) {   /* an emulated rank keeps light-field sums (and a basic estimate) of its own, like a real one */
                if (zeroed_sums(c, S.x, J.n_steps, asize * img, S.x->stream, S.g_num, S.g_den)) return 1;
                if (two) {
                    HIPCK(c, S.x->e_basic.reserve(asize * img * sizeof(float)));
                    S.basic = S.x->e_basic.as<float>();
                    HIPCK(c, hipStreamWaitEvent(S.x->stream, ev_setup, 0));
                }
                if (input_as_basic(c, J, untouched, S.basic, img, S.x->stream)) return 1;
            }
            S.lanes.resize((size_t)lanes_per_rank);
            for (int l = 0; l < lanes_per_rank; l++) {
                lfbm5d_ctx* lx = emulate ? S.x : (l == 0 ? c : c->lanes[(size_t)l - 1]);
                if (lane_buffers(c, lx, win_floats, any_step2, !direct, asize, S.lanes[(size_t)l])) return 1;
                if (lx != c) HIPCK(c, hipStreamWaitEvent(lx->stream, ev_setup, 0));
            }
            if (nranks > 1)
                for (int ch = 0; ch < 2; ch++) {
                    if (!S.x->cs[ch]) HIPCK(c, hipStreamCreateWithFlags(&S.x->cs[ch], hipStreamNonBlocking));
                    HIPCK(c, hipStreamWaitEvent(S.x->cs[ch], ev_setup, 0));
                    if (r > 0) {   /* an emulated rank's own buffers are prepared on its stream */
                        hipEvent_t e = get_event(c);
                        HIPCK(c, hipEventRecord(e, S.x->stream));
                        HIPCK(c, hipStreamWaitEvent(S.x->cs[ch], e, 0));
                    }
                }
        }
        if (ipc) {
            /* what peers read lives in buffers of this context (the caller's may be slices of an allocator's blocks, which have no IPC
             * handle of their own): the basic estimate of a two-step job, the outputs formed at the end */
            RankState& S0 = states[0];
            if (two) {
                HIPCK(c, c->e_basic.reserve(asize * img * sizeof(float)));
                S0.basic = c->e_basic.as<float>();
                if (input_as_basic(c, J, untouched, S0.basic, img, s)) return 1;
            }
            HIPCK(c, c->ipc_out.reserve(asize * img * sizeof(float)));
            HIPCK(c, hipMemsetAsync(c->ipc_flags.as<unsigned>() + 2 * kIpcMaxMsgs, 0, sizeof(unsigned), s));
            HIPCK(c, hipStreamSynchronize(s));
            void* const mine_bufs[7] = {c->ipc_flags.p, S0.g_num[0], two ? (void*)S0.g_num[1] : nullptr, S0.g_den[0], two ? (void*)S0.g_den[1] : nullptr,
                                        two ? (void*)S0.basic : nullptr, c->ipc_out.p};
            if (ipc_exchange_handles(c, mine_bufs)) return 1;
        }
        ipc_own = c->ipc_flags.as<unsigned>();
        if (c->h_counts_cap < NN * kWinCounters) {
            if (c->h_counts) (void)hipHostFree(c->h_counts);
            c->h_counts = nullptr; c->h_counts_cap = 0;
            HIPCK(c, hipHostMalloc((void**)&c->h_counts, NN * kWinCounters * sizeof(unsigned)));
            c->h_counts_cap = NN * kWinCounters;
        }
        done.assign(NN, nullptr); arrived.assign(G.xfers.size(), nullptr);
        n_in.assign(NN, 0);
        sum_xfer.resize(NN);
        for (size_t n = 0; n < NN; n++) sum_xfer[n].assign(G.nodes[n].sai.size(), -1);
        basic_xfer.resize(two ? (size_t)nranks : 0);
        for (auto& v : basic_xfer) v.assign(asize, -1);
        for (size_t i = 0; i < G.xfers.size(); i++) {
            const plan::Xfer& X = G.xfers[i];
            if (X.kind == 0) {
                const plan::Node& pn = G.nodes[X.from];
                sum_xfer[X.from][(size_t)(std::find(pn.sai.begin(), pn.sai.end(), X.sai) - pn.sai.begin())] = (int)i;
            } else basic_xfer[(size_t)X.to_rank][X.sai] = (int)i;
        }
        return 0;
    }

    /* ---- window n of the issue order, owned by rank S that lives here: its waits, then one angular window around SAI (ps, pt),
     * bm5d.cpp:215-402 -- padding, the centre pass, its coverage count, and (optimistic completion) the window's sums back into the
     * light field ---- */
    int enqueue_window(unsigned n, RankState* S) {
        const plan::Node& nd = G.nodes[n];
        const int sl = nd.s, r = nd.rank;
        const Geo& g = geo[sl];
        const Lane& Lw = S->lanes[(size_t)nd.lane];
        hipStream_t ls = Lw.x->stream;
        auto wait_node = [&](int p) -> int {   /* a node of this rank: same lane = stream order */
            if (G.nodes[(size_t)p].lane != nd.lane) HIPCK(c, hipStreamWaitEvent(ls, done[(size_t)p], 0));
            return 0;
        };
        if (seam.io)   /* the SAIs this window is the first to use: into HBM now, the window waits for them on its lane */
            for (unsigned st : nd.sai)
                if (!seam.up[st]) {
                    if (seam.upload(st)) return 1;
                    HIPCK(c, hipStreamWaitEvent(ls, seam.ev_up[st], 0));
                }
        for (size_t i = 0; i < nd.sai.size(); i++) {
            const int pw = nd.prev[i];
            if (pw >= 0) {
                if (G.nodes[(size_t)pw].rank == r) { if (wait_node(pw)) return 1; }
                else {
                    const plan::Node& pn = G.nodes[(size_t)pw];
                    const size_t j = (size_t)(std::find(pn.sai.begin(), pn.sai.end(), nd.sai[i]) - pn.sai.begin());
                    HIPCK(c, hipStreamWaitEvent(ls, arrived[(size_t)sum_xfer[(size_t)pw][j]], 0));
                }
            }
            if (two && sl == 1) {   /* the SAI's basic estimate: finalised behind the first step's last window on it */
                const int f = G.last_touch[0][nd.sai[i]];
                if (f >= 0) {
                    if (G.nodes[(size_t)f].rank == r) { if (wait_node(f)) return 1; }
                    else HIPCK(c, hipStreamWaitEvent(ls, arrived[(size_t)basic_xfer[(size_t)r][nd.sai[i]]], 0));
                }
            }
        }
        const plan::Window win = plan::window_at(grid, nd.ps, nd.pt, J.an[sl]);
        const MaskedWindow m = mask_window(win, h_mask);
        n_in[n] = m.n_in;
        const bool wien = J.step[sl] == 2;
        /* (the estimate buffer as pass_impl lays it out: slack on both sides for the table kernel's row loads) */
        HIPCK(c, Lw.x->est.reserve((kEstLead + g.Aw * (size_t)g.wb * g.hb + 256) * sizeof(float)));
        HIPCK(c, launch_window_begin(ls, J.noisy[sl], wien ? S->basic : nullptr, S->g_num[sl], S->g_den[sl], img, Lw.w_noisy, Lw.w_basic, Lw.w_num,
                                     Lw.w_den, Lw.x->est.as<float>() + kEstLead, g.imgb, m.sl, W, H, C, g.nHW, Lw.d_small));
        lfbm5d_params Pw = *J.P[sl];
        Pw.tau_4D = nd.tau4;
        Pw.sigma = window_sigma(c, J.P[sl], win, h_mask);
        Lw.x->gslot = sl;
        Lw.x->est_ready = true;
        if (direct) { Lw.x->direct.on = true; Lw.x->direct.num = S->g_num[sl]; Lw.x->direct.den = S->g_den[sl]; Lw.x->direct.lf_stride = img; Lw.x->direct.sai = m.sl; }
        const int prc = pass_impl(Lw.x, J.step[sl], &Pw, g.asw, g.asw, g.wb, g.hb, C, Lw.w_noisy, wien ? Lw.w_basic : nullptr, Lw.w_num, Lw.w_den,
                                  m.mask_w.data(), m.proc_w.data(), win.cst_w, win.cst_w);
        Lw.x->gslot = 0;
        if (prc) { if (Lw.x != c) c->err = Lw.x->err; return 1; }
        /* the window's sums back into the light field (direct form: they are there already), and the coverage count of the pass
         * (LF_denoised_percent, utilities_LF.cpp:967-995) -> pinned memory */
        HIPCK(c, launch_window_end(ls, S->g_num[sl], S->g_den[sl], img, Lw.w_num, Lw.w_den, g.imgb, m.sl, W, H, C, g.nHW, J.P[sl]->k, Lw.d_small));
        HIPCK(c, hipMemcpyAsync(c->h_counts + (size_t)n * kWinCounters, Lw.d_small, kWinCounters * sizeof(unsigned), hipMemcpyDeviceToHost, ls));
        if (!nd.fin.empty()) {   /* two-step jobs: these SAIs' first-step sums are final -> their basic estimate as the second step reads it */
            SaiList fl; fl.n = 0;
            for (unsigned st : nd.fin) fl.st[fl.n++] = st;
            const bool colour = C == 3 && J.P[0]->color_space != LFBM5D_RGB;
            HIPCK(c, launch_finalize_multi(ls, S->g_num[0], S->g_den[0], J.noisy[0], S->basic, img, fl, J.P[0]->color_space, W * H, colour ? 1 : 0));
        }
        done[n] = get_event(c);
        HIPCK(c, hipEventRecord(done[n], ls));
        if (seam.io && !seam.outs[n].empty()) {   /* the SAIs nobody touches after this window: their outputs */
            if (seam.form_outputs(ls, seam.outs[n])) return 1;
            seam.ev_out[n] = get_event(c);
            HIPCK(c, hipEventRecord(seam.ev_out[n], ls));
            seam.out_nodes.push_back(n);
        }
        if (Lw.x != c) c->stats.lane_windows += 1;
        return 0;
    }

    /* ---- the messages window n's result feeds, in the order every rank issues them.  Message i of the issue order moves num
     * and den of SAI X.sai (kind 0), or its basic estimate (kind 1), of step slot xsl from rank ra (Sa, where that rank lives
     * here) to rank X.to_rank (Sb) on channel ch; off = the SAI's offset in a light field ---- */
    int post_messages(unsigned n) {
        for (; xi < G.xfers.size() && G.xfers[xi].from == n; xi++) {
            const plan::Xfer& X = G.xfers[xi];
            const int ra = G.nodes[n].rank;
            RankState* Sa = local(ra); RankState* Sb = local(X.to_rank);
            if (!Sa && !Sb) continue;   /* between two other ranks */
            /* one channel when the second communicator could not be created: two streams on one communicator would break the
             * common issue order the exchange relies on */
            const int ch = (emulate || c->comm2 || ipc) ? X.channel : 0;
            if ((this->*message)(xi, X, G.nodes[n].s, ra, ch, Sa, Sb, (size_t)X.sai * img)) return 1;
            n_msgs++;
        }
        return 0;
    }
    /* emulated ranks: both ends live here, the message is a device copy between the two ranks' buffers */
    int message_emulated(size_t i, const plan::Xfer& X, int xsl, int ra, int ch, RankState* Sa, RankState* Sb, size_t off) {
        hipStream_t xs = Sb->x->cs[ch];
        HIPCK(c, hipStreamWaitEvent(xs, done[X.from], 0));
        if (X.kind == 0) {
            HIPCK(c, hipMemcpyAsync(Sb->g_num[xsl] + off, Sa->g_num[xsl] + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
            HIPCK(c, hipMemcpyAsync(Sb->g_den[xsl] + off, Sa->g_den[xsl] + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
        } else
            HIPCK(c, hipMemcpyAsync(Sb->basic + off, Sa->basic + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
        arrived[i] = get_event(c);
        HIPCK(c, hipEventRecord(arrived[i], xs));
        return 0;
    }
    /* the same message between two processes on one GPU: the sender publishes "ready" behind its window, the receiver's
     * exchange stream waits for the word, copies the SAI out of the sender's (mapped) buffers and publishes "taken" */
    int message_ipc(size_t i, const plan::Xfer& X, int xsl, int ra, int ch, RankState* Sa, RankState* Sb, size_t off) {
        hipStream_t xs = c->cs[ch];
        const unsigned ep = c->ipc_epoch;
        if (Sa) {
            HIPCK(c, hipStreamWaitEvent(xs, done[X.from], 0));
            HIPCK(c, launch_ipc_set(xs, ipc_own + i, ep));
            ipc_sent.push_back(i);
        } else {
            const unsigned* const pf = reinterpret_cast<const unsigned*>(c->ipc_peers[(size_t)ra].ptr[0]);
            HIPCK(c, launch_ipc_wait(xs, pf + i, ep, ipc_own + 2 * kIpcMaxMsgs, c->ipc_timeout_s));
            if (X.kind == 0) {
                HIPCK(c, hipMemcpyAsync(Sb->g_num[xsl] + off, ipc_peer(ra, 1 + xsl) + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
                HIPCK(c, hipMemcpyAsync(Sb->g_den[xsl] + off, ipc_peer(ra, 3 + xsl) + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
            } else
                HIPCK(c, hipMemcpyAsync(Sb->basic + off, ipc_peer(ra, 5) + off, img * sizeof(float), hipMemcpyDeviceToDevice, xs));
            HIPCK(c, launch_ipc_set(xs, ipc_own + kIpcMaxMsgs + i, ep));
            arrived[i] = get_event(c);
            HIPCK(c, hipEventRecord(arrived[i], xs));
        }
        return 0;
    }
    /* real ranks: one RCCL group per message, the sender's behind its window's event, the receiver's followed by `arrived` */
    int message_rccl(size_t i, const plan::Xfer& X, int xsl, int ra, int ch, RankState* Sa, RankState* Sb, size_t off) {
        const int rb = X.to_rank;
        hipStream_t xs = c->cs[ch];
        RankState* Sm = Sa ? Sa : Sb;
        if (Sa) HIPCK(c, hipStreamWaitEvent(xs, done[X.from], 0));
        bool ok = ncclGroupStart() == ncclSuccess;
        if (X.kind == 0) {
            if (Sa) ok = ok && ncclSend(Sm->g_num[xsl] + off, img, ncclFloat, rb, comms[ch], xs) == ncclSuccess
                            && ncclSend(Sm->g_den[xsl] + off, img, ncclFloat, rb, comms[ch], xs) == ncclSuccess;
            else    ok = ok && ncclRecv(Sm->g_num[xsl] + off, img, ncclFloat, ra, comms[ch], xs) == ncclSuccess
                            && ncclRecv(Sm->g_den[xsl] + off, img, ncclFloat, ra, comms[ch], xs) == ncclSuccess;
        } else {
            if (Sa) ok = ok && ncclSend(Sm->basic + off, img, ncclFloat, rb, comms[ch], xs) == ncclSuccess;
            else    ok = ok && ncclRecv(Sm->basic + off, img, ncclFloat, ra, comms[ch], xs) == ncclSuccess;
        }
        ok = ncclGroupEnd() == ncclSuccess && ok;
        if (!ok) return fail(c, "RCCL send / recv of a window's SAI failed");
        if (Sb) { arrived[i] = get_event(c); HIPCK(c, hipEventRecord(arrived[i], xs)); }
        return 0;
    }

    /* ---- streamed host seam, downloads.  Everything is enqueued; this thread now delivers every SAI's outputs as the window
     * that makes them final completes (pageable destinations: the copies block, which is all this thread has left to do) ---- */
    int deliver_streamed_outputs() {
        for (unsigned st = 0; st < asize; st++)   /* SAIs no window uses (LFBM5D_MAX_WINDOWS): still part of the result */
            if (h_mask[st] && !seam.up[st] && seam.upload(st)) return 1;
        for (unsigned n : seam.out_nodes) {
            HIPCK(c, hipEventSynchronize(seam.ev_out[n]));
            for (unsigned st : seam.outs[n]) if (seam.download(st)) return 1;
        }
        HIPCK(c, hipStreamSynchronize(c->io_in));
        /* SAIs without a window in the result's step keep that step's input (bm5d.cpp:405 / :1106 with den == 0): formed once every
         * window is done (a two-step job may still finalise their basic estimate late) */
        std::vector<unsigned> rest;
        for (unsigned st = 0; st < asize; st++) if (h_mask[st] && G.last_touch[Ls][st] < 0) rest.push_back(st);
        if (!rest.empty()) {
            for (RankState& S : states) for (Lane& Lq : S.lanes) HIPCK(c, hipStreamSynchronize(Lq.x->stream));
            if (seam.form_outputs(c->io_in, rest)) return 1;
            HIPCK(c, hipStreamSynchronize(c->io_in));
            for (unsigned st : rest) if (seam.download(st)) return 1;
        }
        HIPCK(c, hipStreamSynchronize(c->io_out));
        return 0;
    }

    /* ---- drain: every lane, every exchange stream ---- */
    int drain() {
        for (size_t i : ipc_sent) {   /* IPC: a send is complete when the peer has taken the SAI (what an RCCL send's completion means) */
            const plan::Xfer& X = G.xfers[i];
            const unsigned* const pf = reinterpret_cast<const unsigned*>(c->ipc_peers[(size_t)X.to_rank].ptr[0]);
            HIPCK(c, launch_ipc_wait(c->cs[X.channel], pf + kIpcMaxMsgs + i, c->ipc_epoch, ipc_own + 2 * kIpcMaxMsgs, c->ipc_timeout_s));
        }
        for (RankState& S : states) {
            for (Lane& Lq : S.lanes) HIPCK(c, hipStreamSynchronize(Lq.x->stream));
            for (int ch = 0; ch < 2; ch++) if (S.x->cs[ch]) HIPCK(c, hipStreamSynchronize(S.x->cs[ch]));
        }
        HIPCK(c, hipStreamSynchronize(s));
        if (ipc) {
            unsigned err = 0;
            HIPCK(c, hipMemcpy(&err, ipc_own + 2 * kIpcMaxMsgs, sizeof(unsigned), hipMemcpyDeviceToHost));
            if (err) return fail(c, "ipc transport: a peer did not deliver / take a message within the watchdog");
        }
        drain_guard.armed = false;
        return 0;
    }

    /* ---- did every window of this rank complete with its centre pass?  The lanes' counters are folded; all ranks agree on the
     * answer before any of them goes on to a collective ---- */
    int vote_complete() {
        for (size_t n = 0; n < NN; n++) {
            if (!n_in[n]) continue;
            const int sl = G.nodes[n].s;
            unsigned covered = 0;
            for (unsigned q = 0; q < kWinCounters; q++) covered += c->h_counts[n * kWinCounters + q];
            const float pct = (float)covered * 100.0f / (float)n_in[n] / (float)(H - J.P[sl]->k + 1) / (float)(W - J.P[sl]->k + 1);
            if (!(pct >= 100.0f)) complete = 0;
        }
        if (c->opt->force_redo && nranks == 1) complete = 0;   /* test hook: exercise the sequential redo */
        /* fold the other lanes' / emulated ranks' counters and event times into this context */
        auto fold_all = [&](lfbm5d_ctx* x) -> int {
            drain_events(x);
            for (int sl = 0; sl < J.n_steps; sl++)
                if (fold_counters(x, J.P[sl], geo[sl].Aw, C, J.step[sl], sl)) { c->err = x->err; return 1; }
            return 0;
        };
        for (lfbm5d_ctx* x : c->lanes) {
            if (x->pending.empty() && x->stats.passes == 0) continue;
            if (fold_all(x)) return 1;
            add_stats(c->stats, x->stats);
            std::memset(&x->stats, 0, sizeof(x->stats));
        }
        if (two && fold_all(c)) return 1;   /* (single steps: run_step folds slot 0 of this context itself) */
        if (ipc) {
            std::vector<int> all;
            if (ipc_allgather(c, "complete", complete, all)) return 1;
            for (int v : all) complete = std::min(complete, v);
        } else
        if (nranks > 1 && !emulate) {   /* all ranks must agree before the collective of exchange_estimates */
            HIPCK(c, c->small.reserve((asize + 8 + kWinCounters) * sizeof(unsigned)));
            int* d_flag = reinterpret_cast<int*>(c->small.as<unsigned>());
            HIPCK(c, hipMemcpyAsync(d_flag, &complete, sizeof(int), hipMemcpyHostToDevice, s));
            if (ncclAllReduce(d_flag, d_flag, 1, ncclInt, ncclMin, c->comm, s) != ncclSuccess) return fail(c, "ncclAllReduce(flag) failed");
            HIPCK(c, hipMemcpyAsync(&complete, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCK(c, hipStreamSynchronize(s));
        }
        abort_guard.armed = false;   /* every exchange of the graph has completed; what follows are plain collectives */
        return 0;
    }

    /* ---- several ranks: every SAI's final sums live on the rank of the last window that touched it: that rank forms the SAI's
     * estimate (bm5d.cpp:405 / :1106), then the estimates are exchanged so that every rank ends with the whole result; two-step
     * jobs do the same with the basic estimates, which live where they were finalised ---- */
    int owner_of(int sl, unsigned st) const { return G.last_touch[sl][st] >= 0 ? G.nodes[(size_t)G.last_touch[sl][st]].rank : -1; }
    int exchange_estimates() {
        std::vector<unsigned> own(asize);
        for (RankState& S : states) {
            const float* sub = J.step[Ls] == 1 ? J.noisy[Ls] : S.basic;
            for (unsigned st = 0; st < asize; st++) own[st] = (h_mask[st] && owner_of(Ls, st) == S.rank) ? 1u : 0u;
            HIPCK(c, S.x->d_own.reserve(asize * sizeof(unsigned)));
            HIPCK(c, hipMemcpyAsync(S.x->d_own.p, own.data(), asize * sizeof(unsigned), hipMemcpyHostToDevice, s));
            HIPCK(c, launch_estimate_lf(s, S.g_num[Ls], S.g_den[Ls], sub, ipc ? c->ipc_out.as<float>() : J.d_out, img, asize, S.x->d_own.as<unsigned>()));
            HIPCK(c, hipStreamSynchronize(s));   /* own is reused */
            if (two && emulate && S.x != c)      /* the basic estimates this emulated rank finalised: what the broadcast moves between real ranks */
                for (unsigned st = 0; st < asize; st++)
                    if (h_mask[st] && owner_of(0, st) == S.rank)
                        HIPCK(c, hipMemcpyAsync(J.d_basic + (size_t)st * img, S.basic + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        if (ipc) { if (exchange_ipc()) return 1; }
        else if (!emulate && exchange_rccl()) return 1;
        /* SAIs no window touched (LFBM5D_MAX_WINDOWS) keep the step's input, like the single-rank estimate */
        for (unsigned st = 0; st < asize; st++) own[st] = (h_mask[st] && G.last_touch[Ls][st] < 0) ? 1u : 0u;
        if (std::count(own.begin(), own.end(), 1u)) {
            HIPCK(c, hipMemcpyAsync(c->d_own.p, own.data(), asize * sizeof(unsigned), hipMemcpyHostToDevice, s));
            HIPCK(c, launch_estimate_lf(s, J.g_num[Ls], J.g_den[Ls], J.step[Ls] == 1 ? J.noisy[Ls] : J.d_basic, J.d_out, img, asize, c->d_own.as<unsigned>()));
            HIPCK(c, hipStreamSynchronize(s));
        }
        return 0;
    }
    /* every rank's outputs are formed: pull each SAI from the rank that holds it, then leave together */
    int exchange_ipc() {
        std::vector<int> all;
        if (ipc_allgather(c, "formed", 1, all)) return 1;
        for (unsigned st = 0; st < asize; st++) {
            if (!h_mask[st]) continue;
            const int ro = owner_of(Ls, st), rb = owner_of(0, st);
            if (ro >= 0) {
                const float* src = ro == c->rank ? c->ipc_out.as<float>() : ipc_peer(ro, 6);
                HIPCK(c, hipMemcpyAsync(J.d_out + (size_t)st * img, src + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
            if (two) {   /* (no first-step window: this rank's own copy of the step's input) */
                const float* src = rb < 0 || rb == c->rank ? states[0].basic : ipc_peer(rb, 5);
                HIPCK(c, hipMemcpyAsync(J.d_basic + (size_t)st * img, src + (size_t)st * img, img * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
        }
        HIPCK(c, hipStreamSynchronize(s));
        return ipc_allgather(c, "pulled", 1, all);
    }
    /* one group of broadcasts, every SAI from its owner */
    int exchange_rccl() {
        CommTimer timer{c, s};
        HIPCK(c, timer.begin());
        bool ok = ncclGroupStart() == ncclSuccess;
        for (unsigned st = 0; st < asize && ok; st++) {
            if (!h_mask[st]) continue;
            if (owner_of(Ls, st) >= 0)
                ok = ncclBroadcast(J.d_out + (size_t)st * img, J.d_out + (size_t)st * img, img, ncclFloat, owner_of(Ls, st), c->comm, s) == ncclSuccess;
            if (ok && two && owner_of(0, st) >= 0)
                ok = ncclBroadcast(J.d_basic + (size_t)st * img, J.d_basic + (size_t)st * img, img, ncclFloat, owner_of(0, st), c->comm, s) == ncclSuccess;
        }
        ok = ncclGroupEnd() == ncclSuccess && ok;
        if (!ok) return fail(c, "ncclBroadcast of the estimates failed");
        HIPCK(c, timer.end());
        HIPCK(c, hipStreamSynchronize(s));
        return 0;
    }
};

} /* namespace */

int run_graph(lfbm5d_ctx* c, const GraphJob& J, const plan::Graph& G, const unsigned* h_mask, const plan::Grid& grid,
              unsigned W, unsigned H, unsigned C, int nranks, bool emulate, int* complete_out) {
    *complete_out = 1;
    GraphRun R{c, J, G, h_mask, grid, W, H, C, nranks, emulate};
    if (R.setup()) return 1;
    for (unsigned n : G.order) {   /* every rank walks the whole issue order: its own windows, the messages it takes part in */
        RankState* S = R.local(G.nodes[n].rank);
        if (S && R.enqueue_window(n, S)) return 1;
        if (R.post_messages(n)) return 1;
    }
    if (R.seam.io && R.deliver_streamed_outputs()) return 1;
    if (R.drain()) return 1;
    if (R.vote_complete()) return 1;
    *complete_out = R.complete;
    if (!R.complete) { R.ipc_guard.armed = false; return 0; }   /* (agreed on by all ranks) */
    for (size_t n = 0; n < R.NN; n++) if (R.n_in[n]) c->stats.windows += 1;
    c->stats.messages += R.n_msgs;
    if (nranks > 1 && R.exchange_estimates()) return 1;
    R.ipc_guard.armed = false;
    return 0;
}

} /* namespace lfbm5d_host */
