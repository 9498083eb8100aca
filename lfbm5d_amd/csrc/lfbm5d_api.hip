/*
 * lfbm5d_api.hip -- the C-ABI of include/lfbm5d.h: context and options, communicators, the device and host entry points of
 * the outer seam (lfbm5d_step* / lfbm5d_denoise_* -> lfbm5d_steps.hip), the inner seam (lfbm5d_pass_device -> lfbm5d_pass.hip),
 * per-SAI BM3D, inspection of the last pass.  The host side's other translation units: lfbm5d_ctx.h.
 */
#include "lfbm5d_graph.h"

using namespace lfbm5d_host;
using lfbm5d::plan::plan_windows;

namespace { std::string g_create_error; }

/* ============================================================================================ */
/* C API                                                                                        */
/* ============================================================================================ */
extern "C" {

int lfbm5d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lfbm5d_create(lfbm5d_ctx** out, int device) {
    if (!out) return 1;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = "no HIP device available (liblfbm5d_hip has no CPU fallback)";
        return 1;
    }
    if (device < 0 || device >= n) { g_create_error = "device index out of range"; return 1; }
    if ((e = hipSetDevice(device)) != hipSuccess) { g_create_error = hipGetErrorString(e); return 1; }
    lfbm5d_ctx* c = new_ctx(device, g_create_error);
    if (c) options_from_env(c->opt_store);   /* the library's only read of the environment (lfbm5d_options.h) */
    if (!c) return 1;
    *out = c;
    return 0;
}

int lfbm5d_set_option(lfbm5d_ctx* c, const char* key, const char* value) {
    if (!c || !key) return 1;
    if (!option_set(c->opt_store, key, value)) return fail(c, std::string("unknown option: ") + key);
    return 0;
}
int lfbm5d_get_option(lfbm5d_ctx* c, const char* key, char* value, unsigned long long size) {
    if (!c || !key || !value || size == 0) return 1;
    std::string v;
    if (!option_get(c->opt_store, key, v)) return fail(c, std::string("unknown option: ") + key);
    std::snprintf(value, (size_t)size, "%s", v.c_str());
    return 0;
}

void lfbm5d_destroy(lfbm5d_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (lfbm5d_ctx* x : c->lanes) lfbm5d_destroy(x);
    c->lanes.clear();
    if (c->h_counts) (void)hipHostFree(c->h_counts);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (lfbm5d_ctx::IpcPeer& P : c->ipc_peers) for (void* q : P.ptr) if (q) (void)hipIpcCloseMemHandle(q);
    c->ipc_flags.release(); c->ipc_out.release(); c->pristine.release(); c->pristine_b.release();
    if (c->io_in) (void)hipStreamDestroy(c->io_in);
    if (c->io_out) (void)hipStreamDestroy(c->io_out);
    if (c->team_comm2) ncclCommDestroy(c->team_comm2);
    if (c->team_comm) ncclCommDestroy(c->team_comm);
    if (c->comm2) ncclCommDestroy(c->comm2);
    if (c->comm) ncclCommDestroy(c->comm);
    for (int i = 0; i < 2; i++) if (c->cs[i]) (void)hipStreamDestroy(c->cs[i]);
    for (GeomCache& g : c->gc) { g.refs.release(); g.rslot.release(); g.tb.release(); g.scan_wgs.release(); }
    DevBuf* bufs[] = {&c->est, &c->g_num2, &c->g_den2, &c->n2, &c->e_basic, &c->refmap, &c->scores, &c->tables, &c->self_idx, &c->self_cnt, &c->best,
                      &c->t_noisy, &c->t_basic, &c->t_tnum, &c->t_tden, &c->und_num, &c->und_den, &c->sub_flags, &c->sub_cnt, &c->shape, &c->filt, &c->wgt, &c->aggpos, &c->gpos, &c->gofs, &c->gok, &c->sa_list, &c->gshape, &c->band_noisy, &c->band_basic, &c->band_out, &c->band_src, &c->band_pack, &c->band_gather, &c->counters, &c->small, &c->t_num, &c->t_den, &c->d_mask, &c->g_num, &c->g_den, &c->w_noisy,
                      &c->w_basic, &c->w_num, &c->w_den, &c->h2d_noisy, &c->h2d_basic, &c->h2d_out, &c->d_own, &c->gscratch, &c->scan_lcol};
    for (DevBuf* b : bufs) b->release();
    c->side.sai.release(); c->side.lf.release();
    c->noise.part.release(); c->noise.cells.release(); c->noise.m.release(); c->noise.pool.release();
    c->sr.tab.release(); c->sr.lo.release();
    c->quality.part.release(); c->quality.out.release();
    c->pg.stats.release();
    c->clip.stats.release();
    c->pgclip.tables.release();
    c->imp.stats.release(); c->imp.flags.release();
    c->inp.stats.release(); c->inp.state[0].release(); c->inp.state[1].release(); c->inp.flags.release();
    c->view.table.release(); c->view.stats.release(); c->view.disp.release(); c->view.set.release();
    c->consist.table.release(); c->consist.stats.release(); c->consist.pred.release(); c->consist.disp.release(); c->consist.flags.release();
    c->dbg_agg.tb.release();
    c->photo.table.release(); c->photo.sweep_table.release(); c->photo.stats.release(); c->photo.pred.release(); c->photo.disp.release(); c->photo.x.release();
    c->repair.valid.release(); c->repair.mid.release(); c->repair.rem.release(); c->repair.tiles.release(); c->repair.table.release();
    c->repair.stats.release(); c->repair.codes.release(); c->repair.host.release();
    c->corr_store.dev.release(); c->corrm.lags.release(); c->corrm.score.release(); c->corrm.part.release();
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->h_small) (void)hipHostFree(c->h_small);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* lfbm5d_last_error(const lfbm5d_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
void lfbm5d_reset_stats(lfbm5d_ctx* c) { if (c) std::memset(&c->stats, 0, sizeof(c->stats)); }
void lfbm5d_get_stats(const lfbm5d_ctx* c, lfbm5d_stats* out) { if (c && out) *out = c->stats; }
void* lfbm5d_stream(lfbm5d_ctx* c) { return c ? (void*)c->stream : nullptr; }

void lfbm5d_shard_rows(unsigned n_rows, int rank, int world, unsigned* begin, unsigned* end) {
    if (world < 1) world = 1;
    if (rank < 0) rank = 0;
    *begin = (unsigned)(((unsigned long long)n_rows * (unsigned)rank) / (unsigned)world);
    *end = (unsigned)(((unsigned long long)n_rows * (unsigned)(rank + 1)) / (unsigned)world);
}

int lfbm5d_auto_bands(unsigned awidth, unsigned aheight, unsigned height, unsigned halo, int world) {
    return auto_bands(awidth, aheight, height, halo ? halo : 40u, world);
}

int lfbm5d_comm_unique_id(void* id_out) {
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) <= LFBM5D_UNIQUE_ID_BYTES, "unique id size");
    if (ncclGetUniqueId(&id) != ncclSuccess) return 1;
    std::memset(id_out, 0, LFBM5D_UNIQUE_ID_BYTES);
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

int lfbm5d_comm_init(lfbm5d_ctx* c, const void* idb, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return 1;
    (void)hipSetDevice(c->device);
    /* a second call replaces the communicators (after a job that tore them down, or to change the ranks) */
    if (c->team_comm2) { (void)ncclCommDestroy(c->team_comm2); c->team_comm2 = nullptr; }
    if (c->team_comm) { (void)ncclCommDestroy(c->team_comm); c->team_comm = nullptr; }
    c->team_S = 0;
    if (c->comm2) { (void)ncclCommDestroy(c->comm2); c->comm2 = nullptr; }
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    c->rank = rank; c->world = world;
    if (world == 1) return 0;
    ncclUniqueId id;
    std::memcpy(&id, idb, sizeof(id));
    if (ncclCommInitRank(&c->comm, world, id, rank) != ncclSuccess) return fail(c, "ncclCommInitRank failed");
    /* second channel of the window-graph exchange: same ranks, independent progress.  Optional (one channel is only slower) */
    if (ncclCommSplit(c->comm, 0, rank, &c->comm2, nullptr) != ncclSuccess) c->comm2 = nullptr;
    return 0;
}

int lfbm5d_comm_init_ipc(lfbm5d_ctx* c, int rank, int world, const char* rendezvous_dir, double timeout_s) {
    if (!c || world < 1 || rank < 0 || rank >= world || !rendezvous_dir) return 1;
    (void)hipSetDevice(c->device);
    c->rank = rank; c->world = world;
    if (world == 1) return 0;
    c->ipc = true; c->ipc_dir = rendezvous_dir; c->ipc_timeout_s = timeout_s > 0 ? timeout_s : 30.0; c->ipc_epoch = 0;
    HIPCK(c, c->ipc_flags.reserve((2 * kIpcMaxMsgs + 16) * sizeof(unsigned)));
    HIPCK(c, hipMemset(c->ipc_flags.p, 0, (2 * kIpcMaxMsgs + 16) * sizeof(unsigned)));
    c->ipc_peers.assign((size_t)world, lfbm5d_ctx::IpcPeer());
    for (lfbm5d_ctx::IpcPeer& P : c->ipc_peers) std::memset(&P, 0, sizeof(P));
    std::vector<int> all;   /* every rank is there (and has zeroed its gating words) before anybody's first job */
    return ipc_allgather(c, "init", 1, all);
}

int lfbm5d_plan_windows(unsigned awidth, unsigned aheight, unsigned an, unsigned ang_major, const unsigned* mask,
                        unsigned* out_sai, unsigned cap) {
    if (!mask || !awidth || !aheight || 2 * an + 1 > awidth || 2 * an + 1 > aheight) return -1;
    if (ang_major != LFBM5D_ROWMAJOR && ang_major != LFBM5D_COLMAJOR) return -1;
    std::vector<unsigned> plan;
    plan_windows(mask, plan::Grid{awidth, aheight, ang_major}, an, plan);
    for (size_t i = 0; i < plan.size() && i < cap && out_sai; i++) out_sai[i] = plan[i];
    return (int)plan.size();
}

int lfbm5d_plan_graph(unsigned awidth, unsigned aheight, unsigned an, unsigned ang_major, const unsigned* mask, int world, int lanes,
                      unsigned* out_rank, unsigned* out_lane, unsigned* out_start, unsigned cap) {
    if (!mask || !awidth || !aheight || 2 * an + 1 > awidth || 2 * an + 1 > aheight || world < 1 || lanes < 1) return -1;
    if (ang_major != LFBM5D_ROWMAJOR && ang_major != LFBM5D_COLMAJOR) return -1;
    plan::Graph G;
    const plan::StepDesc sd = {an, LFBM5D_SADCT, 1u};
    plan::build(mask, plan::Grid{awidth, aheight, ang_major}, &sd, 1, world, lanes, 0, G);
    for (size_t i = 0; i < G.nodes.size() && i < cap; i++) {
        if (out_rank) out_rank[i] = (unsigned)G.nodes[i].rank;
        if (out_lane) out_lane[i] = (unsigned)G.nodes[i].lane;
        if (out_start) out_start[i] = G.nodes[i].start;
    }
    return (int)G.nodes.size();
}

int lfbm5d_plan_messages(unsigned awidth, unsigned aheight, unsigned an, unsigned ang_major, const unsigned* mask, int world,
                         unsigned* out, unsigned cap) {
    if (!mask || !awidth || !aheight || 2 * an + 1 > awidth || 2 * an + 1 > aheight || world < 1) return -1;
    if (ang_major != LFBM5D_ROWMAJOR && ang_major != LFBM5D_COLMAJOR) return -1;
    plan::Graph G;
    const plan::StepDesc sd = {an, LFBM5D_SADCT, 1u};
    plan::build(mask, plan::Grid{awidth, aheight, ang_major}, &sd, 1, world, 1, 0, G);
    for (size_t i = 0; i < G.xfers.size() && i < cap && out; i++) {
        out[4 * i] = G.xfers[i].from; out[4 * i + 1] = (unsigned)G.xfers[i].to_node; out[4 * i + 2] = G.xfers[i].sai; out[4 * i + 3] = (unsigned)G.xfers[i].channel;
    }
    return (int)G.xfers.size();
}

int lfbm5d_plan_job(unsigned awidth, unsigned aheight, unsigned ang_major, const unsigned* mask, int n_steps, const unsigned* an,
                    const unsigned* cost, int world, int lanes, unsigned* out_nodes, unsigned node_cap, unsigned* out_msgs, unsigned msg_cap,
                    unsigned* out_counts) {
    if (!mask || !awidth || !aheight || !an || world < 1 || lanes < 1 || n_steps < 1 || n_steps > 2) return -1;
    if (ang_major != LFBM5D_ROWMAJOR && ang_major != LFBM5D_COLMAJOR) return -1;
    plan::StepDesc sd[2];
    for (int i = 0; i < n_steps; i++) {
        if (2 * an[i] + 1 > awidth || 2 * an[i] + 1 > aheight) return -1;
        sd[i] = {an[i], LFBM5D_SADCT, cost ? cost[i] : (n_steps == 2 ? (i == 0 ? 10u : 9u) : 1u)};
    }
    plan::Graph G;
    plan::build(mask, plan::Grid{awidth, aheight, ang_major}, sd, n_steps, world, lanes, 0, G);
    std::vector<unsigned> pos(G.nodes.size(), 0);
    for (size_t i = 0; i < G.order.size(); i++) pos[G.order[i]] = (unsigned)i;
    for (size_t i = 0; i < G.nodes.size() && i < node_cap && out_nodes; i++) {
        const plan::Node& nd = G.nodes[i];
        unsigned* o = out_nodes + 8 * i;
        o[0] = (unsigned)nd.s; o[1] = nd.w; o[2] = nd.pst; o[3] = (unsigned)nd.rank; o[4] = (unsigned)nd.lane; o[5] = nd.start; o[6] = pos[i]; o[7] = nd.chain;
    }
    for (size_t i = 0; i < G.xfers.size() && i < msg_cap && out_msgs; i++) {
        const plan::Xfer& X = G.xfers[i];
        unsigned* o = out_msgs + 6 * i;
        o[0] = (unsigned)X.kind; o[1] = X.from; o[2] = X.to_node < 0 ? 0xffffffffu : (unsigned)X.to_node; o[3] = (unsigned)X.to_rank; o[4] = X.sai; o[5] = (unsigned)X.channel;
    }
    if (out_counts) { out_counts[0] = (unsigned)G.nodes.size(); out_counts[1] = (unsigned)G.xfers.size(); out_counts[2] = G.makespan; out_counts[3] = G.centre_ok ? 1u : 0u; }
    return (int)G.nodes.size();
}

int lfbm5d_last_windows(const lfbm5d_ctx* c, unsigned* out_sai, unsigned cap) {
    if (!c) return -1;
    for (size_t i = 0; i < c->last_windows.size() && i < cap && out_sai; i++) out_sai[i] = c->last_windows[i];
    return (int)c->last_windows.size();
}

int lfbm5d_last_window_sigmas(const lfbm5d_ctx* c, float* out, unsigned cap) {
    if (!c) return -1;
    for (size_t i = 0; i < c->views.last.size() && i < cap && out; i++) out[i] = c->views.last[i];
    return (int)c->views.last.size();
}

int lfbm5d_comm_ranks(const lfbm5d_ctx* c) {
    if (!c || !c->comm) return 0;
    int n = 0;
    return ncclCommCount(c->comm, &n) == ncclSuccess ? n : -1;
}

int lfbm5d_comm_selftest(lfbm5d_ctx* c, unsigned n) {
    if (!c || !n) return 1;
    (void)hipSetDevice(c->device);
    ncclComm_t comm = c->comm;
    bool own = false;
    if (!comm) {   /* no communicator yet: a one-rank one exercises the same RCCL code path */
        ncclUniqueId id;
        if (ncclGetUniqueId(&id) != ncclSuccess) return fail(c, "ncclGetUniqueId failed");
        if (ncclCommInitRank(&comm, 1, id, 0) != ncclSuccess) return fail(c, "ncclCommInitRank failed");
        own = true;
    }
    const int world = own ? 1 : c->world;
    float* d = nullptr;
    std::vector<float> h(n);
    for (unsigned i = 0; i < n; i++) h[i] = (float)(i % 251) + 0.5f;
    int rc = 0;
    if (hipMalloc(&d, n * sizeof(float)) != hipSuccess) rc = fail(c, "hipMalloc failed");
    if (!rc && hipMemcpyAsync(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(c, "copy failed");
    if (!rc && ncclAllReduce(d, d, n, ncclFloat, ncclSum, comm, c->stream) != ncclSuccess) rc = fail(c, "ncclAllReduce failed");
    std::vector<float> r(n);
    if (!rc && hipMemcpyAsync(r.data(), d, n * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(c, "copy failed");
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, "stream failed");
    for (unsigned i = 0; i < n && !rc; i++)
        if (r[i] != h[i] * (float)world) rc = fail(c, "all-reduce returned a wrong sum");
    /* the graph form's primitives: a split communicator, grouped send / recv (to this rank itself: the only peer a
     * one-GPU box has) and a grouped broadcast, on the exchange path's kind of stream */
    if (!rc && n >= 2) {
        ncclComm_t comm2 = nullptr;
        float* d2 = nullptr;
        const unsigned half = n / 2;
        int me = 0;
        if (ncclCommUserRank(comm, &me) != ncclSuccess) rc = fail(c, "ncclCommUserRank failed");
        if (!rc && ncclCommSplit(comm, 0, me, &comm2, nullptr) != ncclSuccess) rc = fail(c, "ncclCommSplit failed");
        if (!rc && hipMalloc(&d2, half * sizeof(float)) != hipSuccess) rc = fail(c, "hipMalloc failed");
        if (!rc && hipMemsetAsync(d2, 0, half * sizeof(float), c->stream) != hipSuccess) rc = fail(c, "memset failed");
        if (!rc) {
            bool ok = ncclGroupStart() == ncclSuccess;
            ok = ok && ncclSend(d, half, ncclFloat, me, comm2, c->stream) == ncclSuccess;
            ok = ok && ncclRecv(d2, half, ncclFloat, me, comm2, c->stream) == ncclSuccess;
            ok = ncclGroupEnd() == ncclSuccess && ok;
            ok = ok && ncclGroupStart() == ncclSuccess;
            ok = ok && ncclBroadcast(d + half, d + half, n - half, ncclFloat, 0, comm, c->stream) == ncclSuccess;
            ok = ncclGroupEnd() == ncclSuccess && ok;
            if (!ok) rc = fail(c, "RCCL send / recv / broadcast failed");
        }
        std::vector<float> r2(half);
        if (!rc && hipMemcpyAsync(r2.data(), d2, half * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(c, "copy failed");
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, "stream failed");
        for (unsigned i = 0; i < half && !rc; i++)
            if (r2[i] != r[i]) rc = fail(c, "send / recv returned wrong data");
        if (d2) (void)hipFree(d2);
        if (comm2) ncclCommDestroy(comm2);
    }
    /* several ranks: the exchange pattern of the window graph between real peers -- both channels at once, each on its
     * exchange stream, channel 0 passing a block to the next rank while channel 1 passes one to the previous rank */
    if (!rc && !own && world > 1 && c->comm2 && n >= 4) {
        int me = c->rank;
        const int nxt = (me + 1) % world, prv = (me + world - 1) % world;
        const unsigned q = n / 4;
        float* e = nullptr;
        hipStream_t xs[2] = {nullptr, nullptr};
        if (hipMalloc(&e, (size_t)4 * q * sizeof(float)) != hipSuccess) rc = fail(c, "hipMalloc failed");
        for (int ch = 0; ch < 2 && !rc; ch++)
            if (hipStreamCreateWithFlags(&xs[ch], hipStreamNonBlocking) != hipSuccess) rc = fail(c, "hipStreamCreate failed");
        std::vector<float> hs(2 * q);
        for (unsigned i = 0; i < 2 * q; i++) hs[i] = (float)(me * 1000) + (float)(i % 97);     /* [0,q): for next, [q,2q): for prev */
        if (!rc && hipMemcpyAsync(e, hs.data(), 2 * q * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(c, "copy failed");
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, "stream failed");
        if (!rc) {
            bool ok = ncclGroupStart() == ncclSuccess;
            ok = ok && ncclSend(e, q, ncclFloat, nxt, c->comm, xs[0]) == ncclSuccess;
            ok = ok && ncclRecv(e + 2 * q, q, ncclFloat, prv, c->comm, xs[0]) == ncclSuccess;
            ok = ncclGroupEnd() == ncclSuccess && ok;
            ok = ok && ncclGroupStart() == ncclSuccess;
            ok = ok && ncclSend(e + q, q, ncclFloat, prv, c->comm2, xs[1]) == ncclSuccess;
            ok = ok && ncclRecv(e + 3 * q, q, ncclFloat, nxt, c->comm2, xs[1]) == ncclSuccess;
            ok = ncclGroupEnd() == ncclSuccess && ok;
            if (!ok) rc = fail(c, "RCCL two-channel exchange failed");
        }
        for (int ch = 0; ch < 2 && !rc; ch++)
            if (hipStreamSynchronize(xs[ch]) != hipSuccess) rc = fail(c, "exchange stream failed");
        std::vector<float> hr(2 * q);
        if (!rc && hipMemcpy(hr.data(), e + 2 * q, 2 * q * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, "copy failed");
        for (unsigned i = 0; i < q && !rc; i++)
            if (hr[i] != (float)(prv * 1000) + (float)(i % 97) || hr[q + i] != (float)(nxt * 1000) + (float)((q + i) % 97))
                rc = fail(c, "two-channel exchange returned wrong data");
        for (int ch = 0; ch < 2; ch++) if (xs[ch]) (void)hipStreamDestroy(xs[ch]);
        if (e) (void)hipFree(e);
    }
    if (d) (void)hipFree(d);
    if (own) ncclCommDestroy(comm);
    return rc;
}

int lfbm5d_set_tiles(lfbm5d_ctx* c, int nb_tiles) {
    if (!c || nb_tiles < 0) return 1;
    int n = 1;
    while (n * 2 <= nb_tiles) n *= 2;     /* main.cpp:101-102 floors nb_threads to a power of two */
    c->tiles = nb_tiles <= 1 ? 1 : n;
    return 0;
}

int lfbm5d_set_shard(lfbm5d_ctx* c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return 1;
    c->rank = rank; c->world = world;
    return 0;
}

int lfbm5d_pass_device(lfbm5d_ctx* c, int step, const lfbm5d_params* P, unsigned aw, unsigned ah,
                       unsigned Wb, unsigned Hb, unsigned C, const float* d_noisy, const float* d_basic,
                       float* d_num, float* d_den, const unsigned* h_mask, const unsigned* h_procSAI,
                       unsigned cst, unsigned pst) {
    if (!c || !P) return 1;
    (void)hipSetDevice(c->device);
    c->pass_rank = c->rank; c->pass_world = c->world; c->pass_reduce = c->comm != nullptr;
    const int rc = pass_impl(c, step, P, aw, ah, Wb, Hb, C, d_noisy, d_basic, d_num, d_den, h_mask, h_procSAI, cst, pst);
    c->pass_rank = 0; c->pass_world = 1; c->pass_reduce = false;
    if (rc) return 1;
    HIPCK(c, hipStreamSynchronize(c->stream));
    drain_events(c);
    return fold_counters(c, P, aw * ah, C, step);
}

int lfbm5d_step1_device(lfbm5d_ctx* c, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask,
                        float* d_basic, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                        unsigned W, unsigned H, unsigned C) {
    if (!c || !P) return 1;
    (void)hipSetDevice(c->device);
    return run_step(c, 1, P, d_noisy, h_mask, nullptr, d_basic, ang_major, awidth, aheight, an, W, H, C);
}

int lfbm5d_step2_device(lfbm5d_ctx* c, const lfbm5d_params* P, float* d_noisy, const unsigned* h_mask,
                        float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth,
                        unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C) {
    if (!c || !P) return 1;
    (void)hipSetDevice(c->device);
    return run_step(c, 2, P, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an, W, H, C);
}

int lfbm5d_denoise_device(lfbm5d_ctx* c, const lfbm5d_params* P1, const lfbm5d_params* P2, float* d_noisy, const unsigned* h_mask,
                          float* d_basic, float* d_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1,
                          unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c || !P1 || !P2 || !h_mask) return 1;
    (void)hipSetDevice(c->device);
    return run_denoise(c, P1, P2, d_noisy, h_mask, d_basic, d_denoised, ang_major, awidth, aheight, an1, an2, W, H, C);
}

/* ---- host seam.  The *_host_sai entry points take the caller's light fields as ONE HOST POINTER PER SAI (what a
 * vector<vector<float>> is); the flat forms below are the same with pointers into one buffer.  On one rank with the window graph
 * the SAIs travel as the graph needs and finishes them; otherwise the whole light fields go up first and come down last. ---- */
namespace {
int host_job(lfbm5d_ctx* c, int kind /* 1 | 2: the step, 3: both */, const lfbm5d_params* P1, const lfbm5d_params* P2, float* const* h_noisy,
             const unsigned* h_mask, float* const* h_basic, float* const* h_out, unsigned ang_major, unsigned awidth, unsigned aheight,
             unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    (void)hipSetDevice(c->device);
    const unsigned asize = awidth * aheight;
    for (unsigned st = 0; st < asize; st++)
        if (h_mask[st] && (!h_noisy[st] || !h_basic[st] || (kind != 1 && !h_out[st]))) return fail(c, "host seam: NULL pointer for a non-empty SAI");
    const size_t bytes = (size_t)asize * C * W * H * sizeof(float);
    HIPCK(c, c->h2d_noisy.reserve(bytes));
    HIPCK(c, c->h2d_basic.reserve(bytes));
    if (kind != 1) HIPCK(c, c->h2d_out.reserve(bytes));
    HostIO io; io.noisy = h_noisy; io.basic = h_basic; io.out = h_out;
    float* const dn = c->h2d_noisy.as<float>(); float* const db = c->h2d_basic.as<float>(); float* const dd = c->h2d_out.as<float>();
    if (kind == 1) return run_step(c, 1, P1, dn, h_mask, nullptr, db, ang_major, awidth, aheight, an1, W, H, C, &io);
    if (kind == 2) return run_step(c, 2, P2, dn, h_mask, db, dd, ang_major, awidth, aheight, an2, W, H, C, &io);
    return run_denoise(c, P1, P2, dn, h_mask, db, dd, ang_major, awidth, aheight, an1, an2, W, H, C, &io);
}
/* pointers into flat [asize][C*H*W] buffers; the outputs of empty SAIs read as zeros (what the flat form has always returned) */
void flat_ptrs(std::vector<float*>& v, float* base, const unsigned* h_mask, unsigned asize, size_t img, bool zero_empty) {
    v.resize(asize);
    for (unsigned st = 0; st < asize; st++) {
        v[st] = base ? base + (size_t)st * img : nullptr;
        if (base && zero_empty && !h_mask[st]) std::memset(v[st], 0, img * sizeof(float));
    }
}
} /* namespace */

int lfbm5d_denoise_host_sai(lfbm5d_ctx* c, const lfbm5d_params* P1, const lfbm5d_params* P2, float* const* h_noisy, const unsigned* h_mask,
                            float* const* h_basic, float* const* h_denoised, unsigned ang_major, unsigned awidth, unsigned aheight,
                            unsigned an1, unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c || !P1 || !P2 || !h_mask || !h_noisy || !h_basic || !h_denoised) return 1;
    return host_job(c, 3, P1, P2, h_noisy, h_mask, h_basic, h_denoised, ang_major, awidth, aheight, an1, an2, W, H, C);
}
int lfbm5d_step1_host_sai(lfbm5d_ctx* c, const lfbm5d_params* P, float* const* h_noisy, const unsigned* h_mask, float* const* h_basic,
                          unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C) {
    if (!c || !P || !h_mask || !h_noisy || !h_basic) return 1;
    return host_job(c, 1, P, nullptr, h_noisy, h_mask, h_basic, nullptr, ang_major, awidth, aheight, an, an, W, H, C);
}
int lfbm5d_step2_host_sai(lfbm5d_ctx* c, const lfbm5d_params* P, float* const* h_noisy, const unsigned* h_mask, float* const* h_basic,
                          float* const* h_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an, unsigned W, unsigned H,
                          unsigned C) {
    if (!c || !P || !h_mask || !h_noisy || !h_basic || !h_denoised) return 1;
    return host_job(c, 2, nullptr, P, h_noisy, h_mask, h_basic, h_denoised, ang_major, awidth, aheight, an, an, W, H, C);
}

int lfbm5d_denoise_host(lfbm5d_ctx* c, const lfbm5d_params* P1, const lfbm5d_params* P2, float* h_noisy, const unsigned* h_mask,
                        float* h_basic, float* h_denoised, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an1,
                        unsigned an2, unsigned W, unsigned H, unsigned C) {
    if (!c || !P1 || !P2 || !h_mask || !h_noisy || !h_basic || !h_denoised) return 1;
    const size_t img = (size_t)C * W * H;
    std::vector<float*> pn, pb, pd;
    flat_ptrs(pn, h_noisy, h_mask, awidth * aheight, img, false);
    flat_ptrs(pb, h_basic, h_mask, awidth * aheight, img, true);
    flat_ptrs(pd, h_denoised, h_mask, awidth * aheight, img, true);
    return host_job(c, 3, P1, P2, pn.data(), h_mask, pb.data(), pd.data(), ang_major, awidth, aheight, an1, an2, W, H, C);
}

int lfbm5d_step1_host(lfbm5d_ctx* c, const lfbm5d_params* P, float* h_noisy, const unsigned* h_mask,
                      float* h_basic, unsigned ang_major, unsigned awidth, unsigned aheight, unsigned an,
                      unsigned W, unsigned H, unsigned C) {
    if (!c || !P || !h_mask || !h_noisy || !h_basic) return 1;
    const size_t img = (size_t)C * W * H;
    std::vector<float*> pn, pb;
    flat_ptrs(pn, h_noisy, h_mask, awidth * aheight, img, false);
    flat_ptrs(pb, h_basic, h_mask, awidth * aheight, img, true);
    return host_job(c, 1, P, nullptr, pn.data(), h_mask, pb.data(), nullptr, ang_major, awidth, aheight, an, an, W, H, C);
}

int lfbm5d_step2_host(lfbm5d_ctx* c, const lfbm5d_params* P, float* h_noisy, const unsigned* h_mask,
                      float* h_basic, float* h_denoised, unsigned ang_major, unsigned awidth,
                      unsigned aheight, unsigned an, unsigned W, unsigned H, unsigned C) {
    if (!c || !P || !h_mask || !h_noisy || !h_basic || !h_denoised) return 1;
    const size_t img = (size_t)C * W * H;
    std::vector<float*> pn, pb, pd;
    flat_ptrs(pn, h_noisy, h_mask, awidth * aheight, img, false);
    flat_ptrs(pb, h_basic, h_mask, awidth * aheight, img, false);
    flat_ptrs(pd, h_denoised, h_mask, awidth * aheight, img, true);
    return host_job(c, 2, nullptr, P, pn.data(), h_mask, pb.data(), pd.data(), ang_major, awidth, aheight, an, an, W, H, C);
}

/* ---- per-SAI BM3D (LFBM3Ddenoising) ---- */
namespace {
/* bm3d_1st_step / bm3d_2nd_step (bm3d.cpp:315-690) on a mirror-padded image already in HBM: the core pass with a
 * one-image "window" (A = 1, no disparity search, no angular transform, Hadamard along the stack), then
 * d_out = numerator / denominator over the whole padded image (pixels no patch reached keep the input). */
int bm3d_step(lfbm5d_ctx* c, int step, const lfbm5d_bm3d_params* B, unsigned Wb, unsigned Hb, unsigned C,
              const float* d_noisy, const float* d_basic, float* d_out) {
    lfbm5d_params P;
    std::memset(&P, 0, sizeof(P));
    P.sigma = B->sigma; P.lambda = B->lambda3D; P.N = B->N; P.nSim = B->nHW; P.nDisp = 0; P.k = B->k; P.p = B->p;
    P.useSD = B->useSD; P.tau_2D = B->tau_2D; P.tau_4D = LFBM5D_ID; P.tau_5D = LFBM5D_HADAMARD; P.color_space = B->color_space;
    const size_t n = (size_t)C * Wb * Hb;
    HIPCK(c, c->w_num.reserve(n * sizeof(float)));
    HIPCK(c, c->w_den.reserve(n * sizeof(float)));
    HIPCK(c, hipMemsetAsync(c->w_num.p, 0, n * sizeof(float), c->stream));
    HIPCK(c, hipMemsetAsync(c->w_den.p, 0, n * sizeof(float), c->stream));
    const unsigned one = 1, zero = 0;
    c->pass_rank = 0; c->pass_world = 1; c->pass_reduce = false;
    if (pass_impl(c, step, &P, 1, 1, Wb, Hb, C, d_noisy, d_basic, c->w_num.as<float>(), c->w_den.as<float>(), &one, &zero, 0, 0, true))
        return 1;
    HIPCK(c, launch_estimate(c->stream, c->w_num.as<float>(), c->w_den.as<float>(), step == 1 ? d_noisy : d_basic, d_out, n));
    return 0;
}
int bm3d_fold(lfbm5d_ctx* c, const lfbm5d_bm3d_params* B, unsigned C, int step) {
    lfbm5d_params P; std::memset(&P, 0, sizeof(P)); P.k = B->k;
    HIPCK(c, hipStreamSynchronize(c->stream));
    drain_events(c);
    return fold_counters(c, &P, 1, C, step);
}
/* run_bm3d_LF (bm3d_LF.cpp:75-125) -> run_bm3d (bm3d.cpp:86-300, nb_threads == 1) on device-resident buffers */
int run_bm3d_lf(lfbm5d_ctx* c, const lfbm5d_bm3d_params* Hd, const lfbm5d_bm3d_params* Wn, float* d_noisy, const unsigned* h_mask,
                float* d_basic, float* d_denoised, unsigned asize, unsigned W, unsigned H, unsigned C) {
    /* the reference pads both steps by nHard, searches the second within nWien and crops it at offset nWien of the nHard-padded
     * image (bm3d.cpp:126-189): a shifted picture unless the two are equal -- reproduced as is for nWien <= nHard.  With
     * nWien > nHard the crop reaches rows and columns the second step never aggregates into, which the reference returns
     * as 0 / 0: no result to reproduce */
    if (Wn->nHW > Hd->nHW) return fail(c, "unsupported: BM3D with nWien > nHard (the reference's own result is undefined there: 0 / 0 in the cropped border)");
    const bool views = !c->views.table.empty();   /* a view table (include/lfbm5d_views.h): SAI v is filtered with sigma_v in both steps */
    if (Hd->color_space != Wn->color_space || (!views && Hd->sigma != Wn->sigma)) return fail(c, "BM3D: both steps share sigma and colour space");
    const unsigned nP = Hd->nHW, Wb = W + 2 * nP, Hb = H + 2 * nP;
    if (check_padding(c, W, H, nP)) return 1;
    const size_t img = (size_t)C * W * H, imgb = (size_t)C * Wb * Hb;
    /* The SAIs are independent images (bm3d_LF.cpp:106-121 is a plain loop): they are dealt to lanes -- contexts with a stream and
     * work buffers of their own -- so that the kernels of several SAIs are in flight together.  One SAI's launches are small (a
     * 512 x 512 image: 99 workgroups of the table kernel, whose duration is one table walk however few they are).
     * LFBM5D_BM3D_LANES (default 3: 64 -> 105 SAI-MP/s on 512 x 512 SAIs; 1: the sequential form); results do not depend on it. */
    unsigned n_sai = 0;
    for (unsigned st = 0; st < asize; st++) n_sai += h_mask[st] ? 1u : 0u;
    const unsigned n_l = std::max(1u, std::min({8u, (unsigned)std::max(1, c->opt->bm3d_lanes), std::max(1u, n_sai)}));
    while (c->lanes.size() + 1 < n_l) {
        std::string e;
        lfbm5d_ctx* x = new_ctx(c->device, e);
        if (!x) return fail(c, "lane context: " + e);
        x->opt = c->opt; x->corr = c->corr;
        c->lanes.push_back(x);
    }
    HIPCK(c, hipStreamSynchronize(c->stream));   /* the caller's stream has produced d_noisy */
    /* an error return must not leave other lanes' kernels running on the caller's buffers */
    struct DrainOnError { bool armed; ~DrainOnError() { if (armed) (void)hipDeviceSynchronize(); } } drain_guard{true};
    unsigned turn = 0;
    for (unsigned st = 0; st < asize; st++) {
        if (!h_mask[st]) continue;
        lfbm5d_ctx* const x = turn % n_l == 0 ? c : c->lanes[turn % n_l - 1];
        turn++;
        hipStream_t s = x->stream;
        HIPCK(c, x->w_noisy.reserve(imgb * sizeof(float)));
        HIPCK(c, x->w_basic.reserve(imgb * sizeof(float)));
        HIPCK(c, x->t_num.reserve(imgb * sizeof(float)));
        float* const wn = x->w_noisy.as<float>(); float* const wb = x->w_basic.as<float>(); float* const wo = x->t_num.as<float>();
        float* noisy = d_noisy + st * img; float* basic = d_basic + st * img; float* deno = d_denoised + st * img;
        lfbm5d_bm3d_params Hv = *Hd, Wv = *Wn;
        if (views) Hv.sigma = Wv.sigma = (float)c->views.table[st];
        if (C == 3) HIPCK(c, launch_color(s, noisy, Hd->color_space, W * H, 1));
        HIPCK(c, launch_symetrize(s, noisy, wn, W, H, C, nP));
        if (bm3d_step(x, 1, &Hv, Wb, Hb, C, wn, nullptr, wo)) { if (x != c) c->err = x->err; return 1; }
        HIPCK(c, launch_unsymetrize(s, basic, wo, W, H, C, nP));
        HIPCK(c, launch_symetrize(s, basic, wb, W, H, C, nP));
        if (bm3d_step(x, 2, &Wv, Wb, Hb, C, wn, wb, wo)) { if (x != c) c->err = x->err; return 1; }
        HIPCK(c, launch_crop(s, deno, wo, W, H, C, nP, Wn->nHW));
        if (C == 3) {
            HIPCK(c, launch_color(s, deno, Hd->color_space, W * H, 0));
            HIPCK(c, launch_color(s, noisy, Hd->color_space, W * H, 0));
            HIPCK(c, launch_color(s, basic, Hd->color_space, W * H, 0));
        }
        if (x->pending.size() >= 64) {   /* bound the event pool on large light fields */
            if (bm3d_fold(x, Hd, C, 1)) { if (x != c) c->err = x->err; return 1; }
        }
    }
    /* drain the lanes, fold their counters and event times into this context */
    for (unsigned l = 1; l < n_l; l++) {
        lfbm5d_ctx* const x = c->lanes[l - 1];
        if (bm3d_fold(x, Wn, C, 2)) { c->err = x->err; return 1; }
        add_stats(c->stats, x->stats);
        std::memset(&x->stats, 0, sizeof(x->stats));
    }
    drain_guard.armed = false;   /* every lane has been synchronised above */
    return bm3d_fold(c, Wn, C, 2);
}
} /* namespace */

int lfbm5d_bm3d_step_device(lfbm5d_ctx* c, int step, const lfbm5d_bm3d_params* P, unsigned Wb, unsigned Hb, unsigned C,
                            const float* d_noisy, const float* d_basic, float* d_out) {
    if (!c || !P || (step != 1 && step != 2)) return 1;
    (void)hipSetDevice(c->device);
    if (step == 2 && !d_basic) return fail(c, "step 2 needs the basic estimate");
    if (bm3d_step(c, step, P, Wb, Hb, C, d_noisy, d_basic, d_out)) return 1;
    return bm3d_fold(c, P, C, step);
}

int lfbm5d_bm3d_lf_device(lfbm5d_ctx* c, const lfbm5d_bm3d_params* hard, const lfbm5d_bm3d_params* wien, float* d_noisy,
                          const unsigned* h_mask, float* d_basic, float* d_denoised, unsigned asize, unsigned W, unsigned H,
                          unsigned C) {
    if (!c || !hard || !wien || !h_mask) return 1;
    (void)hipSetDevice(c->device);
    return run_bm3d_lf(c, hard, wien, d_noisy, h_mask, d_basic, d_denoised, asize, W, H, C);
}

int lfbm5d_bm3d_lf_host(lfbm5d_ctx* c, const lfbm5d_bm3d_params* hard, const lfbm5d_bm3d_params* wien, float* h_noisy,
                        const unsigned* h_mask, float* h_basic, float* h_denoised, unsigned asize, unsigned W, unsigned H,
                        unsigned C) {
    if (!c || !hard || !wien || !h_mask) return 1;
    (void)hipSetDevice(c->device);
    const size_t bytes = (size_t)asize * C * W * H * sizeof(float);
    HIPCK(c, c->h2d_noisy.reserve(bytes));
    HIPCK(c, c->h2d_basic.reserve(bytes));
    HIPCK(c, c->h2d_out.reserve(bytes));
    HIPCK(c, hipMemcpy(c->h2d_noisy.p, h_noisy, bytes, hipMemcpyHostToDevice));
    HIPCK(c, hipMemsetAsync(c->h2d_basic.p, 0, bytes, c->stream));
    HIPCK(c, hipMemsetAsync(c->h2d_out.p, 0, bytes, c->stream));
    if (run_bm3d_lf(c, hard, wien, c->h2d_noisy.as<float>(), h_mask, c->h2d_basic.as<float>(), c->h2d_out.as<float>(), asize, W, H, C)) return 1;
    HIPCK(c, hipMemcpy(h_noisy, c->h2d_noisy.p, bytes, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(h_basic, c->h2d_basic.p, bytes, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(h_denoised, c->h2d_out.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int lfbm5d_last_bm(lfbm5d_ctx* c, unsigned* n_refs, unsigned* h_refs, unsigned* h_self_idx,
                   unsigned* h_self_cnt, unsigned* h_best, unsigned char* h_shape) {
    if (!c) return 1;
    (void)hipSetDevice(c->device);
    HIPCK(c, hipStreamSynchronize(c->stream));
    const unsigned R = c->last_n_refs;
    if (n_refs) *n_refs = R;
    if (!R) return 0;
    if (h_refs) std::memcpy(h_refs, c->gc[c->last_gslot].last_refs_host.data(), R * sizeof(unsigned));
    if (h_self_idx) HIPCK(c, hipMemcpy(h_self_idx, c->self_idx.p, (size_t)R * c->last_N * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (h_self_cnt) HIPCK(c, hipMemcpy(h_self_cnt, c->self_cnt.p, (size_t)R * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (h_best) HIPCK(c, hipMemcpy(h_best, c->best.p, c->last_A * c->last_plane * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (h_shape) HIPCK(c, hipMemcpy(h_shape, c->shape.p, c->last_A * c->last_plane, hipMemcpyDeviceToHost));
    return 0;
}

size_t lfbm5d_last_tables(lfbm5d_ctx* c, float* h_tables, size_t n_floats) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    const size_t have = c->tables.cap / sizeof(float);
    if (!h_tables) return have;
    const size_t n = std::min(have, n_floats);
    if (n && hipMemcpy(h_tables, c->tables.p, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

size_t lfbm5d_last_weights(lfbm5d_ctx* c, float* h_w, size_t n_floats) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    const size_t have = c->wgt.cap / sizeof(float);
    if (!h_w) return have;
    const size_t n = std::min(have, n_floats);
    if (n && hipMemcpy(h_w, c->wgt.p, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

int lfbm5d_last_group_list(lfbm5d_ctx* c, unsigned* n, unsigned* out, unsigned cap) {
    if (!c || !n) return -1;
    (void)hipSetDevice(c->device);
    *n = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (!c->sa_list.p) return 0;
    const size_t slots = c->sa_list.cap / sizeof(unsigned);
    unsigned cnt = 0;
    if (hipMemcpy(&cnt, c->sa_list.p, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    cnt = (unsigned)std::min((size_t)cnt, slots - 1);
    *n = cnt;
    const unsigned m = std::min(cnt, cap);
    if (out && m && hipMemcpy(out, c->sa_list.as<unsigned>() + 1, m * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

size_t lfbm5d_last_scores(lfbm5d_ctx* c, float* h_scores, size_t n_floats) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    /* a pass that skipped the fill of `scores` (pass_impl) left stale values where the table kernel does not write: patched here, at
     * the read-out, rather than by filling whenever a read-out might follow */
    if (c->unfilled.pending) {
        const lfbm5d_ctx::UnfilledScores& u = c->unfilled;
        if (launch_scores_patch(c->stream, c->scores.as<float>(), u.n_rows, u.n_cols, u.W, u.nSim, u.nHW, u.p, u.last_r, u.last_c, u.fill) != hipSuccess) return 0;
        c->unfilled.pending = false;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    const size_t have = c->scores.cap / sizeof(float);
    if (!h_scores) return have;
    const size_t n = std::min(have, n_floats);
    if (n && hipMemcpy(h_scores, c->scores.p, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

int lfbm5d_last_scan_version(const lfbm5d_ctx* c) { return c ? c->last_scan_version : 0; }

int lfbm5d_debug_aggregate(lfbm5d_ctx* c, const lfbm5d_agg_debug* d) {
    if (!c) return 1;
    if (!d) return fail(c, "debug_aggregate: no arguments");
    typedef unsigned long long u64;
    /* what k_aggregate takes for granted (pass_impl guarantees it by construction) */
    if (!d->num || !d->den || !d->filt || !d->wgt || !d->aggpos || !d->mask || !d->proc) return fail(c, "debug_aggregate: NULL pointer");
    if (d->direct && !d->sai) return fail(c, "debug_aggregate: NULL pointer (direct form without a slot-to-SAI list)");
    if (!is_pow2(d->N) || d->N > (unsigned)kMaxN3) return fail(c, "debug_aggregate: N must be a power of two <= 32");
    if (d->k < 2 || d->k > (unsigned)kMaxK) return fail(c, "debug_aggregate: patch size k outside 2..32");
    if (d->C != 1 && d->C != 3) return fail(c, "debug_aggregate: chnls must be 1 or 3");
    if (d->A < 1 || d->A > (unsigned)kBigA || d->pst >= d->A) return fail(c, "debug_aggregate: A outside 1..289 or pst outside the window");
    if (d->Wb > 65535u || d->Hb > 65535u) return fail(c, "debug_aggregate: Wb and Hb must be at most 65535 (positions are 16-bit pairs)");
    if (d->nSim < 1 || d->nSim > 48 || d->nDisp > 24 || d->p < 1) return fail(c, "debug_aggregate: bad search window / step");
    const unsigned nHW = d->nSim + d->nDisp, k2 = d->k * d->k;
    if (d->Wb < 2 * nHW + d->k + 1 || d->Hb < 2 * nHW + d->k + 1) return fail(c, "debug_aggregate: window smaller than 2 nHW + k + 1");
    if (!d->n_groups || d->ref_begin > d->n_refs_total || d->n_groups > d->n_refs_total - d->ref_begin)
        return fail(c, "debug_aggregate: groups [ref_begin, ref_begin + n_groups) outside the reference list");
    if (!d->irregular) {   /* the kernel derives its candidate ranges from the grid's geometry: the counts must be that grid's */
        std::vector<unsigned> rows, cols;
        ind_init(rows, d->Hb - d->k + 1, nHW, d->p);
        ind_init(cols, d->Wb - d->k + 1, nHW, d->p);
        if (d->n_ref_rows != rows.size() || d->n_ref_cols != cols.size() || (u64)d->n_ref_rows * d->n_ref_cols != d->n_refs_total)
            return fail(c, "debug_aggregate: n_ref_rows / n_ref_cols / n_refs_total are not the reference grid of this window");
        if (d->ref_begin % d->n_ref_cols || d->n_groups % d->n_ref_cols) return fail(c, "debug_aggregate: a launch on the regular grid covers whole rows");
    }
    /* sizes: the gathers of the 64-bit form (agg_64bit) are not bounds-checked by a buffer resource */
    const u64 patch = (u64)d->C * k2, launch_patches = (u64)d->n_groups * d->N;
    if (launch_patches * (d->filt_sai_stride ? 1u : d->A) * patch >= (1ull << 32)) return fail(c, "debug_aggregate: patch offsets beyond 32 bits");
    if (d->filt_sai_stride ? (d->filt_sai_stride < launch_patches * patch || d->filt_bytes / sizeof(float) < d->filt_sai_stride * d->A)
                           : d->filt_bytes / sizeof(float) < launch_patches * d->A * patch)
        return fail(c, "debug_aggregate: filt is smaller than the launch's patches");
    if (d->wgt_floats < (u64)d->n_refs_total * d->C) return fail(c, "debug_aggregate: wgt is smaller than [n_refs_total][C]");
    if (d->aggpos_words < (u64)d->A * d->n_refs_total * d->N) return fail(c, "debug_aggregate: aggpos is smaller than [A][n_refs_total][N]");
    if ((uintptr_t)d->aggpos % 16) return fail(c, "debug_aggregate: aggpos must be 16-byte aligned");
    const u64 plane = d->direct ? (u64)(d->Wb - 2 * nHW) * (d->Hb - 2 * nHW) : (u64)d->Wb * d->Hb;
    if (d->direct) {
        if (d->lf_stride < d->C * plane) return fail(c, "debug_aggregate: lf_stride smaller than one SAI");
        for (unsigned st = 0; st < d->A; st++)
            if (d->sums_floats < d->C * plane || (u64)d->sai[st] > (d->sums_floats - d->C * plane) / d->lf_stride)
                return fail(c, "debug_aggregate: num / den are smaller than the light field the SAI list addresses");
    } else if (d->sums_floats < (u64)d->A * d->C * plane) return fail(c, "debug_aggregate: num / den are smaller than [A][C][Hb][Wb]");

    (void)hipSetDevice(c->device);
    if (c->dbg_agg.k != d->k) {   /* the product's own tables for this patch size: the Kaiser window is all the kernel reads of them */
        GroupTables tb;
        build_tables(tb, d->k, 3, 3);
        HIPCK(c, c->dbg_agg.tb.reserve(sizeof(GroupTables)));
        HIPCK(c, hipStreamSynchronize(c->stream));
        HIPCK(c, hipMemcpy(c->dbg_agg.tb.p, &tb, sizeof(tb), hipMemcpyHostToDevice));
        c->dbg_agg.k = d->k;
    }
    AggArgs aa;
    std::memset(&aa, 0, sizeof(aa));
    aa.num = d->num; aa.den = d->den; aa.filt = d->filt; aa.filt_sai_stride = d->filt_sai_stride; aa.filt_bytes = d->filt_bytes;
    aa.wgt = d->wgt; aa.aggpos = d->aggpos; aa.n_refs_total = d->n_refs_total; aa.tb = c->dbg_agg.tb.as<GroupTables>();
    aa.ref_begin = d->ref_begin; aa.n_groups = d->n_groups; aa.n_ref_rows = d->n_ref_rows; aa.n_ref_cols = d->n_ref_cols;
    aa.Wb = d->Wb; aa.Hb = d->Hb; aa.C = d->C; aa.A = d->A; aa.k = d->k; aa.N = d->N; aa.pst = d->pst; aa.p = d->p;
    aa.nHW = nHW; aa.nSim = d->nSim; aa.nDisp = d->nDisp;
    aa.mask_bits = sai_mask_none(); aa.proc_bits = sai_mask_none();
    for (unsigned st = 0; st < d->A; st++) {
        if (d->mask[st]) aa.mask_bits.set(st);
        if (d->proc[st]) aa.proc_bits.set(st);
    }
    aa.irregular = d->irregular ? 1u : 0u; aa.wchan0 = d->wchan0 ? 1u : 0u;
    aa.opt = c->opt->kernels;
    if (d->direct) {
        aa.direct = 1u; aa.lf_stride = d->lf_stride; aa.sai.n = d->A;
        for (unsigned st = 0; st < d->A; st++) aa.sai.st[st] = d->sai[st];
    }
    HIPCK(c, launch_aggregate(c->stream, aa));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int lfbm5d_debug_group(lfbm5d_ctx* c, const lfbm5d_group_debug* d) {
    if (!c) return 1;
    if (!d) return fail(c, "debug_group: no arguments");
    typedef unsigned long long u64;
    if (d->kernels && d->kernels_cap) d->kernels[0] = 0;
    /* what the group kernels take for granted (pass_impl guarantees it by construction, block matching by its search ranges) */
    if (!d->noisy || !d->refs || !d->self_idx || !d->self_cnt || !d->best || !d->shape || !d->filt || !d->wgt || !d->aggpos || !d->counters ||
        !d->mask || !d->params)
        return fail(c, "debug_group: NULL pointer");
    if (d->step != 1 && d->step != 2) return fail(c, "debug_group: step must be 1 or 2");
    if (d->step == 2 && !d->basic) return fail(c, "debug_group: NULL pointer (step 2 needs the basic estimate)");
    const lfbm5d_params* P = d->params;
    if (validate(c, (int)d->step, P, d->aw, d->ah, d->C, d->bm3d != 0)) { c->err = "debug_group: " + c->err; return 1; }
    if (!d->bm3d && P->N < 1) return fail(c, "debug_group: N must be a power of two <= 32");
    const unsigned A = d->aw * d->ah, k = P->k, k2 = k * k, N = P->N, Wb = d->Wb, Hb = d->Hb, C = d->C, R = d->n_refs_total;
    if (Wb > 65535u || Hb > 65535u) return fail(c, "debug_group: Wb and Hb must be at most 65535 (positions are 16-bit pairs)");
    if (Wb < k || Hb < k) return fail(c, "debug_group: window smaller than a patch");
    if (d->pst >= A || !d->mask[d->pst]) return fail(c, "debug_group: pst is not an SAI of the mask");
    if (!d->n_groups || d->ref_begin > R || d->n_groups > R - d->ref_begin)
        return fail(c, "debug_group: groups [ref_begin, ref_begin + n_groups) outside the reference list");
    const u64 plane = (u64)Wb * Hb, patch = (u64)C * k2, launch_patches = (u64)d->n_groups * N;
    if (launch_patches * (d->filt_sai_stride ? 1u : A) * patch >= (1ull << 32)) return fail(c, "debug_group: patch offsets beyond 32 bits");
    if (d->image_floats < (u64)A * C * plane) return fail(c, "debug_group: noisy / basic are smaller than [A][C][Hb][Wb]");
    if (d->table_words < (u64)A * plane) return fail(c, "debug_group: best / shape are smaller than [A][Wb*Hb]");
    if (d->filt_sai_stride && (A == 9 || A == 1) && !(c->opt->kernels & kOptGroupGeneric) && !c->corr->n)
        return fail(c, "debug_group: SAI-major filt is written by the general kernels only (wider windows, option group_generic)");
    if (d->filt_sai_stride ? (d->filt_sai_stride < launch_patches * patch || d->filt_floats < d->filt_sai_stride * A)
                           : d->filt_floats < launch_patches * A * patch)
        return fail(c, "debug_group: filt is smaller than the launch's patches");
    if (d->wgt_floats < (u64)R * C) return fail(c, "debug_group: wgt is smaller than [n_refs_total][C]");
    if (d->aggpos_words < (u64)A * R * N) return fail(c, "debug_group: aggpos is smaller than [A][n_refs_total][N]");

    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    HIPCK(c, hipStreamSynchronize(s));
    SaiMask mask_bits = sai_mask_none();
    for (unsigned st = 0; st < A; st++) if (d->mask[st]) mask_bits.set(st);
    {   /* the tables: every patch the launch gathers lies inside the window */
        const unsigned g0 = d->ref_begin, ng = d->n_groups;
        std::vector<unsigned> refs(ng), cnt(ng), idx((size_t)ng * N), best;
        HIPCK(c, hipMemcpy(refs.data(), d->refs + g0, (size_t)ng * sizeof(unsigned), hipMemcpyDeviceToHost));
        HIPCK(c, hipMemcpy(cnt.data(), d->self_cnt + g0, (size_t)ng * sizeof(unsigned), hipMemcpyDeviceToHost));
        HIPCK(c, hipMemcpy(idx.data(), d->self_idx + (size_t)g0 * N, (size_t)ng * N * sizeof(unsigned), hipMemcpyDeviceToHost));
        auto inside = [&](unsigned p) { return p < plane && p / Wb <= Hb - k && p % Wb <= Wb - k; };
        for (unsigned g = 0; g < ng; g++) {
            if (!inside(refs[g])) return fail(c, "debug_group: a reference patch lies outside [0, Hb-k] x [0, Wb-k]");
            if (!is_pow2(cnt[g]) || cnt[g] > N) return fail(c, "debug_group: a stack size (self_cnt) is not a power of two in 1..N");
            /* BM3D needs N >= 2 (validate), so its selection always runs, and that stores a single match twice (duplicate rule,
             * lfbm5d_bm.hip): k_group_bm3d8 has no fibre of one -- its default branch would read 31 stack slots nobody wrote */
            if (d->bm3d && cnt[g] < 2) return fail(c, "debug_group: a BM3D stack of one patch (self_cnt 1): block matching stores a single match twice");
            for (unsigned n = 0; n < cnt[g]; n++)
                if (!inside(idx[(size_t)g * N + n])) return fail(c, "debug_group: a stack entry (self_idx) lies outside [0, Hb-k] x [0, Wb-k]");
        }
        if (mask_bits.count() > 1) {
            best.resize((size_t)A * plane);
            HIPCK(c, hipMemcpy(best.data(), d->best, best.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
            for (unsigned st = 0; st < A; st++) {
                if (st == d->pst || !mask_bits.test(st)) continue;
                for (unsigned g = 0; g < ng; g++)
                    for (unsigned n = 0; n < cnt[g]; n++)
                        if (!inside(best[(size_t)st * plane + idx[(size_t)g * N + n]]))
                            return fail(c, "debug_group: a disparity match (best) of a stack entry lies outside [0, Hb-k] x [0, Wb-k]");
            }
        }
    }
    const unsigned Nst = N > 1 ? N : 1;
    HIPCK(c, c->gpos.reserve((size_t)A * R * Nst * sizeof(unsigned)));
    HIPCK(c, c->gofs.reserve((size_t)A * R * Nst * sizeof(unsigned)));
    HIPCK(c, c->gok.reserve((size_t)R * Nst * sizeof(unsigned)));
    HIPCK(c, c->sa_list.reserve((size_t)(4 * (size_t)R + 1) * sizeof(unsigned)));
    HIPCK(c, c->gshape.reserve((size_t)R * (A > (unsigned)kMaxA ? kShapeInfoBigBytes : kShapeInfoBytes)));
    if (c->dbg_group.key[0] != k || c->dbg_group.key[1] != d->aw || c->dbg_group.key[2] != d->ah) {
        GroupTables tb;
        build_tables(tb, k, d->aw, d->ah);
        HIPCK(c, c->dbg_group.tb.reserve(sizeof(GroupTables)));
        HIPCK(c, hipMemcpy(c->dbg_group.tb.p, &tb, sizeof(tb), hipMemcpyHostToDevice));
        c->dbg_group.key[0] = k; c->dbg_group.key[1] = d->aw; c->dbg_group.key[2] = d->ah;
    }
    if (!c->counters.p) {   /* (as pass_impl) */
        HIPCK(c, c->counters.reserve(32 * sizeof(unsigned long long)));
        HIPCK(c, hipMemset(c->counters.p, 0, 32 * sizeof(unsigned long long)));
    }
    /* the launch counts into the context's counters like a pass; they are put back afterwards, so that the stats of the passes stay theirs */
    unsigned long long* const d_counters = c->counters.as<unsigned long long>() + 16 * c->gslot;
    unsigned long long before[2], after[2];
    HIPCK(c, hipMemcpy(before, d_counters, sizeof(before), hipMemcpyDeviceToHost));
    GroupArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    ga.noisy = d->noisy; ga.basic = d->basic;
    ga.refs = d->refs; ga.self_idx = d->self_idx; ga.self_cnt = d->self_cnt; ga.best = d->best; ga.shape = d->shape;
    ga.tb = c->dbg_group.tb.as<GroupTables>();
    ga.wgt = d->wgt; ga.aggpos = d->aggpos; ga.gpos = c->gpos.as<unsigned>(); ga.gofs = c->gofs.as<unsigned>(); ga.gok = c->gok.as<unsigned>();
    ga.sa_list = c->sa_list.as<unsigned>(); ga.gshape = c->gshape.p; ga.n_refs_total = R; ga.counters = d_counters;
    ga.ref_begin = d->ref_begin; ga.n_groups = d->n_groups;
    ga.Wb = Wb; ga.Hb = Hb; ga.C = C; ga.A = A; ga.k = k; ga.N = Nst; ga.pst = d->pst;
    ga.mask_bits = mask_bits; ga.proc_bits = sai_mask_none();
    ga.step = (int)d->step; ga.fill_quirk = d->fill_quirk ? 1u : 0u; ga.bm3d = d->bm3d ? 1u : 0u;
    if (group_args_of_pass(c, ga, P)) return 1;
    /* filt is indexed by the absolute group number, as in a band of a pass */
    const size_t per_group = (size_t)Nst * A * patch;
    ga.filt_sai_stride = d->filt_sai_stride;
    ga.filt = d->filt - (size_t)d->ref_begin * (d->filt_sai_stride ? per_group / A : per_group);
    std::string trace;
    hipError_t e = launch_group(s, ga, &trace, corr_table_of_pass(c, ga));
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(after, d_counters, sizeof(after), hipMemcpyDeviceToHost);
    const hipError_t e_back = hipMemcpy(d_counters, before, sizeof(before), hipMemcpyHostToDevice);   /* also when the launch failed */
    if (e != hipSuccess) return fail(c, std::string("debug_group: launch_group: ") + hipGetErrorString(e));
    HIPCK(c, e_back);
    d->counters[0] = after[0] - before[0]; d->counters[1] = after[1] - before[1];
    if (d->kernels && d->kernels_cap) {
        const size_t n = std::min<size_t>(trace.size(), (size_t)d->kernels_cap - 1);
        std::memcpy(d->kernels, trace.data(), n);
        d->kernels[n] = 0;
    }
    return 0;
}

int lfbm5d_debug_window(lfbm5d_ctx* c, const lfbm5d_window_debug* d) {
    if (!c) return 1;
    if (!d) return fail(c, "debug_window: no arguments");
    typedef unsigned long long u64;
    const unsigned op = d->op, W = d->W, H = d->H, C = d->C, N = d->N, k = d->k;
    if (op > LFBM5D_WOP_COPY_ROWS) return fail(c, "debug_window: unknown op");
    /* what the kernels of lfbm5d_window.hip take for granted (the steps guarantee it by construction) */
    const bool flat = op == LFBM5D_WOP_ESTIMATE || op == LFBM5D_WOP_ESTIMATE_MULTI || op == LFBM5D_WOP_ESTIMATE_LF || op == LFBM5D_WOP_COUNT_ZEROS;
    const bool three = op == LFBM5D_WOP_COLOR || op == LFBM5D_WOP_COLOR_ROUNDTRIP || op == LFBM5D_WOP_FINALIZE || op == LFBM5D_WOP_OUTPUT;
    const bool mirrors = op == LFBM5D_WOP_SYMETRIZE || op == LFBM5D_WOP_SYMETRIZE_MULTI || op == LFBM5D_WOP_WINDOW_BEGIN;
    const bool padded = mirrors || op == LFBM5D_WOP_CROP || op == LFBM5D_WOP_UNSYMETRIZE_MULTI || op == LFBM5D_WOP_WINDOW_END || op == LFBM5D_WOP_COUNT_DENOISED;
    const bool counts = op == LFBM5D_WOP_WINDOW_END || op == LFBM5D_WOP_COUNT_DENOISED;
    const bool listed = op == LFBM5D_WOP_SYMETRIZE_MULTI || op == LFBM5D_WOP_UNSYMETRIZE_MULTI || op == LFBM5D_WOP_WINDOW_BEGIN ||
                        op == LFBM5D_WOP_WINDOW_END || op == LFBM5D_WOP_FINALIZE || op == LFBM5D_WOP_OUTPUT;
    const bool masked = op == LFBM5D_WOP_ESTIMATE_MULTI || op == LFBM5D_WOP_COUNT_DENOISED || op == LFBM5D_WOP_COPY_RECT;
    {   /* the pointers the op cannot do without (the optional ones: basic, dmask, the window sums of the direct form) */
        bool null = false;
        switch (op) {
        case LFBM5D_WOP_COLOR: null = !d->noisy; break;
        case LFBM5D_WOP_COLOR_ROUNDTRIP: null = !d->noisy || !d->out; break;
        case LFBM5D_WOP_SYMETRIZE: case LFBM5D_WOP_SYMETRIZE_MULTI: null = !d->noisy || !d->w_noisy; break;
        case LFBM5D_WOP_CROP: case LFBM5D_WOP_UNSYMETRIZE_MULTI: case LFBM5D_WOP_COPY_RECT: case LFBM5D_WOP_COPY_ROWS: null = !d->w_noisy || !d->out; break;
        case LFBM5D_WOP_ESTIMATE: null = !d->num || !d->den || !d->sub || !d->est; break;
        case LFBM5D_WOP_ESTIMATE_MULTI: null = !d->w_num || !d->w_den || !d->w_noisy || !d->est; break;
        case LFBM5D_WOP_ESTIMATE_LF: null = !d->num || !d->den || !d->sub || !d->out; break;
        case LFBM5D_WOP_WINDOW_BEGIN: null = !d->noisy || !d->num || !d->den || !d->w_noisy || !d->est || !d->counters; break;
        case LFBM5D_WOP_WINDOW_END: null = !d->num || !d->den || !d->counters; break;
        case LFBM5D_WOP_FINALIZE: null = !d->num || !d->den || !d->sub || !d->basic; break;
        case LFBM5D_WOP_OUTPUT: null = !d->num || !d->den || !d->sub || !d->out || !d->noisy || !d->noisy_dst; break;
        case LFBM5D_WOP_COUNT_ZEROS: null = !d->den || !d->counters; break;
        case LFBM5D_WOP_COUNT_DENOISED: null = !d->w_den || !d->counters; break;
        }
        if (null) return fail(c, "debug_window: NULL pointer");
        if (listed && !d->list) return fail(c, "debug_window: NULL pointer (the SAI list)");
        if (masked && !d->slot_mask) return fail(c, "debug_window: NULL pointer (the slot mask)");
    }
    if (op != LFBM5D_WOP_ESTIMATE && op != LFBM5D_WOP_ESTIMATE_LF && op != LFBM5D_WOP_COUNT_ZEROS && op != LFBM5D_WOP_COPY_ROWS) {
        if (C != 1 && C != 3) return fail(c, "debug_window: chnls must be 1 or 3");
        if (three && C != 3) return fail(c, "debug_window: this op works on three channels");
    }
    if (!flat) {
        if (!W || !H) return fail(c, "debug_window: W and H must not be 0");
        if (W > 65535u || H > 65535u || N > 65535u) return fail(c, "debug_window: W, H and N must be at most 65535");
    } else if (!d->n || d->n >= (1ull << 32)) return fail(c, "debug_window: n must be 1 .. 2^32 - 1");
    if (three && d->cs > LFBM5D_OPP && (d->colour || op == LFBM5D_WOP_COLOR || op == LFBM5D_WOP_COLOR_ROUNDTRIP))
        return fail(c, "debug_window: the colour kernels know yuv, ycbcr and opp");
    if (mirrors && (N > W || N > H)) return fail(c, "debug_window: the padding N is larger than the image (the mirror reflects once)");
    if (counts && (k < 1 || k > W || k > H)) return fail(c, "debug_window: patch size k outside 1 .. min(W, H)");
    if ((listed || masked) && d->n_list > (unsigned)kBigA) return fail(c, "debug_window: more than 289 slots");
    if ((listed || masked) && !d->n_list) return fail(c, "debug_window: no slots");
    const bool per_sai = op == LFBM5D_WOP_COLOR || op == LFBM5D_WOP_COLOR_ROUNDTRIP || op == LFBM5D_WOP_ESTIMATE_LF || op == LFBM5D_WOP_COUNT_ZEROS ||
                         op == LFBM5D_WOP_COPY_ROWS;
    if (per_sai && (!d->n_sai || d->n_sai > 65535u)) return fail(c, "debug_window: n_sai must be 1 .. 65535");
    const u64 img = (u64)C * W * H, imgb = (u64)C * (W + 2 * N) * (H + 2 * N), planeb = (u64)(W + 2 * N) * (H + 2 * N);
    if (three && img >= (1ull << 32)) return fail(c, "debug_window: image beyond 32-bit offsets");

    /* the light field a list addresses: its SAI count follows from the size of the buffers */
    auto lf_holds = [&](u64 n_sai_) { return n_sai_ && d->lf_floats >= img && (n_sai_ - 1) <= (d->lf_floats - img) / std::max<u64>(d->lf_stride, 1); };
    u64 lf_sais = 0;
    if (listed || op == LFBM5D_WOP_COLOR || op == LFBM5D_WOP_COLOR_ROUNDTRIP) {
        if (d->lf_stride < img) return fail(c, "debug_window: lf_stride smaller than one image");
        if (d->lf_floats < img) return fail(c, "debug_window: a light-field buffer is smaller than the geometry says");
        lf_sais = (d->lf_floats - img) / d->lf_stride + 1;
    }
    if (listed) {
        const bool plain = op == LFBM5D_WOP_FINALIZE || op == LFBM5D_WOP_OUTPUT;
        for (unsigned i = 0; i < d->n_list; i++) {
            if (d->list[i] == 0xffffffffu) { if (plain) return fail(c, "debug_window: an empty slot (0xffffffff) in a list this op does not test"); }
            else if (d->list[i] >= lf_sais) return fail(c, "debug_window: a list entry lies outside the light field");
        }
    }
    const char* const small_msg = "debug_window: a buffer is smaller than the geometry says";
    SaiList L; std::memset(&L, 0, sizeof(L));
    SaiMask bits = sai_mask_none();
    if (listed) { L.n = d->n_list; for (unsigned i = 0; i < d->n_list; i++) L.st[i] = d->list[i]; }
    if (masked) for (unsigned i = 0; i < d->n_list; i++) if (d->slot_mask[i]) bits.set(i);
    if (d->dmask && (op == LFBM5D_WOP_COLOR || op == LFBM5D_WOP_COLOR_ROUNDTRIP || op == LFBM5D_WOP_ESTIMATE_LF) && d->dmask_words < d->n_sai)
        return fail(c, "debug_window: dmask is smaller than n_sai");
    if (padded && listed && !(op == LFBM5D_WOP_WINDOW_END && !d->w_num && !d->w_den) && d->w_stride < imgb)
        return fail(c, "debug_window: w_stride smaller than one padded image");

    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    hipError_t e = hipSuccess;
    switch (op) {
    case LFBM5D_WOP_COLOR:
        if (!lf_holds(d->n_sai)) return fail(c, small_msg);
        e = launch_color_lf(s, d->noisy, d->lf_stride, d->n_sai, d->dmask, d->cs, W * H, d->forward ? 1 : 0);
        break;
    case LFBM5D_WOP_COLOR_ROUNDTRIP:
        if (!lf_holds(d->n_sai)) return fail(c, small_msg);
        e = launch_color_roundtrip_lf(s, d->noisy, d->out, d->lf_stride, d->n_sai, d->dmask, d->cs, W * H);
        break;
    case LFBM5D_WOP_SYMETRIZE:
        if (d->lf_floats < img || d->w_floats < imgb) return fail(c, small_msg);
        e = launch_symetrize(s, d->noisy, d->w_noisy, W, H, C, N);
        break;
    case LFBM5D_WOP_CROP:
        if (d->off > 2 * N) return fail(c, "debug_window: the crop at off leaves the padded image");
        if (d->lf_floats < img || d->w_floats < imgb) return fail(c, small_msg);
        e = launch_crop(s, d->out, d->w_noisy, W, H, C, N, d->off);
        break;
    case LFBM5D_WOP_SYMETRIZE_MULTI:
        if (d->w_floats < (u64)(L.n - 1) * d->w_stride + imgb) return fail(c, small_msg);
        e = launch_symetrize_multi(s, d->noisy, d->lf_stride, d->w_noisy, d->w_stride, L, W, H, C, N);
        break;
    case LFBM5D_WOP_UNSYMETRIZE_MULTI:
        if (d->w_floats < (u64)(L.n - 1) * d->w_stride + imgb) return fail(c, small_msg);
        e = launch_unsymetrize_multi(s, d->out, d->lf_stride, d->w_noisy, d->w_stride, L, W, H, C, N);
        break;
    case LFBM5D_WOP_ESTIMATE:
        if (d->lf_floats < d->n || d->est_floats < d->n) return fail(c, small_msg);
        e = launch_estimate(s, d->num, d->den, d->sub, d->est, d->n);
        break;
    case LFBM5D_WOP_ESTIMATE_MULTI:
        if (d->w_floats < (u64)d->n_list * C * d->n || d->est_floats < (u64)d->n_list * d->n) return fail(c, small_msg);
        e = launch_estimate_multi(s, d->w_num, d->w_den, d->w_noisy, d->est, d->n, C, d->n_list, bits);
        break;
    case LFBM5D_WOP_ESTIMATE_LF:
        if (d->lf_floats < (u64)d->n_sai * d->n) return fail(c, small_msg);
        e = launch_estimate_lf(s, d->num, d->den, d->sub, d->out, d->n, d->n_sai, d->dmask);
        break;
    case LFBM5D_WOP_WINDOW_BEGIN: {
        if ((d->w_num == nullptr) != (d->w_den == nullptr)) return fail(c, "debug_window: NULL pointer (the direct form leaves out w_num AND w_den)");
        if (d->basic && !d->w_basic) return fail(c, "debug_window: NULL pointer (basic without w_basic)");
        if (d->w_floats < (u64)(L.n - 1) * d->w_stride + imgb || d->est_floats < (u64)L.n * planeb || d->counter_words < kWinCounters) return fail(c, small_msg);
        e = launch_window_begin(s, d->noisy, d->basic, d->num, d->den, d->lf_stride, d->w_noisy, d->basic ? d->w_basic : nullptr, d->w_num, d->w_den,
                                d->est, d->w_stride, L, W, H, C, N, d->counters);
        break;
    }
    case LFBM5D_WOP_WINDOW_END:
        if ((d->w_num == nullptr) != (d->w_den == nullptr)) return fail(c, "debug_window: NULL pointer (the direct form leaves out w_num AND w_den)");
        if ((d->w_num && d->w_floats < (u64)(L.n - 1) * d->w_stride + imgb) || d->counter_words < kWinCounters) return fail(c, small_msg);
        e = launch_window_end(s, d->num, d->den, d->lf_stride, d->w_num, d->w_den, d->w_stride, L, W, H, C, N, k, d->counters);
        break;
    case LFBM5D_WOP_FINALIZE:
        e = launch_finalize_multi(s, d->num, d->den, d->sub, d->basic, d->lf_stride, L, d->cs, W * H, d->colour ? 1 : 0);
        break;
    case LFBM5D_WOP_OUTPUT:
        e = launch_output_multi(s, d->num, d->den, d->sub, d->out, d->basic, d->noisy, d->noisy_dst, d->lf_stride, L, d->cs, W * H, d->colour ? 1 : 0);
        break;
    case LFBM5D_WOP_COUNT_ZEROS:
        if (d->lf_floats < (u64)d->n_sai * d->n || d->counter_words < d->n_sai) return fail(c, small_msg);
        e = launch_count_zeros(s, d->den, d->n, d->n_sai, d->counters);
        break;
    case LFBM5D_WOP_COUNT_DENOISED:
        if (d->w_stride < imgb) return fail(c, "debug_window: w_stride smaller than one padded image");
        if (d->w_floats < (u64)(d->n_list - 1) * d->w_stride + imgb || d->counter_words < 1) return fail(c, small_msg);
        e = launch_count_denoised(s, d->w_den, d->w_stride, d->n_list, bits, W, H, C, N, k, d->counters);
        break;
    case LFBM5D_WOP_COPY_RECT: {
        if (!d->sW || !d->sH || d->sW > 65535u || d->sH > 65535u) return fail(c, "debug_window: sW and sH must be 1 .. 65535");
        if (!d->rw || !d->rh) return fail(c, "debug_window: empty rectangle");
        if (d->rw > W || d->dx0 > W - d->rw || d->rh > H || d->dy0 > H - d->rh || d->rw > d->sW || d->sx0 > d->sW - d->rw || d->rh > d->sH || d->sy0 > d->sH - d->rh)
            return fail(c, "debug_window: the rectangle lies outside its image");
        const u64 simg = (u64)C * d->sW * d->sH;
        if (d->lf_stride < img || d->w_stride < simg) return fail(c, "debug_window: a stride is smaller than one image");
        if (d->lf_floats < (u64)(d->n_list - 1) * d->lf_stride + img || d->w_floats < (u64)(d->n_list - 1) * d->w_stride + simg) return fail(c, small_msg);
        e = launch_copy_rect(s, d->out, d->lf_stride, W, H, d->dx0, d->dy0, d->w_noisy, d->w_stride, d->sW, d->sH, d->sx0, d->sy0, d->rw, d->rh, C,
                             d->n_list, bits);
        break;
    }
    case LFBM5D_WOP_COPY_ROWS:
        if (!d->sH || d->sH > 65535u) return fail(c, "debug_window: sH must be 1 .. 65535");
        if (d->rh > d->sH || d->sy0 > d->sH - d->rh || d->rh > H || d->dy0 > H - d->rh) return fail(c, "debug_window: the rows lie outside their image");
        if (d->w_floats < (u64)d->n_sai * d->sH * W || d->lf_floats < (u64)d->n_sai * H * W) return fail(c, small_msg);
        e = launch_copy_rows(s, d->w_noisy, d->sH, d->sy0, d->out, H, d->dy0, d->rh, W, d->n_sai);
        break;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, std::string("debug_window: ") + hipGetErrorString(e));
    return 0;
}

int lfbm5d_sigma_table(float sigma, unsigned C, unsigned color_space, float* out) {
    if (!out) return 1;
    return sigma_table(sigma, C, color_space, out);
}

int lfbm5d_malloc(void** dptr, size_t bytes) { return hipMalloc(dptr, bytes) == hipSuccess ? 0 : 1; }
int lfbm5d_free(void* dptr) { return hipFree(dptr) == hipSuccess ? 0 : 1; }
int lfbm5d_memcpy_h2d(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1; }
int lfbm5d_memcpy_d2h(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1; }

} /* extern "C" */
