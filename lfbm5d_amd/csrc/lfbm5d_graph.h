/*
 * lfbm5d_graph.h -- a JOB of the window graph (run_graph, lfbm5d_graph.hip) as the step functions hand it over, and what the window
 * engines of lfbm5d_graph.hip and lfbm5d_steps.hip share: a window's masked geometry, a lane's buffers, the transports' teardown and
 * the timer of a collective.  Internal.
 */
#ifndef LFBM5D_GRAPH_H
#define LFBM5D_GRAPH_H

#include "lfbm5d_ctx.h"

namespace lfbm5d_host {

struct GraphJob {
    int n_steps = 1;
    int step[2] = {1, 2};                          /* the reference step every slot runs */
    const lfbm5d_params* P[2] = {nullptr, nullptr};
    unsigned an[2] = {1, 1};
    const float* noisy[2] = {nullptr, nullptr};    /* the (colour-transformed) light field every slot reads */
    float* d_basic = nullptr;                      /* step 2: the pilot; two-step jobs: written SAI by SAI as the first step's sums become final */
    float* g_num[2] = {nullptr, nullptr};          /* the light field's sums, zeroed by the caller */
    float* g_den[2] = {nullptr, nullptr};
    float* d_out = nullptr;                        /* several ranks: the last slot's estimate, formed per SAI by its owner and exchanged */
    const unsigned* d_mask = nullptr;
    /* streamed host seam (one rank): the caller's SAIs are uploaded in the order the windows first use them -- forward colour
     * transform (and, two-step jobs, the round trip the second step reads) per SAI behind the copy -- and every SAI's outputs leave
     * as soon as the last window on it is done; d_noisy = the light-field buffer noisy[0] points to (the in / out LF_noisy) */
    const HostIO* io = nullptr;
    float* d_noisy = nullptr;
    float* pristine = nullptr; float* pristine_b = nullptr;
    unsigned color_space = LFBM5D_RGB;
};

int run_graph(lfbm5d_ctx* c, const GraphJob& J, const plan::Graph& G, const unsigned* h_mask, const plan::Grid& grid,
              unsigned W, unsigned H, unsigned C, int nranks, bool emulate, int* complete_out);

/* The mask applied to a window, per slot: which slots hold a SAI (mask_w, bits; sl = their light-field indices, 0xffffffff for an
 * empty slot), which are processed already (proc_w: the empty ones), and how many SAIs the window holds. */
struct MaskedWindow { std::vector<unsigned> mask_w, proc_w; SaiList sl; SaiMask bits = sai_mask_none(); unsigned n_in = 0; };
inline MaskedWindow mask_window(const plan::Window& w, const unsigned* h_mask) {
    const unsigned Aw = w.slots.size();
    MaskedWindow m;
    m.mask_w.assign(Aw, 0); m.proc_w.assign(Aw, 0);
    m.sl.n = Aw;
    for (unsigned i = 0; i < Aw; i++) {
        m.mask_w[i] = h_mask[w.st[i]];
        m.proc_w[i] = !m.mask_w[i];
        m.sl.st[i] = m.mask_w[i] ? w.st[i] : 0xffffffffu;
        if (m.mask_w[i]) { m.bits.set(i); m.n_in++; }
    }
    return m;
}

/* The sigma of a window's passes: the job's own, or with a view table (include/lfbm5d_views.h) the window sigma. */
inline float window_sigma(const lfbm5d_ctx* c, const lfbm5d_params* P, const plan::Window& w, const unsigned* h_mask) {
    return c->views.table.empty() ? P->sigma : plan::window_sigma(c->views.table.data(), w, h_mask);
}
/* What lfbm5d_last_windows / lfbm5d_last_window_sigmas report after a completed graph: every node's processed SAI and sigma, in node
 * order (windows of other ranks included: the sigma is a function of the table and the plan alone).  P, an: per step slot. */
inline void record_graph_windows(lfbm5d_ctx* c, const plan::Graph& G, const plan::Grid& grid, const unsigned* h_mask,
                                 const lfbm5d_params* const* P, const unsigned* an) {
    for (const plan::Node& nd : G.nodes) {
        c->last_windows.push_back(nd.pst);
        c->views.last.push_back(window_sigma(c, P[nd.s], plan::window_at(grid, nd.ps, nd.pt, an[nd.s]), h_mask));
    }
}

/* A lane = a context with its stream, per-pass work buffers and these window buffers (lane 0 is the job's own context).
 * lane_buffers sizes them for windows of win_floats floats; the padded sums only where the form keeps them. */
struct Lane { lfbm5d_ctx* x; float* w_noisy; float* w_basic; float* w_num; float* w_den; unsigned* d_small; };
int lane_buffers(lfbm5d_ctx* c, lfbm5d_ctx* x, size_t win_floats, bool with_basic, bool with_sums, unsigned asize, Lane& L);

/* The light-field sums of the first n_slots step slots (floats each) in context x's buffers, zeroed on stream xs. */
int zeroed_sums(lfbm5d_ctx* c, lfbm5d_ctx* x, int n_slots, size_t floats, hipStream_t xs, float* g_num[2], float* g_den[2]);

/* Teardown of a transport after a failed job.  abort_comms: peers wait in operations this rank will never match, so both
 * communicators are aborted (comm2 first: it was split from comm) and `c->err` says on behalf of what; close_ipc_peers unmaps
 * every buffer of a peer this process has opened. */
void abort_comms(lfbm5d_ctx* c, const char* what);
void close_ipc_peers(lfbm5d_ctx* c);

/* HIP-event time of what is enqueued on `s` between begin() and end(), added to stats.ms_comm when the timer goes out of scope --
 * by then the caller has synchronised the stream.  The events are the context's pooled ones: nothing to release on an error return. */
struct CommTimer {
    lfbm5d_ctx* c; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr; bool closed = false;
    hipError_t begin() { e0 = get_event(c); e1 = get_event(c); return hipEventRecord(e0, s); }
    hipError_t end() { closed = true; return hipEventRecord(e1, s); }
    ~CommTimer() { float ms = 0.0f; if (closed && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) c->stats.ms_comm += ms; }
};

} /* namespace lfbm5d_host */
#endif
