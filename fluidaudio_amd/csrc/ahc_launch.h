// ahc_launch.h — what the kernel units of the linkage (ahc_rounds.hip, ahc_batch.hip) and its host units (ahc_rounds_host.hip, ahc_batch_host.hip, the
// reference-order runs) share: the launchers and their operands, the graph of round launches, the drive loop over replays and the stats fill
// (ahc_ws.h: the map).  Which kernel of a family a launcher starts is an enumerator of ahc_route.h.
#pragma once
#include "ahc_ws.h"

namespace fa_ahc {

inline int sw_int(const fa::Sw s) { const char *e = fa::sw(s); return e ? atoi(e) : 0; }   // a numeric switch, parsed for ahc_route.h (0: not set)

// ---- operands
struct RoundOffsets { unsigned row, node, e2, flags; };   // the small arrays, relative to the state: within 4 GB of it (make_layout puts the matrix last)
inline RoundOffsets round_offsets(const Ws &w) {
    auto off_of = [&](const void *p) { return static_cast<unsigned>(static_cast<const char *>(p) - reinterpret_cast<const char *>(w.state)); };
    return {off_of(w.row), off_of(w.node), off_of(w.e2), off_of(w.flags)};
}
constexpr int kArgProblems = 16;
struct RoundArgs {   // operands of the argument-table round
    Ws w[kArgProblems];
    int32_t first_block[kArgProblems + 1];   // workgroups [first_block[k], first_block[k + 1]) work on problem k
    int32_t count, pad;
};
static_assert(sizeof(RoundArgs) <= 3584, "kernel arguments are limited to 4 KB");

// ---- launchers (no synchronisation, no error check: the caller's).  `*_lds` raises the chosen kernel's dynamic LDS limit to a centroid buffer above 48 KB.
inline void kernel_lds(const void *kernel, const size_t lds) { (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)); (void)hipGetLastError(); }
// ahc_rounds.hip
void launch_round_single(hipStream_t st, route::SingleKernel kernel, int ph, const Ws &w, const RoundOffsets &o, size_t lds);   // one round of one problem
void round_single_lds(route::SingleKernel kernel, size_t lds);
void launch_single_block(hipStream_t st, int cpt, const Ws &w, int rounds, size_t lds);   // `rounds` rounds of a one-block problem in one launch
void single_block_lds(int cpt, size_t lds);
void launch_records(hipStream_t st, int cpt, const Ws &w);   // block records of both parities from the row arrays (needs eps)
void launch_heights(hipStream_t st, const Ws &w);
void launch_adopt(hipStream_t st, const Ws &w, int merges, double eps, const double *pair_a, const double *pair_b);   // state record + row states of an adopted clustering
// ahc_batch.hip
void launch_round_map(hipStream_t st, bool big, int ph, int grid, const Ws *d_table, const int2 *d_map, size_t lds);    // problems found through a block map
void round_map_lds(bool big, size_t lds);
void launch_round_args(hipStream_t st, bool big, int ph, int grid, const RoundArgs &a, size_t lds);                     // <= kArgProblems problems in the arguments
void round_args_lds(bool big, size_t lds);
void launch_round_uni(hipStream_t st, route::UniKernel kernel, int ph, int grid_y, const Ws &w0, const RoundOffsets &o, unsigned stride_pages, size_t lds);
void round_uni_lds(route::UniKernel kernel, size_t lds);

// ---- the graph of round launches
struct RoundGraph {   // `rounds` rounds captured once, replayed until every problem reports done
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = false;
    int rounds = kRoundsPerGraph;
    ~RoundGraph() { if (exec) (void)hipGraphExecDestroy(exec); if (graph) (void)hipGraphDestroy(graph); }
    template <class Launch> void capture(fa_ctx *ctx, Launch &&launch, const int n_rounds) {
        ok = true;
        rounds = n_rounds;
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            for (int i = 0; i < rounds; ++i) launch(i & 3);
            if (hipStreamEndCapture(ctx->stream, &graph) != hipSuccess || !graph) ok = false;
            else if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) ok = false;
        } else ok = false;
        (void)hipGetLastError();
    }
    template <class Launch> fa_status replay(fa_ctx *ctx, Launch &&launch) {
        if (ok) FA_HIP_TRY(ctx, hipGraphLaunch(exec, ctx->stream));
        else for (int i = 0; i < rounds; ++i) launch(i & 3);
        return FA_SUCCESS;
    }
};
struct CachedGraph {   // the round launches of one problem shape, kept in the context between calls
    RoundGraph rg;                // the full length: rounds_for(N)
    RoundGraph shorter[route::kRungs - 1];   // the single-problem route's shorter replays (route::kLadder[1 ..]), captured with rg when route::rungs_for(N) > 1
    const void *base = nullptr;
    size_t N = 0, d = 0;
    int cpt = 1;
    bool spec = false;            // the speculative round (FA_AHC_SPEC)
    int grid_y = 0, kernel = 0;   // uniform batches: problems in the grid and which build of the round serves them
    RoundGraph *of_length(const int rounds) {   // the captured replay of `rounds` rounds (a length route::plan_next hands out)
        if (rounds != rg.rounds) for (RoundGraph &g : shorter) if (g.ok && g.rounds == rounds) return &g;
        return &rg;
    }
};
CachedGraph *cached_graph_renew(fa_ctx *ctx, void *&slot);   // ahc_rounds_host.hip: an empty one in the context's `slot` (ahc_graph / ahc_uni_graph), the old one freed

// ---- the drive loop: replays until no problem of the set is active or the plan's budget is spent.  Per replay: before_replay(rg, rounds) hands out the
// graph to replay — `rounds` is the length the plan asks for (a batch has one length and (re)captures by the caller's own rule); nullptr: launch(0) IS the
// replay (the single-block form: all its rounds in one launch) —, the replay, one state copy per running problem, ONE wait, prob_after_replay for each (a
// problem's failure is its p.st; only a failing call ends the loop).
// A plan of depth 1 (the batches; FA_AHC_SYNC_DRIVE) waits for the stream, with the states copied to Prob::h.  A deeper plan enqueues the next replay BEFORE
// that wait while route::plan_next allows it, so the stream is not empty while the host reads a state and launches a graph of hundreds of nodes: each
// replay's state then goes into its own slot of the context's pinned ring, followed by the slot's event, and the host waits for the OLDEST event.  (The
// ring is not used at depth 1: a batch of 16 problems pays 16 pinned copies per replay, measurably more than the pageable ones in front of a
// synchronisation.)  A replay that runs behind a `halt` or a `done` carries the state forward, like the rest of a replay does; whatever is still queued when
// the loop ends is waited for before it returns.
inline fa_status drive_ring(fa_ctx *ctx, const int count) {   // the ring holds kQueueDepth slots of `count` states
    const size_t slot = (sizeof(AhcState) * static_cast<size_t>(count) + 255) & ~static_cast<size_t>(255);
    if (ctx->ahc_ring_slot_bytes < slot) {
        if (ctx->ahc_ring) { FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipHostFree(ctx->ahc_ring); ctx->ahc_ring = nullptr; ctx->ahc_ring_slot_bytes = 0; }
        FA_HIP_TRY(ctx, hipHostMalloc(&ctx->ahc_ring, slot * route::kQueueDepth, hipHostMallocDefault));
        ctx->ahc_ring_slot_bytes = slot;
    }
    for (auto &e : ctx->ahc_ring_ev) if (!e) FA_HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return FA_SUCCESS;
}
template <class Before, class Launch>
fa_status drive_rounds(fa_ctx *ctx, Prob *probs, const int count, route::DrivePlan plan, Before &&before_replay, Launch &&launch) {
    static_assert(route::kQueueDepth == 2, "the context keeps two ring slots and two events");
    const bool ahead = plan.depth > 1;
    if (ahead) FA_TRY(drive_ring(ctx, count));
    struct Drain {   // nothing of this loop is in flight once it has returned, whichever way
        fa_ctx *ctx; route::DrivePlan &plan;
        ~Drain() { if (plan.queued > 0) (void)hipStreamSynchronize(ctx->stream); }
    } drain{ctx, plan};
    auto slot_of = [&](const int i) { return reinterpret_cast<AhcState *>(static_cast<char *>(ctx->ahc_ring) + ctx->ahc_ring_slot_bytes * static_cast<size_t>(i)); };
    int head = 0;   // ring slot of the oldest replay in flight
    for (;;) {
        bool any = false;
        for (int j = 0; j < count; ++j) any = any || probs[j].active;
        while (any) {
            const int rounds = route::plan_next(plan);
            if (!rounds) break;
            const int at = (head + plan.queued - 1) % route::kQueueDepth;
            RoundGraph *rg = nullptr;
            FA_TRY(before_replay(rg, rounds));
            if (rg) FA_TRY(rg->replay(ctx, launch));
            else { launch(0); FA_HIP_TRY(ctx, hipGetLastError()); }
            for (int j = 0; j < count; ++j)
                if (probs[j].active) FA_HIP_TRY(ctx, hipMemcpyAsync(ahead ? slot_of(at) + j : &probs[j].h, probs[j].w.state, sizeof(AhcState), hipMemcpyDeviceToHost, ctx->stream));
            if (ahead) FA_HIP_TRY(ctx, hipEventRecord(ctx->ahc_ring_ev[at], ctx->stream));
        }
        if (!plan.queued) break;   // nothing active, or the budget is spent
        if (ahead) FA_HIP_TRY(ctx, hipEventSynchronize(ctx->ahc_ring_ev[head]));
        else FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int j = 0; j < count; ++j) if (probs[j].active) { if (ahead) probs[j].h = slot_of(head)[j]; (void)prob_after_replay(ctx, probs[j]); }
        route::plan_retire(plan, static_cast<long long>(probs[0].N) - 1 - probs[0].h.step);
        head = (head + 1) % route::kQueueDepth;
    }
    return FA_SUCCESS;
}

// ---- stats: init_ms / merge_ms are the intervals between the three events of a run (of the whole batch, for a batch)
struct Intervals { float init_ms = 0, merge_ms = 0; };
inline Intervals intervals_of(hipEvent_t (&ev)[3]) {
    Intervals t;
    (void)hipEventElapsedTime(&t.init_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&t.merge_ms, ev[1], ev[2]);
    return t;
}
inline void stats_fill(fa_ahc_stats &o, const Prob &p, const Intervals &t) {   // what the filter-based rounds did with p
    o = fa_ahc_stats{};
    o.merges = p.h.step; o.rounds = p.h.rounds; o.rescans = p.h.rescans; o.exact_fallback = p.fallback; o.windows = p.h.windows;
    o.init_ms = t.init_ms; o.merge_ms = t.merge_ms; o.total_ms = t.init_ms + t.merge_ms;
}
// a reference-order run adds its scans and its time to what an attempt of the rounds before it has left
inline void stats_add(fa_ahc_stats &o, const int merges, const long long rounds, const long long rescans, const long long windows, const Intervals &t) {
    o.merges = merges; o.rounds += rounds; o.rescans += rescans; o.windows += windows;
    if (!o.reference_order) o.reference_order = 1;
    o.init_ms += t.init_ms; o.merge_ms += t.merge_ms; o.total_ms += t.init_ms + t.merge_ms;
}

}  // namespace fa_ahc
