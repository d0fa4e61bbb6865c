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
    RoundGraph rg;
    const void *base = nullptr;
    size_t N = 0, d = 0;
    int cpt = 1;
    bool spec = false;            // the speculative round (FA_AHC_SPEC)
    int grid_y = 0, kernel = 0;   // uniform batches: problems in the grid and which build of the round serves them
};
CachedGraph *cached_graph_renew(fa_ctx *ctx, void *&slot);   // ahc_rounds_host.hip: an empty one in the context's `slot` (ahc_graph / ahc_uni_graph), the old one freed

// ---- the drive loop: replays until no problem of the set is active or `budget` replays are spent.  Per replay: before_replay(rg) hands out the graph to
// replay — (re)captured by the caller's own rule; nullptr: launch(0) IS the replay (the single-block form: all its rounds in one launch) —, the replay, one
// state copy per running problem, ONE synchronisation, prob_after_replay for each (a problem's failure is its p.st; only a failing call ends the loop).
template <class Before, class Launch>
fa_status drive_rounds(fa_ctx *ctx, Prob *probs, const int count, const long long budget, Before &&before_replay, Launch &&launch) {
    for (long long it = 0; it < budget; ++it) {
        bool any = false;
        for (int j = 0; j < count; ++j) any = any || probs[j].active;
        if (!any) break;
        RoundGraph *rg = nullptr;
        FA_TRY(before_replay(rg));
        if (rg) FA_TRY(rg->replay(ctx, launch));
        else { launch(0); FA_HIP_TRY(ctx, hipGetLastError()); }
        for (int j = 0; j < count; ++j)
            if (probs[j].active) FA_HIP_TRY(ctx, hipMemcpyAsync(&probs[j].h, probs[j].w.state, sizeof(AhcState), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int j = 0; j < count; ++j) if (probs[j].active) (void)prob_after_replay(ctx, probs[j]);
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
