// ahc_batch_host.hip — several linkage problems on the host: the block-map and the uniform batch, uniform batches side by side, chains in flight, the
// dispatcher, fa::ahc_run_device_batch (the kernels: ahc_batch.hip; the decisions: ahc_route.h; ahc_ws.h: the map).
#include <memory>

#include "ahc_launch.h"

using namespace fa_ahc;

namespace fa_ahc {   // ahc_route.h's answers under the process's switches (ahc_api.hip plans its workspaces with them)
bool uniform_eligible(int count, const size_t *n, int mode) { return route::uniform_eligible(count, n, mode, fa::sw_on(fa::Sw::AHC_NO_UNIFORM)); }
int uniform_groups(int count, const size_t *n) { return route::uniform_groups(count, n, sw_int(fa::Sw::AHC_UNI_GROUPS)); }
size_t uniform_stride(int count, size_t Nmax, size_t d) {   // bytes of ONE problem's slot in the uniform layout of such a batch
    const int cpt = route::uniform_cpt(0, count, Nmax);
    const size_t Np = route::padded(Nmax, cpt);
    return (make_layout(Nmax, Np, d, route::blocks(Nmax, cpt)).total + 4095) & ~static_cast<size_t>(4095);
}
}  // namespace fa_ahc

namespace {
// What both batch forms do once no problem runs any more.  probs[j] is the caller's problem ord[j].  Finish each, the third event, the sync, the stats (the
// times are the whole batch's), then the problems that met an exact tie at the minimum: one after the other in reference order (every other problem has
// delivered its dendrogram).
fa_status batch_epilogue(fa_ctx *ctx, std::vector<Prob> &probs, const std::vector<int> &ord, hipEvent_t (&ev)[3], fa_ahc_stats *stats, fa_status *statuses,
                         bool *completed) {
    const int count = static_cast<int>(probs.size());
    fa_status worst = FA_SUCCESS;
    auto report = [&](const int j) {
        if (statuses) statuses[ord[j]] = probs[j].st;
        if (probs[j].st != FA_SUCCESS && worst == FA_SUCCESS) worst = probs[j].st;
    };
    for (int j = 0; j < count; ++j) {
        if (probs[j].N >= 2 && probs[j].st == FA_SUCCESS) (void)prob_finish(ctx, probs[j]);
        report(j);
    }
    FA_HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) {
        const Intervals t = intervals_of(ev);
        for (int j = 0; j < count; ++j) stats_fill(stats[ord[j]], probs[j], t);
    }
    for (int j = 0; j < count; ++j) {
        Prob &p = probs[j];
        if (!p.needs_ro || p.st != FA_SUCCESS) continue;
        p.st = ro_run_device(ctx, p.d_data, p.N, p.d, p.d_Z, stats ? &stats[ord[j]] : nullptr, false, p.mode == FA_AHC_MODE_AUTO);
        report(j);
    }
    *completed = true;
    return worst;
}

fa_status batch_reference_order(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, fa_ahc_stats *stats,
                                fa_status *statuses, bool *completed) {   // no batching in this mode: the selection is a serial replay per problem
    fa::WsUse ws_use(ctx);
    fa_status worst = FA_SUCCESS;
    for (int k = 0; k < count; ++k) {
        fa_status st = FA_SUCCESS;
        if (stats) stats[k] = fa_ahc_stats{};
        if (n[k] >= 2) st = ro_run_device(ctx, d_data[k], n[k], d, d_Z[k], stats ? &stats[k] : nullptr);
        if (statuses) statuses[k] = st;
        if (st != FA_SUCCESS && worst == FA_SUCCESS) worst = st;
    }
    *completed = true;
    return worst;
}

// Several independent problems (recordings) advanced by the SAME round launches: one launch = one round of every unfinished
// problem (grid = sum of their blocks), so K serial merge chains share the machine instead of queueing behind each other —
// a chain alone keeps ~N/256 of the 256 CUs busy at one wavefront per SIMD.  Start-up and finish run per problem.
// The launch and the re-capture rule: table of workspaces + block map of the problems still running (rebuilt only when the set changes a lot: finished
// problems' workgroups return after one state load, so a stale map is merely idle workgroups).
struct BlockMapRun {
    fa_ctx *ctx;
    std::vector<Prob> &probs;
    const Ws *d_table;
    int2 *d_map;
    size_t lds;
    bool big;
    std::vector<int2> map;
    int mapped_active = -1, grid = 0;
    bool by_args = false;   // <= kArgProblems running problems: workspaces and block ranges travel in the kernel arguments
    RoundArgs args{};
    std::unique_ptr<RoundGraph> rg;
    void launch(const int ph) const {
        if (by_args) launch_round_args(ctx->stream, big, ph, grid, args, lds);
        else launch_round_map(ctx->stream, big, ph, grid, d_table, d_map, lds);
    }
    fa_status before_replay(RoundGraph *&use, int /* one length: the capture's */) {
        int n_active = 0;
        for (const Prob &p : probs) n_active += p.active ? 1 : 0;
        if (mapped_active < 0 || n_active * 2 <= mapped_active) {   // (re)build the map and the graph over the running problems
            map.clear();
            args = RoundArgs{};
            size_t longest = 0;
            int slot = 0, first = 0;
            by_args = n_active <= kArgProblems;
            for (size_t k = 0; k < probs.size(); ++k) {
                const Prob &p = probs[k];
                if (!p.active) continue;
                for (int b = 0; b < p.w.nblk; ++b) map.push_back(make_int2(static_cast<int>(k), b));
                if (by_args) { args.w[slot] = p.w; args.first_block[slot] = first; first += p.w.nblk; args.first_block[++slot] = first; }
                longest = std::max(longest, p.N);
            }
            args.count = slot;
            grid = static_cast<int>(map.size());
            if (lds > 48 * 1024) { if (by_args) round_args_lds(big, lds); else round_map_lds(big, lds); }
            FA_HIP_TRY(ctx, hipMemcpyAsync(d_map, map.data(), sizeof(int2) * map.size(), hipMemcpyHostToDevice, ctx->stream));
            FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            rg.reset(new RoundGraph());
            rg->capture(ctx, [this](const int ph) { launch(ph); }, route::rounds_for(longest));
            mapped_active = n_active;
        }
        use = rg.get();
        return FA_SUCCESS;
    }
};

fa_status ahc_batch_once(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode,
                         fa_ahc_stats *stats, fa_status *statuses, bool *completed) {
    *completed = false;
    if (mode == FA_AHC_MODE_REFERENCE_ORDER) return batch_reference_order(ctx, count, d_data, n, d, d_Z, stats, statuses, completed);
    std::vector<Prob> probs(static_cast<size_t>(count));
    std::vector<int> ord(static_cast<size_t>(count));   // placement order == the caller's
    std::vector<size_t> at(count, 0);
    size_t total = 0, total_blocks = 0;
    for (int k = 0; k < count; ++k) {
        Prob &p = probs[k];
        ord[k] = k;
        p.N = n[k]; p.d = d; p.Np = route::padded(n[k], 1); p.d_data = d_data[k]; p.d_Z = d_Z[k]; p.mode = mode;
        if (statuses) statuses[k] = FA_SUCCESS;
        p.st = prob_check_shape(ctx, p.N, d);
        if (p.st != FA_SUCCESS || p.N < 2) { p.active = false; continue; }
        p.L = make_layout(p.N, p.Np, d, route::blocks(p.N, 1));
        at[k] = total;
        total += (p.L.total + 4095) & ~static_cast<size_t>(4095);
        total_blocks += route::blocks(p.N, 1);
    }
    const size_t o_table = total;
    total += (sizeof(Ws) * count + 255) & ~static_cast<size_t>(255);
    const size_t o_map = total;
    total += (sizeof(int2) * std::max<size_t>(total_blocks, 1) + 255) & ~static_cast<size_t>(255);
    fa::WsUse ws_use(ctx);
    FA_TRY(fa::ws_acquire(ctx, total));
    char *base = static_cast<char *>(ctx->ahc_ws);
    hipEvent_t ev[3];
    FA_TRY(ctx_events(ctx, ev));
    FA_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
    for (int k = 0; k < count; ++k) {
        Prob &p = probs[k];
        if (!p.active) continue;
        const fa_status st = prob_setup(ctx, p, base + at[k]);
        if (st != FA_SUCCESS) { p.st = st; p.active = false; }
    }
    FA_HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
    std::vector<Ws> table(count);
    long long budget = 64;
    bool big = false;
    for (int k = 0; k < count; ++k) {
        table[k] = probs[k].w;
        if (!probs[k].active) continue;
        big = big || route::single_form(1, probs[k].w.nblk, mode, d, false).big;
        budget = std::max(budget, route::replay_budget(probs[k].N));
    }
    BlockMapRun run{ctx, probs, reinterpret_cast<const Ws *>(base + o_table), reinterpret_cast<int2 *>(base + o_map), sizeof(double) * d, big};
    FA_HIP_TRY(ctx, hipMemcpyAsync(const_cast<Ws *>(run.d_table), table.data(), sizeof(Ws) * count, hipMemcpyHostToDevice, ctx->stream));
    // each state is read before the next replay: before_replay may capture the graph again, from states the replay in front has just delivered
    FA_TRY(drive_rounds(ctx, probs.data(), count, route::drive_plan_batch(kRoundsPerGraph, budget), [&](RoundGraph *&use, const int len) { return run.before_replay(use, len); },
                        [&](const int ph) { run.launch(ph); }));
    return batch_epilogue(ctx, probs, ord, ev, stats, statuses, completed);
}

// The same, with the uniform layout of ahc_round_uni: every problem's workspace has the layout of the LARGEST problem and sits at a constant
// stride, the grid is (blocks of that layout, problems).  Eligible batches (the caller checks: route::uniform_eligible) only.  Problems are placed by size,
// largest first: the running set stays a prefix of the placement, so the grid shrinks in y as the short ones finish.  Per problem the result is the
// single-problem entry's bit for bit (test_uniform_batch_*).
// The launch and the re-capture rule.  The captured launches hold the workspace address, the layout (N of the largest problem, d, slots per thread), the grid
// and the kernel build: the graph of the FIRST capture of a call is kept in the context and reused while all of that is unchanged — a batch job repeats one
// shape, and capture + instantiation of 512 launches is ~3 ms (6 % of a 16 x 1 h call).  The smaller grids of a shrinking batch are captured per call.
struct UniformRun {
    fa_ctx *ctx;
    std::vector<Prob> &probs;   // in placement order
    char *base;
    size_t Nmax, d;
    int cpt;
    unsigned stride_pages;
    Ws w0;
    RoundOffsets offs;
    size_t lds;
    int grid_y = 0, captured_y = -1;
    route::UniKernel kernel = route::kUni;
    RoundGraph *current = nullptr;
    std::unique_ptr<RoundGraph> own;   // the graph of a shrunken grid
    void launch(const int ph) const { launch_round_uni(ctx->stream, kernel, ph, grid_y, w0, offs, stride_pages, lds); }
    fa_status before_replay(RoundGraph *&use, int /* one length: the capture's */) {
        const int count = static_cast<int>(probs.size());
        int last_active = -1;
        size_t longest = 0;
        for (int j = 0; j < count; ++j) if (probs[j].active) { last_active = j; longest = std::max(longest, probs[j].N); }
        // the running set is (nearly) a prefix: shrink the grid when at most half of the captured problems still run
        if (captured_y < 0 || (last_active + 1) * 2 <= captured_y) {
            grid_y = last_active + 1;
            kernel = route::uniform_kernel(cpt, w0.nblk, sw_int(fa::Sw::AHC_UNI_WAVES));
            if (lds > 48 * 1024) round_uni_lds(kernel, lds);
            const int want_rounds = route::rounds_for(longest);
            auto launch_fn = [this](const int ph) { launch(ph); };
            own.reset();
            if (grid_y == count) {   // the full grid of the call: the context's cached graph serves it when nothing it bakes in has changed
                CachedGraph *cg = static_cast<CachedGraph *>(ctx->ahc_uni_graph);
                if (!cg || cg->base != base || cg->N != Nmax || cg->d != d || cg->cpt != cpt || cg->grid_y != grid_y || cg->kernel != kernel || cg->rg.rounds != want_rounds || !cg->rg.ok) {
                    cg = cached_graph_renew(ctx, ctx->ahc_uni_graph);
                    cg->base = base; cg->N = Nmax; cg->d = d; cg->cpt = cpt; cg->grid_y = grid_y; cg->kernel = kernel;
                    cg->rg.capture(ctx, launch_fn, want_rounds);
                }
                current = &cg->rg;
            } else {
                own.reset(new RoundGraph());
                own->capture(ctx, launch_fn, want_rounds);
                current = own.get();
            }
            captured_y = grid_y;
        }
        use = current;
        return FA_SUCCESS;
    }
};

fa_status ahc_batch_uniform(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode,
                            fa_ahc_stats *stats, fa_status *statuses, bool *completed) {
    *completed = false;
    std::vector<int> ord(static_cast<size_t>(count));
    for (int k = 0; k < count; ++k) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return n[a] > n[b]; });
    const size_t Nmax = n[ord[0]];
    const int cpt = route::uniform_cpt(sw_int(fa::Sw::AHC_UNI_CPT), count, Nmax);
    const size_t Npmax = route::padded(Nmax, cpt);
    FA_TRY(prob_check_shape(ctx, Nmax, d));
    const Layout L = make_layout(Nmax, Npmax, d, route::blocks(Nmax, cpt));
    const size_t stride = (L.total + 4095) & ~static_cast<size_t>(4095);
    if ((stride >> 12) > 0xffffffffull) return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "ahc: workspace stride too large");
    fa::WsUse ws_use(ctx);
    FA_TRY(fa::ws_acquire(ctx, stride * static_cast<size_t>(count)));
    char *base = static_cast<char *>(ctx->ahc_ws);
    std::vector<Prob> probs(static_cast<size_t>(count));     // in placement order
    hipEvent_t ev[3];
    FA_TRY(ctx_events(ctx, ev));
    FA_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
    for (int j = 0; j < count; ++j) {
        Prob &p = probs[j];
        const int k = ord[j];
        p.N = n[k]; p.d = d; p.Np = Npmax; p.cpt = cpt; p.d_data = d_data[k]; p.d_Z = d_Z[k]; p.mode = mode; p.L = L;
        if (statuses) statuses[k] = FA_SUCCESS;
        // every problem of the grid gets workgroups, so every state must be initialised: a set-up that fails (a failing launch or copy: the device
        // is in trouble) fails the batch, the caller's splitting logic takes over
        FA_TRY(prob_setup(ctx, p, base + stride * static_cast<size_t>(j)));
    }
    FA_HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
    UniformRun run{ctx, probs, base, Nmax, d, cpt, static_cast<unsigned>(stride >> 12), probs[0].w, round_offsets(probs[0].w), sizeof(double) * d};
    FA_TRY(drive_rounds(ctx, probs.data(), count, route::drive_plan_batch(route::rounds_for(Nmax), route::replay_budget(Nmax)),   // no replay queued ahead: see ahc_batch_once
                        [&](RoundGraph *&use, const int len) { return run.before_replay(use, len); },
                        [&](const int ph) { run.launch(ph); }));
    return batch_epilogue(ctx, probs, ord, ev, stats, statuses, completed);
}

fa_status ensure_helper(fa_ctx *ctx, const int i) {   // helper context i of ctx (own stream, own workspace): created on first use, with the caller's limits
    fa_ctx *&h = ctx->helpers[i];
    if (h) return FA_SUCCESS;
    const fa_status st = fa_ctx_create(ctx->device, nullptr, &h);
    if (st != FA_SUCCESS) { h = nullptr; return st; }
    h->ws_limit = ctx->ws_limit;
    h->ws_cap = ctx->ws_cap;
    return FA_SUCCESS;
}

// Status contract: statuses[k] is the outcome of problem k whatever happens.  An early failure of the batch as a whole (workspace
// allocation, an event, a copy, a graph replay) marks EVERY problem that was to run with that failure — round 2 left them at SUCCESS
// and the callers went on to cut dendrograms that were never written.  When the combined workspace of the batch (sum of N_k^2 * 8 B)
// does not fit, the batch is split in halves down to single problems before anything is reported as ALLOCATION_FAILURE.

// A few LARGE problems: their merge chains run CONCURRENTLY, problem 0 on the caller's context and every other one on a helper context
// (own stream, own workspace, a host thread each) — not as one batched chain.  The chain of a large problem is latency-bound (N - 1
// dependent launches on ~N/256 of the 256 CUs, one wavefront per SIMD), so independent chains overlap almost freely: two recordings of
// 43 200 embeddings take 0.29 s this way against 0.36 s as one batched chain and 0.50 s one after the other; four take 0.37 s (one
// hardware queue each: GPU_MAX_HW_QUEUES >= 8 in the process environment helps, profiles/r03_e2e_in_flight.json).  Many SMALL problems
// are the opposite case (a chain of a 5 400-point problem occupies 22 CUs): those stay batched.
fa_status ahc_batch_in_flight(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode,
                              fa_ahc_stats *stats, fa_status *sts) {
    for (int k = 1; k < count; ++k) {
        const fa_status st = ensure_helper(ctx, k - 1);
        if (st != FA_SUCCESS) return fa::set_error(ctx, st, "ahc: cannot create a helper context");
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the inputs were produced on the caller's stream
    std::vector<std::thread> threads;
    for (int k = 1; k < count; ++k) {
        try {
            threads.emplace_back([&, k]() {
                fa_ctx *h = ctx->helpers[k - 1];
                try {                            // nothing may leave a host thread; ALLOCATION_FAILURE sends the problem to the caller's context below
                    fa::DeviceGuard guard(h->device);
                    sts[k] = fa::ahc_run_device(h, d_data[k], n[k], d, d_Z[k], mode, stats ? &stats[k] : nullptr, false);
                } catch (...) { sts[k] = FA_ALLOCATION_FAILURE; }
            });
        } catch (...) {                          // no thread to be had (std::system_error): that problem runs on the caller's context below
            sts[k] = FA_ALLOCATION_FAILURE;
        }
    }
    sts[0] = fa::ahc_run_device(ctx, d_data[0], n[0], d, d_Z[0], mode, stats ? &stats[0] : nullptr, false);
    for (auto &t : threads) t.join();
    fa_status first = sts[0];
    for (int k = 1; k < count; ++k) {
        if (sts[k] == FA_ALLOCATION_FAILURE) {   // HBM pressure (or no thread): this one runs alone on the caller's context (whose workspace is free again)
            (void)fa_ctx_trim(ctx->helpers[k - 1]);
            sts[k] = fa::ahc_run_device(ctx, d_data[k], n[k], d, d_Z[k], mode, stats ? &stats[k] : nullptr, false);
        }
        if (sts[k] != FA_SUCCESS && ctx->last_error.empty()) ctx->last_error = ctx->helpers[k - 1]->last_error;
        if (first == FA_SUCCESS) first = sts[k];
    }
    return first;
}

fa_status run_device_batch_impl(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode, fa_ahc_stats *stats,
                                fa_status *statuses, bool allow_groups);

// Many LARGE recordings: G uniform batches side by side (round 4).  A uniform batch costs a fixed ~5.3 us per round (kernel boundary + two dependent
// memory round trips: latency) plus ~0.75 us of instruction issue per problem; two batches of K / 2 problems on two streams fill each other's
// latency: 8 recordings of 8 h advance in ~7.5 us per round of both instead of 11 us as one batch.  Group 0 runs on the caller's context, the
// others on its helper contexts (own stream, own workspace, a host thread each — the round-3 in-flight machinery, but with 2 streams instead of
// one per recording, so that two free hardware queues suffice).  A group that cannot get its workspace (or its thread) is run afterwards on the
// caller's context.  How many groups: route::uniform_groups.
fa_status ahc_batch_uniform_groups(fa_ctx *ctx, int groups, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode,
                                   fa_ahc_stats *stats, fa_status *sts) {
    for (int g = 1; g < groups; ++g) if (ensure_helper(ctx, g - 1) != FA_SUCCESS) { groups = g; break; }
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the inputs were produced on the caller's stream
    std::vector<int> first(static_cast<size_t>(groups) + 1, 0);
    for (int g = 0; g <= groups; ++g) first[g] = static_cast<int>(static_cast<long long>(count) * g / groups);
    std::vector<char> done(static_cast<size_t>(groups), 0);
    auto run_group = [&](fa_ctx *c, const int g) {
        const int a = first[g], m = first[g + 1] - first[g];
        bool completed = false;
        try {                                    // nothing may leave a host thread: an exception there would end the process
            fa::DeviceGuard guard(c->device);
            (void)ahc_batch_uniform(c, m, d_data + a, n + a, d, d_Z + a, mode, stats ? stats + a : nullptr, sts + a, &completed);
        } catch (...) { completed = false; }
        done[static_cast<size_t>(g)] = completed ? 1 : 0;
    };
    std::vector<std::thread> threads;
    for (int g = 1; g < groups; ++g) {
        try { threads.emplace_back(run_group, ctx->helpers[g - 1], g); }
        catch (...) { done[static_cast<size_t>(g)] = 0; }   // no thread to be had: that group runs on the caller's context below
    }
    run_group(ctx, 0);
    for (auto &t : threads) t.join();
    fa_status worst = FA_SUCCESS;
    for (int g = 0; g < groups; ++g) {
        const int a = first[g], m = first[g + 1] - first[g];
        if (!done[static_cast<size_t>(g)]) {               // workspace / thread trouble: alone on the caller's context, through the general dispatcher (it splits further)
            if (g > 0 && ctx->helpers[g - 1]) (void)fa_ctx_trim(ctx->helpers[g - 1]);
            (void)run_device_batch_impl(ctx, m, d_data + a, n + a, d, d_Z + a, mode, stats ? stats + a : nullptr, sts + a, false);
        } else if (g > 0 && ctx->last_error.empty()) {
            for (int k = a; k < a + m; ++k) if (sts[k] != FA_SUCCESS) { ctx->last_error = ctx->helpers[g - 1]->last_error; break; }
        }
        for (int k = a; k < a + m; ++k) if (sts[k] != FA_SUCCESS && worst == FA_SUCCESS) worst = sts[k];
    }
    return worst;
}

// A problem the matrix-based rounds cannot hold (more points than block records: N > 196 608) runs alone through the single-problem entry,
// which takes the matrix-free route (fluidaudio_hip.h promises that; inside a batch such a problem used to be marked ALLOCATION_FAILURE and the
// clustering stage degraded its recording to singletons).  The others stay a batch.
fa_status batch_with_oversize(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode, fa_ahc_stats *stats,
                              fa_status *sts, const bool allow_groups) {
    std::vector<int> small;
    fa_status worst = FA_SUCCESS;
    for (int k = 0; k < count; ++k) {
        if (route::fits_matrix(n[k]) || n[k] < 2) { small.push_back(k); continue; }
        sts[k] = fa::ahc_run_device(ctx, d_data[k], n[k], d, d_Z[k], mode, stats ? &stats[k] : nullptr, false);
        if (sts[k] != FA_SUCCESS && worst == FA_SUCCESS) worst = sts[k];
    }
    if (small.empty()) return worst;
    const int m = static_cast<int>(small.size());
    std::vector<const double *> dd(m);
    std::vector<size_t> nn(m);
    std::vector<double *> zz(m);
    std::vector<fa_ahc_stats> ss(m);
    std::vector<fa_status> st2(m, FA_SUCCESS);
    for (int j = 0; j < m; ++j) { dd[j] = d_data[small[j]]; nn[j] = n[small[j]]; zz[j] = d_Z[small[j]]; }
    const fa_status r = run_device_batch_impl(ctx, m, dd.data(), nn.data(), d, zz.data(), mode, stats ? ss.data() : nullptr, st2.data(), allow_groups);
    for (int j = 0; j < m; ++j) { sts[small[j]] = st2[j]; if (stats) stats[small[j]] = ss[j]; }
    return r != FA_SUCCESS && worst == FA_SUCCESS ? r : worst;
}

fa_status run_device_batch_impl(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode, fa_ahc_stats *stats,
                                fa_status *statuses, const bool allow_groups) {
    if (count <= 0) return FA_SUCCESS;
    std::vector<fa_status> local(static_cast<size_t>(count), FA_SUCCESS);
    fa_status *sts = statuses ? statuses : local.data();
    // chains in flight on helper contexts (round 3) only on request since round 4: the uniform-layout batch advances the same problems by
    // ONE launch per round, on one stream — its rate does not depend on which hardware queues the process's streams landed on
    const route::BatchRoute r = route::batch_route(count, n, mode, allow_groups, ctx->ws_cap != static_cast<size_t>(-1), fa::sw_on(fa::Sw::AHC_IN_FLIGHT),
                                                   sw_int(fa::Sw::AHC_UNI_GROUPS), fa::sw_on(fa::Sw::AHC_NO_UNIFORM));
    if (r.route == route::Route::kOversize) return batch_with_oversize(ctx, count, d_data, n, d, d_Z, mode, stats, sts, allow_groups);
    if (r.route == route::Route::kGroups) return ahc_batch_uniform_groups(ctx, r.groups, count, d_data, n, d, d_Z, mode, stats, sts);
    if (r.route == route::Route::kInFlight) return ahc_batch_in_flight(ctx, count, d_data, n, d, d_Z, mode, stats, sts);
    bool completed = false;
    const fa_status st = r.route == route::Route::kUniform ? ahc_batch_uniform(ctx, count, d_data, n, d, d_Z, mode, stats, sts, &completed)
                                                           : ahc_batch_once(ctx, count, d_data, n, d, d_Z, mode, stats, sts, &completed);
    if (completed) return st;
    const fa_status fail = st != FA_SUCCESS ? st : FA_RUNTIME_ERROR;
    if (fail == FA_ALLOCATION_FAILURE && count > 1) {
        const int half = count / 2;
        const fa_status a = run_device_batch_impl(ctx, half, d_data, n, d, d_Z, mode, stats, sts, allow_groups);
        const fa_status b = run_device_batch_impl(ctx, count - half, d_data + half, n + half, d, d_Z + half, mode, stats ? stats + half : nullptr, sts + half, allow_groups);
        return a != FA_SUCCESS ? a : b;
    }
    if (fail == FA_ALLOCATION_FAILURE && count == 1 && n[0] >= 2)   // not even one matrix fits: the single-problem entry knows the matrix-free route
        return sts[0] = fa::ahc_run_device(ctx, d_data[0], n[0], d, d_Z[0], mode, stats ? &stats[0] : nullptr, false);
    for (int k = 0; k < count; ++k) {
        if (n[k] >= 2) sts[k] = fail;
        if (stats) stats[k] = fa_ahc_stats{};
    }
    return fail;
}
}  // namespace

fa_status fa::ahc_run_device_batch(fa_ctx *ctx, int count, const double *const *d_data, const size_t *n, size_t d, double *const *d_Z, int mode,
                                   fa_ahc_stats *stats, fa_status *statuses) {
    return run_device_batch_impl(ctx, count, d_data, n, d, d_Z, mode, stats, statuses, true);
}
