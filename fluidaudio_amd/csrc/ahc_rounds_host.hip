// ahc_rounds_host.hip — the filter-based linkage of ONE problem on the host: set-up / replay / finish, the cached graph, fa::ahc_run_device
// (the kernels: ahc_rounds.hip; ahc_ws.h: the map).
#include "ahc_launch.h"

using namespace fa_ahc;

namespace fa_ahc {
void window_counter_init(WinCounters (&c)[4]) { for (auto &x : c) { x.stale_key = ~0ULL; x.ncand = 0; x.npairs = 0; } }

fa_status prob_check_shape(fa_ctx *ctx, size_t N, size_t d) {
    if (!route::fits_matrix(N)) return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "ahc: N too large for the resident distance matrix");
    if (d * sizeof(double) > 60 * 1024) return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "ahc: dimension too large for the LDS centroid buffer");
    return FA_SUCCESS;
}

// binds the workspace at `base`, uploads the initial state and runs the start-up kernels (matrix, row minima, records, eps)
void prob_bind(Prob &p, char *base) {
    const size_t N = p.N, d = p.d, Np = p.Np;
    const Layout &L = p.L;
    p.base = base;
    Ws &w = p.w;
    w = Ws{};
    w.state = reinterpret_cast<AhcState *>(base + L.state);
    w.cnt = reinterpret_cast<WinCounters *>(base + L.cnt);
    w.flags = reinterpret_cast<int32_t *>(base + L.flags);
    w.prof = reinterpret_cast<unsigned long long *>(base + L.prof);
    w.recA = reinterpret_cast<RecA *>(base + L.reca);
    w.recI = reinterpret_cast<int4 *>(base + L.reci);
    w.recS = reinterpret_cast<RecS *>(base + L.recs);
    w.recP = reinterpret_cast<RecP *>(base + L.recp);
    w.row = reinterpret_cast<RowSt *>(base + L.row);
    w.e2 = reinterpret_cast<double *>(base + L.e2);
    w.node = reinterpret_cast<int32_t *>(base + L.node);
    w.sizes = reinterpret_cast<double *>(base + L.sizes);
    w.Z = reinterpret_cast<double *>(base + L.z);
    w.cand = reinterpret_cast<int2 *>(base + L.cand);
    w.pairs = reinterpret_cast<int4 *>(base + L.pairs);
    w.C = reinterpret_cast<double *>(base + L.c);
    w.XT = reinterpret_cast<double *>(base + L.xt);
    w.M = reinterpret_cast<double *>(base + L.m);
    w.N = static_cast<int32_t>(N); w.Np = static_cast<int32_t>(Np); w.d = static_cast<int32_t>(d); w.nblk = static_cast<int32_t>(Np / (static_cast<size_t>(kBlk) * p.cpt));
}

fa_status prob_setup(fa_ctx *ctx, Prob &p, char *base) {
    prob_bind(p, base);
    const size_t N = p.N, d = p.d, Np = p.Np;
    const Layout &L = p.L;
    Ws &w = p.w;
    const int dev_mode = p.mode == FA_AHC_MODE_EXACT ? FA_AHC_MODE_EXACT : FA_AHC_MODE_AUTO;
    FA_HIP_TRY(ctx, hipMemcpyAsync(w.C, p.d_data, sizeof(double) * N * d, hipMemcpyDeviceToDevice, ctx->stream));
    startup_filter(ctx->stream, w, L, base, dev_mode, p.d_data, N, Np, d);   // ahc_startup.hip: state, rows, transpose, matrix, row minima, eps
    launch_records(ctx->stream, p.cpt, w);   // window counts need eps
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipMemsetAsync(spec_of(w.state), 0, sizeof(AhcSpec), ctx->stream));   // no merge speculated yet: the first round takes the one-merge path
    return FA_SUCCESS;
}

// p.h holds the state after a replay of the round graph: finished, failed, or to be switched to exact rows
fa_status prob_after_replay(fa_ctx *ctx, Prob &p) {
    p.h.rounds = p.h.rounds32;   // the round counter travels in the hot state
    const AhcState &h = p.h;
    if (h.error == 1) { p.active = false; return p.st = fa::set_error(ctx, FA_RUNTIME_ERROR, "ahc: NaN distance"); }
    if (h.error) { p.active = false; return p.st = fa::set_error(ctx, FA_RUNTIME_ERROR, "ahc: internal selection failure (%d)", h.error); }
    if (h.done) { p.active = false; return FA_SUCCESS; }
    if (h.halt && h.need_exact) {
        // An exact tie at the minimum (need_exact 2) or a window overflowing with near-ties (1: duplicated / quantised inputs).  Which of
        // several exactly tied pairs the reference merges is decided by its heap (ahc_reforder.h), so the problem is recomputed in
        // reference order by the caller.  (Round 2 continued with exact rows and its own tie order here: same heights and partitions on
        // duplicates, but a different row order — and, where tied pairs overlap, possibly a different tree.)
        ++p.fallback;
        p.needs_ro = true;
        p.active = false;
        return FA_SUCCESS;
    } else if (h.halt) { p.active = false; return p.st = fa::set_error(ctx, FA_RUNTIME_ERROR, "ahc: halted without a reason"); }
    return FA_SUCCESS;
}

fa_status prob_finish(fa_ctx *ctx, Prob &p) {   // heights from the stored centroids, dendrogram to the caller's device buffer
    if (p.st != FA_SUCCESS) return p.st;
    if (p.needs_ro) return FA_SUCCESS;   // recomputed by ro_run_device
    if (!p.h.done) return p.st = fa::set_error(ctx, FA_RUNTIME_ERROR, "ahc: round budget exhausted at step %d", p.h.step);
    int32_t hflag = 0;
    launch_heights(ctx->stream, p.w);
    FA_HIP_TRY(ctx, hipMemcpyAsync(p.d_Z, p.w.Z, sizeof(double) * 4 * (p.N - 1), p.z_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(&hflag, p.w.flags, sizeof(hflag), hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (hflag) return p.st = fa::set_error(ctx, FA_RUNTIME_ERROR, "ahc: NaN distance");
    return FA_SUCCESS;
}


CachedGraph *cached_graph_renew(fa_ctx *ctx, void *&slot) {
    delete static_cast<CachedGraph *>(slot);
    CachedGraph *cg = new CachedGraph();
    slot = cg;
    ctx->ahc_graph_free = [](void *p) { delete static_cast<CachedGraph *>(p); };
    return cg;
}
fa_status ctx_events(fa_ctx *ctx, hipEvent_t (&ev)[3]) {
    for (int i = 0; i < 3; ++i) {
        if (!ctx->ahc_ev[i]) FA_HIP_TRY(ctx, hipEventCreate(&ctx->ahc_ev[i]));
        ev[i] = ctx->ahc_ev[i];
    }
    return FA_SUCCESS;
}

fa_status prob_adopt(fa_ctx *ctx, Prob &p, const int merges, const double eps, const double *pair_a, const double *pair_b) {
    const Ws &w = p.w;
    if (p.cpt != 1 || merges < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "ahc: nothing to adopt");
    launch_adopt(ctx->stream, w, merges, eps, pair_a, pair_b);
    launch_records(ctx->stream, 1, w);   // needs eps (the state) and the rows
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipMemsetAsync(spec_of(w.state), 0, sizeof(AhcSpec), ctx->stream));   // no hypothesis survives an adoption
    p.h.step = merges;   // what the drive plan of prob_run_rounds counts from
    return FA_SUCCESS;
}

fa_status prob_run_rounds(fa_ctx *ctx, Prob &p) {
    const size_t N = p.N, d = p.d, lds = sizeof(double) * d;
    const Ws w = p.w;
    const route::RoundForm form = route::single_form(p.cpt, w.nblk, p.mode, d, [] { const char *e = fa::sw(fa::Sw::AHC_SPEC); return !(e && e[0] == '0' && e[1] == 0); }());
    const RoundOffsets offs = round_offsets(w);
    const bool single_block = w.nblk == 1 && !fa::sw_on(fa::Sw::AHC_NO_SINGLE_BLOCK);
    const int rounds = route::rounds_for(N);
    if (lds > 48 * 1024) { if (single_block) single_block_lds(p.cpt, lds); else round_single_lds(form.kernel, lds); }
    auto launch = [&](const int ph) {
        if (single_block) launch_single_block(ctx->stream, p.cpt, w, rounds, lds);   // all rounds of a replay in one launch
        else launch_round_single(ctx->stream, form.kernel, ph, w, offs, lds);
    };
    // The captured graphs only hold launch parameters (workspace pointers, block count): they are reused as long as the workspace sits at
    // the same address and the shape is the same — repeated calls on recordings of one length skip capture + instantiation.  A problem whose replay
    // has the full length gets the ladder of shorter replays with it (route::kLadder), whichever drive this call uses.
    CachedGraph *cg = nullptr;
    if (!single_block) {
        cg = static_cast<CachedGraph *>(ctx->ahc_graph);
        if (!cg || cg->base != ctx->ahc_ws || cg->N != N || cg->d != d || cg->cpt != p.cpt || cg->spec != form.spec || !cg->rg.ok) {
            cg = cached_graph_renew(ctx, ctx->ahc_graph);
            cg->base = ctx->ahc_ws; cg->N = N; cg->d = d; cg->cpt = p.cpt; cg->spec = form.spec;
            cg->rg.capture(ctx, launch, rounds);
            for (int r = 1; r < route::rungs_for(N); ++r) cg->shorter[r - 1].capture(ctx, launch, route::kLadder[r]);
        }
    }
    route::DrivePlan plan = route::drive_plan(N, p.h.step, form.spec, fa::sw_on(fa::Sw::AHC_SYNC_DRIVE));
    if (!cg) plan.ladder = false;   // the single-block form: launch(0) runs rounds_for(N) rounds
    else for (int r = 1; r < route::rungs_for(N); ++r) if (!cg->shorter[r - 1].ok) plan.ladder = false;   // a rung that could not be captured: one length
    FA_TRY(drive_rounds(ctx, &p, 1, plan, [&](RoundGraph *&use, const int len) { use = cg ? cg->of_length(len) : nullptr; return FA_SUCCESS; }, launch));
    if (p.st != FA_SUCCESS) return p.st;
    p.spec_hits = 0;
    if (fa::sw_on(fa::Sw::AHC_DEBUG) || fa_debug_hooks_enabled()) {   // the commit counter: only for the debug line and the test hook (one more copy)
        if (form.spec) {
            long long hits = 0;
            FA_HIP_TRY(ctx, hipMemcpyAsync(&hits, &spec_of(w.state)->hits, sizeof(hits), hipMemcpyDeviceToHost, ctx->stream));
            FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            p.spec_hits = hits;
        }
        ctx->ahc_spec_hits = p.spec_hits;
    }
    return prob_finish(ctx, p);
}
}  // namespace fa_ahc

namespace {
void print_profile(const Prob &p) {   // FA_AHC_PROFILE builds: the round's cycle counters
#ifdef FA_AHC_PROFILE
    unsigned long long hp[16];
    const Ws &w = p.w;
    (void)hipMemcpy(hp, w.prof, sizeof(hp), hipMemcpyDeviceToHost);
    const double n = hp[15] ? static_cast<double>(hp[15]) : 1.0;
    fprintf(stderr, "ahc profile (cycles/round, block %d of %d, %llu rounds): load+sync %.0f | decide %.0f | merge loads+dab %.0f | row update %.0f | block reduce %.0f | tail %.0f\n",
            w.nblk / 2, w.nblk, hp[15], hp[0] / n, (hp[1] + hp[6] + hp[7] + hp[8]) / n, (hp[2] + hp[9]) / n, (hp[3] + hp[10] + hp[11] + hp[12] + hp[13]) / n, hp[4] / n, hp[5] / n);
    fprintf(stderr, "  merge loads+dab = operands arrive %.0f | centroid, |ca - cb|^2, wave sum %.0f\n", hp[9] / n, hp[2] / n);
    if (hp[10] + hp[11] + hp[12] + hp[13])   // the speculative round's stamps (slots 10 .. 13)
        fprintf(stderr, "  row update (speculative round) = candidates ranked, z* handed over, trip 3 requested %.0f | Lance-Williams row, row state, stores %.0f | "
                        "trip 3 arrived, |.|^2 of the speculated merge %.0f | the speculated merge's row %.0f | rest %.0f\n",
                hp[10] / n, hp[13] / n, hp[11] / n, hp[12] / n, hp[3] / n);
    fprintf(stderr, "  decide = wave reduction %.0f | barrier + result read %.0f | finished rows + global minimum %.0f | state machine + piggy choice %.0f\n", hp[6] / n, hp[7] / n, hp[8] / n, hp[1] / n);
#else
    (void)p;
#endif
}
}  // namespace

fa_status fa::ahc_run_device(fa_ctx *ctx, const double *d_data, size_t N, size_t d, double *d_Z, int mode, fa_ahc_stats *stats, bool z_on_host) {
    // The filter-based rounds keep an N x N matrix resident (N^2 * 8 B); the reference needs O(N d) (fastcluster_internal.hpp:1625-1800).  When the
    // matrix cannot be had — more points than block records (N > 196 608), not enough HBM, or the context's cap — the problem runs in the
    // reference-order mode instead, which has no matrix: slower per merge (every new row is O(N d) exact sums) but the same dendrogram, where
    // round 3 returned ALLOCATION_FAILURE and AHCClustering degraded to singletons (a >= 36 h recording lost its clustering).
    // stats->reference_order == 2 marks that route.
    fa::WsUse ws_use(ctx);                      // released (and trimmed to the context's limit) when the call returns
    auto without_matrix = [&]() {
        if (stats) { *stats = fa_ahc_stats{}; stats->reference_order = 2; }
        const fa_status st = ro_run_device_mf(ctx, d_data, N, d, d_Z, stats, z_on_host);
        if (st == FA_SUCCESS) ctx->last_error.clear();
        return st;
    };
    if (mode == FA_AHC_MODE_REFERENCE_ORDER) {
        if (stats) *stats = fa_ahc_stats{};
        return ro_run_device(ctx, d_data, N, d, d_Z, stats, z_on_host);
    }
    if (prob_check_shape(ctx, N, d) != FA_SUCCESS) return without_matrix();   // too many points for the block records (a too large d fails in ro_run_device as well)
    Prob p;
    p.z_on_host = z_on_host;
    p.cpt = route::single_cpt(sw_int(fa::Sw::AHC_CPT), fa::sw_on(fa::Sw::AHC_NO_SINGLE_BLOCK), N);   // per call, like the other switches (the tests flip them)
    p.N = N; p.d = d; p.Np = route::padded(N, p.cpt); p.d_data = d_data; p.d_Z = d_Z; p.mode = mode;
    p.L = make_layout(N, p.Np, d, route::blocks(N, p.cpt));
    {
        const fa_status ws = fa::ws_acquire(ctx, p.L.total);
        if (ws == FA_ALLOCATION_FAILURE) return without_matrix();
        FA_TRY(ws);
    }
    hipEvent_t ev[3];
    FA_TRY(ctx_events(ctx, ev));                // created once per context
    FA_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
    FA_TRY(prob_setup(ctx, p, static_cast<char *>(ctx->ahc_ws)));
    FA_HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));

    FA_TRY(prob_run_rounds(ctx, p));
    FA_HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p.needs_ro) {   // exact ties at the minimum: the whole problem again, in the reference's selection order
        if (stats) { stats_fill(*stats, p, intervals_of(ev)); stats->merges = 0; }   // the reference-order run reports its own
        // halted before the first merge (duplicates: the very first window ties), one slot per thread, Gram-form start-up: the matrix in the workspace is the one the
        // reference-order run would build first (ahc_rom.hip shares the arrays)
#ifdef FA_POISON_WORKSPACE
        const bool matrix_ready = false;   // the poisoned build fills the workspace again when the reference-order run acquires it: nothing of the attempt survives
#else
        const bool matrix_ready = mode == FA_AHC_MODE_AUTO && p.h.step == 0 && p.cpt == 1 && d % 16 == 0;
#endif
        return ro_run_device(ctx, d_data, N, d, d_Z, stats, z_on_host, /* may_hand_over = */ mode == FA_AHC_MODE_AUTO, matrix_ready);
    }
    print_profile(p);
    if (fa::sw(fa::Sw::AHC_DEBUG))
        fprintf(stderr, "ahc: N %zu rounds %lld merges %d speculated merges committed %lld forced re-scans %lld piggy-backed re-scans %lld windows %lld fallback %lld (kPiggy %d)\n",
                N, p.h.rounds, p.h.step, p.spec_hits, p.h.rescans, p.h.piggy, p.h.windows, p.fallback, kPiggy);
    if (stats) stats_fill(*stats, p, intervals_of(ev));
    return FA_SUCCESS;
}
