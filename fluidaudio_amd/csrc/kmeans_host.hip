// kmeans_host.hip — the host side of the speaker-count fallback (kernels: kmeans.hip, operands: kmeans_launch.h, draws and guards:
// kmeans_draws.h): the n_init runs walked in lock step — one stream synchronisation per kSyncEvery Lloyd iterations for the whole batch —
// the choice of the best run, and the C ABI.  Built with -ffp-contract=off like kmeans.hip: the inertia is the reference's fp64 sum.
#include <cfloat>

#include "kmeans_launch.h"

namespace {

using namespace fa::kmeans;

struct RunResult {
    int32_t iterations = 0;
    double inertia = 0.0;
};

// Lloyd iterations for a.runs seeds at once; the caller fills the operands up to `list`, the bookkeeping is set up here.  On success
// a.assign[runs][n], a.cen[runs][k][d] hold every run's result.
fa_status lloyd_batch(fa_ctx *ctx, LloydArgs a, int max_iter, const uint64_t *seeds, std::vector<RunResult> &res) {
    hipStream_t st = ctx->stream;
    const int64_t n = a.n;
    const int d = a.d, k = a.k, runs = a.runs;
    std::vector<Rng> rng(runs);
    std::vector<int64_t> idx(n);
    for (int r = 0; r < runs; ++r) {                                     // initializeCentroids (:144-152)
        rng[r].s = seeds[r];
        shuffled_indices(rng[r], idx);
        for (int c = 0; c < k; ++c)
            FA_HIP_TRY(ctx, hipMemcpyAsync(a.cen + (static_cast<int64_t>(r) * k + c) * d, a.xn + idx[c] * d, sizeof(double) * d, hipMemcpyDeviceToDevice, st));
    }
    FA_HIP_TRY(ctx, hipMemsetAsync(a.assign, 0, sizeof(int32_t) * runs * n, st));
    // pre-drawn re-seeding picks + device-side bookkeeping: done[runs] | iters[runs] | cursor[runs] | status[2] | picks[runs][kPicks]
    std::vector<int32_t> h_picks(static_cast<size_t>(runs) * kPicks);
    for (int r = 0; r < runs; ++r) draw_picks(rng[r], n, h_picks.data() + static_cast<size_t>(r) * kPicks);
    fa::DevBuf d_book;
    const size_t book_ints = static_cast<size_t>(3) * runs + 2;
    FA_TRY(fa::take_once(ctx, "kmeans", {{&d_book, sizeof(int32_t) * (book_ints + h_picks.size())}}));
    a.done = d_book.as<int32_t>();
    a.iters = a.done + runs;
    a.cursor = a.iters + runs;
    a.status = a.cursor + runs;
    int32_t *d_picks = a.status + 2;
    a.picks = d_picks;
    FA_HIP_TRY(ctx, hipMemsetAsync(a.done, 0, sizeof(int32_t) * book_ints, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(d_picks, h_picks.data(), sizeof(int32_t) * h_picks.size(), hipMemcpyHostToDevice, st));
    res.assign(runs, RunResult());
    std::vector<int32_t> h_book(book_ints);
    constexpr int kSyncEvery = 8;   // iterations between host checks (launches behind the convergence of every run are no-ops)
    for (int it = 0; it < max_iter; ++it) {
        FA_HIP_TRY(ctx, hipMemsetAsync(a.changed, 0, sizeof(int32_t) * runs, st));
        launch_assign(st, a);
        launch_members(st, a);
        launch_update(st, a);
        launch_step_end(st, a, it);
        FA_HIP_TRY(ctx, hipGetLastError());
        if ((it + 1) % kSyncEvery == 0 || it + 1 == max_iter) {
            FA_HIP_TRY(ctx, hipMemcpyAsync(h_book.data(), a.done, sizeof(int32_t) * book_ints, hipMemcpyDeviceToHost, st));
            FA_HIP_TRY(ctx, hipStreamSynchronize(st));
            if (h_book[3 * runs + 1]) return fa::set_error(ctx, FA_RUNTIME_ERROR, "kmeans: more than %d empty-cluster re-seeds in one run", kPicks);
            bool all = true;
            for (int r = 0; r < runs; ++r) all = all && h_book[r] != 0;
            if (all) break;
        }
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(h_book.data(), a.done, sizeof(int32_t) * book_ints, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // also keeps h_picks alive until its upload has completed
    for (int r = 0; r < runs; ++r) res[r].iterations = h_book[runs + r];
    return FA_SUCCESS;
}

struct Buffers {
    fa::DevBuf x, xn, xt, cen, assign, changed, counts, list, dist;
};

fa_status kmeans_device(fa_ctx *ctx, const double *emb, int64_t n, int d, int k, int max_iter, const uint64_t *seeds, int runs,
                        bool want_inertia, int32_t *labels, double *centroids, int32_t *best_run, double *inertias, int32_t *iterations) {
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    int best = 0;
    double best_inertia = DBL_MAX;
    std::vector<int32_t> best_labels;
    std::vector<double> best_cen;
    for (int r0 = 0; r0 < runs; r0 += kMaxRuns) {
        const int nr = std::min(kMaxRuns, runs - r0);
        Buffers b;
        FA_TRY(fa::take_once(ctx, "kmeans", {{&b.x, sizeof(double) * n * d, true, emb}, {&b.xn, sizeof(double) * n * d}, {&b.xt, sizeof(double) * n * d},
                                             {&b.cen, sizeof(double) * nr * k * d}, {&b.assign, sizeof(int32_t) * nr * n}, {&b.changed, sizeof(int32_t) * nr},
                                             {&b.counts, sizeof(int32_t) * nr * k}, {&b.list, sizeof(int32_t) * nr * n}}));
        launch_normalize(st, b.x.as<double>(), b.xn.as<double>(), b.xt.as<double>(), n, d);
        LloydArgs a{};
        a.xn = b.xn.as<double>(); a.xt = b.xt.as<double>(); a.cen = b.cen.as<double>();
        a.assign = b.assign.as<int32_t>(); a.changed = b.changed.as<int32_t>(); a.counts = b.counts.as<int32_t>(); a.list = b.list.as<int32_t>();
        a.n = n; a.d = d; a.k = k; a.runs = nr;
        std::vector<RunResult> res;
        FA_TRY(lloyd_batch(ctx, a, max_iter, seeds + r0, res));
        std::vector<double> h_dist;
        if (want_inertia) {
            FA_TRY(fa::take_once(ctx, "kmeans", {{&b.dist, sizeof(double) * nr * n}}));
            launch_own_distance(st, a, b.dist.as<double>());
            FA_HIP_TRY(ctx, hipGetLastError());
            h_dist.resize(static_cast<size_t>(nr) * n);
            FA_HIP_TRY(ctx, hipMemcpyAsync(h_dist.data(), b.dist.p, sizeof(double) * nr * n, hipMemcpyDeviceToHost, st));
            FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        for (int r = 0; r < nr; ++r) {
            double inertia = 0.0;
            if (want_inertia) for (int64_t i = 0; i < n; ++i) inertia += h_dist[static_cast<size_t>(r) * n + i];
            if (inertias) inertias[r0 + r] = inertia;
            if (iterations && runs == 1) *iterations = res[r].iterations;
            const bool better = !want_inertia || inertia < best_inertia;  // strict '<': the first best run wins (:122-125)
            if (better || r0 + r == 0) {                                  // run 0 doubles as the fallback of :126-128
                if (better) { best_inertia = inertia; best = r0 + r; }
                best_labels.resize(n);
                best_cen.resize(static_cast<size_t>(k) * d);
                FA_HIP_TRY(ctx, hipMemcpyAsync(best_labels.data(), b.assign.as<int32_t>() + static_cast<int64_t>(r) * n, sizeof(int32_t) * n,
                                               hipMemcpyDeviceToHost, st));
                FA_HIP_TRY(ctx, hipMemcpyAsync(best_cen.data(), b.cen.as<double>() + static_cast<int64_t>(r) * k * d, sizeof(double) * k * d,
                                               hipMemcpyDeviceToHost, st));
                FA_HIP_TRY(ctx, hipStreamSynchronize(st));
            }
        }
    }
    std::copy(best_labels.begin(), best_labels.end(), labels);
    if (centroids) std::copy(best_cen.begin(), best_cen.end(), centroids);
    if (best_run) *best_run = best;
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

uint64_t fa_seeded_rng_next(uint64_t *state) {
    if (!state) return 0;
    Rng r{*state};
    const uint64_t v = r.next();
    *state = r.s;
    return v;
}

uint64_t fa_seeded_rng_below(uint64_t *state, uint64_t upper_bound) {
    if (upper_bound == 0 || !state) return 0;
    Rng r{*state};
    const uint64_t v = r.below(upper_bound);
    *state = r.s;
    return v;
}

fa_status fa_kmeans_cluster(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, int32_t num_clusters, int32_t max_iterations, uint64_t seed,
                            int32_t *labels, double *centroids, int32_t *out_k, int32_t *out_iterations) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (out_iterations) *out_iterations = 0;
    if (n < 0 || (n > 0 && (!labels || (d > 0 && !emb)))) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kmeans: bad arguments");
    if (n > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "kmeans: n exceeds int32");
    return fa::no_throw(ctx, "kmeans", [&]() -> fa_status {
        if (degenerate(emb, n, d, num_clusters, labels, centroids, out_k)) return FA_SUCCESS;
        const int k = static_cast<int>(std::min<int64_t>(num_clusters, n));
        FA_TRY(kmeans_device(ctx, emb, n, d, k, max_iterations, &seed, 1, false, labels, centroids, nullptr, nullptr, out_iterations));
        if (out_k) *out_k = k;
        return FA_SUCCESS;
    });
}

fa_status fa_kmeans_cluster_ninit(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, int32_t num_clusters, int32_t max_iterations, int32_t n_init,
                                  uint64_t base_seed, int32_t *labels, double *centroids, int32_t *out_k, int32_t *best_run, double *inertias) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (best_run) *best_run = 0;
    if (!(n > num_clusters && n_init > 1))                                // guard (:106-110)
        return fa_kmeans_cluster(ctx, emb, n, d, num_clusters, max_iterations, base_seed, labels, centroids, out_k, nullptr);
    if (n < 0 || !labels || (d > 0 && !emb)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kmeans: bad arguments");
    if (n > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "kmeans: n exceeds int32");
    return fa::no_throw(ctx, "kmeans", [&]() -> fa_status {
        if (degenerate(emb, n, d, num_clusters, labels, centroids, out_k)) {  // d == 0 or k <= 0: every run returns the same labels
            if (inertias) std::fill(inertias, inertias + n_init, 0.0);
            return FA_SUCCESS;
        }
        const int k = static_cast<int>(std::min<int64_t>(num_clusters, n));
        std::vector<uint64_t> seeds(n_init);
        for (int i = 0; i < n_init; ++i) seeds[i] = base_seed + static_cast<uint64_t>(i);
        FA_TRY(kmeans_device(ctx, emb, n, d, k, max_iterations, seeds.data(), n_init, true, labels, centroids, best_run, inertias, nullptr));
        if (out_k) *out_k = k;
        return FA_SUCCESS;
    });
}

void fa_speaker_constraints_resolve(int64_t num_embeddings, const int64_t *num_speakers, const int64_t *min_speakers, const int64_t *max_speakers,
                                    int64_t out[3]) {
    if (out) resolve_constraints(num_embeddings, num_speakers, min_speakers, max_speakers, out);
}

}  // extern "C"
