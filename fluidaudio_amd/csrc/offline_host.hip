// offline_host.hip — the clustering stage of the offline diarizer as ONE device-resident call.
//
// Replaces the arithmetic of OfflineDiarizerManager.cluster
// (reference: Sources/FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:270-375) on precomputed embeddings:
//   selectTrainingEmbeddings (:591-611) -> AHCClustering.cluster (threshold, :301-306) -> VBxClustering.refineWithConstraints
//   (:308-333) -> computeCentroids (:613-691, fallback computeCentroidsFromClusters :693-740) -> centroid scores + constrained
//   per-chunk assignment, or the plain cosine argmax (:345-375, :789-822).
// The embeddings (fp32, widened to fp64 on the device like `embeddingFeatures.map { $0.map(Double.init) }`, :286) and the PLDA
// features go up ONCE; between the stages only what the host has to decide on crosses PCIe: the dendrogram (32 bytes per merge)
// for the O(N) cut, the label vector back, 8 bytes of ELBO per VBx iteration, pi (S doubles), and the final labels.  The
// stages themselves are the device cores the single-stage entries use (post_launch.h, fa_common.h), so every intermediate result equals the
// one the stage-by-stage Python glue of round 1 produced.
// (Row kernels: offline.hip.)  A recording is a ClusterJob: prepare(), the linkage (alone or batched with other recordings), finish() — a
// short sequence of named steps over one FinishState.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "offline_launch.h"
#include "post_launch.h"

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what the steps of ClusterJob::finish() hand on to each other; the device buffers live until the recording is delivered
struct FinishState {
    std::vector<int32_t> initial;   // AHC labels of the training rows
    int32_t S = 0;                  // distinct AHC labels
    fa::VbxDevice vbx;
    fa::DevBuf b_lab;
    std::vector<double> pi;
    std::vector<int32_t> hard;      // VBx hard labels (fetched only when the speaker count is constrained)
    bool have_vbx = false, adjusted = false, vbx_degraded = false, constrained = false;
    int32_t vbx_iters = 0;
    std::vector<double> km_centroids;   // of the K-Means fallback (adjusted)
    int32_t km_k = 0;
    fa::DevBuf b_cent, b_spk;
    int32_t K = 0;                  // centroids
    fa::DevBuf b_cn, b_scores, b_out;
    double t_ahc = 0, t_vbx = 0;
};

// One recording's pass through the stage, split where the merge chains of several recordings can run together
// (fa_offline_cluster_batch): prepare() = inputs + training rows + normalised rows on the device; the caller runs the linkage
// (alone or batched); finish() = cut, VBx, centroids, assignment.  Everything is enqueued on the context's stream.
struct ClusterJob {
    fa_ctx *ctx;
    const float *embeddings; int64_t n; int32_t d; const double *rho; int32_t rho_dim; const int32_t *chunk_indices; const double *phi;
    const fa_offline_cluster_config *config; int32_t device_pointers;
    int32_t *labels; double *centroids; int32_t max_centroids; int32_t *n_centroids; fa_offline_cluster_info *info;
    // optional copies of the intermediates (fa_offline_cluster_ex): AHC labels and VBx hard labels of the training rows, ELBO per iteration
    int32_t *aux_ahc = nullptr; int32_t *aux_hard = nullptr; double *aux_elbos = nullptr;
    // the recording runs its linkage alone (link()): the dendrogram goes straight to the context's pinned buffer, where cut() reads it — no device copy
    // of it (b_z), no pageable vector.  A batch (link_batch) leaves its dendrograms on the device, one b_z per recording.
    bool z_to_host = false;
    const double *z_host = nullptr;   // set by link(): the dendrogram is there

    fa::DevBuf b_emb32, b_rho_in, b_ok, b_emb, b_temb, b_trho, b_train, b_norm, b_z;
    const float *d_emb32 = nullptr;
    const double *d_rho_all = nullptr, *d_temb = nullptr, *d_trho = nullptr;
    int64_t nt = 0;
    bool rows_finite = false;   // every training row is free of NaN / Inf (the centroid sums may then add a zero-weight row instead of skipping it: same bits)
    double t_begin = 0, t_inputs = 0;
    fa_ahc_stats ahc_stats{};

    // a buffer of the stage from the context's cache, or the stage's allocation-failure status
    fa_status room(fa::DevBuf &b, const size_t bytes, const char *what = "offline cluster: allocation failed") {
        if (b.alloc(ctx, bytes) == hipSuccess) return FA_SUCCESS;
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "%s", what);
    }
    // the context's pinned buffer for the dendrogram, at least `bytes` large (nothing of an earlier call reads it any more: the entries return behind a synchronisation)
    fa_status z_host_room(const size_t bytes) {
        if (ctx->z_host_bytes >= bytes) return FA_SUCCESS;
        if (ctx->z_host) (void)hipHostFree(ctx->z_host);
        ctx->z_host = nullptr; ctx->z_host_bytes = 0;
        if (hipHostMalloc(&ctx->z_host, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->z_host = nullptr; return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "offline cluster: allocation failed"); }
        ctx->z_host_bytes = bytes;
        return FA_SUCCESS;
    }
    // the training rows on the host (the rare paths that take a host-pointer entry or sum on the host)
    fa_status training_rows_to_host(std::vector<double> &temb_host) {
        temb_host.resize(static_cast<size_t>(nt) * d);
        FA_HIP_TRY(ctx, hipMemcpyAsync(temb_host.data(), d_temb, sizeof(double) * nt * d, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    }

    fa_status check_args() {
        if (!ctx || !config || !labels || !n_centroids) return FA_INVALID_ARGUMENT;
        *n_centroids = 0;
        if (info) memset(info, 0, sizeof(*info));
        if (n <= 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "offline cluster: no embeddings (noSpeechDetected, :281-283)");
        if (n > INT32_MAX || d < 1 || rho_dim < 0 || !embeddings || (rho_dim > 0 && (!rho || !phi)) || (config->constrained_assignment && !chunk_indices))
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "offline cluster: bad arguments");
        return FA_SUCCESS;
    }


    // inputs to the device (once), selectTrainingEmbeddings, unit rows for the linkage (b_norm) and room for the dendrogram (b_z; not with z_to_host) when nt >= 2
    fa_status prepare() {
        hipStream_t st = ctx->stream;
        t_begin = now_s();
        d_emb32 = embeddings;
        d_rho_all = rho;
        if (!device_pointers) {
            FA_TRY(room(b_emb32, sizeof(float) * n * d, "offline cluster: input allocation failed"));
            if (rho_dim > 0) FA_TRY(room(b_rho_in, sizeof(double) * n * rho_dim, "offline cluster: input allocation failed"));
            FA_HIP_TRY(ctx, hipMemcpyAsync(b_emb32.p, embeddings, sizeof(float) * n * d, hipMemcpyHostToDevice, st));
            if (rho_dim > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_rho_in.p, rho, sizeof(double) * n * rho_dim, hipMemcpyHostToDevice, st));
            d_emb32 = b_emb32.as<float>();
            d_rho_all = b_rho_in.as<double>();
        }
        // ---- selectTrainingEmbeddings (:591-611): rows without NaN / Inf; all rows if none qualifies
        FA_TRY(room(b_ok, n));
        fa::offline::launch_finite_rows(st, d_emb32, b_ok.as<uint8_t>(), n, d);
        FA_HIP_TRY(ctx, hipGetLastError());
        std::vector<uint8_t> ok(static_cast<size_t>(n));
        FA_HIP_TRY(ctx, hipMemcpyAsync(ok.data(), b_ok.p, n, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        std::vector<int32_t> train;
        for (int64_t i = 0; i < n; ++i) if (ok[i]) train.push_back(static_cast<int32_t>(i));
        rows_finite = !train.empty();   // the training rows are the finite ones — unless none is, and all rows train (:606-609)
        const bool all_rows = train.empty() || static_cast<int64_t>(train.size()) == n;
        if (train.empty()) { train.resize(n); for (int64_t i = 0; i < n; ++i) train[i] = static_cast<int32_t>(i); }
        nt = static_cast<int64_t>(train.size());
        FA_TRY(room(b_emb, sizeof(double) * n * d));
        fa::offline::launch_widen_rows(st, d_emb32, nullptr, b_emb.as<double>(), n, d);   // Float -> Double (:286)
        d_temb = b_emb.as<double>();
        d_trho = d_rho_all;
        if (!all_rows) {
            FA_TRY(room(b_train, sizeof(int32_t) * nt));
            FA_TRY(room(b_temb, sizeof(double) * nt * d));
            if (rho_dim > 0) FA_TRY(room(b_trho, sizeof(double) * nt * rho_dim));
            FA_HIP_TRY(ctx, hipMemcpyAsync(b_train.p, train.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, st));
            fa::offline::launch_gather_rows(st, b_emb.as<double>(), b_train.as<int32_t>(), b_temb.as<double>(), nt, d);
            if (rho_dim > 0) fa::offline::launch_gather_rows(st, d_rho_all, b_train.as<int32_t>(), b_trho.as<double>(), nt, rho_dim);
            d_temb = b_temb.as<double>();
            d_trho = b_trho.as<double>();
        }
        FA_HIP_TRY(ctx, hipGetLastError());
        if (!all_rows) FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // `train` is a host temporary (nothing of it is in flight when every row trains)
        if (nt >= 2) {   // AHC input (:301-306): unit rows
            FA_TRY(room(b_norm, sizeof(double) * nt * d));
            if (!z_to_host) FA_TRY(room(b_z, sizeof(double) * 4 * (nt - 1)));
            else FA_TRY(z_host_room(sizeof(double) * 4 * static_cast<size_t>(nt - 1)));
            FA_TRY(fa::ahc_normalize_dev(ctx, d_temb, b_norm.as<double>(), nt, d));
        }
        t_inputs = now_s();
        return FA_SUCCESS;
    }

    // ---- cut (:301-306); fewer than 2 training rows -> all 0; a failed linkage degrades to singletons (AHCClustering.swift:52-55)
    fa_status cut(FinishState &s, const fa_status ahc_status) {
        s.initial.assign(static_cast<size_t>(nt), 0);
        if (nt >= 2) {
            if (ahc_status != FA_SUCCESS) {
                for (int64_t i = 0; i < nt; ++i) s.initial[i] = static_cast<int32_t>(i);
            } else if (z_host) {   // delivered by the linkage, behind its own synchronisation
                FA_TRY(fa_ahc_cut(z_host, static_cast<size_t>(nt), config->clustering_threshold, s.initial.data()));
            } else {
                std::vector<double> z(static_cast<size_t>(4 * (nt - 1)));
                FA_HIP_TRY(ctx, hipMemcpyAsync(z.data(), b_z.p, sizeof(double) * z.size(), hipMemcpyDeviceToHost, ctx->stream));
                FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                FA_TRY(fa_ahc_cut(z.data(), static_cast<size_t>(nt), config->clustering_threshold, s.initial.data()));
            }
        }
        if (aux_ahc) memcpy(aux_ahc, s.initial.data(), sizeof(int32_t) * static_cast<size_t>(nt));
        return FA_SUCCESS;
    }

    bool has_constraints() const { return config->num_speakers >= 0 || config->min_speakers >= 0 || config->max_speakers >= 0; }   // :309-312

    // ---- VBx (:308-333) on the PLDA features of the training rows: pi, and the hard labels where somebody reads them, come to the host
    fa_status refine(FinishState &s) {
        s.S = nt > 0 ? std::max(1, fa_vbx_speaker_count(s.initial.data(), nt)) : 0;   // max(1, Set(initialClusters).count) (:78)
        if (rho_dim <= 0 || nt <= 0) return FA_SUCCESS;
        hipStream_t st = ctx->stream;
        FA_TRY(room(s.b_lab, sizeof(int32_t) * nt));
        FA_HIP_TRY(ctx, hipMemcpyAsync(s.b_lab.p, s.initial.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, st));
        std::vector<double> elbos(static_cast<size_t>(std::max(config->max_vbx_iterations, 1)));
        FA_TRY(fa::vbx_refine_dev(ctx, d_trho, nt, rho_dim, s.b_lab.as<int32_t>(), s.S, phi, config->warm_start_fa, config->warm_start_fb, config->max_vbx_iterations,
                                  config->convergence_tolerance, elbos.data(), &s.vbx_iters, s.vbx, "offline cluster: VBx degraded to the AHC clusters", &s.vbx_degraded));
        s.pi.resize(s.S);
        FA_HIP_TRY(ctx, hipMemcpyAsync(s.pi.data(), s.vbx.pi.p, sizeof(double) * s.S, hipMemcpyDeviceToHost, st));
        if (has_constraints()) {
            s.hard.resize(nt);
            FA_HIP_TRY(ctx, hipMemcpyAsync(s.hard.data(), s.vbx.hard.p, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
        }
        if (aux_hard) FA_HIP_TRY(ctx, hipMemcpyAsync(aux_hard, s.vbx.hard.p, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        if (aux_elbos) memcpy(aux_elbos, elbos.data(), sizeof(double) * static_cast<size_t>(std::max(s.vbx_iters, 0)));
        s.have_vbx = true;
        return FA_SUCCESS;
    }

    // ---- refineWithConstraints (VBxClustering.swift:685-733): a speaker count outside the resolved bounds is forced by K-Means on the training rows
    fa_status enforce_speaker_count(FinishState &s) {
        if (!s.have_vbx || !has_constraints()) return FA_SUCCESS;
        const int64_t ns = config->num_speakers, mn = config->min_speakers, mx = config->max_speakers;
        int64_t res[3];
        fa_speaker_constraints_resolve(nt, ns >= 0 ? &ns : nullptr, mn >= 0 ? &mn : nullptr, mx >= 0 ? &mx : nullptr, res);
        std::vector<int32_t> used(s.hard);
        std::sort(used.begin(), used.end());
        const int64_t detected = std::unique(used.begin(), used.end()) - used.begin();   // assignedClusterCount (OfflineDiarizerTypes.swift:687-702)
        if (detected >= res[1] && detected <= res[2]) return FA_SUCCESS;
        const int32_t target = static_cast<int32_t>(std::min(std::max(detected, res[1]), res[2]));
        std::vector<double> temb_host;   // the fallback is rare: it takes the host-pointer K-Means entry
        FA_TRY(training_rows_to_host(temb_host));
        std::vector<int32_t> km_labels(static_cast<size_t>(nt));
        s.km_centroids.assign(static_cast<size_t>(std::max<int64_t>(std::min<int64_t>(target, nt), 1)) * d, 0.0);
        FA_TRY(fa_kmeans_cluster_ninit(ctx, temb_host.data(), nt, d, target, 100, 10, 0, km_labels.data(), s.km_centroids.data(), &s.km_k, nullptr, nullptr));
        s.adjusted = true;
        return FA_SUCCESS;
    }

    // ---- centroids (:613-691), three sources.  The K-Means centroids as they are (:622-629) ...
    fa_status centroids_from_kmeans(FinishState &s) {
        s.K = s.km_k;
        FA_TRY(room(s.b_cent, sizeof(double) * s.K * d));
        FA_HIP_TRY(ctx, hipMemcpyAsync(s.b_cent.p, s.km_centroids.data(), sizeof(double) * s.K * d, hipMemcpyHostToDevice, ctx->stream));
        return FA_SUCCESS;
    }
    // ... gamma-weighted means of the speakers with pi > 1e-7 ...
    fa_status centroids_from_posteriors(FinishState &s) {
        std::vector<int32_t> spk;
        for (int sp = 0; sp < s.S; ++sp) if (s.pi[sp] > 1e-7) spk.push_back(sp);
        s.K = static_cast<int32_t>(spk.size());
        if (s.K == 0) return FA_SUCCESS;
        FA_TRY(room(s.b_cent, sizeof(double) * s.K * d));
        FA_TRY(room(s.b_spk, sizeof(int32_t) * s.K));
        FA_HIP_TRY(ctx, hipMemcpyAsync(s.b_spk.p, spk.data(), sizeof(int32_t) * s.K, hipMemcpyHostToDevice, ctx->stream));
        FA_TRY(fa::centroids_dev(ctx, d_temb, nt, d, s.vbx.gamma.as<double>(), s.S, s.b_spk.as<int32_t>(), s.K, s.b_cent.as<double>(), rows_finite));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // spk is a host temporary
        return FA_SUCCESS;
    }
    // ... per-cluster means of the AHC labels (computeCentroidsFromClusters :693-740, sequential sums on the host)
    fa_status centroids_from_clusters(FinishState &s) {
        std::vector<double> temb_host;
        FA_TRY(training_rows_to_host(temb_host));
        int32_t kmax = 0;
        for (int64_t i = 0; i < nt; ++i) kmax = std::max(kmax, s.initial[i] + 1);
        std::vector<double> sum(static_cast<size_t>(kmax) * d, 0.0);
        std::vector<int64_t> cnt(kmax, 0);
        for (int64_t i = 0; i < nt; ++i) {
            ++cnt[s.initial[i]];
            for (int k = 0; k < d; ++k) sum[static_cast<size_t>(s.initial[i]) * d + k] += temb_host[i * d + k];
        }
        std::vector<double> cen;
        for (int c = 0; c < kmax; ++c) if (cnt[c] > 0) for (int k = 0; k < d; ++k) cen.push_back(sum[static_cast<size_t>(c) * d + k] / static_cast<double>(cnt[c]));
        s.K = static_cast<int32_t>(cen.size() / d);
        FA_TRY(room(s.b_cent, sizeof(double) * std::max(s.K, 1) * d));
        FA_HIP_TRY(ctx, hipMemcpyAsync(s.b_cent.p, cen.data(), sizeof(double) * cen.size(), hipMemcpyHostToDevice, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    }
    fa_status compute_centroids(FinishState &s) {
        if (s.adjusted && s.km_k > 0) FA_TRY(centroids_from_kmeans(s));
        else if (s.have_vbx) FA_TRY(centroids_from_posteriors(s));
        if (s.K == 0 && nt > 0) FA_TRY(centroids_from_clusters(s));
        return FA_SUCCESS;
    }

    // ---- assignment of ALL embeddings (:345-375): constrained per chunk unless the count was forced or there is a single centroid
    fa_status assign(FinishState &s) {
        FA_TRY(room(s.b_cn, sizeof(double) * std::max(s.K, 1) * d));
        FA_TRY(room(s.b_out, sizeof(int32_t) * n));
        s.constrained = config->constrained_assignment && !s.adjusted && s.K > 1;   // :355-358
        if (!s.constrained) return fa::assign_dev(ctx, b_emb.as<double>(), n, d, s.b_cent.as<double>(), s.K, s.b_cn.as<double>(), s.b_out.as<int32_t>());
        FA_TRY(room(s.b_scores, sizeof(double) * n * s.K));
        FA_TRY(fa::scores_dev(ctx, b_emb.as<double>(), n, d, s.b_cent.as<double>(), s.K, s.b_cn.as<double>(), s.b_scores.as<double>()));
        return fa::constrained_assign_dev(ctx, s.b_scores.as<double>(), n, s.K, chunk_indices, s.b_out.as<int32_t>());
    }

    // ---- labels, centroids and `info` to the caller
    fa_status deliver(FinishState &s, const fa_status ahc_status) {
        hipStream_t st = ctx->stream;
        *n_centroids = s.K;
        if (centroids && s.K > max_centroids) {   // checked BEFORE any output copy is enqueued: on this error the caller's buffers are untouched
            FA_HIP_TRY(ctx, hipStreamSynchronize(st));
            return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "offline cluster: %d centroids, room for %d", s.K, max_centroids);
        }
        FA_HIP_TRY(ctx, hipMemcpyAsync(labels, s.b_out.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (centroids && s.K > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(centroids, s.b_cent.p, sizeof(double) * s.K * d, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        const double t_end = now_s();
        if (info) {
            info->training_rows = nt; info->initial_clusters = s.S; info->vbx_iterations = s.vbx_iters; info->was_adjusted = s.adjusted ? 1 : 0;
            info->constrained = s.constrained ? 1 : 0; info->vbx_degraded = s.vbx_degraded ? 1 : 0; info->ahc_degraded = (nt >= 2 && ahc_status != FA_SUCCESS) ? 1 : 0;
            info->inputs_s = t_inputs - t_begin; info->ahc_s = s.t_ahc - t_inputs; info->vbx_s = s.t_vbx - s.t_ahc; info->assign_s = t_end - s.t_vbx;
            info->total_s = t_end - t_begin; info->ahc = ahc_stats;
        }
        return FA_SUCCESS;
    }

    // ahc_status: what the linkage of b_norm into b_z returned (ignored when nt < 2)
    fa_status finish(const fa_status ahc_status) {
        FinishState s;
        FA_TRY(cut(s, ahc_status));
        s.t_ahc = now_s();
        FA_TRY(refine(s));
        FA_TRY(enforce_speaker_count(s));
        s.t_vbx = now_s();
        FA_TRY(compute_centroids(s));
        FA_TRY(assign(s));
        return deliver(s, ahc_status);
    }

    // the linkage of one recording on its own (fa_offline_cluster_batch advances the merge chains of all recordings together instead)
    fa_status link() {
        if (nt < 2) return FA_SUCCESS;
        if (fa::fault_hit(FA_FAULT_AHC)) return FA_RUNTIME_ERROR;
        if (!z_to_host) return fa::ahc_run_device(ctx, b_norm.as<double>(), static_cast<size_t>(nt), static_cast<size_t>(d), b_z.as<double>(), config->ahc_mode, &ahc_stats);
        const fa_status st = fa::ahc_run_device(ctx, b_norm.as<double>(), static_cast<size_t>(nt), static_cast<size_t>(d), static_cast<double *>(ctx->z_host), config->ahc_mode, &ahc_stats,
                                                /* z_on_host = */ true);
        if (st == FA_SUCCESS) z_host = static_cast<const double *>(ctx->z_host);
        return st;
    }
};

// Everything except the linkage is, per recording, a chain of small kernels, copies and host decisions: several recordings run it side
// by side, each worker thread on its own stream of the same device.  Worker contexts live with the caller's context (round 4): their
// streams and buffer caches are reused by the next call.
struct Workers {
    fa_ctx *ctx;
    int32_t count;
    int workers;
    std::vector<fa_ctx *> wctx;
    std::vector<std::string> werr;   // per worker: the text of its first failing recording

    Workers(fa_ctx *c, const int32_t recordings) : ctx(c), count(recordings), workers(std::max(1, std::min<int>(recordings, 8))), wctx(static_cast<size_t>(workers), nullptr), werr(static_cast<size_t>(workers)) {
        wctx[0] = ctx;
        for (int t = 1; t < workers; ++t) {
            fa_ctx *&wk = ctx->workers[t - 1];
            if (!wk && fa_ctx_create(ctx->device, nullptr, &wk) != FA_SUCCESS) wk = nullptr;
            if (wk) { wk->ws_limit = ctx->ws_limit; wk->ws_cap = ctx->ws_cap; wk->last_error.clear(); }
            wctx[t] = wk;
        }
    }

    // worker t's share (the recordings r = stride_from, stride_from + workers, ...) of phase(job index) -> fa_status, for every recording that is still healthy
    template <class Phase>
    void share(std::vector<ClusterJob> &jobs, std::vector<fa_status> &st, Phase &phase, const int t, const int stride_from) {
        fa_ctx *c = wctx[t];
        fa::DeviceGuard g(c->device);
        for (int32_t r = stride_from; r < count; r += workers) {
            if (st[r] != FA_SUCCESS) continue;
            jobs[r].ctx = c;
            try { st[r] = phase(r); }
            catch (const std::bad_alloc &) { st[r] = FA_ALLOCATION_FAILURE; }
            catch (...) { st[r] = FA_UNKNOWN_ERROR; }
            if (st[r] != FA_SUCCESS && werr[t].empty()) werr[t] = c->last_error;
            jobs[r].ctx = ctx;
        }
        (void)hipStreamSynchronize(c->stream);
    }

    template <class Phase>
    void run(std::vector<ClusterJob> &jobs, std::vector<fa_status> &st, Phase &&phase) {
        std::vector<std::thread> th;
        std::vector<char> started(static_cast<size_t>(workers), 0);
        th.reserve(static_cast<size_t>(workers));
        for (int t = 1; t < workers; ++t)
            if (wctx[t]) started[static_cast<size_t>(t)] = fa::start_thread(th, [this, &jobs, &st, &phase, t]() { share(jobs, st, phase, t, t); }) ? 1 : 0;
        share(jobs, st, phase, 0, 0);
        for (auto &x : th) x.join();
        for (int t = 1; t < workers; ++t) {
            if (!wctx[t]) share(jobs, st, phase, 0, t);                               // a worker without a stream of its own: the caller's context takes its share
            else if (!started[static_cast<size_t>(t)]) share(jobs, st, phase, t, t);   // no host thread to be had: the calling thread runs that worker's share on the worker's stream
        }
    }
};

// the merge chains of all healthy recordings advance together (one launch = one round of every unfinished recording); per_job: each recording's linkage status
fa_status link_batch(fa_ctx *ctx, std::vector<ClusterJob> &jobs, const std::vector<fa_status> &st, const int32_t d, const int ahc_mode, std::vector<fa_status> &per_job) {
    std::vector<int32_t> who;
    std::vector<const double *> din;
    std::vector<double *> dz;
    std::vector<size_t> rows;
    for (size_t r = 0; r < jobs.size(); ++r)
        if (st[r] == FA_SUCCESS && jobs[r].nt >= 2) { who.push_back(static_cast<int32_t>(r)); din.push_back(jobs[r].b_norm.as<double>()); dz.push_back(jobs[r].b_z.as<double>()); rows.push_back(static_cast<size_t>(jobs[r].nt)); }
    std::vector<fa_status> ahc_st(who.size(), FA_SUCCESS);
    std::vector<fa_ahc_stats> ahc_stats(who.size());
    if (!who.empty())
        (void)fa::ahc_run_device_batch(ctx, static_cast<int>(who.size()), din.data(), rows.data(), static_cast<size_t>(d), dz.data(), ahc_mode, ahc_stats.data(), ahc_st.data());
    per_job.assign(jobs.size(), FA_SUCCESS);
    for (size_t j = 0; j < who.size(); ++j) { per_job[who[j]] = ahc_st[j]; jobs[who[j]].ahc_stats = ahc_stats[j]; }
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

fa_status cluster_batch(fa_ctx *ctx, int32_t count, const float *const *embeddings, const int64_t *n, int32_t d, const double *const *rho,
                        int32_t rho_dim, const int32_t *const *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                        const int32_t device_pointers, int32_t *const *labels, double *const *centroids, int32_t max_centroids, int32_t *n_centroids,
                        fa_offline_cluster_info *infos, int32_t *statuses) {
    if (!ctx || count < 0 || (count > 0 && (!embeddings || !n || !labels || !n_centroids || !config))) return FA_INVALID_ARGUMENT;
    if (count == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "offline cluster", [&]() -> fa_status {
        // device-resident inputs were produced on the caller's stream; the recordings are prepared on the workers' streams
        if (device_pointers) FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<ClusterJob> jobs;
        jobs.reserve(static_cast<size_t>(count));   // the jobs own device buffers: they must never be copied after prepare()
        std::vector<fa_status> st(static_cast<size_t>(count), FA_SUCCESS);
        for (int32_t r = 0; r < count; ++r) {
            jobs.push_back(ClusterJob{ctx, embeddings[r], n[r], d, rho ? rho[r] : nullptr, rho_dim, chunk_indices ? chunk_indices[r] : nullptr, phi, config, device_pointers,
                                      labels[r], centroids ? centroids[r] : nullptr, max_centroids, &n_centroids[r], infos ? &infos[r] : nullptr});
            st[r] = jobs.back().check_args();
        }
        Workers pool(ctx, count);
        pool.run(jobs, st, [&](const int32_t r) { return jobs[r].prepare(); });
        std::vector<fa_status> per_job_ahc;
        FA_TRY(link_batch(ctx, jobs, st, d, config->ahc_mode, per_job_ahc));
        pool.run(jobs, st, [&](const int32_t r) { return jobs[r].finish(per_job_ahc[r]); });
        for (int t = 1; t < pool.workers; ++t) if (!pool.werr[t].empty() && ctx->last_error.empty()) ctx->last_error = pool.werr[t];
        fa_status first = FA_SUCCESS;
        for (int32_t r = 0; r < count; ++r) {
            if (statuses) statuses[r] = st[r];
            if (first == FA_SUCCESS && st[r] != FA_SUCCESS) first = st[r];
        }
        return first;
    });
}

}  // namespace

extern "C" {

void fa_offline_cluster_default_config(fa_offline_cluster_config *c) {
    if (!c) return;
    c->clustering_threshold = 0.6; c->warm_start_fa = 0.07; c->warm_start_fb = 0.8;     // OfflineDiarizerTypes.swift:155-163,189-192
    c->max_vbx_iterations = 20; c->convergence_tolerance = 1e-4; c->constrained_assignment = 1;
    c->num_speakers = -1; c->min_speakers = -1; c->max_speakers = -1; c->ahc_mode = FA_AHC_MODE_AUTO;
}

// fa_offline_cluster + copies of the stage's intermediates for verification at full size (bench.py and the 8 h digest test compare
// them with the CPU side): ahc_labels [training rows] = AHCClustering.cluster's output, vbx_hard [training rows] = argmax of gamma,
// elbos [max_vbx_iterations] (info->vbx_iterations of them are written).  Every pointer may be NULL.
fa_status fa_offline_cluster_ex(fa_ctx *ctx, const float *embeddings, int64_t n, int32_t d, const double *rho, int32_t rho_dim,
                                const int32_t *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                                int32_t device_pointers, int32_t *labels, double *centroids, int32_t max_centroids, int32_t *n_centroids,
                                fa_offline_cluster_info *info, int32_t *ahc_labels, int32_t *vbx_hard, double *elbos) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    ClusterJob job{ctx, embeddings, n, d, rho, rho_dim, chunk_indices, phi, config, device_pointers, labels, centroids, max_centroids, n_centroids, info,
                   ahc_labels, vbx_hard, elbos};
    job.z_to_host = true;
    FA_TRY(job.check_args());
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "offline cluster", [&]() -> fa_status {
        FA_TRY(job.prepare());
        return job.finish(job.link());
    });
}

fa_status fa_offline_cluster(fa_ctx *ctx, const float *embeddings, int64_t n, int32_t d, const double *rho, int32_t rho_dim,
                             const int32_t *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                             int32_t device_pointers, int32_t *labels, double *centroids, int32_t max_centroids, int32_t *n_centroids,
                             fa_offline_cluster_info *info) {
    return fa_offline_cluster_ex(ctx, embeddings, n, d, rho, rho_dim, chunk_indices, phi, config, device_pointers, labels, centroids, max_centroids, n_centroids, info,
                                 nullptr, nullptr, nullptr);
}

fa_status fa_offline_cluster_batch(fa_ctx *ctx, int32_t count, const float *const *embeddings, const int64_t *n, int32_t d, const double *const *rho,
                                   int32_t rho_dim, const int32_t *const *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                                   int32_t *const *labels, double *const *centroids, int32_t max_centroids, int32_t *n_centroids,
                                   fa_offline_cluster_info *infos, int32_t *statuses) {
    return cluster_batch(ctx, count, embeddings, n, d, rho, rho_dim, chunk_indices, phi, config, 0, labels, centroids, max_centroids, n_centroids, infos, statuses);
}

fa_status fa_offline_cluster_batch_dev(fa_ctx *ctx, int32_t count, const float *const *d_embeddings, const int64_t *n, int32_t d, const double *const *d_rho,
                                       int32_t rho_dim, const int32_t *const *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                                       int32_t *const *labels, double *const *centroids, int32_t max_centroids, int32_t *n_centroids,
                                       fa_offline_cluster_info *infos, int32_t *statuses) {
    return cluster_batch(ctx, count, d_embeddings, n, d, d_rho, rho_dim, chunk_indices, phi, config, 1, labels, centroids, max_centroids, n_centroids, infos, statuses);
}

}  // extern "C"
