// reconstruct_host.hip — the host side of the reconstruction (kernels and launchers: reconstruct.hip, through reconstruct_launch.h): the
// argument checks and the frame plan (reconstruct_geom.h), its staging, the read-back of the per-frame decision (fa_reconstruct_info:
// frame records, speaker counts, ZeroVoteReembedder.detectRuns), the raw segments of the device's runs (appendSegment,
// OfflineReconstruction.swift:400-429), mergeSegments / sanitize / excludeOverlaps (:359-398, :431-496), buildChunkAssignments and the
// C ABI.  Built with -ffp-contract=off: the segment times g * fd and (T - 1) * fd + fd are fp64 without FMA.
//
// Where the reference is not deterministic: raw segments that close at the same frame, and those flushed after the last frame,
// are appended in Swift Dictionary order (hash-seeded), and that order decides merges between speakers whose segments start at the
// same time.  Here the raw order is (closing frame, cluster index ascending); a segment still open after the last frame closes at
// frame totalFrames.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "reconstruct_launch.h"

namespace {

using namespace fa::reconstruct;

// ---------------------------------------------------------------- host passes

bool same_speaker(const fa_rttm_segment &a, const fa_rttm_segment &b) { return strncmp(a.speaker_id, b.speaker_id, sizeof(a.speaker_id)) == 0; }

// blendedQuality (:465-479)
float blended_quality(const fa_rttm_segment &l, const fa_rttm_segment &r) {
    const double ld = static_cast<double>(l.end_seconds - l.start_seconds), rd = static_cast<double>(r.end_seconds - r.start_seconds);
    const double total = ld + rd;
    if (!(total > 0)) return std::min(std::max((l.quality + r.quality) / 2, 0.0f), 1.0f);
    const double weighted = static_cast<double>(l.quality) * ld + static_cast<double>(r.quality) * rd;
    return static_cast<float>(std::min(std::max(weighted / total, 0.0), 1.0));
}

void stable_by_start(std::vector<fa_rttm_segment> &v) {
    std::stable_sort(v.begin(), v.end(), [](const fa_rttm_segment &x, const fa_rttm_segment &y) { return x.start_seconds < y.start_seconds; });
}

// mergeSegments (:431-463) -> sanitize (:481-496) -> excludeOverlaps (:359-398)
std::vector<fa_rttm_segment> finalize(const fa_reconstruct_config &cfg, std::vector<fa_rttm_segment> raw) {
    std::vector<fa_rttm_segment> merged;
    if (!raw.empty()) {
        const double gap_threshold = std::max(cfg.min_gap_duration, cfg.min_duration_off);
        stable_by_start(raw);
        fa_rttm_segment cur = raw[0];
        for (size_t i = 1; i < raw.size(); ++i) {
            const fa_rttm_segment &s = raw[i];
            if (same_speaker(s, cur) && static_cast<double>(s.start_seconds) - static_cast<double>(cur.end_seconds) <= gap_threshold) {
                const float q = blended_quality(cur, s);
                cur.end_seconds = std::max(cur.end_seconds, s.end_seconds);
                cur.quality = q;
                continue;
            }
            merged.push_back(cur);
            cur = s;
        }
        merged.push_back(cur);
    }
    stable_by_start(merged);
    const float min_dur = std::max(static_cast<float>(cfg.min_segment_duration), static_cast<float>(cfg.min_duration_on));
    std::vector<fa_rttm_segment> kept;
    for (const auto &s : merged) if (s.end_seconds - s.start_seconds >= min_dur) kept.push_back(s);
    if (!cfg.exclusive) return kept;
    std::vector<fa_rttm_segment> out;
    const float min_seg = static_cast<float>(cfg.min_segment_duration);
    for (const auto &s : kept) {
        float start = s.start_seconds;
        const float end = s.end_seconds;
        if (!out.empty() && start < out.back().end_seconds) start = out.back().end_seconds;
        if (start >= end) continue;
        const float dur = end - start;
        if (dur < min_seg) continue;
        const float orig = s.end_seconds - s.start_seconds;
        const float scale = orig > 0 ? dur / orig : 1.0f;
        fa_rttm_segment t = s;
        t.start_seconds = start;
        t.quality = std::max(0.0f, std::min(1.0f, s.quality * scale));
        out.push_back(t);
    }
    return out;
}

fa_status write_segments(fa_ctx *ctx, const std::vector<fa_rttm_segment> &segs, fa_rttm_segment *out, int64_t capacity, int64_t *count) {
    *count = static_cast<int64_t>(segs.size());
    if (!out) return FA_SUCCESS;
    if (capacity < *count) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "reconstruct: output holds %lld of %lld segments", (long long)capacity, (long long)*count);
    std::copy(segs.begin(), segs.end(), out);
    return FA_SUCCESS;
}

void set_info(fa_reconstruct_info *info, int64_t T, int64_t raw, double fd) {
    if (!info) return;
    info->total_frames = T;
    info->raw_segments = raw;
    info->frame_duration = fd;
    info->zero_vote_run_count = 0;
    info->frame_slots = 0;
}

struct Call {   // the arguments of fa_offline_reconstruct / fa_offline_reconstruct_dev
    const fa_reconstruct_config *cfg;
    const float *weights;
    int64_t C;
    int32_t F, S;
    const double *offsets;
    int64_t n_offsets;
    const int32_t *hard;
    int32_t K;
    const int64_t *overrides;
    int64_t n_overrides;
    fa_rttm_segment *out;
    int64_t capacity, *count;
    fa_reconstruct_info *info;
    bool device_weights;
};

// Arguments -> frame duration + FramePlan, with every argument and limit check of the entry.  FA_SUCCESS with p.T == 0: an input the
// reference answers with no segments (:30, :33).
fa_status make_plan(fa_ctx *ctx, const Call &c, double &fd, FramePlan &p) {
    if (c.C < 0 || c.F < 0 || c.S < 0 || c.K < 0 || c.n_offsets < 0 || c.n_overrides < 0 || c.capacity < 0 || (c.C > 0 && c.F > 0 && c.S > 0 && !c.weights) ||
        (c.n_offsets > 0 && !c.offsets) || (c.n_overrides > 0 && !c.overrides) || c.S > kSelMask)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: bad arguments");
    if (c.C == 0 || c.F == 0) return FA_SUCCESS;
    fd = frame_duration(c.cfg->frame_duration, c.cfg->window_duration, c.F);
    if (!std::isfinite(fd)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: frame duration is not finite");
    if (!(fd > 0)) return FA_SUCCESS;
    if (c.C > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "reconstruct: more than 2^31 chunks");
    p = frame_plan(c.C, c.F, c.S, c.K, fd, c.cfg->window_duration, c.offsets, c.n_offsets, c.hard, c.overrides, c.n_overrides);
    if (p.error == PlanError::kChunkStart)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: chunk %lld starts at a non-finite time", (long long)p.index);
    if (p.error == PlanError::kFrames) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "reconstruct: %.0f global frames", p.frames);
    set_info(c.info, p.T, 0, fd);
    if (c.info) c.info->frame_slots = p.smax;
    if (p.error == PlanError::kOverride)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: override %lld is out of range", (long long)p.index);
    return FA_SUCCESS;
}

// which of fa_reconstruct_info's optional outputs the caller gave room for
struct Wanted {
    bool frames, counts, runs;
    bool words() const { return frames || counts || runs; }
};
Wanted wanted(const fa_reconstruct_info *info, int32_t T) {
    return Wanted{info && info->frame_capacity >= T && (info->frame_clusters || info->frame_averages || info->expected_count_sums),
                  info && info->speaker_counts && info->speaker_counts_capacity >= T, info && info->zero_vote_runs};
}

struct Buffers {
    fa::DevBuf w, start, first, last, hard, ovr, word, sel, avg, bsum, flags, starts, esum, raw;
    FrameArgs args;   // the frame kernel's operands over them
};

// the buffers of the frame stage, the plan's H2D copies, flags ([0] bad, [1] raw runs) zeroed
fa_status stage(fa_ctx *ctx, const Call &c, const FramePlan &p, double fd, bool want_esum, Buffers &b) {
    hipStream_t st = ctx->stream;
    const int64_t C = c.C, T = p.T, items = T * p.smax;
    const size_t wbytes = sizeof(float) * C * c.F * c.S;
    FA_TRY(fa::take(ctx, "reconstruct", {{&b.w, wbytes, !c.device_weights, c.weights}, {&b.start, sizeof(double) * C, true, p.start.data()},
                                         {&b.first, sizeof(int32_t) * C, true, p.first_g.data()}, {&b.last, sizeof(int32_t) * C, true, p.last_g.data()},
                                         {&b.hard, sizeof(int32_t) * C * c.S, true, p.hard.data()}, {&b.ovr, sizeof(int32_t) * T, !p.ovr.empty(), p.ovr.data()},
                                         {&b.word, sizeof(int32_t) * T}, {&b.sel, sizeof(int32_t) * items}, {&b.avg, sizeof(double) * items},
                                         {&b.bsum, sizeof(int32_t) * run_blocks(items)}, {&b.flags, sizeof(int32_t) * 2}, {&b.starts, sizeof(int64_t) * items},
                                         {&b.esum, sizeof(double) * T, want_esum}}));
    const float *d_w = c.device_weights ? c.weights : b.w.as<float>();
    FA_HIP_TRY(ctx, hipMemsetAsync(b.flags.p, 0, sizeof(int32_t) * 2, st));
    b.args = FrameArgs{d_w, b.start.as<double>(), b.first.as<int32_t>(), b.last.as<int32_t>(), b.hard.as<int32_t>(), p.ovr.empty() ? nullptr : b.ovr.as<int32_t>(),
                       b.word.as<int32_t>(), b.sel.as<int32_t>(), b.avg.as<double>(), b.flags.as<int32_t>(), b.esum.p ? b.esum.as<double>() : nullptr,
                       C, c.F, c.S, p.Kc, p.T, p.smax, p.maxc, p.sorted ? 1 : 0, fd};
    return FA_SUCCESS;
}

// the per-frame decision and the run starts; the run count sizes the next stage (one synchronisation)
fa_status decide_frames(fa_ctx *ctx, const Buffers &b, int64_t &n_raw) {
    hipStream_t st = ctx->stream;
    launch_frames(st, b.args, b.bsum.as<int32_t>(), b.flags.as<int32_t>() + 1, b.starts.as<int64_t>());
    FA_HIP_TRY(ctx, hipGetLastError());
    int32_t flags[2];
    FA_HIP_TRY(ctx, hipMemcpyAsync(flags, b.flags.p, sizeof(flags), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flags[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: a speaker weight is not finite (the reference traps in Int(NaN))");
    n_raw = flags[1];
    return FA_SUCCESS;
}

struct FrameCopy {   // what the host reads back of the per-frame decision
    std::vector<int32_t> words, sel;
    std::vector<double> avg;
};

// the run walk, then everything the host needs back and the call's last synchronisation
fa_status walk_and_fetch(fa_ctx *ctx, const Call &c, const Wanted &want, Buffers &b, int64_t n_raw, std::vector<RawRun> &runs, FrameCopy &f) {
    hipStream_t st = ctx->stream;
    const int64_t T = b.args.T, items = T * b.args.smax;
    runs.resize(static_cast<size_t>(n_raw));
    if (n_raw > 0) {
        FA_TRY(fa::take(ctx, "reconstruct", {{&b.raw, sizeof(RawRun) * n_raw}}));
        launch_walk(st, b.args, b.starts.as<int64_t>(), b.flags.as<int32_t>() + 1, n_raw, b.raw.as<RawRun>());
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipMemcpyAsync(runs.data(), b.raw.p, sizeof(RawRun) * n_raw, hipMemcpyDeviceToHost, st));
    }
    if (want.words()) {
        f.words.resize(static_cast<size_t>(T));
        FA_HIP_TRY(ctx, hipMemcpyAsync(f.words.data(), b.word.p, sizeof(int32_t) * T, hipMemcpyDeviceToHost, st));
    }
    if (want.frames) {
        if (c.info->frame_clusters) { f.sel.resize(static_cast<size_t>(items)); FA_HIP_TRY(ctx, hipMemcpyAsync(f.sel.data(), b.sel.p, sizeof(int32_t) * items, hipMemcpyDeviceToHost, st)); }
        if (c.info->frame_averages) { f.avg.resize(static_cast<size_t>(items)); FA_HIP_TRY(ctx, hipMemcpyAsync(f.avg.data(), b.avg.p, sizeof(double) * items, hipMemcpyDeviceToHost, st)); }
        if (c.info->expected_count_sums) FA_HIP_TRY(ctx, hipMemcpyAsync(c.info->expected_count_sums, b.esum.p, sizeof(double) * T, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FA_SUCCESS;
}

// ZeroVoteReembedder.detectRuns (ZeroVoteReembedder.swift:42-79)
void detect_zero_vote_runs(const fa_reconstruct_config &cfg, fa_reconstruct_info *info, const std::vector<int32_t> &words, double fd) {
    const int64_t T = static_cast<int64_t>(words.size());
    int64_t n = 0;
    auto emit = [&](int64_t lo, int64_t hi) {
        if (!(static_cast<double>(hi - lo) * fd >= cfg.zero_vote_min_duration)) return;
        if (n < info->zero_vote_capacity) { info->zero_vote_runs[2 * n] = lo; info->zero_vote_runs[2 * n + 1] = hi; }
        ++n;
    };
    int64_t run0 = -1;
    for (int64_t g = 0; g < T; ++g) {
        if (words[g] & kZeroVote) { if (run0 < 0) run0 = g; }
        else if (run0 >= 0) { emit(run0, g); run0 = -1; }
    }
    if (run0 >= 0) emit(run0, T);
    info->zero_vote_run_count = n;
}

// the optional outputs of fa_reconstruct_info
void export_frames(const fa_reconstruct_config &cfg, fa_reconstruct_info *info, const Wanted &want, const FrameCopy &f, int32_t T, int32_t smax, double fd) {
    if (want.frames) {   // slots past a frame's active clusters were never written on the device: -1 / 0 here
        for (int64_t e = 0; e < static_cast<int64_t>(T) * smax; ++e) {
            const bool live = e % smax < (f.words[e / smax] & kSelMask);
            if (info->frame_clusters) info->frame_clusters[e] = live ? f.sel[e] : -1;
            if (info->frame_averages) info->frame_averages[e] = live ? f.avg[e] : 0.0;
        }
    }
    if (want.counts) for (int32_t g = 0; g < T; ++g) info->speaker_counts[g] = (f.words[g] >> kSelBits) & kSelMask;
    if (want.runs) detect_zero_vote_runs(cfg, info, f.words, fd);
}

// raw order: (closing frame, cluster) — see the header comment; then the appendSegment records (:400-429)
std::vector<fa_rttm_segment> raw_segments(std::vector<RawRun> &runs, int32_t T, double fd) {
    std::sort(runs.begin(), runs.end(), [](const RawRun &x, const RawRun &y) { return x.g1 != y.g1 ? x.g1 < y.g1 : x.k < y.k; });
    std::vector<fa_rttm_segment> raw;
    raw.reserve(runs.size());
    for (const RawRun &r : runs) {
        const double s = static_cast<double>(r.g0) * fd;
        const double e = r.g1 < T ? static_cast<double>(r.g1) * fd : static_cast<double>(T - 1) * fd + fd;
        if (!(e > s)) continue;
        fa_rttm_segment seg{};
        seg.start_seconds = static_cast<float>(s);
        seg.end_seconds = static_cast<float>(e);
        seg.quality = static_cast<float>(std::min(std::max(r.score / static_cast<double>(r.frames), 0.0), 1.0));
        snprintf(seg.speaker_id, sizeof(seg.speaker_id), "S%d", r.k + 1);
        raw.push_back(seg);
    }
    return raw;
}

fa_status reconstruct(fa_ctx *ctx, const Call &c) {
    if (!ctx || !c.cfg || !c.count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: ctx, config and count are required");
    *c.count = 0;
    set_info(c.info, 0, 0, 0.0);
    return fa::no_throw(ctx, "reconstruct", [&]() -> fa_status {
        double fd = 0.0;
        FramePlan p;
        FA_TRY(make_plan(ctx, c, fd, p));
        if (p.T == 0) return FA_SUCCESS;
        fa::DeviceGuard guard(ctx->device);
        const Wanted want = wanted(c.info, p.T);
        Buffers b;
        int64_t n_raw = 0;
        std::vector<RawRun> runs;
        FrameCopy f;
        FA_TRY(stage(ctx, c, p, fd, want.frames && c.info->expected_count_sums, b));
        FA_TRY(decide_frames(ctx, b, n_raw));
        FA_TRY(walk_and_fetch(ctx, c, want, b, n_raw, runs, f));
        export_frames(*c.cfg, c.info, want, f, p.T, p.smax, fd);
        std::vector<fa_rttm_segment> raw = raw_segments(runs, p.T, fd);
        if (c.info) c.info->raw_segments = static_cast<int64_t>(raw.size());
        return write_segments(ctx, finalize(*c.cfg, std::move(raw)), c.out, c.capacity, c.count);
    });
}

fa_status powerset_decode(fa_ctx *ctx, const float *logits, int64_t C, int32_t F, int32_t classes, float *weights, float *log_probs, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (C < 0 || F < 0 || classes < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "powerset decode: negative size");
    const int64_t rows = C * F;
    if (rows == 0) return FA_SUCCESS;
    if ((classes > 0 && !logits) || !weights) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "powerset decode: bad arguments");
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_x, b_w, b_lp;
    const float *d_x = logits;
    float *d_w = weights, *d_lp = log_probs;
    if (!device) {
        const size_t xbytes = sizeof(float) * rows * std::max(classes, 1);   // without classes one float a row, never read: no upload then
        FA_TRY(fa::take(ctx, "powerset decode", {{&b_x, xbytes, true, classes > 0 ? logits : nullptr}, {&b_w, sizeof(float) * rows * 3}, {&b_lp, xbytes, log_probs != nullptr}}));
        d_x = b_x.as<float>();
        d_w = b_w.as<float>();
        d_lp = log_probs ? b_lp.as<float>() : nullptr;
    }
    launch_powerset(st, d_x, rows, classes, d_w, d_lp);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(weights, d_w, sizeof(float) * rows * 3, hipMemcpyDeviceToHost, st));
        if (log_probs && classes > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(log_probs, d_lp, sizeof(float) * rows * classes, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

void fa_reconstruct_default_config(fa_reconstruct_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->window_duration = 10.0;          // OfflineDiarizerTypes.swift:46-55
    cfg->frame_duration = 0.0;            // windowDuration / frames
    cfg->min_duration_on = 0.0;
    cfg->min_duration_off = 0.0;
    cfg->min_segment_duration = 1.0;      // :97-103
    cfg->min_gap_duration = 0.1;          // :204-214
    cfg->exclusive = 1;
    cfg->zero_vote_enabled = 0;           // :232-247
    cfg->zero_vote_min_duration = 0.4;
}

fa_status fa_powerset_decode_dev(fa_ctx *ctx, const float *d_logits, int64_t chunks, int32_t frames, int32_t classes, float *d_weights, float *d_log_probs) {
    return powerset_decode(ctx, d_logits, chunks, frames, classes, d_weights, d_log_probs, true);
}

fa_status fa_powerset_decode(fa_ctx *ctx, const float *logits, int64_t chunks, int32_t frames, int32_t classes, float *weights, float *log_probs) {
    return powerset_decode(ctx, logits, chunks, frames, classes, weights, log_probs, false);
}

fa_status fa_offline_chunk_assignments(int64_t n, const int32_t *chunk_indices, const int32_t *speaker_indices, const int32_t *labels, int32_t cluster_count,
                                       int32_t chunks, int32_t speakers, int32_t *hard) {
    if (n < 0 || chunks < 0 || speakers < 0 || (n > 0 && (!chunk_indices || !speaker_indices || !labels)) || (static_cast<int64_t>(chunks) * speakers > 0 && !hard))
        return FA_INVALID_ARGUMENT;
    for (int64_t i = 0; i < static_cast<int64_t>(chunks) * speakers; ++i) hard[i] = -2;   // OfflineDiarizerManager.swift:891-894
    for (int64_t i = 0; i < n; ++i) {                                                       // :896-908, later embeddings overwrite
        const int32_t c = chunk_indices[i], s = speaker_indices[i], k = labels[i];
        if (c < 0 || c >= chunks || s < 0 || s >= speakers || k < 0 || k >= cluster_count) continue;
        hard[static_cast<int64_t>(c) * speakers + s] = k;
    }
    return FA_SUCCESS;
}

fa_status fa_offline_reconstruct_dev(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *d_weights, int64_t chunks, int32_t frames, int32_t speakers,
                                     const double *offsets, int64_t n_offsets, const int32_t *hard, int32_t clusters, const int64_t *overrides,
                                     int64_t n_overrides, fa_rttm_segment *out, int64_t capacity, int64_t *count, fa_reconstruct_info *info) {
    return reconstruct(ctx, Call{cfg, d_weights, chunks, frames, speakers, offsets, n_offsets, hard, clusters, overrides, n_overrides, out, capacity, count, info, true});
}

fa_status fa_offline_reconstruct(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *weights, int64_t chunks, int32_t frames, int32_t speakers,
                                 const double *offsets, int64_t n_offsets, const int32_t *hard, int32_t clusters, const int64_t *overrides,
                                 int64_t n_overrides, fa_rttm_segment *out, int64_t capacity, int64_t *count, fa_reconstruct_info *info) {
    return reconstruct(ctx, Call{cfg, weights, chunks, frames, speakers, offsets, n_offsets, hard, clusters, overrides, n_overrides, out, capacity, count, info, false});
}

fa_status fa_segments_finalize(const fa_reconstruct_config *cfg, const fa_rttm_segment *raw, int64_t n, fa_rttm_segment *out, int64_t capacity, int64_t *count) {
    if (!cfg || !count || n < 0 || capacity < 0 || (n > 0 && !raw)) return FA_INVALID_ARGUMENT;
    *count = 0;
    return fa::no_throw(nullptr, "segments finalize", [&]() -> fa_status {
        return write_segments(nullptr, finalize(*cfg, std::vector<fa_rttm_segment>(raw, raw + n)), out, capacity, count);
    });
}

}  // extern "C"
