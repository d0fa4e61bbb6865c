// kws_host.hip — the host side of the CTC word spotter (kernel: kws.hip, shared operands: kws_launch.h): the argument pass, the job
// lists, the arena passes, mergeOverlap (CtcDPAlgorithm.swift:372-391), the per-term threshold (CtcKeywordSpotter.swift:217-222) and the
// C ABI.  Nothing here does a DP step; what is decided here is decided from the arguments alone, before any device work.
//
// A spotting call makes one job per (utterance, keyword) that can match at all (1 <= tokens <= valid frames), ordered by utterance, and
// launches them by width class (1, 2 or 4 states per lane).  The candidates come back through an arena of O(jobs + capacity) records.
// The first pass takes every job; a job whose chunk did not fit reports -1 and is walked again, by passes that take only as many jobs
// as fit the arena at the most candidates a job can have (every other sample of its scan), so each of those passes finishes all its
// jobs.  Sort-by-start and merge run here, on the records, as fa_offline_reconstruct finishes its segments: only records cross PCIe.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>

#include "kws_launch.h"

namespace {

using fa::kws::Job;
using fa::kws::Record;
using fa::kws::WalkArgs;
constexpr int kChunk = fa::kws::kChunk;
constexpr float kDefaultMinScore = -15.0f;   // ContextBiasingConstants.defaultMinSpotterScore

struct Problem {   // the validated arguments both entries share
    int32_t batch = 0, frames = 0, vocab = 0, keywords = 0, blank = 0;
    int64_t row_stride = 0, matrix_stride = 0;
    const int32_t *tokens = nullptr;
    const int64_t *off = nullptr;
    std::vector<int32_t> valid;   // frames of each utterance, clamped to [0, frames]
    int32_t len(const int32_t k) const { return static_cast<int32_t>(off[k + 1] - off[k]); }
};

fa_status check_problem(fa_ctx *ctx, const char *what, const float *lp, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                        const int32_t *valid_frames, const int32_t *tokens, const int64_t *off, int32_t keywords, int32_t blank, Problem &p) {
    if (batch < 0 || frames < 0 || vocab < 1 || row_stride < vocab || keywords < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: bad shape", what);
    if (batch > 0 && frames > 0 && (!lp || (batch > 1 && matrix_stride < static_cast<int64_t>(frames - 1) * row_stride + vocab)))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: bad log-prob pointer or strides", what);
    if (keywords > 0 && !off) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: keyword_offsets is required", what);
    if (keywords > 0 && off[0] < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: keyword_offsets starts below 0", what);
    for (int32_t k = 0; k < keywords; ++k) {
        const int64_t n = off[k + 1] - off[k];
        if (n < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: keyword_offsets does not ascend at keyword %d", what, k);
        if (n > FA_KWS_MAX_TOKENS) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: keyword %d has %lld tokens, at most %d are supported", what, k, (long long)n, (int)FA_KWS_MAX_TOKENS);
    }
    if (keywords > 0 && off[keywords] > off[0] && !tokens) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: keyword_tokens is required", what);
    p.batch = batch; p.frames = frames; p.vocab = vocab; p.keywords = keywords; p.blank = blank;
    p.row_stride = row_stride; p.matrix_stride = matrix_stride; p.tokens = tokens; p.off = off;
    p.valid.assign(static_cast<size_t>(batch), frames);
    if (valid_frames)
        for (int32_t b = 0; b < batch; ++b) p.valid[b] = std::min(frames, std::max(0, valid_frames[b]));
    return FA_SUCCESS;
}

inline int class_of(const int32_t tokens) { return tokens <= fa::kws::max_tokens(1) ? 0 : (tokens <= fa::kws::max_tokens(2) ? 1 : 2); }

// the keywords on the device: tokens, offsets from 0, thresholds
struct DeviceKeywords {
    fa::DevBuf tokens, off, min_score;
};

fa_status upload_keywords(fa_ctx *ctx, const Problem &p, const float *min_scores, DeviceKeywords &d) {
    const int64_t n_tok = p.off[p.keywords] - p.off[0];
    std::vector<int64_t> off(static_cast<size_t>(p.keywords) + 1);
    for (int32_t k = 0; k <= p.keywords; ++k) off[k] = p.off[k] - p.off[0];
    std::vector<float> mins(static_cast<size_t>(p.keywords), kDefaultMinScore);
    if (min_scores) std::copy(min_scores, min_scores + p.keywords, mins.begin());
    FA_TRY(fa::take(ctx, "kws", {{&d.tokens, sizeof(int32_t) * n_tok, true, n_tok > 0 ? p.tokens + p.off[0] : nullptr},
                                 {&d.off, sizeof(int64_t) * off.size(), true, off.data()}, {&d.min_score, sizeof(float) * mins.size(), true, mins.data()}}));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the staging vectors end with this scope
    return FA_SUCCESS;
}

// the host-pointer entries: the matrices as they are laid out, up to the last column read (there is a job, so batch, frames >= 1)
fa_status upload_log_probs(fa_ctx *ctx, const Problem &p, const float *lp, fa::DevBuf &buf, const float *&d_lp) {
    const size_t n = static_cast<size_t>(p.batch - 1) * p.matrix_stride + static_cast<size_t>(p.frames - 1) * p.row_stride + p.vocab;
    FA_TRY(fa::take(ctx, "kws", {{&buf, sizeof(float) * n, true, lp}}));
    d_lp = buf.as<float>();
    return FA_SUCCESS;
}

WalkArgs walk_args(const Problem &p, const float *d_lp, const DeviceKeywords &d) {
    WalkArgs a{};
    a.lp = d_lp; a.row_stride = p.row_stride; a.matrix_stride = p.matrix_stride; a.vocab = p.vocab; a.blank = p.blank;
    a.tokens = d.tokens.as<int32_t>(); a.kw_off = d.off.as<int64_t>(); a.kw_min = d.min_score.as<float>();
    return a;
}

// `ids` (indices into `jobs`) reordered by width class, each class in its former order; n[c] jobs in class c
void order_by_class(const Problem &p, const std::vector<Job> &jobs, std::vector<int32_t> &ids, int32_t (&n)[3]) {
    std::vector<int32_t> out;
    out.reserve(ids.size());
    for (int c = 0; c < 3; ++c) {
        n[c] = 0;
        for (const int32_t i : ids)
            if (class_of(p.len(jobs[i].keyword)) == c) { out.push_back(i); ++n[c]; }
    }
    ids.swap(out);
}

// the launches of one job list that is ordered by class; the bracket for fa_ctx_set_timing adds up over the passes of a call
fa_status launch_classes(fa_ctx *ctx, WalkArgs a, const Job *d_jobs, const int32_t (&n)[3]) {
    FA_TRY(fa::DeviceTiming{ctx}.begin());
    int32_t base = 0;
    for (int c = 0; c < 3; ++c) {
        a.jobs = d_jobs + base; a.n_jobs = n[c]; a.job_base = base;
        fa::kws::launch_walk(ctx->stream, a, 1 << c);
        base += n[c];
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    return fa::DeviceTiming{ctx}.end();
}

// mergeOverlap (:374-391) on one job's candidates, which arrive in the order of their end samples
void merge_overlap(std::vector<Record> &c) {
    std::stable_sort(c.begin(), c.end(), [](const Record &x, const Record &y) { return x.start < y.start; });
    size_t m = 0;
    for (size_t i = 0; i < c.size(); ++i) {
        if (m > 0 && c[i].start <= c[m - 1].end) {
            Record best = c[i].score > c[m - 1].score ? c[i] : c[m - 1];
            best.end = std::max(c[m - 1].end, c[i].end);
            c[m - 1] = best;
        } else {
            c[m++] = c[i];
        }
    }
    c.resize(m);
}

// the most candidates a job can have, rounded up to whole chunks: every other sample of its scan t = N ... T, or the one fallback
inline int64_t worst_records(const Problem &p, const Job &j) {
    const int64_t samples = static_cast<int64_t>(j.t1 - j.t0) - p.len(j.keyword) + 1;
    return ((samples + 1) / 2 + kChunk - 1) / kChunk * kChunk;
}

fa_status spot(fa_ctx *ctx, const float *lp, bool device, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
               const int32_t *valid_frames, const int32_t *tokens, const int64_t *offsets, int32_t keywords, const float *min_scores, int32_t blank_id,
               int32_t merge, fa_kws_detection *dets, int64_t capacity, int64_t *count, int64_t *utt_counts) {
    if (count) *count = 0;
    if (!ctx || !count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_spot: ctx and count are required");
    if (capacity < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_spot: negative capacity");
    return fa::no_throw(ctx, "kws_spot", [&]() -> fa_status {
    Problem p;
    FA_TRY(check_problem(ctx, "kws_spot", lp, batch, frames, vocab, row_stride, matrix_stride, valid_frames, tokens, offsets, keywords, blank_id, p));
    if (utt_counts) std::fill(utt_counts, utt_counts + batch, int64_t{0});
    std::vector<Job> jobs;
    int64_t worst_one = kChunk;
    for (int32_t u = 0; u < batch; ++u)
        for (int32_t k = 0; k < keywords; ++k) {
            const int32_t n = p.len(k), T = p.valid[u];
            if (n == 0 || T == 0 || T < n) continue;   // :321-323, :336
            if (jobs.size() >= static_cast<size_t>(INT32_MAX - 1)) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "kws_spot: 2^31 jobs or more");
            jobs.push_back(Job{u, k, 0, T});
            worst_one = std::max(worst_one, worst_records(p, jobs.back()));
        }
    const int64_t J = static_cast<int64_t>(jobs.size());
    if (J == 0) return FA_SUCCESS;

    // the arena: O(jobs + capacity) records, never less than one job can need; FA_KWS_ARENA (tests) asks for a smaller one
    int64_t cap = std::max<int64_t>(65536, 2 * J + std::min<int64_t>(capacity, int64_t{1} << 26));
    if (const char *e = fa::sw(fa::Sw::KWS_ARENA)) cap = std::max<int64_t>(0, std::atoll(e));
    cap = std::max(worst_one, (cap + kChunk - 1) / kChunk * kChunk);
    const int64_t slice = std::max<int64_t>(1, cap / worst_one);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_lp;
    const float *d_lp = lp;
    if (!device) FA_TRY(upload_log_probs(ctx, p, lp, b_lp, d_lp));
    DeviceKeywords dk;
    FA_TRY(upload_keywords(ctx, p, min_scores, dk));
    fa::DevBuf b_jobs, b_arena, b_state;   // b_state: the cursor, then a status per job of the pass
    const size_t state_bytes = sizeof(unsigned long long) + sizeof(int32_t) * static_cast<size_t>(J);
    FA_TRY(fa::take(ctx, "kws_spot", {{&b_jobs, sizeof(Job) * J}, {&b_arena, sizeof(Record) * cap}, {&b_state, state_bytes}}));
    WalkArgs a = walk_args(p, d_lp, dk);
    a.arena = b_arena.as<Record>(); a.arena_cap = cap; a.cursor = b_state.as<unsigned long long>();
    a.status = reinterpret_cast<int32_t *>(b_state.as<char>() + sizeof(unsigned long long));

    std::vector<Record> done;   // finished candidates; .job is the index into `jobs`
    std::vector<int32_t> pending(static_cast<size_t>(J));
    std::iota(pending.begin(), pending.end(), 0);
    std::vector<Job> pass_jobs;
    std::vector<char> state;
    std::vector<Record> recs, mine;
    std::vector<int64_t> first;
    double device_ms = 0.0;
    int passes = 0;
    while (!pending.empty()) {
        const size_t take = passes == 0 ? pending.size() : std::min<size_t>(pending.size(), static_cast<size_t>(slice));
        std::vector<int32_t> ids(pending.begin(), pending.begin() + take);
        int32_t n_class[3];
        order_by_class(p, jobs, ids, n_class);
        pass_jobs.resize(take);
        for (size_t i = 0; i < take; ++i) pass_jobs[i] = jobs[ids[i]];
        FA_HIP_TRY(ctx, hipMemcpyAsync(b_jobs.p, pass_jobs.data(), sizeof(Job) * take, hipMemcpyHostToDevice, st));
        FA_HIP_TRY(ctx, hipMemsetAsync(b_state.p, 0, sizeof(unsigned long long), st));
        FA_TRY(launch_classes(ctx, a, b_jobs.as<Job>(), n_class));
        state.resize(sizeof(unsigned long long) + sizeof(int32_t) * take);
        FA_HIP_TRY(ctx, hipMemcpyAsync(state.data(), b_state.p, state.size(), hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        FA_TRY(fa::DeviceTiming{ctx}.read(&device_ms));
        unsigned long long cursor;
        std::memcpy(&cursor, state.data(), sizeof(cursor));
        const int32_t *status = reinterpret_cast<const int32_t *>(state.data() + sizeof(unsigned long long));
        const int64_t n_rec = static_cast<int64_t>(std::min<unsigned long long>(cursor, static_cast<unsigned long long>(cap)));
        recs.resize(static_cast<size_t>(n_rec));
        if (n_rec > 0) {
            FA_HIP_TRY(ctx, hipMemcpyAsync(recs.data(), b_arena.p, sizeof(Record) * n_rec, hipMemcpyDeviceToHost, st));
            FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        // the records of each job, in arena order: a job's chunks were reserved one after the other
        first.assign(take + 1, 0);
        for (const Record &r : recs) {
            if (r.job < 0) continue;
            if (static_cast<size_t>(r.job) >= take) return fa::set_error(ctx, FA_RUNTIME_ERROR, "kws_spot: a record names job %d of %zu", r.job, take);
            ++first[r.job + 1];
        }
        for (size_t i = 0; i < take; ++i) first[i + 1] += first[i];
        std::vector<Record> sorted(static_cast<size_t>(first[take]));
        {
            std::vector<int64_t> at(first.begin(), first.end() - 1);
            for (const Record &r : recs)
                if (r.job >= 0) sorted[static_cast<size_t>(at[r.job]++)] = r;
        }
        std::vector<int32_t> again;
        for (size_t i = 0; i < take; ++i) {
            if (status[i] < 0) {
                if (passes > 0) return fa::set_error(ctx, FA_RUNTIME_ERROR, "kws_spot: a job overflowed an arena sized for it");
                again.push_back(ids[i]);
                continue;
            }
            if (first[i + 1] - first[i] != status[i]) return fa::set_error(ctx, FA_RUNTIME_ERROR, "kws_spot: job %zu wrote %lld of %d records", i, (long long)(first[i + 1] - first[i]), status[i]);
            mine.assign(sorted.begin() + first[i], sorted.begin() + first[i + 1]);
            if (merge) merge_overlap(mine);
            for (Record r : mine) { r.job = ids[i]; done.push_back(r); }
        }
        std::sort(again.begin(), again.end());   // back in utterance order
        again.insert(again.end(), pending.begin() + take, pending.end());
        pending.swap(again);
        ++passes;
    }
    // by utterance, then keyword (the job order), then as the reference's array holds them; one pass leaves them by class
    std::stable_sort(done.begin(), done.end(), [](const Record &x, const Record &y) { return x.job < y.job; });
    const int64_t total = static_cast<int64_t>(done.size());
    *count = total;
    if (utt_counts) for (const Record &r : done) ++utt_counts[jobs[r.job].utterance];
    if (!dets || total == 0) return FA_SUCCESS;
    for (int64_t i = 0, n = std::min(total, capacity); i < n; ++i) dets[i] = fa_kws_detection{jobs[done[i].job].utterance, jobs[done[i].job].keyword, done[i].score, done[i].start, done[i].end};
    if (capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "kws_spot: output holds %lld of %lld detections", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

fa_status score_windows(fa_ctx *ctx, const float *lp, bool device, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                        const int32_t *valid_frames, const int32_t *tokens, const int64_t *offsets, int32_t keywords, const fa_kws_window *windows,
                        int64_t n_windows, int32_t blank_id, fa_kws_detection *out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_windows < 0 || n_windows >= INT32_MAX || (n_windows > 0 && (!windows || !out))) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_windows: bad arguments");
    return fa::no_throw(ctx, "kws_windows", [&]() -> fa_status {
    Problem p;
    FA_TRY(check_problem(ctx, "kws_windows", lp, batch, frames, vocab, row_stride, matrix_stride, valid_frames, tokens, offsets, keywords, blank_id, p));
    for (int64_t w = 0; w < n_windows; ++w)
        if (windows[w].utterance < 0 || windows[w].utterance >= batch || windows[w].keyword < 0 || windows[w].keyword >= keywords)
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_windows: window %lld names utterance %d, keyword %d", (long long)w, windows[w].utterance, windows[w].keyword);
    std::vector<Job> jobs;
    std::vector<int32_t> ids;   // the jobs by utterance: the workgroups share rows
    std::vector<int64_t> window_of;
    for (int64_t w = 0; w < n_windows; ++w) {
        const fa_kws_window &q = windows[w];
        const int32_t n = p.len(q.keyword), t0 = std::max(0, q.start_frame), t1 = std::min(p.valid[q.utterance], q.end_frame);   // :260-261
        out[w] = fa_kws_detection{q.utterance, q.keyword, -INFINITY, t0, t0};                                                 // :263-272
        if (n == 0 || t1 <= t0 || t1 - t0 < n) continue;
        ids.push_back(static_cast<int32_t>(jobs.size()));
        jobs.push_back(Job{q.utterance, q.keyword, t0, t1});
        window_of.push_back(w);
    }
    const size_t J = jobs.size();
    if (J == 0) return FA_SUCCESS;
    std::stable_sort(ids.begin(), ids.end(), [&](const int32_t x, const int32_t y) { return jobs[x].utterance < jobs[y].utterance; });
    int32_t n_class[3];
    order_by_class(p, jobs, ids, n_class);
    std::vector<Job> pass_jobs(J);
    for (size_t i = 0; i < J; ++i) pass_jobs[i] = jobs[ids[i]];

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_lp;
    const float *d_lp = lp;
    if (!device) FA_TRY(upload_log_probs(ctx, p, lp, b_lp, d_lp));
    DeviceKeywords dk;
    FA_TRY(upload_keywords(ctx, p, nullptr, dk));
    fa::DevBuf b_jobs, b_out;
    FA_TRY(fa::take(ctx, "kws_windows", {{&b_jobs, sizeof(Job) * J, true, pass_jobs.data()}, {&b_out, sizeof(Record) * J}}));
    WalkArgs a = walk_args(p, d_lp, dk);
    a.constrained = 1;
    a.out = b_out.as<Record>();
    double device_ms = 0.0;
    FA_TRY(launch_classes(ctx, a, b_jobs.as<Job>(), n_class));
    std::vector<Record> recs(J);
    FA_HIP_TRY(ctx, hipMemcpyAsync(recs.data(), b_out.p, sizeof(Record) * J, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation behind the uploads
    FA_TRY(fa::DeviceTiming{ctx}.read(&device_ms));
    for (size_t i = 0; i < J; ++i) {
        fa_kws_detection &d = out[window_of[ids[i]]];
        d.score = recs[i].score; d.start_frame = recs[i].start; d.end_frame = recs[i].end;
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

float fa_kws_adjusted_threshold(int32_t has_base, float base, int32_t token_count) {
    if (!has_base) return kDefaultMinScore;
    return base - static_cast<float>(std::max(0, token_count - 3)) * 1.0f;   // baselineTokenCountForThreshold, thresholdRelaxationPerToken
}

fa_status fa_ctc_kws_spot_batch_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride,
                                    int64_t matrix_stride, const int32_t *valid_frames, const int32_t *keyword_tokens, const int64_t *keyword_offsets,
                                    int32_t keywords, const float *min_scores, int32_t blank_id, int32_t merge_overlap, fa_kws_detection *dets,
                                    int64_t capacity, int64_t *count, int64_t *utterance_counts) {
    return spot(ctx, d_log_probs, true, batch, frames, vocab, row_stride, matrix_stride, valid_frames, keyword_tokens, keyword_offsets, keywords, min_scores,
                blank_id, merge_overlap, dets, capacity, count, utterance_counts);
}

fa_status fa_ctc_kws_spot_batch(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                                const int32_t *valid_frames, const int32_t *keyword_tokens, const int64_t *keyword_offsets, int32_t keywords,
                                const float *min_scores, int32_t blank_id, int32_t merge_overlap, fa_kws_detection *dets, int64_t capacity, int64_t *count,
                                int64_t *utterance_counts) {
    return spot(ctx, log_probs, false, batch, frames, vocab, row_stride, matrix_stride, valid_frames, keyword_tokens, keyword_offsets, keywords, min_scores,
                blank_id, merge_overlap, dets, capacity, count, utterance_counts);
}

fa_status fa_ctc_kws_score_windows_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride,
                                       int64_t matrix_stride, const int32_t *valid_frames, const int32_t *keyword_tokens, const int64_t *keyword_offsets,
                                       int32_t keywords, const fa_kws_window *windows, int64_t n_windows, int32_t blank_id, fa_kws_detection *out) {
    return score_windows(ctx, d_log_probs, true, batch, frames, vocab, row_stride, matrix_stride, valid_frames, keyword_tokens, keyword_offsets, keywords, windows,
                         n_windows, blank_id, out);
}

fa_status fa_ctc_kws_score_windows(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                                   const int32_t *valid_frames, const int32_t *keyword_tokens, const int64_t *keyword_offsets, int32_t keywords,
                                   const fa_kws_window *windows, int64_t n_windows, int32_t blank_id, fa_kws_detection *out) {
    return score_windows(ctx, log_probs, false, batch, frames, vocab, row_stride, matrix_stride, valid_frames, keyword_tokens, keyword_offsets, keywords, windows,
                         n_windows, blank_id, out);
}

}  // extern "C"
