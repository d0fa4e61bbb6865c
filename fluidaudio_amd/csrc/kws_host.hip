// kws_host.hip — the host unit of the CTC word spotter (kernel: kws.hip, operands: kws_launch.h, everything decided from the arguments
// alone: kws_plan.h): a spotting call and a window call as their steps — plan, stage, launch, fetch, hand back to the plan, deliver —
// with every buffer, copy, launch and synchronisation of the stage, the per-term threshold (CtcKeywordSpotter.swift:217-222) and the
// C ABI.  Nothing here does a DP step, and nothing here indexes with a value the device wrote: Passes::absorb (kws_plan.h) does.
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "kws_launch.h"

namespace {

using fa::kws::Job;
using fa::kws::Problem;
using fa::kws::Record;
using fa::kws::WalkArgs;
constexpr float kDefaultMinScore = -15.0f;   // ContextBiasingConstants.defaultMinSpotterScore

// what the plan answered: its refusal goes to the context behind the entry's name
fa_status accepted(fa_ctx *ctx, const char *what, const fa::Verdict &v) {
    return v.status == FA_SUCCESS ? FA_SUCCESS : fa::set_error(ctx, v.status, "%s: %s", what, v.text);
}

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

// One pass over the arena: the jobs up, the cursor cleared, the walk, the cursor and the statuses down, then as many records as were
// reserved and fitted.  `state` and `recs` are the call's, reused from pass to pass.
struct SpotBuffers {
    fa::DevBuf jobs, arena, state;   // state: the cursor, then a status per job of the pass
    std::vector<char> host_state;
    std::vector<Record> recs;
    double device_ms = 0.0;          // the walks of every pass so far (fa_ctx_set_timing)
};

fa_status run_pass(fa_ctx *ctx, const WalkArgs &a, SpotBuffers &b, fa::kws::Passes &passes, const bool merge) {
    hipStream_t st = ctx->stream;
    const size_t take = passes.pass_jobs.size();
    FA_HIP_TRY(ctx, hipMemcpyAsync(b.jobs.p, passes.pass_jobs.data(), sizeof(Job) * take, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemsetAsync(b.state.p, 0, sizeof(unsigned long long), st));
    FA_TRY(launch_classes(ctx, a, b.jobs.as<Job>(), passes.n_class));
    b.host_state.resize(sizeof(unsigned long long) + sizeof(int32_t) * take);
    FA_HIP_TRY(ctx, hipMemcpyAsync(b.host_state.data(), b.state.p, b.host_state.size(), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    FA_TRY(fa::DeviceTiming{ctx}.read(&b.device_ms));
    unsigned long long cursor;
    std::memcpy(&cursor, b.host_state.data(), sizeof(cursor));
    const int64_t n_rec = passes.records(cursor);
    b.recs.resize(static_cast<size_t>(n_rec));
    if (n_rec > 0) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(b.recs.data(), b.arena.p, sizeof(Record) * n_rec, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const int32_t *status = reinterpret_cast<const int32_t *>(b.host_state.data() + sizeof(unsigned long long));
    return accepted(ctx, "kws_spot", passes.absorb(cursor, status, b.recs.data(), merge));
}

fa_status spot(fa_ctx *ctx, const float *lp, bool device, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
               const int32_t *valid_frames, const int32_t *tokens, const int64_t *offsets, int32_t keywords, const float *min_scores, int32_t blank_id,
               int32_t merge, fa_kws_detection *dets, int64_t capacity, int64_t *count, int64_t *utt_counts) {
    if (count) *count = 0;
    if (!ctx || !count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_spot: ctx and count are required");
    if (capacity < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_spot: negative capacity");
    return fa::no_throw(ctx, "kws_spot", [&]() -> fa_status {
        // plan
        Problem p;
        FA_TRY(accepted(ctx, "kws_spot", fa::kws::check_problem(lp, batch, frames, vocab, row_stride, matrix_stride, valid_frames, tokens, offsets, keywords, blank_id, p)));
        if (utt_counts) std::fill(utt_counts, utt_counts + batch, int64_t{0});
        std::vector<Job> jobs;
        int64_t worst_one = 0;
        FA_TRY(accepted(ctx, "kws_spot", fa::kws::spot_jobs(p, jobs, worst_one)));
        const int64_t J = static_cast<int64_t>(jobs.size());
        if (J == 0) return FA_SUCCESS;
        const char *forced = fa::sw(fa::Sw::KWS_ARENA);   // tests ask for a smaller arena
        const fa::kws::Arena arena = fa::kws::arena_of(J, capacity, forced ? std::max<int64_t>(0, std::atoll(forced)) : fa::kws::kArenaNotForced, worst_one);

        // stage
        fa::DeviceGuard guard(ctx->device);
        fa::DevBuf b_lp;
        const float *d_lp = lp;
        if (!device) FA_TRY(upload_log_probs(ctx, p, lp, b_lp, d_lp));
        DeviceKeywords dk;
        FA_TRY(upload_keywords(ctx, p, min_scores, dk));
        SpotBuffers b;
        const size_t state_bytes = sizeof(unsigned long long) + sizeof(int32_t) * static_cast<size_t>(J);
        FA_TRY(fa::take(ctx, "kws_spot", {{&b.jobs, sizeof(Job) * J}, {&b.arena, sizeof(Record) * arena.cap}, {&b.state, state_bytes}}));
        WalkArgs a = walk_args(p, d_lp, dk);
        a.arena = b.arena.as<Record>(); a.arena_cap = arena.cap; a.cursor = b.state.as<unsigned long long>();
        a.status = reinterpret_cast<int32_t *>(b.state.as<char>() + sizeof(unsigned long long));

        // the passes, then the detections in the reference's order
        fa::kws::Passes passes;
        passes.begin(p, jobs, arena);
        while (passes.next()) FA_TRY(run_pass(ctx, a, b, passes, merge != 0));
        return accepted(ctx, "kws_spot", fa::kws::deliver(jobs, passes.done, dets, capacity, count, utt_counts));
    });
}

fa_status score_windows(fa_ctx *ctx, const float *lp, bool device, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                        const int32_t *valid_frames, const int32_t *tokens, const int64_t *offsets, int32_t keywords, const fa_kws_window *windows,
                        int64_t n_windows, int32_t blank_id, fa_kws_detection *out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_windows < 0 || n_windows >= INT32_MAX || (n_windows > 0 && (!windows || !out))) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "kws_windows: bad arguments");
    return fa::no_throw(ctx, "kws_windows", [&]() -> fa_status {
        // plan: every window answered as it stands without a walk, the others as one launch's jobs
        Problem p;
        FA_TRY(accepted(ctx, "kws_windows", fa::kws::check_problem(lp, batch, frames, vocab, row_stride, matrix_stride, valid_frames, tokens, offsets, keywords, blank_id, p)));
        fa::kws::WindowPlan plan;
        FA_TRY(accepted(ctx, "kws_windows", fa::kws::window_jobs(p, windows, n_windows, out, plan)));
        const size_t J = plan.jobs.size();
        if (J == 0) return FA_SUCCESS;

        // stage
        fa::DeviceGuard guard(ctx->device);
        hipStream_t st = ctx->stream;
        fa::DevBuf b_lp;
        const float *d_lp = lp;
        if (!device) FA_TRY(upload_log_probs(ctx, p, lp, b_lp, d_lp));
        DeviceKeywords dk;
        FA_TRY(upload_keywords(ctx, p, nullptr, dk));
        fa::DevBuf b_jobs, b_out;
        FA_TRY(fa::take(ctx, "kws_windows", {{&b_jobs, sizeof(Job) * J, true, plan.jobs.data()}, {&b_out, sizeof(Record) * J}}));
        WalkArgs a = walk_args(p, d_lp, dk);
        a.constrained = 1;
        a.out = b_out.as<Record>();

        // walk, fetch, and each job's answer into its window
        double device_ms = 0.0;
        FA_TRY(launch_classes(ctx, a, b_jobs.as<Job>(), plan.n_class));
        std::vector<Record> recs(J);
        FA_HIP_TRY(ctx, hipMemcpyAsync(recs.data(), b_out.p, sizeof(Record) * J, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation behind the uploads
        FA_TRY(fa::DeviceTiming{ctx}.read(&device_ms));
        for (size_t i = 0; i < J; ++i) {
            fa_kws_detection &d = out[plan.window_of[i]];
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
