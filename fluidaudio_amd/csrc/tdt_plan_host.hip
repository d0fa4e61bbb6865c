// tdt_plan_host.hip — the host side of the TDT window planner (kernels: tdt_plan.hip, shared operands and the argument pass:
// tdt_plan_launch.h, the shared integer arithmetic: tdt_plan_core.h): the uploads of the host-pointer entries, the workspace, the
// synchronisation of a call and the C ABI.  What is decided here is decided from the arguments alone, before any device work.
#include <algorithm>
#include <cmath>
#include <limits>

#include "fa_common.h"
#include "tdt_plan_launch.h"

namespace {

namespace tp = fa::tdt_plan;

struct Five {
    int32_t *audio_frames, *t0, *is_last, *global_offset, *emit_after;
};

fa_status plan(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets, const int32_t batch, fa_tdt_window *windows, const int64_t capacity,
               int64_t *window_range, const Five five, int64_t *speech_end, int32_t *statuses, const bool device) {
    return fa::no_throw(ctx, "tdt_plan_windows", [&]() -> fa_status {
    tp::Geometry g{};
    tp::Plan p;
    const fa::Verdict v = tp::plan_windows(tp::config_or_default(cfg), audio, audio_offsets, batch, windows, capacity, window_range, device, &g, &p);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0) return FA_SUCCESS;
    const size_t B = static_cast<size_t>(batch), slots = static_cast<size_t>(std::min(capacity, p.bound));
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_offsets[batch] - audio_offsets[0]);
    int32_t *const host_five[5] = {five.audio_frames, five.t0, five.is_last, five.global_offset, five.emit_after};

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_rec, b_audio, b_table, b_bad, b_end, b_starts, b_counts, b_kept, b_total, b_out, b_five[5];
    FA_TRY(fa::take(ctx, "tdt_plan_windows",
                    {{&b_rec, sizeof(tp::Recording) * B, true, p.rec.data()}, {&b_audio, audio_bytes, !device, device ? nullptr : audio + audio_offsets[0]},
                     {&b_table, sizeof(float) * static_cast<size_t>(p.table)}, {&b_bad, sizeof(int32_t) * B}, {&b_end, sizeof(int64_t) * B},
                     {&b_starts, sizeof(int64_t) * static_cast<size_t>(p.starts), g.aligned != 0}, {&b_counts, sizeof(int32_t) * B}, {&b_kept, sizeof(int32_t) * B},
                     {&b_total, sizeof(int32_t)}, {&b_out, sizeof(fa_tdt_window) * slots},
                     {&b_five[0], sizeof(int32_t) * slots, !device && host_five[0]}, {&b_five[1], sizeof(int32_t) * slots, !device && host_five[1]},
                     {&b_five[2], sizeof(int32_t) * slots, !device && host_five[2]}, {&b_five[3], sizeof(int32_t) * slots, !device && host_five[3]},
                     {&b_five[4], sizeof(int32_t) * slots, !device && host_five[4]}}));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_bad.p, 0, sizeof(int32_t) * B, st));
    tp::PlanArgs a{};
    a.audio = device ? audio : b_audio.as<float>();
    a.rec = b_rec.as<tp::Recording>();
    a.batch = batch; a.tiles = static_cast<int32_t>(p.tiles);
    a.g = g;
    a.table = b_table.as<float>(); a.sums = nullptr; a.bad = b_bad.as<int32_t>();
    a.speech_end = b_end.as<int64_t>(); a.starts = b_starts.as<int64_t>();
    a.counts = b_counts.as<int32_t>(); a.counts_kept = b_kept.as<int32_t>(); a.total = b_total.as<int32_t>();
    a.out = b_out.as<fa_tdt_window>();
    a.audio_frames = device ? five.audio_frames : b_five[0].as<int32_t>(); a.t0 = device ? five.t0 : b_five[1].as<int32_t>();
    a.is_last = device ? five.is_last : b_five[2].as<int32_t>(); a.global_offset = device ? five.global_offset : b_five[3].as<int32_t>();
    a.emit_after = device ? five.emit_after : b_five[4].as<int32_t>();
    a.capacity = capacity;
    tp::launch_plan(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> counts(B), bad(B);
    std::vector<int64_t> ends(B);
    std::vector<fa_tdt_window> got(slots);
    std::vector<int32_t> got_five[5];
    FA_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), b_kept.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(bad.data(), b_bad.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(ends.data(), b_end.p, sizeof(int64_t) * B, hipMemcpyDeviceToHost, st));
    if (slots) FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_out.p, sizeof(fa_tdt_window) * slots, hipMemcpyDeviceToHost, st));
    for (int k = 0; k < 5; ++k)
        if (!device && host_five[k] && slots) {
            got_five[k].resize(slots);
            FA_HIP_TRY(ctx, hipMemcpyAsync(got_five[k].data(), b_five[k].p, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, st));
        }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    window_range[0] = 0;
    for (size_t b = 0; b < B; ++b) {
        if (counts[b] < 0 || counts[b] > p.rec[b].bound)
            return fa::set_error(ctx, FA_RUNTIME_ERROR, "tdt_plan_windows: recording %zu reports %d windows, its bound is %lld", b, counts[b], (long long)p.rec[b].bound);
        window_range[b + 1] = window_range[b] + counts[b];
        if (speech_end) speech_end[b] = ends[b];
        if (statuses) statuses[b] = bad[b] ? FA_INVALID_ARGUMENT : FA_SUCCESS;
    }
    const int64_t total = window_range[batch];
    if (capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "tdt_plan_windows: output holds %lld of %lld windows", (long long)capacity, (long long)total);
    std::copy(got.begin(), got.begin() + total, windows);
    for (int k = 0; k < 5; ++k)
        if (!got_five[k].empty()) std::copy(got_five[k].begin(), got_five[k].begin() + total, host_five[k]);
    return FA_SUCCESS;
    });
}

fa_status pack(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets, const int32_t batch, const fa_tdt_window *windows,
               const int64_t n_windows, float *rows, const int64_t row_capacity, int32_t *lengths, const bool device) {
    return fa::no_throw(ctx, "tdt_pack_windows", [&]() -> fa_status {
    tp::Geometry g{};
    const fa::Verdict v = tp::plan_pack(tp::config_or_default(cfg), audio, audio_offsets, batch, windows, n_windows, rows, row_capacity, &g);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_windows == 0) return FA_SUCCESS;
    const int64_t a0 = device ? 0 : audio_offsets[0];
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_offsets[batch] - a0);
    const size_t n = static_cast<size_t>(n_windows), row_bytes = sizeof(float) * static_cast<size_t>(g.max_model) * n;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_audio, b_rows, b_lengths;
    FA_TRY(fa::take(ctx, "tdt_pack_windows", {{&b_audio, audio_bytes, !device, device ? nullptr : audio + a0}, {&b_rows, device ? 0 : row_bytes, !device},
                                              {&b_lengths, sizeof(int32_t) * n, !device && lengths}}));
    const float *d_audio = device ? audio : b_audio.as<float>();
    float *d_rows = device ? rows : b_rows.as<float>();
    int32_t *d_lengths = device ? lengths : (lengths ? b_lengths.as<int32_t>() : nullptr);
    const bool wide = reinterpret_cast<uintptr_t>(d_rows) % 16 == 0 && g.max_model % 4 == 0;   // then every row is aligned
    const auto fill = [&](fa::rows::Group &group, const int64_t i, const int32_t k) {
        group.src[k] = audio_offsets[windows[i].recording] - a0 + windows[i].context_start;
        group.len[k] = static_cast<int32_t>(windows[i].length);
    };
    fa::rows::for_each_group(n_windows, fill, [&](const fa::rows::Group &group, const int64_t w0) {
        tp::launch_pack(st, d_audio, group, g.max_model, d_rows + w0 * g.max_model, d_lengths ? d_lengths + w0 : nullptr, wide);
    });
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(rows, b_rows.p, row_bytes, hipMemcpyDeviceToHost, st));
        if (lengths) FA_HIP_TRY(ctx, hipMemcpyAsync(lengths, b_lengths.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the host entry's one synchronisation: its buffers are its own
    }
    return FA_SUCCESS;
    });
}

fa_status gate(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets, const int32_t batch, const float *override_thresholds,
               float *thresholds, const fa_tdt_span *spans, const int64_t n_spans, int64_t *span_frames, double *span_seconds, int32_t *statuses, const bool device) {
    return fa::no_throw(ctx, "tdt_speech_gate", [&]() -> fa_status {
    tp::Geometry g{};
    tp::GatePlan p;
    const fa_tdt_window_config c = tp::config_or_default(cfg);
    const fa::Verdict v = tp::plan_gate(c, audio, audio_offsets, batch, spans, n_spans, device, &g, &p);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0) return FA_SUCCESS;       // without recordings there are no spans
    const size_t B = static_cast<size_t>(batch), S = static_cast<size_t>(n_spans);
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_offsets[batch] - audio_offsets[0]);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_rec, b_audio, b_table, b_sums, b_bad, b_thr, b_over, b_spans, b_frames;
    FA_TRY(fa::take(ctx, "tdt_speech_gate",
                    {{&b_rec, sizeof(tp::Recording) * B, true, p.base.rec.data()}, {&b_audio, audio_bytes, !device, device ? nullptr : audio + audio_offsets[0]},
                     {&b_table, sizeof(float) * static_cast<size_t>(p.base.table)}, {&b_sums, sizeof(float) * static_cast<size_t>(p.base.sums)}, {&b_bad, sizeof(int32_t) * B},
                     {&b_thr, sizeof(float) * B}, {&b_over, sizeof(float) * B, override_thresholds != nullptr, override_thresholds},
                     {&b_spans, sizeof(tp::Span) * S, S > 0, p.spans.data()}, {&b_frames, sizeof(int64_t) * S, S > 0}}));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_bad.p, 0, sizeof(int32_t) * B, st));
    tp::GateArgs a{};
    a.plan.audio = device ? audio : b_audio.as<float>();
    a.plan.rec = b_rec.as<tp::Recording>();
    a.plan.batch = batch; a.plan.tiles = static_cast<int32_t>(p.base.tiles);
    a.plan.g = g;
    a.plan.table = b_table.as<float>(); a.plan.sums = b_sums.as<float>(); a.plan.bad = b_bad.as<int32_t>();
    a.thresholds = b_thr.as<float>();
    a.override_thresholds = override_thresholds ? b_over.as<float>() : nullptr;
    a.spans = b_spans.as<tp::Span>(); a.span_frames = b_frames.as<int64_t>();
    a.n_spans = static_cast<int32_t>(n_spans);
    tp::launch_gate(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> bad(B);
    std::vector<float> thr(B);
    std::vector<int64_t> frames(S);
    FA_HIP_TRY(ctx, hipMemcpyAsync(bad.data(), b_bad.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(thr.data(), b_thr.p, sizeof(float) * B, hipMemcpyDeviceToHost, st));
    if (S) FA_HIP_TRY(ctx, hipMemcpyAsync(frames.data(), b_frames.p, sizeof(int64_t) * S, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    for (size_t b = 0; b < B; ++b) {
        if (thresholds) thresholds[b] = thr[b];
        if (statuses) statuses[b] = bad[b] ? FA_INVALID_ARGUMENT : FA_SUCCESS;
    }
    const double frame_seconds = static_cast<double>(c.frame_samples) / static_cast<double>(c.sample_rate);   // ASRConstants.secondsPerEncoderFrame
    for (size_t i = 0; i < S; ++i) {
        if (span_frames) span_frames[i] = frames[i];
        if (span_seconds) span_seconds[i] = static_cast<double>(frames[i]) * frame_seconds;
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_tdt_window_default_config(fa_tdt_window_config *cfg) {
    if (cfg) *cfg = tp::config_or_default(nullptr);
}

fa_status fa_tdt_window_layout(const fa_tdt_window_config *cfg, int64_t *chunk_samples, int64_t *stride_samples, int64_t *mel_context_samples, int64_t *warmup_prefix_samples) {
    tp::Geometry g{};
    const fa::Verdict v = tp::derive(tp::config_or_default(cfg), &g);
    if (v.status != FA_SUCCESS) return v.status;
    if (chunk_samples) *chunk_samples = g.chunk;
    if (stride_samples) *stride_samples = g.stride;
    if (mel_context_samples) *mel_context_samples = g.mel_context;
    if (warmup_prefix_samples) *warmup_prefix_samples = g.warmup_prefix;
    return FA_SUCCESS;
}

int64_t fa_tdt_window_count_bound(const fa_tdt_window_config *cfg, int64_t samples) {
    tp::Geometry g{};
    if (tp::derive(tp::config_or_default(cfg), &g).status != FA_SUCCESS) return -1;
    return tp::window_count_bound(g, samples);
}

fa_status fa_tdt_plan_windows_dev(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *d_audio, const int64_t *audio_offsets, int32_t batch, fa_tdt_window *windows,
                                  int64_t capacity, int64_t *window_range, int32_t *d_audio_frames, int32_t *d_t0, int32_t *d_is_last, int32_t *d_global_offset,
                                  int32_t *d_emit_after, int64_t *speech_end, int32_t *statuses) {
    return plan(ctx, cfg, d_audio, audio_offsets, batch, windows, capacity, window_range, Five{d_audio_frames, d_t0, d_is_last, d_global_offset, d_emit_after}, speech_end,
                statuses, true);
}

fa_status fa_tdt_plan_windows(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets, int32_t batch, fa_tdt_window *windows,
                              int64_t capacity, int64_t *window_range, int32_t *audio_frames, int32_t *t0, int32_t *is_last, int32_t *global_offset, int32_t *emit_after,
                              int64_t *speech_end, int32_t *statuses) {
    return plan(ctx, cfg, audio, audio_offsets, batch, windows, capacity, window_range, Five{audio_frames, t0, is_last, global_offset, emit_after}, speech_end, statuses, false);
}

fa_status fa_tdt_pack_windows_dev(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *d_audio, const int64_t *audio_offsets, int32_t batch, const fa_tdt_window *windows,
                                  int64_t n_windows, float *d_rows, int64_t row_capacity, int32_t *d_lengths) {
    return pack(ctx, cfg, d_audio, audio_offsets, batch, windows, n_windows, d_rows, row_capacity, d_lengths, true);
}

fa_status fa_tdt_pack_windows(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets, int32_t batch, const fa_tdt_window *windows,
                              int64_t n_windows, float *rows, int64_t row_capacity, int32_t *lengths) {
    return pack(ctx, cfg, audio, audio_offsets, batch, windows, n_windows, rows, row_capacity, lengths, false);
}

fa_status fa_tdt_speech_gate_dev(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *d_audio, const int64_t *audio_offsets, int32_t batch, const float *override_thresholds,
                                 float *thresholds, const fa_tdt_span *spans, int64_t n_spans, int64_t *span_frames, double *span_seconds, int32_t *statuses) {
    return gate(ctx, cfg, d_audio, audio_offsets, batch, override_thresholds, thresholds, spans, n_spans, span_frames, span_seconds, statuses, true);
}

fa_status fa_tdt_speech_gate(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets, int32_t batch, const float *override_thresholds,
                             float *thresholds, const fa_tdt_span *spans, int64_t n_spans, int64_t *span_frames, double *span_seconds, int32_t *statuses) {
    return gate(ctx, cfg, audio, audio_offsets, batch, override_thresholds, thresholds, spans, n_spans, span_frames, span_seconds, statuses, false);
}

}  // extern "C"
