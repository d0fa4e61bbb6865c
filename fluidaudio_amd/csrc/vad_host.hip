// vad_host.hip — the host side of the VAD stages (kernels: vad.hip, shared operands and the argument pass: vad_launch.h): the uploads
// of the host-pointer entries, the workspace, the synchronisation of a call and the C ABI.  No arithmetic of the reference lives here:
// what is decided here is decided from the arguments alone, before any device work.
#include <algorithm>
#include <cmath>

#include "fa_common.h"
#include "vad_launch.h"

namespace {

namespace vd = fa::vad;

fa_status segments(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *probs, const int64_t *frame_range, const int64_t *total_samples, const int32_t batch,
                   fa_vad_segment *segs, const int64_t capacity, int64_t *count, int64_t *recording_counts, const bool device) {
    return fa::no_throw(ctx, "vad_segments", [&]() -> fa_status {
    vd::Operands o{};
    vd::SegPlan plan;
    const fa::Verdict v = vd::plan_segments(vd::config_or_default(cfg), probs, frame_range, total_samples, batch, segs, capacity, count, device, &o, &plan);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    *count = 0;
    if (recording_counts) std::fill(recording_counts, recording_counts + batch, int64_t{0});
    if (batch == 0) return FA_SUCCESS;
    const size_t B = static_cast<size_t>(batch), out_slots = static_cast<size_t>(plan.out_slots);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_rec, b_probs, b_raw, b_rawc, b_kept, b_keptc, b_total, b_out;
    FA_TRY(fa::take(ctx, "vad_segments",
                    {{&b_rec, sizeof(vd::SegRecording) * B, true, plan.rec.data()}, {&b_probs, device ? 0 : sizeof(float) * static_cast<size_t>(plan.frames), !device, (device || plan.frames == 0) ? nullptr : probs + frame_range[0]},
                     {&b_raw, sizeof(vd::RawSpeech) * static_cast<size_t>(plan.raw_slots)}, {&b_rawc, sizeof(int32_t) * B}, {&b_kept, sizeof(int32_t) * B},
                     {&b_keptc, sizeof(int32_t) * B}, {&b_total, sizeof(int32_t)}, {&b_out, sizeof(fa_vad_segment) * out_slots}}));
    vd::SegArgs a{};
    a.probs = device ? probs : b_probs.as<float>();
    a.rec = b_rec.as<vd::SegRecording>();
    a.batch = batch;
    a.o = o;
    a.raw = b_raw.as<vd::RawSpeech>(); a.raw_counts = b_rawc.as<int32_t>();
    a.kept = b_kept.as<int32_t>(); a.kept_counts = b_keptc.as<int32_t>(); a.total = b_total.as<int32_t>();
    a.out = b_out.as<fa_vad_segment>(); a.out_slots = plan.out_slots;
    vd::launch_segments(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> raw_counts(B), kept(B);
    std::vector<fa_vad_segment> got(out_slots);
    FA_HIP_TRY(ctx, hipMemcpyAsync(raw_counts.data(), b_rawc.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(kept.data(), b_keptc.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    if (out_slots) FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_out.p, sizeof(fa_vad_segment) * out_slots, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    int64_t total = 0;
    for (size_t b = 0; b < B; ++b) {
        if (raw_counts[b] < 0 || raw_counts[b] > plan.rec[b].frames || kept[b] < 0 || kept[b] > raw_counts[b])
            return fa::set_error(ctx, FA_RUNTIME_ERROR, "vad_segments: recording %zu of %d frames reports %d raw speeches, %d segments", b, plan.rec[b].frames, raw_counts[b], kept[b]);
        if (recording_counts) recording_counts[b] = kept[b];
        total += kept[b];
    }
    *count = total;
    if (segs) std::copy(got.begin(), got.begin() + std::min<int64_t>(total, plan.out_slots), segs);
    if (segs && capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "vad_segments: output holds %lld of %lld segments", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

fa_status pack(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, const int32_t batch, float *rows, const int64_t row_capacity, int64_t *chunk_range, const bool device) {
    return fa::no_throw(ctx, "vad_pack_chunks", [&]() -> fa_status {
    const fa::Verdict v = vd::plan_pack(audio, audio_offsets, batch, rows, row_capacity, chunk_range);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0 || chunk_range[batch] == 0) return FA_SUCCESS;
    const int64_t a0 = device ? 0 : audio_offsets[0];
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_offsets[batch] - a0);
    const size_t row_bytes = sizeof(float) * vd::kRow * static_cast<size_t>(chunk_range[batch]);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_audio, b_rows;
    FA_TRY(fa::take(ctx, "vad_pack_chunks", {{&b_audio, audio_bytes, !device, device ? nullptr : audio + a0}, {&b_rows, device ? 0 : row_bytes, !device}}));
    const float *d_audio = device ? audio : b_audio.as<float>();
    float *d_rows = device ? rows : b_rows.as<float>();
    const bool wide = reinterpret_cast<uintptr_t>(d_rows) % 16 == 0;   // a row is 16 640 bytes: every row is aligned when the first one is
    // the offsets of up to kPackGroup recordings travel in a launch's arguments: nothing is staged, so the device entry need not wait
    for (int32_t g0 = 0; g0 < batch; g0 += vd::kPackGroup) {
        vd::PackGroup g{};
        g.count = std::min<int32_t>(vd::kPackGroup, batch - g0);
        for (int32_t i = 0; i <= g.count; ++i) {
            g.audio_off[i] = audio_offsets[g0 + i] - a0;
            g.row_off[i] = chunk_range[g0 + i] - chunk_range[g0];
        }
        vd::launch_pack(st, d_audio, g, d_rows + chunk_range[g0] * vd::kRow, wide);
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(rows, b_rows.p, row_bytes, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the host entry's one synchronisation: its buffers are its own
    }
    return FA_SUCCESS;
    });
}

fa_status gather(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, const int32_t batch, const fa_vad_segment *segs, const int64_t n_segments, float *out,
                 const int64_t out_capacity, int64_t *out_range, const bool device) {
    return fa::no_throw(ctx, "vad_gather_segments", [&]() -> fa_status {
    vd::GatherPlan plan;
    const fa::Verdict v = vd::plan_gather(audio, audio_offsets, batch, segs, n_segments, out, out_capacity, out_range, device, &plan);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0 || n_segments == 0 || out_range[n_segments] == 0) return FA_SUCCESS;
    const size_t n = static_cast<size_t>(n_segments);
    const int64_t a0 = device ? 0 : audio_offsets[0];
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_offsets[batch] - a0);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(out_range[n_segments]);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_src, b_range, b_tiles, b_audio, b_out;
    FA_TRY(fa::take(ctx, "vad_gather_segments",
                    {{&b_src, sizeof(int64_t) * n, true, plan.src.data()}, {&b_range, sizeof(int64_t) * (n + 1), true, out_range}, {&b_tiles, sizeof(int64_t) * (n + 1), true, plan.tile_off.data()},
                     {&b_audio, audio_bytes, !device, device ? nullptr : audio + a0}, {&b_out, device ? 0 : out_bytes, !device}}));
    vd::GatherArgs a{};
    a.audio = device ? audio : b_audio.as<float>();
    a.out = device ? out : b_out.as<float>();
    a.src = b_src.as<int64_t>(); a.out_range = b_range.as<int64_t>(); a.tile_off = b_tiles.as<int64_t>();
    a.n_segments = n_segments;
    a.tiles = static_cast<int32_t>(plan.tile_off[n]);
    vd::launch_gather(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) FA_HIP_TRY(ctx, hipMemcpyAsync(out, b_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation: the staged tables are released with it
    return FA_SUCCESS;
    });
}

fa_status stream_advance(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *probs, const int32_t *chunk_counts, const int32_t *chunk_samples, const int32_t streams,
                         const int32_t max_chunks, fa_vad_stream_state *states, const int32_t return_seconds, const int32_t time_resolution, fa_vad_stream_event *events,
                         const int64_t capacity, int64_t *count, const bool device) {
    return fa::no_throw(ctx, "vad_stream_advance", [&]() -> fa_status {
    vd::Operands o{};
    const fa::Verdict v = vd::plan_stream(vd::config_or_default(cfg), probs, chunk_counts, streams, max_chunks, states, time_resolution, events, capacity, count, &o);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    *count = 0;
    const size_t cells = static_cast<size_t>(streams) * static_cast<size_t>(max_chunks), S = static_cast<size_t>(streams);
    if (cells == 0 || !std::any_of(chunk_counts, chunk_counts + streams, [](const int32_t c) { return c > 0; })) return FA_SUCCESS;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_counts, b_states, b_events, b_probs, b_samples;
    FA_TRY(fa::take(ctx, "vad_stream_advance",
                    {{&b_counts, sizeof(int32_t) * S, true, chunk_counts}, {&b_states, sizeof(fa_vad_stream_state) * S, true, states}, {&b_events, sizeof(fa_vad_stream_event) * cells},
                     {&b_probs, device ? 0 : sizeof(float) * cells, !device, probs}, {&b_samples, device ? 0 : sizeof(int32_t) * cells, !device && chunk_samples, chunk_samples}}));
    vd::StreamArgs a{};
    a.probs = device ? probs : b_probs.as<float>();
    a.chunk_counts = b_counts.as<int32_t>();
    a.chunk_samples = !chunk_samples ? nullptr : (device ? chunk_samples : b_samples.as<int32_t>());
    a.streams = streams; a.max_chunks = max_chunks;
    a.o = o;
    a.return_seconds = return_seconds ? 1 : 0;
    a.factor = vd::resolution_factor(time_resolution);
    a.states = b_states.as<fa_vad_stream_state>();
    a.events = b_events.as<fa_vad_stream_event>();
    vd::launch_stream(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<fa_vad_stream_event> got(cells);
    std::vector<fa_vad_stream_state> next(S);
    FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_events.p, sizeof(fa_vad_stream_event) * cells, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(next.data(), b_states.p, sizeof(fa_vad_stream_state) * S, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    std::copy(next.begin(), next.end(), states);
    int64_t total = 0;
    for (size_t s = 0; s < S; ++s)
        for (int32_t k = 0; k < chunk_counts[s]; ++k) {
            const fa_vad_stream_event &e = got[s * static_cast<size_t>(max_chunks) + static_cast<size_t>(k)];
            if (e.kind < 0) continue;
            if (events && total < capacity) events[total] = e;
            ++total;
        }
    *count = total;
    if (events && capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "vad_stream_advance: output holds %lld of %lld events", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_vad_default_config(fa_vad_segmentation_config *cfg) {
    if (cfg) *cfg = vd::config_or_default(nullptr);
}

int64_t fa_vad_chunk_count(int64_t samples) { return vd::chunk_count(samples); }

fa_status fa_vad_segments_dev(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *d_probs, const int64_t *frame_range, const int64_t *total_samples, int32_t batch,
                              fa_vad_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts) {
    return segments(ctx, cfg, d_probs, frame_range, total_samples, batch, segs, capacity, count, recording_counts, true);
}

fa_status fa_vad_segments(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *probs, const int64_t *frame_range, const int64_t *total_samples, int32_t batch,
                          fa_vad_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts) {
    return segments(ctx, cfg, probs, frame_range, total_samples, batch, segs, capacity, count, recording_counts, false);
}

fa_status fa_vad_pack_chunks_dev(fa_ctx *ctx, const float *d_audio, const int64_t *audio_offsets, int32_t batch, float *d_rows, int64_t row_capacity, int64_t *chunk_range) {
    return pack(ctx, d_audio, audio_offsets, batch, d_rows, row_capacity, chunk_range, true);
}

fa_status fa_vad_pack_chunks(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, int32_t batch, float *rows, int64_t row_capacity, int64_t *chunk_range) {
    return pack(ctx, audio, audio_offsets, batch, rows, row_capacity, chunk_range, false);
}

fa_status fa_vad_gather_segments_dev(fa_ctx *ctx, const float *d_audio, const int64_t *audio_offsets, int32_t batch, const fa_vad_segment *segs, int64_t n_segments, float *d_out,
                                     int64_t out_capacity, int64_t *out_range) {
    return gather(ctx, d_audio, audio_offsets, batch, segs, n_segments, d_out, out_capacity, out_range, true);
}

fa_status fa_vad_gather_segments(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, int32_t batch, const fa_vad_segment *segs, int64_t n_segments, float *out,
                                 int64_t out_capacity, int64_t *out_range) {
    return gather(ctx, audio, audio_offsets, batch, segs, n_segments, out, out_capacity, out_range, false);
}

fa_status fa_vad_stream_advance_dev(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *d_probs, const int32_t *chunk_counts, const int32_t *d_chunk_samples,
                                    int32_t streams, int32_t max_chunks, fa_vad_stream_state *states, int32_t return_seconds, int32_t time_resolution,
                                    fa_vad_stream_event *events, int64_t capacity, int64_t *count) {
    return stream_advance(ctx, cfg, d_probs, chunk_counts, d_chunk_samples, streams, max_chunks, states, return_seconds, time_resolution, events, capacity, count, true);
}

fa_status fa_vad_stream_advance(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *probs, const int32_t *chunk_counts, const int32_t *chunk_samples, int32_t streams,
                                int32_t max_chunks, fa_vad_stream_state *states, int32_t return_seconds, int32_t time_resolution, fa_vad_stream_event *events,
                                int64_t capacity, int64_t *count) {
    return stream_advance(ctx, cfg, probs, chunk_counts, chunk_samples, streams, max_chunks, states, return_seconds, time_resolution, events, capacity, count, false);
}

}  // extern "C"
