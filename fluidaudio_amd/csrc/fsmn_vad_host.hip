// fsmn_vad_host.hip — the host side of FSMN-VAD (kernels: fsmn_vad.hip; the argument pass, the chunk schedule and the operands:
// fsmn_vad_launch.h): the uploads of the host-pointer entries, the synchronisation of a call and the C ABI.  No arithmetic of the
// reference lives here: what is decided here is decided from the arguments alone, before any device work.
#include <algorithm>

#include "fa_common.h"
#include "fsmn_vad_launch.h"

namespace {

namespace fv = fa::fsmnvad;

fa_status segments(fa_ctx *ctx, const fa_fsmn_vad_config *cfg, const float *probs, const int64_t *frame_range, const int32_t batch, fa_fsmn_vad_segment *segs,
                   const int64_t capacity, int64_t *count, int64_t *recording_counts, const bool device) {
    return fa::no_throw(ctx, "fsmn_vad_segments", [&]() -> fa_status {
    fv::Params o{};
    fv::SegPlan plan;
    const fa::Verdict v = fv::plan_segments(fv::config_or_default(cfg), probs, frame_range, batch, segs, capacity, count, device, &o, &plan);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    *count = 0;
    if (recording_counts) std::fill(recording_counts, recording_counts + batch, int64_t{0});
    if (batch == 0) return FA_SUCCESS;
    const size_t B = static_cast<size_t>(batch), out_slots = static_cast<size_t>(plan.out_slots);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_rec, b_probs, b_arena, b_counts, b_kept, b_total, b_out;
    FA_TRY(fa::take(ctx, "fsmn_vad_segments",
                    {{&b_rec, sizeof(fv::SegRecording) * B, true, plan.rec.data()}, {&b_probs, device ? 0 : sizeof(float) * static_cast<size_t>(plan.frames), !device, (device || plan.frames == 0) ? nullptr : probs + frame_range[0]},
                     {&b_arena, sizeof(fv::RawSegment) * static_cast<size_t>(plan.arena)}, {&b_counts, sizeof(int32_t) * B}, {&b_kept, sizeof(int32_t) * B}, {&b_total, sizeof(int32_t)},
                     {&b_out, sizeof(fa_fsmn_vad_segment) * out_slots}}));
    fv::SegArgs a{};
    a.probs = device ? probs : b_probs.as<float>();
    a.rec = b_rec.as<fv::SegRecording>();
    a.batch = batch;
    a.o = o;
    a.arena = b_arena.as<fv::RawSegment>();
    a.counts = b_counts.as<int32_t>(); a.kept = b_kept.as<int32_t>(); a.total = b_total.as<int32_t>();
    a.out = b_out.as<fa_fsmn_vad_segment>(); a.out_slots = plan.out_slots;
    fv::launch_segments(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> counts(B);
    std::vector<fa_fsmn_vad_segment> got(out_slots);
    FA_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), b_counts.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    if (out_slots) FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_out.p, sizeof(fa_fsmn_vad_segment) * out_slots, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    int64_t total = 0;
    for (size_t b = 0; b < B; ++b) {
        if (counts[b] < 0 || counts[b] > plan.rec[b].frames)
            return fa::set_error(ctx, FA_RUNTIME_ERROR, "fsmn_vad_segments: recording %zu of %d frames reports %d segments", b, plan.rec[b].frames, counts[b]);
        if (recording_counts) recording_counts[b] = counts[b];
        total += counts[b];
    }
    *count = total;
    if (segs) std::copy(got.begin(), got.begin() + std::min<int64_t>(total, plan.out_slots), segs);
    if (segs && capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "fsmn_vad_segments: output holds %lld of %lld segments", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

fa_status pack(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, const int32_t batch, const fa_fsmn_vad_chunk *chunks, const int64_t n, float *rows,
               const int64_t row_stride, const int64_t row_capacity, const bool device) {
    return fa::no_throw(ctx, "fsmn_vad_pack_waveforms", [&]() -> fa_status {
    const fa::Verdict v = fv::plan_pack(audio, audio_offsets, batch, chunks, n, rows, row_stride, row_capacity);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n == 0 || row_stride == 0) return FA_SUCCESS;
    const int64_t a0 = device ? 0 : audio_offsets[0];
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_offsets[batch] - a0);
    const size_t row_bytes = sizeof(float) * static_cast<size_t>(row_stride) * static_cast<size_t>(n);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_audio, b_rows;
    FA_TRY(fa::take(ctx, "fsmn_vad_pack_waveforms", {{&b_audio, audio_bytes, !device, device ? nullptr : audio + a0}, {&b_rows, device ? 0 : row_bytes, !device}}));
    const float *d_audio = device ? audio : b_audio.as<float>();
    float *d_rows = device ? rows : b_rows.as<float>();
    const bool wide = reinterpret_cast<uintptr_t>(d_rows) % 16 == 0 && row_stride % 4 == 0;   // then every row is aligned
    const auto fill = [&](fa::rows::Group &g, const int64_t i, const int32_t k) {
        g.src[k] = audio_offsets[chunks[i].recording] - a0 + chunks[i].start_sample;
        g.len[k] = static_cast<int32_t>(chunks[i].end_sample - chunks[i].start_sample);
    };
    fa::rows::for_each_group(n, fill, [&](const fa::rows::Group &g, const int64_t g0) { fv::launch_pack(st, d_audio, g, d_rows + g0 * row_stride, row_stride, wide); });
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(rows, b_rows.p, row_bytes, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the host entry's one synchronisation: its buffers are its own
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_fsmn_vad_default_config(fa_fsmn_vad_config *cfg) {
    if (cfg) *cfg = fv::config_or_default(nullptr);
}

int64_t fa_fsmn_vad_frame_count(int64_t samples) { return fv::frame_count(samples); }

fa_status fa_fsmn_vad_plan_chunks(const int64_t *total_samples, int32_t batch, fa_fsmn_vad_chunk *chunks, int64_t capacity, int64_t *count, int64_t *chunk_range,
                                  int64_t *frame_range) {
    return fa::no_throw(nullptr, "fsmn_vad_plan_chunks", [&]() -> fa_status { return fv::plan_chunks(total_samples, batch, chunks, capacity, count, chunk_range, frame_range).status; });
}

fa_status fa_fsmn_vad_pack_waveforms_dev(fa_ctx *ctx, const float *d_audio, const int64_t *audio_offsets, int32_t batch, const fa_fsmn_vad_chunk *chunks, int64_t n_chunks,
                                         float *d_rows, int64_t row_stride, int64_t row_capacity) {
    return pack(ctx, d_audio, audio_offsets, batch, chunks, n_chunks, d_rows, row_stride, row_capacity, true);
}

fa_status fa_fsmn_vad_pack_waveforms(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, int32_t batch, const fa_fsmn_vad_chunk *chunks, int64_t n_chunks, float *rows,
                                     int64_t row_stride, int64_t row_capacity) {
    return pack(ctx, audio, audio_offsets, batch, chunks, n_chunks, rows, row_stride, row_capacity, false);
}

fa_status fa_fsmn_vad_pack_feats_dev(fa_ctx *ctx, const void *d_feats, int32_t dtype, int64_t feat_stride, const fa_fsmn_vad_chunk *chunks, int64_t n_chunks, int32_t bucket,
                                     float *d_out) {
    return fa::no_throw(ctx, "fsmn_vad_pack_feats_dev", [&]() -> fa_status {
    const fa::Verdict v = fv::plan_feats(d_feats, dtype, feat_stride, chunks, n_chunks, bucket, d_out);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_chunks == 0 || bucket == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    const size_t element = dtype == FA_DTYPE_F16 ? 2 : 4;
    const bool wide = reinterpret_cast<uintptr_t>(d_out) % 16 == 0 && reinterpret_cast<uintptr_t>(d_feats) % (4 * element) == 0;   // a feature row is whole groups of four
    const auto fill = [&](fv::FeatGroup &g, const int64_t i, const int32_t k) { g.frames[k] = chunks[i].frames; };
    fa::rows::for_each_group<fv::FeatGroup>(n_chunks, fill, [&](const fv::FeatGroup &g, const int64_t g0) {
        fv::launch_feats(ctx->stream, static_cast<const char *>(d_feats) + static_cast<size_t>(g0) * static_cast<size_t>(feat_stride) * fv::kFeatureDim * element, dtype, feat_stride, g,
                         bucket, d_out + static_cast<size_t>(g0) * static_cast<size_t>(bucket) * fv::kFeatureDim, wide);
    });
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
    });
}

fa_status fa_fsmn_vad_gather_silence_dev(fa_ctx *ctx, const void *d_scores, int32_t dtype, int32_t bucket, int32_t vocab, const fa_fsmn_vad_chunk *chunks, int64_t n_chunks,
                                         const int64_t *frame_range, int32_t batch, float *d_silence, int64_t silence_capacity) {
    return fa::no_throw(ctx, "fsmn_vad_gather_silence_dev", [&]() -> fa_status {
    const fa::Verdict v = fv::plan_gather(d_scores, dtype, bucket, vocab, chunks, n_chunks, frame_range, batch, d_silence, silence_capacity);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_chunks == 0 || bucket == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    const size_t element = dtype == FA_DTYPE_F16 ? 2 : 4;
    const auto fill = [&](fv::GatherGroup &g, const int64_t i, const int32_t k) {
        g.dst[k] = frame_range[chunks[i].recording] + chunks[i].first_frame;
        g.keep_from[k] = chunks[i].keep_from;
        g.frames[k] = chunks[i].frames;
    };
    fa::rows::for_each_group<fv::GatherGroup>(n_chunks, fill, [&](const fv::GatherGroup &g, const int64_t g0) {
        fv::launch_gather(ctx->stream, static_cast<const char *>(d_scores) + static_cast<size_t>(g0) * static_cast<size_t>(bucket) * static_cast<size_t>(vocab) * element, dtype, bucket,
                          vocab, g, d_silence);
    });
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
    });
}

fa_status fa_fsmn_vad_segments_dev(fa_ctx *ctx, const fa_fsmn_vad_config *cfg, const float *d_probs, const int64_t *frame_range, int32_t batch, fa_fsmn_vad_segment *segs,
                                   int64_t capacity, int64_t *count, int64_t *recording_counts) {
    return segments(ctx, cfg, d_probs, frame_range, batch, segs, capacity, count, recording_counts, true);
}

fa_status fa_fsmn_vad_segments(fa_ctx *ctx, const fa_fsmn_vad_config *cfg, const float *probs, const int64_t *frame_range, int32_t batch, fa_fsmn_vad_segment *segs,
                               int64_t capacity, int64_t *count, int64_t *recording_counts) {
    return segments(ctx, cfg, probs, frame_range, batch, segs, capacity, count, recording_counts, false);
}

}  // extern "C"
