// online_host.hip — the host unit of the online diarizer's entries around the networks (kernels and launchers: online.hip, through
// online_launch.h): fa_online_chunk_plan(_dev), fa_online_pack_waveforms_dev and fa_online_chunk_finish_dev — the argument checks, the
// scratch, the launch, and the one count each host-facing entry waits for.  The speaker database fa_online_chunk_finish_dev assigns
// into is speaker_db_host.hip's; only its handle and check_db (online_launch.h) are shared.
#include "online_launch.h"

using fa::online::aligned16;
using fa::online::check_db;

extern "C" {

void fa_online_chunk_default_config(fa_online_chunk_config *c) {
    if (!c) return;   // DiarizerTypes.swift:12, 24; SegmentationProcessor.swift:224-239; SpeakerOperations.swift:106
    c->frames = 589; c->chunk_samples = 160000; c->min_active_frames = 10.0f; c->min_speech_duration = 1.0f; c->validate_min_magnitude = 0.1f;
    c->reserved = 0; c->frame_step = 0.016875;
}

static fa_status chunk_plan(fa_ctx *ctx, const fa_online_chunk_config *cfg, const float *d_weights, const int32_t *d_samples, int32_t streams, int32_t chunks,
                            float *d_activities, fa_online_run *d_runs, int32_t run_capacity, int32_t *run_count, bool count_on_host, float *d_mask_rows) {
    if (!ctx || !cfg) return FA_INVALID_ARGUMENT;
    if (!d_weights || !d_activities || !d_runs || !run_count || !d_mask_rows || streams <= 0 || chunks <= 0 || run_capacity <= 0 || cfg->frames < 1 ||
        cfg->chunk_samples < 1 || static_cast<int64_t>(streams) * chunks * 3 > INT32_MAX)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "online chunk plan: pointers, streams, chunks, run_capacity >= 1, frames >= 1, chunk_samples >= 1");
    return fa::no_throw(ctx, "fa_online_chunk_plan", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t triples = static_cast<size_t>(streams) * chunks * 3;
        fa::DevBuf flags, d_count;
        FA_TRY(fa::take(ctx, "fa_online_chunk_plan", {{&flags, (triples + 1) * sizeof(int32_t)}, {&d_count, sizeof(int32_t), count_on_host}}));
        fa::online::PlanArgs a{d_weights, d_samples, streams, chunks, cfg->frames, cfg->chunk_samples, cfg->min_active_frames, d_activities, flags.as<int32_t>(),
                               d_runs, run_capacity, count_on_host ? d_count.as<int32_t>() : run_count, d_mask_rows};
        fa::online::launch_plan(ctx->stream, a);
        FA_HIP_TRY(ctx, hipGetLastError());
        if (count_on_host) {
            FA_HIP_TRY(ctx, hipMemcpyAsync(run_count, d_count.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return FA_SUCCESS;
    });
}

fa_status fa_online_chunk_plan_dev(fa_ctx *ctx, const fa_online_chunk_config *cfg, const float *d_weights, const int32_t *d_samples_in_chunk, int32_t streams,
                                   int32_t chunks, float *d_activities, fa_online_run *d_runs, int32_t run_capacity, int32_t *d_run_count, float *d_mask_rows) {
    return chunk_plan(ctx, cfg, d_weights, d_samples_in_chunk, streams, chunks, d_activities, d_runs, run_capacity, d_run_count, false, d_mask_rows);
}
fa_status fa_online_chunk_plan(fa_ctx *ctx, const fa_online_chunk_config *cfg, const float *d_weights, const int32_t *d_samples_in_chunk, int32_t streams,
                               int32_t chunks, float *d_activities, fa_online_run *d_runs, int32_t run_capacity, int32_t *run_count, float *d_mask_rows) {
    return chunk_plan(ctx, cfg, d_weights, d_samples_in_chunk, streams, chunks, d_activities, d_runs, run_capacity, run_count, true, d_mask_rows);
}

fa_status fa_online_pack_waveforms_dev(fa_ctx *ctx, const float *d_audio, const int64_t *d_offsets, const int32_t *d_lengths, int32_t rows, int32_t chunk_samples,
                                       int32_t mode, float *d_out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!d_audio || !d_offsets || !d_lengths || !d_out || rows <= 0 || rows > 65535 || chunk_samples < 1 || !aligned16(d_out) ||
        (mode != FA_ONLINE_PACK_ZERO_TAIL && mode != FA_ONLINE_PACK_REPEAT))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "online pack: pointers (rows 16-byte aligned), 1 <= rows <= 65535, chunk_samples >= 1, a mode");
    fa::DeviceGuard guard(ctx->device);
    fa::online::launch_pack(ctx->stream, fa::online::PackArgs{d_audio, d_offsets, d_lengths, rows, chunk_samples, mode == FA_ONLINE_PACK_REPEAT ? 1 : 0, d_out});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_online_chunk_finish_dev(fa_ctx *ctx, const fa_online_chunk_config *cfg, fa_speaker_db *db, const float *d_weights, const float *d_activities,
                                     const float *d_embeddings, const double *chunk_offsets, int32_t chunks, int64_t tick, fa_online_segment *segments,
                                     int64_t capacity, int64_t *count, int32_t *chunk_counts, fa_speaker_assignment *d_assignments) {
    if (!cfg) return FA_INVALID_ARGUMENT;
    FA_TRY(check_db(ctx, db, "fa_online_chunk_finish_dev"));
    if (!d_weights || !d_activities || !d_embeddings || !chunk_offsets || !count || !d_assignments || chunks <= 0 || capacity < 0 || (capacity > 0 && !segments) ||
        cfg->frames < 1 || !aligned16(d_embeddings) || static_cast<int64_t>(db->streams) * chunks > INT32_MAX / 4)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "online chunk finish: pointers (embeddings 16-byte aligned), chunks >= 1, capacity >= 0, frames >= 1");
    return fa::no_throw(ctx, "fa_online_chunk_finish_dev", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t sc = static_cast<size_t>(db->streams) * chunks;
        fa::DevBuf d_off, d_counts, d_seg;
        FA_TRY(fa::take(ctx, "fa_online_chunk_finish_dev", {{&d_off, sc * sizeof(double), true, chunk_offsets}, {&d_counts, (sc + 1) * sizeof(int32_t)},
                                                             {&d_seg, static_cast<size_t>(capacity) * sizeof(fa_online_segment)}}));
        fa::spk::Params p = db->p;
        p.validate_min_magnitude = cfg->validate_min_magnitude;
        fa::online::FinishArgs a{db->arrays(), p, d_weights, d_activities, d_embeddings, d_off.as<double>(), chunks, cfg->frames, cfg->min_active_frames,
                                 cfg->min_speech_duration, cfg->frame_step, tick, reinterpret_cast<fa::spk::Record *>(d_assignments), d_counts.as<int32_t>(),
                                 d_seg.as<fa_online_segment>(), capacity};
        fa::online::launch_finish(ctx->stream, a);
        FA_HIP_TRY(ctx, hipGetLastError());
        std::vector<int32_t> prefix(sc + 1);
        FA_HIP_TRY(ctx, hipMemcpyAsync(prefix.data(), d_counts.p, (sc + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                 // the one synchronisation: the records' count decides the copy
        *count = prefix[sc];
        for (size_t i = 0; chunk_counts && i < sc; ++i) chunk_counts[i] = prefix[i + 1] - prefix[i];
        if (*count > capacity) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "online chunk finish: %lld segments, room for %lld", static_cast<long long>(*count), static_cast<long long>(capacity));
        if (*count > 0) FA_HIP_TRY(ctx, hipMemcpy(segments, d_seg.p, static_cast<size_t>(*count) * sizeof(fa_online_segment), hipMemcpyDeviceToHost));
        return FA_SUCCESS;
    });
}

}  // extern "C"
