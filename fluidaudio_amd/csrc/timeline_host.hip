// timeline_host.hip — the host side of the timeline (kernels: timeline.hip, operands and plan: timeline_launch.h): the staging of the
// host-pointer entry, the launches, the three synchronisations of a call — the raw run count, the segment counts, the fill — and the
// C ABI.
#include <cstring>

#include "fa_common.h"
#include "timeline_launch.h"

namespace {

using namespace fa::timeline;

fa_status timeline_segments(fa_ctx *ctx, const fa_timeline_config *cfg, const float *finalized, const int64_t *fin_frames, const float *tentative,
                            const int64_t *tent_frames, int32_t B, int32_t is_complete, fa_diarizer_segment *segs, int64_t capacity, int64_t *count,
                            int64_t *rec_counts, bool device) {
    if (!ctx || !cfg || !count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "timeline: ctx, config and count are required");
    *count = 0;
    const fa::Verdict cv = check_config(*cfg, B, capacity, fin_frames);
    if (cv.status != FA_SUCCESS) return fa::set_error(ctx, cv.status, "%s", cv.text);
    if (rec_counts) for (int32_t b = 0; b < B; ++b) rec_counts[b] = 0;
    if (B == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "timeline", [&]() -> fa_status {
    const int32_t S = cfg->speakers;
    Plan plan;
    const fa::Verdict pv = make_plan(S, fin_frames, tent_frames, B, finalized, tentative, plan);
    if (pv.status != FA_SUCCESS) return fa::set_error(ctx, pv.status, "%s", pv.text);
    const int64_t fsum = plan.fsum, tsum = plan.tsum, Q = plan.Q, blocks = plan.blocks;
    const int32_t max_tiles = plan.max_tiles;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_fin, b_tent, b_rec, b_tile, b_bsum, b_starts, b_runs, b_count, b_off, b_total, b_out;
    FA_TRY(fa::take(ctx, "timeline", {{&b_rec, sizeof(TlRec) * B, true, plan.rec.data()}, {&b_tile, static_cast<size_t>(blocks)}, {&b_bsum, sizeof(int32_t) * (blocks + 1)},
                                      {&b_count, sizeof(int32_t) * Q}, {&b_off, sizeof(int32_t) * Q}, {&b_total, sizeof(int32_t)},
                                      {&b_fin, sizeof(float) * fsum * S, !device && fsum > 0, finalized}, {&b_tent, sizeof(float) * tsum * S, !device && tsum > 0, tentative}}));
    const float *d_fin = device ? finalized : b_fin.as<float>(), *d_tent = device ? tentative : b_tent.as<float>();
    TlArgs ta{d_fin, d_tent, b_rec.as<TlRec>(), b_tile.as<uint8_t>(), b_bsum.as<int32_t>(), S, max_tiles, cfg->onset_threshold, cfg->offset_threshold};
    launch_tiles(st, ta, blocks, 0, nullptr);
    launch_tile_state(st, ta, Q);
    launch_tiles(st, ta, blocks, 1, nullptr);
    launch_scan_totals(st, b_bsum.as<int32_t>(), blocks, b_bsum.as<int32_t>() + blocks);
    FA_HIP_TRY(ctx, hipGetLastError());
    int32_t n_runs = 0;
    FA_HIP_TRY(ctx, hipMemcpyAsync(&n_runs, b_bsum.as<int32_t>() + blocks, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the raw run count sizes the run buffers
    FA_TRY(fa::take(ctx, "timeline", {{&b_starts, sizeof(int32_t) * std::max(n_runs, 1)}, {&b_runs, sizeof(TlRun) * std::max(n_runs, 1)}}));
    if (n_runs > 0) {
        launch_tiles(st, ta, blocks, 2, b_starts.as<int32_t>());
        launch_run_walk(st, ta, b_starts.as<int32_t>(), Q, n_runs, b_runs.as<TlRun>());
    }
    WalkArgs wa{b_rec.as<TlRec>(), b_bsum.as<int32_t>(), b_runs.as<TlRun>(), b_count.as<int32_t>(), b_off.as<int32_t>(), nullptr, 0, Q, S, max_tiles,
                cfg->onset_pad_frames, cfg->offset_pad_frames, cfg->min_frames_on, cfg->min_frames_off, is_complete ? 1 : 0};
    launch_segment_walk(st, wa, 0);
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_off.p, b_count.p, sizeof(int32_t) * Q, hipMemcpyDeviceToDevice, st));
    launch_scan_totals(st, b_off.as<int32_t>(), Q, b_total.as<int32_t>());
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> counts(static_cast<size_t>(Q));
    FA_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), b_count.p, sizeof(int32_t) * Q, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the segment counts
    int64_t total = 0;
    for (int64_t q = 0; q < Q; ++q) {
        total += counts[q];
        if (rec_counts) rec_counts[q / S] += counts[q];
    }
    *count = total;
    if (!segs || total == 0) return FA_SUCCESS;
    const int64_t n_out = std::min(total, capacity);
    if (n_out > 0) {
        FA_TRY(fa::take(ctx, "timeline", {{&b_out, sizeof(fa_diarizer_segment) * n_out}}));
        wa.out = b_out.as<fa_diarizer_segment>();
        wa.capacity = n_out;
        launch_segment_walk(st, wa, 1);
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipMemcpyAsync(segs, b_out.p, sizeof(fa_diarizer_segment) * n_out, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the fill
    }
    if (capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "timeline: output holds %lld of %lld segments", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_timeline_default_config(fa_timeline_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->onset_threshold = 0.5f;        // DiarizerTimelineConfig.sortformerDefault (DiarizerTimeline.swift:72-87)
    cfg->offset_threshold = 0.5f;
    cfg->frame_duration = 0.08f;
    cfg->speakers = 4;
    cfg->activity_type = FA_ACTIVITY_SIGMOIDS;
}

fa_status fa_timeline_segments_dev(fa_ctx *ctx, const fa_timeline_config *cfg, const float *d_finalized, const int64_t *finalized_frames,
                                   const float *d_tentative, const int64_t *tentative_frames, int32_t batch, int32_t is_complete,
                                   fa_diarizer_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts) {
    return timeline_segments(ctx, cfg, d_finalized, finalized_frames, d_tentative, tentative_frames, batch, is_complete, segs, capacity, count,
                             recording_counts, true);
}

fa_status fa_timeline_segments(fa_ctx *ctx, const fa_timeline_config *cfg, const float *finalized, const int64_t *finalized_frames, const float *tentative,
                               const int64_t *tentative_frames, int32_t batch, int32_t is_complete, fa_diarizer_segment *segs, int64_t capacity,
                               int64_t *count, int64_t *recording_counts) {
    return timeline_segments(ctx, cfg, finalized, finalized_frames, tentative, tentative_frames, batch, is_complete, segs, capacity, count,
                             recording_counts, false);
}

}  // extern "C"
