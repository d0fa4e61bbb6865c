// embedding_host.hip — the host side of the embedding model's inputs (kernels and launchers: embedding.hip, through embedding_launch.h):
// the argument checks and the plan (embedding_geom.h: the config's Geometry, the planned windows, the span geometry), the staging of the
// device buffers, the TimedEmbedding records (OfflineEmbeddingPending, OfflineEmbeddingExtractor.swift:586-611) and the C ABI.  Built
// with -ffp-contract=off: the record times offset + Double(frame) * fd are fp64 without FMA.  The host-pointer and the _dev entries share
// one body each; `device` says which of the caller's pointers are device memory.
#include <algorithm>
#include <cstring>
#include <vector>

#include "embedding_launch.h"

namespace {

using namespace fa::embedding;

// ---------------------------------------------------------------- fa_embedding_plan

struct PlanCall {   // the arguments of fa_embedding_plan / fa_embedding_plan_dev
    const fa_embedding_config *cfg;
    const float *weights;
    int64_t C;
    int32_t F, S;
    const double *offsets;
    int64_t n_offsets, total_samples;
    fa_export_embedding *records;
    int32_t *run_of_job, *window_of_run;
    int64_t *window_start;
    int32_t *window_chunk;
    float *run_weights, *mask_rows;
    fa_embedding_info *info;
    bool device;
};

struct Plan {
    Geometry g;
    Windows win;
    int64_t nw = 0, items = 0;   // planned windows, (window, speaker) items; items == 0: nothing for the device
};

// Arguments -> Geometry + planned windows, with every argument and limit check of the entry; fills the info fields and the window outputs
// that are known without the device.
fa_status make_plan(fa_ctx *ctx, const PlanCall &c, Plan &p) {
    if (c.info) memset(c.info, 0, sizeof(*c.info));
    if (!config_ok(c.cfg)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: bad config");
    const bool any = c.C > 0 && c.F > 0 && c.S > 0;
    if (c.C < 0 || c.F < 0 || c.S < 0 || c.n_offsets < 0 || c.total_samples < 0 || (any && !c.weights) || (c.n_offsets > 0 && !c.offsets))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: bad arguments");
    if (any && (!c.records || !c.run_of_job || !c.window_of_run || !c.run_weights))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: records, run_of_job, window_of_run and run_weights are required");
    if (c.C * static_cast<int64_t>(c.S) > INT32_MAX / 2 || static_cast<int64_t>(c.F) * c.S > INT32_MAX / 2)
        return fa::set_error(ctx, FA_INDEX_OVERFLOW, "embedding plan: more than 2^30 masks");
    p.g = geometry(*c.cfg, c.F);
    if (c.info) {
        c.info->frame_duration = p.g.fd;
        c.info->min_frames = p.g.min_frames;
        c.info->samples_per_window = p.g.spw;
        c.info->batch_size = p.g.B;
    }
    if (c.C == 0 || c.F == 0) return FA_SUCCESS;   // extractEmbeddings skips chunks without frames (:182-186)
    p.win = plan_windows(*c.cfg, p.g, c.C, c.offsets, c.n_offsets, c.total_samples);
    p.nw = static_cast<int64_t>(p.win.chunk.size());
    p.items = p.nw * c.S;
    if (c.info) {
        c.info->planned_chunks = p.nw;
        c.info->batches = (p.nw + p.g.B - 1) / p.g.B;
        c.info->evaluated_masks = p.items;
    }
    if (c.window_start) std::copy(p.win.start.begin(), p.win.start.end(), c.window_start);
    if (c.window_chunk) std::copy(p.win.chunk.begin(), p.win.chunk.end(), c.window_chunk);
    return FA_SUCCESS;
}

struct PlanBuffers {
    fa::DevBuf w, chunk, rec, masks, flags, bsum, job_of_item, item_of_job, is_run, src, run_of_src, job_of_run, run_of_job, window_of_run, rows, mrows;
    const float *d_w = nullptr;                   // the weights on the device: the caller's, or `w`
    float *d_rows = nullptr, *d_mrows = nullptr;  // the row outputs on the device: the caller's, or `rows` / `mrows`
};

// the buffers of the selection stage and their H2D copies; flags ([0] bad, [1] jobs, [2] runs) zeroed
fa_status stage_plan(fa_ctx *ctx, const PlanCall &c, const Plan &p, PlanBuffers &b) {
    hipStream_t st = ctx->stream;
    const size_t wbytes = sizeof(float) * c.C * c.F * c.S, idx = sizeof(int32_t) * p.items;
    FA_TRY(fa::take(ctx, "embedding plan", {{&b.w, wbytes, !c.device, c.weights}, {&b.chunk, sizeof(int32_t) * p.nw, true, p.win.chunk.data()},
                                            {&b.rec, sizeof(ItemRec) * p.items}, {&b.masks, sizeof(float) * p.items * c.F, c.cfg->skip_enabled != 0},
                                            {&b.flags, sizeof(int32_t) * 4}, {&b.bsum, sizeof(int32_t) * select_blocks(p.items)}, {&b.job_of_item, idx},
                                            {&b.item_of_job, idx}, {&b.is_run, idx}, {&b.src, idx}, {&b.run_of_src, idx}, {&b.job_of_run, idx},
                                            {&b.run_of_job, idx}, {&b.window_of_run, idx}}));
    b.d_w = c.device ? c.weights : b.w.as<float>();
    FA_HIP_TRY(ctx, hipMemsetAsync(b.flags.p, 0, sizeof(int32_t) * 4, st));
    return FA_SUCCESS;
}

// the selection stage and its counts (one synchronisation: the row outputs are sized by them)
fa_status select_jobs(fa_ctx *ctx, const PlanCall &c, const Plan &p, const PlanBuffers &b, int64_t &jobs, int64_t &runs) {
    hipStream_t st = ctx->stream;
    const bool skip = c.cfg->skip_enabled != 0;
    const StatsArgs sa{b.d_w, b.chunk.as<int32_t>(), b.rec.as<ItemRec>(), skip ? b.masks.as<float>() : nullptr, b.flags.as<int32_t>(), static_cast<int32_t>(p.nw),
                       c.F, c.S, p.g.W, c.cfg->exclude_overlap != 0, c.cfg->overlap_threshold, static_cast<float>(p.g.min_frames), static_cast<float>(c.F) * 0.2f};
    const SelectArgs se{b.flags.as<int32_t>(), b.bsum.as<int32_t>(), b.job_of_item.as<int32_t>(), b.item_of_job.as<int32_t>(), b.is_run.as<int32_t>(),
                        b.src.as<int32_t>(), b.run_of_src.as<int32_t>(), b.job_of_run.as<int32_t>(), b.run_of_job.as<int32_t>(), b.window_of_run.as<int32_t>(),
                        p.g.B, skip, c.cfg->skip_threshold};
    launch_select(st, sa, se);
    FA_HIP_TRY(ctx, hipGetLastError());
    int32_t flags[4];
    FA_HIP_TRY(ctx, hipMemcpyAsync(flags, b.flags.p, sizeof(flags), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flags[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: a speaker weight of a planned chunk is not finite");
    jobs = flags[1];
    runs = flags[2];
    return FA_SUCCESS;
}

// the model's weight rows and the mask rows, into the caller's device memory or into buffers of this call
fa_status write_rows(fa_ctx *ctx, const PlanCall &c, const Plan &p, PlanBuffers &b, int64_t jobs, int64_t runs) {
    b.d_rows = c.run_weights;
    b.d_mrows = c.mask_rows;
    if (!c.device) {
        FA_TRY(fa::take(ctx, "embedding plan", {{&b.rows, sizeof(float) * runs * p.g.W, runs > 0}, {&b.mrows, sizeof(float) * jobs * c.F, c.mask_rows && jobs > 0}}));
        b.d_rows = b.rows.as<float>();
        b.d_mrows = c.mask_rows ? b.mrows.as<float>() : nullptr;
    }
    const RowArgs ra{b.d_w, b.chunk.as<int32_t>(), b.item_of_job.as<int32_t>(), b.job_of_run.as<int32_t>(), b.rec.as<ItemRec>(), c.F, c.S, p.g.W,
                     c.cfg->exclude_overlap != 0, c.cfg->overlap_threshold};
    launch_rows(ctx->stream, ra, runs, b.d_rows, jobs, b.d_mrows);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

// everything the host needs back, then the call's last synchronisation
fa_status collect_plan(fa_ctx *ctx, const PlanCall &c, const Plan &p, const PlanBuffers &b, int64_t jobs, int64_t runs, std::vector<ItemRec> &rec,
                       std::vector<int32_t> &item_of_job) {
    hipStream_t st = ctx->stream;
    rec.resize(static_cast<size_t>(p.items));
    item_of_job.resize(static_cast<size_t>(jobs));
    FA_HIP_TRY(ctx, hipMemcpyAsync(rec.data(), b.rec.p, sizeof(ItemRec) * p.items, hipMemcpyDeviceToHost, st));
    if (jobs > 0) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(item_of_job.data(), b.item_of_job.p, sizeof(int32_t) * jobs, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(c.run_of_job, b.run_of_job.p, sizeof(int32_t) * jobs, hipMemcpyDeviceToHost, st));
    }
    if (runs > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(c.window_of_run, b.window_of_run.p, sizeof(int32_t) * runs, hipMemcpyDeviceToHost, st));
    if (!c.device) {
        if (runs > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(c.run_weights, b.d_rows, sizeof(float) * runs * p.g.W, hipMemcpyDeviceToHost, st));
        if (b.d_mrows && jobs > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(c.mask_rows, b.d_mrows, sizeof(float) * jobs * c.F, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FA_SUCCESS;
}

// OfflineEmbeddingPending (:586-611): times in fp64, no FMA; the counters of fa_embedding_info
void write_records(const PlanCall &c, const Plan &p, const std::vector<ItemRec> &rec, const std::vector<int32_t> &item_of_job, int64_t jobs, int64_t runs) {
    int64_t empty = 0, fallback = 0;
    for (const ItemRec &r : rec) { empty += (r.flags & kEmpty) != 0; fallback += (r.flags & kFallback) != 0; }
    for (int64_t j = 0; j < jobs; ++j) {
        const int32_t it = item_of_job[j];
        const int64_t win = it / c.S;
        const ItemRec &r = rec[it];
        fa_export_embedding &e = c.records[j];
        e.chunk_index = p.win.chunk[win];
        e.speaker_index = static_cast<int32_t>(it - win * c.S);
        e.start_frame = r.first;
        e.end_frame = r.last;
        const double a = static_cast<double>(r.first) * p.g.fd, b = static_cast<double>(r.last + 1) * p.g.fd;
        e.start_time = p.win.offset[win] + a;
        e.end_time = p.win.offset[win] + b;
    }
    if (c.info) {
        c.info->jobs = jobs;
        c.info->runs = runs;
        c.info->empty_masks = empty;
        c.info->fallback_masks = fallback;
        c.info->skipped_embeddings = jobs - runs;
    }
}

fa_status plan(fa_ctx *ctx, const PlanCall &c) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    return fa::no_throw(ctx, "embedding plan", [&]() -> fa_status {
        Plan p;
        FA_TRY(make_plan(ctx, c, p));
        if (p.items == 0) return FA_SUCCESS;
        fa::DeviceGuard guard(ctx->device);
        PlanBuffers b;
        int64_t jobs = 0, runs = 0;
        std::vector<ItemRec> rec;
        std::vector<int32_t> item_of_job;
        FA_TRY(stage_plan(ctx, c, p, b));
        FA_TRY(select_jobs(ctx, c, p, b, jobs, runs));
        FA_TRY(write_rows(ctx, c, p, b, jobs, runs));
        FA_TRY(collect_plan(ctx, c, p, b, jobs, runs, rec, item_of_job));
        write_records(c, p, rec, item_of_job, jobs, runs);
        return FA_SUCCESS;
    });
}

// ---------------------------------------------------------------- fa_embedding_span_inputs

fa_status span_inputs(fa_ctx *ctx, const fa_embedding_config *cfg, const float *audio, int64_t total_samples, const double *spans, int64_t n,
                      float *windows, float *weights, fa_status *statuses, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!config_ok(cfg)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "span inputs: bad config");
    if (n < 0 || total_samples < 0 || (n > 0 && (!spans || !windows || !weights || !statuses)) || (total_samples > 0 && n > 0 && !audio))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "span inputs: bad arguments");
    if (n == 0) return FA_SUCCESS;
    const Geometry g = geometry(*cfg, 0);
    return fa::no_throw(ctx, "span inputs", [&]() -> fa_status {
    std::vector<int64_t> start(static_cast<size_t>(n)), len(static_cast<size_t>(n));
    std::vector<int32_t> active(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        const Span s = span_geometry(spans[2 * i], spans[2 * i + 1], cfg->sample_rate, g, total_samples);
        statuses[i] = s.ok ? FA_SUCCESS : FA_INVALID_ARGUMENT;
        start[i] = s.start;
        len[i] = s.len;
        active[i] = s.active;
    }
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_audio, b_start, b_len, b_active, b_win, b_w;
    FA_TRY(fa::take(ctx, "span inputs", {{&b_audio, sizeof(float) * total_samples, !device && total_samples > 0, audio},
                                         {&b_start, sizeof(int64_t) * n, true, start.data()}, {&b_len, sizeof(int64_t) * n, true, len.data()},
                                         {&b_active, sizeof(int32_t) * n, true, active.data()}, {&b_win, sizeof(float) * n * g.spw, !device},
                                         {&b_w, sizeof(float) * n * g.W, !device}}));
    const float *d_audio = device ? audio : b_audio.as<float>();
    float *d_win = device ? windows : b_win.as<float>(), *d_w = device ? weights : b_w.as<float>();
    launch_windows(st, d_audio, b_start.as<int64_t>(), b_len.as<int64_t>(), n, g.spw, d_win);
    launch_spans(st, b_active.as<int32_t>(), n, g.W, d_w);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(windows, d_win, sizeof(float) * n * g.spw, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(weights, d_w, sizeof(float) * n * g.W, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the host staging of start / len / active lives until here
    return FA_SUCCESS;
    });
}

// ---------------------------------------------------------------- fa_weight_resample

fa_status weight_resample(fa_ctx *ctx, const float *in, int64_t rows, int32_t n_in, int32_t n_out, float *out, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (rows < 0 || n_in < 0 || n_out < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "weight resample: negative size");
    if (rows == 0 || n_in == 0 || n_out == 0) return FA_SUCCESS;   // resample / resample2D return [] (:98-101, :110-113)
    if (!in || !out) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "weight resample: bad arguments");
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_in, b_out;
    const float *d_in = in;
    float *d_out = out;
    if (!device) {
        FA_TRY(fa::take(ctx, "weight resample", {{&b_in, sizeof(float) * rows * n_in, true, in}, {&b_out, sizeof(float) * rows * n_out}}));
        d_in = b_in.as<float>();
        d_out = b_out.as<float>();
    }
    launch_resample(st, d_in, rows, n_in, n_out, d_out);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(float) * rows * n_out, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

void fa_embedding_default_config(fa_embedding_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->window_duration = 10.0;        // OfflineDiarizerTypes.swift:46-55
    cfg->sample_rate = 16000;
    cfg->samples_per_window = 0;        // Int(Double(sampleRate) * windowDuration) (:348-353)
    cfg->overlap_threshold = 1e-3f;     // OfflineEmbeddingExtractor.swift:303
    cfg->exclude_overlap = 1;           // :297-303
    cfg->min_segment_duration = 1.0;
    cfg->batch_size = 32;
    cfg->skip_enabled = 0;              // EmbeddingSkipStrategy.none (:82-105)
    cfg->skip_threshold = 0.95f;        // the recommended maskSimilarity threshold
    cfg->weight_frames = 589;
    cfg->frame_duration = 0.0;          // windowDuration / frames
}

fa_status fa_embedding_plan(fa_ctx *ctx, const fa_embedding_config *cfg, const float *weights, int64_t chunks, int32_t frames, int32_t speakers,
                            const double *offsets, int64_t n_offsets, int64_t total_samples, fa_export_embedding *records, int32_t *run_of_job,
                            int32_t *window_of_run, int64_t *window_start, int32_t *window_chunk, float *run_weights, float *mask_rows,
                            fa_embedding_info *info) {
    return plan(ctx, PlanCall{cfg, weights, chunks, frames, speakers, offsets, n_offsets, total_samples, records, run_of_job, window_of_run, window_start,
                              window_chunk, run_weights, mask_rows, info, false});
}

fa_status fa_embedding_plan_dev(fa_ctx *ctx, const fa_embedding_config *cfg, const float *d_weights, int64_t chunks, int32_t frames, int32_t speakers,
                                const double *offsets, int64_t n_offsets, int64_t total_samples, fa_export_embedding *records, int32_t *run_of_job,
                                int32_t *window_of_run, int64_t *window_start, int32_t *window_chunk, float *d_run_weights, float *d_mask_rows,
                                fa_embedding_info *info) {
    return plan(ctx, PlanCall{cfg, d_weights, chunks, frames, speakers, offsets, n_offsets, total_samples, records, run_of_job, window_of_run, window_start,
                              window_chunk, d_run_weights, d_mask_rows, info, true});
}

fa_status fa_embedding_windows_dev(fa_ctx *ctx, const float *d_audio, int64_t total_samples, const int64_t *window_start, int64_t count,
                                   int32_t samples_per_window, float *d_out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (count < 0 || total_samples < 0 || samples_per_window <= 0 || (count > 0 && (!window_start || !d_out)) || (count > 0 && total_samples > 0 && !d_audio))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding windows: bad arguments");
    if (count == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "embedding windows", [&]() -> fa_status {
        std::vector<int64_t> sl(static_cast<size_t>(2 * count));   // starts, then lengths (:807-832)
        for (int64_t i = 0; i < count; ++i) {
            if (!slice_ok(window_start[i], total_samples))
                return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding windows: window %lld starts outside the audio", (long long)i);
            const Slice s = window_slice(window_start[i], total_samples, samples_per_window);
            sl[i] = s.start;
            sl[count + i] = s.len;
        }
        fa::DeviceGuard guard(ctx->device);
        hipStream_t st = ctx->stream;
        fa::DevBuf b;
        FA_TRY(fa::take(ctx, "embedding windows", {{&b, sizeof(int64_t) * 2 * count, true, sl.data()}}));
        launch_windows(st, d_audio, b.as<int64_t>(), b.as<int64_t>() + count, count, samples_per_window, d_out);
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the pageable staging above lives until the copy has been read
        return FA_SUCCESS;
    });
}

fa_status fa_embedding_span_inputs(fa_ctx *ctx, const fa_embedding_config *cfg, const float *audio, int64_t total_samples, const double *spans, int64_t n,
                                   float *windows, float *weights, fa_status *statuses) {
    return span_inputs(ctx, cfg, audio, total_samples, spans, n, windows, weights, statuses, false);
}

fa_status fa_embedding_span_inputs_dev(fa_ctx *ctx, const fa_embedding_config *cfg, const float *d_audio, int64_t total_samples, const double *spans,
                                       int64_t n, float *d_windows, float *d_weights, fa_status *statuses) {
    return span_inputs(ctx, cfg, d_audio, total_samples, spans, n, d_windows, d_weights, statuses, true);
}

fa_status fa_weight_resample(fa_ctx *ctx, const float *in, int64_t rows, int32_t in_frames, int32_t out_frames, float *out) {
    return weight_resample(ctx, in, rows, in_frames, out_frames, out, false);
}

fa_status fa_weight_resample_dev(fa_ctx *ctx, const float *d_in, int64_t rows, int32_t in_frames, int32_t out_frames, float *d_out) {
    return weight_resample(ctx, d_in, rows, in_frames, out_frames, d_out, true);
}

}  // extern "C"
