// rnnt_stream_host.hip — the host side of the Nemotron streaming session (kernels and launchers: rnnt_stream.hip, through
// rnnt_stream_launch.h): the handle and its device arrays, the defaults (BlankRescue.swift:26-47, Buffers.swift:35-51), the argument checks
// and the C ABI of the six device steps, the whole-state get / set / reset (session restore; resetRescueState), and the host-pointer
// twins of gate, track and merge_rescued.
#include "rnnt_stream_launch.h"

struct fa_rnnt_stream {
    int device = 0;
    fa::rns::Config c{};
    int32_t streams = 0;
    fa::DevBuf scalars, span, ring, mel_cache, silent, wanted, found, floats;
    fa::rns::StateArrays arrays() const {
        return fa::rns::StateArrays{scalars.as<int32_t>(), span.as<float>(), ring.as<float>(), mel_cache.as<float>(), silent.as<uint64_t>(), wanted.as<uint64_t>(),
                                    found.as<int32_t>(), floats.as<int64_t>(), fa::rns::kMaxWords, streams};
    }
};

static_assert(sizeof(fa_rnnt_stream_config) == sizeof(fa::rns::Config), "fa_rnnt_stream_config is rns::Config");
static_assert(sizeof(fa_rnnt_stream_info) == 16 * 4 && fa::rns::kPreHead == 16, "fa_rnnt_stream_info is the first sixteen scalars");
static_assert(sizeof(fa_rnnt_stream_request) == 40, "a request record is 40 bytes");
static_assert(FA_RNNT_STREAM_NO_LEXICAL == fa::rns::kNoLexical && FA_RNNT_STREAM_INACTIVE == fa::rns::kInactive, "the status codes are rns::Status");
static_assert(FA_RNNT_STREAM_CLASS_LANG_TAG == fa::rns::kLangTag, "the class bits are rns::Class");

namespace {

namespace rns = fa::rns;

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

const char *const kConfigFaults[] = {"", "window_samples a multiple of 4 in 4 .. 8192", "1 <= close_silent_windows <= 1024", "0 <= pre_roll_windows <= 64",
                                     "0 <= min_speech_windows <= 2^20", "1 <= max_span_samples <= 2^24", "0 <= open_slack_frames, close_slack_frames <= 2^20",
                                     "a finite rescue_rms_threshold >= 0", "0 <= vad_rms_threshold < 1", "1 <= vad_hangover_chunks <= 2^20", "1 <= mel_features <= 4096",
                                     "0 <= pre_encode_cache <= 64", "max(1, pre_encode_cache) <= total_mel_frames <= 65536",
                                     "close_silent_windows > open_slack_frames (the closures of a chunk are judged before they are merged)"};

// the config, or the text of its refusal
const char *sound_config(const fa_rnnt_stream_config *cfg, rns::Config *out) {
    std::memcpy(out, cfg, sizeof(*out));
    return kConfigFaults[rns::config_fault(*out)];
}

fa_status check_state(fa_ctx *ctx, const fa_rnnt_stream *st, const char *what) {
    if (!ctx || !st) return FA_INVALID_ARGUMENT;
    if (st->device != ctx->device) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: the state lives on another device than the context", what);
    return FA_SUCCESS;
}

// the byte ranges of one stream (or of all, stream == -1) in the four state arrays
struct Range { void *p; size_t bytes; };
void ranges_of(const fa_rnnt_stream *st, const int32_t stream, Range out[4]) {
    const size_t n = stream < 0 ? static_cast<size_t>(st->streams) : 1, b = stream < 0 ? 0 : static_cast<size_t>(stream);
    const size_t rows[4] = {rns::kScalars * 4, static_cast<size_t>(rns::span_capacity(st->c)) * 4, static_cast<size_t>(rns::pre_roll_capacity(st->c)) * 4,
                            static_cast<size_t>(rns::mel_cache_capacity(st->c)) * 4};
    void *const base[4] = {st->scalars.p, st->span.p, st->ring.p, st->mel_cache.p};
    for (int i = 0; i < 4; ++i) out[i] = Range{static_cast<char *>(base[i]) + b * rows[i], n * rows[i]};
}

// what track and finalize share
const char *track_fault(const fa_rnnt_stream *st, const void *tok_frame, const void *tok_id, const void *tok_count, const int32_t token_capacity, const void *class_of,
                        const int32_t vocab, const int32_t rescue_chunk_samples, const void *requests, const int32_t request_capacity, const void *arena,
                        const int64_t arena_capacity, const void *request_count, const void *status) {
    (void)st;
    if (!tok_count || !request_count || !status || token_capacity < 0 || (token_capacity > 0 && (!tok_frame || !tok_id))) return "token arrays for token_capacity >= 0, a request count, statuses";
    if (vocab < 0 || (vocab > 0 && !class_of)) return "a class table for vocab >= 0";
    if (rescue_chunk_samples < 4 || rescue_chunk_samples % 4 != 0 || rescue_chunk_samples > (1 << 24)) return "rescue_chunk_samples a multiple of 4 in 4 .. 2^24";
    if (request_capacity < 0 || (request_capacity > 0 && !requests)) return "request records for request_capacity >= 0";
    if (arena_capacity < 0 || (arena_capacity > 0 && !arena) || !aligned16(arena)) return "a 16-byte aligned arena for arena_capacity >= 0";
    return "";
}

}  // namespace

extern "C" {

void fa_rnnt_stream_default_config(fa_rnnt_stream_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->window_samples = 1280; c->close_silent_windows = 2; c->pre_roll_windows = 3; c->min_speech_windows = 2; c->max_span_samples = 15 * 16000;   // BlankRescue.swift:44-47
    c->open_slack_frames = 1; c->close_slack_frames = 5;                                                                                          // :145-148
    c->rescue_rms_threshold = 0.0025f;                                                                                                            // :26-33
    c->vad_rms_threshold = 0.0f; c->vad_hangover_chunks = 2;                                                                                      // Buffers.swift:35-51
    c->mel_features = 128; c->pre_encode_cache = 9; c->total_mel_frames = 0;
}

fa_status fa_rnnt_stream_geometry(const fa_rnnt_stream_config *cfg, fa_rnnt_stream_geometry_info *out) {
    if (!cfg || !out) return FA_INVALID_ARGUMENT;
    rns::Config c;
    std::memset(out, 0, sizeof(*out));
    if (sound_config(cfg, &c)[0]) return FA_INVALID_ARGUMENT;
    out->span_capacity = rns::span_capacity(c); out->pre_roll_capacity = rns::pre_roll_capacity(c); out->mel_cache_capacity = rns::mel_cache_capacity(c);
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_rms(const float *x, int64_t n, int32_t gate, float *rms) {
    if (!rms || n < 0 || (n > 0 && !x)) return FA_INVALID_ARGUMENT;
    *rms = rns::rms(x, n, gate ? rns::kGateWaves : 1);
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_create(fa_ctx *ctx, const fa_rnnt_stream_config *cfg, int32_t streams, fa_rnnt_stream **out) {
    if (!ctx || !cfg || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    rns::Config c;
    const char *fault = sound_config(cfg, &c);
    if (fault[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream: %s", fault);
    if (streams < 1 || streams > 65535) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream: 1 <= streams <= 65535");
    return fa::no_throw(ctx, "fa_rnnt_stream_create", [&]() {
        fa::DeviceGuard guard(ctx->device);
        fa_rnnt_stream *st = new fa_rnnt_stream;
        st->device = ctx->device; st->streams = streams; st->c = c;
        const size_t B = static_cast<size_t>(streams);
        const std::pair<fa::DevBuf *, size_t> bufs[] = {
            {&st->scalars, B * rns::kScalars * 4}, {&st->span, B * rns::span_capacity(c) * 4}, {&st->ring, B * rns::pre_roll_capacity(c) * 4},
            {&st->mel_cache, B * rns::mel_cache_capacity(c) * 4}, {&st->silent, B * rns::kMaxWords * 8}, {&st->wanted, B * rns::kMaxWords * 8},
            {&st->found, (B + 1) * 4}, {&st->floats, (B + 1) * 8}};
        fa_status status = FA_SUCCESS;
        for (const auto &b : bufs) {
            if (status == FA_SUCCESS) status = fa::take_once(ctx, "fa_rnnt_stream_create", {{b.first, b.second}});
            if (status == FA_SUCCESS) status = fa::hip_status(ctx, hipMemsetAsync(b.first->p, 0, b.second, ctx->stream), "rnnt_stream: clear");
        }
        if (status == FA_SUCCESS) status = fa::hip_status(ctx, hipStreamSynchronize(ctx->stream), "rnnt_stream: clear");
        if (status != FA_SUCCESS) { delete st; return status; }
        *out = st;
        return FA_SUCCESS;
    });
}

void fa_rnnt_stream_destroy(fa_rnnt_stream *st) {
    if (!st) return;
    fa::DeviceGuard guard(st->device);
    delete st;
}

fa_status fa_rnnt_stream_reset(fa_ctx *ctx, fa_rnnt_stream *st, int32_t stream) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_reset"));
    if (stream < -1 || stream >= st->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream reset: stream %d of %d", stream, st->streams);
    fa::DeviceGuard guard(ctx->device);
    Range r[4];
    ranges_of(st, stream, r);
    for (const Range &x : r) FA_HIP_TRY(ctx, hipMemsetAsync(x.p, 0, x.bytes, ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_get(fa_ctx *ctx, fa_rnnt_stream *st, int32_t stream, fa_rnnt_stream_info *info, float *span_audio, float *pre_roll, float *mel_cache) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_get"));
    if (!info || stream < 0 || stream >= st->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream get: a record and a stream of the state");
    return fa::no_throw(ctx, "fa_rnnt_stream_get", [&]() {
        fa::DeviceGuard guard(ctx->device);
        Range r[4];
        ranges_of(st, stream, r);
        int32_t sc[rns::kScalars];
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpy(sc, r[0].p, sizeof(sc), hipMemcpyDeviceToHost));
        std::memcpy(info, sc, sizeof(*info));
        if (span_audio) {   // the floats of the count, zeros behind them
            std::memset(span_audio, 0, r[1].bytes);
            if (sc[rns::kSpanLen] > 0) FA_HIP_TRY(ctx, hipMemcpy(span_audio, r[1].p, static_cast<size_t>(sc[rns::kSpanLen]) * 4, hipMemcpyDeviceToHost));
        }
        if (pre_roll) {     // the ring, oldest window first
            std::memset(pre_roll, 0, r[2].bytes);
            const int32_t W = st->c.window_samples, P = st->c.pre_roll_windows, held = sc[rns::kPreLen] / W;
            for (int32_t i = 0; i < held; ++i)
                FA_HIP_TRY(ctx, hipMemcpy(pre_roll + static_cast<size_t>(i) * W, static_cast<float *>(r[2].p) + static_cast<size_t>((sc[rns::kPreHead] + i) % P) * W,
                                          static_cast<size_t>(W) * 4, hipMemcpyDeviceToHost));
        }
        if (mel_cache) FA_HIP_TRY(ctx, hipMemcpy(mel_cache, r[3].p, r[3].bytes, hipMemcpyDeviceToHost));
        return FA_SUCCESS;
    });
}

fa_status fa_rnnt_stream_set(fa_ctx *ctx, fa_rnnt_stream *st, int32_t stream, const fa_rnnt_stream_info *info, const float *span_audio, const float *pre_roll,
                             const float *mel_cache) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_set"));
    if (!info || stream < 0 || stream >= st->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream set: a record and a stream of the state");
    const int32_t W = st->c.window_samples, sl = info->span_samples, pl = info->pre_roll_samples, mf = info->mel_cache_frames;
    if (sl < 0 || sl % W != 0 || sl > st->c.max_span_samples || pl < 0 || pl % W != 0 || pl > st->c.pre_roll_windows * W || mf < 0 || mf > st->c.pre_encode_cache ||
        (sl > 0 && (!span_audio || !info->span_open || info->span_overflowed)) || (pl > 0 && !pre_roll) || (mf > 0 && !mel_cache) || info->span_speech_windows < 0 ||
        info->silent_window_run < 0 || info->span_pre_roll_frames < 0)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream set: whole windows within the slabs, an array for every count, span audio only in an open span");
    fa::DeviceGuard guard(ctx->device);
    FA_TRY(fa_rnnt_stream_reset(ctx, st, stream));
    Range r[4];
    ranges_of(st, stream, r);
    int32_t sc[rns::kScalars] = {};
    std::memcpy(sc, info, sizeof(*info));
    sc[rns::kOpen] = info->span_open != 0; sc[rns::kOverflowed] = info->span_overflowed != 0;
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sl > 0) FA_HIP_TRY(ctx, hipMemcpy(r[1].p, span_audio, static_cast<size_t>(sl) * 4, hipMemcpyHostToDevice));
    if (pl > 0) FA_HIP_TRY(ctx, hipMemcpy(r[2].p, pre_roll, static_cast<size_t>(pl) * 4, hipMemcpyHostToDevice));                       // the ring's head at slot 0
    if (mf > 0) FA_HIP_TRY(ctx, hipMemcpy(r[3].p, mel_cache, r[3].bytes, hipMemcpyHostToDevice));
    FA_HIP_TRY(ctx, hipMemcpy(r[0].p, sc, sizeof(sc), hipMemcpyHostToDevice));
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_gate_dev(fa_ctx *ctx, fa_rnnt_stream *st, const float *d_chunks, int32_t chunk_samples, const int32_t *d_active, float *d_rms, int32_t *d_skip,
                                  int32_t *d_run_list, int32_t *d_run_count, int32_t *d_status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_gate_dev"));
    if (chunk_samples < 0 || (chunk_samples > 0 && !d_chunks) || !d_rms || !d_skip || !d_run_list || !d_run_count || !d_status)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream gate: pointers, chunk_samples >= 0");
    fa::DeviceGuard guard(ctx->device);
    rns::launch_gate(ctx->stream, rns::GateArgs{st->arrays(), st->c, d_chunks, chunk_samples, d_active, d_rms, d_skip, d_run_list, d_run_count, d_status});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_mel_inputs_dev(fa_ctx *ctx, fa_rnnt_stream *st, const float *d_mel, int32_t chunk_frames, int64_t stream_stride, int64_t row_stride,
                                        int64_t frame_stride, const int32_t *d_streams, const int32_t *d_count, int32_t max_count, float *d_rows, int32_t *d_status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_mel_inputs_dev"));
    if (chunk_frames < 0 || chunk_frames > (1 << 24) || (chunk_frames > 0 && !d_mel) || stream_stride < 0 || row_stride < 0 || frame_stride < 1 || !d_streams || !d_count ||
        max_count < 0 || max_count > st->streams || !d_rows || !d_status)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream mel_inputs: pointers, 0 <= chunk_frames <= 2^24, strides >= 0 (frames >= 1), 0 <= max_count <= streams");
    if (max_count == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    rns::launch_mel(ctx->stream, rns::MelArgs{st->arrays(), st->c, d_mel, chunk_frames, stream_stride, row_stride, frame_stride, d_streams, d_count, max_count, d_rows, d_status});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_advance_dev(fa_ctx *ctx, fa_rnnt_stream *st, const int32_t *d_streams, const int32_t *d_count, int32_t max_count, const int32_t *d_frames,
                                     int32_t frames) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_advance_dev"));
    if (!d_streams || !d_count || max_count < 0 || max_count > st->streams || frames < 0)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream advance: a list, its count, 0 <= max_count <= streams, frames >= 0");
    if (max_count == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    rns::launch_advance(ctx->stream, rns::AdvanceArgs{st->arrays(), d_streams, d_count, max_count, d_frames, frames});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_track_dev(fa_ctx *ctx, fa_rnnt_stream *st, const float *d_chunks, int32_t chunk_samples, const int32_t *d_active, const int32_t *d_tok_frame,
                                   const int32_t *d_tok_id, const int32_t *d_tok_count, int32_t token_capacity, const uint8_t *d_class, int32_t vocab,
                                   int32_t rescue_chunk_samples, fa_rnnt_stream_request *d_requests, int32_t request_capacity, float *d_arena, int64_t arena_capacity,
                                   int32_t *d_request_count, int32_t *d_status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_track_dev"));
    const char *fault = track_fault(st, d_tok_frame, d_tok_id, d_tok_count, token_capacity, d_class, vocab, rescue_chunk_samples, d_requests, request_capacity, d_arena,
                                    arena_capacity, d_request_count, d_status);
    if (fault[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream track: %s", fault);
    if (chunk_samples < 0 || (chunk_samples > 0 && !d_chunks) || chunk_samples / st->c.window_samples > rns::kMaxWords * 64)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream track: chunk rows, 0 <= chunk_samples <= %d windows", rns::kMaxWords * 64);
    fa::DeviceGuard guard(ctx->device);
    rns::launch_track(ctx->stream, rns::TrackArgs{st->arrays(), st->c, d_chunks, chunk_samples, d_active, nullptr, nullptr, st->streams, 0, d_tok_frame, d_tok_id, d_tok_count,
                                                  token_capacity, d_class, vocab, rescue_chunk_samples, d_requests, request_capacity, d_arena, arena_capacity, d_request_count,
                                                  d_status});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_finalize_dev(fa_ctx *ctx, fa_rnnt_stream *st, const int32_t *d_streams, const int32_t *d_count, int32_t max_count, const int32_t *d_tok_frame,
                                      const int32_t *d_tok_id, const int32_t *d_tok_count, int32_t token_capacity, const uint8_t *d_class, int32_t vocab,
                                      int32_t rescue_chunk_samples, fa_rnnt_stream_request *d_requests, int32_t request_capacity, float *d_arena, int64_t arena_capacity,
                                      int32_t *d_request_count, int32_t *d_status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_finalize_dev"));
    const char *fault = track_fault(st, d_tok_frame, d_tok_id, d_tok_count, token_capacity, d_class, vocab, rescue_chunk_samples, d_requests, request_capacity, d_arena,
                                    arena_capacity, d_request_count, d_status);
    if (fault[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream finalize: %s", fault);
    if (!d_streams || !d_count || max_count < 1 || max_count > st->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream finalize: a list, its count, 1 <= max_count <= streams");
    fa::DeviceGuard guard(ctx->device);
    rns::launch_track(ctx->stream, rns::TrackArgs{st->arrays(), st->c, nullptr, 0, nullptr, d_streams, d_count, max_count, 1, d_tok_frame, d_tok_id, d_tok_count, token_capacity,
                                                  d_class, vocab, rescue_chunk_samples, d_requests, request_capacity, d_arena, arena_capacity, d_request_count, d_status});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_rnnt_stream_merge_rescued_dev(fa_ctx *ctx, fa_rnnt_stream *st, const fa_rnnt_stream_request *d_requests, const int32_t *d_request_count,
                                           int32_t request_capacity, const int32_t *d_staged_ids, const int32_t *d_staged_frames, const int32_t *d_staged_id_count,
                                           const int32_t *d_staged_frame_count, int32_t staged_capacity, int32_t *d_live_ids, int32_t *d_live_frames,
                                           int32_t *d_live_timed_ids, int32_t *d_live_id_count, int32_t *d_live_timed_count, int32_t live_capacity, const uint8_t *d_class,
                                           int32_t vocab, int32_t *d_request_status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_merge_rescued_dev"));
    if (!d_request_count || request_capacity < 0 || (request_capacity > 0 && (!d_requests || !d_staged_id_count || !d_staged_frame_count || !d_request_status)) ||
        staged_capacity < 0 || (staged_capacity > 0 && request_capacity > 0 && (!d_staged_ids || !d_staged_frames)) || live_capacity < 0 ||
        (live_capacity > 0 && (!d_live_ids || !d_live_frames)) || !d_live_id_count || !d_live_timed_count || vocab < 0 || (vocab > 0 && !d_class))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream merge_rescued: arrays for every capacity >= 0, the counts, a class table for vocab >= 0");
    if (request_capacity == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    rns::launch_merge(ctx->stream, rns::MergeArgs{st->arrays(), d_requests, d_request_count, request_capacity, d_staged_ids, d_staged_frames, d_staged_id_count,
                                                  d_staged_frame_count, staged_capacity, d_live_ids, d_live_frames, d_live_timed_ids, d_live_id_count, d_live_timed_count,
                                                  live_capacity, d_class, vocab, d_request_status});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

/* the same on HOST arrays: staged, run, copied back, one synchronisation */
fa_status fa_rnnt_stream_gate(fa_ctx *ctx, fa_rnnt_stream *st, const float *chunks, int32_t chunk_samples, const int32_t *active, float *rms, int32_t *skip,
                              int32_t *run_list, int32_t *run_count, int32_t *status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_gate"));
    if (chunk_samples < 0 || (chunk_samples > 0 && !chunks) || !rms || !skip || !run_list || !run_count || !status)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream gate: pointers, chunk_samples >= 0");
    return fa::no_throw(ctx, "fa_rnnt_stream_gate", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t B = static_cast<size_t>(st->streams);
        fa::DevBuf d_chunks, d_active, d_rms, d_skip, d_list, d_count, d_status;
        FA_TRY(fa::take(ctx, "fa_rnnt_stream_gate", {{&d_chunks, B * chunk_samples * 4, true, chunks}, {&d_active, B * 4, active != nullptr, active}, {&d_rms, B * 4, true, rms},
                                                     {&d_skip, B * 4, true, skip}, {&d_list, B * 4, true, run_list}, {&d_count, 4}, {&d_status, B * 4}}));
        FA_TRY(fa_rnnt_stream_gate_dev(ctx, st, d_chunks.as<float>(), chunk_samples, active ? d_active.as<int32_t>() : nullptr, d_rms.as<float>(), d_skip.as<int32_t>(),
                                       d_list.as<int32_t>(), d_count.as<int32_t>(), d_status.as<int32_t>()));
        FA_HIP_TRY(ctx, hipMemcpyAsync(rms, d_rms.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(skip, d_skip.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(run_list, d_list.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(run_count, d_count.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(status, d_status.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_rnnt_stream_track(fa_ctx *ctx, fa_rnnt_stream *st, const float *chunks, int32_t chunk_samples, const int32_t *active, const int32_t *tok_frame,
                               const int32_t *tok_id, const int32_t *tok_count, int32_t token_capacity, const uint8_t *class_of, int32_t vocab, int32_t rescue_chunk_samples,
                               fa_rnnt_stream_request *requests, int32_t request_capacity, float *arena, int64_t arena_capacity, int32_t *request_count, int32_t *status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_track"));
    const char *fault = track_fault(st, tok_frame, tok_id, tok_count, token_capacity, class_of, vocab, rescue_chunk_samples, requests, request_capacity,
                                    arena ? reinterpret_cast<const void *>(uintptr_t{16}) : nullptr, arena_capacity, request_count, status);   // the staged arena is aligned
    if (fault[0] || (arena_capacity > 0 && !arena)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream track: %s", fault[0] ? fault : "an arena for arena_capacity > 0");
    if (chunk_samples < 0 || (chunk_samples > 0 && !chunks)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream track: chunk rows, chunk_samples >= 0");
    return fa::no_throw(ctx, "fa_rnnt_stream_track", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t B = static_cast<size_t>(st->streams), T = static_cast<size_t>(token_capacity), R = static_cast<size_t>(request_capacity) * sizeof(fa_rnnt_stream_request);
        const size_t A = static_cast<size_t>(arena_capacity) * 4;
        fa::DevBuf d_chunks, d_active, d_frame, d_id, d_count, d_class, d_req, d_arena, d_found, d_status;
        FA_TRY(fa::take(ctx, "fa_rnnt_stream_track", {{&d_chunks, B * chunk_samples * 4, true, chunks}, {&d_active, B * 4, active != nullptr, active},
                                                      {&d_frame, B * T * 4, true, tok_frame}, {&d_id, B * T * 4, true, tok_id}, {&d_count, B * 4, true, tok_count},
                                                      {&d_class, static_cast<size_t>(vocab), true, class_of}, {&d_req, R, true, requests}, {&d_arena, A, true, arena},
                                                      {&d_found, 4}, {&d_status, B * 4}}));
        FA_TRY(fa_rnnt_stream_track_dev(ctx, st, d_chunks.as<float>(), chunk_samples, active ? d_active.as<int32_t>() : nullptr, d_frame.as<int32_t>(), d_id.as<int32_t>(),
                                        d_count.as<int32_t>(), token_capacity, d_class.as<uint8_t>(), vocab, rescue_chunk_samples, d_req.as<fa_rnnt_stream_request>(),
                                        request_capacity, d_arena.as<float>(), arena_capacity, d_found.as<int32_t>(), d_status.as<int32_t>()));
        if (R) FA_HIP_TRY(ctx, hipMemcpyAsync(requests, d_req.p, R, hipMemcpyDeviceToHost, ctx->stream));
        if (A) FA_HIP_TRY(ctx, hipMemcpyAsync(arena, d_arena.p, A, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(request_count, d_found.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(status, d_status.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_rnnt_stream_merge_rescued(fa_ctx *ctx, fa_rnnt_stream *st, const fa_rnnt_stream_request *requests, int32_t request_count, const int32_t *staged_ids,
                                       const int32_t *staged_frames, const int32_t *staged_id_count, const int32_t *staged_frame_count, int32_t staged_capacity,
                                       int32_t *live_ids, int32_t *live_frames, int32_t *live_timed_ids, int32_t *live_id_count, int32_t *live_timed_count,
                                       int32_t live_capacity, const uint8_t *class_of, int32_t vocab, int32_t *request_status) {
    FA_TRY(check_state(ctx, st, "fa_rnnt_stream_merge_rescued"));
    if (request_count < 0 || (request_count > 0 && (!requests || !staged_id_count || !staged_frame_count || !request_status)) || staged_capacity < 0 ||
        (staged_capacity > 0 && request_count > 0 && (!staged_ids || !staged_frames)) || live_capacity < 0 || (live_capacity > 0 && (!live_ids || !live_frames)) ||
        !live_id_count || !live_timed_count || vocab < 0 || (vocab > 0 && !class_of))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt_stream merge_rescued: arrays for every capacity >= 0, the counts, a class table for vocab >= 0");
    if (request_count == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "fa_rnnt_stream_merge_rescued", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t B = static_cast<size_t>(st->streams), N = static_cast<size_t>(request_count), S = N * staged_capacity * 4, L = B * live_capacity * 4;
        fa::DevBuf d_req, d_n, d_sid, d_sfr, d_sic, d_sfc, d_ids, d_fr, d_tid, d_idc, d_tc, d_class, d_status;
        FA_TRY(fa::take(ctx, "fa_rnnt_stream_merge_rescued", {{&d_req, N * sizeof(fa_rnnt_stream_request), true, requests}, {&d_n, 4, true, &request_count}, {&d_sid, S, true, staged_ids},
                                                              {&d_sfr, S, true, staged_frames}, {&d_sic, N * 4, true, staged_id_count}, {&d_sfc, N * 4, true, staged_frame_count},
                                                              {&d_ids, L, true, live_ids}, {&d_fr, L, true, live_frames}, {&d_tid, L, live_timed_ids != nullptr, live_timed_ids},
                                                              {&d_idc, B * 4, true, live_id_count}, {&d_tc, B * 4, true, live_timed_count},
                                                              {&d_class, static_cast<size_t>(vocab), true, class_of}, {&d_status, N * 4}}));
        FA_TRY(fa_rnnt_stream_merge_rescued_dev(ctx, st, d_req.as<fa_rnnt_stream_request>(), d_n.as<int32_t>(), request_count, d_sid.as<int32_t>(), d_sfr.as<int32_t>(),
                                                d_sic.as<int32_t>(), d_sfc.as<int32_t>(), staged_capacity, d_ids.as<int32_t>(), d_fr.as<int32_t>(),
                                                live_timed_ids ? d_tid.as<int32_t>() : nullptr, d_idc.as<int32_t>(), d_tc.as<int32_t>(), live_capacity, d_class.as<uint8_t>(), vocab,
                                                d_status.as<int32_t>()));
        if (L) {
            FA_HIP_TRY(ctx, hipMemcpyAsync(live_ids, d_ids.p, L, hipMemcpyDeviceToHost, ctx->stream));
            FA_HIP_TRY(ctx, hipMemcpyAsync(live_frames, d_fr.p, L, hipMemcpyDeviceToHost, ctx->stream));
            if (live_timed_ids) FA_HIP_TRY(ctx, hipMemcpyAsync(live_timed_ids, d_tid.p, L, hipMemcpyDeviceToHost, ctx->stream));
        }
        FA_HIP_TRY(ctx, hipMemcpyAsync(live_id_count, d_idc.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(live_timed_count, d_tc.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(request_status, d_status.p, N * 4, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

}  // extern "C"
