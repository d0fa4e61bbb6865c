// sortformer_stream_host.hip — the host side of the streaming Sortformer state (kernels and launcher: sortformer_stream.hip, through
// sortformer_stream_launch.h): the handle and its device arrays, the defaults and presets (SortformerTypes.swift:26-97, 121-216), the argument
// checks and the C ABI of the update, the whole-state get / set / reset (session restore; SortformerStreamingState.cleanup), and the pure
// host restatements of the chunk geometry (SortformerDiarizer.swift:933-979, SortformerTypes.swift:347-383) with the thin packer over
// the shared row copy (row_pack_launch.h; the kernel is instantiated in sortformer_stream.hip).
#include "sortformer_stream_launch.h"

struct fa_sortformer_stream {
    int device = 0;
    fa::sfs::Config c{};
    fa::sfs::Slabs s{};
    fa::sfs::Quotas q{};
    int32_t streams = 0;
    fa::DevBuf spkcache, spk_len, fifo, fifo_len, spk_preds, fifo_preds, mean, meta, plan, silent, sel, popped, gathered;
    fa::sfs::StateArrays arrays() const {
        return fa::sfs::StateArrays{spkcache.as<float>(), spk_len.as<int32_t>(), fifo.as<float>(), fifo_len.as<int32_t>(), spk_preds.as<float>(), fifo_preds.as<float>(),
                                    mean.as<float>(), meta.as<int32_t>(), plan.as<fa::sfs::Plan>(), silent.as<uint8_t>(), sel.as<int32_t>(), popped.as<float>(),
                                    gathered.as<float>(), streams};
    }
};

static_assert(sizeof(fa_sortformer_stream_config) == sizeof(fa::sfs::Config), "fa_sortformer_stream_config is sfs::Config");
static_assert(sizeof(fa_sortformer_chunk) == sizeof(fa::sfs::Chunk), "fa_sortformer_chunk is sfs::Chunk");
static_assert(FA_SORTFORMER_STREAM_BAD_OPERAND == fa::sfs::kBadOperand && FA_SORTFORMER_STREAM_INACTIVE == fa::sfs::kInactive, "the status codes are sfs::Status");

namespace {

namespace sfs = fa::sfs;

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

const char *const kConfigFaults[] = {"", "1 <= speakers <= 4", "d_model a multiple of 4 in 4 .. 8192", "contexts, fifo_len, sil_frames_per_spk >= 0; max_chunk_frames, subsampling, n_mels >= 1",
                                     "a length above 2^20", "the boost and quota rates in [0, 1024]", "0 < pred_score_threshold < 1, finite thresholds", "max_index >= 1",
                                     "speakers * (spkcache_len + the longest pop + sil_frames_per_spk) reaches max_index: a live index would be taken for the sentinel",
                                     "the scored rows do not fit one workgroup's LDS"};

// the clamped config, or the text of its refusal
const char *sound_config(const fa_sortformer_stream_config *cfg, sfs::Config *out) {
    std::memcpy(out, cfg, sizeof(*out));
    if (out->speakers < 1 || out->speakers > sfs::kMaxSpeakers) return kConfigFaults[1];   // before the clamps divide by it
    sfs::clamp(*out);
    return kConfigFaults[sfs::config_fault(*out)];
}

fa_status check_state(fa_ctx *ctx, const fa_sortformer_stream *st, const char *what) {
    if (!ctx || !st) return FA_INVALID_ARGUMENT;
    if (st->device != ctx->device) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: the state lives on another device than the context", what);
    return FA_SUCCESS;
}

// the byte ranges of one stream (or of all, stream == -1) in every state array
struct Range { void *p; size_t bytes; };
void ranges_of(const fa_sortformer_stream *st, const int32_t stream, Range out[8]) {
    const size_t n = stream < 0 ? static_cast<size_t>(st->streams) : 1, b = stream < 0 ? 0 : static_cast<size_t>(stream);
    const size_t D = static_cast<size_t>(st->c.d_model), S = static_cast<size_t>(st->c.speakers);
    const size_t rows[8] = {static_cast<size_t>(st->c.spkcache_len) * D * 4, 4, static_cast<size_t>(st->c.fifo_len) * D * 4, 4, static_cast<size_t>(st->s.score_rows) * S * 4,
                            static_cast<size_t>(st->s.fifo_pred_rows) * S * 4, D * 4, sfs::kMetaInts * 4};
    void *const base[8] = {st->spkcache.p, st->spk_len.p, st->fifo.p, st->fifo_len.p, st->spk_preds.p, st->fifo_preds.p, st->mean.p, st->meta.p};
    for (int i = 0; i < 8; ++i) out[i] = Range{static_cast<char *>(base[i]) + b * rows[i], n * rows[i]};
}

struct Preset { int32_t chunk_len, left, right, fifo_len, spkcache_len, period; };
// SortformerTypes.swift:121-216: default = fastV2 = fastV2_1; balancedV2(_1); highContextV2(_1); efficientV2_1
constexpr Preset kPresets[] = {{6, 1, 7, 40, 188, 31}, {6, 1, 7, 188, 188, 144}, {340, 1, 40, 40, 188, 300}, {25, 1, 7, 40, 188, 31}};

}  // namespace

extern "C" {

fa_status fa_sortformer_stream_preset_config(int32_t preset, fa_sortformer_stream_config *c) {
    if (!c || preset < 0 || preset >= static_cast<int32_t>(sizeof(kPresets) / sizeof(kPresets[0]))) return FA_INVALID_ARGUMENT;
    const Preset &p = kPresets[preset];
    std::memset(c, 0, sizeof(*c));
    c->speakers = 4; c->d_model = 512; c->subsampling = 8; c->n_mels = 128;                                  // SortformerTypes.swift:23-29, 74
    c->chunk_len = p.chunk_len; c->chunk_left_context = p.left; c->chunk_right_context = p.right; c->fifo_len = p.fifo_len;
    c->spkcache_len = p.spkcache_len; c->spkcache_update_period = p.period;
    c->sil_frames_per_spk = 3; c->max_index = 99999;                                                        // :55, :97
    c->silence_threshold = 0.2f; c->pred_score_threshold = 0.25f; c->scores_boost_latest = 0.05f;            // :79-94
    c->strong_boost_rate = 0.75f; c->weak_boost_rate = 1.5f; c->min_pos_scores_rate = 0.5f;
    sfs::Config k;
    std::memcpy(&k, c, sizeof(k));
    sfs::clamp(k);
    std::memcpy(c, &k, sizeof(k));
    c->max_chunk_frames = c->chunk_len + c->chunk_left_context + c->chunk_right_context;
    return FA_SUCCESS;
}

void fa_sortformer_stream_default_config(fa_sortformer_stream_config *c) { (void)fa_sortformer_stream_preset_config(FA_SORTFORMER_STREAM_PRESET_DEFAULT, c); }

fa_status fa_sortformer_stream_geometry(const fa_sortformer_stream_config *cfg, fa_sortformer_stream_geometry_info *out) {
    if (!cfg || !out) return FA_INVALID_ARGUMENT;
    sfs::Config c;
    std::memset(out, 0, sizeof(*out));
    if (sound_config(cfg, &c)[0]) return FA_INVALID_ARGUMENT;
    const sfs::Slabs s = sfs::slabs(c);
    const sfs::Quotas q = sfs::quotas(c);
    out->chunk_len = c.chunk_len; out->spkcache_len = c.spkcache_len; out->spkcache_update_period = c.spkcache_update_period;
    out->max_pop = s.max_pop; out->score_rows = s.score_rows; out->out_rows = c.max_chunk_frames;
    out->chunk_mel_frames = (c.chunk_len + c.chunk_left_context + c.chunk_right_context) * c.subsampling;
    out->spkcache_len_per_spk = q.len_per_spk; out->strong_boost_per_spk = q.strong; out->weak_boost_per_spk = q.weak; out->min_pos_scores_per_spk = q.min_pos;
    out->lds_bytes = static_cast<int32_t>(s.lds_bytes);
    return FA_SUCCESS;
}

int32_t fa_sortformer_stream_pop_out_length(const fa_sortformer_stream_config *cfg, int32_t context_length) {
    sfs::Config c;
    if (!cfg || sound_config(cfg, &c)[0] || context_length < 0) return -1;
    return context_length > c.fifo_len ? sfs::pop_out_length(c.spkcache_update_period, context_length, c.fifo_len) : 0;
}

fa_status fa_sortformer_stream_create(fa_ctx *ctx, const fa_sortformer_stream_config *cfg, int32_t streams, fa_sortformer_stream **out) {
    if (!ctx || !cfg || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    sfs::Config c;
    const char *fault = sound_config(cfg, &c);
    if (fault[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream: %s", fault);
    if (streams < 1 || streams > 65535) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream: 1 <= streams <= 65535");
    return fa::no_throw(ctx, "fa_sortformer_stream_create", [&]() {
        fa::DeviceGuard guard(ctx->device);
        fa_sortformer_stream *st = new fa_sortformer_stream;
        st->device = ctx->device; st->streams = streams; st->c = c; st->s = sfs::slabs(c); st->q = sfs::quotas(c);
        const size_t B = static_cast<size_t>(streams), D = static_cast<size_t>(c.d_model), S = static_cast<size_t>(c.speakers);
        const size_t cap = static_cast<size_t>(c.spkcache_len), pop = static_cast<size_t>(st->s.max_pop);
        const std::pair<fa::DevBuf *, size_t> bufs[] = {
            {&st->spkcache, B * cap * D * 4}, {&st->spk_len, B * 4}, {&st->fifo, B * c.fifo_len * D * 4}, {&st->fifo_len, B * 4}, {&st->spk_preds, B * st->s.score_rows * S * 4},
            {&st->fifo_preds, B * st->s.fifo_pred_rows * S * 4}, {&st->mean, B * D * 4}, {&st->meta, B * sfs::kMetaInts * 4}, {&st->plan, B * sizeof(sfs::Plan)},
            {&st->silent, B * pop}, {&st->sel, B * cap * 4}, {&st->popped, B * pop * D * 4}, {&st->gathered, B * cap * D * 4}};
        fa_status status = FA_SUCCESS;
        for (const auto &b : bufs) {
            if (status == FA_SUCCESS) status = fa::take_once(ctx, "fa_sortformer_stream_create", {{b.first, b.second}});
            if (status == FA_SUCCESS && b.second) status = fa::hip_status(ctx, hipMemsetAsync(b.first->p, 0, b.second, ctx->stream), "sortformer_stream: clear");
        }
        if (status == FA_SUCCESS) status = fa::hip_status(ctx, hipStreamSynchronize(ctx->stream), "sortformer_stream: clear");
        if (status != FA_SUCCESS) { delete st; return status; }
        *out = st;
        return FA_SUCCESS;
    });
}

void fa_sortformer_stream_destroy(fa_sortformer_stream *st) {
    if (!st) return;
    fa::DeviceGuard guard(st->device);
    delete st;
}

fa_status fa_sortformer_stream_inputs(fa_ctx *ctx, fa_sortformer_stream *st, float **d_spkcache, int32_t **d_spkcache_lengths, float **d_fifo, int32_t **d_fifo_lengths) {
    FA_TRY(check_state(ctx, st, "fa_sortformer_stream_inputs"));
    if (d_spkcache) *d_spkcache = st->spkcache.as<float>();
    if (d_spkcache_lengths) *d_spkcache_lengths = st->spk_len.as<int32_t>();
    if (d_fifo) *d_fifo = st->fifo.as<float>();
    if (d_fifo_lengths) *d_fifo_lengths = st->fifo_len.as<int32_t>();
    return FA_SUCCESS;
}

fa_status fa_sortformer_stream_reset(fa_ctx *ctx, fa_sortformer_stream *st, int32_t stream) {
    FA_TRY(check_state(ctx, st, "fa_sortformer_stream_reset"));
    if (stream < -1 || stream >= st->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream reset: stream %d of %d", stream, st->streams);
    fa::DeviceGuard guard(ctx->device);
    Range r[8];
    ranges_of(st, stream, r);
    for (const Range &x : r)
        if (x.bytes) FA_HIP_TRY(ctx, hipMemsetAsync(x.p, 0, x.bytes, ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_sortformer_stream_get(fa_ctx *ctx, fa_sortformer_stream *st, int32_t stream, fa_sortformer_stream_info *info, float *spkcache, float *spkcache_preds,
                                   float *fifo, float *fifo_preds, float *mean_silence) {
    FA_TRY(check_state(ctx, st, "fa_sortformer_stream_get"));
    if (!info || stream < 0 || stream >= st->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream get: a record and a stream of the state");
    fa::DeviceGuard guard(ctx->device);
    Range r[8];
    ranges_of(st, stream, r);
    int32_t meta[sfs::kMetaInts], lens[2];
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpy(&lens[0], r[1].p, 4, hipMemcpyDeviceToHost));
    FA_HIP_TRY(ctx, hipMemcpy(&lens[1], r[3].p, 4, hipMemcpyDeviceToHost));
    FA_HIP_TRY(ctx, hipMemcpy(meta, r[7].p, sizeof(meta), hipMemcpyDeviceToHost));
    info->spkcache_length = lens[0]; info->fifo_length = lens[1]; info->spkcache_preds_present = meta[sfs::kMetaSpkPreds]; info->fifo_preds_present = meta[sfs::kMetaFifoPreds];
    info->silence_frame_count = meta[sfs::kMetaSilCount]; info->reserved = 0;
    const size_t S4 = static_cast<size_t>(st->c.speakers) * 4;
    if (spkcache) FA_HIP_TRY(ctx, hipMemcpy(spkcache, r[0].p, r[0].bytes, hipMemcpyDeviceToHost));
    if (fifo) FA_HIP_TRY(ctx, hipMemcpy(fifo, r[2].p, r[2].bytes, hipMemcpyDeviceToHost));
    if (mean_silence) FA_HIP_TRY(ctx, hipMemcpy(mean_silence, r[6].p, r[6].bytes, hipMemcpyDeviceToHost));
    if (spkcache_preds) {   // [spkcache_len][speakers]: the rows of the length when present, zeros behind them
        std::memset(spkcache_preds, 0, st->c.spkcache_len * S4);
        if (meta[sfs::kMetaSpkPreds] && lens[0] > 0) FA_HIP_TRY(ctx, hipMemcpy(spkcache_preds, r[4].p, lens[0] * S4, hipMemcpyDeviceToHost));
    }
    if (fifo_preds) {
        std::memset(fifo_preds, 0, st->c.fifo_len * S4);
        if (meta[sfs::kMetaFifoPreds] && lens[1] > 0) FA_HIP_TRY(ctx, hipMemcpy(fifo_preds, r[5].p, lens[1] * S4, hipMemcpyDeviceToHost));
    }
    return FA_SUCCESS;
}

fa_status fa_sortformer_stream_set(fa_ctx *ctx, fa_sortformer_stream *st, int32_t stream, const fa_sortformer_stream_info *info, const float *spkcache,
                                   const float *spkcache_preds, const float *fifo, const float *fifo_preds, const float *mean_silence) {
    FA_TRY(check_state(ctx, st, "fa_sortformer_stream_set"));
    if (!info || !mean_silence || stream < 0 || stream >= st->streams)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream set: a record, a mean silence embedding and a stream of the state");
    const int32_t sl = info->spkcache_length, fl = info->fifo_length;
    const bool sp = info->spkcache_preds_present != 0, fp = info->fifo_preds_present != 0;
    if (sl < 0 || sl > st->c.spkcache_len || fl < 0 || fl > st->c.fifo_len || info->silence_frame_count < 0 || (sl > 0 && !spkcache) || (fl > 0 && !fifo) ||
        (sp && sl > 0 && !spkcache_preds) || (fl > 0 && (!fp || !fifo_preds)))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream set: lengths within the slabs, rows for every length, the FIFO's preds with its rows");
    const size_t S = static_cast<size_t>(st->c.speakers), D4 = static_cast<size_t>(st->c.d_model) * 4;
    const auto in_unit = [](const float *p, const size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (!(p[i] >= 0.0f && p[i] <= 1.0f)) return false;
        return true;
    };
    if ((sp && sl > 0 && !in_unit(spkcache_preds, sl * S)) || (fl > 0 && !in_unit(fifo_preds, fl * S)))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream set: a pred that is NaN or outside [0, 1]");
    fa::DeviceGuard guard(ctx->device);
    FA_TRY(fa_sortformer_stream_reset(ctx, st, stream));
    Range r[8];
    ranges_of(st, stream, r);
    const int32_t meta[sfs::kMetaInts] = {sp ? 1 : 0, fp ? 1 : 0, info->silence_frame_count, 0};
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sl > 0) FA_HIP_TRY(ctx, hipMemcpy(r[0].p, spkcache, sl * D4, hipMemcpyHostToDevice));
    if (fl > 0) FA_HIP_TRY(ctx, hipMemcpy(r[2].p, fifo, fl * D4, hipMemcpyHostToDevice));
    if (sp && sl > 0) FA_HIP_TRY(ctx, hipMemcpy(r[4].p, spkcache_preds, sl * S * 4, hipMemcpyHostToDevice));
    if (fl > 0) FA_HIP_TRY(ctx, hipMemcpy(r[5].p, fifo_preds, fl * S * 4, hipMemcpyHostToDevice));
    FA_HIP_TRY(ctx, hipMemcpy(r[6].p, mean_silence, D4, hipMemcpyHostToDevice));
    FA_HIP_TRY(ctx, hipMemcpy(r[1].p, &sl, 4, hipMemcpyHostToDevice));
    FA_HIP_TRY(ctx, hipMemcpy(r[3].p, &fl, 4, hipMemcpyHostToDevice));
    FA_HIP_TRY(ctx, hipMemcpy(r[7].p, meta, sizeof(meta), hipMemcpyHostToDevice));
    return FA_SUCCESS;
}

fa_status fa_sortformer_stream_update_dev(fa_ctx *ctx, fa_sortformer_stream *st, const void *d_chunk_embs, int32_t emb_dtype, const int32_t *d_emb_len, const float *d_preds,
                                          int32_t pred_stride, const int32_t *d_pred_rows, const int32_t *d_left, const int32_t *d_right, const int32_t *d_active,
                                          float *d_confirmed, float *d_tentative, int32_t *d_counts, int32_t *d_status, float *d_log_scores) {
    FA_TRY(check_state(ctx, st, "fa_sortformer_stream_update_dev"));
    if (!d_chunk_embs || !d_emb_len || !d_preds || !d_pred_rows || !d_left || !d_right || !d_confirmed || !d_tentative || !d_counts || !d_status || pred_stride < 1 ||
        pred_stride > (1 << 24) || !aligned16(d_chunk_embs) || (emb_dtype != FA_DTYPE_F32 && emb_dtype != FA_DTYPE_F16))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream update: pointers (embeddings 16-byte aligned), 1 <= pred_stride <= 2^24, fp32 or fp16 rows");
    fa::DeviceGuard guard(ctx->device);
    sfs::UpdateArgs a{st->arrays(), st->c, st->s, st->q, d_chunk_embs, emb_dtype == FA_DTYPE_F16 ? 1 : 0, d_emb_len, d_preds, pred_stride, d_pred_rows, d_left, d_right,
                      d_active, d_confirmed, d_tentative, d_counts, d_status, d_log_scores};
    sfs::launch_update(ctx->stream, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

/* the same on HOST arrays: staged, run, copied back, one synchronisation */
fa_status fa_sortformer_stream_update(fa_ctx *ctx, fa_sortformer_stream *st, const void *chunk_embs, int32_t emb_dtype, const int32_t *emb_len, const float *preds,
                                      int32_t pred_stride, const int32_t *pred_rows, const int32_t *left, const int32_t *right, const int32_t *active, float *confirmed,
                                      float *tentative, int32_t *counts, int32_t *status, float *log_scores) {
    FA_TRY(check_state(ctx, st, "fa_sortformer_stream_update"));
    if (!chunk_embs || !emb_len || !preds || !pred_rows || !left || !right || !confirmed || !tentative || !counts || !status || pred_stride < 1 || pred_stride > (1 << 24) ||
        (emb_dtype != FA_DTYPE_F32 && emb_dtype != FA_DTYPE_F16))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream update: pointers, 1 <= pred_stride <= 2^24, fp32 or fp16 rows");
    return fa::no_throw(ctx, "fa_sortformer_stream_update", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t B = static_cast<size_t>(st->streams), S = static_cast<size_t>(st->c.speakers), D = static_cast<size_t>(st->c.d_model);
        const size_t out_bytes = B * st->c.max_chunk_frames * S * 4, score_bytes = B * st->s.score_rows * S * 4;
        fa::DevBuf d_embs, d_len, d_preds, d_rows, d_left, d_right, d_active, d_conf, d_tent, d_counts, d_status, d_scores;
        FA_TRY(fa::take(ctx, "fa_sortformer_stream_update", {{&d_embs, B * st->c.max_chunk_frames * D * (emb_dtype == FA_DTYPE_F16 ? 2 : 4), true, chunk_embs},
                                                             {&d_len, B * 4, true, emb_len}, {&d_preds, B * pred_stride * S * 4, true, preds}, {&d_rows, B * 4, true, pred_rows},
                                                             {&d_left, B * 4, true, left}, {&d_right, B * 4, true, right}, {&d_active, B * 4, active != nullptr, active},
                                                             {&d_conf, out_bytes}, {&d_tent, out_bytes}, {&d_counts, B * 8}, {&d_status, B * 4},
                                                             {&d_scores, score_bytes, log_scores != nullptr, log_scores}}));
        FA_TRY(fa_sortformer_stream_update_dev(ctx, st, d_embs.p, emb_dtype, d_len.as<int32_t>(), d_preds.as<float>(), pred_stride, d_rows.as<int32_t>(), d_left.as<int32_t>(),
                                               d_right.as<int32_t>(), active ? d_active.as<int32_t>() : nullptr, d_conf.as<float>(), d_tent.as<float>(), d_counts.as<int32_t>(),
                                               d_status.as<int32_t>(), log_scores ? d_scores.as<float>() : nullptr));
        FA_HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts.p, B * 8, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(status, d_status.p, B * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (log_scores) FA_HIP_TRY(ctx, hipMemcpyAsync(log_scores, d_scores.p, score_bytes, hipMemcpyDeviceToHost, ctx->stream));
        // the rows of a refused stream are not written on the device: only the counted rows travel back
        std::vector<float> conf(out_bytes / 4), tent(out_bytes / 4);
        FA_HIP_TRY(ctx, hipMemcpyAsync(conf.data(), d_conf.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(tent.data(), d_tent.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const size_t row = static_cast<size_t>(st->c.max_chunk_frames) * S;
        for (size_t b = 0; b < B; ++b) {
            std::memcpy(confirmed + b * row, conf.data() + b * row, static_cast<size_t>(counts[2 * b]) * S * 4);
            std::memcpy(tentative + b * row, tent.data() + b * row, static_cast<size_t>(counts[2 * b + 1]) * S * 4);
        }
        return FA_SUCCESS;
    });
}

// ---- the chunk geometry: pure host
fa_status fa_sortformer_stream_chunk_plan(const fa_sortformer_stream_config *cfg, const int64_t *feat_frames, const int64_t *start_feat, int32_t streams, fa_sortformer_chunk *out) {
    sfs::Config c;
    if (!cfg || !feat_frames || !start_feat || !out || streams < 1 || sound_config(cfg, &c)[0]) return FA_INVALID_ARGUMENT;
    for (int32_t b = 0; b < streams; ++b)
        if (feat_frames[b] < 0 || start_feat[b] < 0 || feat_frames[b] > (int64_t{1} << 40) || start_feat[b] > (int64_t{1} << 40)) return FA_INVALID_ARGUMENT;
    for (int32_t b = 0; b < streams; ++b) {
        const sfs::Chunk k = sfs::stream_chunk(c, feat_frames[b], start_feat[b]);
        std::memcpy(&out[b], &k, sizeof(k));
    }
    return FA_SUCCESS;
}

fa_status fa_sortformer_stream_file_chunks(const fa_sortformer_stream_config *cfg, int64_t feat_length, int64_t feat_seq_length, fa_sortformer_chunk *chunks, int64_t capacity,
                                           int64_t *count, int64_t *num_chunks) {
    sfs::Config c;
    if (!cfg || !count || capacity < 0 || (capacity > 0 && !chunks) || feat_length < 0 || feat_seq_length < 0 || feat_length > (int64_t{1} << 40) ||
        feat_seq_length > (int64_t{1} << 40) || sound_config(cfg, &c)[0])
        return FA_INVALID_ARGUMENT;
    if (num_chunks) *num_chunks = sfs::file_num_chunks(c, feat_length);
    int64_t n = 0, start = 0;
    for (;;) {
        const sfs::Chunk k = sfs::file_chunk(c, feat_length, feat_seq_length, start);
        if (!k.ready) break;
        if (n < capacity) std::memcpy(&chunks[n], &k, sizeof(k));
        ++n;
        start = k.new_start_feat;
    }
    *count = n;
    return n > capacity ? FA_OUTPUT_TOO_SMALL : FA_SUCCESS;
}

fa_status fa_sortformer_stream_pack_chunks_dev(fa_ctx *ctx, const fa_sortformer_stream_config *cfg, const float *d_mel, const int64_t *stream_offsets,
                                               const fa_sortformer_chunk *chunks, int32_t streams, float *d_rows) {
    if (!ctx || !cfg) return FA_INVALID_ARGUMENT;
    sfs::Config c;
    const char *fault = sound_config(cfg, &c);
    if (fault[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream pack: %s", fault);
    if (!d_mel || !stream_offsets || !chunks || !d_rows || streams < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream pack: pointers, streams >= 1");
    const int64_t T = static_cast<int64_t>(c.chunk_len + c.chunk_left_context + c.chunk_right_context) * c.subsampling, row = T * c.n_mels;
    for (int32_t b = 0; b < streams; ++b)
        if (stream_offsets[b] < 0 || (chunks[b].ready && (chunks[b].start_frame < 0 || chunks[b].rows < 0 || chunks[b].rows > T)) || row > INT32_MAX)
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer_stream pack: stream %d: a chunk outside its buffer or longer than a row", b);
    fa::DeviceGuard guard(ctx->device);
    const bool wide = aligned16(d_rows) && row % 4 == 0;
    const auto fill = [&](fa::rows::Group &g, const int64_t b, const int32_t k) {   // a stream without a chunk: a row of zeros
        g.src[k] = chunks[b].ready ? (stream_offsets[b] + chunks[b].start_frame) * c.n_mels : 0;
        g.len[k] = chunks[b].ready ? static_cast<int32_t>(chunks[b].rows * c.n_mels) : 0;
    };
    fa::rows::for_each_group(streams, fill, [&](const fa::rows::Group &g, const int64_t b0) { sfs::launch_pack(ctx->stream, d_mel, g, row, d_rows + b0 * row, wide); });
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // extern "C"
