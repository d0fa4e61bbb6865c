// speaker_db_host.hip — the host unit of the online diarizer's speaker database (kernels and launchers: online.hip, through
// online_launch.h, which also declares the handle): the defaults, the arithmetic on its own, create and destroy, the argument checks and
// the C ABI of assign / distances / mergeable pairs on device arrays and on host arrays, and the management entries.
// Those take host pointers and wait for the context's stream; for_streams fetches a range of streams' slot scalars, runs one of
// speaker_db_core.h's edits on each and writes back what changed.  What an edit decides is decided there, in plain C++; here are the
// copies, and the rows of the embeddings an accepted edit moves.
#include "online_launch.h"

static_assert(sizeof(fa_speaker_db_config) == sizeof(fa::spk::Params), "fa_speaker_db_config is spk::Params");
static_assert(sizeof(fa_speaker_assignment) == sizeof(fa::spk::Record), "fa_speaker_assignment is spk::Record");
static_assert(sizeof(fa::spk::SlotMeta) == 40, "SlotMeta is 40 bytes");

namespace {

using fa::online::aligned16;
using fa::online::check_db;
using fa::spk::HostStream;
using fa::spk::SlotMeta;
constexpr int kDim = fa::spk::kDim;

float *current_row(const fa_speaker_db *db, const int32_t stream, const int slot) {
    return db->current.as<float>() + (static_cast<int64_t>(stream) * db->p.max_speakers + slot) * kDim;
}
float *raw_row(const fa_speaker_db *db, const int32_t stream, const int slot, const int r) {
    return db->raws.as<float>() + ((static_cast<int64_t>(stream) * db->p.max_speakers + slot) * db->p.raw_capacity + r) * kDim;
}

// edit(b, h, changed) on every stream of [stream, stream + 1), or of the whole database for stream == -1.  An edit that sets `changed`
// has its stream written back; one that returns another status than FA_SUCCESS (with its text set) ends the call there, nothing written.
template <class F> fa_status for_streams(fa_ctx *ctx, fa_speaker_db *db, const int32_t stream, const char *what, F &&edit) {
    FA_TRY(check_db(ctx, db, what));
    if (stream < -1 || stream >= db->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: stream %d of %d", what, stream, db->streams);
    return fa::no_throw(ctx, what, [&]() -> fa_status {   // one copy of the range's scalars each way, however many streams it spans
        fa::DeviceGuard guard(ctx->device);
        const int32_t lo = stream < 0 ? 0 : stream, hi = stream < 0 ? db->streams : stream + 1;
        const size_t S = static_cast<size_t>(db->p.max_speakers), n = static_cast<size_t>(hi - lo);
        std::vector<SlotMeta> meta(n * S);
        std::vector<int32_t> next(n);
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpy(meta.data(), db->meta.as<SlotMeta>() + static_cast<size_t>(lo) * S, sizeof(SlotMeta) * n * S, hipMemcpyDeviceToHost));
        FA_HIP_TRY(ctx, hipMemcpy(next.data(), db->next_id.as<int32_t>() + lo, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        bool any = false;
        HostStream h;
        for (int32_t b = lo; b < hi; ++b) {
            h.meta.assign(meta.begin() + static_cast<ptrdiff_t>((b - lo) * S), meta.begin() + static_cast<ptrdiff_t>((b - lo + 1) * S));
            h.next_id = next[static_cast<size_t>(b - lo)];
            bool changed = false;
            FA_TRY(edit(b, h, changed));
            if (!changed) continue;
            std::copy(h.meta.begin(), h.meta.end(), meta.begin() + static_cast<ptrdiff_t>((b - lo) * S));
            next[static_cast<size_t>(b - lo)] = h.next_id;
            any = true;
        }
        if (any) {
            FA_HIP_TRY(ctx, hipMemcpy(db->meta.as<SlotMeta>() + static_cast<size_t>(lo) * S, meta.data(), sizeof(SlotMeta) * n * S, hipMemcpyHostToDevice));
            FA_HIP_TRY(ctx, hipMemcpy(db->next_id.as<int32_t>() + lo, next.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
        }
        return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_speaker_db_default_config(fa_speaker_db_config *c) {
    if (!c) return;   // SpeakerManager.init's defaults (SpeakerManager.swift:45-50), the ring of SpeakerTypes.swift:111, alpha of SpeakerManager.swift:452; plain SpeakerManager: no validation
    c->speaker_threshold = 0.65f; c->embedding_threshold = 0.45f; c->min_speech_duration = 1.0f; c->ema_alpha = 0.9f; c->validate_min_magnitude = -1.0f;
    c->max_speakers = 16; c->raw_capacity = 50;
}

// The arithmetic on its own (VDSPOperations.l2Normalize, SpeakerUtilities.cosineDistance / validateEmbedding): no context, no device.
fa_status fa_speaker_l2_normalize(const float *embedding, float *out) {
    if (!embedding || !out) return FA_INVALID_ARGUMENT;
    fa::spk::l2_normalize(fa::spk::Vec256::load(embedding)).store(out);
    return FA_SUCCESS;
}

float fa_speaker_cosine_distance(const float *a, const float *b) {
    if (!a || !b) return fa::spk::inf32();
    const fa::spk::Vec256 x = fa::spk::Vec256::load(a), y = fa::spk::Vec256::load(b);
    return fa::spk::cosine_from_sums(fa::spk::Vec256::dot(x, y), fa::spk::sumsq(x), fa::spk::sumsq(y));
}

int32_t fa_speaker_validate_embedding(const float *embedding, float min_magnitude) {
    if (!embedding) return 0;
    const fa::spk::Vec256 e = fa::spk::Vec256::load(embedding);
    return sqrtf(fa::spk::sumsq(e)) > min_magnitude && e.finite() ? 1 : 0;
}

fa_status fa_speaker_db_create(fa_ctx *ctx, const fa_speaker_db_config *cfg, int32_t streams, fa_speaker_db **out) {
    if (!ctx || !cfg || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    if (streams <= 0 || cfg->max_speakers < 1 || cfg->max_speakers > fa::spk::kMaxSpeakers || cfg->raw_capacity < 1)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db: streams >= 1, 1 <= max_speakers <= %d, raw_capacity >= 1", fa::spk::kMaxSpeakers);
    return fa::no_throw(ctx, "fa_speaker_db_create", [&]() {
        fa::DeviceGuard guard(ctx->device);
        fa_speaker_db *db = new fa_speaker_db;
        db->device = ctx->device; db->streams = streams;
        std::memcpy(&db->p, cfg, sizeof(db->p));
        const size_t slots = static_cast<size_t>(streams) * cfg->max_speakers;
        const std::vector<int32_t> ones(static_cast<size_t>(streams), 1);
        fa_status st = fa::take_once(ctx, "fa_speaker_db_create", {{&db->current, slots * kDim * sizeof(float)},
                                                                   {&db->raws, slots * cfg->raw_capacity * kDim * sizeof(float)},
                                                                   {&db->meta, slots * sizeof(SlotMeta)},
                                                                   {&db->next_id, ones.size() * sizeof(int32_t), true, ones.data()}});
        if (st == FA_SUCCESS) st = fa::hip_status(ctx, hipMemsetAsync(db->current.p, 0, slots * kDim * sizeof(float), ctx->stream), "speaker_db: clear");
        if (st == FA_SUCCESS) st = fa::hip_status(ctx, hipMemsetAsync(db->raws.p, 0, slots * cfg->raw_capacity * kDim * sizeof(float), ctx->stream), "speaker_db: clear");
        if (st == FA_SUCCESS) st = fa::hip_status(ctx, hipMemsetAsync(db->meta.p, 0, slots * sizeof(SlotMeta), ctx->stream), "speaker_db: clear");
        if (st == FA_SUCCESS) st = fa::hip_status(ctx, hipStreamSynchronize(ctx->stream), "speaker_db: clear");
        if (st != FA_SUCCESS) { delete db; return st; }
        *out = db;
        return FA_SUCCESS;
    });
}

void fa_speaker_db_destroy(fa_speaker_db *db) {
    if (!db) return;
    fa::DeviceGuard guard(db->device);
    delete db;
}

fa_status fa_speaker_db_assign_dev(fa_ctx *ctx, fa_speaker_db *db, const float *d_embeddings, const float *d_durations, const int32_t *d_skip,
                                   int32_t per, int64_t tick, fa_speaker_assignment *d_out) {
    FA_TRY(check_db(ctx, db, "fa_speaker_db_assign_dev"));
    if (!d_embeddings || !d_durations || !d_out || per <= 0 || !aligned16(d_embeddings))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db assign: embeddings (16-byte aligned), durations and records, per >= 1");
    fa::DeviceGuard guard(ctx->device);
    fa::online::AssignArgs a{db->arrays(), db->p, d_embeddings, d_durations, d_skip, per, tick, reinterpret_cast<fa::spk::Record *>(d_out)};
    fa::online::launch_assign(ctx->stream, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_speaker_db_distances_dev(fa_ctx *ctx, fa_speaker_db *db, const float *d_queries, int32_t per, float *d_dist, int32_t *d_best_slot) {
    FA_TRY(check_db(ctx, db, "fa_speaker_db_distances_dev"));
    if (!d_queries || !d_dist || per <= 0 || !aligned16(d_queries))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db distances: queries (16-byte aligned) and distances, per >= 1");
    fa::DeviceGuard guard(ctx->device);
    fa::online::launch_distances(ctx->stream, fa::online::DistanceArgs{db->arrays(), d_queries, per, d_dist, d_best_slot});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_speaker_db_mergeable_pairs_dev(fa_ctx *ctx, fa_speaker_db *db, float threshold, int32_t exclude_if_both_permanent,
                                            fa_speaker_pair *d_pairs, int32_t capacity, int32_t *d_counts) {
    FA_TRY(check_db(ctx, db, "fa_speaker_db_mergeable_pairs_dev"));
    if (!d_counts || capacity < 0 || (capacity > 0 && !d_pairs))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db mergeable pairs: counts, and records for a capacity above 0");
    fa::DeviceGuard guard(ctx->device);
    fa::online::launch_pairs(ctx->stream, fa::online::PairArgs{db->arrays(), threshold, exclude_if_both_permanent, d_pairs, capacity, d_counts});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

/* the three above on HOST arrays: copied to the device, run, copied back, one synchronisation */
fa_status fa_speaker_db_assign(fa_ctx *ctx, fa_speaker_db *db, const float *embeddings, const float *durations, const int32_t *skip, int32_t per,
                               int64_t tick, fa_speaker_assignment *out) {
    FA_TRY(check_db(ctx, db, "fa_speaker_db_assign"));
    if (!embeddings || !durations || !out || per <= 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db assign: embeddings, durations and records, per >= 1");
    return fa::no_throw(ctx, "fa_speaker_db_assign", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t n = static_cast<size_t>(db->streams) * per;
        fa::DevBuf d_emb, d_dur, d_skip, d_out;
        FA_TRY(fa::take(ctx, "fa_speaker_db_assign", {{&d_emb, n * kDim * sizeof(float), true, embeddings}, {&d_dur, n * sizeof(float), true, durations},
                                                       {&d_skip, n * sizeof(int32_t), skip != nullptr, skip}, {&d_out, n * sizeof(fa_speaker_assignment)}}));
        FA_TRY(fa_speaker_db_assign_dev(ctx, db, d_emb.as<float>(), d_dur.as<float>(), skip ? d_skip.as<int32_t>() : nullptr, per, tick, d_out.as<fa_speaker_assignment>()));
        FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, n * sizeof(fa_speaker_assignment), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_speaker_db_distances(fa_ctx *ctx, fa_speaker_db *db, const float *queries, int32_t per, float *dist, int32_t *best_slot) {
    FA_TRY(check_db(ctx, db, "fa_speaker_db_distances"));
    if (!queries || !dist || per <= 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db distances: queries and distances, per >= 1");
    return fa::no_throw(ctx, "fa_speaker_db_distances", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t n = static_cast<size_t>(db->streams) * per;
        fa::DevBuf d_q, d_dist, d_best;
        FA_TRY(fa::take(ctx, "fa_speaker_db_distances", {{&d_q, n * kDim * sizeof(float), true, queries}, {&d_dist, n * db->p.max_speakers * sizeof(float)},
                                                          {&d_best, n * sizeof(int32_t)}}));
        FA_TRY(fa_speaker_db_distances_dev(ctx, db, d_q.as<float>(), per, d_dist.as<float>(), d_best.as<int32_t>()));
        FA_HIP_TRY(ctx, hipMemcpyAsync(dist, d_dist.p, n * db->p.max_speakers * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (best_slot) FA_HIP_TRY(ctx, hipMemcpyAsync(best_slot, d_best.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_speaker_db_mergeable_pairs(fa_ctx *ctx, fa_speaker_db *db, float threshold, int32_t exclude_if_both_permanent, fa_speaker_pair *pairs,
                                        int32_t capacity, int32_t *counts) {
    FA_TRY(check_db(ctx, db, "fa_speaker_db_mergeable_pairs"));
    if (!counts || capacity < 0 || (capacity > 0 && !pairs)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db mergeable pairs: counts, and records for a capacity above 0");
    return fa::no_throw(ctx, "fa_speaker_db_mergeable_pairs", [&]() {
        fa::DeviceGuard guard(ctx->device);
        const size_t n = static_cast<size_t>(db->streams);
        fa::DevBuf d_pairs, d_counts;
        FA_TRY(fa::take(ctx, "fa_speaker_db_mergeable_pairs", {{&d_pairs, n * capacity * sizeof(fa_speaker_pair)}, {&d_counts, n * sizeof(int32_t)}}));
        FA_TRY(fa_speaker_db_mergeable_pairs_dev(ctx, db, threshold, exclude_if_both_permanent, d_pairs.as<fa_speaker_pair>(), capacity, d_counts.as<int32_t>()));
        if (capacity > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(pairs, d_pairs.p, n * capacity * sizeof(fa_speaker_pair), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_speaker_db_upsert(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, const fa_speaker_info *info, const float *current, const float *raws) {
    if (!info || !current || stream < 0 || info->id < 1 || info->raw_count < 0 || (info->raw_count > 0 && !raws))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db upsert: a stream, an id >= 1, a current embedding, 0 <= raw_count <= raw_capacity rows");
    return for_streams(ctx, db, stream, "fa_speaker_db_upsert", [&](const int32_t b, HostStream &h, bool &changed) -> fa_status {
        const fa::spk::Upsert u = fa::spk::upsert_edit(h, *info, db->p.raw_capacity, b);   // behind check_db: db is known to be there
        if (u.verdict.status != FA_SUCCESS) return fa::set_error(ctx, u.verdict.status, "%s", u.verdict.text);
        fa::spk::Vec256 cur = fa::spk::Vec256::load(current);
        if (u.normalise) cur = fa::spk::l2_normalize(cur);
        if (hipMemcpy(current_row(db, b, u.slot), cur.v, sizeof(cur.v), hipMemcpyHostToDevice) != hipSuccess ||
            (info->raw_count > 0 && hipMemcpy(raw_row(db, b, u.slot, 0), raws, sizeof(float) * kDim * info->raw_count, hipMemcpyHostToDevice) != hipSuccess))
            return fa::set_error(ctx, FA_RUNTIME_ERROR, "speaker_db upsert: copying the rows failed");
        changed = true;
        return FA_SUCCESS;
    });
}

fa_status fa_speaker_db_get(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, fa_speaker_info *info, float *current, float *raws,
                            int32_t raw_rows) {
    if (!info || stream < 0 || raw_rows < 0 || (raw_rows > 0 && !raws)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db get: a stream, a record, rows for raw_rows above 0");
    return for_streams(ctx, db, stream, "fa_speaker_db_get", [&](const int32_t b, HostStream &h, bool &) -> fa_status {
        const int slot = fa::spk::get_edit(h, id, info);
        if (slot < 0) return FA_SUCCESS;
        const SlotMeta &m = h.meta[slot];
        bool copied = !current || hipMemcpy(current, current_row(db, b, slot), sizeof(float) * kDim, hipMemcpyDeviceToHost) == hipSuccess;
        for (int k = 0; raws && k < m.count && k < raw_rows; ++k)   // oldest first
            copied &= hipMemcpy(raws + static_cast<int64_t>(k) * kDim, raw_row(db, b, slot, (m.head + k) % db->p.raw_capacity), sizeof(float) * kDim, hipMemcpyDeviceToHost) == hipSuccess;
        return copied ? FA_SUCCESS : fa::set_error(ctx, FA_RUNTIME_ERROR, "speaker_db get: copying the rows failed");
    });
}

fa_status fa_speaker_db_ids(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t *ids, int32_t *count) {
    if (!ids || !count || stream < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db ids: a stream, max_speakers ids and a count");
    return for_streams(ctx, db, stream, "fa_speaker_db_ids", [&](int32_t, HostStream &h, bool &) { *count = fa::spk::ids(h, ids); return FA_SUCCESS; });
}

fa_status fa_speaker_db_count(fa_ctx *ctx, fa_speaker_db *db, int32_t *counts) {
    if (!counts) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db count: one count per stream");
    return for_streams(ctx, db, -1, "fa_speaker_db_count", [&](const int32_t b, HostStream &h, bool &) { counts[b] = fa::spk::count(h); return FA_SUCCESS; });
}

fa_status fa_speaker_db_remove(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, int32_t keep_if_permanent) {
    if (stream < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db remove: a stream");
    return for_streams(ctx, db, stream, "fa_speaker_db_remove", [&](int32_t, HostStream &h, bool &changed) { changed = fa::spk::remove(h, id, keep_if_permanent != 0); return FA_SUCCESS; });
}

fa_status fa_speaker_db_remove_inactive(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int64_t since_tick, int32_t keep_if_permanent) {
    return for_streams(ctx, db, stream, "fa_speaker_db_remove_inactive",
                       [&](int32_t, HostStream &h, bool &changed) { changed = fa::spk::remove_inactive(h, since_tick, keep_if_permanent != 0); return FA_SUCCESS; });
}

fa_status fa_speaker_db_set_permanent(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, int32_t permanent) {
    if (stream < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db set_permanent: a stream");
    return for_streams(ctx, db, stream, "fa_speaker_db_set_permanent", [&](int32_t, HostStream &h, bool &changed) { changed = fa::spk::set_permanent(h, id, permanent != 0); return FA_SUCCESS; });
}

fa_status fa_speaker_db_reset(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t keep_if_permanent) {
    return for_streams(ctx, db, stream, "fa_speaker_db_reset", [&](int32_t, HostStream &h, bool &changed) { changed = fa::spk::reset(h, keep_if_permanent != 0); return FA_SUCCESS; });
}

}  // extern "C"
