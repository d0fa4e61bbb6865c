// online_host.hip — the host side of the online diarizer (kernels and launchers: online.hip, through online_launch.h): at the end the entries
// around the networks (fa_online_chunk_plan, fa_online_pack_waveforms_dev, fa_online_chunk_finish_dev); before them the speaker database:
// the handle and its device arrays, the defaults, the argument checks and the C ABI of assign / distances / mergeable pairs, and the
// management entries (upsertSpeaker, getSpeaker, removeSpeaker, removeSpeakersInactive, makeSpeakerPermanent / revokePermanence, reset,
// speakerCount: SpeakerManager.swift:223-242, 334-367, 500-628).  Those take host pointers, wait for the context's stream, and edit one
// stream's slot scalars on the host with the arithmetic of speaker_db_core.h (Vec256: the same bits as the kernels').
#include "online_launch.h"

struct fa_speaker_db {
    int device = 0;
    fa::spk::Params p{};
    int32_t streams = 0;
    fa::DevBuf current, raws, meta, next_id;
    fa::online::DbArrays arrays() const {
        return fa::online::DbArrays{current.as<float>(), raws.as<float>(), meta.as<fa::spk::SlotMeta>(), next_id.as<int32_t>(), streams, p.max_speakers, p.raw_capacity};
    }
};

static_assert(sizeof(fa_speaker_db_config) == sizeof(fa::spk::Params), "fa_speaker_db_config is spk::Params");
static_assert(sizeof(fa_speaker_assignment) == sizeof(fa::spk::Record), "fa_speaker_assignment is spk::Record");
static_assert(sizeof(fa::spk::SlotMeta) == 40, "SlotMeta is 40 bytes");

namespace {

using fa::spk::SlotMeta;
constexpr int kDim = fa::spk::kDim;

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

fa_status check_db(fa_ctx *ctx, const fa_speaker_db *db, const char *what) {
    if (!ctx || !db) return FA_INVALID_ARGUMENT;
    if (db->device != ctx->device) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: the database lives on another device than the context", what);
    return FA_SUCCESS;
}

// One stream's slot scalars on the host: fetched behind the stream's work (for_streams), edited, written back.
struct HostStream {
    std::vector<SlotMeta> meta;
    int32_t next_id = 1;
    int find(const int32_t id) const {
        for (size_t s = 0; s < meta.size(); ++s)
            if ((meta[s].flags & fa::spk::kLive) && meta[s].id == id) return static_cast<int>(s);
        return -1;
    }
    int lowest_free() const {
        for (size_t s = 0; s < meta.size(); ++s)
            if (!(meta[s].flags & fa::spk::kLive)) return static_cast<int>(s);
        return -1;
    }
};

float *current_row(const fa_speaker_db *db, const int32_t stream, const int slot) {
    return db->current.as<float>() + (static_cast<int64_t>(stream) * db->p.max_speakers + slot) * kDim;
}
float *raw_row(const fa_speaker_db *db, const int32_t stream, const int slot, const int r) {
    return db->raws.as<float>() + ((static_cast<int64_t>(stream) * db->p.max_speakers + slot) * db->p.raw_capacity + r) * kDim;
}

// `edit` on every stream of [stream, stream + 1), or of the whole database for stream == -1
template <class F> fa_status for_streams(fa_ctx *ctx, fa_speaker_db *db, const int32_t stream, const char *what, F &&edit) {
    FA_TRY(check_db(ctx, db, what));
    if (stream < -1 || stream >= db->streams) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: stream %d of %d", what, stream, db->streams);
    return fa::no_throw(ctx, what, [&]() {   // one copy of the range's scalars each way, however many streams it spans
        fa::DeviceGuard guard(ctx->device);
        const int32_t lo = stream < 0 ? 0 : stream, hi = stream < 0 ? db->streams : stream + 1;
        const size_t S = static_cast<size_t>(db->p.max_speakers), n = static_cast<size_t>(hi - lo);
        std::vector<SlotMeta> meta(n * S);
        std::vector<int32_t> next(n);
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpy(meta.data(), db->meta.as<SlotMeta>() + static_cast<size_t>(lo) * S, sizeof(SlotMeta) * n * S, hipMemcpyDeviceToHost));
        FA_HIP_TRY(ctx, hipMemcpy(next.data(), db->next_id.as<int32_t>() + lo, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        bool changed = false;
        HostStream h;
        for (int32_t b = lo; b < hi; ++b) {
            h.meta.assign(meta.begin() + static_cast<ptrdiff_t>((b - lo) * S), meta.begin() + static_cast<ptrdiff_t>((b - lo + 1) * S));
            h.next_id = next[static_cast<size_t>(b - lo)];
            if (!edit(b, h)) continue;
            std::copy(h.meta.begin(), h.meta.end(), meta.begin() + static_cast<ptrdiff_t>((b - lo) * S));
            next[static_cast<size_t>(b - lo)] = h.next_id;
            changed = true;
        }
        if (changed) {
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
    fa_status found = FA_SUCCESS;
    FA_TRY(for_streams(ctx, db, stream, "fa_speaker_db_upsert", [&](const int32_t b, HostStream &h) {
        if (info->raw_count > db->p.raw_capacity) { found = FA_INVALID_ARGUMENT; return false; }   // behind check_db: db is known to be there
        int slot = h.find(info->id);
        fa::spk::Vec256 cur = fa::spk::Vec256::load(current);
        if (slot >= 0) {   // :565-580: the fields as given, createdAt kept, permanence only ever set
            SlotMeta &m = h.meta[slot];
            m.duration = info->duration; m.updates = info->update_count; m.updated = info->updated_tick;
            if (info->is_permanent) m.flags |= fa::spk::kPermanent;
        } else {           // :582-602: Speaker.init normalises
            slot = h.lowest_free();
            if (slot < 0) { found = FA_OUTPUT_TOO_SMALL; return false; }
            cur = fa::spk::l2_normalize(cur);
            h.meta[slot] = fa::spk::fresh_meta(info->id, info->duration, info->created_tick, info->updated_tick, info->is_permanent != 0);
            h.meta[slot].updates = info->update_count;
            h.next_id = h.next_id > info->id + 1 ? h.next_id : info->id + 1;
        }
        h.meta[slot].head = 0; h.meta[slot].count = info->raw_count;
        if (hipMemcpy(current_row(db, b, slot), cur.v, sizeof(cur.v), hipMemcpyHostToDevice) != hipSuccess ||
            (info->raw_count > 0 && hipMemcpy(raw_row(db, b, slot, 0), raws, sizeof(float) * kDim * info->raw_count, hipMemcpyHostToDevice) != hipSuccess)) {
            found = FA_RUNTIME_ERROR;
            return false;
        }
        return true;
    }));
    if (found == FA_INVALID_ARGUMENT) return fa::set_error(ctx, found, "speaker_db upsert: more raw embeddings than raw_capacity");
    if (found == FA_OUTPUT_TOO_SMALL) return fa::set_error(ctx, found, "speaker_db upsert: no free slot in stream %d", stream);
    if (found != FA_SUCCESS) return fa::set_error(ctx, found, "speaker_db upsert: copying the rows failed");
    return FA_SUCCESS;
}

fa_status fa_speaker_db_get(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, fa_speaker_info *info, float *current, float *raws,
                            int32_t raw_rows) {
    if (!info || stream < 0 || raw_rows < 0 || (raw_rows > 0 && !raws)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db get: a stream, a record, rows for raw_rows above 0");
    fa_status copied = FA_SUCCESS;
    FA_TRY(for_streams(ctx, db, stream, "fa_speaker_db_get", [&](const int32_t b, HostStream &h) {
        std::memset(info, 0, sizeof(*info));
        info->slot = -1;
        const int slot = h.find(id);
        if (slot < 0) return false;
        const SlotMeta &m = h.meta[slot];
        info->id = m.id; info->slot = slot; info->raw_count = m.count; info->update_count = m.updates; info->is_permanent = (m.flags & fa::spk::kPermanent) ? 1 : 0;
        info->duration = m.duration; info->created_tick = m.created; info->updated_tick = m.updated;
        if (current && hipMemcpy(current, current_row(db, b, slot), sizeof(float) * kDim, hipMemcpyDeviceToHost) != hipSuccess) copied = FA_RUNTIME_ERROR;
        for (int k = 0; raws && k < m.count && k < raw_rows; ++k)   // oldest first
            if (hipMemcpy(raws + static_cast<int64_t>(k) * kDim, raw_row(db, b, slot, (m.head + k) % db->p.raw_capacity), sizeof(float) * kDim, hipMemcpyDeviceToHost) != hipSuccess)
                copied = FA_RUNTIME_ERROR;
        return false;
    }));
    if (copied != FA_SUCCESS) return fa::set_error(ctx, copied, "speaker_db get: copying the rows failed");
    return FA_SUCCESS;
}

fa_status fa_speaker_db_ids(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t *ids, int32_t *count) {
    if (!ids || !count || stream < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db ids: a stream, max_speakers ids and a count");
    return for_streams(ctx, db, stream, "fa_speaker_db_ids", [&](int32_t, HostStream &h) {
        *count = 0;
        for (const SlotMeta &m : h.meta)
            if (m.flags & fa::spk::kLive) ids[(*count)++] = m.id;
        return false;
    });
}

fa_status fa_speaker_db_count(fa_ctx *ctx, fa_speaker_db *db, int32_t *counts) {
    if (!counts) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db count: one count per stream");
    return for_streams(ctx, db, -1, "fa_speaker_db_count", [&](const int32_t b, HostStream &h) {
        counts[b] = 0;
        for (const SlotMeta &m : h.meta) counts[b] += (m.flags & fa::spk::kLive) ? 1 : 0;
        return false;
    });
}

fa_status fa_speaker_db_remove(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, int32_t keep_if_permanent) {
    if (stream < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db remove: a stream");
    return for_streams(ctx, db, stream, "fa_speaker_db_remove", [&](int32_t, HostStream &h) {
        const int slot = h.find(id);
        if (slot < 0 || (keep_if_permanent && (h.meta[slot].flags & fa::spk::kPermanent))) return false;
        h.meta[slot] = SlotMeta{};
        return true;
    });
}

fa_status fa_speaker_db_remove_inactive(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int64_t since_tick, int32_t keep_if_permanent) {
    return for_streams(ctx, db, stream, "fa_speaker_db_remove_inactive", [&](int32_t, HostStream &h) {
        bool changed = false;
        for (SlotMeta &m : h.meta)
            if ((m.flags & fa::spk::kLive) && m.updated < since_tick && !(keep_if_permanent && (m.flags & fa::spk::kPermanent))) { m = SlotMeta{}; changed = true; }
        return changed;
    });
}

fa_status fa_speaker_db_set_permanent(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, int32_t permanent) {
    if (stream < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "speaker_db set_permanent: a stream");
    return for_streams(ctx, db, stream, "fa_speaker_db_set_permanent", [&](int32_t, HostStream &h) {
        const int slot = h.find(id);
        if (slot < 0) return false;
        h.meta[slot].flags = fa::spk::kLive | (permanent ? fa::spk::kPermanent : 0);
        return true;
    });
}

fa_status fa_speaker_db_reset(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t keep_if_permanent) {
    return for_streams(ctx, db, stream, "fa_speaker_db_reset", [&](int32_t, HostStream &h) {
        int32_t max_id = 0;   // :610-628
        for (SlotMeta &m : h.meta) {
            if (keep_if_permanent && (m.flags & fa::spk::kLive) && (m.flags & fa::spk::kPermanent)) max_id = m.id > max_id ? m.id : max_id;
            else m = SlotMeta{};
        }
        h.next_id = max_id + 1;
        return true;
    });
}

// ---- around the networks
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
