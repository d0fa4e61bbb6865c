// speaker_db_core.h — the arithmetic and the state layout of the online speaker database (SpeakerManager.swift:135-212, 411-492,
// SpeakerTypes.swift:36-162, 213-217, SpeakerOperations.swift:62-126, VDSPOperations.swift:12-23) that the host and the kernels of
// online.hip share, and at the end the management edits of one stream's slot scalars (upsertSpeaker, getSpeaker, removeSpeaker,
// removeSpeakersInactive, makeSpeakerPermanent / revokePermanence, reset, speakerCount: SpeakerManager.swift:223-242, 334-367, 500-628),
// which speaker_db_host.hip runs between a fetch and a write-back.  Plain C++ in its host half: no HIP type is named unless hipcc
// compiles it; tests/cpu/speaker_db_core_main.cpp walks it under the sanitizers.
//
// The fp32 arithmetic is THIS library's definition.  vDSP_dotpr / vDSP_svesq specify no summation order, so Accelerate's bits are out of
// reach and a decision within an ulp of a threshold may differ from a Mac.  Defined here, and used by everything of this feature:
//   dot256(a, b)  lane l of 64 holds dimensions 4l .. 4l+3; its partial is ((a0 b0 + a1 b1) + a2 b2) + a3 b3, every product and sum rounded
//                 on its own (no FMA: the units that include this header are built with -ffp-contract=off); then six butterfly steps with
//                 lane offsets 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l ^ off].  Addition commutes, so every lane ends with the same bits.
//   sumsq(a)      dot256(a, a)
//   l2Normalize   norm = max(sqrtf(sumsq), 1e-12f), scale = 1 / norm, out = a * scale
//   cosine        SpeakerOperations.swift:62-101 on those sums
//   mean of raws  the reference's own loop: per dimension a sequential fp32 sum from the oldest raw to the newest from 0.0f, then / Float(count)
// The algorithm is written once, over a vector type V: Vec256 below (the host: an array of 256 floats, the tree on a 64-element array) or
// the kernels' lane vector (online.hip: four floats per lane, the butterfly by cross-lane reads).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fa_verdict.h"

#if defined(__HIPCC__)
#define FA_SPK_HD __host__ __device__
#define FA_SPK_UNROLL _Pragma("unroll")
#else
#define FA_SPK_HD
#define FA_SPK_UNROLL
#endif

namespace fa {
namespace spk {

constexpr int kDim = 256;     // SpeakerManager.embeddingSize
constexpr int kLanes = 64;
constexpr int kMaxSpeakers = 64;
constexpr int kInFlight = 4;   // rows requested together by the search and by the re-average

enum Kind : int32_t { kSkipped = 0, kUpdated = 1, kDurationOnly = 2, kLowEnergy = 3, kCreated = 4, kTooShort = 5, kInvalid = 6, kFull = 7 };
enum Flags : int32_t { kLive = 1, kPermanent = 2 };

struct Params {
    float speaker_threshold, embedding_threshold, min_speech_duration, ema_alpha, validate_min_magnitude;
    int32_t max_speakers, raw_capacity;
};

// One slot's scalars.  head: the ring index of the OLDEST raw; count raws follow it.
struct SlotMeta {
    int32_t id, flags, head, count, updates;
    float duration;
    int64_t created, updated;
};

struct Record {   // fa_speaker_assignment
    int32_t id, slot, kind;
    float distance;
};

// One stream's part of the database.
struct View {
    float *current;     // [max_speakers][256]
    float *raws;        // [max_speakers][raw_capacity][256]
    SlotMeta *meta;     // [max_speakers]
    int32_t *next_id;   // [1]
    int32_t S, R;
    uint64_t live;      // bit s: slot s holds a speaker (meta[s].flags & kLive), kept in step by everything below
    FA_SPK_HD float *cur(int s) const { return current + static_cast<int64_t>(s) * kDim; }
    FA_SPK_HD float *raw(int s, int r) const { return raws + (static_cast<int64_t>(s) * R + r) * kDim; }
};

FA_SPK_HD inline float inf32() { return __builtin_huge_valf(); }

// The four dimensions of one lane.
FA_SPK_HD inline float partial4(const float a0, const float a1, const float a2, const float a3, const float b0, const float b1, const float b2,
                                const float b3) {
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

// The scale of l2Normalize for a sum of squares.
FA_SPK_HD inline float norm_scale(const float ss) {
    const float root = sqrtf(ss);
    const float norm = 1e-12f >= root ? 1e-12f : root;   // Swift's max(x, y) is y >= x ? y : x
    return 1.0f / norm;
}

// SpeakerUtilities.cosineDistance (:62-101) from the three sums.  Swift's min / max keep a NaN first operand.
FA_SPK_HD inline float cosine_from_sums(const float dot, const float ssa, const float ssb, int *non_unit = nullptr) {
    if (!(ssa > 0.0f && ssb > 0.0f)) return inf32();
    const bool unit_a = fabsf(ssa - 1.0f) <= 1e-3f, unit_b = fabsf(ssb - 1.0f) <= 1e-3f;
    float sim;
    if (unit_a && unit_b) {
        sim = dot;
    } else {
        if (non_unit) *non_unit += 1;
        const float ma = sqrtf(ssa), mb = sqrtf(ssb);
        if (!(ma > 0.0f && mb > 0.0f)) return inf32();
        sim = dot / (ma * mb);
    }
    const float lo = -1.0f >= sim ? -1.0f : sim;   // max(similarity, -1.0)
    const float cl = 1.0f < lo ? 1.0f : lo;        // min(.., 1.0)
    return 1.0f - cl;
}

// ---- the host's vector: 256 floats, dot256 as the tree on a 64-element array
struct Vec256 {
    float v[kDim];
    static Vec256 load(const float *p) { Vec256 r; for (int i = 0; i < kDim; ++i) r.v[i] = p[i]; return r; }
    void store(float *p) const { for (int i = 0; i < kDim; ++i) p[i] = v[i]; }
    static Vec256 zero() { Vec256 r; for (int i = 0; i < kDim; ++i) r.v[i] = 0.0f; return r; }
    static float dot(const Vec256 &a, const Vec256 &b) {
        float p[kLanes], q[kLanes];
        for (int l = 0; l < kLanes; ++l)
            p[l] = partial4(a.v[4 * l], a.v[4 * l + 1], a.v[4 * l + 2], a.v[4 * l + 3], b.v[4 * l], b.v[4 * l + 1], b.v[4 * l + 2], b.v[4 * l + 3]);
        for (int off = 32; off >= 1; off >>= 1) {
            for (int l = 0; l < kLanes; ++l) q[l] = p[l] + p[l ^ off];
            for (int l = 0; l < kLanes; ++l) p[l] = q[l];
        }
        return p[0];
    }
    Vec256 scaled(const float s) const { Vec256 r; for (int i = 0; i < kDim; ++i) r.v[i] = v[i] * s; return r; }
    Vec256 plus(const Vec256 &o) const { Vec256 r; for (int i = 0; i < kDim; ++i) r.v[i] = v[i] + o.v[i]; return r; }
    Vec256 over(const float d) const { Vec256 r; for (int i = 0; i < kDim; ++i) r.v[i] = v[i] / d; return r; }
    static Vec256 blend(const float a, const Vec256 &x, const float b, const Vec256 &y) {   // a x + b y, the products rounded before the sum
        Vec256 r;
        for (int i = 0; i < kDim; ++i) r.v[i] = a * x.v[i] + b * y.v[i];
        return r;
    }
    bool finite() const { for (int i = 0; i < kDim; ++i) if (!std::isfinite(v[i])) return false; return true; }
};

template <class V> FA_SPK_HD inline float sumsq(const V &a) { return V::dot(a, a); }
template <class V> FA_SPK_HD inline V l2_normalize(const V &a) { return a.scaled(norm_scale(sumsq(a))); }

// Speaker.recalculateMainEmbedding (:132-162): the mean of the ring, oldest first, normalised; the tick is set.
template <class V> FA_SPK_HD inline void recalculate(const View &db, const int slot, SlotMeta &m, const int64_t tick) {
    if (m.count <= 0) return;
    V avg = V::zero();
    int r = m.head;
    for (int k = 0; k < m.count; k += kInFlight) {   // the rows' loads go out together; the sum stays sequential, oldest first
        V row[kInFlight];
FA_SPK_UNROLL
        for (int u = 0; u < kInFlight; ++u) {
            if (k + u < m.count) row[u] = V::load(db.raw(slot, r));
            r = r + 1 == db.R ? 0 : r + 1;
        }
FA_SPK_UNROLL
        for (int u = 0; u < kInFlight; ++u)
            if (k + u < m.count) avg = avg.plus(row[u]);
    }
    avg = avg.over(static_cast<float>(m.count));
    l2_normalize(avg).store(db.cur(slot));
    m.updated = tick;
}

// Speaker.addRawEmbedding (:104-117) of an already normalised raw (RawEmbedding.init): its own energy check, the FIFO, the recalculation.
template <class V> FA_SPK_HD inline bool add_raw(const View &db, const int slot, SlotMeta &m, const V &raw, const int64_t tick) {
    if (!(sumsq(raw) > 0.01f)) return false;
    if (m.count >= db.R) {   // removeFirst
        m.head = m.head + 1 == db.R ? 0 : m.head + 1;
        m.count -= 1;
    }
    int at = m.head + m.count;
    if (at >= db.R) at -= db.R;
    raw.store(db.raw(slot, at));
    m.count += 1;
    recalculate<V>(db, slot, m, tick);
    return true;
}

// Speaker.updateMainEmbedding (:68-101) with n the embedding assignSpeaker normalised.
template <class V> FA_SPK_HD inline void update_main(const View &db, const int slot, SlotMeta &m, const V &n, const float duration, const float alpha,
                                                     const int64_t tick) {
    if (!(sumsq(n) > 0.01f)) return;
    const V nm = l2_normalize(n);
    add_raw<V>(db, slot, m, l2_normalize(nm), tick);   // RawEmbedding.init normalises again
    const V blended = V::blend(alpha, V::load(db.cur(slot)), 1.0f - alpha, nm);
    l2_normalize(blended).store(db.cur(slot));
    m.duration += duration;
    m.updated = tick;
    m.updates += 1;
}

// Speaker.init + upsert's / createNewSpeaker's fields in a free slot.
FA_SPK_HD inline SlotMeta fresh_meta(const int32_t id, const float duration, const int64_t created, const int64_t updated, const bool permanent) {
    SlotMeta m;
    m.id = id; m.flags = kLive | (permanent ? kPermanent : 0); m.head = 0; m.count = 0; m.updates = 1; m.duration = duration;
    m.created = created; m.updated = updated;
    return m;
}

FA_SPK_HD inline uint64_t live_mask(const SlotMeta *meta, const int S) {
    uint64_t live = 0;
    for (int s = 0; s < S; ++s)
        if (meta[s].flags & kLive) live |= 1ull << s;
    return live;
}

FA_SPK_HD inline int lowest_free_slot(const View &db) {
    const uint64_t free_slots = ~db.live & (db.S >= 64 ? ~0ull : (1ull << db.S) - 1);
    return free_slots ? __builtin_ctzll(free_slots) : -1;
}

// findClosestSpeaker (:417-430) over the slots in ascending order: the strict minimum, a tie to the lowest slot.  Counts the non-unit
// branch and the ties for the tests' coverage condition (nullable).
template <class V> FA_SPK_HD inline int closest(const View &db, const V &q, float *distance, int *non_unit = nullptr, int *ties = nullptr) {
    const float ssq = sumsq(q);
    float best = inf32();
    int at = -1;
    for (uint64_t left = db.live; left;) {   // kInFlight rows are requested before the first of them is reduced
        V c[kInFlight];
        int slot[kInFlight];
FA_SPK_UNROLL
        for (int u = 0; u < kInFlight; ++u) {
            slot[u] = left ? __builtin_ctzll(left) : -1;
            if (slot[u] >= 0) c[u] = V::load(db.cur(slot[u]));
            left &= left - 1;
        }
FA_SPK_UNROLL
        for (int u = 0; u < kInFlight; ++u) {
            if (slot[u] < 0) continue;
            const float d = cosine_from_sums(V::dot(q, c[u]), ssq, sumsq(c[u]), non_unit);
            if (ties && at >= 0 && d == best) *ties += 1;
            if (d < best) { best = d; at = slot[u]; }
        }
    }
    *distance = best;
    return at;
}

// SpeakerManager.assignSpeaker (:135-177) for one item.  On the device every lane holds the same scalars and stores them: a lane reads back
// what it wrote itself, in program order.
template <class V> FA_SPK_HD inline Record assign_one(View &db, const Params &p, const V &e, const float duration, const int64_t tick) {
    Record out{0, -1, kInvalid, inf32()};
    if (!e.finite()) return out;                                                         // this library: no NaN speaker
    if (p.validate_min_magnitude >= 0.0f && !(sqrtf(sumsq(e)) > p.validate_min_magnitude)) return out;   // validateEmbedding (:106-126)
    const V n = l2_normalize(e);
    const int at = closest<V>(db, n, &out.distance);
    if (at >= 0 && out.distance < p.speaker_threshold) {                                 // updateExistingSpeaker (:432-460)
        SlotMeta m = db.meta[at];
        out.id = m.id; out.slot = at;
        if (out.distance < p.embedding_threshold) {
            if (sumsq(n) > 0.01f) {
                update_main<V>(db, at, m, n, duration, p.ema_alpha, tick);
                out.kind = kUpdated;
            } else {
                out.kind = kLowEnergy;
                return out;
            }
        } else {
            m.duration += duration;
            m.updated = tick;
            out.kind = kDurationOnly;
        }
        db.meta[at] = m;
        return out;
    }
    if (!(duration >= p.min_speech_duration)) { out.kind = kTooShort; return out; }
    const int slot = lowest_free_slot(db);
    if (slot < 0) { out.kind = kFull; return out; }
    const V ne = l2_normalize(n);                                                        // createNewSpeaker (:462-492)
    const int32_t id = *db.next_id;
    SlotMeta m = fresh_meta(id, duration, tick, tick, false);
    l2_normalize(ne).store(db.cur(slot));                                                // Speaker.init
    add_raw<V>(db, slot, m, l2_normalize(ne), tick);                                     // RawEmbedding.init, addRawEmbedding
    db.meta[slot] = m;
    *db.next_id = id + 1;
    db.live |= 1ull << slot;
    out.id = id; out.slot = slot; out.kind = kCreated;
    return out;
}

// ---- the management edits: one stream's slot scalars on the host.  Each returns whether it changed them; the embeddings' rows stay
// where they are (the host unit copies them once an edit has accepted).
struct HostStream {
    std::vector<SlotMeta> meta;   // [max_speakers]
    int32_t next_id = 1;
    int find(const int32_t id) const {
        for (size_t s = 0; s < meta.size(); ++s)
            if ((meta[s].flags & kLive) && meta[s].id == id) return static_cast<int>(s);
        return -1;
    }
    int lowest_free() const {
        for (size_t s = 0; s < meta.size(); ++s)
            if (!(meta[s].flags & kLive)) return static_cast<int>(s);
        return -1;
    }
};

struct Upsert {
    Verdict verdict;          // refused: nothing was edited
    int slot = -1;            // where the current embedding and the raws go
    bool normalise = false;   // a new speaker: Speaker.init normalises the current embedding
};

// upsertSpeaker (:552-606) of info->id >= 1 with 0 <= info->raw_count raws.
inline Upsert upsert_edit(HostStream &h, const fa_speaker_info &info, const int32_t raw_capacity, const int32_t stream) {
    Upsert u;
    if (info.raw_count > raw_capacity) { u.verdict = refuse(FA_INVALID_ARGUMENT, "speaker_db upsert: more raw embeddings than raw_capacity"); return u; }
    u.slot = h.find(info.id);
    if (u.slot >= 0) {   // :565-580: the fields as given, createdAt kept, permanence only ever set
        SlotMeta &m = h.meta[u.slot];
        m.duration = info.duration; m.updates = info.update_count; m.updated = info.updated_tick;
        if (info.is_permanent) m.flags |= kPermanent;
    } else {             // :582-602
        u.slot = h.lowest_free();
        if (u.slot < 0) { u.verdict = refuse(FA_OUTPUT_TOO_SMALL, "speaker_db upsert: no free slot in stream %d", stream); return u; }
        u.normalise = true;
        h.meta[u.slot] = fresh_meta(info.id, info.duration, info.created_tick, info.updated_tick, info.is_permanent != 0);
        h.meta[u.slot].updates = info.update_count;
        h.next_id = h.next_id > info.id + 1 ? h.next_id : info.id + 1;
    }
    h.meta[u.slot].head = 0; h.meta[u.slot].count = info.raw_count;
    return u;
}

// getSpeaker: *info (id 0, slot -1 without such a speaker); the slot, whose meta tells the caller where the rows are.
inline int get_edit(const HostStream &h, const int32_t id, fa_speaker_info *info) {
    std::memset(info, 0, sizeof(*info));
    info->slot = -1;
    const int slot = h.find(id);
    if (slot < 0) return slot;
    const SlotMeta &m = h.meta[slot];
    info->id = m.id; info->slot = slot; info->raw_count = m.count; info->update_count = m.updates; info->is_permanent = (m.flags & kPermanent) ? 1 : 0;
    info->duration = m.duration; info->created_tick = m.created; info->updated_tick = m.updated;
    return slot;
}

// the live ids in slot order into ids[max_speakers]; their number
inline int32_t ids(const HostStream &h, int32_t *out) {
    int32_t n = 0;
    for (const SlotMeta &m : h.meta)
        if (m.flags & kLive) out[n++] = m.id;
    return n;
}

inline int32_t count(const HostStream &h) {
    int32_t n = 0;
    for (const SlotMeta &m : h.meta) n += (m.flags & kLive) ? 1 : 0;
    return n;
}

inline bool remove(HostStream &h, const int32_t id, const bool keep_if_permanent) {   // :334-347
    const int slot = h.find(id);
    if (slot < 0 || (keep_if_permanent && (h.meta[slot].flags & kPermanent))) return false;
    h.meta[slot] = SlotMeta{};
    return true;
}

inline bool remove_inactive(HostStream &h, const int64_t since_tick, const bool keep_if_permanent) {   // :353-367
    bool changed = false;
    for (SlotMeta &m : h.meta)
        if ((m.flags & kLive) && m.updated < since_tick && !(keep_if_permanent && (m.flags & kPermanent))) { m = SlotMeta{}; changed = true; }
    return changed;
}

inline bool set_permanent(HostStream &h, const int32_t id, const bool permanent) {
    const int slot = h.find(id);
    if (slot < 0) return false;
    h.meta[slot].flags = kLive | (permanent ? kPermanent : 0);
    return true;
}

inline bool reset(HostStream &h, const bool keep_if_permanent) {   // :610-628
    int32_t max_id = 0;
    for (SlotMeta &m : h.meta) {
        if (keep_if_permanent && (m.flags & kLive) && (m.flags & kPermanent)) max_id = m.id > max_id ? m.id : max_id;
        else m = SlotMeta{};
    }
    h.next_id = max_id + 1;
    return true;
}

}  // namespace spk
}  // namespace fa
