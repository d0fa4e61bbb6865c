// A stand-alone program over the host half of fluidaudio_amd/csrc/speaker_db_core.h, built with the address and undefined-behaviour
// sanitizers by tests/test_speaker_db_core_asan.py: it assigns into databases whose arrays have exactly their size (raw_capacity 1, 3
// and 50; one-slot and several-slot tables), fills every slot, overflows the table and wraps the ring, and prints every record and the
// final state as bits for the test to hold against tests/online_restatement.py.  The inputs come from integer arithmetic the test repeats.
// Then it runs one script of management edits (upsert, get, ids, count, remove, remove_inactive, permanence, reset) on a HostStream whose
// table has exactly its size (1, 3 and 64 slots) and prints the state after every step; the test repeats the script on SpeakerManager.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/speaker_db_core.h"

namespace spk = fa::spk;

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s; }
// 256 values k / 32768, k in [-32768, 32767]: exact in fp32
static void draw(uint32_t seed, float *out) {
    for (int i = 0; i < spk::kDim; ++i) out[i] = static_cast<float>(static_cast<int>(lcg(seed) >> 8 & 0xFFFFu) - 32768) / 32768.0f;
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void run(const int S, const int R, const int items) {
    // every array exactly its size, on the heap: one element past any of them is the sanitizer's
    float *current = static_cast<float *>(std::calloc(static_cast<size_t>(S) * spk::kDim, sizeof(float)));
    float *raws = static_cast<float *>(std::calloc(static_cast<size_t>(S) * R * spk::kDim, sizeof(float)));
    spk::SlotMeta *meta = static_cast<spk::SlotMeta *>(std::calloc(S, sizeof(spk::SlotMeta)));
    int32_t *next_id = static_cast<int32_t *>(std::malloc(sizeof(int32_t)));
    *next_id = 1;
    spk::View db{current, raws, meta, next_id, S, R, 0};
    const spk::Params p{0.65f, 0.45f, 1.0f, 0.9f, 0.1f, S, R};
    std::printf("CONFIG %d %d %d\n", S, R, items);
    std::vector<float> voice(spk::kDim), noise(spk::kDim);
    uint32_t pick = 12345u + static_cast<uint32_t>(S * 131 + R);
    for (int it = 0; it < items; ++it) {
        const uint32_t r = lcg(pick) >> 10;
        const int v = (r & 3u) ? 0 : static_cast<int>((r >> 2) % static_cast<uint32_t>(S + 2));   // voice 0 three times in four: its ring wraps
        const float scale = ((r >> 12) % 3u) == 0 ? 2.0f : ((r >> 12) % 3u) == 1 ? 0.25f : 0.015625f;
        const float duration = ((r >> 16) & 7u) == 0 ? 0.5f : 2.0f;
        draw(1000u + static_cast<uint32_t>(v), voice.data());
        draw(77777u + static_cast<uint32_t>(it), noise.data());
        spk::Vec256 e;
        for (int i = 0; i < spk::kDim; ++i) e.v[i] = voice[i] + noise[i] * scale;
        const spk::Record rec = spk::assign_one<spk::Vec256>(db, p, e, duration, it);
        std::printf("REC %d %d %d %08" PRIx32 "\n", rec.id, rec.slot, rec.kind, bits(rec.distance));
    }
    for (int s = 0; s < S; ++s) {
        const spk::SlotMeta &m = meta[s];
        if (!(m.flags & spk::kLive)) continue;
        std::printf("SLOT %d %d %d %d %08" PRIx32 " %" PRId64 " %" PRId64, s, m.id, m.count, m.updates, bits(m.duration), m.created, m.updated);
        for (int i = 0; i < spk::kDim; ++i) std::printf(" %08" PRIx32, bits(db.cur(s)[i]));
        std::printf("\n");
    }
    std::free(current); std::free(raws); std::free(meta); std::free(next_id);
}

// ---- the management edits.  The script is the test's too (test_speaker_db_core_asan.py: script()).
static void state(const char *step, const spk::HostStream &h, const fa::Verdict &v) {
    int32_t *ids = new int32_t[h.meta.size()];
    const int32_t n = spk::ids(h, ids);
    std::printf("STEP %s %d %d %d |", step, static_cast<int>(v.status), h.next_id, spk::count(h));
    for (int32_t i = 0; i < n; ++i) {
        fa_speaker_info info;
        const int slot = spk::get_edit(h, ids[i], &info);
        std::printf(" %d %d %d %d %d %08" PRIx32 " %" PRId64 " %" PRId64, slot, info.id, info.raw_count, info.update_count, info.is_permanent, bits(info.duration),
                    info.created_tick, info.updated_tick);
    }
    if (n != spk::count(h)) std::printf(" COUNT-MISMATCH");
    std::printf("\nTEXT %s\n", v.text);
    delete[] ids;
}

static fa::Verdict upsert(spk::HostStream &h, const int R, int32_t id, int32_t raws, int32_t updates, bool permanent, float duration, int64_t created, int64_t updated) {
    const fa_speaker_info info{id, -1, raws, updates, permanent ? 1 : 0, duration, created, updated};
    const spk::Upsert u = spk::upsert_edit(h, info, R, 0);
    if (u.verdict.status == FA_SUCCESS && (u.slot < 0 || static_cast<size_t>(u.slot) >= h.meta.size())) std::printf("BAD-SLOT\n");
    return u.verdict;
}

static void manage(const int S, const int R) {
    spk::HostStream h;
    h.meta = std::vector<spk::SlotMeta>(static_cast<size_t>(S));   // exactly S entries on the heap
    const fa::Verdict ok;
    std::printf("MANAGE %d %d\n", S, R);
    state("empty", h, ok);
    state("upsert_new", h, upsert(h, R, 5, 0, 2, false, 1.5f, 10, 11));
    state("upsert_existing", h, upsert(h, R, 5, R, 7, true, 2.5f, 99, 20));
    state("upsert_too_many_raws", h, upsert(h, R, 9, R + 1, 1, false, 1.0f, 0, 0));
    for (int i = 0; i < S - 1; ++i) upsert(h, R, 100 + i, i % (R + 1), 1, i % 3 == 0, 0.25f * static_cast<float>(i), i, i);
    state("filled", h, ok);
    state("upsert_full", h, upsert(h, R, 999, 0, 1, false, 1.0f, 0, 0));
    spk::remove(h, 4242, true);
    state("remove_missing", h, ok);
    spk::remove(h, 5, true);
    state("remove_permanent_kept", h, ok);
    spk::set_permanent(h, 5, false);
    spk::set_permanent(h, 4242, true);
    state("revoked", h, ok);
    spk::remove(h, 5, true);
    state("removed", h, ok);
    state("upsert_low_id", h, upsert(h, R, 3, 1, 1, false, 3.0f, 7, 8));
    spk::set_permanent(h, 3, true);
    state("made_permanent", h, ok);
    spk::remove(h, 3, false);
    state("remove_permanent_forced", h, ok);
    spk::remove_inactive(h, S / 2, true);
    state("remove_inactive", h, ok);
    spk::reset(h, true);
    state("reset_keep", h, ok);
    state("upsert_after_reset", h, upsert(h, R, 2, 0, 1, false, 1.0f, 1, 1));
    spk::reset(h, false);
    state("reset_all", h, ok);
}

int main() {
    run(1, 1, 12);
    run(3, 3, 60);
    run(4, 50, 260);
    run(64, 1, 40);
    // the cosine's branches on their own: a zero vector, a non-unit one
    spk::Vec256 a = spk::Vec256::zero(), b = spk::Vec256::zero();
    b.v[0] = 3.0f; b.v[1] = 4.0f;
    std::printf("COS %08" PRIx32 " %08" PRIx32 "\n", bits(spk::cosine_from_sums(spk::Vec256::dot(a, b), spk::sumsq(a), spk::sumsq(b))),
                bits(spk::cosine_from_sums(spk::Vec256::dot(b, b), spk::sumsq(b), spk::sumsq(b))));
    manage(1, 3);
    manage(3, 3);
    manage(64, 3);
    return 0;
}
