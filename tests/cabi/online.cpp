// A C++ host of the online speaker database's entries and their Swift-shaped mirror (include/fluidaudio.hpp: SpeakerUtilities,
// RawEmbedding, Speaker, SpeakerManager), built by tests/test_cabi_online.py with g++ -Werror.  Without an argument no device is
// touched: the layouts, the defaults, the arithmetic entries (which take no context) and every refusal (the context is NULL).
//   LAYOUT name size offsets...     the C structs as the compiler lays them out
//   CFG ...                         fa_speaker_db_default_config, floats as hex bits
//   NORM / COS / VALID              the arithmetic on the reference's test patterns, as bits
//   ST name status...               the status of every refusal
// With the argument "device" it runs the mirror's SpeakerManager on device 0 instead and prints what the reference's tests look at:
//   REC id slot kind distance       after every assignSpeaker;  SPK id count updates duration current...   getSpeaker's answer
#include <cinttypes>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "fluidaudio.hpp"

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static std::vector<float> distinct(int pattern) {   // createDistinctEmbedding
    std::vector<float> e(256);
    for (int i = 0; i < 256; ++i) e[static_cast<size_t>(i)] = static_cast<float>(std::sin(static_cast<double>(static_cast<float>(i + pattern * 100) * 0.1f)));
    return e;
}

static void print_speaker(const std::optional<fluidaudio::Speaker> &s) {
    if (!s) { printf("SPK none\n"); return; }
    printf("SPK %d %zu %d %08x %" PRId64 " %" PRId64 " %d", s->id, s->rawEmbeddings.size(), s->updateCount, bits(s->duration), s->createdAt, s->updatedAt, s->isPermanent ? 1 : 0);
    for (const float v : s->currentEmbedding) printf(" %08x", bits(v));
    printf("\n");
}

static int device_run() {
    fluidaudio::Context ctx(0);
    fluidaudio::SpeakerManager m(ctx, 0.3f, 0.2f, 1.0f, 4, 3);
    const auto rec = [&]() { printf("REC %d %d %d %08x\n", m.lastAssignment.id, m.lastAssignment.slot, m.lastAssignment.kind, bits(m.lastAssignment.distance)); };
    std::vector<float> e1 = distinct(1), e2 = distinct(1);
    e2[0] += 0.01f;
    print_speaker(m.assignSpeaker(e1, 3.0f, 5)); rec();
    print_speaker(m.assignSpeaker(e2, 0.5f, 6)); rec();
    print_speaker(m.assignSpeaker(distinct(2), 0.5f, 7)); rec();
    print_speaker(m.assignSpeaker(distinct(2), 2.0f, 8)); rec();
    m.upsertSpeaker(fluidaudio::Speaker(7, distinct(3), 5.0f, 1, 2, true));
    const auto found = m.findSpeaker(fluidaudio::SpeakerUtilities::l2Normalize(distinct(3)));
    printf("FIND %d %08x\n", found.first.value_or(0), bits(found.second));
    for (const auto &p : m.findMatchingSpeakers(fluidaudio::SpeakerUtilities::l2Normalize(distinct(1)), 2.0f)) printf("MATCH %d %08x\n", p.first, bits(p.second));
    for (const auto &p : m.findMergeablePairs(2.0f, false)) printf("PAIR %d %d\n", p.speakerToMerge, p.destination);
    m.removeSpeaker(7);
    m.reset(true);
    printf("IDS");
    for (const int id : m.speakerIds()) printf(" %d", id);
    printf(" | %d\n", m.speakerCount());
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "device") == 0) return device_run();
    printf("LAYOUT config %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_speaker_db_config), offsetof(fa_speaker_db_config, speaker_threshold),
           offsetof(fa_speaker_db_config, embedding_threshold), offsetof(fa_speaker_db_config, min_speech_duration), offsetof(fa_speaker_db_config, ema_alpha),
           offsetof(fa_speaker_db_config, validate_min_magnitude), offsetof(fa_speaker_db_config, max_speakers), offsetof(fa_speaker_db_config, raw_capacity));
    printf("LAYOUT assignment %zu %zu %zu %zu %zu\n", sizeof(fa_speaker_assignment), offsetof(fa_speaker_assignment, id), offsetof(fa_speaker_assignment, slot),
           offsetof(fa_speaker_assignment, kind), offsetof(fa_speaker_assignment, distance));
    printf("LAYOUT pair %zu %zu %zu %zu %zu %zu\n", sizeof(fa_speaker_pair), offsetof(fa_speaker_pair, source_id), offsetof(fa_speaker_pair, destination_id),
           offsetof(fa_speaker_pair, source_slot), offsetof(fa_speaker_pair, destination_slot), offsetof(fa_speaker_pair, distance));
    printf("LAYOUT info %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_speaker_info), offsetof(fa_speaker_info, id), offsetof(fa_speaker_info, slot),
           offsetof(fa_speaker_info, raw_count), offsetof(fa_speaker_info, update_count), offsetof(fa_speaker_info, is_permanent), offsetof(fa_speaker_info, duration),
           offsetof(fa_speaker_info, created_tick), offsetof(fa_speaker_info, updated_tick));

    fa_speaker_db_config d;
    memset(&d, 0xff, sizeof(d));
    fa_speaker_db_default_config(&d);
    printf("CFG %08x %08x %08x %08x %08x %d %d\n", bits(d.speaker_threshold), bits(d.embedding_threshold), bits(d.min_speech_duration), bits(d.ema_alpha),
           bits(d.validate_min_magnitude), d.max_speakers, d.raw_capacity);

    using U = fluidaudio::SpeakerUtilities;
    for (int p = 1; p <= 3; ++p) {
        printf("NORM");
        for (const float v : U::l2Normalize(distinct(p))) printf(" %08x", bits(v));
        printf("\n");
    }
    std::vector<float> zero(256, 0.0f), low(256, 0.0f), custom(256, 0.0f), bad = distinct(1);
    low[0] = 0.01f; custom[0] = 0.2f; bad[5] = std::nanf("");
    printf("COS %08x %08x %08x %08x %08x\n", bits(U::cosineDistance(distinct(1), distinct(2))), bits(U::cosineDistance(U::l2Normalize(distinct(1)), U::l2Normalize(distinct(3)))),
           bits(U::cosineDistance(zero, distinct(1))), bits(U::cosineDistance(distinct(1), std::vector<float>(128, 0.5f))), bits(fluidaudio::RawEmbedding(distinct(2)).embedding[7]));
    printf("VALID %d %d %d %d %d\n", U::validateEmbedding(distinct(1)) ? 1 : 0, U::validateEmbedding(zero) ? 1 : 0, U::validateEmbedding(low, 0.1f) ? 1 : 0,
           U::validateEmbedding(custom, 0.1f) ? 1 : 0, U::validateEmbedding(bad) ? 1 : 0);

    // every refusal, with nothing launched: NULL pointers, non-positive counts, max_speakers outside 1 .. 64, raw_capacity < 1
    fa_speaker_db *db = reinterpret_cast<fa_speaker_db *>(&d), *made = nullptr;   // never dereferenced: the NULL context is refused first
    fa_speaker_db_config c = d;
    const float e[256] = {0.0f};
    float dist[64];
    int32_t n = 0, ids[64];
    fa_speaker_assignment rec;
    fa_speaker_pair pair;
    fa_speaker_info info{};
    printf("ST create %d %d %d", fa_speaker_db_create(nullptr, &d, 1, &made), fa_speaker_db_create(nullptr, nullptr, 1, &made), fa_speaker_db_create(nullptr, &d, 1, nullptr));
    c = d; c.max_speakers = 0;
    printf(" %d", fa_speaker_db_create(nullptr, &c, 1, &made));
    c = d; c.max_speakers = 65;
    printf(" %d", fa_speaker_db_create(nullptr, &c, 1, &made));
    c = d; c.raw_capacity = 0;
    printf(" %d %d\n", fa_speaker_db_create(nullptr, &c, 1, &made), fa_speaker_db_create(nullptr, &d, 0, &made));
    printf("ST calls %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", fa_speaker_db_assign_dev(nullptr, db, e, e, nullptr, 1, 0, &rec), fa_speaker_db_assign(nullptr, db, e, e, nullptr, 1, 0, &rec),
           fa_speaker_db_distances_dev(nullptr, db, e, 1, dist, nullptr), fa_speaker_db_distances(nullptr, db, e, 1, dist, nullptr),
           fa_speaker_db_mergeable_pairs_dev(nullptr, db, 0.5f, 1, &pair, 1, &n), fa_speaker_db_mergeable_pairs(nullptr, db, 0.5f, 1, &pair, 1, &n),
           fa_speaker_db_upsert(nullptr, db, 0, &info, e, nullptr), fa_speaker_db_get(nullptr, db, 0, 1, &info, nullptr, nullptr, 0), fa_speaker_db_ids(nullptr, db, 0, ids, &n),
           fa_speaker_db_count(nullptr, db, &n), fa_speaker_db_remove(nullptr, db, 0, 1, 1), fa_speaker_db_remove_inactive(nullptr, db, -1, 0, 1),
           fa_speaker_db_set_permanent(nullptr, db, 0, 1, 1), fa_speaker_db_reset(nullptr, db, -1, 0));
    printf("ST null %d %08x %d\n", fa_speaker_l2_normalize(nullptr, dist), bits(fa_speaker_cosine_distance(nullptr, e)), fa_speaker_validate_embedding(nullptr, 0.1f));
    fa_speaker_db_destroy(nullptr);
    bool threw = false;
    try { (void)U::l2Normalize(std::vector<float>(128, 0.5f)); } catch (const fluidaudio::Error &) { threw = true; }
    printf("THROW %d\n", threw ? 1 : 0);
    return made == nullptr ? 0 : 1;
}
