// A stand-alone program over the host half of fluidaudio_amd/csrc/speaker_db_core.h, built with the address and undefined-behaviour
// sanitizers by tests/test_speaker_db_core_asan.py: it assigns into databases whose arrays have exactly their size (raw_capacity 1, 3
// and 50; one-slot and several-slot tables), fills every slot, overflows the table and wraps the ring, and prints every record and the
// final state as bits for the test to hold against tests/online_restatement.py.  The inputs come from integer arithmetic the test repeats.
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
    return 0;
}
