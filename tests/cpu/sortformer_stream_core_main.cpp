// The integers of fluidaudio_amd/csrc/sortformer_stream_core.h — clamps, quotas, slab sizes, pop-out lengths, one update's plan, the two
// chunk plans — printed over a sweep of geometries by a stand-alone program built with -fsanitize=address,undefined -ffp-contract=off
// (tests/test_sortformer_stream_cpu.py compares every line with the restatement).  The arrays it indexes have exactly their size.
#include <cstdio>
#include <vector>

#include "../../fluidaudio_amd/csrc/sortformer_stream_core.h"

using namespace fa::sfs;

struct Geo { int speakers, cache, fifo, chunk, lc, rc, period, sil; float strong, weak, minpos; };

int main() {
    const Geo geos[] = {{4, 188, 40, 6, 1, 7, 31, 3, 0.75f, 1.5f, 0.5f},   {4, 188, 188, 6, 1, 7, 144, 3, 0.75f, 1.5f, 0.5f}, {4, 188, 40, 340, 1, 40, 300, 3, 0.75f, 1.5f, 0.5f},
                        {4, 188, 40, 25, 1, 7, 31, 3, 0.75f, 1.5f, 0.5f},  {4, 32, 5, 3, 1, 2, 4, 3, 0.75f, 1.5f, 0.5f},      {2, 32, 5, 3, 1, 2, 4, 3, 0.3f, 0.7f, 0.9f},
                        {3, 32, 5, 3, 1, 2, 4, 3, 0.7f, 1.1f, 0.35f},      {4, 16, 5, 3, 1, 2, 4, 3, 0.75f, 1.5f, 0.5f},      {4, 3, 2, 0, 0, 0, 100, 3, 0.75f, 1.5f, 0.5f},
                        {1, 50, 7, 4, 2, 3, 1, 0, 0.1f, 0.0f, 1.0f},       {3, 100, 0, 5, 0, 0, 9, 1, 0.99f, 2.5f, 0.01f}};
    int index = 0;
    for (const Geo &g : geos) {
        Config c{};
        c.speakers = g.speakers; c.d_model = 8; c.chunk_len = g.chunk; c.chunk_left_context = g.lc; c.chunk_right_context = g.rc; c.fifo_len = g.fifo;
        c.spkcache_len = g.cache; c.spkcache_update_period = g.period; c.sil_frames_per_spk = g.sil; c.max_index = 99999; c.subsampling = 8; c.n_mels = 128;
        c.silence_threshold = 0.2f; c.pred_score_threshold = 0.25f; c.scores_boost_latest = 0.05f;
        c.strong_boost_rate = g.strong; c.weak_boost_rate = g.weak; c.min_pos_scores_rate = g.minpos;
        clamp(c);
        c.max_chunk_frames = c.chunk_len + c.chunk_left_context + c.chunk_right_context;
        std::printf("GEO %d %d %d %d %d\n", index++, c.chunk_len, c.spkcache_len, c.spkcache_update_period, config_fault(c));
        const Quotas q = quotas(c);
        const Slabs s = slabs(c);
        std::printf("QUOTA %d %d %d %d\n", q.len_per_spk, q.strong, q.weak, q.min_pos);
        std::printf("SLAB %d %d %d %d\n", s.max_pop, s.score_rows, s.fifo_pred_rows, s.keys);
        std::printf("POP");
        std::vector<int> pops(static_cast<size_t>(c.max_chunk_frames));
        for (int k = 0; k < c.max_chunk_frames; ++k) pops[static_cast<size_t>(k)] = pop_out_length(c.spkcache_update_period, c.fifo_len + 1 + k, c.fifo_len);
        for (const int p : pops) std::printf(" %d", p);
        std::printf("\n");
        // one update's plan over the lengths, the operands and the short pred counts
        const int spks[] = {0, c.spkcache_len / 2, c.spkcache_len}, fifos[] = {0, c.fifo_len / 2, c.fifo_len};
        for (const int spk : spks)
            for (const int fifo : fifos)
                for (int present = 0; present < 2; ++present)
                    for (const int emb : {0, c.chunk_len + c.chunk_right_context, c.max_chunk_frames, c.max_chunk_frames + 1})
                        for (const int lc : {0, c.chunk_left_context, -1})
                            for (const int rc : {-1, c.chunk_right_context})
                                for (const int cut : {0, 1, c.chunk_right_context + 1, emb + 1}) {
                                    const int rows = spk + fifo + emb - cut;
                                    const Plan p = plan_update(c, spk, fifo, present, emb, rows, c.spkcache_len + c.fifo_len + c.max_chunk_frames + 1, lc, rc);
                                    std::printf("PLAN %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %d\n", spk, fifo, present, emb, lc, rc, rows, p.status, p.mode, p.core, p.pop,
                                                p.new_fifo, p.new_spk, p.first_overflow, p.status == kOk ? p.chunk_start : 0);
                                }
        // mel frames arriving 13 at a time: getNextChunkFeaturesLocked until it has nothing, the consumed frames dropped
        int64_t buffered = 0, start = 0;
        for (int arrival = 0; arrival < 60; ++arrival) {
            buffered += 13;
            for (;;) {
                const Chunk k = stream_chunk(c, buffered, start);
                if (!k.ready) break;
                std::printf("CHUNK %d %d %d %d %lld %lld %lld %lld\n", k.ready, k.chunk_length, k.left_offset, k.right_offset, static_cast<long long>(k.start_frame),
                            static_cast<long long>(k.rows), static_cast<long long>(k.new_start_feat), static_cast<long long>(k.frames_to_drop));
                buffered -= k.frames_to_drop;
                start = k.new_start_feat;
            }
        }
        for (const int64_t feat : {int64_t{0}, int64_t{5}, int64_t{100}, int64_t{777}, int64_t{3001}}) {
            const int64_t seq = feat > 9 ? feat - 9 : feat;
            int64_t at = 0, n = 0;
            std::printf("FILE %lld %lld %lld", static_cast<long long>(feat), static_cast<long long>(seq), static_cast<long long>(file_num_chunks(c, feat)));
            for (;;) {
                const Chunk k = file_chunk(c, feat, seq, at);
                if (!k.ready) break;
                std::printf(" %d,%d,%d,%lld,%lld,%lld", k.chunk_length, k.left_offset, k.right_offset, static_cast<long long>(k.start_frame), static_cast<long long>(k.rows),
                            static_cast<long long>(k.new_start_feat));
                at = k.new_start_feat;
                ++n;
            }
            std::printf(" | %lld\n", static_cast<long long>(n));
        }
    }
    return 0;
}
