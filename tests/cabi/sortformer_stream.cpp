// A C++ host of the streaming Sortformer entries and their Swift-shaped mirror (include/fluidaudio.hpp: SortformerConfig,
// StreamingUpdateResult, SortformerStreamingState), built by tests/test_cabi_sortformer_stream.py with g++ -Werror.  No device is touched:
// the layouts, the defaults and presets, the derived integers, the two host plan functions and every refusal (the context is NULL).
//   LAYOUT name size offsets...     the C structs as the compiler lays them out
//   CFG preset ints... floats       fa_sortformer_stream_preset_config, floats as hex bits
//   GEO preset ...                  fa_sortformer_stream_geometry
//   POP ...                         fa_sortformer_stream_pop_out_length over contexts
//   CHUNK ... / FILE ...            the plan functions through the mirror
//   ST name status...               the status of every refusal
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "fluidaudio.hpp"

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static void print_chunk(const char *tag, const fa_sortformer_chunk &k) {
    printf("%s %d %d %d %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", tag, k.ready, k.chunk_length, k.left_offset, k.right_offset, k.start_frame, k.rows, k.new_start_feat,
           k.frames_to_drop);
}

int main() {
    printf("LAYOUT config %zu %zu %zu %zu %zu %zu\n", sizeof(fa_sortformer_stream_config), offsetof(fa_sortformer_stream_config, speakers), offsetof(fa_sortformer_stream_config, max_index),
           offsetof(fa_sortformer_stream_config, n_mels), offsetof(fa_sortformer_stream_config, silence_threshold), offsetof(fa_sortformer_stream_config, min_pos_scores_rate));
    printf("LAYOUT geometry %zu %zu %zu\n", sizeof(fa_sortformer_stream_geometry_info), offsetof(fa_sortformer_stream_geometry_info, max_pop), offsetof(fa_sortformer_stream_geometry_info, lds_bytes));
    printf("LAYOUT info %zu %zu\n", sizeof(fa_sortformer_stream_info), offsetof(fa_sortformer_stream_info, silence_frame_count));
    printf("LAYOUT chunk %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_sortformer_chunk), offsetof(fa_sortformer_chunk, ready), offsetof(fa_sortformer_chunk, chunk_length),
           offsetof(fa_sortformer_chunk, left_offset), offsetof(fa_sortformer_chunk, right_offset), offsetof(fa_sortformer_chunk, start_frame), offsetof(fa_sortformer_chunk, rows),
           offsetof(fa_sortformer_chunk, new_start_feat), offsetof(fa_sortformer_chunk, frames_to_drop));

    for (int preset = 0; preset < 4; ++preset) {
        const fluidaudio::SortformerConfig cfg(preset);
        const fa_sortformer_stream_config &c = cfg.c;
        printf("CFG %d %d %d %d %d %d %d %d %d %d %d %d %d %d %08x %08x %08x %08x %08x %08x\n", preset, c.speakers, c.d_model, c.chunk_len, c.chunk_left_context, c.chunk_right_context,
               c.fifo_len, c.spkcache_len, c.spkcache_update_period, c.sil_frames_per_spk, c.max_index, c.max_chunk_frames, c.subsampling, c.n_mels, bits(c.silence_threshold),
               bits(c.pred_score_threshold), bits(c.scores_boost_latest), bits(c.strong_boost_rate), bits(c.weak_boost_rate), bits(c.min_pos_scores_rate));
        const fa_sortformer_stream_geometry_info g = cfg.geometry();
        printf("GEO %d %d %d %d %d %d %d %d %d %d %d %d\n", preset, g.chunk_len, g.spkcache_len, g.spkcache_update_period, g.max_pop, g.score_rows, g.out_rows, g.chunk_mel_frames,
               g.spkcache_len_per_spk, g.strong_boost_per_spk, g.weak_boost_per_spk, g.min_pos_scores_per_spk);
        printf("POP %d", preset);
        for (int context = 0; context <= c.fifo_len + c.max_chunk_frames; context += 3) printf(" %d", fa_sortformer_stream_pop_out_length(&c, context));
        printf("\n");
        // mel frames arriving 29 at a time
        int64_t buffered = 0, start = 0;
        for (int arrival = 0; arrival < 40; ++arrival) {
            buffered += 29;
            for (;;) {
                const fa_sortformer_chunk k = cfg.nextChunk(buffered, start);
                if (!k.ready) break;
                print_chunk("CHUNK", k);
                buffered -= k.frames_to_drop;
                start = k.new_start_feat;
            }
        }
        for (const int64_t feat : {int64_t{0}, int64_t{103}, int64_t{104}, int64_t{1000}}) {
            int64_t num = -1;
            const std::vector<fa_sortformer_chunk> chunks = cfg.fileChunks(feat, feat > 20 ? feat - 20 : feat, &num);
            printf("FILE %" PRId64 " %" PRId64 " %zu\n", feat, num, chunks.size());
            for (const fa_sortformer_chunk &k : chunks) print_chunk("FCHUNK", k);
        }
    }
    // the clamps through the geometry: chunk_len 0, a cache below (1 + sil) * speakers, a period above fifo_len + chunk_len
    fa_sortformer_stream_config d, c;
    fa_sortformer_stream_default_config(&d);
    c = d; c.chunk_len = 0; c.spkcache_len = 3; c.spkcache_update_period = 1000;
    fa_sortformer_stream_geometry_info g{};
    const fa_status clamped = fa_sortformer_stream_geometry(&c, &g);
    printf("CLAMP %d %d %d %d\n", clamped, g.chunk_len, g.spkcache_len, g.spkcache_update_period);

    // every refusal, with nothing launched
    fa_sortformer_stream *made = nullptr, *st = reinterpret_cast<fa_sortformer_stream *>(&d);   // never dereferenced: the NULL context is refused first
    printf("ST config");
    const auto refused = [&](const fa_sortformer_stream_config &k) { printf(" %d", fa_sortformer_stream_geometry(&k, &g)); };
    c = d; c.speakers = 0; refused(c);
    c = d; c.speakers = 5; refused(c);
    c = d; c.d_model = 510; refused(c);
    c = d; c.fifo_len = -1; refused(c);
    c = d; c.max_chunk_frames = 0; refused(c);
    c = d; c.strong_boost_rate = -0.5f; refused(c);
    c = d; c.pred_score_threshold = 0.0f; refused(c);
    c = d; c.pred_score_threshold = 1.0f; refused(c);
    c = d; c.max_index = 4 * (188 + 31 + 3); refused(c);          // a live index would reach the sentinel
    c = d; c.max_index = 4 * (188 + 31 + 3) + 1; refused(c);      // the smallest sentinel that is safe: accepted
    c = d; c.spkcache_len = 4000; refused(c);                     // the scored rows exceed one workgroup's LDS
    printf(" %d %d %d\n", fa_sortformer_stream_geometry(nullptr, &g), fa_sortformer_stream_geometry(&d, nullptr), fa_sortformer_stream_pop_out_length(nullptr, 50));
    c = d; c.speakers = 9;
    printf("ST create %d %d %d %d %d\n", fa_sortformer_stream_create(nullptr, &d, 1, &made), fa_sortformer_stream_create(nullptr, nullptr, 1, &made),
           fa_sortformer_stream_create(nullptr, &d, 1, nullptr), fa_sortformer_stream_create(nullptr, &c, 1, &made), fa_sortformer_stream_create(nullptr, &d, 0, &made));
    float f[4] = {0, 0, 0, 0}, *pf = nullptr;
    int32_t i4[4] = {0, 0, 0, 0}, *pi = nullptr;
    int64_t n = 0, l4[2] = {10, 0};
    fa_sortformer_stream_info info{};
    fa_sortformer_chunk k{};
    printf("ST calls %d %d %d %d %d %d %d\n", fa_sortformer_stream_inputs(nullptr, st, &pf, &pi, &pf, &pi), fa_sortformer_stream_get(nullptr, st, 0, &info, f, f, f, f, f),
           fa_sortformer_stream_set(nullptr, st, 0, &info, f, f, f, f, f), fa_sortformer_stream_reset(nullptr, st, -1),
           fa_sortformer_stream_update_dev(nullptr, st, f, FA_DTYPE_F32, i4, f, 1, i4, i4, i4, nullptr, f, f, i4, i4, nullptr),
           fa_sortformer_stream_update(nullptr, st, f, FA_DTYPE_F32, i4, f, 1, i4, i4, i4, nullptr, f, f, i4, i4, nullptr),
           fa_sortformer_stream_pack_chunks_dev(nullptr, &d, f, l4, &k, 1, f));
    c = d; c.speakers = 0;
    l4[0] = -1;
    printf("ST plans %d %d %d %d %d %d %d\n", fa_sortformer_stream_chunk_plan(nullptr, l4, l4, 1, &k), fa_sortformer_stream_chunk_plan(&d, nullptr, l4, 1, &k),
           fa_sortformer_stream_chunk_plan(&d, l4, l4 + 1, 1, &k), fa_sortformer_stream_chunk_plan(&c, l4 + 1, l4 + 1, 1, &k), fa_sortformer_stream_chunk_plan(&d, l4 + 1, l4 + 1, 0, &k),
           fa_sortformer_stream_file_chunks(&d, -1, 0, nullptr, 0, &n, nullptr), fa_sortformer_stream_file_chunks(&d, 10, 10, nullptr, 0, nullptr, nullptr));
    const fa_status small = fa_sortformer_stream_file_chunks(&d, 1000, 1000, &k, 1, &n, nullptr);
    printf("ST small %d %" PRId64 "\n", small, n);
    printf("ST preset %d %d %d\n", fa_sortformer_stream_preset_config(-1, &c), fa_sortformer_stream_preset_config(4, &c), fa_sortformer_stream_preset_config(0, nullptr));
    fa_sortformer_stream_destroy(nullptr);
    fa_sortformer_stream_default_config(nullptr);
    bool threw = false;
    try { (void)fluidaudio::SortformerConfig(17); } catch (const fluidaudio::Error &) { threw = true; }
    printf("THROW %d\n", threw ? 1 : 0);
    return made == nullptr ? 0 : 1;
}
