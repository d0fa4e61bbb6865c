// A C++ host of the TDT window-planner entries and their Swift-shaped mirror (include/fluidaudio.hpp: ChunkLayout, ChunkStartDecision,
// TdtWindowPlanner), built by tests/test_cabi_tdt_plan.py with g++ -Werror.  No device is touched: every call here is answered from its
// arguments alone (the context is NULL).
//   LAYOUT name size offsets...     the C structs as the compiler lays them out
//   CFG ...                         fa_tdt_window_default_config and the mirror's defaults, the double as hex bits
//   CHUNKS ...                      fa_tdt_window_layout and the mirror's chunkLayout
//   BOUND ...                       fa_tdt_window_count_bound
//   ST name status...               the status of every refusal
#include <cinttypes>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>

#include "fluidaudio.hpp"

static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

static void print_cfg(const fa_tdt_window_config &c) {
    printf("CFG %d %d %d %d %016" PRIx64 " %d %d %d %d\n", c.sample_rate, c.frame_samples, c.mel_hop, c.max_model_samples, bits(c.overlap_seconds), c.mel_chunk_context,
           c.silence_aligned, c.warmup_prefix_frames, c.end_aligned);
}

int main() {
    printf("LAYOUT config %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_tdt_window_config), offsetof(fa_tdt_window_config, sample_rate),
           offsetof(fa_tdt_window_config, frame_samples), offsetof(fa_tdt_window_config, mel_hop), offsetof(fa_tdt_window_config, max_model_samples),
           offsetof(fa_tdt_window_config, overlap_seconds), offsetof(fa_tdt_window_config, mel_chunk_context), offsetof(fa_tdt_window_config, silence_aligned),
           offsetof(fa_tdt_window_config, warmup_prefix_frames), offsetof(fa_tdt_window_config, end_aligned));
    printf("LAYOUT window %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_tdt_window), offsetof(fa_tdt_window, recording),
           offsetof(fa_tdt_window, use_warmup_prefix), offsetof(fa_tdt_window, is_last), offsetof(fa_tdt_window, emit_after_frame), offsetof(fa_tdt_window, global_frame_offset),
           offsetof(fa_tdt_window, context_frames), offsetof(fa_tdt_window, actual_audio_frames), offsetof(fa_tdt_window, reserved), offsetof(fa_tdt_window, chunk_start),
           offsetof(fa_tdt_window, warmup_samples), offsetof(fa_tdt_window, context_samples), offsetof(fa_tdt_window, context_start), offsetof(fa_tdt_window, length));
    printf("LAYOUT span %zu %zu %zu %zu\n", sizeof(fa_tdt_span), offsetof(fa_tdt_span, recording), offsetof(fa_tdt_span, from_sample), offsetof(fa_tdt_span, to_sample));

    fa_tdt_window_config d;
    memset(&d, 0xff, sizeof(d));
    fa_tdt_window_default_config(&d);
    print_cfg(d);
    print_cfg(fluidaudio::TdtWindowPlanner{}.abi());                                            // the mirror's defaults are the same
    fluidaudio::TdtWindowPlanner path_b;
    path_b.melChunkContext = false; path_b.silenceAligned = true; path_b.warmupPrefixFrames = 7;
    print_cfg(path_b.abi());
    int64_t l[4];
    fa_tdt_window_layout(nullptr, &l[0], &l[1], &l[2], &l[3]);
    printf("CHUNKS %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", l[0], l[1], l[2], l[3]);
    const fluidaudio::ChunkLayout m = path_b.chunkLayout();
    printf("CHUNKS %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", m.chunkSamples, m.strideSamples, m.melContextSamples, m.warmupPrefixSamples);
    const fa_tdt_window_config b = path_b.abi();
    fa_tdt_window_config refused = d;
    refused.frame_samples = 0;
    printf("BOUND %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", fa_tdt_window_count_bound(nullptr, -3),
           fa_tdt_window_count_bound(nullptr, 0), fa_tdt_window_count_bound(nullptr, 1), fa_tdt_window_count_bound(nullptr, 206080), fa_tdt_window_count_bound(nullptr, 206081),
           fa_tdt_window_count_bound(&b, 207360), fa_tdt_window_count_bound(&b, 207361), fa_tdt_window_count_bound(&refused, 5));

    const float audio[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t offsets[3] = {0, 3, 8}, descending[3] = {0, 5, 4}, negative[3] = {-1, 3, 8}, huge[2] = {0, int64_t{1280} * 2147483646};
    fa_tdt_window windows[4];
    int64_t window_range[3] = {-7, -7, -7};
    const auto bad_cfg = [&](void (*edit)(fa_tdt_window_config &)) {
        fa_tdt_window_config c = d;
        edit(c);
        return static_cast<int>(fa_tdt_plan_windows(nullptr, &c, audio, offsets, 2, windows, 4, window_range, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    };
    printf("ST config %d %d %d %d %d %d %d %d %d %d %d %d\n", bad_cfg([](fa_tdt_window_config &c) { c.sample_rate = 0; }), bad_cfg([](fa_tdt_window_config &c) { c.frame_samples = -1; }),
           bad_cfg([](fa_tdt_window_config &c) { c.mel_hop = 0; }), bad_cfg([](fa_tdt_window_config &c) { c.max_model_samples = 0; }),
           bad_cfg([](fa_tdt_window_config &c) { c.warmup_prefix_frames = -1; }), bad_cfg([](fa_tdt_window_config &c) { c.overlap_seconds = NAN; }),
           bad_cfg([](fa_tdt_window_config &c) { c.overlap_seconds = std::numeric_limits<double>::infinity(); }), bad_cfg([](fa_tdt_window_config &c) { c.overlap_seconds = -0.5; }),
           bad_cfg([](fa_tdt_window_config &c) { c.max_model_samples = 6 * 1280 + 160; }),     // a chunk of six frames does not exceed the six-frame overlap
           bad_cfg([](fa_tdt_window_config &c) { c.frame_samples = 1000; }),                   // a search radius of 64 frames
           bad_cfg([](fa_tdt_window_config &c) { c.max_model_samples = 8 * 1280; c.mel_chunk_context = 0; c.warmup_prefix_frames = 7; }),
           bad_cfg([](fa_tdt_window_config &) {}));                                            // the last: a good config reaches the missing context
    const auto plan = [&](const float *a, const int64_t *off, int32_t batch, fa_tdt_window *w, int64_t capacity, int64_t *range, bool device) {
        return static_cast<int>((device ? fa_tdt_plan_windows_dev : fa_tdt_plan_windows)(nullptr, nullptr, a, off, batch, w, capacity, range, nullptr, nullptr, nullptr, nullptr,
                                                                                          nullptr, nullptr, nullptr));
    };
    printf("ST plan %d %d %d %d %d %d %d %d %d\n", plan(audio, offsets, -1, windows, 4, window_range, false), plan(audio, offsets, 2, windows, -1, window_range, false),
           plan(audio, offsets, 2, nullptr, 4, window_range, false), plan(audio, nullptr, 2, windows, 4, window_range, false), plan(audio, offsets, 2, windows, 4, nullptr, false),
           plan(audio, descending, 2, windows, 4, window_range, false), plan(audio, negative, 2, windows, 4, window_range, true), plan(nullptr, offsets, 2, windows, 4, window_range, false),
           plan(audio, huge, 1, windows, 4, window_range, true));
    printf("RANGE %" PRId64 " %" PRId64 " %" PRId64 "\n", window_range[0], window_range[1], window_range[2]);   // a refusal writes nothing

    float rows[4];
    const fa_tdt_window good[2] = {{0, 0, 1, -1, 0, 0, 1, 0, 0, 0, 0, 0, 3}, {1, 0, 1, -1, 0, 0, 1, 0, 0, 0, 0, 1, 4}}, outside[1] = {{2, 0, 1, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1}},
                        beyond[1] = {{0, 0, 1, -1, 0, 0, 1, 0, 0, 0, 0, 2, 2}}, before[1] = {{1, 0, 1, -1, 0, 0, 1, 0, 0, 0, 0, -1, 2}};
    const auto pack = [&](const float *a, const int64_t *off, int32_t batch, const fa_tdt_window *w, int64_t n, float *r, int64_t capacity, bool device) {
        return static_cast<int>((device ? fa_tdt_pack_windows_dev : fa_tdt_pack_windows)(nullptr, nullptr, a, off, batch, w, n, r, capacity, nullptr));
    };
    printf("ST pack %d %d %d %d %d %d %d %d %d %d %d\n", pack(audio, offsets, -1, good, 2, rows, 2, false), pack(audio, offsets, 2, good, -1, rows, 2, false),
           pack(audio, offsets, 2, good, 2, rows, -1, false), pack(audio, nullptr, 2, good, 2, rows, 2, false), pack(audio, offsets, 2, nullptr, 2, rows, 2, false),
           pack(audio, offsets, 2, outside, 1, rows, 2, false), pack(audio, offsets, 2, beyond, 1, rows, 2, true), pack(audio, offsets, 2, before, 1, rows, 2, false),
           pack(audio, offsets, 2, good, 2, nullptr, 2, false), pack(nullptr, offsets, 2, good, 2, rows, 2, true), pack(audio, offsets, 2, good, 2, rows, 1, true));

    const fa_tdt_span spans[2] = {{0, 0, 0, 3}, {1, 0, 1, 5}}, other[1] = {{2, 0, 0, 1}}, early[1] = {{0, 0, -1, 2}}, late[1] = {{0, 0, 0, 4}};
    float thresholds[2] = {-7.0f, -7.0f};
    int64_t frames[2];
    const auto gate = [&](const float *a, const int64_t *off, int32_t batch, const fa_tdt_span *s, int64_t n, bool device) {
        return static_cast<int>((device ? fa_tdt_speech_gate_dev : fa_tdt_speech_gate)(nullptr, nullptr, a, off, batch, nullptr, thresholds, s, n, frames, nullptr, nullptr));
    };
    printf("ST gate %d %d %d %d %d %d %d %d %d %d\n", gate(audio, offsets, -1, spans, 2, false), gate(audio, offsets, 2, spans, -1, false), gate(audio, nullptr, 2, spans, 2, false),
           gate(audio, descending, 2, spans, 2, true), gate(audio, offsets, 2, nullptr, 2, false), gate(audio, offsets, 2, other, 1, false), gate(audio, offsets, 2, early, 1, true),
           gate(audio, offsets, 2, late, 1, false), gate(nullptr, offsets, 2, spans, 2, false), gate(audio, offsets, 0, spans, 1, false));
    printf("THR %d\n", static_cast<int>(thresholds[0]));
    // the mirror throws what the entry answered
    try {
        fluidaudio::TdtWindowPlanner p;
        p.overlapSeconds = -1.0;
        (void)p.chunkLayout();
        printf("THROW none\n");
    } catch (const fluidaudio::Error &e) {
        printf("THROW %d\n", static_cast<int>(e.status));
    }
    return 0;
}
