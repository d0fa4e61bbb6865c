// A C++ host of the VAD entries and their Swift-shaped mirror (include/fluidaudio.hpp: VadConfig, VadSegmentationConfig, VadSegment,
// VadStreamState, VadStreamEvent), built by tests/test_cabi_vad.py with g++ -Werror.  No device is touched: every call here is answered
// from its arguments alone (the context is NULL).
//   LAYOUT name size offsets...     the C structs as the compiler lays them out
//   CFG ...                         fa_vad_default_config and the mirror's defaults, floats and doubles as hex bits
//   ST name status...               the status of every refusal
#include <cinttypes>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>

#include "fluidaudio.hpp"

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

static void print_cfg(const char *tag, const fa_vad_segmentation_config &c) {
    printf("%s %08x %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %08x %d %08x %08x %016" PRIx64 " %d\n", tag, bits(c.default_threshold), bits(c.min_speech_duration),
           bits(c.min_silence_duration), bits(c.max_speech_duration), bits(c.speech_padding), bits(c.silence_threshold_for_split), c.has_negative_threshold,
           bits(c.negative_threshold), bits(c.negative_threshold_offset), bits(c.min_silence_at_max_speech), c.use_max_possible_silence_at_max_speech);
}

int main() {
    printf("LAYOUT config %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_vad_segmentation_config), offsetof(fa_vad_segmentation_config, default_threshold),
           offsetof(fa_vad_segmentation_config, min_speech_duration), offsetof(fa_vad_segmentation_config, min_silence_duration), offsetof(fa_vad_segmentation_config, max_speech_duration),
           offsetof(fa_vad_segmentation_config, speech_padding), offsetof(fa_vad_segmentation_config, silence_threshold_for_split),
           offsetof(fa_vad_segmentation_config, has_negative_threshold), offsetof(fa_vad_segmentation_config, negative_threshold),
           offsetof(fa_vad_segmentation_config, negative_threshold_offset), offsetof(fa_vad_segmentation_config, min_silence_at_max_speech),
           offsetof(fa_vad_segmentation_config, use_max_possible_silence_at_max_speech));
    printf("LAYOUT segment %zu %zu %zu %zu %zu %zu\n", sizeof(fa_vad_segment), offsetof(fa_vad_segment, recording), offsetof(fa_vad_segment, start_sample),
           offsetof(fa_vad_segment, end_sample), offsetof(fa_vad_segment, start_time), offsetof(fa_vad_segment, end_time));
    printf("LAYOUT state %zu %zu %zu %zu %zu\n", sizeof(fa_vad_stream_state), offsetof(fa_vad_stream_state, triggered), offsetof(fa_vad_stream_state, has_temp_end),
           offsetof(fa_vad_stream_state, temp_end_sample), offsetof(fa_vad_stream_state, processed_samples));
    printf("LAYOUT event %zu %zu %zu %zu %zu %zu\n", sizeof(fa_vad_stream_event), offsetof(fa_vad_stream_event, stream), offsetof(fa_vad_stream_event, chunk),
           offsetof(fa_vad_stream_event, kind), offsetof(fa_vad_stream_event, sample_index), offsetof(fa_vad_stream_event, time));

    fa_vad_segmentation_config d;
    memset(&d, 0xff, sizeof(d));
    fa_vad_default_config(&d);
    print_cfg("CFG", d);
    print_cfg("CFG", fluidaudio::VadSegmentationConfig{}.abi());                                // the mirror's defaults are the same
    fluidaudio::VadSegmentationConfig m;
    m.negativeThreshold = 0.2f; m.negativeThresholdOffset = 0.05f; m.maxSpeechDuration = std::numeric_limits<double>::infinity();
    print_cfg("CFG", m.abi(fluidaudio::VadConfig{0.8f}));
    printf("NEG %08x %08x\n", bits(fluidaudio::VadSegmentationConfig{}.effectiveNegativeThreshold(0.85f)), bits(m.effectiveNegativeThreshold(0.85f)));
    const fluidaudio::VadSegment seg{1001.0 / 16000.0, 2000.0 / 16000.0};
    printf("SEG %" PRId64 " %" PRId64 " %" PRId64 "\n", seg.startSample(16000), seg.endSample(16000), seg.sampleCount(16000));
    printf("CHUNKS %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", fa_vad_chunk_count(-5), fa_vad_chunk_count(0), fa_vad_chunk_count(1), fa_vad_chunk_count(4096),
           fa_vad_chunk_count(4097));

    const float probs[4] = {0.9f, 0.1f, 0.9f, 0.9f};
    const int64_t range[2] = {0, 4}, total[1] = {4 * 4096}, descending[3] = {0, 3, 2}, negative[2] = {-1, 3}, huge[2] = {0, int64_t{1} << 31}, totals2[2] = {9, 9};
    fa_vad_segment segs[4];
    int64_t count = -7, counts[2];
    const auto bad_cfg = [&](void (*edit)(fa_vad_segmentation_config &)) {
        fa_vad_segmentation_config c = d;
        edit(c);
        return static_cast<int>(fa_vad_segments(nullptr, &c, probs, range, total, 1, segs, 4, &count, nullptr));
    };
    printf("ST config %d %d %d %d %d %d %d %d %d %d %d %d\n", bad_cfg([](fa_vad_segmentation_config &c) { c.min_speech_duration = -1; }),
           bad_cfg([](fa_vad_segmentation_config &c) { c.min_silence_duration = -1; }), bad_cfg([](fa_vad_segmentation_config &c) { c.max_speech_duration = 0; }),
           bad_cfg([](fa_vad_segmentation_config &c) { c.speech_padding = -1; }), bad_cfg([](fa_vad_segmentation_config &c) { c.silence_threshold_for_split = 1.5f; }),
           bad_cfg([](fa_vad_segmentation_config &c) { c.negative_threshold_offset = -1; }), bad_cfg([](fa_vad_segmentation_config &c) { c.min_silence_at_max_speech = -1; }),
           bad_cfg([](fa_vad_segmentation_config &c) { c.has_negative_threshold = 1; c.negative_threshold = 2; }), bad_cfg([](fa_vad_segmentation_config &c) { c.speech_padding = NAN; }),
           bad_cfg([](fa_vad_segmentation_config &c) { c.min_silence_duration = 1e300; }), bad_cfg([](fa_vad_segmentation_config &c) { c.max_speech_duration = 1e300; }),
           bad_cfg([](fa_vad_segmentation_config &) {}));                                       // the last: a good config reaches the missing context
    printf("ST segments %d %d %d %d %d %d %d %d %d\n", fa_vad_segments(nullptr, nullptr, probs, range, total, -1, segs, 4, &count, nullptr),
           fa_vad_segments(nullptr, nullptr, probs, range, total, 1, segs, -1, &count, nullptr), fa_vad_segments(nullptr, nullptr, probs, range, total, 1, segs, 4, nullptr, nullptr),
           fa_vad_segments(nullptr, nullptr, probs, nullptr, total, 1, segs, 4, &count, nullptr), fa_vad_segments(nullptr, nullptr, probs, range, nullptr, 1, segs, 4, &count, nullptr),
           fa_vad_segments(nullptr, nullptr, probs, descending, totals2, 2, segs, 4, &count, counts), fa_vad_segments(nullptr, nullptr, probs, negative, total, 1, segs, 4, &count, nullptr),
           fa_vad_segments(nullptr, nullptr, nullptr, range, total, 1, segs, 4, &count, nullptr), fa_vad_segments_dev(nullptr, nullptr, probs, huge, total, 1, segs, 4, &count, nullptr));
    printf("COUNT %" PRId64 "\n", count);                                                       // a refusal writes nothing

    float rows[4160];
    int64_t chunk_range[3] = {-1, -1, -1}, out_range[3] = {-1, -1, -1};
    const int64_t offsets[3] = {0, 10, 4106};
    printf("ST pack %d %d %d %d %d %d", fa_vad_pack_chunks(nullptr, probs, offsets, -1, rows, 1, chunk_range), fa_vad_pack_chunks(nullptr, probs, nullptr, 2, rows, 1, chunk_range),
           fa_vad_pack_chunks(nullptr, probs, offsets, 2, rows, 1, nullptr), fa_vad_pack_chunks(nullptr, probs, descending, 2, rows, 9, chunk_range),
           fa_vad_pack_chunks(nullptr, nullptr, offsets, 2, rows, 9, chunk_range), fa_vad_pack_chunks_dev(nullptr, probs, offsets, 2, rows, 1, chunk_range));
    printf(" | %" PRId64 " %" PRId64 " %" PRId64 "\n", chunk_range[0], chunk_range[1], chunk_range[2]);
    const fa_vad_segment good[2] = {{0, 0, 0, 0, 0.0, 5.0 / 16000.0}, {1, 0, 0, 0, 0.0, 1.0}}, outside[1] = {{2, 0, 0, 0, 0.0, 1.0}}, nan_time[1] = {{0, 0, 0, 0, NAN, 1.0}};
    float out[16];
    printf("ST gather %d %d %d %d %d %d %d", fa_vad_gather_segments(nullptr, probs, offsets, 2, good, 2, out, 16, nullptr), fa_vad_gather_segments(nullptr, probs, offsets, 2, good, -1, out, 16, out_range),
           fa_vad_gather_segments(nullptr, probs, nullptr, 2, good, 2, out, 16, out_range), fa_vad_gather_segments(nullptr, probs, offsets, 2, nullptr, 2, out, 16, out_range),
           fa_vad_gather_segments(nullptr, probs, offsets, 2, outside, 1, out, 16, out_range), fa_vad_gather_segments(nullptr, probs, offsets, 2, nan_time, 1, out, 16, out_range),
           fa_vad_gather_segments_dev(nullptr, probs, offsets, 2, good, 2, out, 16, out_range));
    printf(" | %" PRId64 " %" PRId64 " %" PRId64 "\n", out_range[0], out_range[1], out_range[2]);
    fa_vad_stream_state states[2] = {};
    fa_vad_stream_event events[4];
    const int32_t two[2] = {2, 2}, three[2] = {3, 0}, minus[2] = {-1, 0};
    const auto stream = [&](const int32_t *chunk_counts, int32_t resolution, int64_t capacity, int64_t *cnt, const float *p) {
        return static_cast<int>(fa_vad_stream_advance(nullptr, nullptr, p, chunk_counts, nullptr, 2, 2, states, 1, resolution, events, capacity, cnt));
    };
    printf("ST stream %d %d %d %d %d %d %d %d %d\n", stream(two, -1, 4, &count, probs), stream(two, 23, 4, &count, probs), stream(three, 1, 4, &count, probs), stream(minus, 1, 4, &count, probs),
           stream(two, 1, -1, &count, probs), stream(two, 1, 4, nullptr, probs), stream(nullptr, 1, 4, &count, probs), stream(two, 1, 4, &count, nullptr), stream(two, 22, 4, &count, probs));
    // the mirror throws what the entry answered
    try {
        fluidaudio::VadSegmentationConfig c;
        c.speechPadding = -1.0;
        const fa_vad_segmentation_config abi = c.abi();
        const fa_status st = fa_vad_segments(nullptr, &abi, probs, range, total, 1, segs, 4, &count, nullptr);
        if (st != FA_SUCCESS) throw fluidaudio::Error(st, "fa_vad_segments");
        printf("THROW none\n");
    } catch (const fluidaudio::Error &e) {
        printf("THROW %d\n", static_cast<int>(e.status));
    }
    return 0;
}
