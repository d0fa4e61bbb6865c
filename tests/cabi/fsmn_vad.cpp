// A C++ host of the FSMN-VAD entries and their Swift-shaped mirror (include/fluidaudio.hpp: FsmnVadSegment, FsmnVadConfig,
// FsmnVadManager), built by tests/test_cabi_fsmn_vad.py with g++ -Werror.  No device is touched: every call here is answered from its
// arguments alone (the context is NULL).
//   LAYOUT name size offsets...     the C structs as the compiler lays them out
//   CFG ...                         fa_fsmn_vad_default_config and the mirror's defaults, the threshold as hex bits
//   ST name status...               the status of every refusal
#include <cinttypes>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "fluidaudio.hpp"

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static void print_cfg(const fa_fsmn_vad_config &c) {
    printf("CFG %08x %d %d %d %d %d %d %d %d\n", bits(c.silence_threshold), c.window_frames, c.sil_to_speech_frames, c.speech_to_sil_frames, c.max_end_silence_frames,
           c.lookback_frames, c.lookahead_frames, c.max_segment_frames, c.frame_ms);
}

int main() {
    printf("LAYOUT config %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_fsmn_vad_config), offsetof(fa_fsmn_vad_config, silence_threshold),
           offsetof(fa_fsmn_vad_config, window_frames), offsetof(fa_fsmn_vad_config, sil_to_speech_frames), offsetof(fa_fsmn_vad_config, speech_to_sil_frames),
           offsetof(fa_fsmn_vad_config, max_end_silence_frames), offsetof(fa_fsmn_vad_config, lookback_frames), offsetof(fa_fsmn_vad_config, lookahead_frames),
           offsetof(fa_fsmn_vad_config, max_segment_frames), offsetof(fa_fsmn_vad_config, frame_ms));
    printf("LAYOUT chunk %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_fsmn_vad_chunk), offsetof(fa_fsmn_vad_chunk, recording), offsetof(fa_fsmn_vad_chunk, bucket),
           offsetof(fa_fsmn_vad_chunk, start_sample), offsetof(fa_fsmn_vad_chunk, end_sample), offsetof(fa_fsmn_vad_chunk, frames), offsetof(fa_fsmn_vad_chunk, keep_from),
           offsetof(fa_fsmn_vad_chunk, first_frame));
    printf("LAYOUT segment %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fa_fsmn_vad_segment), offsetof(fa_fsmn_vad_segment, recording), offsetof(fa_fsmn_vad_segment, reason),
           offsetof(fa_fsmn_vad_segment, start_frame), offsetof(fa_fsmn_vad_segment, end_frame), offsetof(fa_fsmn_vad_segment, start_ms), offsetof(fa_fsmn_vad_segment, end_ms));

    fa_fsmn_vad_config d;
    memset(&d, 0xff, sizeof(d));
    fa_fsmn_vad_default_config(&d);
    print_cfg(d);
    print_cfg(fluidaudio::FsmnVadConfig{}.abi());                                             // the mirror's defaults are the same
    printf("FRAMES %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", fa_fsmn_vad_frame_count(399), fa_fsmn_vad_frame_count(400), fa_fsmn_vad_frame_count(1040),
           fluidaudio::FsmnVadManager::lfrFrameCount(488320));
    int64_t mirror_frames = 0;
    const std::vector<fa_fsmn_vad_chunk> mirror = fluidaudio::FsmnVadManager::chunks(495533, &mirror_frames);
    printf("MIRROR %zu %" PRId64 " %d %d %" PRId64 "\n", mirror.size(), mirror_frames, mirror[1].frames, mirror[1].keep_from, mirror[1].first_frame);

    const float probs[4] = {0.1f, 0.1f, 0.9f, 0.9f};
    const int64_t range[2] = {0, 4}, descending[3] = {0, 3, 2}, negative[2] = {-1, 3}, huge[2] = {0, int64_t{1} << 31};
    fa_fsmn_vad_segment segs[4];
    int64_t count = -7;
    const auto bad_cfg = [&](void (*edit)(fa_fsmn_vad_config &)) {
        fa_fsmn_vad_config c = d;
        edit(c);
        return static_cast<int>(fa_fsmn_vad_segments(nullptr, &c, probs, range, 1, segs, 4, &count, nullptr));
    };
    printf("ST config %d %d %d %d %d %d %d %d %d %d %d %d %d\n", bad_cfg([](fa_fsmn_vad_config &c) { c.silence_threshold = NAN; }),
           bad_cfg([](fa_fsmn_vad_config &c) { c.window_frames = 0; }), bad_cfg([](fa_fsmn_vad_config &c) { c.window_frames = 65; }),
           bad_cfg([](fa_fsmn_vad_config &c) { c.sil_to_speech_frames = 21; }), bad_cfg([](fa_fsmn_vad_config &c) { c.sil_to_speech_frames = -1; }),
           bad_cfg([](fa_fsmn_vad_config &c) { c.speech_to_sil_frames = 21; }), bad_cfg([](fa_fsmn_vad_config &c) { c.speech_to_sil_frames = -1; }),
           bad_cfg([](fa_fsmn_vad_config &c) { c.max_end_silence_frames = 0; }), bad_cfg([](fa_fsmn_vad_config &c) { c.max_segment_frames = 0; }),
           bad_cfg([](fa_fsmn_vad_config &c) { c.frame_ms = 0; }), bad_cfg([](fa_fsmn_vad_config &c) { c.lookback_frames = -1; }),
           bad_cfg([](fa_fsmn_vad_config &c) { c.lookahead_frames = -1; }), bad_cfg([](fa_fsmn_vad_config &) {}));   // the last: a good config reaches the missing context
    printf("ST segments %d %d %d %d %d %d %d %d\n", fa_fsmn_vad_segments(nullptr, nullptr, probs, range, -1, segs, 4, &count, nullptr),
           fa_fsmn_vad_segments(nullptr, nullptr, probs, range, 1, segs, -1, &count, nullptr), fa_fsmn_vad_segments(nullptr, nullptr, probs, range, 1, segs, 4, nullptr, nullptr),
           fa_fsmn_vad_segments(nullptr, nullptr, probs, nullptr, 1, segs, 4, &count, nullptr), fa_fsmn_vad_segments(nullptr, nullptr, probs, descending, 2, segs, 4, &count, nullptr),
           fa_fsmn_vad_segments(nullptr, nullptr, probs, negative, 1, segs, 4, &count, nullptr), fa_fsmn_vad_segments(nullptr, nullptr, nullptr, range, 1, segs, 4, &count, nullptr),
           fa_fsmn_vad_segments_dev(nullptr, nullptr, probs, huge, 1, segs, 4, &count, nullptr));
    printf("COUNT %" PRId64 "\n", count);                                                     // a refusal writes nothing

    // the schedule: the ranges are written before the capacity is judged
    const int64_t totals[2] = {495533, 300};
    fa_fsmn_vad_chunk chunks[4];
    int64_t chunk_range[3] = {-1, -1, -1}, frame_range[3] = {-1, -1, -1}, n = -1;
    printf("ST plan %d %d %d %d", fa_fsmn_vad_plan_chunks(totals, -1, chunks, 4, &n, chunk_range, frame_range), fa_fsmn_vad_plan_chunks(totals, 2, chunks, 4, nullptr, chunk_range, frame_range),
           fa_fsmn_vad_plan_chunks(nullptr, 2, chunks, 4, &n, chunk_range, frame_range), fa_fsmn_vad_plan_chunks(totals, 2, chunks, 1, &n, chunk_range, frame_range));
    printf(" | %" PRId64 " | %" PRId64 " %" PRId64 " %" PRId64 " | %" PRId64 " %" PRId64 " %" PRId64 " | %" PRId64 "\n", n, chunk_range[0], chunk_range[1], chunk_range[2], frame_range[0],
           frame_range[1], frame_range[2], chunks[0].end_sample);
    const int empty = fa_fsmn_vad_plan_chunks(nullptr, 0, nullptr, 0, &n, nullptr, nullptr);       // batch == 0: SUCCESS, and the count is set
    printf("ST plan0 %d %" PRId64 "\n", empty, n);

    float audio[2000] = {}, rows[4000];
    const int64_t offsets[3] = {0, 1500, 2000};
    const fa_fsmn_vad_chunk good[2] = {{0, 512, 0, 1500, 5, 0, 0}, {1, 512, 0, 500, 0, 0, 0}}, outside[1] = {{2, 512, 0, 10, 0, 0, 0}}, beyond[1] = {{1, 512, 0, 501, 0, 0, 0}},
                            backwards[1] = {{0, 512, 10, 5, 0, 0, 0}};
    printf("ST pack %d %d %d %d %d %d %d %d %d\n", fa_fsmn_vad_pack_waveforms(nullptr, audio, offsets, -1, good, 2, rows, 1500, 2), fa_fsmn_vad_pack_waveforms(nullptr, audio, nullptr, 2, good, 2, rows, 1500, 2),
           fa_fsmn_vad_pack_waveforms(nullptr, audio, offsets, 2, nullptr, 2, rows, 1500, 2), fa_fsmn_vad_pack_waveforms(nullptr, audio, offsets, 2, outside, 1, rows, 1500, 2),
           fa_fsmn_vad_pack_waveforms(nullptr, audio, offsets, 2, beyond, 1, rows, 1500, 2), fa_fsmn_vad_pack_waveforms(nullptr, audio, offsets, 2, backwards, 1, rows, 1500, 2),
           fa_fsmn_vad_pack_waveforms(nullptr, audio, offsets, 2, good, 2, rows, 1499, 2),                      // row_stride below the longest chunk
           fa_fsmn_vad_pack_waveforms(nullptr, nullptr, offsets, 2, good, 2, rows, 1500, 2), fa_fsmn_vad_pack_waveforms_dev(nullptr, audio, offsets, 2, good, 2, rows, 1500, 1));
    const fa_fsmn_vad_chunk large[1] = {{0, 1024, 0, 100000, 513, 0, 0}};
    printf("ST feats %d %d %d %d %d\n", fa_fsmn_vad_pack_feats_dev(nullptr, audio, 7, 600, good, 2, 512, rows), fa_fsmn_vad_pack_feats_dev(nullptr, audio, FA_DTYPE_F32, 600, large, 1, 512, rows),
           fa_fsmn_vad_pack_feats_dev(nullptr, audio, FA_DTYPE_F16, 512, large, 1, 1024, rows), fa_fsmn_vad_pack_feats_dev(nullptr, nullptr, FA_DTYPE_F32, 600, good, 2, 512, rows),
           fa_fsmn_vad_pack_feats_dev(nullptr, audio, FA_DTYPE_F32, 600, good, 2, 512, rows));              // the last: sound arguments reach the missing context
    const int64_t frames2[3] = {0, 5, 5}, short2[3] = {0, 4, 4};
    printf("ST gather %d %d %d %d %d %d\n", fa_fsmn_vad_gather_silence_dev(nullptr, audio, FA_DTYPE_F32, 512, 0, good, 2, frames2, 2, rows, 5),
           fa_fsmn_vad_gather_silence_dev(nullptr, audio, FA_DTYPE_F32, 512, 2, good, 2, nullptr, 2, rows, 5), fa_fsmn_vad_gather_silence_dev(nullptr, audio, FA_DTYPE_F32, 512, 2, outside, 1, frames2, 2, rows, 5),
           fa_fsmn_vad_gather_silence_dev(nullptr, audio, FA_DTYPE_F32, 512, 2, good, 2, short2, 2, rows, 5),      // the chunk ends beyond its recording's frames
           fa_fsmn_vad_gather_silence_dev(nullptr, audio, FA_DTYPE_F32, 4, 2, good, 2, frames2, 2, rows, 5), fa_fsmn_vad_gather_silence_dev(nullptr, audio, FA_DTYPE_F32, 512, 2, good, 2, frames2, 2, rows, 4));
    // the mirror throws what the entry answered
    try {
        fluidaudio::FsmnVadConfig c;
        c.windowFrames = 65;
        const fa_fsmn_vad_config abi = c.abi();
        const fa_status st = fa_fsmn_vad_segments(nullptr, &abi, probs, range, 1, segs, 4, &count, nullptr);
        if (st != FA_SUCCESS) throw fluidaudio::Error(st, "fa_fsmn_vad_segments");
        printf("THROW none\n");
    } catch (const fluidaudio::Error &e) {
        printf("THROW %d\n", static_cast<int>(e.status));
    }
    return 0;
}
