// The argument pass and the plans of the VAD entries (fluidaudio_amd/csrc/vad_launch.h: the operands the reference derives from a config,
// every refusal of a call, the offsets and workspace sizes vad_host.hip sizes its buffers with) driven over stdin: one call per line.
// Test infrastructure: built by tests/test_vad_plan.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
// Doubles and floats travel as hex bits.  cfg is 11 words: default_threshold(f32) min_speech min_silence max_speech padding (f64)
// split_threshold(f32) has_negative negative(f32) offset(f32) min_silence_at_max(f64) use_max.
//   derive cfg                       -> "0 | thr neg split | min_speech pad max_speech min_silence min_silence_at_max use_max"
//   seg cfg device have_probs have_segs capacity have_count B have_ranges range[B + 1] total[B]
//                                    -> "0 | frames raw_slots out_slots | B x (frame0 raw0 frames total)"
//   pack have_audio have_rows row_capacity B have_offsets offsets[B + 1]
//                                    -> "status | text | chunk_range[B + 1]" (the ranges as far as they were written, '-' otherwise)
//   gather device out_capacity B offsets[B + 1] N N x (recording start_time end_time)
//                                    -> "status | text | out_range[N + 1] | src[N] | tile_off[N + 1]"
//   stream cfg S K resolution capacity have_probs have_count counts[S]
//                                    -> "0 | factor"
// A refusal prints "status | text".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/vad_launch.h"

namespace vd = fa::vad;

static bool word(char *w) { return scanf("%63s", w) == 1; }
static int64_t i64() { char w[64]; if (!word(w)) exit(2); return strtoll(w, nullptr, 10); }
static double f64() { char w[64]; if (!word(w)) exit(2); uint64_t b = strtoull(w, nullptr, 16); double d; memcpy(&d, &b, 8); return d; }
static float f32() { char w[64]; if (!word(w)) exit(2); uint32_t b = static_cast<uint32_t>(strtoul(w, nullptr, 16)); float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

static fa_vad_segmentation_config config() {
    fa_vad_segmentation_config c;
    memset(&c, 0, sizeof(c));
    c.default_threshold = f32();
    c.min_speech_duration = f64(); c.min_silence_duration = f64(); c.max_speech_duration = f64(); c.speech_padding = f64();
    c.silence_threshold_for_split = f32();
    c.has_negative_threshold = static_cast<int32_t>(i64());
    c.negative_threshold = f32(); c.negative_threshold_offset = f32();
    c.min_silence_at_max_speech = f64();
    c.use_max_possible_silence_at_max_speech = static_cast<int32_t>(i64());
    return c;
}

static bool refused(const fa::Verdict &v) {
    if (v.status == FA_SUCCESS) return false;
    printf("%d | %s\n", static_cast<int>(v.status), v.text);
    return true;
}

// exactly n entries: the sanitizers watch the plan's reads
static std::vector<int64_t> list(const int64_t n) {
    std::vector<int64_t> v(static_cast<size_t>(n > 0 ? n : 0));
    for (int64_t &x : v) x = i64();
    return v;
}

int main() {
    char cmd[64];
    int dummy = 0;
    while (word(cmd)) {
        if (!strcmp(cmd, "derive")) {
            vd::Operands o{};
            if (refused(vd::derive(config(), &o))) continue;
            printf("0 | %08x %08x %08x | %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", bits(o.threshold), bits(o.negative_threshold), bits(o.split_threshold),
                   o.min_speech, o.pad, o.max_speech, o.min_silence, o.min_silence_at_max, o.use_max);
        } else if (!strcmp(cmd, "seg")) {
            const fa_vad_segmentation_config c = config();
            const bool device = i64(), have_probs = i64(), have_segs = i64();
            const int64_t capacity = i64();
            const bool have_count = i64();
            const int32_t B = static_cast<int32_t>(i64());
            const bool have_ranges = i64();
            const std::vector<int64_t> range = have_ranges ? list(static_cast<int64_t>(B) + 1) : std::vector<int64_t>(), total = have_ranges ? list(B) : std::vector<int64_t>();
            vd::Operands o{};
            vd::SegPlan p;
            if (refused(vd::plan_segments(c, have_probs ? &dummy : nullptr, have_ranges ? range.data() : nullptr, have_ranges ? total.data() : nullptr, B, have_segs ? &dummy : nullptr,
                                          capacity, have_count ? &dummy : nullptr, device, &o, &p)))
                continue;
            printf("0 | %" PRId64 " %" PRId64 " %" PRId64 " |", p.frames, p.raw_slots, p.out_slots);
            for (const vd::SegRecording &r : p.rec) printf(" %" PRId64 " %" PRId64 " %d %" PRId64, r.frame0, r.raw0, r.frames, r.total);
            printf("\n");
        } else if (!strcmp(cmd, "pack")) {
            const bool have_audio = i64(), have_rows = i64();
            const int64_t row_capacity = i64();
            const int32_t B = static_cast<int32_t>(i64());
            const bool have_offsets = i64();
            const std::vector<int64_t> offsets = have_offsets ? list(static_cast<int64_t>(B) + 1) : std::vector<int64_t>();
            std::vector<int64_t> chunk_range(static_cast<size_t>(B > 0 ? B : 0) + 1, -1);
            const fa::Verdict v = vd::plan_pack(have_audio ? &dummy : nullptr, have_offsets ? offsets.data() : nullptr, B, have_rows ? &dummy : nullptr, row_capacity, chunk_range.data());
            printf("%d | %s |", static_cast<int>(v.status), v.text);
            for (const int64_t x : chunk_range) printf(" %" PRId64, x);
            printf("\n");
        } else if (!strcmp(cmd, "gather")) {
            const bool device = i64();
            const int64_t out_capacity = i64();
            const int32_t B = static_cast<int32_t>(i64());
            const std::vector<int64_t> offsets = list(static_cast<int64_t>(B) + 1);
            const int64_t N = i64();
            std::vector<fa_vad_segment> segs(static_cast<size_t>(N > 0 ? N : 0));
            for (fa_vad_segment &s : segs) {
                memset(&s, 0, sizeof(s));
                s.recording = static_cast<int32_t>(i64());
                s.start_time = f64(); s.end_time = f64();
            }
            std::vector<int64_t> out_range(segs.size() + 1, -1);
            vd::GatherPlan p;
            const fa::Verdict v = vd::plan_gather(&dummy, offsets.data(), B, segs.data(), N, &dummy, out_capacity, out_range.data(), device, &p);
            printf("%d | %s |", static_cast<int>(v.status), v.text);
            for (const int64_t x : out_range) printf(" %" PRId64, x);
            printf(" |");
            for (const int64_t x : p.src) printf(" %" PRId64, x);
            printf(" |");
            for (const int64_t x : p.tile_off) printf(" %" PRId64, x);
            printf("\n");
        } else if (!strcmp(cmd, "stream")) {
            const fa_vad_segmentation_config c = config();
            const int32_t S = static_cast<int32_t>(i64()), K = static_cast<int32_t>(i64()), resolution = static_cast<int32_t>(i64());
            const int64_t capacity = i64();
            const bool have_probs = i64(), have_count = i64();
            const std::vector<int64_t> wide = list(S);
            const std::vector<int32_t> counts(wide.begin(), wide.end());
            const std::vector<fa_vad_stream_state> states(counts.size());
            vd::Operands o{};
            if (refused(vd::plan_stream(c, have_probs ? &dummy : nullptr, counts.data(), S, K, states.data(), resolution, &dummy, capacity, have_count ? &dummy : nullptr, &o))) continue;
            printf("0 | %016" PRIx64 "\n", bits(vd::resolution_factor(resolution)));
        } else {
            return 2;
        }
    }
    return 0;
}
