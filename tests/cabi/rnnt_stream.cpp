// A C++ caller of NemotronStreamConfig / NemotronStreamSession (include/fluidaudio.hpp) and of the fa_rnnt_stream_* entries, built with
// -Wall -Wextra -Werror by tests/test_cabi_rnnt_stream.py.  Without an argument: layouts, defaults and every refusal that needs no
// device.  "device": the refusals that name their bound, and one pass of gate, track and merge through the mirror.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fluidaudio.hpp"

using namespace fluidaudio;

static uint32_t bits(const float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

// the test's audio: a window is loud (0.05 * a sawtooth) or silent (0.0005 * the same)
static std::vector<float> audio(const std::string &pattern, const int window) {
    std::vector<float> x;
    uint32_t s = 12345;
    for (const char ch : pattern)
        for (int i = 0; i < window; ++i) {
            s = s * 1664525u + 1013904223u;
            x.push_back((static_cast<float>(s >> 8) / 8388608.0f - 1.0f) * (ch == '1' ? 0.05f : 0.0005f));
        }
    return x;
}

static int device() {
    Context ctx(0);
    fa_rnnt_stream *st = nullptr;
    NemotronStreamConfig cfg(65);
    // refusals with their bound in the text
    const auto refused = [&](const char *tag, const fa_rnnt_stream_config &c, const int32_t streams) {
        const fa_status s = fa_rnnt_stream_create(ctx.handle(), &c, streams, &st);
        std::printf("REFUSED %s %d %s\n", tag, static_cast<int>(s), fa_ctx_last_error(ctx.handle()));
    };
    fa_rnnt_stream_config bad = cfg.c;
    bad.window_samples = 1282; refused("window", bad, 1);
    bad = cfg.c; bad.total_mel_frames = 0; refused("total", bad, 1);
    bad = cfg.c; bad.open_slack_frames = 2; refused("slack", bad, 1);
    bad = cfg.c; bad.vad_rms_threshold = 1.0f; refused("vad", bad, 1);
    refused("streams", cfg.c, 0);
    // class table: 0 punctuation, 1 a language tag, 2 .. 9 words
    std::vector<uint8_t> classes = {0, FA_RNNT_STREAM_CLASS_LANG_TAG | FA_RNNT_STREAM_CLASS_LEXICAL, 1, 1, 1, 1, 1, 1, 1, 1};
    cfg.c.vad_rms_threshold = 0.003f;
    NemotronStreamSession session(ctx, cfg, classes);
    float r = 0.0f;
    const std::vector<float> quiet = audio("0000000", 1280), chunk = audio("0011000", 1280);
    const bool s1 = session.gate(quiet, &r), s2 = session.gate(quiet), s3 = session.gate(chunk);
    std::printf("GATE %d %d %d %08x %08x\n", s1, s2, s3, bits(r), bits(NemotronStreamSession::rms(quiet, true)));
    std::vector<int> ids = {1, 5};
    std::vector<NemotronTokenTiming> timings = {{5, 40}};
    const std::vector<RescueRequest> found = session.track(chunk, timings, 4480);
    for (const RescueRequest &q : found) {
        size_t same = 0;
        for (size_t i = 0; i < 4 * 1280; ++i) same += bits(q.audio[i]) == bits(chunk[i]);          // two pre-roll windows, then the two loud ones
        for (size_t i = 6 * 1280; i < q.audio.size(); ++i) same += q.audio[i] == 0.0f;
        std::printf("REQUEST %d %d %d %d %d %zu %zu\n", q.record.span_start_frame, q.record.span_end_frame, q.record.speech_windows, q.record.audio_samples, q.record.decode_chunks,
                    q.audio.size(), same);
    }
    if (found.size() == 1) {
        const bool none = session.mergeRescued(found[0], {1, 0}, {2}, ids, timings);
        const bool done = session.mergeRescued(found[0], {1, 6, 0, 7}, {1, 3, 9}, ids, timings);
        std::printf("MERGE %d %d |", none, done);
        for (const int i : ids) std::printf(" %d", i);
        std::printf(" |");
        for (const NemotronTokenTiming &t : timings) std::printf(" %d@%d", t.tokenId, t.frame);
        std::printf(" | %d %d %a\n", session.detectedBlankSpanCount(), session.blankRescueCount(), timings[0].startTime());
    }
    session.reset();
    std::printf("RESET %d %d\n", session.detectedBlankSpanCount(), session.info().frame_cursor);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "device") return device();
    std::printf("LAYOUT config %zu %zu %zu %zu\n", sizeof(fa_rnnt_stream_config), offsetof(fa_rnnt_stream_config, vad_hangover_chunks), offsetof(fa_rnnt_stream_config, total_mel_frames),
                offsetof(fa_rnnt_stream_config, rescue_rms_threshold));
    std::printf("LAYOUT info %zu %zu %zu\n", sizeof(fa_rnnt_stream_info), offsetof(fa_rnnt_stream_info, span_samples), offsetof(fa_rnnt_stream_info, mel_cache_frames));
    std::printf("LAYOUT request %zu %zu %zu %zu\n", sizeof(fa_rnnt_stream_request), offsetof(fa_rnnt_stream_request, audio_samples), offsetof(fa_rnnt_stream_request, status),
                offsetof(fa_rnnt_stream_request, audio_offset));
    std::printf("LAYOUT geometry %zu\n", sizeof(fa_rnnt_stream_geometry_info));
    NemotronStreamConfig cfg(65);
    const fa_rnnt_stream_config &c = cfg.c;
    fa_rnnt_stream_default_config(nullptr);
    std::printf("CFG %d %d %d %d %d %d %d %d %d %d %d %08x %08x\n", c.window_samples, c.close_silent_windows, c.pre_roll_windows, c.min_speech_windows, c.max_span_samples,
                c.open_slack_frames, c.close_slack_frames, c.vad_hangover_chunks, c.mel_features, c.pre_encode_cache, c.total_mel_frames, bits(c.rescue_rms_threshold),
                bits(c.vad_rms_threshold));
    const fa_rnnt_stream_geometry_info g = cfg.geometry();
    std::printf("GEO %d %d %d\n", g.span_capacity, g.pre_roll_capacity, g.mel_cache_capacity);
    // the geometry entry answers every unsound config
    fa_rnnt_stream_geometry_info out{};
    std::printf("ST config");
    const auto with = [&](const auto &edit) { fa_rnnt_stream_config k = cfg.c; edit(k); std::printf(" %d", static_cast<int>(fa_rnnt_stream_geometry(&k, &out))); };
    with([](fa_rnnt_stream_config &k) { k.window_samples = 0; });
    with([](fa_rnnt_stream_config &k) { k.window_samples = 8196; });
    with([](fa_rnnt_stream_config &k) { k.window_samples = 1282; });
    with([](fa_rnnt_stream_config &k) { k.close_silent_windows = 0; });
    with([](fa_rnnt_stream_config &k) { k.pre_roll_windows = 65; });
    with([](fa_rnnt_stream_config &k) { k.min_speech_windows = -1; });
    with([](fa_rnnt_stream_config &k) { k.max_span_samples = 0; });
    with([](fa_rnnt_stream_config &k) { k.close_slack_frames = -1; });
    with([](fa_rnnt_stream_config &k) { k.open_slack_frames = 2; });
    with([](fa_rnnt_stream_config &k) { k.rescue_rms_threshold = -1.0f; });
    with([](fa_rnnt_stream_config &k) { k.vad_rms_threshold = 1.0f; });
    with([](fa_rnnt_stream_config &k) { k.vad_hangover_chunks = 0; });
    with([](fa_rnnt_stream_config &k) { k.mel_features = 0; });
    with([](fa_rnnt_stream_config &k) { k.pre_encode_cache = 65; });
    with([](fa_rnnt_stream_config &k) { k.total_mel_frames = 8; });
    with([](fa_rnnt_stream_config &k) { k.total_mel_frames = 0; });
    with([](fa_rnnt_stream_config &k) { k.rescue_rms_threshold = 0.0f; k.vad_rms_threshold = 0.5f; k.pre_encode_cache = 0; k.total_mel_frames = 1; });   // sound
    std::printf(" %d %d\n", static_cast<int>(fa_rnnt_stream_geometry(nullptr, &out)), static_cast<int>(fa_rnnt_stream_geometry(&cfg.c, nullptr)));
    // without a context or a state every entry answers INVALID_ARGUMENT
    fa_rnnt_stream *st = nullptr;
    fa_rnnt_stream_info info{};
    float f = 0.0f;
    int32_t i = 0;
    fa_rnnt_stream_request q{};
    uint8_t cls = 0;
    std::printf("ST null %d %d %d %d", static_cast<int>(fa_rnnt_stream_create(nullptr, &cfg.c, 1, &st)), static_cast<int>(fa_rnnt_stream_reset(nullptr, nullptr, 0)),
                static_cast<int>(fa_rnnt_stream_get(nullptr, nullptr, 0, &info, nullptr, nullptr, nullptr)), static_cast<int>(fa_rnnt_stream_set(nullptr, nullptr, 0, &info, nullptr, nullptr, nullptr)));
    std::printf(" %d %d %d", static_cast<int>(fa_rnnt_stream_gate_dev(nullptr, nullptr, &f, 4, nullptr, &f, &i, &i, &i, &i)),
                static_cast<int>(fa_rnnt_stream_mel_inputs_dev(nullptr, nullptr, &f, 1, 1, 1, 1, &i, &i, 1, &f, &i)), static_cast<int>(fa_rnnt_stream_advance_dev(nullptr, nullptr, &i, &i, 1, nullptr, 1)));
    std::printf(" %d %d", static_cast<int>(fa_rnnt_stream_track_dev(nullptr, nullptr, &f, 4, nullptr, &i, &i, &i, 1, &cls, 1, 4, &q, 1, &f, 4, &i, &i)),
                static_cast<int>(fa_rnnt_stream_finalize_dev(nullptr, nullptr, &i, &i, 1, &i, &i, &i, 1, &cls, 1, 4, &q, 1, &f, 4, &i, &i)));
    std::printf(" %d %d %d %d\n", static_cast<int>(fa_rnnt_stream_merge_rescued_dev(nullptr, nullptr, &q, &i, 1, &i, &i, &i, &i, 1, &i, &i, &i, &i, &i, 1, &cls, 1, &i)),
                static_cast<int>(fa_rnnt_stream_gate(nullptr, nullptr, &f, 4, nullptr, &f, &i, &i, &i, &i)),
                static_cast<int>(fa_rnnt_stream_track(nullptr, nullptr, &f, 4, nullptr, &i, &i, &i, 1, &cls, 1, 4, &q, 1, &f, 4, &i, &i)),
                static_cast<int>(fa_rnnt_stream_merge_rescued(nullptr, nullptr, &q, 1, &i, &i, &i, &i, 1, &i, &i, &i, &i, &i, 1, &cls, 1, &i)));
    fa_rnnt_stream_destroy(nullptr);
    const float x[5] = {0.5f, 0.5f, 0.5f, 0.5f, 0.5f};
    const int r0 = static_cast<int>(fa_rnnt_stream_rms(nullptr, 4, 0, &f)), r1 = static_cast<int>(fa_rnnt_stream_rms(x, -1, 0, &f)), r2 = static_cast<int>(fa_rnnt_stream_rms(x, 5, 1, &f));
    std::printf("ST rms %d %d %d %08x\n", r0, r1, r2, bits(f));
    std::printf("RMS %08x %08x\n", bits(NemotronStreamSession::rms({})), bits(NemotronStreamSession::rms({3.0f, 4.0f, 0.0f, 0.0f})));
    return 0;
}
