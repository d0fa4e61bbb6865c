// rnnt_stream_core.h — the integers and the fp32 sum order of the Nemotron streaming session that the host entries, the kernels and the
// tests share (reference: Sources/FluidAudio/ASR/Parakeet/Streaming/Nemotron/StreamingNemotronMultilingualAsrManager+BlankRescue.swift:70-164,
// 243-251, 323-354, +Pipeline.swift:86-104, +Buffers.swift:53-63): the config's limits and slab sizes, the order in which an RMS adds its
// squares, the gate's counter, one window of the span machine with the copy it asks for, the closing test's frame window, a request's
// padded length and the two insert indices of mergeRescuedTokens as word steps.  Plain C++: it compiles on the host alone
// (tests/cpu/rnnt_stream_core_main.cpp runs it under the sanitizers) and inside the kernels.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FA_RNS_HD __host__ __device__
#else
#define FA_RNS_HD
#endif

namespace fa {
namespace rns {

// fa_rnnt_stream_config, field for field (rnnt_stream_host.hip asserts the sizes).
struct Config {
    int32_t window_samples, close_silent_windows, pre_roll_windows, min_speech_windows, max_span_samples, open_slack_frames, close_slack_frames;
    int32_t vad_hangover_chunks, mel_features, pre_encode_cache, total_mel_frames, reserved;
    float rescue_rms_threshold, vad_rms_threshold;
};

enum Status : int32_t { kOk = 0, kInactive = 1, kBadOperand = 2, kOutputTooSmall = 3, kNoLexical = 4 };
enum Class : uint8_t { kLexical = 1, kLangTag = 2 };

constexpr int kLanes = 64;
constexpr int kGateWaves = 4;   // wavefronts that share one chunk's RMS

// one stream's scalars, in the order of fa_rnnt_stream_info; behind them the ring's head
enum Scalar : int32_t {
    kCursor = 0, kOpen, kStart, kLast, kSpeech, kPreFrames, kRun, kOverflowed, kSpanLen, kPreLen, kVadLow, kVadSkips, kFrameBase, kDetected, kRescued,
    kMelFrames, kPreHead, kScalars = 20
};

// 0: sound; otherwise the index of the refusal's text (rnnt_stream_host.hip)
FA_RNS_HD inline int config_fault(const Config &c) {
    if (c.window_samples < 4 || c.window_samples > 8192 || c.window_samples % 4 != 0) return 1;
    if (c.close_silent_windows < 1 || c.close_silent_windows > 1024) return 2;
    if (c.pre_roll_windows < 0 || c.pre_roll_windows > 64) return 3;
    if (c.min_speech_windows < 0 || c.min_speech_windows > (1 << 20)) return 4;
    if (c.max_span_samples < 1 || c.max_span_samples > (1 << 24)) return 5;
    if (c.open_slack_frames < 0 || c.open_slack_frames > (1 << 20) || c.close_slack_frames < 0 || c.close_slack_frames > (1 << 20)) return 6;
    if (!(c.rescue_rms_threshold >= 0.0f) || !(c.rescue_rms_threshold <= 3.0e38f)) return 7;
    if (!(c.vad_rms_threshold >= 0.0f) || !(c.vad_rms_threshold < 1.0f)) return 8;
    if (c.vad_hangover_chunks < 1 || c.vad_hangover_chunks > (1 << 20)) return 9;
    if (c.mel_features < 1 || c.mel_features > 4096) return 10;
    if (c.pre_encode_cache < 0 || c.pre_encode_cache > kLanes) return 11;
    if (c.total_mel_frames < 1 || c.total_mel_frames < c.pre_encode_cache || c.total_mel_frames > 65536) return 12;
    // the closures of one chunk are judged before any of them is merged: equal to the reference's order only while a rescued frame
    // (at most last + 1) cannot reach the next span's window, which begins at start' - open_slack >= last + close + 1 - open_slack
    if (c.close_silent_windows <= c.open_slack_frames) return 13;
    return 0;
}

// the span slab: max_span_samples rounded up to whole windows, plus one window
FA_RNS_HD inline int32_t span_capacity(const Config &c) {
    const int32_t w = c.window_samples;
    return (c.max_span_samples + w - 1) / w * w + w;
}
FA_RNS_HD inline int32_t pre_roll_capacity(const Config &c) { return (c.pre_roll_windows > 0 ? c.pre_roll_windows : 1) * c.window_samples; }
FA_RNS_HD inline int32_t mel_cache_capacity(const Config &c) { return c.mel_features * (c.pre_encode_cache > 0 ? c.pre_encode_cache : 1); }

// ---- the RMS.  Element i belongs to lane (i / 4) % 64 of wavefront (i / 256) % waves; a lane adds its squares in ascending i with a
// fused multiply-add; the lanes of a wavefront meet in six butterfly steps (xor 32, 16, 8, 4, 2, 1: fp32 addition commutes, so both
// partners hold the same bits); the wavefronts' sums are added in ascending order; one divide by n, one square root.
FA_RNS_HD inline float square_add(const float x, const float acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmaf(x, x, acc);
#else
    return std::fmaf(x, x, acc);
#endif
}
FA_RNS_HD inline float rms_of_sum(const float sum, const int64_t n) {
    if (n <= 0) return 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    return sqrtf(sum / static_cast<float>(n));   // correctly rounded both (hipcc's default); __fsqrt_rn is the native approximation
#else
    return std::sqrt(sum / static_cast<float>(n));
#endif
}
// the groups of four elements lane `lane` of wavefront `wave` owns: group k of them is ((k * waves + wave) * 64 + lane)
FA_RNS_HD inline int64_t lane_group(const int64_t k, const int wave, const int lane, const int waves) { return (k * waves + wave) * kLanes + lane; }

// the host's emulation of the kernels' order
inline float sum_squares(const float *x, const int64_t n, const int waves) {
    float total = 0.0f;
    for (int w = 0; w < waves; ++w) {
        float acc[kLanes];
        for (int l = 0; l < kLanes; ++l) {
            float a = 0.0f;
            for (int64_t k = 0;; ++k) {
                const int64_t i0 = lane_group(k, w, l, waves) * 4;
                if (i0 >= n) break;
                for (int64_t i = i0; i < i0 + 4 && i < n; ++i) a = square_add(x[i], a);
            }
            acc[l] = a;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            float next[kLanes];
            for (int l = 0; l < kLanes; ++l) next[l] = acc[l] + acc[l ^ off];
            for (int l = 0; l < kLanes; ++l) acc[l] = next[l];
        }
        total = w == 0 ? acc[0] : total + acc[0];
    }
    return total;
}
inline float rms(const float *x, const int64_t n, const int waves) { return rms_of_sum(sum_squares(x, n, waves), n); }

// ---- the gate (Pipeline.swift:86-104).  low / skips / base are the stream's counters; returns 1 when the chunk skips the encoder.
FA_RNS_HD inline int32_t gate_step(const Config &c, const bool silent, const int32_t chunk_samples, int32_t &low, int32_t &skips, int32_t &base) {
    if (!(c.vad_rms_threshold > 0.0f)) return 0;
    if (!silent) { low = 0; return 0; }
    low = static_cast<int32_t>(static_cast<uint32_t>(low) + 1u);                  // &+=
    if (low < c.vad_hangover_chunks) return 0;
    skips = static_cast<int32_t>(static_cast<uint32_t>(skips) + 1u);
    base += chunk_samples / c.window_samples;
    return 1;
}

// ---- the span machine (BlankRescue.swift:70-119).  The audio lives in the span slab and in a ring of pre_roll_windows window slots
// (head: the oldest); a step says where the window goes and what to copy first.
struct Span {
    int32_t open, start, last, speech, pre_frames, run, overflowed;
    int32_t len;                    // samples in the slab
    int32_t pre_head, pre_count;    // ring: oldest slot, windows held
};
struct Closure { int32_t start, last, speech, pre_frames, len, overflowed; };
enum Dest : int32_t { kNowhere = 0, kToSpan = 1, kToRing = 2 };
struct Step {
    int32_t ring_windows;   // on opening: the ring's windows (from ring_head, oldest first) go to the slab's front before the window
    int32_t ring_head;
    int32_t dest;           // Dest
    int32_t offset;         // kToSpan: samples into the slab; kToRing: the slot
    int32_t closed;
    Closure closure;
};

FA_RNS_HD inline Closure close_span(Span &s) {                                    // :124-136
    const Closure c{s.start, s.last, s.speech, s.pre_frames, s.len, s.overflowed};
    s.open = 0; s.len = 0; s.speech = 0; s.run = 0; s.overflowed = 0;
    s.pre_head = 0; s.pre_count = 0;                                              // the silence that closed the span is its own
    return c;
}

FA_RNS_HD inline Step window_step(const Config &c, Span &s, const bool silent, const int32_t frame) {
    Step r{};
    const int32_t W = c.window_samples, P = c.pre_roll_windows;
    if (s.open) {                                                                 // :82-89
        if (silent) { s.run += 1; } else { s.run = 0; s.last = frame; s.speech += 1; }
    } else if (!silent) {                                                         // :90-99
        s.open = 1; s.start = frame; s.last = frame; s.speech = 1; s.run = 0;
        r.ring_windows = s.pre_count; r.ring_head = s.pre_head;
        s.len = s.pre_count * W; s.pre_frames = s.pre_count; s.overflowed = 0;
    }
    if (s.open && !s.overflowed) {                                                // :101-106
        if (static_cast<int64_t>(s.len) + W > c.max_span_samples) {
            s.overflowed = 1; s.len = 0; r.ring_windows = 0;                      // the audio is dropped: nothing to copy
        } else {
            r.dest = kToSpan; r.offset = s.len; s.len += W;
        }
    } else if (!s.open && P > 0) {                                                // :107-113
        r.dest = kToRing;
        if (s.pre_count < P) { r.offset = (s.pre_head + s.pre_count) % P; s.pre_count += 1; }
        else { r.offset = s.pre_head; s.pre_head = (s.pre_head + 1) % P; }
    }
    if (s.open && s.run >= c.close_silent_windows) { r.closed = 1; r.closure = close_span(s); }   // :115-117
    return r;
}

// :138: the spans the closing test looks at
FA_RNS_HD inline bool qualifies(const Config &c, const Closure &k) { return !k.overflowed && k.speech >= c.min_speech_windows; }
// :145-156 on frames: a lexical token in [start - open_slack, last + close_slack] means the span emitted
FA_RNS_HD inline bool in_span_window(const Config &c, const Closure &k, const int32_t frame) {
    return static_cast<int64_t>(frame) >= static_cast<int64_t>(k.start) - c.open_slack_frames && static_cast<int64_t>(frame) <= static_cast<int64_t>(k.last) + c.close_slack_frames;
}
// :243-251
FA_RNS_HD inline int32_t decode_chunks(const int32_t samples, const int32_t chunk_samples) { return (samples + chunk_samples - 1) / chunk_samples + 1; }

FA_RNS_HD inline uint8_t class_of(const uint8_t *table, const int32_t vocab, const int32_t id) { return id >= 0 && id < vocab ? table[id] : 0; }

// ---- mergeRescuedTokens' indices (:331-347) as steps over 64 entries.
// position of the k-th (0-based) set bit of m; m has more than k set bits
FA_RNS_HD inline int nth_set_bit(uint64_t m, int k) {
    for (; k > 0; --k) m &= m - 1;
    return __builtin_ctzll(m);
}
FA_RNS_HD inline int popcount64(const uint64_t m) { return __builtin_popcountll(m); }
// timingInsertIndex: the first entry with frame > key.  `above`: bit j set where entry base + j > key.  -1: not in this word.
FA_RNS_HD inline int32_t timing_word(const uint64_t above, const int32_t base) { return above ? base + nth_set_bit(above, 0) : -1; }
// idsInsertIndex: the entry that is the `need`-th (0-based) one without a language tag.  `plain`: bit j set where entry base + j has no tag.
// -1: not in this word, `need` reduced by the word's plain entries.
FA_RNS_HD inline int32_t ids_word(const uint64_t plain, const int32_t base, int32_t &need) {
    const int have = popcount64(plain);
    if (have > need) return base + nth_set_bit(plain, need);
    need -= have;
    return -1;
}

}  // namespace rns
}  // namespace fa
