// aed_core.h — the integers that the host side and the kernels of the AED (attention encoder-decoder) unit share: the long-form
// window plan (CoherePipeline.swift:525-572, CanaryManager.swift:50-71), the valid-frame rule (CoherePipeline.swift:670-676), the
// layout of the per-utterance decode state and the bookkeeping of a decode step (CoherePipeline.swift:728-803,
// CanaryManager.swift:212-275).  Plain C++ without a HIP call: host code, kernels and tests/cpu/aed_core_main.cpp compile it.
// Internal; not part of the C ABI.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fluidaudio_hip.h"

#if defined(__HIPCC__)
#define FA_AED_HD __host__ __device__
#else
#define FA_AED_HD
#endif

namespace fa {
namespace aed {

// ---- the window plan.  The loop of transcribeLong, line by line; starts / lens may be null (count only).
FA_AED_HD inline int64_t plan_windows_one(const int64_t samples, const int64_t chunk, const int64_t hop, int64_t *starts, int64_t *lens) {
    if (samples <= chunk) {   // `if audio.count <= chunkSamples`: the single-chunk path, an empty recording included
        if (starts) { starts[0] = 0; lens[0] = samples; }
        return 1;
    }
    int64_t start = 0, index = 0;
    while (start < samples) {
        const int64_t end = (samples - start > chunk) ? start + chunk : samples;   // min(start + chunk, samples) without the overflow
        if (index > 0 && (end - start) <= (chunk - hop)) break;                    // a tail of pure overlap
        if (starts) { starts[index] = start; lens[index] = end - start; }
        ++index;
        if (end >= samples) break;
        start += hop;
    }
    return index;
}
// The count of that loop in closed form (a window follows only a window that did not reach the end, so it always holds more than
// chunk - hop samples): 1 + ceil((samples - chunk) / hop) beyond one chunk.
FA_AED_HD inline int64_t window_count(const int64_t samples, const int64_t chunk, const int64_t hop) {
    if (samples <= chunk) return 1;
    const int64_t rest = samples - chunk;
    return 1 + rest / hop + (rest % hop != 0 ? 1 : 0);
}

// encoderValidFrames: Int((Double(featureLength * encoderFrames) / Double(melFrames)).rounded(.up)), clamped to [1, encoderSeqLen]
inline int64_t encoder_valid_frames(const int64_t feature_length, const int64_t encoder_seq_len, const int64_t mel_frames, const int64_t encoder_frames) {
    const double raw = std::ceil(static_cast<double>(feature_length * encoder_frames) / static_cast<double>(mel_frames));
    const int64_t r = static_cast<int64_t>(raw);
    const int64_t lo = r < encoder_seq_len ? r : encoder_seq_len;
    return lo > 1 ? lo : 1;
}

// ---- the decode state: per utterance kHead header words, then the history, the prompt and the output tokens (all int32).
enum Word : int32_t { kHistLen = 0, kStep = 1, kCur = 2, kOutCount = 3, kReason = 4, kPromptLen = 5, kHead = 8 };

FA_AED_HD inline int32_t max_out_of(const fa_aed_config &c) {
    if (c.mode == FA_AED_FEED_SEQUENCE) return c.max_seq;
    return c.max_new + 1 < c.max_seq ? c.max_new + 1 : c.max_seq;   // steps P - 1 ... min(max_new + P, max_seq) - 1 emit one token each
}
struct Layout {
    int32_t max_seq, max_out;
    FA_AED_HD int64_t words() const { return kHead + 2 * static_cast<int64_t>(max_seq) + max_out; }
    FA_AED_HD int32_t *utt(int32_t *state, const int64_t b) const { return state + b * words(); }
    FA_AED_HD const int32_t *utt(const int32_t *state, const int64_t b) const { return state + b * words(); }
    FA_AED_HD int64_t hist() const { return kHead; }
    FA_AED_HD int64_t prompt() const { return kHead + max_seq; }
    FA_AED_HD int64_t out() const { return kHead + 2 * static_cast<int64_t>(max_seq); }
};
FA_AED_HD inline Layout layout_of(const fa_aed_config &c) { return Layout{c.max_seq, max_out_of(c)}; }

// ---- the step bookkeeping of the token feed: `for step in 0..<min(maxNewTokens + prompt.count, maxSeqLen)`
FA_AED_HD inline int32_t token_last_step(const int32_t max_new, const int32_t prompt_len, const int32_t max_seq) {
    const int64_t e = static_cast<int64_t>(max_new) + prompt_len;
    return static_cast<int32_t>(e < max_seq ? e : max_seq) - 1;
}
FA_AED_HD inline bool token_decides(const int32_t step, const int32_t prompt_len) { return step >= prompt_len - 1; }

constexpr float kMasked = -1.0e4f;             // the additive mask's invalid value
constexpr uint16_t kMaskedF16 = 0xF0E2;        // its binary16 bits
constexpr float kBanned = -1e9f;               // applyNoRepeatNgram

}  // namespace aed
}  // namespace fa
