// pockettts_core.h — the integers and the EOS machine of the PocketTTS session (kernels: pockettts.hip, host code: pockettts_host.hip),
// restated from TTS/PocketTTS/PocketTtsConstants.swift, Pipeline/PocketTtsVoiceCloner.swift:131-143,296-299,
// PocketTtsSynthesizer+KVCache.swift:190-240,254-357,368-455, PocketTtsStateEngine.swift:80-111,119-162,227-262 and
// PocketTtsSynthesizer.swift:527-568.  Plain C++: no HIP type appears here.  Every count is decided on the host before a launch;
// tests/cpu/pockettts_core_main.cpp runs the plan and the machine against the naive loop.
//
// The EOS machine (advance): one call per generation step of a running stream, in the order of the reference's loop body: a first
// eosLogit > -4 sets eos_step; step >= eos_step + frames_after_eos + 2 ends the stream before this step's frame; otherwise the step emits
// (frames + 1, step + 1) and reaching max_gen_len ends the stream.  A NaN logit is not EOS (the comparison is false).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FA_PTTS_HD __host__ __device__ __forceinline__
#else
#define FA_PTTS_HD inline
#endif

namespace fa {
namespace pockettts {

constexpr int kDim = 1024;              // embeddingDim
constexpr int kLatent = 32;             // latentDim
constexpr int kWindow = 256;            // condPrefillMaxTokens
constexpr int kKvSeq = 512;             // kvCacheMaxLen
constexpr int kKvRow = 16 * 64;         // heads x head dim: elements of one cached position
constexpr int64_t kPlane = static_cast<int64_t>(kKvSeq) * kKvRow;   // elements of K (or V) of one layer
constexpr float kEosThreshold = -4.0f;
constexpr int kExtraFrames = 2;         // extraFramesAfterDetection
constexpr int kFrameSamples = 1920;
constexpr int kEncoderSamples = 240000;
constexpr int kSampleRate = 24000;
constexpr int kMaxVoiceFrames = 125;
constexpr int kMaxLayers = 24;

enum KvFormat : int32_t { kKvCombined = 0, kKvSplit = 1, kKvHalf = 2 };

// status of a clip, a voice or a stream: 0, or what the reference throws
enum Status : int32_t {
    kOk = 0,
    kClipTooShort = 1,       // VoiceCloner :138: under one second
    kLayerCount = 2,         // KVCache :373: the snapshot's layer count is not the model's
    kSeqTooLong = 3,         // KVCache :380: srcSeq beyond the capacity
    kFloatCount = 4,         // KVCache :416: a layer is not 2 * srcSeq * 1024 floats
    kNoBosBeforeVoice = 5,   // KVCache :277: a cloned voice without the bos_before_voice constant
    kNoVoice = 6,            // the voice slot holds nothing
    kTooManyWindows = 7,     // the session's window arena is full
    kTooManyFrames = 8,      // max_gen_len beyond the session's audio slab
};

enum Reason : int32_t { kIdle = 0, kRunning = 1, kEndEos = 2, kEndMaxLen = 3 };

// VoiceCloner :137-143: durationSeconds >= 1.0 on the original length
inline int32_t clip_status(const int64_t samples) { return static_cast<double>(samples) / kSampleRate >= 1.0 ? kOk : kClipTooShort; }

// VoiceCloner :148, :296-299
inline int32_t usable_frames(const int64_t samples, const int32_t available) {
    const int64_t real = samples < kEncoderSamples ? samples : kEncoderSamples;
    int64_t n = (real + kFrameSamples - 1) / kFrameSamples;
    n = n < available ? n : available;
    n = n < kMaxVoiceFrames ? n : kMaxVoiceFrames;
    return static_cast<int32_t>(n < 0 ? 0 : n);
}

// KVCache :373-421 / StateEngine :230-252
inline int32_t snapshot_status(const int32_t layers, const int32_t model_layers, const int32_t src_seq, const int32_t capacity, const int64_t *float_counts) {
    if (layers != model_layers) return kLayerCount;
    if (src_seq > capacity) return kSeqTooLong;
    for (int l = 0; l < layers; ++l)
        if (float_counts[l] != 2 * static_cast<int64_t>(src_seq) * kKvRow) return kFloatCount;
    return kOk;
}

// where K (kv 0) or V (kv 1) of (stream, layer) starts in the cache slab, in elements
FA_PTTS_HD int64_t kv_plane_at(const int32_t format, const int32_t streams, const int32_t layers, const int32_t stream, const int32_t layer, const int32_t kv) {
    const int64_t sl = static_cast<int64_t>(stream) * layers + layer;
    return (format == kKvCombined ? sl * 2 + kv : static_cast<int64_t>(kv) * streams * layers + sl) * kPlane;
}
FA_PTTS_HD int32_t positions_of(const int32_t format, const int32_t layers) { return format == kKvHalf ? 1 : layers; }

// ---- the prefill windows.  A block of `tokens` rows is cut into windows of at most kWindow (KVCache :206-239); the voice block
// [bos_before_voice, voice rows...] comes first, then the text block (KVCache :482-500), and they never share a window.
struct Window {
    int32_t stream, block, first, n;   // block 0: voice, 1: text; rows [first, first + n) of the block
    int32_t voice, ids_at, before, pad;   // the stream's voice; where the stream's token ids start; rows of this plan in front of the window
};

struct VoiceFacts {
    int32_t present, has_snapshot, prompt_length;
};

// the voice rows a stream prefills: 1 + promptLength for a cloned voice without a snapshot, else none (KVCache :267-275, :482)
inline int32_t voice_block_rows(const VoiceFacts &v) { return (v.present && !v.has_snapshot && v.prompt_length > 0) ? 1 + v.prompt_length : 0; }

// appends the windows of one stream; returns its status.  `out` holds `capacity` windows, *count of them are taken.
inline int32_t plan_stream(const int32_t stream, const int32_t voice, const VoiceFacts &v, const bool have_bos, const int32_t tokens, const int32_t ids_at, Window *out,
                           const int32_t capacity, int32_t *count) {
    if (!v.present) return kNoVoice;
    const int32_t rows[2] = {voice_block_rows(v), tokens > 0 ? tokens : 0};
    if (rows[0] > 0 && !have_bos) return kNoBosBeforeVoice;
    const int32_t need = (rows[0] + kWindow - 1) / kWindow + (rows[1] + kWindow - 1) / kWindow;
    if (*count + need > capacity) return kTooManyWindows;
    int32_t before = 0;
    for (int block = 0; block < 2; ++block)
        for (int32_t done = 0; done < rows[block];) {
            const int32_t n = rows[block] - done < kWindow ? rows[block] - done : kWindow;
            out[(*count)++] = Window{stream, block, done, n, voice, ids_at, before, 0};
            done += n;
            before += n;
        }
    return kOk;
}

// ---- the generation loop's scalar side
struct StreamState {
    int32_t step, eos_step, max_gen, after, frames, reason, emit, pad;
};

// Synthesizer :527-533 (max_gen = estimateMaxFrames, after = framesAfterEos; the loop `for step in 0..<maxGenLen` of an empty range never runs)
FA_PTTS_HD StreamState begin_state(const int32_t max_gen, const int32_t after) {
    return StreamState{0, -1, max_gen, after, 0, max_gen > 0 ? kRunning : kEndMaxLen, 0, 0};
}

// Synthesizer :543-568; true: this step's frame is decoded and fed back
FA_PTTS_HD bool advance(StreamState &m, const float eos_logit) {
    m.emit = 0;
    if (m.reason != kRunning) return false;
    if (eos_logit > kEosThreshold && m.eos_step < 0) m.eos_step = m.step;
    if (m.eos_step >= 0 && m.step >= m.eos_step + m.after + kExtraFrames) { m.reason = kEndEos; return false; }
    m.emit = 1;
    ++m.frames;
    if (++m.step >= m.max_gen) m.reason = kEndMaxLen;
    return true;
}

}  // namespace pockettts
}  // namespace fa
