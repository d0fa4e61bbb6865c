// vad_launch.h — what the host side of the VAD stages (vad_host.hip: the C ABI, uploads, the synchronisation of a call) and their
// kernels (vad.hip) share: the argument pass of the four entries (plain C++: decided from the arguments alone, nothing is written but
// the plan), the operands the reference derives from a config, the layout of the workspace, the kernels' operands and their launchers.
// Internal; not part of the C ABI.  The stand-alone program tests/cpu/vad_plan.cpp walks the argument pass and the plan on the host.
//
// Restated: segmentSpeech(from:totalSamples:config:) and detectSpeechSampleRanges (FluidAudio/VAD/VadManager+SpeechSegmentation.swift:22-51,
// 71-234), the model rows of processAudioSamples / processChunk (VadManager.swift:162-206, 352-376), the bounds of segmentSpeechAudio
// (:55-67) and streamingStateMachine (VadManager+Streaming.swift:31-107).
// OUT OF SCOPE: the Silero network and its LSTM state (the caller's: they run the model on the packed rows), isSilentAudio
// (VadManager.swift:157-160).  FSMN-VAD (VAD/Fsmn/: its decide and its chunk schedule) is fsmn_vad_launch.h.
//
// The raw speeches of one recording (before the padding) start on frame boundaries, each on a frame of its own: a speech that follows a
// cut starts where the chosen silence ended, behind the end of the one before it.  The frame of a cut that resumes does go on to the
// end-of-speech test, but never flushes a second time: the cut has cleared tempEnd, the test opens its silence at that very frame, and
// with min_silence == 0 — where 0 >= min_silence would hold — no candidate is ever recorded, so no cut resumes.  So a recording of F
// frames has at most F raw speeches, not 2 F + 1: tests/test_vad_cpu.py walks every sequence of up to 8 frames to check both, vad_machine
// counts beyond the slice without writing, and the host entry refuses a count above it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fa_verdict.h"

namespace fa {
namespace vad {

constexpr int kWave = 64;
constexpr int kChunk = 4096;                 // VadManager.chunkSize: samples of a frame (hop and window)
constexpr int kContext = 64;                 // VadState.contextLength
constexpr int kRow = kContext + kChunk;      // VadManager.modelInputSize
constexpr double kRate = 16000.0;            // Double(VadManager.sampleRate)
constexpr int64_t kNone = INT64_MAX;         // Int.max: no maximal speech duration
constexpr int kPackGroup = 64;               // recordings whose offsets travel in one launch's arguments
constexpr int kGatherTile = 2048;            // samples of a workgroup of the ragged copy

inline fa_vad_segmentation_config config_or_default(const fa_vad_segmentation_config *cfg) {
    if (cfg) return *cfg;
    fa_vad_segmentation_config c{};          // VadTypes.swift:13, 37-47
    c.default_threshold = 0.85f;
    c.min_speech_duration = 0.15; c.min_silence_duration = 0.75; c.max_speech_duration = 14.0; c.speech_padding = 0.1;
    c.silence_threshold_for_split = 0.3f;
    c.has_negative_threshold = 0; c.negative_threshold = 0.0f; c.negative_threshold_offset = 0.15f;
    c.min_silence_at_max_speech = 0.098;
    c.use_max_possible_silence_at_max_speech = 1;
    return c;
}

// What detectSpeechSampleRanges (:85-100) and streamingStateMachine (:45-53) derive from a config.
struct Operands {
    float threshold, negative_threshold, split_threshold;
    int64_t min_speech, pad, max_speech, min_silence, min_silence_at_max;   // samples; max_speech kNone for +inf
    int32_t use_max;
};

// Int(seconds * 16000.0): false where Swift traps (NaN, infinities, a product outside Int)
inline bool to_samples(const double seconds, int64_t *out) {
    const double x = seconds * kRate;
    if (!(x > -9223372036854775808.0 && x < 9223372036854775808.0)) return false;
    *out = static_cast<int64_t>(x);          // truncates, as Int(_:) does
    return true;
}

// The preconditions of VadSegmentationConfig.init (VadTypes.swift:50-66) in their order, then what would trap further down.
inline Verdict derive(const fa_vad_segmentation_config &c, Operands *o) {
    if (!(c.min_speech_duration >= 0)) return refuse(FA_INVALID_ARGUMENT, "minSpeechDuration must be non-negative");
    if (!(c.min_silence_duration >= 0)) return refuse(FA_INVALID_ARGUMENT, "minSilenceDuration must be non-negative");
    if (!(c.max_speech_duration > 0)) return refuse(FA_INVALID_ARGUMENT, "maxSpeechDuration must be positive");
    if (!(c.speech_padding >= 0)) return refuse(FA_INVALID_ARGUMENT, "speechPadding must be non-negative");
    if (!(c.silence_threshold_for_split >= 0 && c.silence_threshold_for_split <= 1)) return refuse(FA_INVALID_ARGUMENT, "silenceThresholdForSplit must be in [0, 1]");
    if (!(c.negative_threshold_offset >= 0)) return refuse(FA_INVALID_ARGUMENT, "negativeThresholdOffset must be non-negative");
    if (!(c.min_silence_at_max_speech >= 0)) return refuse(FA_INVALID_ARGUMENT, "minSilenceAtMaxSpeech must be non-negative");
    if (c.has_negative_threshold && !(c.negative_threshold >= 0 && c.negative_threshold <= 1)) return refuse(FA_INVALID_ARGUMENT, "negativeThreshold must be in [0, 1]");
    Operands r{};
    if (c.has_negative_threshold) {          // :31-35 and effectiveNegativeThreshold, in fp32
        const float sum = c.negative_threshold + c.negative_threshold_offset;
        r.threshold = sum < 1.0f ? sum : 1.0f;                          // min(1.0, x): x unless 1.0 is smaller
        r.negative_threshold = c.negative_threshold;
    } else {
        r.threshold = c.default_threshold;
        const float diff = c.default_threshold - c.negative_threshold_offset;
        r.negative_threshold = 0.01f >= diff ? 0.01f : diff;            // max(x, 0.01) is `0.01 >= x ? 0.01 : x`: a NaN passes through
    }
    r.split_threshold = c.silence_threshold_for_split;
    r.use_max = c.use_max_possible_silence_at_max_speech ? 1 : 0;
    if (!to_samples(c.min_speech_duration, &r.min_speech) || !to_samples(c.speech_padding, &r.pad) || !to_samples(c.min_silence_duration, &r.min_silence) ||
        !to_samples(c.min_silence_at_max_speech, &r.min_silence_at_max))
        return refuse(FA_INVALID_ARGUMENT, "a duration times the sample rate does not fit Int");
    int64_t two_pad = 0;
    if (__builtin_mul_overflow(r.pad, int64_t{2}, &two_pad)) return refuse(FA_INVALID_ARGUMENT, "twice the padding does not fit Int");
    if (std::isinf(c.max_speech_duration)) {
        r.max_speech = kNone;
    } else {
        int64_t raw = 0;
        if (!to_samples(c.max_speech_duration, &raw)) return refuse(FA_INVALID_ARGUMENT, "a duration times the sample rate does not fit Int");
        if (__builtin_sub_overflow(raw, int64_t{kChunk}, &raw) || __builtin_sub_overflow(raw, two_pad, &raw))
            return refuse(FA_INVALID_ARGUMENT, "the maximal speech less the padding does not fit Int");
        r.max_speech = raw > 0 ? raw : 0;
    }
    *o = r;
    return Verdict{};
}

// ---- segments
struct SegRecording {
    int64_t frame0;                          // first frame in the array the kernel is given
    int64_t raw0;                            // first slot of the recording's slice of raw speeches
    int32_t frames;                          // 0 when the recording yields nothing (no frames, or total_samples <= 0)
    int32_t pad;
    int64_t total;                           // total_samples
};

struct RawSpeech {                           // both in frames: start * 4096 and min(end * 4096, total) are the samples
    int32_t start;
    int32_t end;                             // -1: the tail flush, which ends at total
};

struct SegPlan {
    std::vector<SegRecording> rec;
    int64_t frames = 0;                      // frames uploaded by the host-pointer entry: frame_range[batch] - frame_range[0]
    int64_t raw_slots = 0;                   // slots of the raw workspace: one per frame of a recording that can yield something
    int64_t out_slots = 0;                   // records of the device arena: min(capacity, raw_slots), none without an output
};

// device: the probabilities are addressed from the caller's array (frame_range as given); otherwise from frame_range[0], where the upload starts
inline Verdict plan_segments(const fa_vad_segmentation_config &c, const void *probs, const int64_t *frame_range, const int64_t *total_samples, const int32_t batch,
                             const void *segs, const int64_t capacity, const void *count, const bool device, Operands *o, SegPlan *p) {
    if (batch < 0 || capacity < 0 || !count) return refuse(FA_INVALID_ARGUMENT, "vad_segments: bad arguments");
    const Verdict v = derive(c, o);
    if (v.status != FA_SUCCESS) return v;
    if (batch > 0 && (!frame_range || !total_samples)) return refuse(FA_INVALID_ARGUMENT, "vad_segments: frame_range and total_samples are required");
    if (batch > 0 && frame_range[0] < 0) return refuse(FA_INVALID_ARGUMENT, "vad_segments: frame_range starts below 0");
    p->rec.assign(static_cast<size_t>(batch), SegRecording{});
    for (int32_t b = 0; b < batch; ++b) {
        const int64_t n = frame_range[b + 1] - frame_range[b];
        if (frame_range[b + 1] < frame_range[b]) return refuse(FA_INVALID_ARGUMENT, "vad_segments: frame_range descends at recording %d", b);
        if (n > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "vad_segments: recording %d has 2^31 frames or more", b);
        SegRecording &r = p->rec[static_cast<size_t>(b)];
        r.frame0 = frame_range[b] - (device ? 0 : frame_range[0]);
        r.raw0 = p->raw_slots;
        r.frames = total_samples[b] > 0 ? static_cast<int32_t>(n) : 0;
        r.total = total_samples[b];
        p->raw_slots += r.frames;
    }
    p->frames = batch > 0 ? frame_range[batch] - frame_range[0] : 0;
    if (p->frames > 0 && !probs) return refuse(FA_INVALID_ARGUMENT, "vad_segments: probs is NULL");
    p->out_slots = segs ? (capacity < p->raw_slots ? capacity : p->raw_slots) : 0;
    return Verdict{};
}

struct SegArgs {
    const float *probs;
    const SegRecording *rec;                 // [batch]
    int32_t batch;
    Operands o;
    RawSpeech *raw;                          // [raw_slots]
    int32_t *raw_counts;                     // [batch]: what vad_machine flushed, also beyond the slice
    int32_t *kept;                           // [batch]: records of the recording; scan_totals turns them into offsets
    int32_t *kept_counts;                    // [batch]: the same, left as counts
    int32_t *total;                          // [1]
    fa_vad_segment *out;                     // [out_slots]
    int64_t out_slots;
};

#if defined(__HIPCC__)
// vad_machine, vad_count, scan_totals and vad_write, in stream order
void launch_segments(hipStream_t stream, const SegArgs &a);
#endif

// ---- the model rows
constexpr int64_t chunk_count(const int64_t n) { return n > 0 ? (n + kChunk - 1) / kChunk : 0; }

// chunk_range is written (when it is there and the offsets are sound) before the capacity is judged
inline Verdict plan_pack(const void *audio, const int64_t *audio_offsets, const int32_t batch, const void *rows, const int64_t row_capacity, int64_t *chunk_range) {
    if (batch < 0 || row_capacity < 0) return refuse(FA_INVALID_ARGUMENT, "vad_pack_chunks: bad arguments");
    if (batch == 0) return Verdict{};
    if (!audio_offsets || !chunk_range) return refuse(FA_INVALID_ARGUMENT, "vad_pack_chunks: audio_offsets and chunk_range are required");
    if (audio_offsets[0] < 0) return refuse(FA_INVALID_ARGUMENT, "vad_pack_chunks: audio_offsets starts below 0");
    for (int32_t b = 0; b < batch; ++b)
        if (audio_offsets[b + 1] < audio_offsets[b]) return refuse(FA_INVALID_ARGUMENT, "vad_pack_chunks: audio_offsets descends at recording %d", b);
    chunk_range[0] = 0;
    for (int32_t b = 0; b < batch; ++b) chunk_range[b + 1] = chunk_range[b] + chunk_count(audio_offsets[b + 1] - audio_offsets[b]);
    if (chunk_range[batch] > 0 && (!audio || !rows)) return refuse(FA_INVALID_ARGUMENT, "vad_pack_chunks: audio and rows are required");
    if (chunk_range[batch] > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "vad_pack_chunks: more than INT32_MAX rows");
    if (chunk_range[batch] > row_capacity)
        return refuse(FA_OUTPUT_TOO_SMALL, "vad_pack_chunks: output holds %lld of %lld rows", (long long)row_capacity, (long long)chunk_range[batch]);
    return Verdict{};
}

struct PackGroup {                           // up to kPackGroup recordings, by value in the launch's arguments: no table to upload
    int64_t audio_off[kPackGroup + 1];       // from the array the kernel is given
    int64_t row_off[kPackGroup + 1];         // rows from the group's first row
    int32_t count;
};

#if defined(__HIPCC__)
// one launch per group that has rows, on the stream; rows: the group's first row.  wide: 16-byte stores (rows is 16-byte aligned)
void launch_pack(hipStream_t stream, const float *audio, const PackGroup &g, float *rows, bool wide);
#endif

// ---- the speech audio
struct GatherPlan {
    std::vector<int64_t> src;                // [n]: first sample of a segment in the array the kernel is given
    std::vector<int64_t> tile_off;           // [n + 1]: tiles of kGatherTile samples in front of a segment
};

// out_range is written before the capacity is judged.  device as in plan_segments: the host entry uploads from audio_offsets[0] on.
inline Verdict plan_gather(const void *audio, const int64_t *audio_offsets, const int32_t batch, const fa_vad_segment *segs, const int64_t n_segments, const void *out,
                           const int64_t out_capacity, int64_t *out_range, const bool device, GatherPlan *p) {
    if (batch < 0 || n_segments < 0 || out_capacity < 0 || !out_range) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: bad arguments");
    if (batch > 0 && !audio_offsets) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: audio_offsets is required");
    if (batch > 0 && audio_offsets[0] < 0) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: audio_offsets starts below 0");
    for (int32_t b = 0; b < batch; ++b)
        if (audio_offsets[b + 1] < audio_offsets[b]) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: audio_offsets descends at recording %d", b);
    if (n_segments > 0 && !segs) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: segs is NULL");
    p->src.assign(static_cast<size_t>(n_segments), 0);
    p->tile_off.assign(static_cast<size_t>(n_segments) + 1, 0);
    out_range[0] = 0;
    for (int64_t i = 0; i < n_segments; ++i) {
        const fa_vad_segment &s = segs[i];
        if (s.recording < 0 || s.recording >= batch) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: segment %lld names recording %d", (long long)i, s.recording);
        int64_t start = 0, end = 0;          // VadSegment.startSample / endSample: Int(time * Double(sampleRate))
        if (!to_samples(s.start_time, &start) || !to_samples(s.end_time, &end)) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: a time of segment %lld does not fit Int", (long long)i);
        const int64_t n = audio_offsets[s.recording + 1] - audio_offsets[s.recording];
        const int64_t lo = std::max<int64_t>(0, std::min(start, n)), hi = std::max(lo, std::min(end, n));   // :63-64
        p->src[static_cast<size_t>(i)] = audio_offsets[s.recording] - (device ? 0 : audio_offsets[0]) + lo;
        out_range[i + 1] = out_range[i] + (hi - lo);
        p->tile_off[static_cast<size_t>(i) + 1] = p->tile_off[static_cast<size_t>(i)] + (hi - lo + kGatherTile - 1) / kGatherTile;
    }
    if (out_range[n_segments] > 0 && (!audio || !out)) return refuse(FA_INVALID_ARGUMENT, "vad_gather_segments: audio and out are required");
    if (out_range[n_segments] > out_capacity)
        return refuse(FA_OUTPUT_TOO_SMALL, "vad_gather_segments: output holds %lld of %lld samples", (long long)out_capacity, (long long)out_range[n_segments]);
    if (p->tile_off[static_cast<size_t>(n_segments)] > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "vad_gather_segments: more than INT32_MAX workgroups");
    return Verdict{};
}

struct GatherArgs {
    const float *audio;
    float *out;
    const int64_t *src, *out_range, *tile_off;   // device copies of the plan's tables and of out_range
    int64_t n_segments;
    int32_t tiles;
};
#if defined(__HIPCC__)
void launch_gather(hipStream_t stream, const GatherArgs &a);
#endif

// ---- streaming
// pow(10.0, Double(timeResolution)) for 0 ... 22: every product is exact
inline double resolution_factor(const int32_t time_resolution) {
    double f = 1.0;
    for (int32_t i = 0; i < time_resolution; ++i) f *= 10.0;
    return f;
}

inline Verdict plan_stream(const fa_vad_segmentation_config &c, const void *probs, const int32_t *chunk_counts, const int32_t streams, const int32_t max_chunks,
                           const fa_vad_stream_state *states, const int32_t time_resolution, const void *events, const int64_t capacity, const void *count, Operands *o) {
    if (streams < 0 || max_chunks < 0 || capacity < 0 || !count) return refuse(FA_INVALID_ARGUMENT, "vad_stream_advance: bad arguments");
    const Verdict v = derive(c, o);
    if (v.status != FA_SUCCESS) return v;
    if (time_resolution < 0 || time_resolution > 22) return refuse(FA_INVALID_ARGUMENT, "vad_stream_advance: time_resolution is 0 ... 22");
    if (streams > 0 && (!chunk_counts || !states)) return refuse(FA_INVALID_ARGUMENT, "vad_stream_advance: chunk_counts and states are required");
    bool any = false;
    for (int32_t s = 0; s < streams; ++s) {
        if (chunk_counts[s] < 0 || chunk_counts[s] > max_chunks) return refuse(FA_INVALID_ARGUMENT, "vad_stream_advance: stream %d has a chunk count outside [0, max_chunks]", s);
        any = any || chunk_counts[s] > 0;
    }
    if (any && !probs) return refuse(FA_INVALID_ARGUMENT, "vad_stream_advance: probs is NULL");
    if (static_cast<int64_t>(streams) * max_chunks > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "vad_stream_advance: more than INT32_MAX chunks in the call");
    (void)events;
    return Verdict{};
}

struct StreamArgs {
    const float *probs;                      // [streams][max_chunks]
    const int32_t *chunk_counts;             // [streams]
    const int32_t *chunk_samples;            // [streams][max_chunks] or nullptr: 4096
    int32_t streams, max_chunks;
    Operands o;
    int32_t return_seconds;
    double factor;
    fa_vad_stream_state *states;             // [streams], in and out
    fa_vad_stream_event *events;             // [streams][max_chunks]: kind -1 where a chunk has no event
};
#if defined(__HIPCC__)
void launch_stream(hipStream_t stream, const StreamArgs &a);
#endif

}  // namespace vad
}  // namespace fa
