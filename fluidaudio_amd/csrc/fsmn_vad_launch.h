// fsmn_vad_launch.h — what the host side of FSMN-VAD (fsmn_vad_host.hip: the C ABI, uploads, the synchronisation of a call) and its
// kernels (fsmn_vad.hip) share: the argument pass of every entry (plain C++: decided from the arguments alone, nothing is written but the
// plan and the ranges), the chunk schedule, the kernels' operands and their launchers.  The integers and the word step are in
// fsmn_vad_core.h.  Internal; not part of the C ABI.  The stand-alone program tests/cpu/fsmn_vad_core_main.cpp walks both on the host.
//
// Restated: FsmnVadManager (Sources/FluidAudio/VAD/Fsmn/FsmnVadManager.swift) — concatenateChunks :91-109, lfrFrameCount :113-117, the
// rows of chunkSilence :119-155 (the scaled waveform :123, the zero-padded bucket :131-140, the strided gather :146-153) and decide
// :159-201.  OUT OF SCOPE: the preprocessor and the scorer (the caller's), detect(audioURL:)'s file reading and resampling.
//
// A recording of F frames closes at most F segments: every segment opens at a frame of its own.  The kernel counts beyond a recording's
// slice without writing, and a slice never needs more than `capacity` records: when a recording closes more, the output is too small
// whatever the others do, and the first `capacity` records of the call lie in the slices up to that one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fa_verdict.h"
#include "fsmn_vad_core.h"
#include "row_pack_launch.h"

namespace fa {
namespace fsmnvad {

constexpr int kGroup = rows::kGroup;          // chunks whose operands travel in one launch's arguments: nothing is staged, no entry waits

inline fa_fsmn_vad_config config_or_default(const fa_fsmn_vad_config *cfg) {
    if (cfg) return *cfg;
    return fa_fsmn_vad_config{0.2f, 20, 15, 15, 80, 20, 10, 6000, 10};   // FsmnVadManager.swift:37-45
}

inline Verdict derive(const fa_fsmn_vad_config &c, Params *o) {
    if (std::isnan(c.silence_threshold)) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad: silence_threshold is NaN");
    if (c.window_frames < 1 || c.window_frames > kWave) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad: window_frames is 1 ... 64");
    if (c.sil_to_speech_frames < 0 || c.sil_to_speech_frames > c.window_frames || c.speech_to_sil_frames < 0 || c.speech_to_sil_frames > c.window_frames)
        return refuse(FA_INVALID_ARGUMENT, "fsmn_vad: a threshold count is 0 ... window_frames");
    if (c.max_end_silence_frames < 1 || c.max_segment_frames < 1 || c.frame_ms < 1)
        return refuse(FA_INVALID_ARGUMENT, "fsmn_vad: max_end_silence_frames, max_segment_frames and frame_ms are at least 1");
    if (c.lookback_frames < 0 || c.lookahead_frames < 0) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad: lookback_frames and lookahead_frames are not negative");
    *o = Params{c.silence_threshold, c.window_frames, c.sil_to_speech_frames, c.speech_to_sil_frames, c.max_end_silence_frames, c.lookback_frames, c.lookahead_frames,
                c.max_segment_frames, c.frame_ms};
    return Verdict{};
}

// ---- the chunk schedule: concatenateChunks (:91-109) with lfrFrameCount standing for the scorer's frame count
// visit(start, end, frames, keep_from, first_frame) per kept chunk; returns the frames of the concatenated array
template <class Visit>
inline int64_t schedule(const int64_t samples, const Visit &visit) {
    int64_t start = 0, so_far = 0;
    while (start < samples) {
        const int64_t end = std::min(start + kChunkSamples, samples);
        const int64_t frames = frame_count(end - start);
        const int64_t keep_from = start == 0 ? 0 : kLfrPad;
        if (!(frames > keep_from)) break;
        visit(start, end, frames, keep_from, so_far);
        so_far += frames - keep_from;
        if (end == samples) break;
        start = (so_far - kLfrPad) * kHop;
    }
    return so_far;
}

// The ranges are written (when they are there and the lengths are sound) before the capacity is judged; records beyond it are not.
inline Verdict plan_chunks(const int64_t *total_samples, const int32_t batch, fa_fsmn_vad_chunk *chunks, const int64_t capacity, int64_t *count, int64_t *chunk_range,
                           int64_t *frame_range) {
    if (batch < 0 || capacity < 0 || !count) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_plan_chunks: bad arguments");
    if (batch > 0 && (!total_samples || !chunk_range || !frame_range)) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_plan_chunks: total_samples and the two ranges are required");
    for (int32_t b = 0; b < batch; ++b)
        if (total_samples[b] > INT64_MAX - kChunkSamples) return refuse(FA_INDEX_OVERFLOW, "fsmn_vad_plan_chunks: recording %d is too long", b);
    int64_t n = 0, frames = 0;
    if (chunk_range) chunk_range[0] = 0;
    if (frame_range) frame_range[0] = 0;
    for (int32_t b = 0; b < batch; ++b) {
        frames += schedule(total_samples[b], [&](const int64_t start, const int64_t end, const int64_t f, const int64_t keep_from, const int64_t first) {
            if (chunks && n < capacity) chunks[n] = fa_fsmn_vad_chunk{b, bucket_for(f), start, end, static_cast<int32_t>(f), static_cast<int32_t>(keep_from), first};
            ++n;
        });
        chunk_range[b + 1] = n;
        frame_range[b + 1] = frames;
    }
    *count = n;
    if (chunks && capacity < n) return refuse(FA_OUTPUT_TOO_SMALL, "fsmn_vad_plan_chunks: output holds %lld of %lld chunks", (long long)capacity, (long long)n);
    return Verdict{};
}

// ---- segments
struct SegRecording {
    int64_t frame0;                          // first frame in the array the kernel is given
    int64_t slot0;                           // first record of the recording's slice of the arena
    int32_t frames;
    int32_t slots;                           // min(frames, capacity); 0 without an output
};

struct RawSegment {
    int32_t start, end, reason;
};

struct SegPlan {
    std::vector<SegRecording> rec;
    int64_t frames = 0;                      // frames uploaded by the host-pointer entry: frame_range[batch] - frame_range[0]
    int64_t arena = 0;                       // records of all slices
    int64_t out_slots = 0;                   // records of the device output: min(capacity, arena)
};

// device: the probabilities are addressed from the caller's array (frame_range as given); otherwise from frame_range[0], where the upload starts
inline Verdict plan_segments(const fa_fsmn_vad_config &c, const void *probs, const int64_t *frame_range, const int32_t batch, const void *segs, const int64_t capacity,
                             const void *count, const bool device, Params *o, SegPlan *p) {
    if (batch < 0 || capacity < 0 || !count) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_segments: bad arguments");
    const Verdict v = derive(c, o);
    if (v.status != FA_SUCCESS) return v;
    if (batch > 0 && !frame_range) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_segments: frame_range is required");
    if (batch > 0 && frame_range[0] < 0) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_segments: frame_range starts below 0");
    p->rec.assign(static_cast<size_t>(batch), SegRecording{});
    for (int32_t b = 0; b < batch; ++b) {
        if (frame_range[b + 1] < frame_range[b]) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_segments: frame_range descends at recording %d", b);
        const int64_t n = frame_range[b + 1] - frame_range[b];
        if (n > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "fsmn_vad_segments: recording %d has 2^31 frames or more", b);
        if (n + o->lookahead > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "fsmn_vad_segments: recording %d with the look-ahead reaches frame 2^31", b);
        SegRecording &r = p->rec[static_cast<size_t>(b)];
        r.frame0 = frame_range[b] - (device ? 0 : frame_range[0]);
        r.slot0 = p->arena;
        r.frames = static_cast<int32_t>(n);
        r.slots = segs ? static_cast<int32_t>(std::min<int64_t>(n, capacity)) : 0;
        p->arena += r.slots;
    }
    p->frames = batch > 0 ? frame_range[batch] - frame_range[0] : 0;
    if (p->frames > 0 && !probs) return refuse(FA_INVALID_ARGUMENT, "fsmn_vad_segments: probs is NULL");
    if (p->arena > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "fsmn_vad_segments: more than INT32_MAX records in the arena");
    p->out_slots = std::min(capacity, p->arena);
    return Verdict{};
}

struct SegArgs {
    const float *probs;
    const SegRecording *rec;                 // [batch]
    int32_t batch;
    Params o;
    RawSegment *arena;                       // [arena]
    int32_t *counts;                         // [batch]: segments closed, also beyond the slice
    int32_t *kept;                           // [batch]: min(count, slots); scan_totals turns them into offsets
    int32_t *total;                          // [1]
    fa_fsmn_vad_segment *out;                // [out_slots]
    int64_t out_slots;
};

#if defined(__HIPCC__)
// fsmn_vad_machine, scan_totals and fsmn_vad_write, in stream order
void launch_segments(hipStream_t stream, const SegArgs &a);
#endif

// ---- round the two networks: a run of chunk records
// what every entry asks of its records; `lengths` HOST int64[batch + 1] are the recordings' samples (audio_offsets) or nullptr
inline Verdict check_chunks(const char *who, const fa_fsmn_vad_chunk *chunks, const int64_t n, const int32_t batch, const int64_t *lengths) {
    if (n > 0 && !chunks) return refuse(FA_INVALID_ARGUMENT, "%s: chunks is NULL", who);
    for (int64_t i = 0; i < n; ++i) {
        const fa_fsmn_vad_chunk &c = chunks[i];
        if (c.recording < 0 || c.recording >= batch) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld names recording %d", who, (long long)i, c.recording);
        if (c.start_sample < 0 || c.end_sample < c.start_sample || (lengths && c.end_sample > lengths[c.recording + 1] - lengths[c.recording]))
            return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld lies outside its recording", who, (long long)i);
        if (c.frames < 0 || c.keep_from < 0 || c.first_frame < 0) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld has a negative count", who, (long long)i);
    }
    return Verdict{};
}

inline Verdict plan_pack(const void *audio, const int64_t *audio_offsets, const int32_t batch, const fa_fsmn_vad_chunk *chunks, const int64_t n, const void *rows,
                         const int64_t row_stride, const int64_t row_capacity) {
    const char *who = "fsmn_vad_pack_waveforms";
    if (batch < 0 || n < 0 || row_stride < 0 || row_capacity < 0) return refuse(FA_INVALID_ARGUMENT, "%s: bad arguments", who);
    if (n == 0) return Verdict{};
    if (!audio_offsets) return refuse(FA_INVALID_ARGUMENT, "%s: audio_offsets is required", who);
    if (batch > 0 && audio_offsets[0] < 0) return refuse(FA_INVALID_ARGUMENT, "%s: audio_offsets starts below 0", who);
    for (int32_t b = 0; b < batch; ++b)
        if (audio_offsets[b + 1] < audio_offsets[b]) return refuse(FA_INVALID_ARGUMENT, "%s: audio_offsets descends at recording %d", who, b);
    const Verdict v = check_chunks(who, chunks, n, batch, audio_offsets);
    if (v.status != FA_SUCCESS) return v;
    for (int64_t i = 0; i < n; ++i)
        if (chunks[i].end_sample - chunks[i].start_sample > row_stride) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld is longer than row_stride", who, (long long)i);
    if (!audio || !rows) return refuse(FA_INVALID_ARGUMENT, "%s: audio and rows are required", who);
    if (n > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "%s: more than INT32_MAX rows", who);
    if (n > row_capacity) return refuse(FA_OUTPUT_TOO_SMALL, "%s: output holds %lld of %lld rows", who, (long long)row_capacity, (long long)n);
    return Verdict{};
}

inline Verdict plan_feats(const void *feats, const int32_t dtype, const int64_t feat_stride, const fa_fsmn_vad_chunk *chunks, const int64_t n, const int32_t bucket,
                          const void *out) {
    const char *who = "fsmn_vad_pack_feats_dev";
    if (n < 0 || feat_stride < 0 || bucket < 0 || (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16)) return refuse(FA_INVALID_ARGUMENT, "%s: bad arguments", who);
    if (n == 0) return Verdict{};
    const Verdict v = check_chunks(who, chunks, n, INT32_MAX, nullptr);
    if (v.status != FA_SUCCESS) return v;
    for (int64_t i = 0; i < n; ++i) {
        if (chunks[i].frames > bucket) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld has more frames than the bucket", who, (long long)i);
        if (chunks[i].frames > feat_stride) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld has more frames than feat_stride", who, (long long)i);
    }
    if (bucket > 0 && (!out || !feats)) return refuse(FA_INVALID_ARGUMENT, "%s: feats and out are required", who);
    if (n > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "%s: more than INT32_MAX chunks", who);
    return Verdict{};
}

struct FeatGroup {
    int32_t frames[kGroup];
    int32_t count;
};

inline Verdict plan_gather(const void *scores, const int32_t dtype, const int32_t bucket, const int32_t vocab, const fa_fsmn_vad_chunk *chunks, const int64_t n,
                           const int64_t *frame_range, const int32_t batch, const void *silence, const int64_t capacity) {
    const char *who = "fsmn_vad_gather_silence_dev";
    if (n < 0 || batch < 0 || bucket < 0 || vocab < 1 || capacity < 0 || (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16)) return refuse(FA_INVALID_ARGUMENT, "%s: bad arguments", who);
    if (n == 0) return Verdict{};
    if (!frame_range) return refuse(FA_INVALID_ARGUMENT, "%s: frame_range is required", who);
    if (batch > 0 && frame_range[0] < 0) return refuse(FA_INVALID_ARGUMENT, "%s: frame_range starts below 0", who);
    for (int32_t b = 0; b < batch; ++b)
        if (frame_range[b + 1] < frame_range[b]) return refuse(FA_INVALID_ARGUMENT, "%s: frame_range descends at recording %d", who, b);
    const Verdict v = check_chunks(who, chunks, n, batch, nullptr);
    if (v.status != FA_SUCCESS) return v;
    bool any = false;
    for (int64_t i = 0; i < n; ++i) {
        const fa_fsmn_vad_chunk &c = chunks[i];
        if (c.frames > bucket) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld has more frames than the bucket", who, (long long)i);
        if (c.frames <= c.keep_from) continue;
        any = true;
        const int64_t kept = c.frames - c.keep_from, room = frame_range[c.recording + 1] - frame_range[c.recording];
        if (c.first_frame > room || kept > room - c.first_frame) return refuse(FA_INVALID_ARGUMENT, "%s: chunk %lld ends beyond its recording's frames", who, (long long)i);
    }
    if (any && (!scores || !silence)) return refuse(FA_INVALID_ARGUMENT, "%s: scores and silence are required", who);
    if (batch > 0 && frame_range[batch] > capacity)
        return refuse(FA_OUTPUT_TOO_SMALL, "%s: output holds %lld of %lld frames", who, (long long)capacity, (long long)frame_range[batch]);
    if (n > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "%s: more than INT32_MAX chunks", who);
    return Verdict{};
}

struct GatherGroup {
    int64_t dst[kGroup];                     // where the chunk's first kept frame goes
    int32_t keep_from[kGroup], frames[kGroup];
    int32_t count;
};

#if defined(__HIPCC__)
// a chunk is a row of a rows::Group (row_pack_launch.h): src its first sample in the array the kernel is given, len its samples.
// rows: the group's first row.  wide: 16-byte stores (rows is 16-byte aligned and row_stride a multiple of 4)
void launch_pack(hipStream_t stream, const float *audio, const rows::Group &g, float *rows, int64_t row_stride, bool wide);
// feats / out: the group's first chunk.  wide: feats and out are 16-byte aligned (8-byte for fp16 feats)
void launch_feats(hipStream_t stream, const void *feats, int32_t dtype, int64_t feat_stride, const FeatGroup &g, int32_t bucket, float *out, bool wide);
void launch_gather(hipStream_t stream, const void *scores, int32_t dtype, int32_t bucket, int32_t vocab, const GatherGroup &g, float *silence);
#endif

}  // namespace fsmnvad
}  // namespace fa
