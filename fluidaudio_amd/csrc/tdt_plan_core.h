// tdt_plan_core.h — the integer arithmetic of the TDT window planner that host and device share (kernels: tdt_plan.hip, host side:
// tdt_plan_host.hip, operands and argument pass: tdt_plan_launch.h): the layout, the fill of the last window and one turn of the window
// loop.  Plain C++ (tests/cpu/tdt_plan_core.cpp walks it on the host against tests/tdt_plan_restatement.py); the same text is
// __host__ __device__ under hipcc.
//
// Restated from FluidAudio/ASR/Parakeet/SlidingWindow/TDT/ChunkProcessor.swift: chunkLayout :48-75 and :140-161,
// lastChunkWarmupSamples :85-102, the body of process' window loop :520-565 and :577, transcribeChunk's frame counts :771-778, and
// ASRConstants.calculateEncoderFrames (Shared/ASRConstants.swift:71-73).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fluidaudio_hip.h"

#if defined(__HIPCC__)
#define FA_TP_HD __host__ __device__
#else
#define FA_TP_HD
#endif

namespace fa {
namespace tdt_plan {

constexpr int kMinOverlapFrames = 6;         // minimumOverlapSamples = frameSamples * 6 (:198)

// What the reference derives from its constants and the mode, in samples unless it says frames.
struct Geometry {
    int64_t frame, chunk, stride, mel_context, warmup_prefix, max_model;
    int64_t lookahead, stable_quiet, probe_window;   // shouldUseWarmupPrefix :351-353
    int32_t silence_radius, valley_radius;           // frames (:195-196)
    int32_t end_aligned;
    int32_t aligned;                                 // chunkStarts takes silenceAlignedChunkStarts (:169)
    int32_t can_warmup;                              // warmupPrefixSamples > 0
    int32_t pad;
};

template <class T> FA_TP_HD inline T lesser(const T a, const T b) { return b < a ? b : a; }
template <class T> FA_TP_HD inline T greater(const T a, const T b) { return a < b ? b : a; }

// chunkLayout with `warmup_prefix_frames` as the prefix; `requested_overlap` is Int(overlapSeconds * Double(sampleRate)), which the
// caller has checked to fit.  With the defaults: 238 080 / 206 080 with the mel context, 239 360 / 207 360 without.
FA_TP_HD inline void layout(const int64_t frame, const int64_t mel_hop, const int64_t max_model, const int64_t requested_overlap, const bool mel_chunk_context,
                            const int64_t warmup_prefix_frames, Geometry *g) {
    g->frame = frame;
    g->max_model = max_model;
    g->mel_context = mel_chunk_context ? frame : 0;                                      // :34, :48-50
    g->warmup_prefix = mel_chunk_context ? 0 : warmup_prefix_frames * frame;             // :43-45, :52-55
    const int64_t raw = greater(max_model - g->mel_context - mel_hop, frame);            // :59-64
    g->chunk = raw / frame * frame;
    const int64_t overlap = lesser(requested_overlap, g->chunk / 2) / frame * frame;     // :66-70
    g->stride = greater(g->chunk - overlap, frame) / frame * frame;                      // :72-75
}

FA_TP_HD inline int64_t last_chunk_warmup(const int64_t chunk_start, const int64_t default_warmup, const int64_t chunk, const int64_t total, const int64_t speech_end,
                                          const int64_t frame) {
    const int64_t default_visible = greater(frame, chunk - default_warmup);
    const bool is_last = chunk_start + default_visible >= total;
    const int64_t remaining = lesser(speech_end, total) - chunk_start;
    if (!(is_last && remaining > 0 && chunk_start > 0)) return default_warmup;
    const int64_t fill = (chunk - remaining) / frame * frame;                            // frame-aligned: the suppression boundary is a frame
    if (!(fill > 0)) return default_warmup;
    const int64_t available = chunk_start / frame * frame;
    return greater(default_warmup, lesser(available, fill));
}

// Int(ceil(Double(samples) / Double(samplesPerEncoderFrame)))
FA_TP_HD inline int64_t encoder_frames(const int64_t samples, const int64_t frame) {
    return static_cast<int64_t>(ceil(static_cast<double>(samples) / static_cast<double>(frame)));
}

// One turn of the loop `while chunkStart < totalSamples` for window `index` at `chunk_start`: whether it leaves a record, and whether
// the loop ends with it.
struct Turn {
    fa_tdt_window w;
    bool record;                             // false: the loop ended in front of this window (:520, :545, :552)
    bool ends;                               // the loop ends here: no record, or the last chunk (:626)
};

FA_TP_HD inline Turn turn(const Geometry &g, const int32_t recording, const int64_t total, const int64_t speech_end, const int64_t chunk_start, const bool use_warmup,
                          const int64_t index) {
    Turn t{};
    t.record = false;
    t.ends = true;
    if (!(chunk_start < total)) return t;
    const int64_t default_warmup = index > 0 && use_warmup ? lesser(g.warmup_prefix, chunk_start) : 0;
    const int64_t warmup = g.end_aligned ? last_chunk_warmup(chunk_start, default_warmup, g.chunk, total, speech_end, g.frame) : default_warmup;
    const int64_t visible = greater(g.frame, g.chunk - warmup);
    const int64_t candidate_end = chunk_start + visible;
    const bool is_last = candidate_end >= total;
    const int64_t chunk_end = is_last ? total : candidate_end;
    if (chunk_end <= chunk_start) return t;
    const int64_t audio_end = is_last && g.end_aligned ? lesser(chunk_end, speech_end) : chunk_end;
    if (audio_end <= chunk_start) return t;                                              // a pure-silence tail
    const int64_t context = warmup > 0 ? 0 : (index > 0 ? g.mel_context : 0);
    const int64_t context_start = chunk_start - greater(warmup, context);
    const int64_t offset = warmup > 0 ? context_start : chunk_start;                     // chunkStartOffset :577
    t.record = true;
    t.ends = is_last;
    t.w.recording = recording;
    t.w.use_warmup_prefix = use_warmup ? 1 : 0;
    t.w.is_last = is_last ? 1 : 0;
    t.w.emit_after_frame = warmup > 0 ? static_cast<int32_t>(chunk_start / g.frame) : -1;
    t.w.global_frame_offset = static_cast<int32_t>(offset / g.frame);
    t.w.context_frames = static_cast<int32_t>(context / g.frame);
    t.w.actual_audio_frames = static_cast<int32_t>(encoder_frames(audio_end - context_start - context, g.frame));
    t.w.reserved = 0;
    t.w.chunk_start = chunk_start;
    t.w.warmup_samples = warmup;
    t.w.context_samples = context;
    t.w.context_start = context_start;
    t.w.length = audio_end - context_start;
    return t;
}

// The entries of a recording's list of chunk starts: 0 and one per multiple of the stride below n.
FA_TP_HD inline int64_t listed_starts(const Geometry &g, const int64_t n) { return n > 0 ? 1 + (n - 1) / g.stride : 0; }

// The most windows a recording of n samples can get.  The listed starts ascend strictly and lie below n; a window whose start is not
// below n leaves no record.  Regular starts are every multiple of the stride below n, so a step beyond the list ends the loop.
// Aligned starts may lie in front of their targets, so the loop can step beyond the list: by the stride each time, from a start that is
// not negative, and below n — at most (n - 1) / stride times.
FA_TP_HD inline int64_t window_count_bound(const Geometry &g, const int64_t n) {
    if (n <= 0) return 0;
    return listed_starts(g, n) + (g.aligned ? (n - 1) / g.stride : 0);
}

// Entries of a recording's boundary table: frame f stands for the window [f F - F, f F + F) clipped to the recording, for every f
// whose window holds a sample.
FA_TP_HD inline int64_t table_entries(const int64_t frame, const int64_t n) { return n > 0 ? (n - 1) / frame + 2 : 0; }

}  // namespace tdt_plan
}  // namespace fa
