// tdt_plan_launch.h — what the host side of the TDT window planner (tdt_plan_host.hip: the C ABI, uploads, the synchronisation of a
// call) and its kernels (tdt_plan.hip) share: the argument pass of the entries (plain C++: decided from the arguments alone, nothing
// is written but the plan and, where the header says so, a range), the geometry the reference derives from its constants, the layout
// of the workspace, the kernels' operands and their launchers.  The integer arithmetic itself is tdt_plan_core.h.  Internal; not part
// of the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fa_verdict.h"
#include "row_pack_launch.h"
#include "tdt_plan_core.h"

namespace fa {
namespace tdt_plan {

constexpr int kWave = 64;
constexpr int kEnergyBlock = 128;            // frames of a workgroup of the energy kernel
constexpr int kStage = 32;                   // samples of a lane's run that pass through LDS at a time
constexpr int kMaxRadius = 63;               // candidates of a search: 2 * 63 + 1 <= 128 slots

inline fa_tdt_window_config config_or_default(const fa_tdt_window_config *cfg) {
    if (cfg) return *cfg;
    fa_tdt_window_config c{};
    c.sample_rate = 16000; c.frame_samples = 1280; c.mel_hop = 160; c.max_model_samples = 240000;
    c.overlap_seconds = 2.0;
    c.mel_chunk_context = 1; c.silence_aligned = 0; c.warmup_prefix_frames = 0; c.end_aligned = 1;
    return c;
}

// Int(x) of a fp64 value known to lie in int32: truncation
inline bool to_int32(const double x, int64_t *out) {
    if (!(x > -2147483649.0 && x < 2147483648.0)) return false;
    *out = static_cast<int64_t>(x);
    return true;
}

inline Verdict derive(const fa_tdt_window_config &c, Geometry *g) {
    if (c.sample_rate < 1 || c.frame_samples < 1 || c.mel_hop < 1 || c.max_model_samples < 1) return refuse(FA_INVALID_ARGUMENT, "tdt_plan: the geometry holds a size below 1");
    if (c.warmup_prefix_frames < 0) return refuse(FA_INVALID_ARGUMENT, "tdt_plan: warmup_prefix_frames is negative");
    int64_t requested = 0;
    if (!std::isfinite(c.overlap_seconds) || c.overlap_seconds < 0 || !to_int32(c.overlap_seconds * static_cast<double>(c.sample_rate), &requested))
        return refuse(FA_INVALID_ARGUMENT, "tdt_plan: the overlap is not finite, negative, or does not fit");
    Geometry r{};
    layout(c.frame_samples, c.mel_hop, c.max_model_samples, requested, c.mel_chunk_context != 0, c.warmup_prefix_frames, &r);
    if (!(r.chunk > r.frame * kMinOverlapFrames)) return refuse(FA_INVALID_ARGUMENT, "tdt_plan: a chunk of %lld samples does not exceed the six-frame overlap", (long long)r.chunk);
    if (r.chunk + r.mel_context > r.max_model || r.warmup_prefix >= r.chunk) return refuse(FA_INVALID_ARGUMENT, "tdt_plan: a window does not fit a row of max_model_samples");
    const double rate = static_cast<double>(c.sample_rate), frame = static_cast<double>(c.frame_samples);
    r.silence_radius = static_cast<int32_t>(std::max<int64_t>(1, static_cast<int64_t>((4.0 * rate) / frame)));        // :195
    r.valley_radius = static_cast<int32_t>(std::max<int64_t>(1, static_cast<int64_t>((0.5 * rate) / frame)));         // :196
    r.lookahead = static_cast<int64_t>(0.5 * rate);                                                                  // :351
    r.stable_quiet = static_cast<int64_t>(0.2 * rate);                                                               // :352
    r.probe_window = std::max<int64_t>(1, c.sample_rate / 50);                                                       // :353
    if (r.silence_radius > kMaxRadius || r.valley_radius > kMaxRadius) return refuse(FA_INVALID_ARGUMENT, "tdt_plan: a search radius above %d frames", kMaxRadius);
    if ((r.lookahead + r.probe_window - 1) / r.probe_window > kWave) return refuse(FA_INVALID_ARGUMENT, "tdt_plan: a look-ahead of more than %d windows", kWave);
    r.end_aligned = c.end_aligned ? 1 : 0;
    r.can_warmup = r.warmup_prefix > 0 ? 1 : 0;
    r.aligned = (c.silence_aligned || r.can_warmup) ? 1 : 0;                                                          // :169
    *g = r;
    return Verdict{};
}

// The checks every entry makes on its recordings.
inline Verdict check_offsets(const char *who, const int64_t *audio_offsets, const int32_t batch, const int64_t frame) {
    if (batch < 0) return refuse(FA_INVALID_ARGUMENT, "%s: batch is negative", who);
    if (batch == 0) return Verdict{};
    if (!audio_offsets) return refuse(FA_INVALID_ARGUMENT, "%s: audio_offsets is required", who);
    if (audio_offsets[0] < 0) return refuse(FA_INVALID_ARGUMENT, "%s: audio_offsets starts below 0", who);
    for (int32_t b = 0; b < batch; ++b) {
        if (audio_offsets[b + 1] < audio_offsets[b]) return refuse(FA_INVALID_ARGUMENT, "%s: audio_offsets descends at recording %d", who, b);
        if ((audio_offsets[b + 1] - audio_offsets[b]) / frame >= INT32_MAX - 1) return refuse(FA_INDEX_OVERFLOW, "%s: recording %d has 2^31 - 2 frames or more", who, b);
    }
    return Verdict{};
}

// A recording as the kernels see it; the offsets count from the arrays the kernels are given.
struct Recording {
    int64_t audio0, n;
    int64_t table0;                          // first entry of its boundary table
    int64_t sums0;                           // first of its n / F frame sums
    int64_t tile0;                           // first workgroup of the energy kernel
    int64_t starts0;                         // first slot of its listed starts
    int64_t listed;                          // listed_starts
    int64_t bound;                           // window_count_bound
};

struct Plan {
    std::vector<Recording> rec;
    int64_t table = 0, sums = 0, tiles = 0, starts = 0, bound = 0;
};

// device: the samples are addressed from the caller's array; otherwise from audio_offsets[0], where the upload starts
inline Verdict lay_out(const char *who, const Geometry &g, const int64_t *audio_offsets, const int32_t batch, const bool device, Plan *p) {
    p->rec.assign(static_cast<size_t>(batch), Recording{});
    for (int32_t b = 0; b < batch; ++b) {
        Recording &r = p->rec[static_cast<size_t>(b)];
        r.audio0 = audio_offsets[b] - (device ? 0 : audio_offsets[0]);
        r.n = audio_offsets[b + 1] - audio_offsets[b];
        r.table0 = p->table; r.sums0 = p->sums; r.tile0 = p->tiles; r.starts0 = p->starts;
        r.listed = listed_starts(g, r.n);
        r.bound = window_count_bound(g, r.n);
        const int64_t entries = table_entries(g.frame, r.n);
        p->table += entries;
        p->sums += r.n / g.frame;
        p->tiles += (entries + kEnergyBlock - 1) / kEnergyBlock;
        p->starts += r.listed;
        p->bound += r.bound;
    }
    if (p->bound > INT32_MAX || p->tiles > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "%s: more than INT32_MAX windows or workgroups in the call", who);
    return Verdict{};
}

inline Verdict plan_windows(const fa_tdt_window_config &c, const void *audio, const int64_t *audio_offsets, const int32_t batch, const void *windows, const int64_t capacity,
                            const int64_t *window_range, const bool device, Geometry *g, Plan *p) {
    const Verdict v = derive(c, g);
    if (v.status != FA_SUCCESS) return v;
    if (capacity < 0 || (capacity > 0 && !windows)) return refuse(FA_INVALID_ARGUMENT, "tdt_plan_windows: capacity is negative, or windows is NULL");
    const Verdict o = check_offsets("tdt_plan_windows", audio_offsets, batch, g->frame);
    if (o.status != FA_SUCCESS) return o;
    if (batch > 0 && !window_range) return refuse(FA_INVALID_ARGUMENT, "tdt_plan_windows: window_range is required");
    if (batch > 0 && audio_offsets[batch] > audio_offsets[0] && !audio) return refuse(FA_INVALID_ARGUMENT, "tdt_plan_windows: audio is NULL");
    return lay_out("tdt_plan_windows", *g, audio_offsets, batch, device, p);
}

struct PlanArgs {
    const float *audio;
    const Recording *rec;                    // [batch]
    int32_t batch;
    int32_t tiles;
    Geometry g;
    float *table;                            // [plan.table]: mean squares
    float *sums;                             // [plan.sums]: the frame sums from offset 0 (nullptr: not wanted)
    int32_t *bad;                            // [batch]: 1 where a table sum is not finite; zeroed before the launch
    int64_t *speech_end;                     // [batch]
    int64_t *starts;                         // [plan.starts]: start << 1 | useWarmupPrefix (aligned starts only)
    int32_t *counts;                         // [batch]: windows of the recording; scan_totals turns them into offsets
    int32_t *counts_kept;                    // [batch]: the same, left as counts
    int32_t *total;                          // [1]
    fa_tdt_window *out;                      // [capacity]
    int32_t *audio_frames, *t0, *is_last, *global_offset, *emit_after;   // [capacity] each, nullable
    int64_t capacity;
};

#if defined(__HIPCC__)
// tp_energy, tp_speech_end, tp_chain (aligned starts), tp_count, scan_totals and tp_write, in stream order
void launch_plan(hipStream_t stream, const PlanArgs &a);
#endif

// ---- the rows (row_pack_launch.h: a window is a row of a rows::Group)
inline Verdict plan_pack(const fa_tdt_window_config &c, const void *audio, const int64_t *audio_offsets, const int32_t batch, const fa_tdt_window *windows,
                         const int64_t n_windows, const void *rows, const int64_t row_capacity, Geometry *g) {
    const Verdict v = derive(c, g);
    if (v.status != FA_SUCCESS) return v;
    if (n_windows < 0 || row_capacity < 0) return refuse(FA_INVALID_ARGUMENT, "tdt_pack_windows: a size is negative");
    const Verdict o = check_offsets("tdt_pack_windows", audio_offsets, batch, g->frame);
    if (o.status != FA_SUCCESS) return o;
    if (n_windows > 0 && !windows) return refuse(FA_INVALID_ARGUMENT, "tdt_pack_windows: windows is NULL");
    if (n_windows > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "tdt_pack_windows: more than INT32_MAX windows");
    for (int64_t i = 0; i < n_windows; ++i) {
        const fa_tdt_window &w = windows[i];
        if (w.recording < 0 || w.recording >= batch) return refuse(FA_INVALID_ARGUMENT, "tdt_pack_windows: window %lld names recording %d", (long long)i, w.recording);
        const int64_t n = audio_offsets[w.recording + 1] - audio_offsets[w.recording];
        if (w.context_start < 0 || w.length < 0 || w.length > g->max_model || w.context_start > n || w.length > n - w.context_start)
            return refuse(FA_INVALID_ARGUMENT, "tdt_pack_windows: window %lld lies outside its recording or is longer than a row", (long long)i);
    }
    if (n_windows > 0 && !rows) return refuse(FA_INVALID_ARGUMENT, "tdt_pack_windows: rows is NULL");
    if (n_windows > 0 && !audio && std::any_of(windows, windows + n_windows, [](const fa_tdt_window &w) { return w.length > 0; }))
        return refuse(FA_INVALID_ARGUMENT, "tdt_pack_windows: audio is NULL");
    if (n_windows > row_capacity) return refuse(FA_OUTPUT_TOO_SMALL, "tdt_pack_windows: output holds %lld of %lld rows", (long long)row_capacity, (long long)n_windows);
    return Verdict{};
}

#if defined(__HIPCC__)
// rows / lengths: the group's first row.  wide: 16-byte stores (the rows are 16-byte aligned)
void launch_pack(hipStream_t stream, const float *audio, const rows::Group &g, int64_t row_samples, float *rows, int32_t *lengths, bool wide);
#endif

// ---- the gate
struct Span {
    int64_t audio0;                          // from_sample in the array the kernel is given
    int64_t frames;                          // whole frames below to_sample
    int32_t recording, pad;
};

struct GatePlan {
    Plan base;
    std::vector<Span> spans;
};

inline Verdict plan_gate(const fa_tdt_window_config &c, const void *audio, const int64_t *audio_offsets, const int32_t batch, const fa_tdt_span *spans, const int64_t n_spans,
                         const bool device, Geometry *g, GatePlan *p) {
    const Verdict v = derive(c, g);
    if (v.status != FA_SUCCESS) return v;
    if (n_spans < 0) return refuse(FA_INVALID_ARGUMENT, "tdt_speech_gate: n_spans is negative");
    const Verdict o = check_offsets("tdt_speech_gate", audio_offsets, batch, g->frame);
    if (o.status != FA_SUCCESS) return o;
    if (n_spans > 0 && !spans) return refuse(FA_INVALID_ARGUMENT, "tdt_speech_gate: spans is NULL");
    if (n_spans > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "tdt_speech_gate: more than INT32_MAX spans");
    if (batch > 0 && audio_offsets[batch] > audio_offsets[0] && !audio) return refuse(FA_INVALID_ARGUMENT, "tdt_speech_gate: audio is NULL");
    const Verdict l = lay_out("tdt_speech_gate", *g, audio_offsets, batch, device, &p->base);
    if (l.status != FA_SUCCESS) return l;
    p->spans.assign(static_cast<size_t>(n_spans), Span{});
    for (int64_t i = 0; i < n_spans; ++i) {
        const fa_tdt_span &s = spans[i];
        if (s.recording < 0 || s.recording >= batch) return refuse(FA_INVALID_ARGUMENT, "tdt_speech_gate: span %lld names recording %d", (long long)i, s.recording);
        const Recording &r = p->base.rec[static_cast<size_t>(s.recording)];
        if (s.from_sample < 0 || s.to_sample > r.n) return refuse(FA_INVALID_ARGUMENT, "tdt_speech_gate: span %lld leaves its recording", (long long)i);
        Span &d = p->spans[static_cast<size_t>(i)];
        d.audio0 = r.audio0 + s.from_sample;
        d.frames = s.to_sample > s.from_sample ? (s.to_sample - s.from_sample) / g->frame : 0;
        d.recording = s.recording;
    }
    return Verdict{};
}

struct GateArgs {
    PlanArgs plan;                           // the energy kernel's operands: table, sums, bad
    float *thresholds;                       // [batch]
    const float *override_thresholds;        // [batch] or nullptr
    const Span *spans;
    int64_t *span_frames;                    // [n_spans]
    int32_t n_spans;
};

#if defined(__HIPCC__)
// tp_energy, tp_threshold and tp_spans, in stream order
void launch_gate(hipStream_t stream, const GateArgs &a);
#endif

}  // namespace tdt_plan
}  // namespace fa
