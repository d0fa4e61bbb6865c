// embedding_geom.h — the host arithmetic of the embedding inputs (embedding_host.hip), in plain C++ without a HIP header so that
// tests/cpu/embedding_geom.cpp walks it on the CPU: what a config means (Geometry), which chunks become fbank windows
// (OfflineEmbeddingExtractor.swift:650-668), the samples and weight frames of a span (embedSpan, :243-297) and the slice check of
// fa_embedding_windows_dev.  All of it is the reference's fp64 host code; the units that include it are built with -ffp-contract=off.
// Every "start, length of a window" comes from window_slice, every rounded sample position from rounded_sample.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/fluidaudio_hip.h"

namespace fa {
namespace embedding {

constexpr int kMaxBatch = 32;   // modelBatchLimit (:162)

inline int32_t samples_per_window(const fa_embedding_config &cfg) {
    if (cfg.samples_per_window > 0) return cfg.samples_per_window;
    const double v = static_cast<double>(cfg.sample_rate) * cfg.window_duration;   // OfflineDiarizerTypes.swift:348-353
    return v >= 1.0 && v < static_cast<double>(INT32_MAX) ? static_cast<int32_t>(v) : 0;
}

inline bool config_ok(const fa_embedding_config *cfg) {
    return cfg && cfg->sample_rate > 0 && std::isfinite(cfg->window_duration) && cfg->weight_frames > 0 && samples_per_window(*cfg) > 0 &&
           std::isfinite(cfg->overlap_threshold) && !std::isnan(cfg->min_segment_duration) && std::isfinite(cfg->frame_duration);
}

// What every entry derives from a config that passed config_ok, and the chunk length F (0 where no chunk is involved: fd 0, min_frames 1).
struct Geometry {
    int32_t spw, W, B;     // samples per window, weight frames, clamp(batch_size, 1, kMaxBatch) (:162, :309)
    double fd;             // frame duration (:373-382)
    int32_t min_frames;    // clamp(ceil(min_segment_duration / fd), 1, Int32.max) (:384-390)
};
inline Geometry geometry(const fa_embedding_config &cfg, int32_t F) {
    Geometry g{};
    g.spw = samples_per_window(cfg);
    g.W = cfg.weight_frames;
    g.B = std::max(1, std::min(cfg.batch_size, kMaxBatch));
    g.fd = cfg.frame_duration > 0 ? cfg.frame_duration : (F > 0 ? cfg.window_duration / F : 0.0);
    const double mf = g.fd > 0 ? std::ceil(cfg.min_segment_duration / g.fd) : 1.0;
    g.min_frames = static_cast<int32_t>(std::max(1.0, std::min(mf, 2147483647.0)));
    return g;
}

// Int((seconds * rate).rounded()) before its clamp: rounded() is half away from zero (std::round)
inline double rounded_sample(double seconds, int32_t rate) { return std::round(seconds * static_cast<double>(rate)); }

// clamp(rounded_sample, 0, total)
inline int64_t sample_index(double seconds, int32_t rate, int64_t total) {
    const double r = rounded_sample(seconds, rate);
    if (!(r > 0.0)) return 0;
    if (r >= static_cast<double>(total)) return total;
    return static_cast<int64_t>(r);
}

// audio[start : min(start + spw, limit)]: the samples a window copies before its zeros; len <= 0: nothing to copy
struct Slice { int64_t start, len; };
inline Slice window_slice(int64_t start, int64_t limit, int32_t spw) { return Slice{start, std::min(limit - start, static_cast<int64_t>(spw))}; }

// fa_embedding_windows_dev takes the caller's starts: one inside [0, total] (total itself: a window of zeros)
inline bool slice_ok(int64_t start, int64_t total) { return start >= 0 && start <= total; }

// Planned chunks (:650-668), in chunk order.  A missing or non-finite offset is c * window_duration; a chunk whose window holds no audio
// (it starts at or past total_samples) is not planned.
struct Windows {
    std::vector<int32_t> chunk;
    std::vector<int64_t> start;
    std::vector<double> offset;
};
inline Windows plan_windows(const fa_embedding_config &cfg, const Geometry &g, int64_t C, const double *offsets, int64_t n_offsets, int64_t total_samples) {
    Windows w;
    for (int64_t c = 0; c < C; ++c) {
        double off = c < n_offsets ? offsets[c] : static_cast<double>(c) * cfg.window_duration;
        if (!std::isfinite(off)) off = static_cast<double>(c) * cfg.window_duration;
        const Slice s = window_slice(sample_index(off, cfg.sample_rate, total_samples), total_samples, g.spw);
        if (s.len <= 0) continue;
        w.chunk.push_back(static_cast<int32_t>(c));
        w.start.push_back(s.start);
        w.offset.push_back(off);
    }
    return w;
}

// embedSpan (:243-297): the samples [start, start + len) of the span [t0, t1] seconds and its all-active weight frames.  Past 9e18 the
// rounded positions are pinned to +-Int64.max / 2, so that end - start cannot overflow.  !ok (a non-finite bound, or no sample): all zero.
struct Span {
    int64_t start, len;
    int32_t active;
    bool ok;
};
inline Span span_geometry(double t0, double t1, int32_t rate, const Geometry &g, int64_t total_samples) {
    const double rs = rounded_sample(t0, rate), re = rounded_sample(t1, rate);
    const int64_t s = rs > 0 ? (rs < 9.0e18 ? static_cast<int64_t>(rs) : INT64_MAX / 2) : 0;
    const int64_t e = re < static_cast<double>(total_samples) ? (re > -9.0e18 ? static_cast<int64_t>(re) : -INT64_MAX / 2) : total_samples;
    const Slice sl = window_slice(s, e, g.spw);
    if (!(std::isfinite(t0) && std::isfinite(t1) && sl.len > 0)) return Span{0, 0, 0, false};
    const double frac = static_cast<double>(sl.len) / static_cast<double>(g.spw);
    const double r = std::round(frac * static_cast<double>(g.W));
    return Span{sl.start, sl.len, static_cast<int32_t>(std::max(1.0, std::min(static_cast<double>(g.W), r))), true};
}

}  // namespace embedding
}  // namespace fa
