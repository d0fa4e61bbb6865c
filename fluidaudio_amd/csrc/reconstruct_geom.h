// reconstruct_geom.h — the arithmetic of the reconstruction that is not a kernel, in plain C++ without a HIP header so that
// tests/cpu/reconstruct_geom.cpp walks it on the CPU: the powerset table and the chunk-frame -> global-frame map (FA_RECON_HD: the
// kernels of reconstruct.hip call them too), the frame-duration rule, and the FramePlan that reconstruct_host.hip stages: chunk starts
// (OfflineReconstruction.swift:498-507), the global frame count (:37-47), each chunk's first / last global frame, the sanitised hard
// labels (:81-83) and the zero-vote override table (:284-286).  fp64 without FMA: the units that include it are built with
// -ffp-contract=off.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define FA_RECON_HD __host__ __device__ inline
#else
#define FA_RECON_HD inline
#endif

namespace fa {
namespace reconstruct {

// powerset (OfflineSegmentationProcessor.swift:15-24): [] [0] [1] [2] [0,1] [0,2] [1,2] [0,1,2] as speaker bit masks, one nibble per class
FA_RECON_HD unsigned powerset_mask(int cls) { return (0x76534210u >> (4 * cls)) & 0xFu; }

// chunk frame -> global frame (:69-77): frameStart = offset + Double(f) * fd (two roundings), rounded half away from zero, clamped
FA_RECON_HD int global_frame(double offset, int f, double fd, int T) {
    const double fs = offset + static_cast<double>(f) * fd;   // built with -ffp-contract=off: no FMA
    const double r = round(fs / fd);
    if (!(r > 0.0)) return 0;
    if (r >= static_cast<double>(T)) return T - 1;
    return static_cast<int>(r);
}

// OfflineSegmentationProcessor.swift:286; F > 0
inline double frame_duration(double configured, double window_duration, int32_t F) { return configured > 0 ? configured : window_duration / F; }

enum class PlanError : int32_t {
    kNone = 0,
    kChunkStart,   // chunk `index` starts at a non-finite time
    kFrames,       // `frames` global frames times smax slots do not fit an int32
    kOverride,     // override `index` is out of range; T, Kc, maxc and smax are valid (the caller reports them)
};

struct FramePlan {
    PlanError error = PlanError::kNone;
    int64_t index = -1;
    double frames = 0.0;             // ceil(max chunk end / fd) before its clamp
    std::vector<double> start;       // [C]
    bool sorted = true;              // start is non-decreasing
    int32_t T = 0, Kc = 0, maxc = 0, smax = 0;   // global frames, max(K, 1), min(Kc, S), max(maxc, 1) slots per frame
    std::vector<int32_t> first_g, last_g;        // [C] global frame of chunk frame 0 / F - 1
    std::vector<int32_t> hard;       // [C][S] cluster of each local speaker, -1 for anything outside [0, Kc)
    std::vector<int32_t> ovr;        // [T] override cluster or -1; empty without overrides
};

// C, F > 0, fd > 0 and finite.  hard: [C][S] or nullptr (no speaker has a cluster); overrides: n_overrides x (lo, hi, cluster), applied in order.
inline FramePlan frame_plan(int64_t C, int32_t F, int32_t S, int32_t K, double fd, double window_duration, const double *offsets, int64_t n_offsets,
                            const int32_t *hard, const int64_t *overrides, int64_t n_overrides) {
    FramePlan p;
    auto fail = [&](PlanError e, int64_t index) -> FramePlan & { p.error = e; p.index = index; return p; };
    p.start.resize(static_cast<size_t>(C));
    double max_time = 0.0;
    for (int64_t c = 0; c < C; ++c) {
        p.start[c] = c < n_offsets ? offsets[c] : static_cast<double>(c) * window_duration;
        if (!std::isfinite(p.start[c])) return fail(PlanError::kChunkStart, c);
        if (c > 0 && p.start[c] < p.start[c - 1]) p.sorted = false;
        const double end = p.start[c] + static_cast<double>(F) * fd;
        if (end > max_time) max_time = end;
    }
    p.frames = std::ceil(max_time / fd);
    p.Kc = std::max(K, 1);
    p.maxc = std::min(p.Kc, S);
    p.smax = std::max(p.maxc, 1);
    if (!(p.frames < static_cast<double>(INT32_MAX) / p.smax)) return fail(PlanError::kFrames, -1);
    p.T = std::max(1, static_cast<int32_t>(p.frames));
    p.first_g.resize(static_cast<size_t>(C));
    p.last_g.resize(static_cast<size_t>(C));
    for (int64_t c = 0; c < C; ++c) { p.first_g[c] = global_frame(p.start[c], 0, fd, p.T); p.last_g[c] = global_frame(p.start[c], F - 1, fd, p.T); }
    p.hard.assign(static_cast<size_t>(C * S), -1);
    if (hard) for (int64_t i = 0; i < C * S; ++i) p.hard[i] = hard[i] >= 0 && hard[i] < p.Kc ? hard[i] : -1;
    if (n_overrides > 0) {
        p.ovr.assign(static_cast<size_t>(p.T), -1);
        for (int64_t i = 0; i < n_overrides; ++i) {
            const int64_t lo = overrides[3 * i], hi = overrides[3 * i + 1], k = overrides[3 * i + 2];
            if (lo < 0 || hi < lo || hi > p.T || k < 0 || k >= p.Kc) return fail(PlanError::kOverride, i);
            for (int64_t g = lo; g < hi; ++g) p.ovr[g] = static_cast<int32_t>(k);
        }
    }
    return p;
}

}  // namespace reconstruct
}  // namespace fa
