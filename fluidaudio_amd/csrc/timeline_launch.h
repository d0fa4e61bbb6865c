// timeline_launch.h — what the timeline's host code (timeline_host.hip: staging, the three synchronisations of a call, the C ABI) and its
// kernel unit (timeline.hip) share: the recordings' records, the kernels' operands, the argument pass and the plan of a call (offsets,
// tiles, workgroups) and the launchers.  The argument pass and the plan are plain C++ without a HIP call and without a context, walked
// on the host by tests/cpu/timeline_plan.cpp; a refusal comes back as a verdict: the status and the text timeline_host.hip hands to the
// context.  Only the launchers' declarations at the end are for hipcc alone.  Internal; not part of the C ABI.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#include "fa_verdict.h"

namespace fa {
namespace timeline {

constexpr int kThreads = 256;       // fa::scan::kThreads: the kernels call block_exclusive
constexpr int kPer = 8;             // frames per thread of the state scan
constexpr int kTile = kThreads * kPer;

struct TlRec { int64_t fin_off, tent_off; int32_t nf, nt; };   // frame offsets into the two prediction arrays; frames of this recording

struct TlArgs {
    const float *fin, *tent;
    const TlRec *rec;          // [B]
    uint8_t *tile;             // [Q][max_tiles]: the composed map of a tile, then (tl_tile_state) the state at its start
    int32_t *bsum;             // [Q * max_tiles] onsets of a tile, then their exclusive offsets
    int32_t S, max_tiles;
    float onset, offset;
};

struct TlRun { int32_t on, off; float sum; };   // frames [on, off) speaking; off == frames of the recording: still speaking at the end

struct WalkArgs {
    const TlRec *rec;
    const int32_t *boff;       // as tl_run_walk
    const TlRun *runs;
    int32_t *count;            // [Q] segments of each (recording, speaker)
    const int32_t *seg_off;    // [Q] exclusive offsets of count (fill pass)
    fa_diarizer_segment *out;  // fill pass: capacity records
    int64_t capacity, Q;
    int32_t S, max_tiles, pad_on, pad_off, min_on, min_off, complete;
};

// What is refused before any output but *count is touched.
inline Verdict check_config(const fa_timeline_config &cfg, const int32_t B, const int64_t capacity, const int64_t *fin_frames) {
    if (B < 0 || capacity < 0 || cfg.speakers < 1 || (B > 0 && !fin_frames) || cfg.onset_pad_frames < 0 || cfg.offset_pad_frames < 0 ||
        cfg.min_frames_on < 0 || cfg.min_frames_off < 0)
        return refuse(FA_INVALID_ARGUMENT, "timeline: bad arguments");
    if (cfg.activity_type != FA_ACTIVITY_SIGMOIDS) return refuse(FA_INVALID_ARGUMENT, "timeline: only the sigmoid activity type is supported");
    return Verdict{};
}

struct Plan {
    std::vector<TlRec> rec;    // [B]
    int64_t fsum = 0, tsum = 0;   // frames of the two prediction arrays
    int64_t Q = 0;             // (recording, speaker) pairs
    int32_t max_tiles = 1;     // tiles of the longest recording, at least one
    int64_t blocks = 0;        // workgroups of tl_tiles: Q * max_tiles
};

// The plan of a call that passed check_config, B >= 1.  Recording by recording a negative count is refused before a sum of 2^31 - 1
// frames or more; then missing predictions, then the workgroup count.
inline Verdict make_plan(const int32_t S, const int64_t *fin_frames, const int64_t *tent_frames, const int32_t B, const void *finalized, const void *tentative,
                         Plan &plan) {
    plan = Plan{};
    plan.rec.resize(static_cast<size_t>(B));
    int64_t max_len = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t nf = fin_frames[b], nt = tent_frames ? tent_frames[b] : 0;
        if (nf < 0 || nt < 0) return refuse(FA_INVALID_ARGUMENT, "timeline: recording %d has a negative frame count", b);
        if (nf + nt >= INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "timeline: recording %d has 2^31 frames or more", b);
        plan.rec[b] = TlRec{plan.fsum, plan.tsum, static_cast<int32_t>(nf), static_cast<int32_t>(nt)};
        plan.fsum += nf;
        plan.tsum += nt;
        max_len = std::max(max_len, nf + nt);
    }
    if ((plan.fsum > 0 && !finalized) || (plan.tsum > 0 && !tentative)) return refuse(FA_INVALID_ARGUMENT, "timeline: predictions are required");
    plan.Q = static_cast<int64_t>(B) * S;
    plan.max_tiles = static_cast<int32_t>(std::max<int64_t>(1, (max_len + kTile - 1) / kTile));
    plan.blocks = plan.Q * plan.max_tiles;
    if (plan.blocks >= INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "timeline: %lld tiles", (long long)plan.blocks);
    return Verdict{};
}

#if defined(__HIPCC__)
// timeline.hip.  Launch errors surface through hipGetLastError().
void launch_tiles(hipStream_t stream, const TlArgs &a, int64_t blocks, int mode, int32_t *starts);   // mode 0, 1, 2: tl_tiles
void launch_tile_state(hipStream_t stream, const TlArgs &a, int64_t Q);
void launch_scan_totals(hipStream_t stream, int32_t *bsum, int64_t nb, int32_t *total);              // block_scan.h's, one workgroup
void launch_run_walk(hipStream_t stream, const TlArgs &a, const int32_t *starts, int64_t Q, int32_t n_runs, TlRun *runs);
void launch_segment_walk(hipStream_t stream, const WalkArgs &a, int fill);
#endif

}  // namespace timeline
}  // namespace fa
