// tdt_merge_launch.h — the host plan of the TDT seam merge (kernel: tdt_merge.hip, entries: tdt_merge_host.hip, the fold itself:
// tdt_merge_core.h): the argument pass, the recordings' records, the wave slots and the layout of a slot's workspace, and the
// kernel's operands.  Plain C++ without a HIP call, shared with tests/cpu/tdt_merge_emul.cpp.  Internal; not part of the C ABI.
//
// One wavefront folds one recording; a grid of `slots` wavefronts strides over the recordings.  A slot owns one piece of workspace:
// the staging area of a seam (as many tokens as the largest output slice) and the scratch of a seam whose overlap sides do not fit
// LDS (left side up to the largest slice, right side up to max_out) — sized from the arguments alone, because the windows' counts are
// on the device.  The bit table of that scratch is the large part (largest slice x max_out bits), so the number of slots shrinks
// until the workspace is below kWorkspaceBudget, but not below kMinSlots.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <vector>

#include "../../include/fluidaudio_hip.h"
#include "fa_verdict.h"
#include "tdt_merge_core.h"

namespace fa {
namespace tdtmerge {

constexpr int kWave = 64;
constexpr int32_t kMaxSlots = 1024, kMinSlots = 32;
constexpr int64_t kWorkspaceBudget = int64_t{1} << 30;

struct Rec {
    int64_t w_lo, w_hi;      // its windows, counted from the first window of the call
    int64_t out_off, cap;    // its output slice, counted from the first token of the call's output
};

struct Args {                // the kernel's operands; every array starts at the call's first window / first output token
    Stream win;              // [windows][max_out] (read only)
    const int32_t *counts;   // [windows]
    int32_t max_out;
    const Rec *recs;
    int32_t n_recs;
    Tables tb;
    Times tm;
    Stream out;
    int32_t *runmax;         // [output tokens]
    unsigned char *ws;       // [slots][slot_bytes]
    int64_t slot_bytes, big_l, big_r;
    int32_t small_side;      // <= kLdsSide
    int32_t *routes;         // [windows]
    int32_t *out_counts, *statuses;   // [n_recs]
};

constexpr int64_t slot_bytes_of(const int64_t big_l, const int64_t big_r) { return 16 * big_l + scratch_bytes(big_l, big_r); }
// a slot's piece: the staging arrays, then the scratch
FA_TM_HD inline void slot_views(unsigned char *p, const int64_t big_l, const int64_t big_r, Stream &stage, Scratch &big) {
    stage.tok = reinterpret_cast<int32_t *>(p);
    stage.time = stage.tok + big_l;
    stage.dur = stage.time + big_l;
    stage.conf = reinterpret_cast<float *>(stage.dur + big_l);
    big = carve(p + 16 * big_l, big_l, big_r);
}

inline fa_tdt_merge_config config_or_default(const fa_tdt_merge_config *cfg) {
    if (cfg) return *cfg;
    return fa_tdt_merge_config{static_cast<double>(1280) / static_cast<double>(16000), 2.0};   // ASRConstants.secondsPerEncoderFrame, overlapSeconds
}

// The argument pass: nothing is written, no device is touched.
inline Verdict check(const fa_tdt_merge_config &c, const void *tok, const void *time, const void *dur, const void *conf, const void *count, const int32_t max_out,
                     const int64_t *window_range, const int64_t n, const int32_t vocab, const void *out_tok, const void *out_time, const void *out_dur,
                     const void *out_conf, const int64_t *out_range, const void *out_counts, const void *statuses) {
    if (n < 0 || max_out < 0 || vocab < 0) return refuse(FA_INVALID_ARGUMENT, "a negative size");
    if (!(c.frame_seconds > 0.0) || !std::isfinite(c.frame_seconds) || !(c.overlap_seconds >= 0.0) || !std::isfinite(c.overlap_seconds))
        return refuse(FA_INVALID_ARGUMENT, "the frame must be positive and the overlap non-negative, both finite");
    if (n == 0) return Verdict{};
    if (n >= INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "2^31 - 1 recordings or more");
    if (!window_range || !out_range || !out_counts || !statuses) return refuse(FA_INVALID_ARGUMENT, "the ranges, out_counts and statuses are required");
    if (window_range[0] < 0 || out_range[0] < 0) return refuse(FA_INVALID_ARGUMENT, "a range starts below 0");
    for (int64_t r = 0; r < n; ++r) {
        if (window_range[r + 1] < window_range[r] || out_range[r + 1] < out_range[r]) return refuse(FA_INVALID_ARGUMENT, "the ranges do not ascend");
        if (out_range[r + 1] - out_range[r] > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "an output slice is longer than INT32_MAX");
    }
    const int64_t windows = window_range[n] - window_range[0];
    if (windows > 0 && !count) return refuse(FA_INVALID_ARGUMENT, "the windows' counts are required");
    if (windows > 0 && max_out > 0 && (!tok || !time || !dur || !conf)) return refuse(FA_INVALID_ARGUMENT, "the windows' arrays are required");
    if (window_range[n] > INT64_MAX / std::max(max_out, 1)) return refuse(FA_INDEX_OVERFLOW, "the windows' arrays are beyond int64");
    if (out_range[n] > out_range[0] && (!out_tok || !out_time || !out_dur || !out_conf)) return refuse(FA_INVALID_ARGUMENT, "the output arrays are required");
    return Verdict{};
}

struct Plan {
    std::vector<Rec> recs;
    int64_t windows = 0, out_tokens = 0;
    int64_t big_l = 1, big_r = 1, slot_bytes = 0;
    int32_t slots = 0;
};

inline void make_plan(const int64_t *window_range, const int64_t *out_range, const int64_t n, const int32_t max_out, Plan &plan) {
    plan.recs.resize(static_cast<size_t>(n));
    plan.big_l = 1;
    for (int64_t r = 0; r < n; ++r) {
        plan.recs[r] = Rec{window_range[r] - window_range[0], window_range[r + 1] - window_range[0], out_range[r] - out_range[0], out_range[r + 1] - out_range[r]};
        plan.big_l = std::max(plan.big_l, plan.recs[r].cap);
    }
    plan.windows = window_range[n] - window_range[0];
    plan.out_tokens = out_range[n] - out_range[0];
    plan.big_r = std::max<int64_t>(max_out, 1);
    plan.slot_bytes = slot_bytes_of(plan.big_l, plan.big_r);
    int64_t slots = std::min<int64_t>(n, kMaxSlots);
    while (slots > kMinSlots && slots * plan.slot_bytes > kWorkspaceBudget) slots = (slots + 1) / 2;
    plan.slots = static_cast<int32_t>(slots);
}

// the LDS limit a call runs with: kLdsSide, or what FA_TDT_MERGE_LDS_SIDE (tests) lowers it to
inline int32_t small_side_of(const char *sw) {
    if (!sw) return kLdsSide;
    const long v = std::atol(sw);
    return static_cast<int32_t>(std::min<long>(kLdsSide, std::max<long>(0, v)));
}

}  // namespace tdtmerge
}  // namespace fa
