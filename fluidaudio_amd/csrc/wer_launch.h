// wer_launch.h — the host plan of the edit-distance kernel (kernel: wer.hip, entries: wer_host.hip): the argument pass over the ranges,
// each pair's class and panel count, the job list by class, the layout of the boundary workspace, where in the wavefront a pair's
// answer ends up, and the kernel's operands.  Plain C++ without a HIP call, shared by the two units and by tests/cpu/wer_emul.cpp,
// which walks the kernel's schedule on the host; only the launcher's declaration at the end is for hipcc alone.  Internal; not part
// of the C ABI.
//
// One wavefront walks one pair.  Lane l owns a strip of C = 1, 2, 4, 8 or 16 consecutive reference columns (class 0 ... 4, the smallest
// that covers the reference in one pass: up to 64 C columns); a reference of more than 1024 columns is walked panel by panel, 1024
// columns each at C = 16.  Panel p's last column (one cell per hypothesis row) goes through the workspace to panel p + 1: two buffers
// per multi-panel pair, panel p writes buffer p & 1 and reads buffer (p - 1) & 1, each three planes (dp, sub, del) of m entries, row i
// at [i - 1].  Row 0 of a boundary is never stored: cell(0, j) = (j, 0, 0).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/fluidaudio_hip.h"

namespace fa {
namespace wer {

constexpr int kWave = 64;
constexpr int kClasses = 5;
constexpr int kMaxStrip = 16;
constexpr int kPanelCols = kWave * kMaxStrip;   // 1024
constexpr int kWavesPerGroup = 4;               // pairs of one workgroup
constexpr int kPlanes = 3;                      // dp, sub, del

constexpr int strip_of(const int cls) { return 1 << cls; }
inline int class_of(const int32_t n) {
    int c = 0;
    while (c < kClasses - 1 && n > kWave * strip_of(c)) ++c;
    return c;
}
constexpr int32_t panels_of(const int32_t n) { return n <= kPanelCols ? 1 : (n - 1) / kPanelCols + 1; }

// (constexpr: the kernel calls them too)
// cell(m, n) is slot last_slot of lane last_lane's strip in the last panel, once that lane has done row m
constexpr int last_lane(const int32_t n, const int strip) { return ((n - 1) % (kWave * strip)) / strip; }
constexpr int last_slot(const int32_t n, const int strip) { return (n - 1) % strip; }
// steps of a panel: at step s lane l works on row s - l (from 0); only the lanes up to the answer's matter in the last panel
constexpr uint32_t steps_of(const int32_t m, const int32_t n, const int strip, const bool last_panel) {
    return static_cast<uint32_t>(m) + static_cast<uint32_t>(last_panel ? last_lane(n, strip) : kWave - 1);
}

constexpr int64_t boundary_ints(const int32_t m, const int32_t panels) { return panels > 1 ? int64_t{2} * kPlanes * m : 0; }
constexpr int64_t boundary_at(const int32_t m, const int buffer, const int plane) { return (static_cast<int64_t>(buffer) * kPlanes + plane) * m; }

struct Job {
    int64_t hyp_off, ref_off;   // first symbol of each side in the arrays the kernel is given
    int64_t ws_off;             // first int32 of its boundary buffers (multi-panel pairs)
    int32_t m, n, panels;       // rows (hypothesis), columns (reference); m, n >= 1
    int32_t pair;               // index in the caller's batch
};

struct Plan {
    std::vector<Job> jobs;      // class after class, each class in input order
    int32_t n_class[kClasses] = {0, 0, 0, 0, 0};
    int64_t ws_ints = 0;
};

struct Verdict {
    fa_status status = FA_SUCCESS;
    int64_t pair = -1;          // the pair the status is about
    const char *what = "";
};

// The argument pass (nothing is written): the ranges ascend from a non-negative start, no side is longer than INT32_MAX, and a side
// that has symbols has an array.  n_pairs >= 1.
inline Verdict check_ranges(const int32_t *hyp, const int64_t *hyp_range, const int32_t *ref, const int64_t *ref_range, const int64_t n_pairs) {
    if (hyp_range[0] < 0 || ref_range[0] < 0) return Verdict{FA_INVALID_ARGUMENT, 0, "a range starts below 0"};
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int64_t m = hyp_range[k + 1] - hyp_range[k], n = ref_range[k + 1] - ref_range[k];
        if (hyp_range[k + 1] < hyp_range[k] || ref_range[k + 1] < ref_range[k]) return Verdict{FA_INVALID_ARGUMENT, k, "the ranges do not ascend"};
        if (m > INT32_MAX || n > INT32_MAX) return Verdict{FA_INDEX_OVERFLOW, k, "a side is longer than INT32_MAX"};
    }
    if ((hyp_range[n_pairs] > hyp_range[0] && !hyp) || (ref_range[n_pairs] > ref_range[0] && !ref)) return Verdict{FA_INVALID_ARGUMENT, -1, "the symbol arrays are required"};
    return Verdict{};
}

// Every pair's lengths go to `out`; a pair with an empty side is answered here (:182-187), the others become jobs.  The kernel is given
// the arrays from symbol hyp_base / ref_base on.
inline void make_plan(const int64_t *hyp_range, const int64_t *ref_range, const int64_t n_pairs, const int64_t hyp_base, const int64_t ref_base,
                      fa_edit_counts *out, Plan &plan) {
    std::vector<Job> jobs;
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t m = static_cast<int32_t>(hyp_range[k + 1] - hyp_range[k]), n = static_cast<int32_t>(ref_range[k + 1] - ref_range[k]);
        if (m == 0) out[k] = fa_edit_counts{n, n, 0, 0, m, n};
        else if (n == 0) out[k] = fa_edit_counts{m, 0, m, 0, m, n};
        else {
            out[k] = fa_edit_counts{0, 0, 0, 0, m, n};
            jobs.push_back(Job{hyp_range[k] - hyp_base, ref_range[k] - ref_base, 0, m, n, panels_of(n), static_cast<int32_t>(k)});
            ++plan.n_class[class_of(n)];
        }
    }
    plan.jobs.reserve(jobs.size());
    plan.ws_ints = 0;
    for (int c = 0; c < kClasses; ++c)
        for (const Job &j : jobs)
            if (class_of(j.n) == c) {
                plan.jobs.push_back(j);
                plan.jobs.back().ws_off = plan.ws_ints;
                plan.ws_ints += boundary_ints(j.m, j.panels);
            }
}

struct WalkArgs {               // the kernel's operands
    const int32_t *hyp, *ref;
    const Job *jobs;
    int32_t n_jobs;
    int32_t *ws;       // boundary buffers
    int32_t *out;      // [n_jobs][4]: total, insertions, deletions, substitutions
};

#if defined(__HIPCC__)
void launch_walk(hipStream_t stream, const WalkArgs &a, int cls);   // wer.hip: the jobs of class cls, strip_of(cls) columns per lane
#endif

}  // namespace wer
}  // namespace fa
