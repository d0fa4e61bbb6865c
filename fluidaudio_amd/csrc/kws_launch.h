// kws_launch.h — what the CTC word spotter's host unit (kws_host.hip: staging, launches, synchronisations, the C ABI) and its kernel
// unit (kws.hip) share beyond the plan (kws_plan.h: the limits, a job, a candidate record, everything the host decides): the kernel's
// tiling constants, its operands and its one launcher.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"
#include "kws_plan.h"

namespace fa {
namespace kws {

constexpr int kWavesPerGroup = 4;   // jobs of one workgroup: consecutive in the job list, which is ordered by utterance
constexpr int kAhead = 8;           // frames whose emissions a wavefront has in flight ahead of the DP step that needs them
constexpr int kXcds = 8;            // workgroups with equal blockIdx % 8 share an L2

struct WalkArgs {
    const float *lp;                // matrix u at u * matrix_stride, row t at t * row_stride, `vocab` columns read
    int64_t row_stride, matrix_stride;
    int32_t vocab, blank;
    const int32_t *tokens;          // concatenated keywords
    const int64_t *kw_off;          // [keywords + 1]
    const float *kw_min;            // [keywords] thresholds (spotting)
    const Job *jobs;
    int32_t n_jobs, job_base;       // records carry job_base + the job's index in `jobs`
    int32_t constrained;            // 0: ctcWordSpotMultiple's candidates -> arena; 1: ctcWordSpotConstrained -> out[job_base + index]
    Record *arena;
    int64_t arena_cap;
    unsigned long long *cursor;     // records reserved so far, whether they fitted or not
    int32_t *status;                // [job_base + index]: candidates written, or -1 when a chunk did not fit
    Record *out;
};

// kws_walk<states_per_lane> (1, 2 or 4) on a.n_jobs jobs, none wider than max_tokens(states_per_lane).  Launch errors surface through
// hipGetLastError().
void launch_walk(hipStream_t stream, const WalkArgs &a, int states_per_lane);

}  // namespace kws
}  // namespace fa
