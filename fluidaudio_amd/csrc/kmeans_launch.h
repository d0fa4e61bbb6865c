// kmeans_launch.h — what the k-means fallback's host code (kmeans_host.hip: the lock-step Lloyd loop, the best-run choice, the C ABI)
// and its kernel unit (kmeans.hip) share beside the draws (kmeans_draws.h): the limits, the operands of a batch of runs and one
// launcher per kernel family.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"
#include "kmeans_draws.h"

namespace fa {
namespace kmeans {

constexpr int kThreads = 256;
constexpr int kChunk = 16;     // running distances per thread in the assignment kernel
constexpr int kMaxRuns = 64;   // runs per batch (active set is a 64-bit kernel argument)
constexpr int kAhead = 8;      // independent loads in flight per thread in the ordered centroid sums

struct LloydArgs {             // a batch of `runs` runs over the same n x d embeddings
    const double *xn, *xt;     // normalised embeddings [n][d] and their transpose [d][n]
    double *cen;               // [runs][k][d]
    int32_t *assign;           // [runs][n]
    int32_t *changed;          // [runs]
    int32_t *counts;           // [runs][k]
    int32_t *list;             // [runs][n] members, cluster after cluster in index order
    int32_t *done, *iters, *cursor;   // [runs] each
    int32_t *status;           // [2]; status[1]: a run needed more than kPicks re-seeds
    const int32_t *picks;      // [runs][kPicks]
    int64_t n;
    int d, k, runs;
};

// kmeans.hip.  Launch errors surface through hipGetLastError().
void launch_normalize(hipStream_t stream, const double *x, double *xn, double *xt, int64_t n, int d);
void launch_assign(hipStream_t stream, const LloydArgs &a);
void launch_members(hipStream_t stream, const LloydArgs &a);     // the counting pass, then the writing pass
void launch_update(hipStream_t stream, const LloydArgs &a);
void launch_step_end(hipStream_t stream, const LloydArgs &a, int it);
void launch_own_distance(hipStream_t stream, const LloydArgs &a, double *dist);   // [runs][n]

}  // namespace kmeans
}  // namespace fa
