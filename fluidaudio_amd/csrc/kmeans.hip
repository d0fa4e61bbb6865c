// kmeans.hip — the kernels of the speaker-count fallback of the offline diarizer on gfx950 (fp64, bit-identical to the CPU restatement;
// entries: kmeans_host.hip, operands: kmeans_launch.h, the host's draws: kmeans_draws.h).
//
// Replaces KMeansClustering.clusterWithCentroids / clusterWithCentroidsNInit (reference:
// Sources/FluidAudio/Diarizer/Offline/Clustering/KMeansClustering.swift:39-129) and SpeakerCountConstraints.resolve
// (SpeakerCountConstraints.swift:25-62), which VBxClustering.refineWithConstraints (VBxClustering.swift:685-733) calls when the
// number of clusters the VBx posteriors actually use falls outside the caller's [min, max] speakers: best of n_init = 10
// Lloyd runs (seeds 0..9, <= 100 iterations) over the unit-normalised 256-d training embeddings.
//
// Design.  The n_init runs are independent, so they are BATCHED: every kernel has a (work, run) grid and the host walks all
// runs in lock step — one stream synchronisation per Lloyd iteration for the whole batch instead of one per run (the
// reference runs them back to back).  Parity demands the reference's summation orders: distances are accumulated
// sequentially over the dimension, centroid sums sequentially over the embedding index (`sums[cluster][d] += e[d]` in index
// order, :187-193).  So
//   * assignment: one thread per embedding reads the TRANSPOSED embeddings xt[d][n] (coalesced) and carries 16 running
//     distances in registers; centroid values are wave-uniform, i.e. scalar loads.
//   * update: a stable compaction (one wave per cluster: ballot + prefix popcount) builds each cluster's member list in index
//     order, then one thread per (cluster, dimension) walks the list with 8 independent loads in flight and adds in order.
// The random draws (initial shuffle, re-seeding of empty clusters) happen on the host between iterations: they are the
// reference's LCG (SeededRNG, :212-223) pushed through the Swift standard library's `next(upperBound:)` (Lemire's method),
// `shuffle(using:)` and `randomElement(using:)`, restated in kmeans_draws.h because that library is the only specification
// of the draw sequence (third-party, unpinned).
#include <cfloat>

#include "kmeans_launch.h"

namespace {

using namespace fa::kmeans;

// normalizeEmbeddings (:131-142): norm = sqrt(sum of squares); rows with norm <= 1e-10 (or NaN) are kept as they are.
__global__ void km_normalize(const double *__restrict__ x, double *__restrict__ xn, double *__restrict__ xt, int64_t n, int d) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = x + i * d;
    double ss = 0.0;
    for (int k = 0; k < d; ++k) ss = __dadd_rn(ss, __dmul_rn(r[k], r[k]));
    const double norm = __dsqrt_rn(ss);
    const bool scale = norm > 1e-10;
    const double inv = scale ? __ddiv_rn(1.0, norm) : 1.0;
    for (int k = 0; k < d; ++k) {
        const double v = scale ? __dmul_rn(r[k], inv) : r[k];
        xn[i * d + k] = v;
        xt[static_cast<int64_t>(k) * n + i] = v;
    }
}

// assignToCentroids (:154-168): first strict minimum of the sequentially accumulated squared distances.
__global__ void __launch_bounds__(kThreads) km_assign(const double *__restrict__ xt, const double *__restrict__ cen, int32_t *__restrict__ assign,
                                                      int32_t *__restrict__ changed, int64_t n, int d, int k, const int32_t *__restrict__ done) {
    const int r = blockIdx.y;
    if (done[r]) return;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;
    const double *c_run = cen + static_cast<int64_t>(r) * k * d;
    double bd = DBL_MAX;
    int best = 0;
    for (int c0 = 0; c0 < k; c0 += kChunk) {
        const int kk = min(kChunk, k - c0);
        double acc[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) acc[j] = 0.0;
        for (int q = 0; q < d; ++q) {
            const double x = xt[static_cast<int64_t>(q) * n + ii];
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                if (j < kk) {
                    const double df = __dsub_rn(x, c_run[static_cast<int64_t>(c0 + j) * d + q]);
                    acc[j] = __dadd_rn(acc[j], __dmul_rn(df, df));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (j < kk && acc[j] < bd) { bd = acc[j]; best = c0 + j; }
    }
    bool diff = false;
    if (live) {
        int32_t *a = assign + static_cast<int64_t>(r) * n + i;
        diff = *a != best;
        *a = best;
    }
    if (__any(diff) && (threadIdx.x & 63) == 0) atomicOr(changed + r, 1);
}

// members of cluster c of run r, counted (pass 0) or written in index order at the cluster's offset (pass 1); one wave each
template <int PASS>
__global__ void __launch_bounds__(64) km_members(const int32_t *__restrict__ assign, const int32_t *__restrict__ changed, int32_t *__restrict__ counts,
                                                 int32_t *__restrict__ list, int64_t n, int k, const int32_t *__restrict__ done) {
    const int r = blockIdx.y, c = blockIdx.x, lane = threadIdx.x;
    if (done[r] || !changed[r]) return;
    const int32_t *a = assign + static_cast<int64_t>(r) * n;
    int64_t base = 0;
    if (PASS == 1) {
        int64_t part = 0;
        for (int j = lane; j < c; j += 64) part += counts[static_cast<int64_t>(r) * k + j];
        for (int s = 32; s; s >>= 1) part += __shfl_xor(part, s);
        base = part;
    }
    int64_t total = 0;
    constexpr int kRows = 8;   // 8 x 64 assignments requested before the first is looked at (one load per step made every step a memory round trip)
    for (int64_t i0 = 0; i0 < n; i0 += 64 * kRows) {
        int32_t av[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) { const int64_t i = i0 + 64 * u + lane; av[u] = i < n ? a[i] : -1; }
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
            const int64_t i = i0 + 64 * u + lane;
            const bool m = av[u] == c;
            const uint64_t mask = __ballot(m);
            if (PASS == 1 && m) list[static_cast<int64_t>(r) * n + base + total + __popcll(mask & ((1ull << lane) - 1))] = static_cast<int32_t>(i);
            total += __popcll(mask);
        }
    }
    if (PASS == 0 && lane == 0) counts[static_cast<int64_t>(r) * k + c] = static_cast<int32_t>(total);
}

// updateCentroids (:179-207) for the non-empty clusters: sums in embedding-index order, times 1 / count.
__global__ void __launch_bounds__(kThreads) km_update(const double *__restrict__ xn, const int32_t *__restrict__ changed, const int32_t *__restrict__ counts,
                                                      const int32_t *__restrict__ list, double *__restrict__ cen, int64_t n, int d, int k,
                                                      const int32_t *__restrict__ done) {
    const int r = blockIdx.y, c = blockIdx.x;
    if (done[r] || !changed[r]) return;
    const int32_t *cnts = counts + static_cast<int64_t>(r) * k;
    const int cnt = cnts[c];
    if (cnt == 0) return;                       // re-seeded by km_step_end from the run's pre-drawn random stream
    int64_t base = 0;
    for (int j = 0; j < c; ++j) base += cnts[j];
    const int32_t *mine = list + static_cast<int64_t>(r) * n + base;
    const double inv = __ddiv_rn(1.0, static_cast<double>(cnt));
    for (int q = threadIdx.x; q < d; q += blockDim.x) {
        double s = 0.0;
        int j = 0;
        for (; j + kAhead <= cnt; j += kAhead) {
            double v[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) v[u] = xn[static_cast<int64_t>(mine[j + u]) * d + q];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) s = __dadd_rn(s, v[u]);
        }
        for (; j < cnt; ++j) s = __dadd_rn(s, xn[static_cast<int64_t>(mine[j]) * d + q]);
        cen[(static_cast<int64_t>(r) * k + c) * d + q] = __dmul_rn(s, inv);
    }
}

// End of a Lloyd iteration for run r (one wavefront): convergence (newAssignments == assignments, :70-73) and the re-seeding of
// empty clusters in cluster order from the run's random stream (randomElement, :196-199).  The draws do not depend on the data
// — every one is below(n) on the same generator — so the host pre-draws the sequence (picks[r][0..kPicks)) and the device only
// keeps a cursor: no host synchronisation inside the iteration loop.  status[1] is raised if a run needs more than kPicks draws.
__global__ void __launch_bounds__(64) km_step_end(const int32_t *__restrict__ changed, const int32_t *__restrict__ counts, int32_t *__restrict__ done,
                                                  int32_t *__restrict__ iters, const int32_t *__restrict__ picks, int32_t *__restrict__ cursor,
                                                  const double *__restrict__ xn, double *__restrict__ cen, int32_t *__restrict__ status, int it, int d, int k) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (done[r]) return;
    if (lane == 0) iters[r] = it + 1;
    if (!changed[r]) { if (lane == 0) done[r] = 1; return; }
    int cur = cursor[r];
    for (int c = 0; c < k; ++c) {   // wave-uniform walk over the clusters, the row copy spread over the lanes
        if (counts[static_cast<int64_t>(r) * k + c] != 0) continue;
        if (cur >= kPicks) { if (lane == 0) status[1] = 1; break; }
        const int64_t pick = picks[static_cast<int64_t>(r) * kPicks + cur];
        ++cur;
        for (int q = lane; q < d; q += 64) cen[(static_cast<int64_t>(r) * k + c) * d + q] = xn[pick * d + q];
    }
    if (lane == 0) cursor[r] = cur;
}

// per-embedding squared distance to its own centroid (the terms of the inertia, :118-121)
__global__ void km_own_distance(const double *__restrict__ xt, const double *__restrict__ cen, const int32_t *__restrict__ assign,
                                double *__restrict__ dist, int64_t n, int d, int k) {
    const int r = blockIdx.y;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *c = cen + (static_cast<int64_t>(r) * k + assign[static_cast<int64_t>(r) * n + i]) * d;
    double s = 0.0;
    for (int q = 0; q < d; ++q) {
        const double df = __dsub_rn(xt[static_cast<int64_t>(q) * n + i], c[q]);
        s = __dadd_rn(s, __dmul_rn(df, df));
    }
    dist[static_cast<int64_t>(r) * n + i] = s;
}

}  // namespace

namespace fa {
namespace kmeans {

void launch_normalize(hipStream_t stream, const double *x, double *xn, double *xt, const int64_t n, const int d) {
    hipLaunchKernelGGL(km_normalize, dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64), 0, stream, x, xn, xt, n, d);
}

void launch_assign(hipStream_t stream, const LloydArgs &a) {
    const dim3 pgrid(static_cast<unsigned>((a.n + kThreads - 1) / kThreads), a.runs);
    hipLaunchKernelGGL(km_assign, pgrid, dim3(kThreads), 0, stream, a.xt, a.cen, a.assign, a.changed, a.n, a.d, a.k, a.done);
}

void launch_members(hipStream_t stream, const LloydArgs &a) {
    const dim3 cgrid(a.k, a.runs);
    hipLaunchKernelGGL(km_members<0>, cgrid, dim3(64), 0, stream, a.assign, a.changed, a.counts, a.list, a.n, a.k, a.done);
    hipLaunchKernelGGL(km_members<1>, cgrid, dim3(64), 0, stream, a.assign, a.changed, a.counts, a.list, a.n, a.k, a.done);
}

void launch_update(hipStream_t stream, const LloydArgs &a) {
    hipLaunchKernelGGL(km_update, dim3(a.k, a.runs), dim3(std::min(kThreads, ((a.d + 63) / 64) * 64)), 0, stream, a.xn, a.changed, a.counts, a.list, a.cen, a.n, a.d,
                       a.k, a.done);
}

void launch_step_end(hipStream_t stream, const LloydArgs &a, const int it) {
    hipLaunchKernelGGL(km_step_end, dim3(a.runs), dim3(64), 0, stream, a.changed, a.counts, a.done, a.iters, a.picks, a.cursor, a.xn, a.cen, a.status, it, a.d, a.k);
}

void launch_own_distance(hipStream_t stream, const LloydArgs &a, double *dist) {
    const dim3 pgrid(static_cast<unsigned>((a.n + kThreads - 1) / kThreads), a.runs);
    hipLaunchKernelGGL(km_own_distance, pgrid, dim3(kThreads), 0, stream, a.xt, a.cen, a.assign, dist, a.n, a.d, a.k);
}

}  // namespace kmeans
}  // namespace fa
