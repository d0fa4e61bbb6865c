// reconstruct.hip — from segmentation logits and per-chunk cluster labels to speaker segments: the kernels and one launcher per stage.
// The frame plan's staging, the host passes over the raw runs and the C ABI are reconstruct_host.hip; the host arithmetic is
// reconstruct_geom.h; what the two units share is reconstruct_launch.h.
//
//   * powerset decode (reference: Sources/FluidAudio/Diarizer/Offline/Segmentation/OfflineSegmentationProcessor.swift:316-409):
//     per chunk frame the first strict maximum of the class logits (seeded at -Float.greatestFiniteMagnitude, so NaN never wins and
//     an all-NaN / all--inf row is class 0), winningClass = min(best, 7), binary weights of the speakers of powerset[winningClass]
//     (table :15-24), and optionally the log-probabilities logits - logSumExp(logits) (VDSPOperations.swift:142-155) in fp32.
//   * OfflineReconstruction.buildSegments (Diarizer/Offline/Utils/OfflineReconstruction.swift:24-237): the chunk frames fold into
//     global frames g = round-half-away((offset + f*fd) / fd) (fp64, no FMA), clamped to [0, totalFrames); per global frame the
//     fp64 activation sums / counts per cluster and the expected speaker count are added in increasing chunk, then frame order;
//     count = clamp(rint_even(expSum / weight), 0, min(K, S)); the first `count` clusters by activation sum descending, ties to the
//     lower index (Swift's stable sort); zero-vote frames (count 1, every sum 0, ZeroVoteReembedder.swift:42-79); a caller's
//     zero-vote overrides replace a frame's clusters by [cluster] (:176-186, :249-298).  Then the segment walk (:188-233): every
//     maximal run of frames in which a cluster is active is one raw segment, start g0*fd, end g1*fd when closed at frame g1 and
//     g_last*fd + fd when still open at the last frame, quality = Float(clamp(scoreSum / frames, 0, 1)) with scoreSum the
//     sequential fp64 sum of the run's per-frame averages (:400-429).
//   * mergeSegments / sanitize / excludeOverlaps (:359-398, :431-496) as host code over the compact raw list (one D2H): reconstruct_host.hip.
//
// Where the reference is not deterministic: raw segments that close at the same frame, and those flushed after the last frame,
// are appended in Swift Dictionary order (hash-seeded), and that order decides merges between speakers whose segments start at the
// same time.  Here the raw order is (closing frame, cluster index ascending); a segment still open after the last frame closes at
// frame totalFrames.
//
// No float atomics: every global frame is owned by one wavefront, which gathers its contributions in the reference's order.
// Non-decreasing chunk offsets (what the segmentation producer emits, offset = c * step) find the chunks covering a tile of global
// frames by binary search; any other offsets (unsorted, duplicated, negative, off-grid) list them with an ordered scan over all
// chunks.  Both visit chunks in increasing index and, per chunk, the frames whose exact forward map is g.
#include <algorithm>
#include <climits>

#include "block_scan.h"
#include "reconstruct_launch.h"

namespace {

using namespace fa::reconstruct;
using fa::grid_for;
constexpr int kThreads = fa::scan::kThreads;

// ---------------------------------------------------------------- powerset decode

__device__ inline void decode_row(const float *x, int classes, float *w, float *lp) {
    int best = 0;
    float bv = -3.40282347e38f;                              // -Float.greatestFiniteMagnitude (:326-335)
    for (int c = 0; c < classes; ++c) if (x[c] > bv) { bv = x[c]; best = c; }
    const unsigned m = powerset_mask(best < 7 ? best : 7);   // min(bestIndex, powerset.count - 1)
    w[0] = (m & 1u) ? 1.0f : 0.0f;
    w[1] = (m & 2u) ? 1.0f : 0.0f;
    w[2] = (m & 4u) ? 1.0f : 0.0f;
    if (lp && classes > 0) {                                 // logSumExp (VDSPOperations.swift:142-155): log(sum(exp(x - max))) + max
        float mx = x[0];
        for (int c = 1; c < classes; ++c) if (mx < x[c]) mx = x[c];
        float s = 0.0f;
        for (int c = 0; c < classes; ++c) s += expf(x[c] - mx);
        const float lse = logf(s) + mx;
        for (int c = 0; c < classes; ++c) lp[c] = x[c] + (-lse);
    }
}

// 7 classes (the community-1 model): 4 rows = 7 float4 in, 3 float4 of weights and 7 float4 of log-probs out per thread
__global__ __launch_bounds__(kThreads) void powerset_decode7(const float4 *__restrict__ x, int64_t groups, float4 *__restrict__ w, float4 *__restrict__ lp) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= groups) return;
    float v[28], wv[12], lv[28];
#pragma unroll
    for (int k = 0; k < 7; ++k) { const float4 t = x[i * 7 + k]; v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w; }
#pragma unroll
    for (int r = 0; r < 4; ++r) decode_row(v + 7 * r, 7, wv + 3 * r, lp ? lv + 7 * r : nullptr);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[i * 3 + k] = make_float4(wv[4 * k], wv[4 * k + 1], wv[4 * k + 2], wv[4 * k + 3]);
    if (lp) {
#pragma unroll
        for (int k = 0; k < 7; ++k) lp[i * 7 + k] = make_float4(lv[4 * k], lv[4 * k + 1], lv[4 * k + 2], lv[4 * k + 3]);
    }
}

// any class count, one row per thread (also the tail rows of the 7-class kernel)
__global__ __launch_bounds__(kThreads) void powerset_decode_rows(const float *__restrict__ x, int64_t row0, int64_t rows, int classes, float *__restrict__ w,
                                                                 float *__restrict__ lp) {
    const int64_t r = row0 + static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float wv[3];
    if (classes <= 16) {
        float v[16];
        for (int c = 0; c < classes; ++c) v[c] = x[r * classes + c];
        decode_row(v, classes, wv, lp ? lp + r * classes : nullptr);
    } else {
        decode_row(x + r * classes, classes, wv, lp ? lp + r * classes : nullptr);
    }
    w[r * 3] = wv[0];
    w[r * 3 + 1] = wv[1];
    w[r * 3 + 2] = wv[2];
}

// ---------------------------------------------------------------- per-frame accumulation and decision

// first index in [0, n) with a[i] >= v (a non-decreasing)
__device__ inline int64_t lower_bound_i32(const int32_t *a, int64_t n, int v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
    return lo;
}

struct Best { double s; int k; int n; };
// (sum descending, cluster ascending): the order of Swift's stable sort by activation sum (:167-174)
__device__ inline bool better(double s, int k, double bs, int bk) { return s > bs || (s == bs && k < bk); }

// One wavefront per global frame.  Lane l holds the sums / counts of clusters kb + l + 64 i (i < KPL) of the tile kb; K > 64 KPL sweeps
// the contributions once per tile and selected rank.
template <int KPL>
__global__ __launch_bounds__(kThreads) void recon_frames(FrameArgs a) {
    __shared__ int32_t list[kListCap];
    __shared__ int32_t wcnt[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g0 = blockIdx.x * kTileG;
    const int g1 = min(g0 + kTileG, a.T) - 1;
    int64_t clo = 0, chi = a.C;
    int nlist = 0;
    bool use_list = false;
    if (a.sorted) {   // chunks whose frames can land in [g0, g1]: last_g >= g0 and first_g <= g1 (both non-decreasing)
        clo = lower_bound_i32(a.last_g, a.C, g0);
        chi = lower_bound_i32(a.first_g, a.C, g1 + 1);
    } else {          // ordered compaction of the chunks whose [first_g, last_g] meets the tile, in increasing chunk index
        int base = 0;
        for (int64_t c0 = 0; c0 < a.C; c0 += kThreads) {
            const int64_t c = c0 + tid;
            const bool hit = c < a.C && a.first_g[c] <= g1 && a.last_g[c] >= g0;
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wcnt[wid] = __popcll(m);
            __syncthreads();
            int off = base, tot = 0;
            for (int v = 0; v < kThreads / 64; ++v) { if (v < wid) off += wcnt[v]; tot += wcnt[v]; }
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
            if (hit && pos < kListCap) list[pos] = static_cast<int32_t>(c);
            base += tot;
            __syncthreads();
        }
        nlist = base;
        use_list = base <= kListCap;
    }

    for (int g = g0 + wid; g <= g1; g += kThreads / 64) {
        // every (c, f) with global_frame(c, f) == g, in increasing c, then f
        auto visit = [&](auto &&fn) {
            auto chunk = [&](int64_t c) {
                if (a.first_g[c] > g || a.last_g[c] < g) return;
                const double off = a.start[c];
                // first f with global_frame >= g: global_frame(c, f) is first_g + f up to rounding, so try that f before a binary search
                int lo = min(max(g - a.first_g[c], 0), a.F - 1);
                if (!((lo == 0 || global_frame(off, lo - 1, a.fd, a.T) < g) && global_frame(off, lo, a.fd, a.T) >= g)) {
                    int hi = a.F;
                    lo = 0;
                    while (lo < hi) { const int m = (lo + hi) >> 1; if (global_frame(off, m, a.fd, a.T) < g) lo = m + 1; else hi = m; }
                }
                for (int f = lo; f < a.F && global_frame(off, f, a.fd, a.T) == g; ++f) fn(c, f);
            };
            if (a.sorted) for (int64_t c = clo; c < chi; ++c) chunk(c);
            else if (use_list) for (int i = 0; i < nlist; ++i) chunk(list[i]);
            else for (int64_t c = 0; c < a.C; ++c) chunk(c);
        };
        double sum[KPL];
        int cnt[KPL];
        double esum = 0.0;
        int ew = 0, badv = 0;
        auto pass = [&](int kb) {   // :79-104 for the clusters of tile kb
            for (int i = 0; i < KPL; ++i) { sum[i] = 0.0; cnt[i] = 0; }
            esum = 0.0;
            ew = 0;
            visit([&](int64_t c, int f) {
                const float *wr = a.w + (c * a.F + f) * a.S;
                const int32_t *hr = a.hard + c * a.S;
                double act[KPL];
                for (int i = 0; i < KPL; ++i) act[i] = 0.0;
                double e = 0.0;
                for (int s = 0; s < a.S; ++s) {
                    const float v = wr[s];
                    if (!isfinite(v)) badv = 1;
                    const double dv = static_cast<double>(v);
                    e += dv;                                          // expectedCount: sequential over the speakers (:90-92)
                    const int k = hr[s] - kb - lane;                  // == 64 i when this lane holds that cluster
                    if (k >= 0 && (k & 63) == 0) {
#pragma unroll
                        for (int i = 0; i < KPL; ++i) if (k == 64 * i && dv > act[i]) act[i] = dv;   // max over the speakers, strict > from 0
                    }
                }
                esum += e;
                ew += 1;
#pragma unroll
                for (int i = 0; i < KPL; ++i) if (act[i] > 0.0) { sum[i] += act[i]; cnt[i] += 1; }
            });
        };
        // the lane's best cluster of the current tile ranked after (ps, pk), reduced over the wavefront
        auto tile_best = [&](int kb, double ps, int pk, Best &b) {
            Best m{-1.0, INT_MAX, 0};
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int k = kb + lane + 64 * i;
                if (k < a.K && better(ps, pk, sum[i], k) && better(sum[i], k, m.s, m.k)) m = Best{sum[i], k, cnt[i]};
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double os = __shfl_xor(m.s, off);
                const int ok = __shfl_xor(m.k, off), on = __shfl_xor(m.n, off);
                if (better(os, ok, m.s, m.k)) m = Best{os, ok, on};
            }
            if (better(m.s, m.k, b.s, b.k)) b = m;
        };
        const int ovr = a.ovr ? a.ovr[g] : -1;
        const int span = 64 * KPL, tiles = (a.K + span - 1) / span;
        int count = 0, nsel = 0;
        bool touched = false;
        double ps = INFINITY, ovr_avg = 0.0;
        int pk = -1;
        for (int r = 0;; ++r) {
            Best b{-1.0, INT_MAX, 0};
            for (int t = 0; t < tiles; ++t) {
                const int kb = t * span;
                if (tiles > 1 || r == 0) pass(kb);
                if (r == 0 && t == 0) {   // :145-156
                    if (ew > 0) {
                        double x = rint(esum / static_cast<double>(ew));
                        if (x > static_cast<double>(a.maxc)) x = static_cast<double>(a.maxc);
                        count = x > 0.0 ? static_cast<int>(x) : 0;
                    }
                    nsel = ovr >= 0 ? 1 : count;
                }
                if (r == 0) {
                    bool any = false;
#pragma unroll
                    for (int i = 0; i < KPL; ++i) any |= cnt[i] > 0;
                    touched |= __any(any) != 0;
                    if (ovr >= kb && ovr < kb + span) {   // the override's average (0 on a zero-vote frame)
                        const int rel = ovr - kb, owner = rel & 63, slot = rel >> 6;
                        double s = 0.0;
                        int n = 0;
#pragma unroll
                        for (int i = 0; i < KPL; ++i) if (i == slot) { s = sum[i]; n = cnt[i]; }
                        s = __shfl(s, owner);
                        n = __shfl(n, owner);
                        ovr_avg = n > 0 ? s / static_cast<double>(n) : 0.0;
                    }
                }
                if (ovr < 0 && r < count) tile_best(kb, ps, pk, b);
            }
            if (ovr < 0 && r < count) {
                if (lane == 0) {
                    a.sel[static_cast<int64_t>(g) * a.smax + r] = b.k;
                    a.avg[static_cast<int64_t>(g) * a.smax + r] = b.n > 0 ? b.s / static_cast<double>(b.n) : 0.0;   // :107-143
                }
                ps = b.s;
                pk = b.k;
            }
            if (ovr >= 0 || r + 1 >= count) break;
        }
        if (lane == 0) {
            if (ovr >= 0) {
                a.sel[static_cast<int64_t>(g) * a.smax] = ovr;
                a.avg[static_cast<int64_t>(g) * a.smax] = ovr_avg;
            }
            a.word[g] = nsel | (count << kSelBits) | ((count == 1 && !touched) ? kZeroVote : 0);
            if (a.esum_out) a.esum_out[g] = esum;
            if (badv) atomicOr(a.bad, 1);
        }
    }
}

// ---------------------------------------------------------------- segment runs

// slot of cluster k among frame g's active clusters, -1 if inactive
__device__ inline int active_slot(const int32_t *word, const int32_t *sel, int smax, int g, int k) {
    const int n = word[g] & kSelMask;
    const int32_t *s = sel + static_cast<int64_t>(g) * smax;
    for (int j = 0; j < n; ++j) if (s[j] == k) return j;
    return -1;
}

// item e = g * smax + j starts a run: slot j is active at g and its cluster was not active at g - 1 (the predicate of block_scan.h's compact)
struct RunStart {
    const int32_t *word, *sel;
    int smax;
    __device__ int operator()(int64_t e) const {
        const int g = static_cast<int>(e / smax), j = static_cast<int>(e - static_cast<int64_t>(g) * smax);
        if (j >= (word[g] & kSelMask)) return 0;
        return g == 0 || active_slot(word, sel, smax, g - 1, sel[e]) < 0;
    }
};
struct StartSink {   // starts[k] = the item of run k
    int64_t *starts;
    __device__ void kept(int64_t e, int pos) const { starts[pos] = e; }
    __device__ void dropped(int64_t) const {}
};

// one lane per run: walk forward while the cluster stays active
__global__ __launch_bounds__(kThreads) void run_walk(const int64_t *__restrict__ starts, const int32_t *__restrict__ total, const int32_t *__restrict__ word,
                                                     const int32_t *__restrict__ sel, const double *__restrict__ avg, int smax, int T, RawRun *__restrict__ out) {
    const int n = *total;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e = starts[i];
        const int g0 = static_cast<int>(e / smax), k = sel[e];
        double s = avg[e];
        int g = g0 + 1;
        for (; g < T; ++g) {
            const int j = active_slot(word, sel, smax, g, k);
            if (j < 0) break;
            s += avg[static_cast<int64_t>(g) * smax + j];
        }
        out[i] = RawRun{g0, g, k, g - g0, s};
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers (reconstruct_launch.h)

namespace fa {
namespace reconstruct {

void launch_powerset(hipStream_t st, const float *x, int64_t rows, int32_t classes, float *w, float *lp) {
    const auto aligned = [](const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    int64_t row0 = 0;
    if (classes == 7 && aligned(x) && aligned(w) && aligned(lp)) {
        const int64_t groups = rows / 4;
        if (groups > 0)
            hipLaunchKernelGGL(powerset_decode7, dim3(grid_for(groups, kThreads)), dim3(kThreads), 0, st, reinterpret_cast<const float4 *>(x), groups,
                               reinterpret_cast<float4 *>(w), reinterpret_cast<float4 *>(lp));
        row0 = groups * 4;
    }
    if (row0 < rows) hipLaunchKernelGGL(powerset_decode_rows, dim3(grid_for(rows - row0, kThreads)), dim3(kThreads), 0, st, x, row0, rows, classes, w, lp);
}

int64_t run_blocks(int64_t items) { return fa::scan::compact_blocks(items); }

void launch_frames(hipStream_t st, const FrameArgs &a, int32_t *bsum, int32_t *total, int64_t *starts) {
    const unsigned fgrid = grid_for(a.T, kTileG);
    if (a.K <= 64) hipLaunchKernelGGL(recon_frames<1>, dim3(fgrid), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(recon_frames<4>, dim3(fgrid), dim3(kThreads), 0, st, a);
    fa::scan::compact(st, RunStart{a.word, a.sel, a.smax}, StartSink{starts}, static_cast<int64_t>(a.T) * a.smax, bsum, total);
}

void launch_walk(hipStream_t st, const FrameArgs &a, const int64_t *starts, const int32_t *total, int64_t n_raw, RawRun *out) {
    hipLaunchKernelGGL(run_walk, dim3(std::min<unsigned>(grid_for(n_raw, kThreads), 4096)), dim3(kThreads), 0, st, starts, total, a.word, a.sel, a.avg, a.smax,
                       a.T, out);
}

}  // namespace reconstruct
}  // namespace fa
