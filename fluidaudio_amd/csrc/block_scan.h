// block_scan.h — the ordered compaction of the kernel units, in three pieces:
//   block_exclusive, workgroup_exclusive  the exclusive prefix over one workgroup, and the loop that carries it over n items, kThreads a pass;
//   scan_totals                           that loop over per-block (per-recording, per-chunk) counts in place: counts -> offsets, sum -> *total;
//   compact (_count, _write, _blocks)     `items` items under a predicate: per-block counts, scan_totals, a write pass that places the kept.
// Users: embedding.hip (jobs, model runs) and reconstruct.hip (segment run starts) call compact; online.hip scans its run flags with
// workgroup_exclusive and its chunks' segment counts with scan_totals; vad.hip counts with block_exclusive, places its recordings with
// scan_totals and its records with workgroup_exclusive; fsmn_vad.hip and tdt_plan.hip place their recordings' records with scan_totals;
// timeline.hip calls block_exclusive and scan_totals around its own fused tile pass.  The host units never see any of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fa {
namespace scan {

constexpr int kThreads = 256;   // workgroup size of every kernel that calls block_exclusive
constexpr int kPer = 8;         // items per thread of a compaction

// exclusive prefix over the workgroup; *total = the sum
__device__ inline int block_exclusive(int v, int *total) {
    __shared__ int wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off); if (lane >= off) x += y; }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < kThreads / 64; ++w) { if (w < wid) base += wsum[w]; tot += wsum[w]; }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// The exclusive prefix of value_of(i), i in [0, n), over one workgroup of kThreads: place(i, v, at) with at = the sum of the values before
// i; the sum of all is returned.  block_exclusive holds a static __shared__ array and two barriers, so every thread must call it the
// same number of times: the trip count depends on n alone, and a thread past n takes part with 0.  Its second barrier also separates
// one pass from the next.  value_of(i) and place(i, ...) of one i run in the same thread.
template <class Index, class ValueOf, class Place>
__device__ inline int workgroup_exclusive(const Index n, const ValueOf &value_of, const Place &place) {
    int base = 0;
    for (Index i0 = 0; i0 < n; i0 += kThreads) {
        const Index i = i0 + static_cast<Index>(threadIdx.x);
        const int v = i < n ? value_of(i) : 0;
        int tot;
        const int at = base + block_exclusive(v, &tot);
        if (i < n) place(i, v, at);
        base += tot;
    }
    return base;
}

// exclusive scan of the nb block totals in place, one workgroup of kThreads; the sum -> *total.  A template so that every unit including
// this header shares one definition.
template <int kBlock = kThreads>
__global__ __launch_bounds__(kBlock) void scan_totals(int32_t *__restrict__ bsum, int64_t nb, int32_t *__restrict__ total) {
    static_assert(kBlock == kThreads, "block_exclusive assumes kThreads");
    const int sum = workgroup_exclusive(nb, [&](const int64_t b) { return bsum[b]; }, [&](const int64_t b, int, const int at) { bsum[b] = at; });
    if (threadIdx.x == 0) *total = sum;
}

// ---- the compaction of `items` items: a thread takes kPer consecutive items, a workgroup kThreads * kPer.
// Pred:  int operator()(int64_t item), item < items.
// Sink:  kept(int64_t item, int pos) for the item that is the pos-th kept one, dropped(int64_t item) for every other item below `items`.

inline int64_t compact_blocks(const int64_t items) { return (items + kThreads * kPer - 1) / (kThreads * kPer); }

template <class Pred>
__global__ __launch_bounds__(kThreads) void compact_count(const Pred pred, const int64_t items, int32_t *__restrict__ bsum) {
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kPer;
    int c = 0;
    for (int i = 0; i < kPer; ++i) if (e0 + i < items) c += pred(e0 + i) ? 1 : 0;
    int tot;
    (void)block_exclusive(c, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// boff: the block offsets scan_totals left.  The predicate is evaluated once per item, into the flag word.
template <class Pred, class Sink>
__global__ __launch_bounds__(kThreads) void compact_write(const Pred pred, const Sink sink, const int64_t items, const int32_t *__restrict__ boff) {
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kPer;
    int flags = 0, c = 0;
    for (int i = 0; i < kPer; ++i) if (e0 + i < items && pred(e0 + i)) { flags |= 1 << i; ++c; }
    int tot;
    int pos = boff[blockIdx.x] + block_exclusive(c, &tot);
    for (int i = 0; i < kPer; ++i) {
        if (e0 + i >= items) break;
        if (flags & (1 << i)) sink.kept(e0 + i, pos++);
        else sink.dropped(e0 + i);
    }
}

// count, scan_totals, write, in stream order.  bsum: compact_blocks(items) ints; the number kept -> *total.
template <class Pred, class Sink>
inline void compact(hipStream_t stream, const Pred pred, const Sink sink, const int64_t items, int32_t *bsum, int32_t *total) {
    const int64_t nb = compact_blocks(items);
    const dim3 grid(static_cast<unsigned>(nb));
    hipLaunchKernelGGL((compact_count<Pred>), grid, dim3(kThreads), 0, stream, pred, items, bsum);
    hipLaunchKernelGGL(scan_totals<>, dim3(1), dim3(kThreads), 0, stream, bsum, nb, total);
    hipLaunchKernelGGL((compact_write<Pred, Sink>), grid, dim3(kThreads), 0, stream, pred, sink, items, bsum);
}

}  // namespace scan
}  // namespace fa
