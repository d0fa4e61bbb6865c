// block_scan.h — the scan behind the block-scan compactions of the kernel units reconstruct.hip (segment run starts, issued by its
// launch_frames) and embedding.hip (jobs, model runs, issued by its launch_select); their host units never see it.  A per-block count
// kernel writes one total per workgroup, scan_totals turns them into exclusive offsets in one workgroup, and a write kernel places each
// kept item at its block's offset plus block_exclusive of its thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fa {
namespace scan {

constexpr int kThreads = 256;   // workgroup size of every kernel that calls block_exclusive

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

// exclusive scan of the nb block totals in place, one workgroup of kThreads; the sum -> *total.  A template so that every unit including
// this header shares one definition.
template <int kBlock = kThreads>
__global__ __launch_bounds__(kBlock) void scan_totals(int32_t *__restrict__ bsum, int64_t nb, int32_t *__restrict__ total) {
    static_assert(kBlock == kThreads, "block_exclusive assumes kThreads");
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kBlock) {
        const int64_t b = b0 + threadIdx.x;
        const int v = b < nb ? bsum[b] : 0;
        int tot;
        const int ex = block_exclusive(v, &tot);
        if (b < nb) bsum[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

}  // namespace scan
}  // namespace fa
