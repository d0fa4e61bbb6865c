// sortformer.hip — the offline Sortformer diarizer around its network, on the device: the kernels and one launcher per kernel family.
//
//   * packing (reference: Sources/FluidAudio/Diarizer/Sortformer/Offline/OfflineSortformerDiarizer.swift:98-119, 303-363): a recording's
//     mel is tiled into windows of windowOutputFrames * subsampling mel frames that overlap by overlapOutputFrames output frames; each
//     window becomes one model input [n_mels, windowMel] with a zero tail and its mel_length.
//   * stitching (:321-358, SortformerSpeakerStitcher.swift:27-77): per window the S x S correlation of the global timeline's overlap
//     region with the window's first frames (a += g * w: a multiply and an add, this file is built with -ffp-contract=off), the best of
//     the S! bijections in the reference's enumeration order (the swap recursion :80-90), and the merge into the global timeline
//     (first writer stores, later ones average).
//     With 2 * overlap <= window the overlap region has been written by the previous window only and never averaged: it is that
//     window's values moved by its mapping.  So the correlations of all windows are independent (one wavefront each, against the
//     previous window's own columns), the mappings are a short chain per recording over 16 numbers per window, and the merge is
//     parallel over global frames.  Any other geometry runs window by window, one workgroup per recording (stitch_serial): slow.
//
// The host side — window geometry, the window plan, the enumeration of the bijections and the C ABI — is sortformer_host.hip; what both
// share is sortformer_launch.h.  The diarizer timeline that consumes the stitched predictions is a unit of its own, timeline.hip.
#include <climits>

#include "sortformer_launch.h"

namespace {

using namespace fa::sortformer;
constexpr int kThreads = 256;
static_assert(kMergeItems == kThreads, "stitch_merge: one item per thread");

// ---------------------------------------------------------------- packing

// mel-major [n_mels][frame_stride] rows: one workgroup per (window, mel row) copies the row slice and zero-fills the tail.  Stores are
// 16 bytes when the output rows are 16-byte aligned; a group of four loads as 16 bytes when its source is aligned and wholly valid.
__global__ __launch_bounds__(kThreads) void pack_rows(PackArgs a, int vec) {
    const int64_t row = blockIdx.x;
    const int64_t w = row / a.n_mels;
    const int m = static_cast<int>(row - w * a.n_mels);
    const fa_sortformer_window win = a.win[w];
    const float *src = a.mel + win.recording * a.rec_stride + m * a.frame_stride + win.mel_start;
    float *dst = a.out + row * a.window_mel;
    const int valid = win.valid_mel;
    if (m == 0 && threadIdx.x == 0) a.mel_length[w] = valid;
    if (vec) {
        const bool src_al = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
        for (int t = 4 * threadIdx.x; t < a.window_mel; t += 4 * kThreads) {
            float4 v;
            if (src_al && t + 4 <= valid) {
                v = *reinterpret_cast<const float4 *>(src + t);
            } else {
                v.x = t < valid ? src[t] : 0.0f;
                v.y = t + 1 < valid ? src[t + 1] : 0.0f;
                v.z = t + 2 < valid ? src[t + 2] : 0.0f;
                v.w = t + 3 < valid ? src[t + 3] : 0.0f;
            }
            *reinterpret_cast<float4 *>(dst + t) = v;
        }
    } else {
        for (int t = threadIdx.x; t < a.window_mel; t += kThreads) dst[t] = t < valid ? src[t] : 0.0f;
    }
}

// time-major [T][n_mels]: 64 frames x 64 mels through LDS, coalesced along the mels on the way in and along the frames on the way out
__global__ __launch_bounds__(kThreads) void pack_transpose(PackArgs a, int t_tiles, int m_tiles) {
    __shared__ float tile[64][65];
    int64_t b = blockIdx.x;
    const int mt = static_cast<int>(b % m_tiles);
    b /= m_tiles;
    const int tt = static_cast<int>(b % t_tiles);
    const int64_t w = b / t_tiles;
    const fa_sortformer_window win = a.win[w];
    const int valid = win.valid_mel, t0 = tt * 64, m0 = mt * 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    if (tt == 0 && mt == 0 && threadIdx.x == 0) a.mel_length[w] = valid;
    const float *src = a.mel + win.recording * a.rec_stride + win.mel_start * a.n_mels;
    for (int k = 0; k < 16; ++k) {
        const int t = t0 + 4 * k + ly, m = m0 + lx;
        tile[4 * k + ly][lx] = (t < valid && m < a.n_mels) ? src[static_cast<int64_t>(t) * a.n_mels + m] : 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        const int m = m0 + 4 * k + ly, t = t0 + lx;
        if (m < a.n_mels && t < a.window_mel) a.out[(w * a.n_mels + m) * a.window_mel + t] = tile[lx][4 * k + ly];
    }
}

// ---------------------------------------------------------------- stitching

// alignment's search (:56-76) on one wavefront: lane p scores permutation p over corr[g][w] (row g already in global order).  Returns
// the winning permutation's index in every lane, -1 when no score exceeds -Float.greatestFiniteMagnitude (the identity stays).
__device__ inline int best_perm(const Perms &perms, const float *corr, int S, int lane) {
    float score = 0.0f;
    bool ok = lane < perms.n;
    if (ok) {
        for (int g = 0; g < S; ++g) score += corr[g * S + perms.p[lane][g]];
        ok = score > -3.40282347e38f;
    }
    int idx = ok ? lane : INT_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(score, off);
        const int oi = __shfl_xor(idx, off);
        if (oi != INT_MAX && (idx == INT_MAX || os > score || (os == score && oi < idx))) { score = os; idx = oi; }
    }
    return idx == INT_MAX ? -1 : idx;
}

__device__ inline int overlap_frames(const StitchArgs &a, const fa_sortformer_window &w) {
    if (w.first || a.overlap <= 0) return 0;
    const int64_t total = a.gofs[w.recording + 1] - a.gofs[w.recording];
    const int64_t room = total - w.g_start > 0 ? total - w.g_start : 0;
    const int64_t ov = a.overlap < w.valid_out ? a.overlap : w.valid_out;
    return static_cast<int>(ov < room ? ov : room);
}

// One wavefront per window: the overlap region of the global timeline is the previous window's frames hop .. hop + ov in that window's
// own columns.  Lanes < S * S carry one sequential chain each, in frame order; all lanes stage the frames through LDS.
__global__ __launch_bounds__(64) void stitch_corr(StitchArgs a) {
    __shared__ float sp[64 * kMaxSpeakers], sc[64 * kMaxSpeakers];
    const int64_t w = blockIdx.x;
    const fa_sortformer_window win = a.win[w];
    const int lane = threadIdx.x, S = a.S;
    const int ov = overlap_frames(a, win);
    if (lane == 0) a.ov[w] = ov;
    if (ov == 0) return;
    const float *prev = a.preds + ((w - 1) * a.window + a.hop) * S;
    const float *cur = a.preds + w * a.window * S;
    const int g = lane / S, c = lane - g * S;
    float acc = 0.0f;
    for (int f0 = 0; f0 < ov; f0 += 64) {
        const int nf = ov - f0 < 64 ? ov - f0 : 64;
        for (int i = lane; i < nf * S; i += 64) { sp[i] = prev[f0 * S + i]; sc[i] = cur[f0 * S + i]; }
        __syncthreads();
        if (lane < S * S) {
            for (int f = 0; f < nf; ++f) {
                const float gv = sp[f * S + g];
                if (gv != 0.0f) acc += gv * sc[f * S + c];   // guard gv != 0 (:49); multiply, then add
            }
        }
        __syncthreads();
    }
    if (lane < S * S) a.corr[w * S * S + lane] = acc;
}

// One wavefront per recording walks its windows: correlation rows re-indexed through the previous window's inverse mapping, the search,
// and mapping[w] = g.
__global__ __launch_bounds__(64) void stitch_chain(StitchArgs a, Perms perms) {
    __shared__ float corr[kMaxSpeakers * kMaxSpeakers];
    const int r = blockIdx.x, lane = threadIdx.x, S = a.S;
    int inv[kMaxSpeakers] = {0, 1, 2, 3};   // inv[g] = the previous window's column that went to global column g (its winning permutation)
    for (int64_t w = a.range[r]; w < a.range[r + 1]; ++w) {
        int best = -1;
        if (a.ov[w] > 0) {
            if (lane < S * S) { const int g = lane / S, c = lane - g * S; corr[lane] = a.corr[w * S * S + inv[g] * S + c]; }
            __syncthreads();
            best = best_perm(perms, corr, S, lane);
            __syncthreads();
        }
        for (int g = 0; g < S; ++g) inv[g] = best >= 0 ? perms.p[best][g] : g;
        if (lane < S) { int m = 0; for (int g = 0; g < S; ++g) if (inv[g] == lane) m = g; a.mapping[w * S + lane] = m; }
    }
}

// One thread per (global frame, global column): its covering windows in window order (:342-358)
__global__ __launch_bounds__(kThreads) void stitch_merge(StitchArgs a, int64_t items, int reach) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= items) return;
    const int S = a.S;
    const int64_t gf_all = e / S;
    const int g = static_cast<int>(e - gf_all * S);
    int lo = 0, hi = a.B;   // the recording: last r with gofs[r] <= gf_all
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (a.gofs[m] <= gf_all) lo = m; else hi = m; }
    const int r = lo;
    const int64_t gf = gf_all - a.gofs[r], w0 = a.range[r], nw = a.range[r + 1] - w0;
    float v = 0.0f;
    bool filled = false;
    if (nw > 0) {
        const int64_t last = gf / a.hop < nw - 1 ? gf / a.hop : nw - 1;
        for (int64_t i = last > reach ? last - reach : 0; i <= last; ++i) {
            const fa_sortformer_window win = a.win[w0 + i];
            if (gf < win.g_start || gf >= win.g_start + win.valid_out) continue;
            int c = 0;
            for (int k = 0; k < S; ++k) if (a.mapping[(w0 + i) * S + k] == g) c = k;
            const float p = a.preds[((w0 + i) * a.window + (gf - win.g_start)) * S + c];
            v = filled ? (v + p) * 0.5f : p;
            filled = true;
        }
    }
    a.global[e] = v;
}

// Any geometry, as the reference walks it: one workgroup per recording, window by window against the global timeline itself.
__global__ __launch_bounds__(kThreads) void stitch_serial(StitchArgs a, Perms perms) {
    __shared__ float corr[kMaxSpeakers * kMaxSpeakers];
    __shared__ int map[kMaxSpeakers];
    const int r = blockIdx.x, tid = threadIdx.x, S = a.S;
    const int64_t total = a.gofs[r + 1] - a.gofs[r];
    float *global = a.global + a.gofs[r] * S;
    int64_t prev_end = 0;
    for (int64_t w = a.range[r]; w < a.range[r + 1]; ++w) {
        const fa_sortformer_window win = a.win[w];
        const float *cur = a.preds + w * a.window * S;
        const int ov = overlap_frames(a, win);
        if (tid < S) map[tid] = tid;
        if (ov > 0 && tid < S * S) {
            const int g = tid / S, c = tid - g * S;
            float acc = 0.0f;
            for (int f = 0; f < ov; ++f) {
                const float gv = global[(win.g_start + f) * S + g];
                if (gv != 0.0f) acc += gv * cur[f * S + c];
            }
            corr[tid] = acc;
        }
        __syncthreads();
        if (ov > 0 && tid < 64) {
            const int best = best_perm(perms, corr, S, tid);
            if (best >= 0 && tid < S) map[perms.p[best][tid]] = tid;   // mapping[bestPerm[g]] = g
        }
        __syncthreads();
        if (tid < S) a.mapping[w * S + tid] = map[tid];
        for (int i = tid; i < win.valid_out * S; i += kThreads) {
            const int j = i / S, c = i - j * S;
            const int64_t gf = win.g_start + j;
            if (gf >= total) continue;
            const int64_t idx = gf * S + map[c];
            const float p = cur[i];
            global[idx] = (!win.first && gf < prev_end) ? (global[idx] + p) * 0.5f : p;
        }
        prev_end = win.g_start + win.valid_out;
        __syncthreads();
    }
}

}  // namespace

namespace fa {
namespace sortformer {

void launch_pack(hipStream_t stream, const PackArgs &a, const int32_t layout, const int64_t W) {
    if (layout == FA_MEL_LAYOUT_MEL_MAJOR) {
        const int vec = (reinterpret_cast<uintptr_t>(a.out) & 15u) == 0 && a.window_mel % 4 == 0;
        hipLaunchKernelGGL(pack_rows, dim3(static_cast<unsigned>(W * a.n_mels)), dim3(kThreads), 0, stream, a, vec);
    } else {
        const int t_tiles = (a.window_mel + kPackTile - 1) / kPackTile, m_tiles = (a.n_mels + kPackTile - 1) / kPackTile;
        hipLaunchKernelGGL(pack_transpose, dim3(static_cast<unsigned>(W * t_tiles * m_tiles)), dim3(kThreads), 0, stream, a, t_tiles, m_tiles);
    }
}

hipError_t launch_stitch(hipStream_t stream, const StitchArgs &a, const Perms &perms, const int64_t W, const int64_t items) {
    if (2 * a.overlap <= a.window) {
        hipLaunchKernelGGL(stitch_corr, dim3(static_cast<unsigned>(W)), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(stitch_chain, dim3(static_cast<unsigned>(a.B)), dim3(64), 0, stream, a, perms);
        if (items > 0) {
            const int reach = (a.window + a.hop - 1) / a.hop;   // windows that can cover one frame
            hipLaunchKernelGGL(stitch_merge, dim3(fa::grid_for(items, kThreads)), dim3(kThreads), 0, stream, a, items, reach);
        }
        return hipSuccess;
    }
    if (items > 0) {
        const hipError_t e = hipMemsetAsync(a.global, 0, sizeof(float) * items, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(stitch_serial, dim3(static_cast<unsigned>(a.B)), dim3(kThreads), 0, stream, a, perms);
    return hipSuccess;
}

}  // namespace sortformer
}  // namespace fa
