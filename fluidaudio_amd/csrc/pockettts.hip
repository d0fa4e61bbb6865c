// pockettts.hip — the kernels of the PocketTTS session (host code: pockettts_host.hip; the integers and the EOS machine:
// pockettts_core.h; operands and geometry: pockettts_launch.h).
//
//   clone_kernel      conditioning extraction fused with the re-projection (VoiceCloner :79-118, :321-376), grid (frame tile, clone).  A
//                     tile past `usable` leaves before any load.  Per slice of 256 dims the workgroup loads 32 frames x 256 dims once
//                     with 16-byte loads (strides and the fp16 widening resolved there; the strided source with scalar loads) into
//                     LDS; wavefront w multiplies dims [64 w, 64 w + 64) of the slice into its 32 x 32 partial of the latents with
//                     v_mfma_f32_32x32x2_f32: lane (m = lane % 32, h = lane / 32) reads frame m's dims 4 h .. 4 h + 3 of an 8-dim chunk as
//                     one float4 and feeds them to four issues, whose B operand is Pinv[dim][n = lane % 32] (128-byte lines through
//                     L2).  The four partials meet in LDS as ((p0 + p1) + p2) + p3.  Stage two: lane (m, h) holds latents[m][16 h ..
//                     16 h + 15], the B operand of issue j is W[d0 + n][16 h + j] (64 contiguous bytes a lane), a wavefront makes 8
//                     column tiles of 32; a store instruction writes two rows' 128-byte segments.  The latents never reach HBM, no
//                     atomics, rows from `usable` on are not written.  Projection -1: the loaded rows go straight out.
//   kv_reset_kernel   grid (slices, layer x side, stream): head rows from the voice's snapshot, the zero tail behind them, 16-byte
//                     loads and stores, fp32 -> fp16 round to nearest even; the first workgroup of a stream writes its positions.
//   kv_capture_kernel the way back: rows [0, seq) of a stream's cache into the voice table (fp16 widened), positions -> offsets.
//   prefill_kernel    one wavefront per (window, row), four 16-byte stores a lane; advance_kernel adds the streams' rows to their positions.
//   step_kernel       one workgroup, lane = stream: the EOS machine, sequence <- latent, positions + 1, the running list by the block scan.
//   append_kernel     an emitting stream's 1920 samples to its frame of the audio slab.
#include <hip/hip_fp16.h>

#include "block_scan.h"
#include "pockettts_launch.h"
#include "row_pack.h"

using namespace fa::pockettts;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float widen(const float v) { return v; }
__device__ __forceinline__ float widen(const _Float16 v) { return static_cast<float>(v); }

// the row of the 32 x 32 result a lane holds in register i
__device__ __forceinline__ int mfma_row(const int i, const int h) { return 8 * (i >> 2) + 4 * h + (i & 3); }

template <class T, bool kVec>
__global__ __launch_bounds__(kCloneThreads) void clone_kernel(const CloneArgs a) {
    constexpr int G = 16 / sizeof(T);   // dims of a 16-byte load
    __shared__ __attribute__((aligned(16))) float slice[kTileFrames * kSliceStride];
    __shared__ float part[kCloneThreads / 64][kTileFrames * kLatent];
    __shared__ float lat[kTileFrames * kLatStride];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, f0 = static_cast<int>(blockIdx.x) * kTileFrames;
    const CloneItem it = a.items[b];
    if (f0 >= it.usable) return;
    const int live = it.usable - f0 < kTileFrames ? it.usable - f0 : kTileFrames;
    const bool copy = it.projection < 0;
    const T *cond = static_cast<const T *>(a.cond) + b * a.item_stride + f0 * a.frame_stride;
    float *out = a.voice_rows + (static_cast<int64_t>(it.voice) * kMaxVoiceFrames + f0) * kDim;
    const float *pinv = a.projections + static_cast<int64_t>(copy ? 0 : it.projection) * 2 * kDim * kLatent, *w = pinv + kDim * kLatent;

    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int ks = 0; ks < kSteps; ++ks) {
        for (int i = tid; i < kTileFrames * kSliceDims / G; i += kCloneThreads) {
            const int f = i / (kSliceDims / G), c = G * (i - f * (kSliceDims / G)), d = ks * kSliceDims + c;
            float v[G];
#pragma unroll
            for (int j = 0; j < G; ++j) v[j] = 0.0f;
            if (f < live) {
                const T *src = cond + f * a.frame_stride + d * a.dim_stride;
                if (kVec) {
                    const uint4 raw = *reinterpret_cast<const uint4 *>(src);
                    const T *e = reinterpret_cast<const T *>(&raw);
#pragma unroll
                    for (int j = 0; j < G; ++j) v[j] = widen(e[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < G; ++j) v[j] = widen(src[j * a.dim_stride]);
                }
            }
            float *dst = copy ? out + static_cast<int64_t>(f) * kDim + d : slice + f * kSliceStride + c;
            if (copy && f >= live) continue;
#pragma unroll
            for (int j = 0; j < G; j += 4) *reinterpret_cast<float4 *>(dst + j) = make_float4(v[j], v[j + 1], v[j + 2], v[j + 3]);
        }
        if (copy) continue;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kSliceDims / 4 / 8; ++c) {
            const int cc = wave * (kSliceDims / 4) + c * 8 + 4 * h;
            const float4 av = *reinterpret_cast<const float4 *>(slice + m * kSliceStride + cc);
            const float *bp = pinv + static_cast<int64_t>(ks * kSliceDims + cc) * kLatent + m;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bp[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bp[kLatent], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bp[2 * kLatent], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bp[3 * kLatent], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (copy) return;

#pragma unroll
    for (int i = 0; i < 16; ++i) part[wave][mfma_row(i, h) * kLatent + m] = acc[i];
    __syncthreads();
    for (int e = tid; e < kTileFrames * kLatent; e += kCloneThreads)
        lat[(e / kLatent) * kLatStride + (e % kLatent)] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
    __syncthreads();

    float av[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) av[j] = lat[m * kLatStride + 16 * h + j];
    for (int nt = 0; nt < kDim / 4 / 32; ++nt) {
        const int d0 = wave * (kDim / 4) + nt * 32;
        const float4 *bp = reinterpret_cast<const float4 *>(w + static_cast<int64_t>(d0 + m) * kLatent + 16 * h);
        float bv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float4 t = bp[q]; bv[4 * q] = t.x; bv[4 * q + 1] = t.y; bv[4 * q + 2] = t.z; bv[4 * q + 3] = t.w; }
        floatx16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], o, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mfma_row(i, h);
            if (row < live) out[static_cast<int64_t>(row) * kDim + d0 + m] = o[i];
        }
    }
}

__device__ __forceinline__ uint32_t half_pair(const float lo, const float hi) {   // round to nearest even, each
    const _Float16 a = static_cast<_Float16>(lo), b = static_cast<_Float16>(hi);
    uint16_t ua, ub;
    __builtin_memcpy(&ua, &a, 2);
    __builtin_memcpy(&ub, &b, 2);
    return static_cast<uint32_t>(ua) | (static_cast<uint32_t>(ub) << 16);
}

template <bool kHalf>
__global__ __launch_bounds__(kThreads) void kv_reset_kernel(const KvArgs a) {
    constexpr int E = kHalf ? 8 : 4;   // elements of a 16-byte store
    const KvItem it = a.items[blockIdx.z];
    const int layer = blockIdx.y >> 1, kv = blockIdx.y & 1, tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < a.n_positions)
        a.positions[static_cast<int64_t>(it.stream) * a.n_positions + tid] = it.voice >= 0 ? a.voice_offsets[it.voice * kMaxLayers + tid] : 0.0f;
    const int64_t head = it.voice >= 0 ? static_cast<int64_t>(it.src_seq) * kKvRow : 0;
    const float *src = a.voice_kv + ((static_cast<int64_t>(it.voice >= 0 ? it.voice : 0) * a.layers + layer) * 2 + kv) * a.voice_plane;
    const int64_t at = kv_plane_at(a.format, a.streams, a.layers, it.stream, layer, kv);
    uint4 *dst = kHalf ? reinterpret_cast<uint4 *>(static_cast<uint16_t *>(a.kv) + at) : reinterpret_cast<uint4 *>(static_cast<float *>(a.kv) + at);
    const int64_t u0 = static_cast<int64_t>(blockIdx.x) * kKvUnits * kThreads + tid;   // kPlane is a multiple of E kKvUnits kThreads
    uint4 v[kKvUnits];
#pragma unroll
    for (int j = 0; j < kKvUnits; ++j) {   // every load of the thread is in flight before its first store
        const int64_t e0 = (u0 + j * kThreads) * E;
        v[j] = make_uint4(0u, 0u, 0u, 0u);
        if (e0 < head) {   // head is a multiple of 1024: a unit lies on one side
            if (kHalf) {
                const float4 p = *reinterpret_cast<const float4 *>(src + e0), q = *reinterpret_cast<const float4 *>(src + e0 + 4);
                v[j] = make_uint4(half_pair(p.x, p.y), half_pair(p.z, p.w), half_pair(q.x, q.y), half_pair(q.z, q.w));
            } else {
                v[j] = *reinterpret_cast<const uint4 *>(src + e0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kKvUnits; ++j) dst[u0 + j * kThreads] = v[j];
}
static_assert(kPlane % (8 * kKvUnits * kThreads) == 0, "a plane is whole workgroups of the reset");

template <bool kHalf>
__global__ __launch_bounds__(kThreads) void kv_capture_kernel(const KvArgs a) {
    constexpr int E = kHalf ? 8 : 4;
    const KvItem it = a.items[0];
    const int layer = blockIdx.y >> 1, kv = blockIdx.y & 1, tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < a.layers)
        a.voice_offsets[it.voice * kMaxLayers + tid] = a.positions[static_cast<int64_t>(it.stream) * a.n_positions + (a.n_positions == 1 ? 0 : tid)];
    const int64_t u = static_cast<int64_t>(blockIdx.x) * kThreads + tid, e0 = u * E;
    if (e0 >= static_cast<int64_t>(it.src_seq) * kKvRow) return;
    float *dst = a.voice_kv + ((static_cast<int64_t>(it.voice) * a.layers + layer) * 2 + kv) * a.voice_plane + e0;
    const int64_t at = kv_plane_at(a.format, a.streams, a.layers, it.stream, layer, kv) + e0;
    if (kHalf) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(a.kv) + at);
        const _Float16 *e = reinterpret_cast<const _Float16 *>(&raw);
        *reinterpret_cast<float4 *>(dst) = make_float4(widen(e[0]), widen(e[1]), widen(e[2]), widen(e[3]));
        *reinterpret_cast<float4 *>(dst + 4) = make_float4(widen(e[4]), widen(e[5]), widen(e[6]), widen(e[7]));
    } else {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(static_cast<const float *>(a.kv) + at);
    }
}

__global__ __launch_bounds__(kThreads) void prefill_kernel(const PrefillArgs a) {
    const int y = blockIdx.y, lane = threadIdx.x & 63, r = static_cast<int>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
    const Window w = a.windows[y];
    float4 *dst = reinterpret_cast<float4 *>(a.arena + (static_cast<int64_t>(y) * kWindow + r) * kDim);
    const float4 *src = nullptr;
    if (r < w.n) {
        const int t = w.first + r;
        if (w.block == 0) {   // KVCache :292-297
            src = reinterpret_cast<const float4 *>(t == 0 ? a.bos_before_voice : a.voice_rows + (static_cast<int64_t>(w.voice) * kMaxVoiceFrames + t - 1) * kDim);
        } else {              // Synthesizer :1213-1222
            int id = a.ids[w.ids_at + t];
            id = id < 0 ? 0 : (id > a.vocab - 1 ? a.vocab - 1 : id);
            src = reinterpret_cast<const float4 *>(a.table + static_cast<int64_t>(id) * kDim);
        }
    }
#pragma unroll
    for (int j = 0; j < kDim / 4 / 64; ++j) dst[lane + 64 * j] = src ? src[lane + 64 * j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r == 0 && lane == 0) {
        a.valid_len[y] = static_cast<float>(w.n);
        a.window_position[y] = a.positions[static_cast<int64_t>(w.stream) * a.n_positions] + static_cast<float>(w.before);
    }
}

__global__ __launch_bounds__(kThreads) void advance_kernel(const AdvanceItem *items, const int n, float *positions, const int n_positions) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    for (int p = 0; p < n_positions; ++p) positions[static_cast<int64_t>(items[i].stream) * n_positions + p] += static_cast<float>(items[i].rows);
}

__global__ void position_set_kernel(float *positions, const int n_positions, const float value) {
    if (static_cast<int>(threadIdx.x) < n_positions) positions[threadIdx.x] = value;
}

__global__ __launch_bounds__(kLatent) void step_begin_kernel(const BeginItem *items, StreamState *state, float *sequence, const float *bos_embedding, const int use_bos) {
    const BeginItem it = items[blockIdx.x];
    const int j = threadIdx.x;
    if (j == 0) state[it.stream] = begin_state(it.max_gen, it.after);
    sequence[it.stream * kLatent + j] = use_bos ? bos_embedding[j] : __builtin_nanf("");   // Synthesizer :1255-1277
}

// eos_logit nullptr: no step is taken, the running list alone is rebuilt (after step_begin)
__global__ __launch_bounds__(fa::scan::kThreads) void step_kernel(const StepArgs a) {
    const int total = fa::scan::workgroup_exclusive(
        a.streams,
        [&](const int s) {
            StreamState m = a.state[s];
            if (a.eos_logit) {
                if (m.reason == kRunning && advance(m, a.eos_logit[s])) {   // Synthesizer :552-567, StateEngine :212
                    for (int j = 0; j < kLatent; ++j) a.sequence[s * kLatent + j] = a.latent[s * kLatent + j];
                    for (int p = 0; p < a.n_positions; ++p) a.positions[static_cast<int64_t>(s) * a.n_positions + p] += 1.0f;
                } else {
                    m.emit = 0;
                }
                a.state[s] = m;
            }
            return m.reason == kRunning ? 1 : 0;
        },
        [&](const int s, const int v, const int at) { if (v) a.running[at] = s; });
    if (threadIdx.x == 0) *a.n_running = total;
}

__global__ __launch_bounds__(kThreads) void append_kernel(const StreamState *state, const float *samples, float *audio, const int max_frames) {
    const int s = blockIdx.x;
    const StreamState m = state[s];
    if (!m.emit) return;
    float *dst = audio + (static_cast<int64_t>(s) * max_frames + m.frames - 1) * kFrameSamples;
    for (int i = threadIdx.x; i < kFrameSamples; i += kThreads) dst[i] = samples[static_cast<int64_t>(s) * kFrameSamples + i];
}

}  // namespace

namespace fa {
namespace pockettts {

void run_encoder_rows(const float *pcm, const rows::Group &g, float *rows, const bool wide, hipStream_t stream) {
    rows::launch_pack<false>(stream, pcm, g, kEncoderSamples, rows, nullptr, wide);   // VoiceCloner :281-288
}

void run_clone(const CloneArgs &a, const int32_t dtype, const int n, hipStream_t stream) {
    const dim3 grid((kMaxVoiceFrames + kTileFrames - 1) / kTileFrames, static_cast<unsigned>(n));
    if (dtype == FA_DTYPE_F16) {
        if (a.vec) hipLaunchKernelGGL((clone_kernel<_Float16, true>), grid, dim3(kCloneThreads), 0, stream, a);
        else hipLaunchKernelGGL((clone_kernel<_Float16, false>), grid, dim3(kCloneThreads), 0, stream, a);
    } else {
        if (a.vec) hipLaunchKernelGGL((clone_kernel<float, true>), grid, dim3(kCloneThreads), 0, stream, a);
        else hipLaunchKernelGGL((clone_kernel<float, false>), grid, dim3(kCloneThreads), 0, stream, a);
    }
}

void run_kv_reset(const KvArgs &a, const int n, hipStream_t stream) {
    const bool half = a.format == kKvHalf;
    const dim3 grid(static_cast<unsigned>(kPlane / ((half ? 8 : 4) * kKvUnits * kThreads)), static_cast<unsigned>(2 * a.layers), static_cast<unsigned>(n));
    if (half) hipLaunchKernelGGL(kv_reset_kernel<true>, grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(kv_reset_kernel<false>, grid, dim3(kThreads), 0, stream, a);
}

void run_kv_capture(const KvArgs &a, hipStream_t stream) {
    const bool half = a.format == kKvHalf;
    const dim3 grid(grid_for(a.voice_plane / (half ? 8 : 4), kThreads), static_cast<unsigned>(2 * a.layers));
    if (half) hipLaunchKernelGGL(kv_capture_kernel<true>, grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(kv_capture_kernel<false>, grid, dim3(kThreads), 0, stream, a);
}

void run_prefill(const PrefillArgs &a, const int n_windows, const AdvanceItem *advance, float *positions, const int n_streams, hipStream_t stream) {
    if (n_windows > 0) hipLaunchKernelGGL(prefill_kernel, dim3(kWindow / (kThreads / 64), static_cast<unsigned>(n_windows)), dim3(kThreads), 0, stream, a);
    if (n_streams > 0) hipLaunchKernelGGL(advance_kernel, dim3(grid_for(n_streams, kThreads)), dim3(kThreads), 0, stream, advance, n_streams, positions, a.n_positions);
}

void run_position_set(float *positions, const int n_positions, const float value, hipStream_t stream) {
    hipLaunchKernelGGL(position_set_kernel, dim3(1), dim3(64), 0, stream, positions, n_positions, value);
}

void run_step_begin(const BeginItem *items, const int n, StreamState *state, float *sequence, const float *bos_embedding, const int use_bos, hipStream_t stream) {
    if (n > 0) hipLaunchKernelGGL(step_begin_kernel, dim3(static_cast<unsigned>(n)), dim3(kLatent), 0, stream, items, state, sequence, bos_embedding, use_bos);
}

void run_step(const StepArgs &a, hipStream_t stream) { hipLaunchKernelGGL(step_kernel, dim3(1), dim3(fa::scan::kThreads), 0, stream, a); }

void run_append_audio(const StreamState *state, const float *samples, float *audio, const int streams, const int max_frames, hipStream_t stream) {
    hipLaunchKernelGGL(append_kernel, dim3(static_cast<unsigned>(streams)), dim3(kThreads), 0, stream, state, samples, audio, max_frames);
}

}  // namespace pockettts
}  // namespace fa
