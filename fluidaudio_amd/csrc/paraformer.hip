// paraformer.hip — the kernels of the Paraformer stages: continuous integrate-and-fire with the decoder's input packing
// (ParaformerCif.swift:19-50, ParaformerManager.swift:416-448, 465-486) and the raw token spans of decodeWithTimestamps
// (ParaformerManager.swift:134-358).  Every fp32 chain of the reference is evaluated in the reference's order, one operation at a time
// (this unit is built without FMA contraction), the time arithmetic is fp64: the results are the reference's bit for bit.
// paraformer_launch.h says how the work is laid out; the host side is paraformer_host.hip.
//
// No kernel here uses an atomic on memory another workgroup reads, and no wavefront waits for another.  What one lane of a wavefront
// writes to the workspace and another lane of the SAME wavefront reads later (fire frames, kept positions, spacings) is ordered by a
// workgroup-scope fence.
#include "paraformer_launch.h"

namespace {

using fa::paraformer::CifArgs;
using fa::paraformer::Span;
using fa::paraformer::StampArgs;
constexpr int kWave = fa::paraformer::kWave;
constexpr int kHop = fa::paraformer::kHop;
constexpr int kEnvBlock = fa::paraformer::kEnvBlock;
constexpr int kEnvChunk = fa::paraformer::kEnvChunk;
constexpr int kRows = 4;   // encoder rows a wavefront has in flight before it adds them, in order

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ inline float lane_value(const float v, const int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }   // i is wave-uniform
__device__ inline int below(const unsigned long long m, const int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }
__device__ inline void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

// V elements of a row from p, widened to fp32
template <int V> __device__ inline void load_row(const float *p, float (&h)[V]) {
    if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
        h[0] = v[0]; h[1] = v[1]; h[2] = v[2]; h[3] = v[3];
    } else {
        static_assert(V == 1, "fp32 rows are loaded 4 or 1 at a time");
        h[0] = p[0];
    }
}
template <int V> __device__ inline void load_row(const _Float16 *p, float (&h)[V]) {
    if constexpr (V == 8) {
        const f16x8 v = *reinterpret_cast<const f16x8 *>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = static_cast<float>(v[i]);
    } else if constexpr (V == 4) {
        const f16x4 v = *reinterpret_cast<const f16x4 *>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = static_cast<float>(v[i]);
    } else {
        static_assert(V == 1, "fp16 rows are loaded 8, 4 or 1 at a time");
        h[0] = static_cast<float>(p[0]);
    }
}
template <int V> __device__ inline void store_row(float *p, const float (&h)[V]) {
    if constexpr (V == 1) {
        p[0] = h[0];
    } else {
#pragma unroll
        for (int i = 0; i < V; i += 4) *reinterpret_cast<f32x4 *>(p + i) = f32x4{h[i], h[i + 1], h[i + 2], h[i + 3]};
    }
}

// ---------------------------------------------------------------------------------------------------------------- CIF
// One wavefront per utterance walks the alpha chain (:33-47), every lane the same chain: the alphas arrive 64 at a time, one per lane, and
// are handed round by readlane; lane i keeps what step i of the block decided.  The fire frames are compacted by a ballot.
__global__ __launch_bounds__(kWave) void cif_scan(const CifArgs a) {
    const int lane = threadIdx.x;
    const int32_t b = blockIdx.x;
    const int32_t T = a.valid[b];
    const int64_t base = static_cast<int64_t>(b) * (a.frames + 1);
    const float *alpha = a.alphas + static_cast<int64_t>(b) * a.alpha_stride;
    const float threshold = a.threshold;
    float integrate = 0.0f;
    int32_t count = 0;
    for (int32_t c0 = 0; c0 <= T; c0 += kWave) {
        const int32_t t = c0 + lane;
        const float mine = t < T ? alpha[t] : a.tail;   // frame T is the tail frame; the lanes behind it are not stepped
        float my_w = 0.0f, my_seed = 0.0f;
        bool my_fire = false;
        const int steps = min(kWave, T + 1 - c0);
        for (int i = 0; i < steps; ++i) {
            const float al = lane_value(mine, i);
            integrate += al;
            float w = al, seed = 0.0f;
            bool fire = false;
            if (!(integrate < threshold)) {
                const float used = al - (integrate - threshold);
                w = used;
                integrate -= threshold;
                seed = al - used;
                fire = true;
            }
            if (lane == i) { my_w = w; my_seed = seed; my_fire = fire; }
        }
        if (t <= T) { a.w[base + t] = my_w; a.seed[base + t] = my_seed; }
        const unsigned long long m = __ballot(my_fire);
        if (my_fire) a.fires[base + count + below(m, lane)] = t;
        count += __popcll(m);
    }
    for (int32_t i = count + lane; i <= a.frames; i += kWave) a.fires[base + i] = -1;
    if (lane == 0) {
        a.counts[b] = min(count, a.max_tokens);
        a.counts[a.batch + b] = count;
    }
}

// One wavefront per (utterance, token, slice of 64 V elements): the token's rows in ascending order into one accumulator per element,
// from the seed product on (:41-46); kRows loads are in flight before the adds that need them.  Tokens behind the count are zeros.
template <int V, class E>
__global__ __launch_bounds__(kWave) void cif_gather(const CifArgs a, const int32_t slices) {
    const int lane = threadIdx.x;
    const int32_t slice = blockIdx.x % slices, l = (blockIdx.x / slices) % a.max_tokens, b = blockIdx.x / slices / a.max_tokens;
    const int32_t d0 = (slice * kWave + lane) * V;
    if (d0 >= a.dim) return;   // V divides dim: a lane's elements are all inside or all outside
    float *out = a.ac + (static_cast<int64_t>(b) * a.max_tokens + l) * a.dim + d0;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0f;
    if (l >= a.counts[b]) {
        store_row<V>(out, acc);
        return;
    }
    const int32_t T = a.valid[b];
    const int64_t base = static_cast<int64_t>(b) * (a.frames + 1);
    const E *rows = static_cast<const E *>(a.enc) + static_cast<int64_t>(b) * a.matrix_stride + d0;
    const float *w = a.w + base;
    int32_t t = 0;
    if (l > 0) {   // the leftover of the frame that fired the token before: a product, not zero plus a product
        const int32_t f = a.fires[base + l - 1];
        const float left = a.seed[base + f];
        float h[V];
#pragma unroll
        for (int v = 0; v < V; ++v) h[v] = 0.0f;
        if (f < T) load_row<V>(rows + static_cast<int64_t>(f) * a.row_stride, h);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = h[v] * left;
        t = f + 1;
    }
    const int32_t f = a.fires[base + l];
    for (; t <= f; t += kRows) {
        float h[kRows][V];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
#pragma unroll
            for (int v = 0; v < V; ++v) h[k][v] = 0.0f;   // the tail frame's hidden row
            if (t + k <= f && t + k < T) load_row<V>(rows + static_cast<int64_t>(t + k) * a.row_stride, h[k]);
        }
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            if (t + k <= f) {
                const float wk = w[t + k];
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += wk * h[k][v];
            }
        }
    }
    store_row<V>(out, acc);
}

// The decoder's enc (:423-426): rows below min(valid, enc_frames) widened, zeros behind them.
template <int V, class E>
__global__ __launch_bounds__(kWave) void cif_pack(const CifArgs a, const int32_t slices) {
    const int lane = threadIdx.x;
    const int32_t slice = blockIdx.x % slices, r = (blockIdx.x / slices) % a.enc_frames, b = blockIdx.x / slices / a.enc_frames;
    const int32_t d0 = (slice * kWave + lane) * V;
    if (d0 >= a.dim) return;
    float h[V];
#pragma unroll
    for (int v = 0; v < V; ++v) h[v] = 0.0f;
    if (r < a.valid[b]) load_row<V>(static_cast<const E *>(a.enc) + static_cast<int64_t>(b) * a.matrix_stride + static_cast<int64_t>(r) * a.row_stride + d0, h);
    store_row<V>(a.enc_packed + (static_cast<int64_t>(b) * a.enc_frames + r) * a.dim + d0, h);
}

template <int V, class E>
void launch_rows(hipStream_t stream, const CifArgs &a) {
    const int32_t slices = (a.dim + kWave * V - 1) / (kWave * V);
    hipLaunchKernelGGL((cif_gather<V, E>), dim3(static_cast<unsigned>(static_cast<int64_t>(a.batch) * a.max_tokens * slices)), dim3(kWave), 0, stream, a, slices);
    if (a.enc_packed && a.enc_frames > 0)
        hipLaunchKernelGGL((cif_pack<V, E>), dim3(static_cast<unsigned>(static_cast<int64_t>(a.batch) * a.enc_frames * slices)), dim3(kWave), 0, stream, a, slices);
}

// ---------------------------------------------------------------------------------------------------------------- timestamps
// energyEnvelope (:277-293): one lane per 10 ms frame adds its 160 squares in order; the workgroup's samples go through LDS 32 per frame
// at a time, so that consecutive lanes load consecutive samples.  Rows of 33: the lanes' reads fall into different banks.
__global__ __launch_bounds__(kEnvBlock) void pf_envelope(const StampArgs a) {
    __shared__ float tile[kEnvBlock * (kEnvChunk + 1)];
    const int tid = threadIdx.x;
    const int32_t b = blockIdx.x / a.env_blocks;
    const int64_t e0 = a.env_off[b], ne = a.env_off[b + 1] - e0, f0 = static_cast<int64_t>(blockIdx.x % a.env_blocks) * kEnvBlock;
    if (f0 >= ne) return;   // the whole workgroup
    const int nf = static_cast<int>(min(static_cast<int64_t>(kEnvBlock), ne - f0));
    const float *x = a.audio + a.audio_off[b] + f0 * kHop;
    float sum = 0.0f;
    for (int k = 0; k < kHop / kEnvChunk; ++k) {
#pragma unroll 4
        for (int j = 0; j < kEnvChunk; ++j) {
            const int e = j * kEnvBlock + tid, fr = e / kEnvChunk, s = e % kEnvChunk;
            if (fr < nf) tile[fr * (kEnvChunk + 1) + s] = x[fr * kHop + k * kEnvChunk + s];
        }
        __syncthreads();
        if (tid < nf) {
#pragma unroll
            for (int s = 0; s < kEnvChunk; ++s) {
                const float v = tile[tid * (kEnvChunk + 1) + s];
                sum += v * v;
            }
        }
        __syncthreads();
    }
    if (tid < nf) a.env_raw[e0 + f0 + tid] = sqrtf(sum / static_cast<float>(kHop));
}

// smooth(_, window: 3) (:304-316): untouched unless there are more than 3 frames
__global__ __launch_bounds__(kEnvBlock) void pf_smooth(const StampArgs a) {
    const int32_t b = blockIdx.x / a.env_blocks;
    const int64_t e0 = a.env_off[b], ne = a.env_off[b + 1] - e0, i = static_cast<int64_t>(blockIdx.x % a.env_blocks) * kEnvBlock + threadIdx.x;
    if (i >= ne) return;
    const float *x = a.env_raw + e0;
    float out = x[i];
    if (ne > 3) {
        const int64_t lo = max(int64_t{0}, i - 1), hi = min(ne - 1, i + 1);
        float sum = 0.0f;
        for (int64_t k = lo; k <= hi; ++k) sum += x[k];
        out = sum / static_cast<float>(hi - lo + 1);
    }
    a.env[e0 + i] = out;
}

// percentile(env, 0.1) (:296-301) by exact rank selection — four passes over the bits of the values, most significant byte first, each
// counting the candidates' next byte — and energyThreshold = max(floor * 2.5, 1e-4) (:196).  One workgroup per utterance.
__device__ inline uint32_t order_key(const float v) {   // ascending as unsigned where the floats ascend
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__global__ __launch_bounds__(256) void pf_floor(const StampArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t pick[2];
    const int tid = threadIdx.x;
    const int32_t b = blockIdx.x;
    const int64_t e0 = a.env_off[b], ne = a.env_off[b + 1] - e0;
    float floor = 0.0f;
    if (ne > 0) {
        const int64_t pos = max(int64_t{0}, min(ne - 1, static_cast<int64_t>(static_cast<float>(ne - 1) * 0.1f)));
        uint32_t prefix = 0, mask = 0, k = static_cast<uint32_t>(pos);
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < ne; i += 256) {
                const uint32_t u = order_key(a.env[e0 + i]);
                if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t before = 0, bin = 0;
                while (bin < 255u && before + hist[bin] <= k) before += hist[bin++];
                pick[0] = bin;
                pick[1] = k - before;
            }
            __syncthreads();
            prefix |= pick[0] << shift;
            mask |= 255u << shift;
            k = pick[1];
            __syncthreads();
        }
        floor = __uint_as_float((prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix);
    }
    if (tid == 0) {
        const float v = floor * 2.5f;
        a.threshold[b] = 1e-4f >= v ? 1e-4f : v;   // Swift's max(x, y): y >= x ? y : x
    }
}

__device__ inline double swift_min(const double x, const double y) { return y < x ? y : x; }
__device__ inline double swift_max(const double x, const double y) { return y >= x ? y : x; }
__device__ inline int64_t to_int(const double x) {   // Int(x) where Swift would not trap; saturated elsewhere
    if (!(x == x)) return 0;
    if (x >= 4.0e18) return int64_t{4000000000000000000};
    if (x <= -4.0e18) return -int64_t{4000000000000000000};
    return static_cast<int64_t>(x);
}

// cifWoHiddenFireIndices (:262-273) on the 3x repeated alphas with the tail appended, each multiplied by `scale` first (1 changes
// nothing); the sequential sum of the values as well (:174).  Every lane walks the same chain.
__device__ inline int32_t fire_scan(const float *alpha, const int32_t T, const float tail, const float scale, const float threshold, int32_t *fires,
                                    const int lane, float &total) {
    const int32_t U = fa::paraformer::kUpsample * T + 1;
    float integrate = 0.0f, sum = 0.0f;
    int32_t count = 0;
    for (int32_t c0 = 0; c0 < U; c0 += kWave) {
        const int32_t u = c0 + lane;
        const float mine = (u < U - 1 ? alpha[u / fa::paraformer::kUpsample] : tail) * scale;
        bool my_fire = false;
        const int steps = min(kWave, U - c0);
        for (int i = 0; i < steps; ++i) {
            const float al = lane_value(mine, i);
            sum += al;
            integrate += al;
            bool fire = false;
            if (integrate >= threshold) {
                fire = true;
                integrate -= 1.0f;
            }
            if (lane == i) my_fire = fire;
        }
        const unsigned long long m = __ballot(my_fire);
        if (my_fire) fires[count + below(m, lane)] = u;
        count += __popcll(m);
    }
    total = sum;
    return count;
}

// One wavefront per utterance: the kept tokens (:146-156 through the keep table), the fires with FunASR's fallback (:162-179), the
// typical spacing (:201-202) and the walk (:203-226) with energySpan (:322-358), whose runs are read off ballots of 64 frames.
__global__ __launch_bounds__(kWave) void pf_walk(const StampArgs a) {
    const int lane = threadIdx.x;
    const int32_t b = blockIdx.x;
    int32_t *kept = a.kept + static_cast<int64_t>(b) * a.max_tokens;
    int32_t *fires = a.fires + static_cast<int64_t>(b) * (fa::paraformer::kUpsample * static_cast<int64_t>(a.frames) + 1);
    float *spacing = a.spacing + static_cast<int64_t>(b) * a.max_tokens;
    Span *spans = a.spans + static_cast<int64_t>(b) * a.max_tokens;
    const int32_t nt = a.token_counts[b];
    int32_t nc = 0;
    for (int32_t i0 = 0; i0 < nt; i0 += kWave) {
        const int32_t i = i0 + lane;
        bool k = false;
        if (i < nt) {
            const int32_t id = a.token_ids[static_cast<int64_t>(b) * a.max_tokens + i];
            k = id >= 0 && id < a.vocab && a.keep[id] != 0;
        }
        const unsigned long long m = __ballot(k);
        if (k) kept[nc + below(m, lane)] = i;
        nc += __popcll(m);
    }
    int32_t n = 0;
    if (nc >= 1) {   // :157
        const float *alpha = a.alphas + static_cast<int64_t>(b) * a.alpha_stride;
        const int32_t T = a.valid[b];
        const float threshold = 1.0f - 1e-4f;   // :139, in fp32
        float total;
        int32_t nf = fire_scan(alpha, T, a.tail, 1.0f, threshold, fires, lane, total);
        if (nf != nc + 1) {   // :172-178
            const float target = static_cast<float>(nc + 1);
            const float scale = target / (1e-6f >= total ? 1e-6f : total);
            nf = fire_scan(alpha, T, a.tail, scale, threshold, fires, lane, total);
        }
        if (nf >= 2) n = min(nc, nf - 1);   // :179, :198
    }
    wave_fence();
    constexpr double kTimeRate = 10.0 * 6.0 / 1000.0 / 3.0;   // :138
    constexpr double kHopSec = 0.01;
    // :201-202: the 0.5 percentile of the n - 1 spacings by rank — an element's rank is the number of smaller ones, earlier equals included
    double typical = static_cast<double>(0.3f);
    const int32_t ns = n - 1;
    if (ns > 0) {
        for (int32_t i = 1 + lane; i < n; i += kWave) spacing[i - 1] = static_cast<float>(static_cast<double>(fires[i]) * kTimeRate - static_cast<double>(fires[i - 1]) * kTimeRate);
        wave_fence();
        const int32_t pos = max(0, min(ns - 1, static_cast<int32_t>(static_cast<float>(ns - 1) * 0.5f)));
        float median = 0.0f;
        for (int32_t e0 = 0; e0 < ns; e0 += kWave) {
            const int32_t e = e0 + lane;
            const float mine = e < ns ? spacing[e] : 0.0f;
            int32_t rank = 0;
            for (int32_t j = 0; j < ns; ++j) {
                const float other = spacing[j];
                rank += (other < mine || (other == mine && j < e)) ? 1 : 0;
            }
            const unsigned long long hit = __ballot(e < ns && rank == pos);
            if (hit) median = lane_value(mine, __ffsll(static_cast<long long>(hit)) - 1);
        }
        typical = static_cast<double>(median);
    }
    const int64_t e0 = a.env_off[b], ne = a.env_off[b + 1] - e0;
    const float *env = a.env + e0;
    const float energy = a.threshold[b];
    const double audio_end = static_cast<double>(a.audio_off[b + 1] - a.audio_off[b]) / 16000.0;
    double cursor = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        const double centroid = static_cast<double>(fires[i]) * kTimeRate;
        const double dur = i < n - 1 ? static_cast<double>(fires[i + 1]) * kTimeRate - centroid : swift_min(audio_end - centroid, swift_max(typical * 2.0, 0.4));
        const double search_end = swift_min(audio_end, centroid + dur * 1.5 + 0.15);
        bool found = false;
        int64_t best_lo = 0, best_hi = 0, best_d = 0;
        if (ne > 0 && search_end > cursor) {
            const int64_t i0 = max(int64_t{0}, to_int(cursor / kHopSec)), i1 = min(ne - 1, max(i0, to_int(search_end / kHopSec)));
            const int64_t ci = to_int(centroid / kHopSec);
            bool open = false;
            int64_t lo = 0;
            const auto close = [&](const int64_t hi) {
                if (hi - lo + 1 >= fa::paraformer::kMinRun) {
                    const int64_t s = lo + hi - 2 * ci, d = s < 0 ? -s : s;
                    if (!found || d < best_d) { found = true; best_d = d; best_lo = lo; best_hi = hi; }
                }
                open = false;
            };
            for (int64_t j0 = i0; j0 <= i1; j0 += kWave) {
                const int64_t j = j0 + lane;
                const unsigned long long m = __ballot(j <= i1 && env[j] > energy);
                const int len = static_cast<int>(min(static_cast<int64_t>(kWave), i1 - j0 + 1));
                int p = 0;
                while (p < len) {
                    if (!open) {
                        const unsigned long long rest = m >> p;
                        if (rest == 0) break;
                        p += __ffsll(static_cast<long long>(rest)) - 1;
                        open = true;
                        lo = j0 + p;
                    }
                    const unsigned long long gaps = ~m >> p;   // m has no bit behind len: a run ends there at the latest
                    if (gaps == 0) break;                      // the run goes on in the next 64 frames
                    p += __ffsll(static_cast<long long>(gaps)) - 1;
                    close(j0 + p - 1);
                }
            }
            if (open) close(i1);
        }
        double s, e;
        if (found) {
            s = static_cast<double>(best_lo) * kHopSec;
            e = static_cast<double>(best_hi) * kHopSec;
        } else {   // :218-223
            s = cursor;
            e = swift_min(audio_end, cursor + swift_max(dur, 0.1));
        }
        cursor = e;
        if (lane == 0) spans[i] = Span{kept[i], 0, s, e};
    }
    if (lane == 0) a.span_counts[b] = n;
}

}  // namespace

namespace fa {
namespace paraformer {

void launch_cif(hipStream_t stream, const CifArgs &a, const int width, const bool fp16) {
    if (a.batch <= 0) return;
    hipLaunchKernelGGL(cif_scan, dim3(static_cast<unsigned>(a.batch)), dim3(kWave), 0, stream, a);
    if (fp16) {
        if (width == 8) launch_rows<8, _Float16>(stream, a);
        else if (width == 4) launch_rows<4, _Float16>(stream, a);
        else launch_rows<1, _Float16>(stream, a);
    } else {
        if (width == 4) launch_rows<4, float>(stream, a);
        else launch_rows<1, float>(stream, a);
    }
}

void launch_stamps(hipStream_t stream, const StampArgs &a) {
    if (a.batch <= 0) return;
    if (a.env_blocks > 0) {
        const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(a.env_blocks) * a.batch));
        hipLaunchKernelGGL(pf_envelope, grid, dim3(kEnvBlock), 0, stream, a);
        hipLaunchKernelGGL(pf_smooth, grid, dim3(kEnvBlock), 0, stream, a);
    }
    hipLaunchKernelGGL(pf_floor, dim3(static_cast<unsigned>(a.batch)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(pf_walk, dim3(static_cast<unsigned>(a.batch)), dim3(kWave), 0, stream, a);
}

}  // namespace paraformer
}  // namespace fa
