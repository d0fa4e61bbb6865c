// lseend.hip — the LS-EEND front end for gfx950 (Diarizer/LS-EEND/LSEENDPreprocessor.swift:249-279,185-202; LSEENDInference.swift:95-119):
// STFT -> power -> Slaney mel -> log -> log10 rescale -> cumulative mean normalisation -> the overlapping [mel_frames, n_mels] windows
// the network reads, with each window's decoder mask and warm-up count, batched over items (recordings, or streams with carried state).
// Three launches per call whatever the batch; every count is a host integer of lseend_core.h, nothing waits for another workgroup.
//
//   mel_tiles  a workgroup (256 threads = 16 groups of 16 lanes) owns 32 consecutive frames of one item.  Their samples go to LDS once,
//              16 bytes per load: the carried audio tail, then the new audio, zeros for the flush.  n_fft = 256 = 16 x 16: a group takes a
//              frame per pass, lane l holds the windowed samples 16 n1 + l, one radix-16 pass, the W256 twiddles, a transpose through the
//              group's LDS region, the second radix-16 pass leaves Z[l + 16 k2]; the frame is real, so bins 0 .. 128 are the registers
//              k2 < 8 of every lane and k2 = 8 of lane 0, with no recombination.  Slaney triangles as bin ranges, log(max(v, floor)),
//              times float(1 / ln 10).  The rows stay in LDS for the per-mel fp64 column sums (ascending frames) and go to the row array.
//              One more workgroup per item carries the samples behind the last frame into the stream's other tail buffer.
//   carry      one wavefront per item, lane = mel bin (two bins beyond 64): a plain ascending loop over the item's tile sums from the
//              carried sum, four loads in flight, leaves every tile's exclusive prefix and the carried-out sum.
//   emit       a workgroup per tile rereads its rows, thread = mel bin forms S_k (tile prefix plus in-tile ascending sum), mu = float(S_k / k),
//              y = x - mu, and the tile's y go straight into every (window, row) slot that takes the frame (lseend_core.h: for_each_slot)
//              and into the stream's mel tail.  One more workgroup per item places the carried rows (zeros for a fresh state: the left
//              context of the first windows) the same way and writes the masks, warm-up counts and row offsets of the item's windows.
//   gather     LSEENDInference.predict's copy: rows [warmup, chunk) x speakers of every window into the dense [frames, speakers] array.
#include "lseend_launch.h"

using namespace fa::lseend;
using namespace fa::melcore;

namespace {

// sample p of the item's sequence: carried tail | new audio | zeros
__device__ __forceinline__ float sample_at(const Item &it, const float *pcm, const int64_t p) {
    if (p < it.tail_in) return it.tail_src ? it.tail_src[p] : 0.0f;
    const int64_t e = p - it.tail_in;
    return e < it.n_new ? pcm[it.pcm_off + e] : 0.0f;
}

// dst[e - e_lo] = src[e] for e in [e_lo, e_hi), 0 <= e_lo, e_hi <= total: whole aligned groups of four inside [0, total) by one 16-byte load
__device__ __forceinline__ void stage(const float *src, const int64_t total, const int64_t e_lo, const int64_t e_hi, float *dst, const bool vec, const int tid) {
    for (int64_t c = (e_lo & ~static_cast<int64_t>(3)) + 4 * tid; c < e_hi; c += 4 * kThreads) {
        float v[4];
        if (vec && c + 3 < total) {
            const float4 t = *reinterpret_cast<const float4 *>(src + c);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = c + k >= e_lo && c + k < e_hi ? src[c + k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k >= e_lo && c + k < e_hi) dst[c + k - e_lo] = v[k];
    }
}

__global__ __launch_bounds__(kThreads, 2) void mel_tiles_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int n_mels = a.g.n_mels, hop = a.g.hop;
    if (static_cast<int>(blockIdx.x) >= a.n_tiles) {   // the item's audio tail: the samples behind its last frame
        const Item it = a.items[blockIdx.x - a.n_tiles];
        if (!it.tail_dst) return;
        const int64_t p0 = static_cast<int64_t>(it.frames) * hop;
        for (int i = tid; i < it.tail_out; i += kThreads) it.tail_dst[i] = sample_at(it, a.pcm, p0 + i);
        return;
    }
    float *samples = smem;
    float *regions = samples + a.stage_alloc;
    float *rows = regions + kGroups * kRegionFloats;
    int32_t *mtab = reinterpret_cast<int32_t *>(rows + kTileFrames * n_mels);
    float *mw = reinterpret_cast<float *>(mtab + 2 * n_mels);

    const Item it = a.items[a.tile_item[blockIdx.x]];
    const int t0 = (static_cast<int>(blockIdx.x) - it.tile0) * kTileFrames;
    const int live = it.frames - t0 < kTileFrames ? it.frames - t0 : kTileFrames;
    const int need = (live - 1) * hop + a.g.n_fft;           // <= stage_alloc; all inside the item's sequence by the definition of `frames`
    const int64_t n0 = static_cast<int64_t>(t0) * hop;

    for (int i = tid; i < 2 * n_mels; i += kThreads) mtab[i] = a.mel_tab[i];
    for (int i = tid; i < a.n_weights; i += kThreads) mw[i] = a.mel_w[i];
    {   // staging: [n0, n0 + need) of the sequence = a piece of the tail, a piece of the new audio, zeros; the three are disjoint
        const int64_t end = n0 + need, new_end = static_cast<int64_t>(it.tail_in) + it.n_new;
        const int64_t tail_hi = end < it.tail_in ? end : it.tail_in;                       // tail piece [n0, tail_hi)
        const int64_t new_lo = n0 > it.tail_in ? n0 : it.tail_in, new_hi = end < new_end ? end : new_end;   // audio piece [new_lo, new_hi)
        for (int i = tid; i < need; i += kThreads) {
            const int64_t p = n0 + i;
            if (p >= new_end || (p < it.tail_in && !it.tail_src)) samples[i] = 0.0f;
        }
        if (it.tail_src && n0 < tail_hi) stage(it.tail_src, (a.g.audio_tail_cap + 3) & ~3, n0, tail_hi, samples, true, tid);
        if (new_lo < new_hi)
            stage(a.pcm, a.pcm_total, it.pcm_off + new_lo - it.tail_in, it.pcm_off + new_hi - it.tail_in, samples + (new_lo - n0), a.vec != 0, tid);
    }
    const int l = tid & (kGroup - 1), grp = tid >> 4;
    float wz[16], t1r[15], t1i[15];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) wz[n1] = a.windowz[16 * n1 + l];
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) { const float2 w = a.tw256[(l * k1) & 255]; t1r[k1 - 1] = w.x; t1i[k1 - 1] = w.y; }
    __syncthreads();

    float *Rg = static_cast<float *>(__builtin_assume_aligned(regions + grp * kRegionFloats, 8));
#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int f = pass * kGroups + grp;
        if (f >= live) continue;   // uniform inside the 16-lane group: everything below stays inside it
        const float *fs = samples + f * hop;
        Lane v;
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) { v.re[n1] = fs[16 * n1 + l] * wz[n1]; v.im[n1] = 0.0f; }
        fft16(v);                  // v[k1] = sum_n1 x[16 n1 + l] W16^(n1 k1)
        Rg[2 * l] = v.re[0];
        Rg[2 * l + 1] = v.im[0];
#pragma unroll
        for (int k1 = 1; k1 < 16; ++k1) {
            cmul(v.re[k1], v.im[k1], t1r[k1 - 1], t1i[k1 - 1]);
            Rg[2 * (k1 * kEStride + l)] = v.re[k1];
            Rg[2 * (k1 * kEStride + l) + 1] = v.im[k1];
        }
        phase_b1(l, Rg, v);        // v[k2] = Z[l + 16 k2]
        // LDS operations of a wavefront complete in program order: the power bins may overwrite the transpose buffer
#pragma unroll
        for (int j = 0; j < 8; ++j) Rg[l + 16 * j] = v.re[j] * v.re[j] + v.im[j] * v.im[j];
        if (l == 0) Rg[128] = v.re[8] * v.re[8] + v.im[8] * v.im[8];
        float *out = a.rows + (it.row0 + t0 + f) * n_mels;
        for (int m = l; m < n_mels; m += kGroup) {   // lane l owns the mels l, l + 16, ...
            const int packed = mtab[2 * m];
            const float *P = Rg + (packed & 0xffff);
            const float *wgt = mw + mtab[2 * m + 1];
            const int cnt = packed >> 16;
            float acc = 0.0f;
            for (int j = 0; j < cnt; ++j) acc += wgt[j] * P[j];
            const float val = logf(fmaxf(acc, a.log_floor)) * a.log10_scale;   // :78-79 clamped floor, :259-261 the log10 rescale
            rows[f * n_mels + m] = val;
            out[m] = val;
        }
    }
    __syncthreads();
    if (tid < n_mels) {   // the tile's column sums: fp64, ascending frames, from 0.0 (lseend_core.h)
        double s = 0.0;
        for (int f = 0; f < live; ++f) s += static_cast<double>(rows[f * n_mels + tid]);
        a.tile_sums[static_cast<int64_t>(blockIdx.x) * n_mels + tid] = s;
    }
}

__global__ __launch_bounds__(64) void carry_kernel(const Args a) {
    const Item it = a.items[blockIdx.x];
    const int n = a.g.n_mels, m0 = threadIdx.x, m1 = threadIdx.x + 64;
    const bool h0 = m0 < n, h1 = m1 < n;
    double run0 = h0 && it.sum_src ? it.sum_src[m0] : 0.0, run1 = h1 && it.sum_src ? it.sum_src[m1] : 0.0;
    const double *ts = a.tile_sums + static_cast<int64_t>(it.tile0) * n;
    double *tp = a.tile_prefix + static_cast<int64_t>(it.tile0) * n;
    for (int t = 0; t < it.tiles; t += 4) {
        double x0[4], x1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // the four loads leave before the first addition needs one
            const bool in = t + u < it.tiles;
            x0[u] = h0 && in ? ts[static_cast<int64_t>(t + u) * n + m0] : 0.0;
            x1[u] = h1 && in ? ts[static_cast<int64_t>(t + u) * n + m1] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (t + u >= it.tiles) break;
            if (h0) { tp[static_cast<int64_t>(t + u) * n + m0] = run0; run0 += x0[u]; }
            if (h1) { tp[static_cast<int64_t>(t + u) * n + m1] = run1; run1 += x1[u]; }
        }
    }
    if (it.sum_dst) {
        if (h0) it.sum_dst[m0] = run0;
        if (h1) it.sum_dst[m1] = run1;
    }
}

// row q of the item's mel queue, value y of mel m: into every window of this call that holds it, and into the carried rows
__device__ __forceinline__ void place(const Args &a, const Item &it, const int64_t q, const int m, const float y) {
    const int n = a.g.n_mels;
    for_each_slot(a.g, q, it.windows0, it.windows1, [&](const int64_t c, const int row) {
        a.windows[((it.win0 + (c - it.windows0)) * a.g.mel_frames + row) * n + m] = y;
    });
    const int64_t behind = q - it.windows1 * a.g.chunk_mels;
    if (it.mel_dst && behind >= 0) it.mel_dst[behind * n + m] = y;
}

__global__ __launch_bounds__(kThreads) void emit_kernel(const Args a) {
    __shared__ float rows[kTileFrames * kMaxMels];
    const int tid = threadIdx.x, n = a.g.n_mels;
    if (static_cast<int>(blockIdx.x) >= a.n_tiles) {   // the item's carried rows, and what describes its windows
        const Item it = a.items[blockIdx.x - a.n_tiles];
        for (int i = tid; i < it.mel_in * n; i += kThreads) {
            const int r = i / n;
            place(a, it, it.windows0 * a.g.chunk_mels + r, i - r * n, it.mel_src ? it.mel_src[i] : 0.0f);
        }
        const int nw = static_cast<int>(it.windows1 - it.windows0), chunk = a.g.chunk;
        if (a.masks)
            for (int i = tid; i < nw * chunk; i += kThreads) {   // decoderMask[end - chunk, end): 0 below conv_delay, 1 from it on (:65-67,:193-197)
                const int k = i / chunk, j = i - k * chunk;
                a.masks[(it.win0 + k) * chunk + j] = mask_end_of(a.g, it.windows0 + k + 1) - chunk + j >= a.g.conv_delay ? 1.0f : 0.0f;
            }
        for (int k = tid; k < nw; k += kThreads) {
            if (a.warmups) a.warmups[it.win0 + k] = warmup_of(a.g, it.windows0 + k);
            if (a.out_rows) a.out_rows[it.win0 + k] = it.out_row0 + rows_before(a.g, it.windows0 + k) - rows_before(a.g, it.windows0);
        }
        return;
    }
    const Item it = a.items[a.tile_item[blockIdx.x]];
    const int t0 = (static_cast<int>(blockIdx.x) - it.tile0) * kTileFrames;
    const int live = it.frames - t0 < kTileFrames ? it.frames - t0 : kTileFrames;
    const float *src = a.rows + (it.row0 + t0) * n;
    for (int i = tid; i < live * n; i += kThreads) rows[i] = src[i];
    __syncthreads();
    if (tid < n) {   // S_k = tile prefix + the tile's frames up to k, one by one; mu = float(S_k / k); y = x - mu in fp32
        double s = a.tile_prefix[static_cast<int64_t>(blockIdx.x) * n + tid];
        const int64_t k0 = it.frames0 + t0;
        for (int f = 0; f < live; ++f) {
            const float x = rows[f * n + tid];
            s += static_cast<double>(x);
            const float mu = static_cast<float>(s / static_cast<double>(k0 + f + 1));
            rows[f * n + tid] = x - mu;
        }
    }
    __syncthreads();
    const int64_t q0 = a.g.context + it.frames0 + t0;
    for (int i = tid; i < live * n; i += kThreads) {
        const int f = i / n;
        place(a, it, q0 + f, i - f * n, rows[i]);
    }
}

__global__ __launch_bounds__(kThreads) void gather_kernel(const GatherArgs a) {
    const int w = blockIdx.x;
    int wu = a.warmups[w];
    wu = wu < 0 ? 0 : (wu > a.chunk ? a.chunk : wu);
    const int64_t r0 = a.out_rows[w];
    if (r0 < 0 || r0 + (a.chunk - wu) > a.out_capacity) return;   // never past the caller's array
    const float *src = a.probs + w * a.window_stride + wu * a.row_stride;
    float *dst = a.out + r0 * a.speakers;
    for (int i = threadIdx.x; i < (a.chunk - wu) * a.speakers; i += kThreads) {
        const int r = i / a.speakers;
        dst[i] = src[r * a.row_stride + (i - r * a.speakers)];
    }
}

}  // namespace

namespace fa {
namespace lseend {

void run(const Args &a, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(a.n_tiles + a.n_items));
    hipLaunchKernelGGL(mel_tiles_kernel, grid, dim3(kThreads), lds_bytes(a), stream, a);
    hipLaunchKernelGGL(carry_kernel, dim3(static_cast<unsigned>(a.n_items)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(emit_kernel, grid, dim3(kThreads), 0, stream, a);
}

void gather(const GatherArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(gather_kernel, dim3(static_cast<unsigned>(a.windows)), dim3(kThreads), 0, stream, a);
}

}  // namespace lseend
}  // namespace fa
