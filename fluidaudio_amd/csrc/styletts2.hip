// styletts2.hip — the host arithmetic of one StyleTTS2 (LibriTTS, iteration_3) synthesis for gfx950, batched over (reference clip, text)
// pairs, on slabs the networks read in place (TTS/StyleTTS2/Pipeline/Preprocess/StyleTTS2MelExtractor.swift:77-141,
// Synthesize/StyleTTS2Synthesizer.swift:105-132,163-175,246-259, StyleTTS2GlueOps.swift:23-161).  Every count is a host integer of
// styletts2_core.h; no kernel waits for another workgroup, none uses an atomic.
//
//   mel        a workgroup (4 wavefronts) owns 16 consecutive frames of one item, so that every mel row leaves the tile as 64 contiguous
//              bytes.  The window is a Hann of `win` = 1200 samples centred in n_fft = 2048: only the (16 - 1) hop + win samples under it
//              are staged in LDS, once, with 16-byte loads, the reflect padding resolved there with the reference's clamps
//              (min(pad - i, n - 1), max(n - 2 - i, 0); an empty clip is zeros).  A wavefront takes a frame.  The 2048-point real
//              transform runs as a 1024-point complex one on z[n] = xw[2n] + i xw[2n + 1], 16 points per lane: lane l holds
//              z[64 n1 + l] (a lane multiplies only the samples under the window, the others are zeros), one radix-16 pass over n1
//              (mel_core.h: fft16), W1024^(l k1), a transpose through the wavefront's LDS region (rows of 68 complex), lane (k1, q)
//              gathers the points l = 4 m + q of row k1, the second radix-16 pass over m, W64^(q k2a), the radix-4 pass over q as two
//              lane exchanges (xor 32, xor 16): the arrangement of luxtts.hip.  Z goes back into the region (quarters 16 complex apart,
//              so the four lane groups of a store fall on different banks), and lane l recombines the bins k = l + 64 i with their
//              mirrors: X[k] = (Z[k] + conj Z[1024 - k]) / 2 - i W2048^k (Z[k] - conj Z[1024 - k]) / 2, power re^2 + im^2, 1025 bins
//              (bin 1024 by lane 0).  HTK triangles built for the 16 kHz filter rate cover all 1025 bins as contiguous ranges;
//              (log(acc + eps) - mean) / std goes into an LDS tile [n_mels][16 + 1] and from there out along f with 16-byte stores:
//              there is no [T, 80] intermediate.  Columns behind the item's frames, and every column of a refused item, are zeros.
//              One float32 transform per frame: the reference clip's mel is a power mel under log(. + 1e-5), which hides the weak
//              bands' share of the strong bands' rounding error that luxtts.hip:7-23 had to work round for its magnitude mel under
//              log(max(., 1e-7)); measured figures stand in DESIGN.md.
//   inputs     token ids zero-padded, attention mask, and the seeded Gaussian stack: one lane per element, the SplitMix64 stream as a
//              counter (luxtts_core.h: gaussian_at), draws 0..255 into noise_init and the rest into noises_aux[s, b, :].
//   blend      ref / s from s_pred and ref_s in the order of styletts2_core.h.
//   durations  one workgroup per item, a lane per token: the sigmoid sum in the order of styletts2_core.h, round, clamp, the exclusive scan
//              of block_scan.h into starts and total_frames, the status of an item that passes the frame capacity.
//   align      a workgroup owns 64 consecutive frames of one item and 64 channels of one of the two maps.  tok(f') per frame by binary
//              search in the item's start table staged in LDS; the 64 frames touch one run of at most 64 tokens.  en: the run's rows of
//              the token-major d come in with 16-byte loads along c into an LDS tile (rows of 68 floats) and go out along f; asr: lanes
//              along f read the channel-major t_en[c, tok] directly.  16-byte stores where the address allows; frames behind
//              total_frames up to the stride are zeros.  The causal shift is f' = max(f - 1, 0).
//   finish     the rows without their last min(50, len) samples, stored ragged.
#include "block_scan.h"
#include "styletts2_launch.h"

using namespace fa::styletts2;
using fa::melcore::cmul;
using fa::melcore::fft16;
using fa::melcore::Lane;

namespace {

__device__ __forceinline__ int z_slot(const int k) { return k + ((k >> 8) << 4); }   // where Z[k] lies in the region, in complex elements

__global__ __launch_bounds__(kMelThreads) void mel_kernel(const MelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, b = blockIdx.y, n_mels = a.n_mels, hop = a.hop, win = a.win, lead = a.lead;
    const Item it = a.items[b];
    const int t0 = static_cast<int>(blockIdx.x) * kTileFrames;
    int live = it.status == kOk ? it.ref_frames - t0 : 0;
    live = live < 0 ? 0 : (live > kTileFrames ? kTileFrames : live);
    const int stage_floats = (kTileFrames - 1) * hop + win;
    float *samples = smem;
    float *regions = samples + stage_floats;
    int32_t *mtab = reinterpret_cast<int32_t *>(regions + kMelWaves * kRegionFloats);
    float *tile = reinterpret_cast<float *>(mtab + 2 * n_mels);
    if (live > 0) {
        for (int i = tid; i < 2 * n_mels; i += kMelThreads) mtab[i] = a.mel_tab[i];
        // staging: position p of the reflect-padded clip, p = t0 hop + lead + i; every frame below ref_frames ends inside n + n_fft
        const int64_t off = a.offsets[b], n = it.samples, p0 = static_cast<int64_t>(t0) * hop + lead;
        const float *x = a.pcm + off;
        const bool vec = a.vec && (off & 3) == 0;
        const int need = (live - 1) * hop + win, pad = kHalf;
        for (int i = 4 * tid; i < need; i += 4 * kMelThreads) {
            const int64_t p = p0 + i;
            float v[4];
            if (vec && p >= pad && p + 3 < pad + n) {
                const float4 t = *reinterpret_cast<const float4 *>(x + (p - pad));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {   // MelExtractor :226-250
                    const int64_t q = p + c;
                    int64_t idx = q < pad ? (pad - q < n - 1 ? pad - q : n - 1) : (q < pad + n ? q - pad : n - 2 - (q - pad - n));
                    idx = idx < 0 ? 0 : idx;
                    v[c] = i + c < need && n > 0 ? x[idx] : 0.0f;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i + c < need) samples[i + c] = v[c];
        }
    }
    __syncthreads();
    const int l = tid & 63, w = tid >> 6, k1 = l & 15, q = l >> 4;
    const int kb = ((q & 1) << 1) | (q >> 1);   // the output quarter this lane ends with: q = 0, 1, 2, 3 -> Z_0, Z_2, Z_1, Z_3
    float *R = static_cast<float *>(__builtin_assume_aligned(regions + w * kRegionFloats, 8));
#pragma unroll 1
    for (int f = w; f < live; f += kMelWaves) {   // uniform in the wavefront; nothing below leaves its own region
        const float *fs = samples + f * hop;      // fs[j - lead] is sample j of the frame
        Lane v;
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            const int jj = 128 * n1 + 2 * l - lead;   // lead and win are even: a pair lies under the window or outside
            v.re[n1] = 0.0f; v.im[n1] = 0.0f;
            if (jj >= 0 && jj < win) {
                const float2 s = *reinterpret_cast<const float2 *>(fs + jj), h = *reinterpret_cast<const float2 *>(a.window + jj);
                v.re[n1] = s.x * h.x; v.im[n1] = s.y * h.y;
            }
        }
        fft16(v);   // v[k1] = sum_n1 z[64 n1 + l] W16^(n1 k1)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k) { const float2 t = a.tw2048[2 * ((l * k) & (kHalf - 1))]; cmul(v.re[k], v.im[k], t.x, t.y); }
            *reinterpret_cast<float2 *>(R + 2 * (k * kRowStride + l)) = make_float2(v.re[k], v.im[k]);
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const float2 t = *reinterpret_cast<const float2 *>(R + 2 * (k1 * kRowStride + 4 * m + q));
            v.re[m] = t.x; v.im[m] = t.y;
        }
        __builtin_amdgcn_wave_barrier();   // LDS operations of a wavefront complete in program order: Z may overwrite the buffer
        fft16(v);   // v[k2a] = sum_m B[k1][4 m + q] W16^(m k2a)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j) { const float2 t = a.tw2048[32 * q * j]; cmul(v.re[j], v.im[j], t.x, t.y); }   // W64^(q k2a)
            // radix-4 over q: y_q of the lanes l, l ^ 16, l ^ 32, l ^ 48
            const float pr = __shfl_xor(v.re[j], 32), pi = __shfl_xor(v.im[j], 32);
            const float tr = q < 2 ? v.re[j] + pr : pr - v.re[j], ti = q < 2 ? v.im[j] + pi : pi - v.im[j];   // y0 + y2, y1 + y3, y0 - y2, y1 - y3
            const float ur = __shfl_xor(tr, 16), ui = __shfl_xor(ti, 16);
            float zr, zi;
            if (q == 0) { zr = tr + ur; zi = ti + ui; }
            else if (q == 1) { zr = ur - tr; zi = ui - ti; }
            else if (q == 2) { zr = tr + ui; zi = ti - ur; }   // t - i u
            else { zr = ur - ti; zi = ui + tr; }               // u + i t
            *reinterpret_cast<float2 *>(R + 2 * z_slot(k1 + 16 * j + 256 * kb)) = make_float2(zr, zi);   // Z[k1 + 16 k2a + 256 k2b]
        }
        __builtin_amdgcn_wave_barrier();
        float pw[17];
#pragma unroll
        for (int i = 0; i < 16; ++i) {   // MelExtractor :118-123 on X[k] = E[k] + W2048^k O[k], E and O the transforms of the even and the odd samples
            const int k = l + 64 * i;
            const float2 za = *reinterpret_cast<const float2 *>(R + 2 * z_slot(k)), zb = *reinterpret_cast<const float2 *>(R + 2 * z_slot((kHalf - k) & (kHalf - 1)));
            const float sr = za.x + zb.x, si = za.y - zb.y;     // 2 E = Z[k] + conj Z[N - k]
            float orr = za.y + zb.y, oi = zb.x - za.x;          // 2 O = -i (Z[k] - conj Z[N - k])
            const float2 t = a.tw2048[k];
            cmul(orr, oi, t.x, t.y);
            const float xr = sr + orr, xi = si + oi;
            pw[i] = 0.25f * (xr * xr + xi * xi);
        }
        {   // bin 1024: E[0] - O[0]
            const float2 z0 = *reinterpret_cast<const float2 *>(R);
            const float xr = z0.x - z0.y;
            pw[16] = xr * xr;
        }
        __builtin_amdgcn_wave_barrier();   // every lane has read its Z: the power bins take the buffer
#pragma unroll
        for (int i = 0; i < 16; ++i) R[l + 64 * i] = pw[i];
        if (l == 0) R[kHalf] = pw[16];
        __builtin_amdgcn_wave_barrier();
        for (int m = l; m < n_mels; m += 64) {
            const int packed = mtab[2 * m], cnt = packed >> 16;
            const float *bins = R + (packed & 0xffff), *wgt = a.mel_w + mtab[2 * m + 1];
            float acc = 0.0f;
            for (int j = 0; j < cnt; ++j) acc += wgt[j] * bins[j];
            // :136; the logarithm in fp64, rounded once: logf came out 2 float32 spacings off at the floor value log(eps), which a silent
            // clip has in every cell, and 80 logarithms a frame cost nothing beside the transform
            const float lg = static_cast<float>(log(static_cast<double>(acc + a.log_eps)));
            tile[m * kTileStride + f] = (lg - a.log_mean) / a.log_std;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    float *dst = a.mel + static_cast<int64_t>(b) * n_mels * a.stride + t0;
    for (int t = tid; t < n_mels * (kTileFrames / 4); t += kMelThreads) {
        const int m = t / (kTileFrames / 4), c0 = 4 * (t - m * (kTileFrames / 4));
        if (t0 + c0 >= a.stride) continue;   // the stride is a multiple of 4
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = c0 + c < live ? tile[m * kTileStride + c0 + c] : 0.0f;
        *reinterpret_cast<float4 *>(dst + static_cast<int64_t>(m) * a.stride + c0) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

__global__ __launch_bounds__(kThreads) void inputs_kernel(const InputArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x, part = blockIdx.x;
    const Item it = a.items[b];
    const float g = it.status == kOk ? gaussian_at(a.seeds[b], static_cast<uint64_t>(part) * kStyle + tid) : 0.0f;   // Synthesizer :248-259: one stream
    if (part == 0) a.s.noise_init[static_cast<int64_t>(b) * kStyle + tid] = g;
    else a.s.noises_aux[(static_cast<int64_t>(part - 1) * a.batch + b) * kStyle + tid] = g;
    if (part) return;
    const int32_t *ids = a.token_ids + a.token_offsets[b];
    for (int i = tid; i < a.token_stride; i += kThreads) {   // :166-174
        a.s.tokens[static_cast<int64_t>(b) * a.token_stride + i] = i < it.tokens ? ids[i] : 0;
        a.s.attention_mask[static_cast<int64_t>(b) * a.token_stride + i] = i < it.tokens ? 1 : 0;
    }
}

__global__ __launch_bounds__(kStyle / 2) void blend_kernel(const BlendArgs a) {
    const int b = blockIdx.x, i = threadIdx.x;
    const float *sp = a.s_pred + b * a.s_pred_stride, *rs = a.ref_s + b * a.ref_s_stride;
    a.s.ref[b * (kStyle / 2) + i] = blend_of(a.alphas[b], sp[i], rs[i]);
    a.s.s[b * (kStyle / 2) + i] = blend_of(a.betas[b], sp[kStyle / 2 + i], rs[kStyle / 2 + i]);
}

__global__ __launch_bounds__(fa::scan::kThreads) void durations_kernel(const DurationArgs a) {
    const int b = blockIdx.x, t = threadIdx.x;
    const Item it = a.items[b];
    int dur = 0;
    if (t < it.tokens) {   // GlueOps :36-44
        const float *x = a.logits + b * a.item_stride + t * a.token_stride;
        float sum = 0.0f;
        for (int c = 0; c < a.channels; ++c) sum += sigmoid_term(x[c * a.channel_stride]);
        dur = round_duration(sum);
    }
    int total;
    const int start = fa::scan::block_exclusive(dur, &total);
    if (t < a.token_stride_out) {
        a.s.durations[static_cast<int64_t>(b) * a.token_stride_out + t] = dur;
        a.s.starts[static_cast<int64_t>(b) * a.token_stride_out + t] = t < it.tokens ? start : total;
    }
    if (t == 0) {
        a.s.total_frames[b] = total;
        a.s.status[b] = it.status != kOk ? it.status : (total > a.max_frames ? kTooManyFrames : kOk);
    }
}

__global__ __launch_bounds__(kThreads) void align_kernel(const AlignArgs a) {
    __shared__ int32_t starts[kMaxTokens];
    __shared__ int32_t tokf[kAlignFrames];
    __shared__ __attribute__((aligned(16))) float tile[kAlignFrames * kAlignStride];
    const int tid = threadIdx.x, b = blockIdx.z, y = blockIdx.y;
    const Item it = a.items[b];
    const int total = a.s.status[b] == kOk ? a.s.total_frames[b] : 0, n = it.tokens;
    const int f0 = static_cast<int>(blockIdx.x) * kAlignFrames;
    int nf = total - f0;
    nf = nf < 0 ? 0 : (nf > kAlignFrames ? kAlignFrames : nf);
    const bool is_en = y < a.d_slabs;
    const int c0 = (is_en ? y : y - a.d_slabs) * kAlignChannels, C = is_en ? a.d_channels : a.asr_channels;
    const int nc = C - c0 < kAlignChannels ? C - c0 : kAlignChannels;
    const float *t_en = a.t_en + b * a.t_item_stride + static_cast<int64_t>(c0) * a.t_row_stride;
    int tok_lo = 0;
    if (nf > 0) {   // uniform in the workgroup
        for (int i = tid; i < n; i += kThreads) starts[i] = a.s.starts[static_cast<int64_t>(b) * a.token_stride + i];
        __syncthreads();
        if (tid < kAlignFrames) {   // the token of frame f' (Synthesizer :121-134 fused): the last one whose start is <= f'
            int fp = f0 + tid - (a.shift ? 1 : 0);
            fp = fp < 0 ? 0 : (fp > total - 1 ? total - 1 : fp);
            int lo = 0, hi = n - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (starts[mid] <= fp) lo = mid; else hi = mid - 1;
            }
            tokf[tid] = lo;
        }
        __syncthreads();
        tok_lo = tokf[0];
        if (is_en) {   // every duration is >= 1: nf frames touch at most nf <= 64 consecutive tokens
            const int ntok = tokf[nf - 1] - tok_lo + 1;
            const float *d = a.d + b * a.d_item_stride + static_cast<int64_t>(tok_lo) * a.d_row_stride + c0;
            for (int i = tid; i < ntok * (kAlignChannels / 4); i += kThreads) {
                const int tk = i / (kAlignChannels / 4), c4 = 4 * (i - tk * (kAlignChannels / 4));
                if (c4 >= nc) continue;   // the channel counts are multiples of 4
                const float *src = d + static_cast<int64_t>(tk) * a.d_row_stride + c4;
                *reinterpret_cast<float4 *>(tile + tk * kAlignStride + c4) = a.vec_d ? *reinterpret_cast<const float4 *>(src) : make_float4(src[0], src[1], src[2], src[3]);
            }
            __syncthreads();
        }
    }
    float *out = (is_en ? a.en : a.asr) + (static_cast<int64_t>(b) * C + c0) * a.frame_stride + f0;
    for (int i = tid; i < kAlignChannels * (kAlignFrames / 4); i += kThreads) {
        const int g = i & (kAlignFrames / 4 - 1), c = i >> 4, fl = 4 * g;
        if (c >= nc || f0 + fl >= a.frame_stride) continue;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0.0f;
            if (fl + j < nf) { const int tk = tokf[fl + j]; v[j] = is_en ? tile[(tk - tok_lo) * kAlignStride + c] : t_en[static_cast<int64_t>(c) * a.t_row_stride + tk]; }
        }
        float *o = out + static_cast<int64_t>(c) * a.frame_stride + fl;
        if (a.vec_out) { *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]); continue; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (f0 + fl + j < a.frame_stride) o[j] = v[j];
    }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const FinishArgs a) {
    const int b = blockIdx.y;
    const int64_t at = a.ranges[b], cnt = a.ranges[b + 1] - at, so = b * a.row_stride;
    const int64_t i = 4 * (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x);
    if (i >= cnt) return;
    const float *src = a.audio + so + i;
    float *dst = a.out + at + i;
    if (a.vec && ((so | at) & 3) == 0 && i + 3 < cnt) { *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src); return; }
    for (int c = 0; c < 4 && i + c < cnt; ++c) dst[c] = src[c];
}

unsigned blocks_for(const int64_t items, const int per) { return static_cast<unsigned>((items + per - 1) / per); }

}  // namespace

namespace fa {
namespace styletts2 {

void run_reference_mel(const MelArgs &a, const int batch, hipStream_t stream) {
    const dim3 grid(blocks_for(a.stride, kTileFrames), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(mel_kernel, grid, dim3(kMelThreads), mel_lds_bytes(a), stream, a);
}

void run_inputs(const InputArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(inputs_kernel, dim3(static_cast<unsigned>(a.aux_steps + 1), static_cast<unsigned>(a.batch)), dim3(kThreads), 0, stream, a);
}

void run_blend(const BlendArgs &a, const int batch, hipStream_t stream) {
    hipLaunchKernelGGL(blend_kernel, dim3(static_cast<unsigned>(batch)), dim3(kStyle / 2), 0, stream, a);
}

void run_durations(const DurationArgs &a, const int batch, hipStream_t stream) {
    hipLaunchKernelGGL(durations_kernel, dim3(static_cast<unsigned>(batch)), dim3(fa::scan::kThreads), 0, stream, a);
}

void run_align(const AlignArgs &a, const int batch, hipStream_t stream) {
    const dim3 grid(blocks_for(a.frame_stride, kAlignFrames), static_cast<unsigned>(a.d_slabs + blocks_for(a.asr_channels, kAlignChannels)), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(align_kernel, grid, dim3(kThreads), 0, stream, a);
}

void run_finish(const FinishArgs &a, const int batch, const int64_t longest, hipStream_t stream) {
    if (longest < 1) return;
    hipLaunchKernelGGL(finish_kernel, dim3(blocks_for((longest + 3) / 4, kThreads), static_cast<unsigned>(batch)), dim3(kThreads), 0, stream, a);
}

}  // namespace styletts2
}  // namespace fa
