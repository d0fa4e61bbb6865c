// luxtts.hip — the host arithmetic of one LuxTTS (ZipVoice-Distill) synthesis for gfx950, batched over utterances, on slabs the networks
// read in place (TTS/LuxTts/LuxTtsSynthesizer.swift:70-299, LuxTtsMelExtractor.swift:52-132, LuxTtsSolver.swift).  Every count is a host
// integer of luxtts_core.h; no kernel waits for another workgroup, none uses an atomic.
//
//   loudness   one workgroup per item: the mean square of the capped prompt in the order luxtts_core.h defines (16-byte loads, lane-strided
//              fmaf, butterfly, wavefronts in order), then rms, gain and the silent-prompt status into the item's record.
//   mel        a workgroup (4 wavefronts) owns 8 consecutive frames of one item and stages their 7 x 256 + 1024 samples in LDS once, the
//              reflect padding (clamped for n <= 512) resolved per sample and the gain multiplied in.  A wavefront takes a frame, 16 points
//              per lane, in two transforms.  Speech has 80 dB and more between its low and its high bands inside a frame, and a float32
//              FFT leaves every bin the rounding error of the strongest one (measured: 1.0e-4 on the reference's fixture, where a
//              float32 matrix DFT has 1.8e-5).  So the bins below 256 come from the transform of the windowed frame xw, and the bins
//              from 256 on from the transform of its circular first difference y[j] = xw[j] - xw[j - 1], which takes the strong low
//              bands down before the first butterfly: Y[k] = X[k] (1 - W^k), |X[k]| = |Y[k]| / (2 sin(pi k / 1024)) from a table; at
//              256 that factor is sqrt(2), so white input loses nothing.  Lane l holds z[64 n1 + l], one radix-16 pass
//              over n1 (mel_core.h: fft16), W1024^(l k1), a
//              transpose through the wavefront's LDS region (rows of 68 complex: the gather below touches every bank pair twice, the
//              least 64 lanes of 8 bytes can), lane (k1, q) gathers the points l = 4 m + q of row k1, the second radix-16 pass over m,
//              W64^(q k2a), and the radix-4 pass over q as two lane exchanges (xor 32, xor 16); the frame is real, so the lanes that end
//              with the quarters 0 and 1 (and one lane with bin 512) hold all the bins and leave their magnitudes behind the buffer.  HTK
//              triangles as contiguous bin ranges, log(max(v, floor)) * feat_scale, stored straight into speech_condition[b, frame, :];
//              rows behind prompt_frames are zeros.  (prompt_frames = (n + hop / 2) / hop never exceeds the STFT's 1 + n / hop frames,
//              so the lhotse tail of LuxTtsMelExtractor.swift:126-130 has nothing to repeat.  Two frames as the real and imaginary part
//              of one transform were tried and dropped: a quiet frame beside a loud one takes the loud one's rounding error.)
//   inputs     token ids, both masks and the seeded Gaussian start: one lane per element, the SplitMix64 stream as a counter, fp64.
//   text       frame f copies embedding row f / avg (the pad slot for the remainder frames) from the stride-padded encoder output.
//   step       one anchor-Euler update of the active rows of x on the stride-padded velocity, in the order of luxtts_core.h.
//   vocoder    x[b, prompt_frames + f, m] / feat_scale -> mel[k, m, f] through an LDS tile of 64 frames (rows of 65 floats), the log floor
//              behind gen_frames, 16-byte stores along f wherever the row's address allows.
//   finish     clip, loudness restore, ragged store.
#include "luxtts_launch.h"

using namespace fa::luxtts;
using fa::melcore::cmul;
using fa::melcore::fft16;
using fa::melcore::Lane;

namespace {

__global__ __launch_bounds__(kRmsThreads) void loudness_kernel(const MelArgs a) {
    __shared__ float wsum[kRmsThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const Item it = a.items[b];
    if (it.status != kOk) {
        if (tid == 0) a.s.records[b] = Record{0.0f, 0.0f, 1.0f, it.status};
        return;
    }
    const int64_t off = a.offsets[b], n = it.samples;
    const float *x = a.pcm + off;
    const bool vec = a.vec && (off & 3) == 0;
    float acc = 0.0f;
    for (int64_t g = tid; 4 * g < n; g += kRmsThreads) {   // sample e belongs to accumulator (e / 4) % kRmsThreads, ascending
        if (vec && 4 * g + 3 < n) {
            const float4 t = *reinterpret_cast<const float4 *>(x + 4 * g);
            acc = fmaf(t.x, t.x, acc); acc = fmaf(t.y, t.y, acc); acc = fmaf(t.z, t.z, acc); acc = fmaf(t.w, t.w, acc);
        } else {
            for (int c = 0; c < 4 && 4 * g + c < n; ++c) { const float v = x[4 * g + c]; acc = fmaf(v, v, acc); }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float total = wsum[0];
        for (int w = 1; w < kRmsThreads / 64; ++w) total += wsum[w];
        const Loudness r = loudness_of(total / static_cast<float>(n), a.target_rms);
        a.s.records[b] = Record{r.mean_square, r.rms, r.gain, r.status};
    }
}

// xw[j] - xw[j - 1] of the windowed frame, each product taken with its rounding error (p + e = x w exactly), so the small difference of two
// large neighbours keeps its low bits.  No contraction here: p has to be the rounded product e is the error of.
__device__ __forceinline__ float windowed_difference(const float x, const float w, const float xm, const float wm) {
#pragma clang fp contract(off)
    const float p = x * w, pm = xm * wm;
    const float e = fmaf(x, w, -p), em = fmaf(xm, wm, -pm);
    return (p - pm) + (e - em);
}

__global__ __launch_bounds__(kMelThreads) void mel_kernel(const MelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, b = blockIdx.y, n_mels = a.n_mels, hop = a.hop;
    const Item it = a.items[b];
    const Record rec = a.s.records[b];
    const int t0 = static_cast<int>(blockIdx.x) * kTileFrames;
    int live = it.status == kOk && rec.status == kOk ? it.prompt_frames - t0 : 0;
    live = live < 0 ? 0 : (live > kTileFrames ? kTileFrames : live);
    float *dst = a.s.speech_condition + (static_cast<int64_t>(b) * a.max_frames + t0) * n_mels;
    {   // rows behind prompt_frames, and every row of a refused or silent item
        float4 *z = reinterpret_cast<float4 *>(dst);
        for (int i = live * (n_mels / 4) + tid; i < kTileFrames * (n_mels / 4); i += kMelThreads) z[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (live == 0) return;
    const int stage_floats = (kTileFrames - 1) * hop + kNfft;
    float *samples = smem;
    float *regions = samples + stage_floats;
    int32_t *mtab = reinterpret_cast<int32_t *>(regions + kMelWaves * kRegionFloats);
    float *mw = reinterpret_cast<float *>(mtab + 2 * n_mels);
    for (int i = tid; i < 2 * n_mels; i += kMelThreads) mtab[i] = a.mel_tab[i];
    for (int i = tid; i < a.n_weights; i += kMelThreads) mw[i] = a.mel_w[i];
    {   // staging: position p of the reflect-padded prompt, p = t0 hop + i; every frame below prompt_frames ends inside n + n_fft
        const int64_t off = a.offsets[b], n = it.samples, p0 = static_cast<int64_t>(t0) * hop;
        const float *x = a.pcm + off;
        const bool vec = a.vec && (off & 3) == 0 && (hop & 3) == 0;
        const int need = (live - 1) * hop + kNfft, pad = kNfft / 2;
        for (int i = 4 * tid; i < need; i += 4 * kMelThreads) {
            const int64_t p = p0 + i;
            float v[4];
            if (vec && p >= pad && p + 3 < pad + n) {
                const float4 t = *reinterpret_cast<const float4 *>(x + (p - pad));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {   // LuxTtsMelExtractor.swift:60-64
                    const int64_t q = p + c;
                    int64_t idx = q < pad ? (pad - q < n - 1 ? pad - q : n - 1) : (q < pad + n ? q - pad : n - 2 - (q - pad - n));
                    idx = idx < 0 ? 0 : idx;
                    v[c] = i + c < need ? x[idx] : 0.0f;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i + c < need) samples[i + c] = v[c] * rec.gain;
        }
    }
    __syncthreads();
    const int l = tid & 63, w = tid >> 6, k1 = l & 15, q = l >> 4;
    const int kb = ((q & 1) << 1) | (q >> 1);   // the output quarter this lane ends with: q = 0, 1, 2, 3 -> X_0, X_2, X_1, X_3
    float *R = static_cast<float *>(__builtin_assume_aligned(regions + w * kRegionFloats, 8));
    float *M = R + kTransposeFloats;            // the frame's kBins magnitudes
#pragma unroll 1
    for (int f = w; f < live; f += kMelWaves) {   // uniform in the wavefront; nothing below leaves its own region
        const float *fs = samples + f * hop;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {   // 0: the windowed frame, bins below kSplit; 1: its first difference, the bins from kSplit on
            Lane v;
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                const int j = 64 * n1 + l, jm = (j - 1) & (kNfft - 1);
                v.re[n1] = pass ? windowed_difference(fs[j], a.window[j], fs[jm], a.window[jm]) : fs[j] * a.window[j];
                v.im[n1] = 0.0f;
            }
            fft16(v);   // v[k1] = sum_n1 z[64 n1 + l] W16^(n1 k1)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k) { const float2 t = a.tw1024[(l * k) & (kNfft - 1)]; cmul(v.re[k], v.im[k], t.x, t.y); }
                *reinterpret_cast<float2 *>(R + 2 * (k * kRowStride + l)) = make_float2(v.re[k], v.im[k]);
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float2 t = *reinterpret_cast<const float2 *>(R + 2 * (k1 * kRowStride + 4 * m + q));
                v.re[m] = t.x; v.im[m] = t.y;
            }
            fft16(v);   // v[k2a] = sum_m B[k1][4 m + q] W16^(m k2a)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j) { const float2 t = a.tw1024[16 * q * j]; cmul(v.re[j], v.im[j], t.x, t.y); }   // W64^(q k2a)
                // radix-4 over q: y_q of the lanes l, l ^ 16, l ^ 32, l ^ 48
                const float pr = __shfl_xor(v.re[j], 32), pi = __shfl_xor(v.im[j], 32);
                const float tr = q < 2 ? v.re[j] + pr : pr - v.re[j], ti = q < 2 ? v.im[j] + pi : pi - v.im[j];   // y0 + y2, y1 + y3, y0 - y2, y1 - y3
                const float ur = __shfl_xor(tr, 16), ui = __shfl_xor(ti, 16);
                float zr, zi;
                if (q == 0) { zr = tr + ur; zi = ti + ui; }
                else if (q == 1) { zr = ur - tr; zi = ui - ti; }
                else if (q == 2) { zr = tr + ui; zi = ti - ur; }   // t - i u
                else { zr = ur - ti; zi = ui + tr; }               // u + i t
                const int k = k1 + 16 * j + 256 * kb;              // Z[k1 + 16 k2a + 256 k2b]; the frame is real: bins 0 .. 512 are all there is
                const float mag = sqrtf(zr * zr + zi * zi);        // LuxTtsMelExtractor.swift:100-105, power = 1
                if (pass == 0 && k < kSplit) M[k] = mag;
                if (pass == 1 && k >= kSplit && k <= kNfft / 2) M[k] = mag * a.undo[k];   // |X[k]| = |Y[k]| / |1 - W^k|
            }
            __builtin_amdgcn_wave_barrier();   // LDS operations of a wavefront complete in program order: the next pass may overwrite the buffer
        }
        float *out = dst + f * n_mels;
        for (int m = l; m < n_mels; m += 64) {
            const int packed = mtab[2 * m], cnt = packed >> 16;
            const float *bins = M + (packed & 0xffff), *wgt = mw + mtab[2 * m + 1];
            float acc = 0.0f;
            for (int j = 0; j < cnt; ++j) acc += wgt[j] * bins[j];
            out[m] = logf(fmaxf(acc, a.log_floor)) * a.feat_scale;   // :121-122, Synthesizer :176
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(kThreads) void inputs_kernel(const InputArgs a) {
    const int b = blockIdx.y;
    const Item it = a.items[b];
    const int64_t gt = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x, threads = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t total = static_cast<int64_t>(a.max_frames) * a.n_mels, active = static_cast<int64_t>(it.features_length) * a.n_mels;
    const uint64_t seed = a.seeds[b];
    float *x = a.s.x + static_cast<int64_t>(b) * total;
    for (int64_t e = 4 * gt; e < total; e += 4 * threads) {   // Synthesizer :185-187: element i of the start noise, zeros behind
        float4 o;
        o.x = e < active ? gaussian_at(seed, e) : 0.0f;
        o.y = e + 1 < active ? gaussian_at(seed, e + 1) : 0.0f;
        o.z = e + 2 < active ? gaussian_at(seed, e + 2) : 0.0f;
        o.w = e + 3 < active ? gaussian_at(seed, e + 3) : 0.0f;
        *reinterpret_cast<float4 *>(x + e) = o;
    }
    const int32_t *ids = a.token_ids + a.token_offsets[b];
    for (int64_t i = gt; i < a.max_tokens; i += threads) {    // :133-141
        a.s.tokens[static_cast<int64_t>(b) * a.max_tokens + i] = i < it.tokens ? ids[i] : 0;
        a.s.token_mask[static_cast<int64_t>(b) * a.max_tokens + i] = i < it.tokens ? 0.0f : 1.0f;
    }
    for (int64_t i = gt; i < a.max_frames; i += threads)      // :180-182
        a.s.frame_mask[static_cast<int64_t>(b) * a.max_frames + i] = i < it.features_length ? 0.0f : 1.0f;
}

__device__ __forceinline__ float4 load_row4(const float *p, const bool vec) {
    return vec ? *reinterpret_cast<const float4 *>(p) : make_float4(p[0], p[1], p[2], p[3]);
}

__global__ __launch_bounds__(kThreads) void text_condition_kernel(const RowArgs a) {
    const int b = blockIdx.y, n4 = a.n_mels / 4;
    const Item it = a.items[b];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.max_frames * n4) return;
    const int f = i / n4, c = 4 * (i - f * n4);
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (f < it.features_length)   // Synthesizer :163-171 on the stride-padded rows of :153-156
        o = load_row4(a.src + b * a.item_stride + token_row(f, it.tokens, it.avg) * a.row_stride + c, a.vec != 0);
    *reinterpret_cast<float4 *>(a.s.text_condition + (static_cast<int64_t>(b) * a.max_frames + f) * a.n_mels + c) = o;
}

__global__ __launch_bounds__(kThreads) void step_kernel(const RowArgs a) {
    const int b = blockIdx.y, n4 = a.n_mels / 4;
    const Item it = a.items[b];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= it.features_length * n4) return;   // rows behind stay zero
    const int f = i / n4, c = 4 * (i - f * n4);
    float4 *xp = reinterpret_cast<float4 *>(a.s.x + (static_cast<int64_t>(b) * a.max_frames + f) * a.n_mels + c);
    const float4 v = load_row4(a.src + b * a.item_stride + f * a.row_stride + c, a.vec != 0);
    float4 x = *xp;
    x.x = anchor_euler(x.x, v.x, a.times); x.y = anchor_euler(x.y, v.y, a.times);
    x.z = anchor_euler(x.z, v.z, a.times); x.w = anchor_euler(x.w, v.w, a.times);
    *xp = x;
}

__global__ __launch_bounds__(kThreads) void vocoder_input_kernel(const VocoderArgs a) {
    __shared__ float tile[kMaxMels * kVocStride];
    const int tid = threadIdx.x, k = blockIdx.y, n_mels = a.n_mels, bucket = a.bucket;
    const int b = a.list[k];
    const Item it = a.items[b];
    const int f0 = static_cast<int>(blockIdx.x) * kVocTile;
    int nf = it.gen_frames - f0;
    nf = nf < 0 ? 0 : (nf > kVocTile ? kVocTile : nf);
    const float *x = a.s.x + (static_cast<int64_t>(b) * a.max_frames + it.prompt_frames + f0) * n_mels;   // nf rows, contiguous
    for (int i = 4 * tid; i < nf * n_mels; i += 4 * kThreads) {
        const float4 t = *reinterpret_cast<const float4 *>(x + i);
        const int f = i / n_mels, m = i - f * n_mels;
        tile[m * kVocStride + f] = t.x * a.inv_scale; tile[(m + 1) * kVocStride + f] = t.y * a.inv_scale;   // Synthesizer :259
        tile[(m + 2) * kVocStride + f] = t.z * a.inv_scale; tile[(m + 3) * kVocStride + f] = t.w * a.inv_scale;
    }
    __syncthreads();
    const int fend = f0 + kVocTile < bucket ? f0 + kVocTile : bucket;
    constexpr int kGroups = kVocTile / 4 + 1;   // aligned groups of four that 64 consecutive floats can touch
    for (int t = tid; t < n_mels * kGroups; t += kThreads) {
        const int m = t / kGroups, gi = t - m * kGroups;
        const int64_t e0 = (static_cast<int64_t>(k) * n_mels + m) * bucket + f0, e1 = e0 + (fend - f0);
        const int64_t e = ((e0 >> 2) + gi) << 2;
        if (e >= e1) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int fl = static_cast<int>(e + c - e0);
            v[c] = fl >= 0 && fl < nf ? tile[m * kVocStride + fl] : a.floor_value;   // :261
        }
        if (a.vec && e >= e0 && e + 3 < e1) {
            *reinterpret_cast<float4 *>(a.mel + e) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (e + c >= e0 && e + c < e1) a.mel[e + c] = v[c];
        }
    }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const FinishArgs a) {
    const int b = blockIdx.y;
    const Item it = a.items[b];
    const int64_t i = 4 * (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x);
    if (i >= it.sample_count) return;
    const Record rec = a.s.records[b];
    const bool boosted = rec.rms < a.target_rms;          // Synthesizer :284-287
    const float back = rec.rms / a.target_rms;
    const int64_t so = b * a.row_stride, dof = a.sample_offsets[b];
    const float *src = a.audio + so + i;
    float *dst = a.out + dof + i;
    const bool vec = a.vec && ((so | dof) & 3) == 0 && i + 3 < it.sample_count;
    float v[4];
    if (vec) { const float4 t = *reinterpret_cast<const float4 *>(src); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!vec) v[c] = i + c < it.sample_count ? src[c] : 0.0f;
        v[c] = fminf(fmaxf(v[c], -1.0f), 1.0f);           // :281
        if (boosted) v[c] *= back;
    }
    if (vec) { *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]); return; }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (i + c < it.sample_count) dst[c] = v[c];
}

unsigned blocks_for(const int64_t items) { return static_cast<unsigned>((items + kThreads - 1) / kThreads); }

}  // namespace

namespace fa {
namespace luxtts {

void run_prompt(const MelArgs &a, const int batch, hipStream_t stream) {
    hipLaunchKernelGGL(loudness_kernel, dim3(static_cast<unsigned>(batch)), dim3(kRmsThreads), 0, stream, a);
    const dim3 grid(static_cast<unsigned>((a.max_frames + kTileFrames - 1) / kTileFrames), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(mel_kernel, grid, dim3(kMelThreads), mel_lds_bytes(a), stream, a);
}

void run_inputs(const InputArgs &a, const int batch, hipStream_t stream) {
    const dim3 grid(blocks_for(static_cast<int64_t>(a.max_frames) * a.n_mels / 4), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(inputs_kernel, grid, dim3(kThreads), 0, stream, a);
}

void run_text_condition(const RowArgs &a, const int batch, hipStream_t stream) {
    const dim3 grid(blocks_for(static_cast<int64_t>(a.max_frames) * a.n_mels / 4), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(text_condition_kernel, grid, dim3(kThreads), 0, stream, a);
}

void run_step(const RowArgs &a, const int batch, hipStream_t stream) {
    const dim3 grid(blocks_for(static_cast<int64_t>(a.max_frames) * a.n_mels / 4), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(step_kernel, grid, dim3(kThreads), 0, stream, a);
}

void run_vocoder_input(const VocoderArgs &a, const int n, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((a.bucket + kVocTile - 1) / kVocTile), static_cast<unsigned>(n));
    hipLaunchKernelGGL(vocoder_input_kernel, grid, dim3(kThreads), 0, stream, a);
}

void run_finish(const FinishArgs &a, const int batch, const int64_t max_samples, hipStream_t stream) {
    if (max_samples < 1) return;
    const dim3 grid(blocks_for((max_samples + 3) / 4), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(finish_kernel, grid, dim3(kThreads), 0, stream, a);
}

}  // namespace luxtts
}  // namespace fa
