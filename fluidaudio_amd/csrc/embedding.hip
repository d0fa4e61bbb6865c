// embedding.hip — the kernels of the embedding model's inputs and one launcher per stage: which (chunk, local speaker) pairs get an
// embedding, their masks resampled to the model's weight length, the fbank windows.  The plan, the staging, the TimedEmbedding records and
// the C ABI are embedding_host.hip; the host arithmetic is embedding_geom.h; what the two units share is embedding_launch.h.
//
//   * OfflineEmbeddingExtractor.extractEmbeddings (reference: Sources/FluidAudio/Diarizer/Offline/Extraction/OfflineEmbeddingExtractor.swift:
//     177-711).  A chunk is planned (becomes an fbank window) when start = clamp(round-half-away(offset * rate), 0, total) is below
//     end = min(start + samples_per_window, total) (:655-668); planned chunks form batches of clamp(batch_size, 1, 32) (:162, :309).
//     Per planned chunk and local speaker, in this order (:421-613): overlap frames (more than one speaker > threshold), baseSum <= 0
//     -> empty, the clean mask (overlap frames zeroed, only with exclude_overlap), cleanSum < Float(frames) * 0.2 -> empty, cleanSum >=
//     Float(minFrames) picks clean and otherwise base (a fallback), the mask resampled to weight_frames (WeightInterpolation.swift:19-116)
//     and its energy sum <= 0 -> empty.  firstActive / lastActive: the first / last index of the chosen mask > threshold (0 / firstActive
//     when none); the times offset + Double(frame) * fd are host code (fp64, no FMA).
//   * EmbeddingSkipStrategy.maskSimilarity (:338-352, :565-584, :632-640): per batch and local speaker, a job whose chosen mask has cosine
//     >= threshold against the mask of the last job that ran the model reuses that run's embedding; the cache is cleared after each batch.
//   * WeightInterpolation.resample: identity when the lengths agree; otherwise scale = Float(out) / Float(in), pos = (Float(i) + 0.5) /
//     scale - 0.5 clamped to [0, in - 1], left = floor, right = min(left + 1, in - 1), v = l * (1 - wr) + r * wr, all fp32 with separate
//     roundings (this file is built with -ffp-contract=off and spells them with __f*_rn).
//
// Summation order.  vDSP_sve / vDSP_dotpr do not specify one.  Every sum (baseSum, cleanSum, the resampled energy) and every dot product of
// the cosine is sequential in frame order, fp32.  For 0/1 weights (fa_powerset_decode's output) each is an exact integer below 2^24, so any
// order gives the reference's bits; for soft weights the result is pinned to the restatement (tests/embedding_restatement.py).
//
// Departure: a non-finite weight in a planned chunk is INVALID_ARGUMENT (the reference would hand NaN to the model).
//
// Kernels: emb_stats (one wavefront per planned chunk: the chunk staged in LDS, overlap flags, active bounds and tiles of mask and
// resampled values over the lanes, the sequential sums on one lane per (sum, speaker) walking those tiles), two block-scan compactions (valid masks -> jobs, jobs that run the model -> runs), the
// skip chain (one wavefront per (batch, speaker): pairwise dots over the lanes, the walk on lane 0), and byte-bound row writers.  No float
// atomics.  The planned-chunk list itself is host arithmetic over the host offsets (embedding_geom.h: one pass over the chunks).
#include <climits>

#include "block_scan.h"
#include "embedding_launch.h"

namespace {

using namespace fa::embedding;
using fa::grid_for;
constexpr int kThreads = fa::scan::kThreads;
constexpr int kLdsFloats = 8192;        // chunks of up to this many weights are staged in LDS (32 KiB); larger ones are read in place

// WeightInterpolation.InterpolationCoefficients (:19-52) for output index i
struct Coef { int l, r; float wl, wr; };
__host__ __device__ inline Coef coef(int i, int in, float scale) {
    const float pos = __fsub_rn(__fdiv_rn(__fadd_rn(static_cast<float>(i), 0.5f), scale), 0.5f);
    const float cl = fminf(fmaxf(pos, 0.0f), static_cast<float>(in - 1));
    const int l = static_cast<int>(floorf(cl));
    const float wr = __fsub_rn(cl, static_cast<float>(l));
    return Coef{l, min(l + 1, in - 1), __fsub_rn(1.0f, wr), wr};
}
__host__ __device__ inline float interp(float lv, float rv, const Coef &c) { return __fadd_rn(__fmul_rn(lv, c.wl), __fmul_rn(rv, c.wr)); }

// value of frame f of a chunk's chosen mask: the weight, or 0 on an overlap frame of a clean mask
__device__ inline bool overlap_frame(const float *row, int S, float thr) {
    int n = 0;
    for (int s = 0; s < S; ++s) n += row[s] > thr;
    return n > 1;
}
__device__ inline float mask_value(const float *chunk, int f, int s, int S, float thr, bool clean) {
    const float *row = chunk + static_cast<int64_t>(f) * S;
    return clean && overlap_frame(row, S, thr) ? 0.0f : row[s];
}

// One wavefront per planned window.  The chunk is staged in LDS (16-byte loads over its aligned body) and the lanes mark the overlap
// frames.  Then, per group of up to kGroup speakers, the lanes fill tiles of per-frame mask values and per-output resampled values (the
// interpolation coefficients are computed once per output, by the lanes), and one lane per (speaker, sum) walks each tile in order:
// baseSum, cleanSum, the energy of the resampled base mask and of the resampled clean mask.  Only these fp32 adds are sequential.
constexpr int kGroup = 4, kTile = 256, kMaxFlags = 8192;
__global__ __launch_bounds__(64) void emb_stats(StatsArgs a) {
    extern __shared__ float lds[];
    __shared__ float tile[kGroup][4][kTile + 1];   // [speaker][kind][position], rows padded: the 16 walkers read 16 banks: kind 0 base, 1 clean (frames), 2 base, 3 clean (resampled)
    __shared__ unsigned char ovl[kMaxFlags];
    __shared__ float sums[4][kGroup];
    __shared__ int32_t bounds[4][kGroup];
    const int win = blockIdx.x, lane = threadIdx.x;
    const int F = a.F, S = a.S, W = a.W, n = F * S;
    const float *g = a.w + static_cast<int64_t>(a.win_chunk[win]) * n;
    const bool staged = n <= kLdsFloats;
    int bad = 0;
    if (staged) {
        const int head = min(n, static_cast<int>(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2));
        const int body = (n - head) >> 2;
        const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
        for (int i = lane; i < head; i += 64) { const float v = g[i]; bad |= !isfinite(v); lds[i] = v; }
        for (int i = lane; i < body; i += 64) {
            const float4 v = g4[i];
            bad |= !isfinite(v.x) || !isfinite(v.y) || !isfinite(v.z) || !isfinite(v.w);
            float *d = lds + head + 4 * i;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        for (int i = head + 4 * body + lane; i < n; i += 64) { const float v = g[i]; bad |= !isfinite(v); lds[i] = v; }
    } else {
        for (int i = lane; i < n; i += 64) bad |= !isfinite(g[i]);
    }
    if (__any(bad) && lane == 0) atomicOr(a.bad, 1);
    __syncthreads();
    const float *m = staged ? lds : g;
    const bool excl = a.exclude != 0, flags_ok = F <= kMaxFlags;
    if (excl && flags_ok) for (int f = lane; f < F; f += 64) ovl[f] = overlap_frame(m + static_cast<int64_t>(f) * S, S, a.thr);
    __syncthreads();
    // frame f of speaker s's base (clean = false) or clean mask
    auto value = [&](int f, int s, bool clean) {
        const float v = m[static_cast<int64_t>(f) * S + s];
        if (!clean || !excl) return v;
        return (flags_ok ? ovl[f] != 0 : overlap_frame(m + static_cast<int64_t>(f) * S, S, a.thr)) ? 0.0f : v;
    };
    const float scale = __fdiv_rn(static_cast<float>(W), static_cast<float>(F));
    const int len = max(F, W);
    for (int s0 = 0; s0 < S; s0 += kGroup) {
        const int ns = min(kGroup, S - s0);
        const int wj = lane >> 2, wk = lane & 3;   // walker lanes: speaker s0 + wj, sum wk
        const bool walker = lane < 4 * ns;
        float acc = 0.0f;
        for (int t0 = 0; t0 < len; t0 += kTile) {
            const int nt = min(kTile, len - t0);
            for (int i = lane; i < nt; i += 64) {
                const int p = t0 + i;
                Coef c{};
                if (p < W && F != W) c = coef(p, F, scale);
                for (int j = 0; j < ns; ++j) {
                    const int s = s0 + j;
                    if (p < F) { tile[j][0][i] = value(p, s, false); tile[j][1][i] = value(p, s, true); }
                    if (p < W && F != W) {
                        tile[j][2][i] = interp(value(c.l, s, false), value(c.r, s, false), c);
                        tile[j][3][i] = interp(value(c.l, s, true), value(c.r, s, true), c);
                    }
                }
            }
            __syncthreads();
            if (walker) {
                const int lim = wk < 2 ? F : (F == W ? 0 : W);   // the identity resample's energy is the mask sum itself
                const int stop = min(nt, lim - t0);
                for (int i = 0; i < stop; ++i) acc = __fadd_rn(acc, tile[wj][wk][i]);
            }
            __syncthreads();
        }
        if (walker) sums[wk][wj] = acc;
        // first / last active frame of the base and the clean mask
        for (int j = 0; j < ns; ++j) {
            const int sj = s0 + j;
            int fb = INT_MAX, lb = -1, fc = INT_MAX, lc = -1;
            for (int f = lane; f < F; f += 64) {
                if (value(f, sj, false) > a.thr) { fb = min(fb, f); lb = max(lb, f); }
                if (value(f, sj, true) > a.thr) { fc = min(fc, f); lc = max(lc, f); }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                fb = min(fb, __shfl_xor(fb, off));
                lb = max(lb, __shfl_xor(lb, off));
                fc = min(fc, __shfl_xor(fc, off));
                lc = max(lc, __shfl_xor(lc, off));
            }
            if (lane == 0) { bounds[0][j] = fb; bounds[1][j] = lb; bounds[2][j] = fc; bounds[3][j] = lc; }
        }
        __syncthreads();
        if (lane < ns) {
            const int s = s0 + lane;
            const float base = sums[0][lane], clean = sums[1][lane];
            const float e_base = F == W ? base : sums[2][lane], e_clean = F == W ? clean : sums[3][lane];
            int flags = 0, first = 0, last = 0;
            if (!(base > 0.0f) || clean < a.min_active) {
                flags = kEmpty;
            } else {
                const bool use_clean = clean >= a.min_frames;
                if (!use_clean) flags |= kFallback;
                const int fi = use_clean ? bounds[2][lane] : bounds[0][lane], la = use_clean ? bounds[3][lane] : bounds[1][lane];
                first = fi == INT_MAX ? 0 : fi;
                last = la < 0 ? first : la;
                flags |= (use_clean ? e_clean : e_base) > 0.0f ? kValid : kEmpty;
            }
            a.rec[static_cast<int64_t>(win) * S + s] = ItemRec{flags, first, last, 0};
        }
        __syncthreads();
        if (a.masks) {   // the chosen mask of every valid slot, for the skip chain
            for (int j = 0; j < ns; ++j) {
                const int sj = s0 + j;
                const int flags = a.rec[static_cast<int64_t>(win) * S + sj].flags;
                if (!(flags & kValid)) continue;
                float *dst = a.masks + (static_cast<int64_t>(win) * S + sj) * F;
                for (int f = lane; f < F; f += 64) dst[f] = value(f, sj, !(flags & kFallback));
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- compaction: the predicates and the sink of block_scan.h's compact

struct ValidPred {   // item i is a job
    const ItemRec *rec;
    __device__ int operator()(int64_t i) const { return (rec[i].flags & kValid) != 0; }
};
struct RunPred {     // job j runs the model (j < jobs)
    const int32_t *is_run;
    const int32_t *jobs;
    __device__ int operator()(int64_t j) const { return j < *jobs && is_run[j] != 0; }
};

// idx_of[i] = compacted index or -1; item_of[k] = i
struct IndexSink {
    int32_t *idx_of, *item_of;
    __device__ void kept(int64_t i, int pos) const { idx_of[i] = pos; item_of[pos] = static_cast<int32_t>(i); }
    __device__ void dropped(int64_t i) const { idx_of[i] = -1; }
};

// every job runs the model (skipping off, or before the skip chain decides)
__global__ __launch_bounds__(kThreads) void runs_init(const int32_t *__restrict__ jobs, int64_t cap, int32_t *__restrict__ is_run, int32_t *__restrict__ src) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= cap || j >= *jobs) return;
    is_run[j] = 1;
    src[j] = static_cast<int32_t>(j);
}

__device__ inline float seq_dot(const float *x, const float *y, int F) {
    float acc = 0.0f;
    for (int f = 0; f < F; ++f) acc = __fadd_rn(acc, __fmul_rn(x[f], y[f]));
    return acc;
}

// One wavefront per (batch, local speaker): the jobs of that speaker in the batch's windows, in order; every pairwise dot product and
// norm over the lanes, then the cache walk on lane 0 (maskCosineSimilarity, :835-842; cache updated only when the model runs).
__global__ __launch_bounds__(64) void skip_chain(const int32_t *__restrict__ job_of_item, const float *__restrict__ masks, int32_t nw, int32_t S,
                                                 int32_t F, int32_t B, float threshold, int32_t *__restrict__ is_run, int32_t *__restrict__ src) {
    __shared__ int32_t job[kMaxBatch], item[kMaxBatch];
    __shared__ float dots[kMaxBatch * kMaxBatch];
    __shared__ int32_t njobs;
    const int b = blockIdx.x / S, s = blockIdx.x - b * S, lane = threadIdx.x;
    const int w0 = b * B, nwin = min(B, nw - w0);
    const int it = (w0 + lane) * S + s;
    const int j = lane < nwin ? job_of_item[it] : -1;
    const unsigned long long bal = __ballot(j >= 0);
    if (j >= 0) { const int pos = __popcll(bal & ((1ull << lane) - 1ull)); job[pos] = j; item[pos] = it; }
    if (lane == 0) njobs = __popcll(bal);
    __syncthreads();
    const int n = njobs;
    for (int p = lane; p < n * (n + 1) / 2; p += 64) {   // pairs (x, y), y <= x, row-major over the lower triangle
        int x = 0;
        while ((x + 1) * (x + 2) / 2 <= p) ++x;
        const int y = p - x * (x + 1) / 2;
        dots[x * kMaxBatch + y] = seq_dot(masks + static_cast<int64_t>(item[x]) * F, masks + static_cast<int64_t>(item[y]) * F, F);
    }
    __syncthreads();
    if (lane != 0) return;
    int cache = -1;
    for (int x = 0; x < n; ++x) {
        if (cache >= 0) {
            const float dot = dots[x * kMaxBatch + cache], na = dots[x * kMaxBatch + x], nb = dots[cache * kMaxBatch + cache];
            const float denom = __fmul_rn(__fsqrt_rn(na), __fsqrt_rn(nb));
            const float cs = denom > 0.0f ? __fdiv_rn(dot, denom) : 0.0f;
            if (cs >= threshold) { is_run[job[x]] = 0; src[job[x]] = job[cache]; continue; }
        }
        cache = x;
    }
}

// run_of_job[j] = run index of the job whose embedding j carries; window_of_run[r] = window of run r's job
__global__ __launch_bounds__(kThreads) void runs_finish(const int32_t *__restrict__ totals, int64_t cap, const int32_t *__restrict__ src,
                                                        const int32_t *__restrict__ run_of_src, const int32_t *__restrict__ job_of_run,
                                                        const int32_t *__restrict__ item_of_job, int32_t S, int32_t *__restrict__ run_of_job,
                                                        int32_t *__restrict__ window_of_run) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= cap) return;
    if (j < totals[0]) run_of_job[j] = run_of_src[src[j]];
    if (j < totals[1]) window_of_run[j] = item_of_job[job_of_run[j]] / S;
}

// the model's weights input: one thread per (run, output frame)
__global__ __launch_bounds__(kThreads) void run_rows(RowArgs a, int64_t runs, float *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= runs * a.W) return;
    const int64_t r = e / a.W;
    const int i = static_cast<int>(e - r * a.W);
    const int it = a.item_of_job[a.job_of_run[r]];
    const int win = it / a.S, s = it - win * a.S;
    const float *chunk = a.w + static_cast<int64_t>(a.win_chunk[win]) * a.F * a.S;
    const bool clean = a.exclude && !(a.rec[it].flags & kFallback);
    if (a.F == a.W) { out[e] = mask_value(chunk, i, s, a.S, a.thr, clean); return; }
    const Coef c = coef(i, a.F, __fdiv_rn(static_cast<float>(a.W), static_cast<float>(a.F)));
    out[e] = interp(mask_value(chunk, c.l, s, a.S, a.thr, clean), mask_value(chunk, c.r, s, a.S, a.thr, clean), c);
}

// TimedEmbedding.frameWeights: one thread per (job, frame)
__global__ __launch_bounds__(kThreads) void mask_rows(RowArgs a, int64_t jobs, float *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= jobs * a.F) return;
    const int64_t j = e / a.F;
    const int f = static_cast<int>(e - j * a.F);
    const int it = a.item_of_job[j];
    const int win = it / a.S, s = it - win * a.S;
    const float *chunk = a.w + static_cast<int64_t>(a.win_chunk[win]) * a.F * a.S;
    out[e] = mask_value(chunk, f, s, a.S, a.thr, a.exclude && !(a.rec[it].flags & kFallback));
}

// audio[start, start + len) then zeros, one thread per output sample of `count` rows of spw samples
__global__ __launch_bounds__(kThreads) void window_rows(const float *__restrict__ audio, const int64_t *__restrict__ start, const int64_t *__restrict__ len,
                                                        int64_t count, int32_t spw, float *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= count * spw) return;
    const int64_t r = e / spw, i = e - r * spw;
    out[e] = i < len[r] ? audio[start[r] + i] : 0.0f;
}

// the span's all-active weight row: 1 for the first active[r] frames
__global__ __launch_bounds__(kThreads) void span_rows(const int32_t *__restrict__ active, int64_t count, int32_t W, float *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= count * W) return;
    const int64_t r = e / W;
    out[e] = e - r * W < active[r] ? 1.0f : 0.0f;
}

// WeightInterpolation.resample2D over rows: one thread per output element
__global__ __launch_bounds__(kThreads) void resample_rows(const float *__restrict__ in, int64_t rows, int32_t n_in, int32_t n_out, float *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= rows * n_out) return;
    const int64_t r = e / n_out;
    const int i = static_cast<int>(e - r * n_out);
    const float *x = in + r * n_in;
    if (n_in == n_out) { out[e] = x[i]; return; }
    const Coef c = coef(i, n_in, __fdiv_rn(static_cast<float>(n_out), static_cast<float>(n_in)));
    out[e] = interp(x[c.l], x[c.r], c);
}

}  // namespace

// ---------------------------------------------------------------- launchers (embedding_launch.h)

namespace fa {
namespace embedding {

int64_t select_blocks(int64_t items) { return fa::scan::compact_blocks(items); }

void launch_select(hipStream_t st, const StatsArgs &a, const SelectArgs &s) {
    const int64_t nw = a.nw, items = nw * a.S;
    const int32_t n_fs = a.F * a.S;
    const size_t lds = n_fs <= kLdsFloats ? sizeof(float) * n_fs : 0;
    hipLaunchKernelGGL(emb_stats, dim3(static_cast<unsigned>(nw)), dim3(64), lds, st, a);
    fa::scan::compact(st, ValidPred{a.rec}, IndexSink{s.job_of_item, s.item_of_job}, items, s.bsum, s.flags + 1);
    hipLaunchKernelGGL(runs_init, dim3(grid_for(items, kThreads)), dim3(kThreads), 0, st, s.flags + 1, items, s.is_run, s.src);
    if (s.skip)
        hipLaunchKernelGGL(skip_chain, dim3(static_cast<unsigned>(((nw + s.B - 1) / s.B) * a.S)), dim3(64), 0, st, s.job_of_item, a.masks, a.nw, a.S, a.F, s.B,
                           s.skip_threshold, s.is_run, s.src);
    fa::scan::compact(st, RunPred{s.is_run, s.flags + 1}, IndexSink{s.run_of_src, s.job_of_run}, items, s.bsum, s.flags + 2);
    hipLaunchKernelGGL(runs_finish, dim3(grid_for(items, kThreads)), dim3(kThreads), 0, st, s.flags + 1, items, s.src, s.run_of_src, s.job_of_run, s.item_of_job,
                       a.S, s.run_of_job, s.window_of_run);
}

void launch_rows(hipStream_t st, const RowArgs &a, int64_t runs, float *rows, int64_t jobs, float *mrows) {
    if (runs > 0) hipLaunchKernelGGL(run_rows, dim3(grid_for(runs * a.W, kThreads)), dim3(kThreads), 0, st, a, runs, rows);
    if (mrows && jobs > 0) hipLaunchKernelGGL(mask_rows, dim3(grid_for(jobs * a.F, kThreads)), dim3(kThreads), 0, st, a, jobs, mrows);
}

void launch_windows(hipStream_t st, const float *audio, const int64_t *start, const int64_t *len, int64_t count, int32_t spw, float *out) {
    hipLaunchKernelGGL(window_rows, dim3(grid_for(count * spw, kThreads)), dim3(kThreads), 0, st, audio, start, len, count, spw, out);
}

void launch_spans(hipStream_t st, const int32_t *active, int64_t count, int32_t W, float *out) {
    hipLaunchKernelGGL(span_rows, dim3(grid_for(count * W, kThreads)), dim3(kThreads), 0, st, active, count, W, out);
}

void launch_resample(hipStream_t st, const float *in, int64_t rows, int32_t n_in, int32_t n_out, float *out) {
    hipLaunchKernelGGL(resample_rows, dim3(grid_for(rows * n_out, kThreads)), dim3(kThreads), 0, st, in, rows, n_in, n_out, out);
}

}  // namespace embedding
}  // namespace fa
