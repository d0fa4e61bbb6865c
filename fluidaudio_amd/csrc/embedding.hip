// embedding.hip — the embedding model's inputs on the device: which (chunk, local speaker) pairs get an embedding, their masks
// resampled to the model's weight length, the fbank windows, and the TimedEmbedding metadata.
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
// atomics.  The planned-chunk list itself is host arithmetic over the host offsets (one pass over the chunks).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "block_scan.h"
#include "fa_common.h"

namespace {

using fa::grid_for;
using fa::scan::block_exclusive;
constexpr int kThreads = fa::scan::kThreads;
constexpr int kScanPer = 8;             // items per thread of a compaction
constexpr int kMaxBatch = 32;           // modelBatchLimit (:162)
constexpr int kLdsFloats = 8192;        // chunks of up to this many weights are staged in LDS (32 KiB); larger ones are read in place
constexpr int kValid = 1, kFallback = 2, kEmpty = 4;

struct ItemRec {   // one (planned window, local speaker)
    int32_t flags, first, last, pad;
};

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

struct StatsArgs {
    const float *w;            // [C][F][S]
    const int32_t *win_chunk;  // [nw] chunk of each planned window
    ItemRec *rec;              // [nw][S]
    float *masks;              // [nw][S][F] chosen masks (skip chain only) or nullptr
    int32_t *bad;
    int32_t nw, F, S, W, exclude;
    float thr, min_frames, min_active;   // Float(minFrames), Float(frames) * 0.2
};

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

// ---------------------------------------------------------------- compaction (block_scan.h: per-block counts, scan_totals, a write pass)


struct ValidPred {   // item i is a job
    const ItemRec *rec;
    __device__ int operator()(int64_t i) const { return (rec[i].flags & kValid) != 0; }
};
struct RunPred {     // job j runs the model (j < jobs)
    const int32_t *is_run;
    const int32_t *jobs;
    __device__ int operator()(int64_t j) const { return j < *jobs && is_run[j] != 0; }
};

template <class P>
__global__ __launch_bounds__(kThreads) void flag_count(P p, int64_t n, int32_t *__restrict__ bsum) {
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kScanPer;
    int c = 0;
    for (int i = 0; i < kScanPer; ++i) if (e0 + i < n) c += p(e0 + i);
    int tot;
    (void)block_exclusive(c, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}


// idx_of[i] = compacted index or -1; item_of[k] = i
template <class P>
__global__ __launch_bounds__(kThreads) void flag_write(P p, int64_t n, const int32_t *__restrict__ boff, int32_t *__restrict__ idx_of,
                                                       int32_t *__restrict__ item_of) {
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kScanPer;
    int flags = 0, c = 0;
    for (int i = 0; i < kScanPer; ++i) if (e0 + i < n && p(e0 + i)) { flags |= 1 << i; ++c; }
    int tot;
    int pos = boff[blockIdx.x] + block_exclusive(c, &tot);
    for (int i = 0; i < kScanPer; ++i) {
        if (e0 + i >= n) break;
        if (flags & (1 << i)) { idx_of[e0 + i] = pos; item_of[pos] = static_cast<int32_t>(e0 + i); ++pos; }
        else idx_of[e0 + i] = -1;
    }
}

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

struct RowArgs {
    const float *w;
    const int32_t *win_chunk, *item_of_job, *job_of_run;
    const ItemRec *rec;
    int32_t F, S, W, exclude;
    float thr;
};

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

// ---------------------------------------------------------------- host side

int32_t samples_per_window(const fa_embedding_config &cfg) {
    if (cfg.samples_per_window > 0) return cfg.samples_per_window;
    const double v = static_cast<double>(cfg.sample_rate) * cfg.window_duration;   // OfflineDiarizerTypes.swift:348-353
    return v >= 1.0 && v < static_cast<double>(INT32_MAX) ? static_cast<int32_t>(v) : 0;
}

// clamp(Int((x * rate).rounded()), 0, total): rounded() is half away from zero (std::round)
int64_t sample_index(double seconds, int32_t rate, int64_t total) {
    const double r = std::round(seconds * static_cast<double>(rate));
    if (!(r > 0.0)) return 0;
    if (r >= static_cast<double>(total)) return total;
    return static_cast<int64_t>(r);
}

bool config_ok(const fa_embedding_config *cfg) {
    return cfg && cfg->sample_rate > 0 && std::isfinite(cfg->window_duration) && cfg->weight_frames > 0 && samples_per_window(*cfg) > 0 &&
           std::isfinite(cfg->overlap_threshold) && !std::isnan(cfg->min_segment_duration) && std::isfinite(cfg->frame_duration);
}

void clear_info(fa_embedding_info *info) { if (info) memset(info, 0, sizeof(*info)); }

fa_status plan(fa_ctx *ctx, const fa_embedding_config *cfg, const float *weights, int64_t C, int32_t F, int32_t S, const double *offsets, int64_t n_offsets,
               int64_t total_samples, fa_export_embedding *records, int32_t *run_of_job, int32_t *window_of_run, int64_t *window_start,
               int32_t *window_chunk, float *run_weights, float *mask_rows_out, fa_embedding_info *info, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    clear_info(info);
    if (!config_ok(cfg)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: bad config");
    if (C < 0 || F < 0 || S < 0 || n_offsets < 0 || total_samples < 0 || (C > 0 && F > 0 && S > 0 && !weights) || (n_offsets > 0 && !offsets))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: bad arguments");
    if (C > 0 && F > 0 && S > 0 && (!records || !run_of_job || !window_of_run || !run_weights))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: records, run_of_job, window_of_run and run_weights are required");
    if (C * static_cast<int64_t>(S) > INT32_MAX / 2 || static_cast<int64_t>(F) * S > INT32_MAX / 2)
        return fa::set_error(ctx, FA_INDEX_OVERFLOW, "embedding plan: more than 2^30 masks");
    const int32_t spw = samples_per_window(*cfg), W = cfg->weight_frames, B = std::max(1, std::min(cfg->batch_size, kMaxBatch));
    const double fd = cfg->frame_duration > 0 ? cfg->frame_duration : (F > 0 ? cfg->window_duration / F : 0.0);   // :373-382
    double mf = fd > 0 ? std::ceil(cfg->min_segment_duration / fd) : 1.0;                                       // :384-390
    mf = std::max(1.0, std::min(mf, 2147483647.0));
    if (info) {
        info->frame_duration = fd;
        info->min_frames = static_cast<int32_t>(mf);
        info->samples_per_window = spw;
        info->batch_size = B;
    }
    if (C == 0 || F == 0) return FA_SUCCESS;   // extractEmbeddings skips chunks without frames (:182-186)
    return fa::no_throw(ctx, "embedding plan", [&]() -> fa_status {
    // planned chunks (:650-668)
    std::vector<int32_t> win_chunk;
    std::vector<int64_t> win_start;
    std::vector<double> win_offset;
    for (int64_t c = 0; c < C; ++c) {
        double off = c < n_offsets ? offsets[c] : static_cast<double>(c) * cfg->window_duration;
        if (!std::isfinite(off)) off = static_cast<double>(c) * cfg->window_duration;
        const int64_t start = sample_index(off, cfg->sample_rate, total_samples);
        const int64_t end = std::min(start + static_cast<int64_t>(spw), total_samples);
        if (start >= end) continue;
        win_chunk.push_back(static_cast<int32_t>(c));
        win_start.push_back(start);
        win_offset.push_back(off);
    }
    const int64_t nw = static_cast<int64_t>(win_chunk.size()), items = nw * S;
    if (info) {
        info->planned_chunks = nw;
        info->batches = (nw + B - 1) / B;
        info->evaluated_masks = items;
    }
    if (window_start) std::copy(win_start.begin(), win_start.end(), window_start);
    if (window_chunk) std::copy(win_chunk.begin(), win_chunk.end(), window_chunk);
    if (items == 0) return FA_SUCCESS;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    const bool skip = cfg->skip_enabled != 0;
    const int64_t nb = (items + kThreads * kScanPer - 1) / (kThreads * kScanPer);
    fa::DevBuf b_w, b_chunk, b_rec, b_masks, b_flags, b_bsum, b_job_of_item, b_item_of_job, b_is_run, b_src, b_run_of_src, b_job_of_run, b_run_of_job,
        b_window_of_run, b_rows, b_mrows;
    auto alloc = [&](fa::DevBuf &b, size_t bytes) { return b.alloc(ctx, bytes) == hipSuccess; };
    const size_t wbytes = sizeof(float) * C * F * S;
    if ((!device && !alloc(b_w, wbytes)) || !alloc(b_chunk, sizeof(int32_t) * nw) || !alloc(b_rec, sizeof(ItemRec) * items) ||
        (skip && !alloc(b_masks, sizeof(float) * items * F)) || !alloc(b_flags, sizeof(int32_t) * 4) || !alloc(b_bsum, sizeof(int32_t) * nb) ||
        !alloc(b_job_of_item, sizeof(int32_t) * items) || !alloc(b_item_of_job, sizeof(int32_t) * items) || !alloc(b_is_run, sizeof(int32_t) * items) ||
        !alloc(b_src, sizeof(int32_t) * items) || !alloc(b_run_of_src, sizeof(int32_t) * items) || !alloc(b_job_of_run, sizeof(int32_t) * items) ||
        !alloc(b_run_of_job, sizeof(int32_t) * items) || !alloc(b_window_of_run, sizeof(int32_t) * items)) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "embedding plan: device allocation failed");
    }
    const float *d_w = weights;
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(b_w.p, weights, wbytes, hipMemcpyHostToDevice, st));
        d_w = b_w.as<float>();
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_chunk.p, win_chunk.data(), sizeof(int32_t) * nw, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_flags.p, 0, sizeof(int32_t) * 4, st));   // [0] bad, [1] jobs, [2] runs
    int32_t *d_flags = b_flags.as<int32_t>();
    const int32_t n_fs = F * S;
    StatsArgs sa{d_w, b_chunk.as<int32_t>(), b_rec.as<ItemRec>(), skip ? b_masks.as<float>() : nullptr, d_flags, static_cast<int32_t>(nw), F, S, W,
                 cfg->exclude_overlap != 0, cfg->overlap_threshold, static_cast<float>(mf), static_cast<float>(F) * 0.2f};
    const size_t lds = n_fs <= kLdsFloats ? sizeof(float) * n_fs : 0;
    hipLaunchKernelGGL(emb_stats, dim3(static_cast<unsigned>(nw)), dim3(64), lds, st, sa);
    const unsigned nbu = static_cast<unsigned>(nb);
    hipLaunchKernelGGL(flag_count<ValidPred>, dim3(nbu), dim3(kThreads), 0, st, ValidPred{b_rec.as<ItemRec>()}, items, b_bsum.as<int32_t>());
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(kThreads), 0, st, b_bsum.as<int32_t>(), nb, d_flags + 1);
    hipLaunchKernelGGL(flag_write<ValidPred>, dim3(nbu), dim3(kThreads), 0, st, ValidPred{b_rec.as<ItemRec>()}, items, b_bsum.as<int32_t>(),
                       b_job_of_item.as<int32_t>(), b_item_of_job.as<int32_t>());
    hipLaunchKernelGGL(runs_init, dim3(grid_for(items, kThreads)), dim3(kThreads), 0, st, d_flags + 1, items, b_is_run.as<int32_t>(), b_src.as<int32_t>());
    if (skip)
        hipLaunchKernelGGL(skip_chain, dim3(static_cast<unsigned>(((nw + B - 1) / B) * S)), dim3(64), 0, st, b_job_of_item.as<int32_t>(), b_masks.as<float>(),
                           static_cast<int32_t>(nw), S, F, B, cfg->skip_threshold, b_is_run.as<int32_t>(), b_src.as<int32_t>());
    const RunPred rp{b_is_run.as<int32_t>(), d_flags + 1};
    hipLaunchKernelGGL(flag_count<RunPred>, dim3(nbu), dim3(kThreads), 0, st, rp, items, b_bsum.as<int32_t>());
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(kThreads), 0, st, b_bsum.as<int32_t>(), nb, d_flags + 2);
    hipLaunchKernelGGL(flag_write<RunPred>, dim3(nbu), dim3(kThreads), 0, st, rp, items, b_bsum.as<int32_t>(), b_run_of_src.as<int32_t>(),
                       b_job_of_run.as<int32_t>());
    hipLaunchKernelGGL(runs_finish, dim3(grid_for(items, kThreads)), dim3(kThreads), 0, st, d_flags + 1, items, b_src.as<int32_t>(), b_run_of_src.as<int32_t>(),
                       b_job_of_run.as<int32_t>(), b_item_of_job.as<int32_t>(), S, b_run_of_job.as<int32_t>(), b_window_of_run.as<int32_t>());
    FA_HIP_TRY(ctx, hipGetLastError());
    int32_t flags[4];
    FA_HIP_TRY(ctx, hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flags[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding plan: a speaker weight of a planned chunk is not finite");
    const int64_t jobs = flags[1], runs = flags[2];

    RowArgs ra{d_w, b_chunk.as<int32_t>(), b_item_of_job.as<int32_t>(), b_job_of_run.as<int32_t>(), b_rec.as<ItemRec>(), F, S, W, cfg->exclude_overlap != 0,
               cfg->overlap_threshold};
    float *d_rows = run_weights, *d_mrows = mask_rows_out;
    if (!device) {
        if ((runs > 0 && !alloc(b_rows, sizeof(float) * runs * W)) || (mask_rows_out && jobs > 0 && !alloc(b_mrows, sizeof(float) * jobs * F))) {
            (void)hipGetLastError();
            return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "embedding plan: device allocation failed");
        }
        d_rows = b_rows.as<float>();
        d_mrows = mask_rows_out ? b_mrows.as<float>() : nullptr;
    }
    if (runs > 0) hipLaunchKernelGGL(run_rows, dim3(grid_for(runs * W, kThreads)), dim3(kThreads), 0, st, ra, runs, d_rows);
    if (d_mrows && jobs > 0) hipLaunchKernelGGL(mask_rows, dim3(grid_for(jobs * F, kThreads)), dim3(kThreads), 0, st, ra, jobs, d_mrows);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<ItemRec> rec(static_cast<size_t>(items));
    std::vector<int32_t> item_of_job(static_cast<size_t>(jobs));
    FA_HIP_TRY(ctx, hipMemcpyAsync(rec.data(), b_rec.p, sizeof(ItemRec) * items, hipMemcpyDeviceToHost, st));
    if (jobs > 0) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(item_of_job.data(), b_item_of_job.p, sizeof(int32_t) * jobs, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(run_of_job, b_run_of_job.p, sizeof(int32_t) * jobs, hipMemcpyDeviceToHost, st));
    }
    if (runs > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(window_of_run, b_window_of_run.p, sizeof(int32_t) * runs, hipMemcpyDeviceToHost, st));
    if (!device) {
        if (runs > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(run_weights, d_rows, sizeof(float) * runs * W, hipMemcpyDeviceToHost, st));
        if (d_mrows && jobs > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(mask_rows_out, d_mrows, sizeof(float) * jobs * F, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    int64_t empty = 0, fallback = 0;
    for (const ItemRec &r : rec) { empty += (r.flags & kEmpty) != 0; fallback += (r.flags & kFallback) != 0; }
    for (int64_t j = 0; j < jobs; ++j) {   // OfflineEmbeddingPending (:586-611): times in fp64, no FMA
        const int32_t it = item_of_job[j];
        const int64_t win = it / S;
        const ItemRec &r = rec[it];
        fa_export_embedding &e = records[j];
        e.chunk_index = win_chunk[win];
        e.speaker_index = static_cast<int32_t>(it - win * S);
        e.start_frame = r.first;
        e.end_frame = r.last;
        const double a = static_cast<double>(r.first) * fd, b = static_cast<double>(r.last + 1) * fd;
        e.start_time = win_offset[win] + a;
        e.end_time = win_offset[win] + b;
    }
    if (info) {
        info->jobs = jobs;
        info->runs = runs;
        info->empty_masks = empty;
        info->fallback_masks = fallback;
        info->skipped_embeddings = jobs - runs;
    }
    return FA_SUCCESS;
    });
}

fa_status span_inputs(fa_ctx *ctx, const fa_embedding_config *cfg, const float *audio, int64_t total_samples, const double *spans, int64_t n,
                      float *windows, float *weights, fa_status *statuses, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!config_ok(cfg)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "span inputs: bad config");
    if (n < 0 || total_samples < 0 || (n > 0 && (!spans || !windows || !weights || !statuses)) || (total_samples > 0 && n > 0 && !audio))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "span inputs: bad arguments");
    if (n == 0) return FA_SUCCESS;
    const int32_t spw = samples_per_window(*cfg), W = cfg->weight_frames;
    return fa::no_throw(ctx, "span inputs", [&]() -> fa_status {
    std::vector<int64_t> start(static_cast<size_t>(n)), len(static_cast<size_t>(n));
    std::vector<int32_t> active(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {   // embedSpan (:243-297)
        const double rate = static_cast<double>(cfg->sample_rate);
        const double rs = std::round(spans[2 * i] * rate), re = std::round(spans[2 * i + 1] * rate);
        const int64_t s = rs > 0 ? (rs < 9.0e18 ? static_cast<int64_t>(rs) : INT64_MAX / 2) : 0;
        const int64_t e = re < static_cast<double>(total_samples) ? (re > -9.0e18 ? static_cast<int64_t>(re) : -INT64_MAX / 2) : total_samples;
        const int64_t l = std::min(e - s, static_cast<int64_t>(spw));
        statuses[i] = std::isfinite(spans[2 * i]) && std::isfinite(spans[2 * i + 1]) && l > 0 ? FA_SUCCESS : FA_INVALID_ARGUMENT;
        start[i] = statuses[i] == FA_SUCCESS ? s : 0;
        len[i] = statuses[i] == FA_SUCCESS ? l : 0;
        const double frac = static_cast<double>(len[i]) / static_cast<double>(spw);
        const double r = std::round(frac * static_cast<double>(W));
        active[i] = statuses[i] == FA_SUCCESS ? static_cast<int32_t>(std::max(1.0, std::min(static_cast<double>(W), r))) : 0;
    }
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_audio, b_start, b_len, b_active, b_win, b_w;
    auto alloc = [&](fa::DevBuf &b, size_t bytes) { return b.alloc(ctx, bytes) == hipSuccess; };
    if ((!device && total_samples > 0 && !alloc(b_audio, sizeof(float) * total_samples)) || !alloc(b_start, sizeof(int64_t) * n) ||
        !alloc(b_len, sizeof(int64_t) * n) || !alloc(b_active, sizeof(int32_t) * n) || (!device && !alloc(b_win, sizeof(float) * n * spw)) ||
        (!device && !alloc(b_w, sizeof(float) * n * W))) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "span inputs: device allocation failed");
    }
    const float *d_audio = device ? audio : b_audio.as<float>();
    float *d_win = device ? windows : b_win.as<float>(), *d_w = device ? weights : b_w.as<float>();
    if (!device && total_samples > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_audio.p, audio, sizeof(float) * total_samples, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_start.p, start.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_len.p, len.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_active.p, active.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(window_rows, dim3(grid_for(n * spw, kThreads)), dim3(kThreads), 0, st, d_audio, b_start.as<int64_t>(), b_len.as<int64_t>(), n, spw, d_win);
    hipLaunchKernelGGL(span_rows, dim3(grid_for(n * W, kThreads)), dim3(kThreads), 0, st, b_active.as<int32_t>(), n, W, d_w);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(windows, d_win, sizeof(float) * n * spw, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(weights, d_w, sizeof(float) * n * W, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the host staging of start / len / active lives until here
    return FA_SUCCESS;
    });
}

fa_status weight_resample(fa_ctx *ctx, const float *in, int64_t rows, int32_t n_in, int32_t n_out, float *out, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (rows < 0 || n_in < 0 || n_out < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "weight resample: negative size");
    if (rows == 0 || n_in == 0 || n_out == 0) return FA_SUCCESS;   // resample / resample2D return [] (:98-101, :110-113)
    if (!in || !out) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "weight resample: bad arguments");
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_in, b_out;
    const float *d_in = in;
    float *d_out = out;
    if (!device) {
        if (b_in.alloc(ctx, sizeof(float) * rows * n_in) != hipSuccess || b_out.alloc(ctx, sizeof(float) * rows * n_out) != hipSuccess) {
            (void)hipGetLastError();
            return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "weight resample: device allocation failed");
        }
        FA_HIP_TRY(ctx, hipMemcpyAsync(b_in.p, in, sizeof(float) * rows * n_in, hipMemcpyHostToDevice, st));
        d_in = b_in.as<float>();
        d_out = b_out.as<float>();
    }
    hipLaunchKernelGGL(resample_rows, dim3(grid_for(rows * n_out, kThreads)), dim3(kThreads), 0, st, d_in, rows, n_in, n_out, d_out);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(float) * rows * n_out, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

void fa_embedding_default_config(fa_embedding_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->window_duration = 10.0;        // OfflineDiarizerTypes.swift:46-55
    cfg->sample_rate = 16000;
    cfg->samples_per_window = 0;        // Int(Double(sampleRate) * windowDuration) (:348-353)
    cfg->overlap_threshold = 1e-3f;     // OfflineEmbeddingExtractor.swift:303
    cfg->exclude_overlap = 1;           // :297-303
    cfg->min_segment_duration = 1.0;
    cfg->batch_size = 32;
    cfg->skip_enabled = 0;              // EmbeddingSkipStrategy.none (:82-105)
    cfg->skip_threshold = 0.95f;        // the recommended maskSimilarity threshold
    cfg->weight_frames = 589;
    cfg->frame_duration = 0.0;          // windowDuration / frames
}

fa_status fa_embedding_plan(fa_ctx *ctx, const fa_embedding_config *cfg, const float *weights, int64_t chunks, int32_t frames, int32_t speakers,
                            const double *offsets, int64_t n_offsets, int64_t total_samples, fa_export_embedding *records, int32_t *run_of_job,
                            int32_t *window_of_run, int64_t *window_start, int32_t *window_chunk, float *run_weights, float *mask_rows,
                            fa_embedding_info *info) {
    return plan(ctx, cfg, weights, chunks, frames, speakers, offsets, n_offsets, total_samples, records, run_of_job, window_of_run, window_start,
                window_chunk, run_weights, mask_rows, info, false);
}

fa_status fa_embedding_plan_dev(fa_ctx *ctx, const fa_embedding_config *cfg, const float *d_weights, int64_t chunks, int32_t frames, int32_t speakers,
                                const double *offsets, int64_t n_offsets, int64_t total_samples, fa_export_embedding *records, int32_t *run_of_job,
                                int32_t *window_of_run, int64_t *window_start, int32_t *window_chunk, float *d_run_weights, float *d_mask_rows,
                                fa_embedding_info *info) {
    return plan(ctx, cfg, d_weights, chunks, frames, speakers, offsets, n_offsets, total_samples, records, run_of_job, window_of_run, window_start,
                window_chunk, d_run_weights, d_mask_rows, info, true);
}

fa_status fa_embedding_windows_dev(fa_ctx *ctx, const float *d_audio, int64_t total_samples, const int64_t *window_start, int64_t count,
                                   int32_t samples_per_window, float *d_out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (count < 0 || total_samples < 0 || samples_per_window <= 0 || (count > 0 && (!window_start || !d_out)) || (count > 0 && total_samples > 0 && !d_audio))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding windows: bad arguments");
    if (count == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "embedding windows", [&]() -> fa_status {
        std::vector<int64_t> sl(static_cast<size_t>(2 * count));   // audio[start : min(start + spw, total)], then zeros (:807-832)
        for (int64_t i = 0; i < count; ++i) {
            const int64_t s = window_start[i];
            if (s < 0 || s > total_samples) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "embedding windows: window %lld starts outside the audio", (long long)i);
            sl[i] = s;
            sl[count + i] = std::min<int64_t>(samples_per_window, total_samples - s);
        }
        fa::DeviceGuard guard(ctx->device);
        hipStream_t st = ctx->stream;
        fa::DevBuf b;
        if (b.alloc(ctx, sizeof(int64_t) * 2 * count) != hipSuccess) { (void)hipGetLastError(); return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "embedding windows: device allocation failed"); }
        FA_HIP_TRY(ctx, hipMemcpyAsync(b.p, sl.data(), sizeof(int64_t) * 2 * count, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(window_rows, dim3(grid_for(count * samples_per_window, kThreads)), dim3(kThreads), 0, st, d_audio, b.as<int64_t>(),
                           b.as<int64_t>() + count, count, samples_per_window, d_out);
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the pageable staging above lives until the copy has been read
        return FA_SUCCESS;
    });
}

fa_status fa_embedding_span_inputs(fa_ctx *ctx, const fa_embedding_config *cfg, const float *audio, int64_t total_samples, const double *spans, int64_t n,
                                   float *windows, float *weights, fa_status *statuses) {
    return span_inputs(ctx, cfg, audio, total_samples, spans, n, windows, weights, statuses, false);
}

fa_status fa_embedding_span_inputs_dev(fa_ctx *ctx, const fa_embedding_config *cfg, const float *d_audio, int64_t total_samples, const double *spans,
                                       int64_t n, float *d_windows, float *d_weights, fa_status *statuses) {
    return span_inputs(ctx, cfg, d_audio, total_samples, spans, n, d_windows, d_weights, statuses, true);
}

fa_status fa_weight_resample(fa_ctx *ctx, const float *in, int64_t rows, int32_t in_frames, int32_t out_frames, float *out) {
    return weight_resample(ctx, in, rows, in_frames, out_frames, out, false);
}

fa_status fa_weight_resample_dev(fa_ctx *ctx, const float *d_in, int64_t rows, int32_t in_frames, int32_t out_frames, float *d_out) {
    return weight_resample(ctx, d_in, rows, in_frames, out_frames, d_out, true);
}

}  // extern "C"
