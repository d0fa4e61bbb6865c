// reconstruct.hip — from segmentation logits and per-chunk cluster labels to speaker segments, on the device.
//
//   * powerset decode (reference: Sources/FluidAudio/Diarizer/Offline/Segmentation/OfflineSegmentationProcessor.swift:316-409):
//     per chunk frame the first strict maximum of the class logits (seeded at -Float.greatestFiniteMagnitude, so NaN never wins and
//     an all-NaN / all--inf row is class 0), winningClass = min(best, 7), binary weights of the speakers of powerset[winningClass]
//     (table :15-24), and optionally the log-probabilities logits - logSumExp(logits) (VDSPOperations.swift:142-155) in fp32.
//   * OfflineReconstruction.buildSegments (Diarizer/Offline/Utils/OfflineReconstruction.swift:24-237): the chunk frames fold into
//     global frames g = round-half-away((offset + f*fd) / fd) (fp64, no FMA), clamped to [0, totalFrames); per global frame the
//     fp64 activation sums / counts per cluster and the expected speaker count are added in increasing chunk, then frame order;
//     count = clamp(rint_even(expSum / weight), 0, min(K, S)); the first `count` clusters by activation sum descending, ties to the
//     lower index (Swift's stable sort); zero-vote frames (count 1, every sum 0, ZeroVoteReembedder.swift:42-79); a caller's
//     zero-vote overrides replace a frame's clusters by [cluster] (:176-186, :249-298).  Then the segment walk (:188-233): every
//     maximal run of frames in which a cluster is active is one raw segment, start g0*fd, end g1*fd when closed at frame g1 and
//     g_last*fd + fd when still open at the last frame, quality = Float(clamp(scoreSum / frames, 0, 1)) with scoreSum the
//     sequential fp64 sum of the run's per-frame averages (:400-429).
//   * mergeSegments / sanitize / excludeOverlaps (:359-398, :431-496) as host code over the compact raw list (one D2H).
//
// Where the reference is not deterministic: raw segments that close at the same frame, and those flushed after the last frame,
// are appended in Swift Dictionary order (hash-seeded), and that order decides merges between speakers whose segments start at the
// same time.  Here the raw order is (closing frame, cluster index ascending); a segment still open after the last frame closes at
// frame totalFrames.
//
// No float atomics: every global frame is owned by one wavefront, which gathers its contributions in the reference's order.
// Non-decreasing chunk offsets (what the segmentation producer emits, offset = c * step) find the chunks covering a tile of global
// frames by binary search; any other offsets (unsorted, duplicated, negative, off-grid) list them with an ordered scan over all
// chunks.  Both visit chunks in increasing index and, per chunk, the frames whose exact forward map is g.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "block_scan.h"
#include "fa_common.h"

namespace {

using fa::grid_for;
using fa::scan::block_exclusive;
constexpr int kThreads = fa::scan::kThreads;
constexpr int kTileG = 64;        // global frames per workgroup of the frame kernel (16 per wavefront)
constexpr int kListCap = 1024;    // chunks of a tile listed in LDS (irregular offsets); more: every wavefront scans all chunks
constexpr int kScanPer = 8;       // items per thread of the run compaction
constexpr int kSelBits = 15;      // per-frame word: [0, 15) clusters active, [15, 30) speakerCountPerFrame, bit 30 zero-vote
constexpr int kSelMask = (1 << kSelBits) - 1;
constexpr int kZeroVote = 1 << 30;

// powerset (OfflineSegmentationProcessor.swift:15-24): [] [0] [1] [2] [0,1] [0,2] [1,2] [0,1,2] as speaker bit masks, one nibble per class
__host__ __device__ inline unsigned powerset_mask(int cls) { return (0x76534210u >> (4 * cls)) & 0xFu; }

// chunk frame -> global frame (:69-77): frameStart = offset + Double(f) * fd (two roundings), rounded half away from zero, clamped
__host__ __device__ inline int global_frame(double offset, int f, double fd, int T) {
    const double fs = offset + static_cast<double>(f) * fd;   // this file is built with -ffp-contract=off: no FMA
    const double r = round(fs / fd);
    if (!(r > 0.0)) return 0;
    if (r >= static_cast<double>(T)) return T - 1;
    return static_cast<int>(r);
}

// ---------------------------------------------------------------- powerset decode

__device__ inline void decode_row(const float *x, int classes, float *w, float *lp) {
    int best = 0;
    float bv = -3.40282347e38f;                              // -Float.greatestFiniteMagnitude (:326-335)
    for (int c = 0; c < classes; ++c) if (x[c] > bv) { bv = x[c]; best = c; }
    const unsigned m = powerset_mask(best < 7 ? best : 7);   // min(bestIndex, powerset.count - 1)
    w[0] = (m & 1u) ? 1.0f : 0.0f;
    w[1] = (m & 2u) ? 1.0f : 0.0f;
    w[2] = (m & 4u) ? 1.0f : 0.0f;
    if (lp && classes > 0) {                                 // logSumExp (VDSPOperations.swift:142-155): log(sum(exp(x - max))) + max
        float mx = x[0];
        for (int c = 1; c < classes; ++c) if (mx < x[c]) mx = x[c];
        float s = 0.0f;
        for (int c = 0; c < classes; ++c) s += expf(x[c] - mx);
        const float lse = logf(s) + mx;
        for (int c = 0; c < classes; ++c) lp[c] = x[c] + (-lse);
    }
}

// 7 classes (the community-1 model): 4 rows = 7 float4 in, 3 float4 of weights and 7 float4 of log-probs out per thread
__global__ __launch_bounds__(kThreads) void powerset_decode7(const float4 *__restrict__ x, int64_t groups, float4 *__restrict__ w, float4 *__restrict__ lp) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= groups) return;
    float v[28], wv[12], lv[28];
#pragma unroll
    for (int k = 0; k < 7; ++k) { const float4 t = x[i * 7 + k]; v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w; }
#pragma unroll
    for (int r = 0; r < 4; ++r) decode_row(v + 7 * r, 7, wv + 3 * r, lp ? lv + 7 * r : nullptr);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[i * 3 + k] = make_float4(wv[4 * k], wv[4 * k + 1], wv[4 * k + 2], wv[4 * k + 3]);
    if (lp) {
#pragma unroll
        for (int k = 0; k < 7; ++k) lp[i * 7 + k] = make_float4(lv[4 * k], lv[4 * k + 1], lv[4 * k + 2], lv[4 * k + 3]);
    }
}

// any class count, one row per thread (also the tail rows of the 7-class kernel)
__global__ __launch_bounds__(kThreads) void powerset_decode_rows(const float *__restrict__ x, int64_t row0, int64_t rows, int classes, float *__restrict__ w,
                                                                 float *__restrict__ lp) {
    const int64_t r = row0 + static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float wv[3];
    if (classes <= 16) {
        float v[16];
        for (int c = 0; c < classes; ++c) v[c] = x[r * classes + c];
        decode_row(v, classes, wv, lp ? lp + r * classes : nullptr);
    } else {
        decode_row(x + r * classes, classes, wv, lp ? lp + r * classes : nullptr);
    }
    w[r * 3] = wv[0];
    w[r * 3 + 1] = wv[1];
    w[r * 3 + 2] = wv[2];
}

// ---------------------------------------------------------------- per-frame accumulation and decision

struct FrameArgs {
    const float *w;          // [C][F][S] speaker weights
    const double *start;     // [C] chunk start times
    const int32_t *first_g;  // [C] global frame of chunk frame 0 / F-1
    const int32_t *last_g;
    const int32_t *hard;     // [C][S] cluster of each local speaker, -1 = none (host-mapped from anything outside [0, K))
    const int32_t *ovr;      // [T] zero-vote override cluster or -1; nullptr: none
    int32_t *word;           // [T] kSelBits fields (see above)
    int32_t *sel;            // [T][smax] active clusters, by rank
    double *avg;             // [T][smax] their activation averages
    int32_t *bad;            // set when a weight is not finite
    double *esum_out;        // [T] the fp64 expected-count sum of each frame, or nullptr (fa_reconstruct_info.expected_count_sums)
    int64_t C;
    int32_t F, S, K, T, smax, maxc, sorted;
    double fd;
};

// first index in [0, n) with a[i] >= v (a non-decreasing)
__device__ inline int64_t lower_bound_i32(const int32_t *a, int64_t n, int v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
    return lo;
}

struct Best { double s; int k; int n; };
// (sum descending, cluster ascending): the order of Swift's stable sort by activation sum (:167-174)
__device__ inline bool better(double s, int k, double bs, int bk) { return s > bs || (s == bs && k < bk); }

// One wavefront per global frame.  Lane l holds the sums / counts of clusters kb + l + 64 i (i < KPL) of the tile kb; K > 64 KPL sweeps
// the contributions once per tile and selected rank.
template <int KPL>
__global__ __launch_bounds__(kThreads) void recon_frames(FrameArgs a) {
    __shared__ int32_t list[kListCap];
    __shared__ int32_t wcnt[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g0 = blockIdx.x * kTileG;
    const int g1 = min(g0 + kTileG, a.T) - 1;
    int64_t clo = 0, chi = a.C;
    int nlist = 0;
    bool use_list = false;
    if (a.sorted) {   // chunks whose frames can land in [g0, g1]: last_g >= g0 and first_g <= g1 (both non-decreasing)
        clo = lower_bound_i32(a.last_g, a.C, g0);
        chi = lower_bound_i32(a.first_g, a.C, g1 + 1);
    } else {          // ordered compaction of the chunks whose [first_g, last_g] meets the tile, in increasing chunk index
        int base = 0;
        for (int64_t c0 = 0; c0 < a.C; c0 += kThreads) {
            const int64_t c = c0 + tid;
            const bool hit = c < a.C && a.first_g[c] <= g1 && a.last_g[c] >= g0;
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wcnt[wid] = __popcll(m);
            __syncthreads();
            int off = base, tot = 0;
            for (int v = 0; v < kThreads / 64; ++v) { if (v < wid) off += wcnt[v]; tot += wcnt[v]; }
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
            if (hit && pos < kListCap) list[pos] = static_cast<int32_t>(c);
            base += tot;
            __syncthreads();
        }
        nlist = base;
        use_list = base <= kListCap;
    }

    for (int g = g0 + wid; g <= g1; g += kThreads / 64) {
        // every (c, f) with global_frame(c, f) == g, in increasing c, then f
        auto visit = [&](auto &&fn) {
            auto chunk = [&](int64_t c) {
                if (a.first_g[c] > g || a.last_g[c] < g) return;
                const double off = a.start[c];
                // first f with global_frame >= g: global_frame(c, f) is first_g + f up to rounding, so try that f before a binary search
                int lo = min(max(g - a.first_g[c], 0), a.F - 1);
                if (!((lo == 0 || global_frame(off, lo - 1, a.fd, a.T) < g) && global_frame(off, lo, a.fd, a.T) >= g)) {
                    int hi = a.F;
                    lo = 0;
                    while (lo < hi) { const int m = (lo + hi) >> 1; if (global_frame(off, m, a.fd, a.T) < g) lo = m + 1; else hi = m; }
                }
                for (int f = lo; f < a.F && global_frame(off, f, a.fd, a.T) == g; ++f) fn(c, f);
            };
            if (a.sorted) for (int64_t c = clo; c < chi; ++c) chunk(c);
            else if (use_list) for (int i = 0; i < nlist; ++i) chunk(list[i]);
            else for (int64_t c = 0; c < a.C; ++c) chunk(c);
        };
        double sum[KPL];
        int cnt[KPL];
        double esum = 0.0;
        int ew = 0, badv = 0;
        auto pass = [&](int kb) {   // :79-104 for the clusters of tile kb
            for (int i = 0; i < KPL; ++i) { sum[i] = 0.0; cnt[i] = 0; }
            esum = 0.0;
            ew = 0;
            visit([&](int64_t c, int f) {
                const float *wr = a.w + (c * a.F + f) * a.S;
                const int32_t *hr = a.hard + c * a.S;
                double act[KPL];
                for (int i = 0; i < KPL; ++i) act[i] = 0.0;
                double e = 0.0;
                for (int s = 0; s < a.S; ++s) {
                    const float v = wr[s];
                    if (!isfinite(v)) badv = 1;
                    const double dv = static_cast<double>(v);
                    e += dv;                                          // expectedCount: sequential over the speakers (:90-92)
                    const int k = hr[s] - kb - lane;                  // == 64 i when this lane holds that cluster
                    if (k >= 0 && (k & 63) == 0) {
#pragma unroll
                        for (int i = 0; i < KPL; ++i) if (k == 64 * i && dv > act[i]) act[i] = dv;   // max over the speakers, strict > from 0
                    }
                }
                esum += e;
                ew += 1;
#pragma unroll
                for (int i = 0; i < KPL; ++i) if (act[i] > 0.0) { sum[i] += act[i]; cnt[i] += 1; }
            });
        };
        // the lane's best cluster of the current tile ranked after (ps, pk), reduced over the wavefront
        auto tile_best = [&](int kb, double ps, int pk, Best &b) {
            Best m{-1.0, INT_MAX, 0};
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int k = kb + lane + 64 * i;
                if (k < a.K && better(ps, pk, sum[i], k) && better(sum[i], k, m.s, m.k)) m = Best{sum[i], k, cnt[i]};
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double os = __shfl_xor(m.s, off);
                const int ok = __shfl_xor(m.k, off), on = __shfl_xor(m.n, off);
                if (better(os, ok, m.s, m.k)) m = Best{os, ok, on};
            }
            if (better(m.s, m.k, b.s, b.k)) b = m;
        };
        const int ovr = a.ovr ? a.ovr[g] : -1;
        const int span = 64 * KPL, tiles = (a.K + span - 1) / span;
        int count = 0, nsel = 0;
        bool touched = false;
        double ps = INFINITY, ovr_avg = 0.0;
        int pk = -1;
        for (int r = 0;; ++r) {
            Best b{-1.0, INT_MAX, 0};
            for (int t = 0; t < tiles; ++t) {
                const int kb = t * span;
                if (tiles > 1 || r == 0) pass(kb);
                if (r == 0 && t == 0) {   // :145-156
                    if (ew > 0) {
                        double x = rint(esum / static_cast<double>(ew));
                        if (x > static_cast<double>(a.maxc)) x = static_cast<double>(a.maxc);
                        count = x > 0.0 ? static_cast<int>(x) : 0;
                    }
                    nsel = ovr >= 0 ? 1 : count;
                }
                if (r == 0) {
                    bool any = false;
#pragma unroll
                    for (int i = 0; i < KPL; ++i) any |= cnt[i] > 0;
                    touched |= __any(any) != 0;
                    if (ovr >= kb && ovr < kb + span) {   // the override's average (0 on a zero-vote frame)
                        const int rel = ovr - kb, owner = rel & 63, slot = rel >> 6;
                        double s = 0.0;
                        int n = 0;
#pragma unroll
                        for (int i = 0; i < KPL; ++i) if (i == slot) { s = sum[i]; n = cnt[i]; }
                        s = __shfl(s, owner);
                        n = __shfl(n, owner);
                        ovr_avg = n > 0 ? s / static_cast<double>(n) : 0.0;
                    }
                }
                if (ovr < 0 && r < count) tile_best(kb, ps, pk, b);
            }
            if (ovr < 0 && r < count) {
                if (lane == 0) {
                    a.sel[static_cast<int64_t>(g) * a.smax + r] = b.k;
                    a.avg[static_cast<int64_t>(g) * a.smax + r] = b.n > 0 ? b.s / static_cast<double>(b.n) : 0.0;   // :107-143
                }
                ps = b.s;
                pk = b.k;
            }
            if (ovr >= 0 || r + 1 >= count) break;
        }
        if (lane == 0) {
            if (ovr >= 0) {
                a.sel[static_cast<int64_t>(g) * a.smax] = ovr;
                a.avg[static_cast<int64_t>(g) * a.smax] = ovr_avg;
            }
            a.word[g] = nsel | (count << kSelBits) | ((count == 1 && !touched) ? kZeroVote : 0);
            if (a.esum_out) a.esum_out[g] = esum;
            if (badv) atomicOr(a.bad, 1);
        }
    }
}

// ---------------------------------------------------------------- segment runs

// slot of cluster k among frame g's active clusters, -1 if inactive
__device__ inline int active_slot(const int32_t *word, const int32_t *sel, int smax, int g, int k) {
    const int n = word[g] & kSelMask;
    const int32_t *s = sel + static_cast<int64_t>(g) * smax;
    for (int j = 0; j < n; ++j) if (s[j] == k) return j;
    return -1;
}

// item e = g * smax + j starts a run: slot j is active at g and its cluster was not active at g - 1
__device__ inline int run_start(const int32_t *word, const int32_t *sel, int smax, int64_t items, int64_t e) {
    if (e >= items) return 0;
    const int g = static_cast<int>(e / smax), j = static_cast<int>(e - static_cast<int64_t>(g) * smax);
    if (j >= (word[g] & kSelMask)) return 0;
    return g == 0 || active_slot(word, sel, smax, g - 1, sel[e]) < 0;
}

__global__ __launch_bounds__(kThreads) void run_count(const int32_t *__restrict__ word, const int32_t *__restrict__ sel, int smax, int64_t items,
                                                      int32_t *__restrict__ bsum) {
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kScanPer;
    int n = 0;
    for (int i = 0; i < kScanPer; ++i) n += run_start(word, sel, smax, items, e0 + i);
    int tot;
    (void)block_exclusive(n, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kThreads) void run_write(const int32_t *__restrict__ word, const int32_t *__restrict__ sel, int smax, int64_t items,
                                                      const int32_t *__restrict__ boff, int64_t *__restrict__ starts) {
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kScanPer;
    int flags = 0, n = 0;
    for (int i = 0; i < kScanPer; ++i) if (run_start(word, sel, smax, items, e0 + i)) { flags |= 1 << i; ++n; }
    int tot;
    int pos = boff[blockIdx.x] + block_exclusive(n, &tot);
    for (int i = 0; i < kScanPer; ++i) if (flags & (1 << i)) starts[pos++] = e0 + i;
}

struct RawRun {
    int32_t g0, g1, k, frames;   // frames [g0, g1) of cluster k
    double score;                // sequential fp64 sum of the per-frame averages (:207-213)
};

// one lane per run: walk forward while the cluster stays active
__global__ __launch_bounds__(kThreads) void run_walk(const int64_t *__restrict__ starts, const int32_t *__restrict__ total, const int32_t *__restrict__ word,
                                                     const int32_t *__restrict__ sel, const double *__restrict__ avg, int smax, int T, RawRun *__restrict__ out) {
    const int n = *total;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e = starts[i];
        const int g0 = static_cast<int>(e / smax), k = sel[e];
        double s = avg[e];
        int g = g0 + 1;
        for (; g < T; ++g) {
            const int j = active_slot(word, sel, smax, g, k);
            if (j < 0) break;
            s += avg[static_cast<int64_t>(g) * smax + j];
        }
        out[i] = RawRun{g0, g, k, g - g0, s};
    }
}

// ---------------------------------------------------------------- host passes

bool same_speaker(const fa_rttm_segment &a, const fa_rttm_segment &b) { return strncmp(a.speaker_id, b.speaker_id, sizeof(a.speaker_id)) == 0; }

// blendedQuality (:465-479)
float blended_quality(const fa_rttm_segment &l, const fa_rttm_segment &r) {
    const double ld = static_cast<double>(l.end_seconds - l.start_seconds), rd = static_cast<double>(r.end_seconds - r.start_seconds);
    const double total = ld + rd;
    if (!(total > 0)) return std::min(std::max((l.quality + r.quality) / 2, 0.0f), 1.0f);
    const double weighted = static_cast<double>(l.quality) * ld + static_cast<double>(r.quality) * rd;
    return static_cast<float>(std::min(std::max(weighted / total, 0.0), 1.0));
}

void stable_by_start(std::vector<fa_rttm_segment> &v) {
    std::stable_sort(v.begin(), v.end(), [](const fa_rttm_segment &x, const fa_rttm_segment &y) { return x.start_seconds < y.start_seconds; });
}

// mergeSegments (:431-463) -> sanitize (:481-496) -> excludeOverlaps (:359-398)
std::vector<fa_rttm_segment> finalize(const fa_reconstruct_config &cfg, std::vector<fa_rttm_segment> raw) {
    std::vector<fa_rttm_segment> merged;
    if (!raw.empty()) {
        const double gap_threshold = std::max(cfg.min_gap_duration, cfg.min_duration_off);
        stable_by_start(raw);
        fa_rttm_segment cur = raw[0];
        for (size_t i = 1; i < raw.size(); ++i) {
            const fa_rttm_segment &s = raw[i];
            if (same_speaker(s, cur) && static_cast<double>(s.start_seconds) - static_cast<double>(cur.end_seconds) <= gap_threshold) {
                const float q = blended_quality(cur, s);
                cur.end_seconds = std::max(cur.end_seconds, s.end_seconds);
                cur.quality = q;
                continue;
            }
            merged.push_back(cur);
            cur = s;
        }
        merged.push_back(cur);
    }
    stable_by_start(merged);
    const float min_dur = std::max(static_cast<float>(cfg.min_segment_duration), static_cast<float>(cfg.min_duration_on));
    std::vector<fa_rttm_segment> kept;
    for (const auto &s : merged) if (s.end_seconds - s.start_seconds >= min_dur) kept.push_back(s);
    if (!cfg.exclusive) return kept;
    std::vector<fa_rttm_segment> out;
    const float min_seg = static_cast<float>(cfg.min_segment_duration);
    for (const auto &s : kept) {
        float start = s.start_seconds;
        const float end = s.end_seconds;
        if (!out.empty() && start < out.back().end_seconds) start = out.back().end_seconds;
        if (start >= end) continue;
        const float dur = end - start;
        if (dur < min_seg) continue;
        const float orig = s.end_seconds - s.start_seconds;
        const float scale = orig > 0 ? dur / orig : 1.0f;
        fa_rttm_segment t = s;
        t.start_seconds = start;
        t.quality = std::max(0.0f, std::min(1.0f, s.quality * scale));
        out.push_back(t);
    }
    return out;
}

fa_status write_segments(fa_ctx *ctx, const std::vector<fa_rttm_segment> &segs, fa_rttm_segment *out, int64_t capacity, int64_t *count) {
    *count = static_cast<int64_t>(segs.size());
    if (!out) return FA_SUCCESS;
    if (capacity < *count) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "reconstruct: output holds %lld of %lld segments", (long long)capacity, (long long)*count);
    std::copy(segs.begin(), segs.end(), out);
    return FA_SUCCESS;
}

void set_info(fa_reconstruct_info *info, int64_t T, int64_t raw, double fd) {
    if (!info) return;
    info->total_frames = T;
    info->raw_segments = raw;
    info->frame_duration = fd;
    info->zero_vote_run_count = 0;
    info->frame_slots = 0;
}

fa_status reconstruct(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *weights, int64_t C, int32_t F, int32_t S, const double *offsets,
                      int64_t n_offsets, const int32_t *hard, int32_t K, const int64_t *overrides, int64_t n_overrides, fa_rttm_segment *out,
                      int64_t capacity, int64_t *count, fa_reconstruct_info *info, bool device_weights) {
    if (!ctx || !cfg || !count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: ctx, config and count are required");
    *count = 0;
    set_info(info, 0, 0, 0.0);
    if (C < 0 || F < 0 || S < 0 || K < 0 || n_offsets < 0 || n_overrides < 0 || capacity < 0 || (C > 0 && F > 0 && S > 0 && !weights) ||
        (n_offsets > 0 && !offsets) || (n_overrides > 0 && !overrides) || S > kSelMask)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: bad arguments");
    if (C == 0 || F == 0) return FA_SUCCESS;                                   // :30
    const double fd = cfg->frame_duration > 0 ? cfg->frame_duration : cfg->window_duration / F;   // OfflineSegmentationProcessor.swift:286
    if (!std::isfinite(fd)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: frame duration is not finite");
    if (!(fd > 0)) return FA_SUCCESS;                                          // :33
    if (C > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "reconstruct: more than 2^31 chunks");
    return fa::no_throw(ctx, "reconstruct", [&]() -> fa_status {
    // chunk starts (:498-507) and the global frame count (:37-47)
    std::vector<double> start(static_cast<size_t>(C));
    double max_time = 0.0;
    bool sorted = true;
    for (int64_t c = 0; c < C; ++c) {
        start[c] = c < n_offsets ? offsets[c] : static_cast<double>(c) * cfg->window_duration;
        if (!std::isfinite(start[c])) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: chunk %lld starts at a non-finite time", (long long)c);
        if (c > 0 && start[c] < start[c - 1]) sorted = false;
        const double end = start[c] + static_cast<double>(F) * fd;
        if (end > max_time) max_time = end;
    }
    const double tf = std::ceil(max_time / fd);
    const int32_t Kc = std::max(K, 1);
    const int32_t maxc = std::min(Kc, S), smax = std::max(maxc, 1);
    if (!(tf < static_cast<double>(INT32_MAX) / smax)) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "reconstruct: %.0f global frames", tf);
    const int32_t T = std::max(1, static_cast<int32_t>(tf));
    set_info(info, T, 0, fd);
    if (info) info->frame_slots = smax;
    std::vector<int32_t> first_g(static_cast<size_t>(C)), last_g(static_cast<size_t>(C));
    for (int64_t c = 0; c < C; ++c) { first_g[c] = global_frame(start[c], 0, fd, T); last_g[c] = global_frame(start[c], F - 1, fd, T); }
    std::vector<int32_t> hard_m(static_cast<size_t>(C * S), -1);
    if (hard) for (int64_t i = 0; i < C * S; ++i) hard_m[i] = hard[i] >= 0 && hard[i] < Kc ? hard[i] : -1;   // :81-83
    std::vector<int32_t> ovr;
    if (n_overrides > 0) {   // :284-286, applied in order
        ovr.assign(static_cast<size_t>(T), -1);
        for (int64_t i = 0; i < n_overrides; ++i) {
            const int64_t lo = overrides[3 * i], hi = overrides[3 * i + 1], k = overrides[3 * i + 2];
            if (lo < 0 || hi < lo || hi > T || k < 0 || k >= Kc) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: override %lld is out of range", (long long)i);
            for (int64_t g = lo; g < hi; ++g) ovr[g] = static_cast<int32_t>(k);
        }
    }

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    const int64_t items = static_cast<int64_t>(T) * smax;
    const int64_t nb = (items + kThreads * kScanPer - 1) / (kThreads * kScanPer);
    const bool want_frames = info && info->frame_capacity >= T && (info->frame_clusters || info->frame_averages || info->expected_count_sums);
    fa::DevBuf b_w, b_start, b_first, b_last, b_hard, b_ovr, b_word, b_sel, b_avg, b_bsum, b_flags, b_starts, b_esum;
    auto alloc = [&](fa::DevBuf &b, size_t bytes) { return b.alloc(ctx, bytes) == hipSuccess; };
    if ((!device_weights && !alloc(b_w, sizeof(float) * C * F * S)) || !alloc(b_start, sizeof(double) * C) || !alloc(b_first, sizeof(int32_t) * C) ||
        !alloc(b_last, sizeof(int32_t) * C) || !alloc(b_hard, sizeof(int32_t) * C * S) || (!ovr.empty() && !alloc(b_ovr, sizeof(int32_t) * T)) ||
        !alloc(b_word, sizeof(int32_t) * T) || !alloc(b_sel, sizeof(int32_t) * items) || !alloc(b_avg, sizeof(double) * items) ||
        !alloc(b_bsum, sizeof(int32_t) * nb) || !alloc(b_flags, sizeof(int32_t) * 2) || !alloc(b_starts, sizeof(int64_t) * items) ||
        (want_frames && info->expected_count_sums && !alloc(b_esum, sizeof(double) * T))) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "reconstruct: device allocation failed");
    }
    const float *d_w = weights;
    if (!device_weights) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(b_w.p, weights, sizeof(float) * C * F * S, hipMemcpyHostToDevice, st));
        d_w = b_w.as<float>();
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_start.p, start.data(), sizeof(double) * C, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_first.p, first_g.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_last.p, last_g.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice, st));
    if (C * S > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_hard.p, hard_m.data(), sizeof(int32_t) * C * S, hipMemcpyHostToDevice, st));
    if (!ovr.empty()) FA_HIP_TRY(ctx, hipMemcpyAsync(b_ovr.p, ovr.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_flags.p, 0, sizeof(int32_t) * 2, st));

    FrameArgs fa_args{d_w, b_start.as<double>(), b_first.as<int32_t>(), b_last.as<int32_t>(), b_hard.as<int32_t>(), ovr.empty() ? nullptr : b_ovr.as<int32_t>(),
                      b_word.as<int32_t>(), b_sel.as<int32_t>(), b_avg.as<double>(), b_flags.as<int32_t>(),
                      b_esum.p ? b_esum.as<double>() : nullptr, C, F, S, Kc, T, smax, maxc, sorted ? 1 : 0, fd};
    const unsigned fgrid = grid_for(T, kTileG);
    if (Kc <= 64) hipLaunchKernelGGL(recon_frames<1>, dim3(fgrid), dim3(kThreads), 0, st, fa_args);
    else hipLaunchKernelGGL(recon_frames<4>, dim3(fgrid), dim3(kThreads), 0, st, fa_args);
    hipLaunchKernelGGL(run_count, dim3(static_cast<unsigned>(nb)), dim3(kThreads), 0, st, b_word.as<int32_t>(), b_sel.as<int32_t>(), smax, items, b_bsum.as<int32_t>());
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(kThreads), 0, st, b_bsum.as<int32_t>(), nb, b_flags.as<int32_t>() + 1);
    hipLaunchKernelGGL(run_write, dim3(static_cast<unsigned>(nb)), dim3(kThreads), 0, st, b_word.as<int32_t>(), b_sel.as<int32_t>(), smax, items,
                       b_bsum.as<int32_t>(), b_starts.as<int64_t>());
    FA_HIP_TRY(ctx, hipGetLastError());
    int32_t flags[2];
    FA_HIP_TRY(ctx, hipMemcpyAsync(flags, b_flags.p, sizeof(flags), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flags[0]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "reconstruct: a speaker weight is not finite (the reference traps in Int(NaN))");
    const int64_t n_raw = flags[1];
    std::vector<RawRun> runs(static_cast<size_t>(n_raw));
    if (n_raw > 0) {
        fa::DevBuf b_raw;
        if (!alloc(b_raw, sizeof(RawRun) * n_raw)) { (void)hipGetLastError(); return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "reconstruct: device allocation failed"); }
        hipLaunchKernelGGL(run_walk, dim3(std::min<unsigned>(grid_for(n_raw, kThreads), 4096)), dim3(kThreads), 0, st, b_starts.as<int64_t>(), b_flags.as<int32_t>() + 1,
                           b_word.as<int32_t>(), b_sel.as<int32_t>(), b_avg.as<double>(), smax, T, b_raw.as<RawRun>());
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipMemcpyAsync(runs.data(), b_raw.p, sizeof(RawRun) * n_raw, hipMemcpyDeviceToHost, st));
    }
    const bool want_counts = info && info->speaker_counts && info->speaker_counts_capacity >= T;
    const bool want_runs = info && info->zero_vote_runs;
    std::vector<int32_t> words, sel;
    std::vector<double> avg;
    if (want_counts || want_runs || want_frames) {
        words.resize(static_cast<size_t>(T));
        FA_HIP_TRY(ctx, hipMemcpyAsync(words.data(), b_word.p, sizeof(int32_t) * T, hipMemcpyDeviceToHost, st));
    }
    if (want_frames) {
        if (info->frame_clusters) { sel.resize(static_cast<size_t>(items)); FA_HIP_TRY(ctx, hipMemcpyAsync(sel.data(), b_sel.p, sizeof(int32_t) * items, hipMemcpyDeviceToHost, st)); }
        if (info->frame_averages) { avg.resize(static_cast<size_t>(items)); FA_HIP_TRY(ctx, hipMemcpyAsync(avg.data(), b_avg.p, sizeof(double) * items, hipMemcpyDeviceToHost, st)); }
        if (info->expected_count_sums) FA_HIP_TRY(ctx, hipMemcpyAsync(info->expected_count_sums, b_esum.p, sizeof(double) * T, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (want_frames) {   // slots past a frame's active clusters were never written on the device: -1 / 0 here
        for (int64_t e = 0; e < items; ++e) {
            const bool live = e % smax < (words[e / smax] & kSelMask);
            if (info->frame_clusters) info->frame_clusters[e] = live ? sel[e] : -1;
            if (info->frame_averages) info->frame_averages[e] = live ? avg[e] : 0.0;
        }
    }
    if (want_counts) for (int32_t g = 0; g < T; ++g) info->speaker_counts[g] = (words[g] >> kSelBits) & kSelMask;
    if (want_runs) {   // ZeroVoteReembedder.detectRuns (:42-79)
        int64_t n = 0;
        auto emit = [&](int64_t lo, int64_t hi) {
            if (!(static_cast<double>(hi - lo) * fd >= cfg->zero_vote_min_duration)) return;
            if (n < info->zero_vote_capacity) { info->zero_vote_runs[2 * n] = lo; info->zero_vote_runs[2 * n + 1] = hi; }
            ++n;
        };
        int64_t run0 = -1;
        for (int32_t g = 0; g < T; ++g) {
            if (words[g] & kZeroVote) { if (run0 < 0) run0 = g; }
            else if (run0 >= 0) { emit(run0, g); run0 = -1; }
        }
        if (run0 >= 0) emit(run0, T);
        info->zero_vote_run_count = n;
    }
    // raw order: (closing frame, cluster) — see the header comment; then the appendSegment records (:400-429)
    std::sort(runs.begin(), runs.end(), [](const RawRun &x, const RawRun &y) { return x.g1 != y.g1 ? x.g1 < y.g1 : x.k < y.k; });
    std::vector<fa_rttm_segment> raw;
    raw.reserve(runs.size());
    for (const RawRun &r : runs) {
        const double s = static_cast<double>(r.g0) * fd;
        const double e = r.g1 < T ? static_cast<double>(r.g1) * fd : static_cast<double>(T - 1) * fd + fd;
        if (!(e > s)) continue;
        fa_rttm_segment seg{};
        seg.start_seconds = static_cast<float>(s);
        seg.end_seconds = static_cast<float>(e);
        seg.quality = static_cast<float>(std::min(std::max(r.score / static_cast<double>(r.frames), 0.0), 1.0));
        snprintf(seg.speaker_id, sizeof(seg.speaker_id), "S%d", r.k + 1);
        raw.push_back(seg);
    }
    if (info) info->raw_segments = static_cast<int64_t>(raw.size());
    return write_segments(ctx, finalize(*cfg, std::move(raw)), out, capacity, count);
    });
}

fa_status powerset_decode(fa_ctx *ctx, const float *logits, int64_t C, int32_t F, int32_t classes, float *weights, float *log_probs, bool device) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (C < 0 || F < 0 || classes < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "powerset decode: negative size");
    const int64_t rows = C * F;
    if (rows == 0) return FA_SUCCESS;
    if ((classes > 0 && !logits) || !weights) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "powerset decode: bad arguments");
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_x, b_w, b_lp;
    const float *d_x = logits;
    float *d_w = weights, *d_lp = log_probs;
    if (!device) {
        if (b_x.alloc(ctx, sizeof(float) * rows * std::max(classes, 1)) != hipSuccess || b_w.alloc(ctx, sizeof(float) * rows * 3) != hipSuccess ||
            (log_probs && b_lp.alloc(ctx, sizeof(float) * rows * std::max(classes, 1)) != hipSuccess)) {
            (void)hipGetLastError();
            return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "powerset decode: device allocation failed");
        }
        if (classes > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_x.p, logits, sizeof(float) * rows * classes, hipMemcpyHostToDevice, st));
        d_x = b_x.as<float>();
        d_w = b_w.as<float>();
        d_lp = log_probs ? b_lp.as<float>() : nullptr;
    }
    const auto aligned = [](const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    int64_t row0 = 0;
    if (classes == 7 && aligned(d_x) && aligned(d_w) && aligned(d_lp)) {
        const int64_t groups = rows / 4;
        if (groups > 0)
            hipLaunchKernelGGL(powerset_decode7, dim3(grid_for(groups, kThreads)), dim3(kThreads), 0, st, reinterpret_cast<const float4 *>(d_x), groups,
                               reinterpret_cast<float4 *>(d_w), reinterpret_cast<float4 *>(d_lp));
        row0 = groups * 4;
    }
    if (row0 < rows)
        hipLaunchKernelGGL(powerset_decode_rows, dim3(grid_for(rows - row0, kThreads)), dim3(kThreads), 0, st, d_x, row0, rows, classes, d_w, d_lp);
    FA_HIP_TRY(ctx, hipGetLastError());
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(weights, d_w, sizeof(float) * rows * 3, hipMemcpyDeviceToHost, st));
        if (log_probs && classes > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(log_probs, d_lp, sizeof(float) * rows * classes, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

void fa_reconstruct_default_config(fa_reconstruct_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->window_duration = 10.0;          // OfflineDiarizerTypes.swift:46-55
    cfg->frame_duration = 0.0;            // windowDuration / frames
    cfg->min_duration_on = 0.0;
    cfg->min_duration_off = 0.0;
    cfg->min_segment_duration = 1.0;      // :97-103
    cfg->min_gap_duration = 0.1;          // :204-214
    cfg->exclusive = 1;
    cfg->zero_vote_enabled = 0;           // :232-247
    cfg->zero_vote_min_duration = 0.4;
}

fa_status fa_powerset_decode_dev(fa_ctx *ctx, const float *d_logits, int64_t chunks, int32_t frames, int32_t classes, float *d_weights, float *d_log_probs) {
    return powerset_decode(ctx, d_logits, chunks, frames, classes, d_weights, d_log_probs, true);
}

fa_status fa_powerset_decode(fa_ctx *ctx, const float *logits, int64_t chunks, int32_t frames, int32_t classes, float *weights, float *log_probs) {
    return powerset_decode(ctx, logits, chunks, frames, classes, weights, log_probs, false);
}

fa_status fa_offline_chunk_assignments(int64_t n, const int32_t *chunk_indices, const int32_t *speaker_indices, const int32_t *labels, int32_t cluster_count,
                                       int32_t chunks, int32_t speakers, int32_t *hard) {
    if (n < 0 || chunks < 0 || speakers < 0 || (n > 0 && (!chunk_indices || !speaker_indices || !labels)) || (static_cast<int64_t>(chunks) * speakers > 0 && !hard))
        return FA_INVALID_ARGUMENT;
    for (int64_t i = 0; i < static_cast<int64_t>(chunks) * speakers; ++i) hard[i] = -2;   // OfflineDiarizerManager.swift:891-894
    for (int64_t i = 0; i < n; ++i) {                                                       // :896-908, later embeddings overwrite
        const int32_t c = chunk_indices[i], s = speaker_indices[i], k = labels[i];
        if (c < 0 || c >= chunks || s < 0 || s >= speakers || k < 0 || k >= cluster_count) continue;
        hard[static_cast<int64_t>(c) * speakers + s] = k;
    }
    return FA_SUCCESS;
}

fa_status fa_offline_reconstruct_dev(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *d_weights, int64_t chunks, int32_t frames, int32_t speakers,
                                     const double *offsets, int64_t n_offsets, const int32_t *hard, int32_t clusters, const int64_t *overrides,
                                     int64_t n_overrides, fa_rttm_segment *out, int64_t capacity, int64_t *count, fa_reconstruct_info *info) {
    return reconstruct(ctx, cfg, d_weights, chunks, frames, speakers, offsets, n_offsets, hard, clusters, overrides, n_overrides, out, capacity, count, info, true);
}

fa_status fa_offline_reconstruct(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *weights, int64_t chunks, int32_t frames, int32_t speakers,
                                 const double *offsets, int64_t n_offsets, const int32_t *hard, int32_t clusters, const int64_t *overrides,
                                 int64_t n_overrides, fa_rttm_segment *out, int64_t capacity, int64_t *count, fa_reconstruct_info *info) {
    return reconstruct(ctx, cfg, weights, chunks, frames, speakers, offsets, n_offsets, hard, clusters, overrides, n_overrides, out, capacity, count, info, false);
}

fa_status fa_segments_finalize(const fa_reconstruct_config *cfg, const fa_rttm_segment *raw, int64_t n, fa_rttm_segment *out, int64_t capacity, int64_t *count) {
    if (!cfg || !count || n < 0 || capacity < 0 || (n > 0 && !raw)) return FA_INVALID_ARGUMENT;
    *count = 0;
    return fa::no_throw(nullptr, "segments finalize", [&]() -> fa_status {
        return write_segments(nullptr, finalize(*cfg, std::vector<fa_rttm_segment>(raw, raw + n)), out, capacity, count);
    });
}

}  // extern "C"
