// der.hip — the kernels of the frame-wise diarization error rate with the optimal speaker mapping, batched over recordings (entries:
// der_host.hip, argument pass and plan: der_geom.h, operands: der_launch.h): DiarizationDER.compute
// (Sources/FluidAudio/Diarizer/DiarizationDER.swift:52-231) and the integer Kuhn-Munkres it calls (Diarizer/HungarianAssignment.swift:8-61).
// Every quantity is an integer count, so the result is pinned bit for bit; the fp64 arithmetic is one division, one subtraction and a
// ceil / floor per range end (this unit is built with -ffp-contract=off like the other restatements).
//
// A label's activity is a BIT PLANE: one uint64 word per 64 frames.  Per recording: R reference planes, H hypothesis planes and one
// "excluded" plane for the collar, each ceil(numFrames / 64) words.
//   der_raster      segments and collar boundaries -> bits (atomicOr: order-independent, hence deterministic)
//   der_overlap     O[h][r] += popc(hyp[h][w] & ref[r][w]): wave sums -> LDS table -> the recording's int64 table
//   der_assign      HungarianAssignment.solve, one wavefront per recording (lane j - 1 owns column j)
//   der_accumulate  lane = frame: miss / false alarm / confusion / reference counts -> int64 atomicAdd
// The geometry (label counts, maxEnd, numFrames, word offsets) is decided by the host in the pass that validates the arguments: that
// pass has to read every segment before any device work anyway, and the planes have to be sized before the call's one synchronisation.
#include "der_launch.h"

namespace {

using namespace fa::der;

// max(0, min(limit, Int(x))) for an x that is already integral (a ceil or a floor) or infinite, without converting what does not fit
__device__ inline int32_t clamp_frame(const double x, const int32_t limit) {
    if (!(x > 0.0)) return 0;
    if (x >= static_cast<double>(limit)) return limit;
    return static_cast<int32_t>(x);
}

__device__ inline int32_t recording_of(const DerRec *rec, const int32_t B, const int64_t i, const bool hyp) {
    int32_t lo = 0, hi = B - 1;   // the first recording whose end is past i: a recording without segments on this side is passed over
    while (lo < hi) {
        const int32_t mid = (lo + hi) / 2;
        const int64_t end = hyp ? rec[mid].hyp_end : rec[mid].ref_end;
        if (i < end) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Items: the reference segments, the hypothesis segments, then (collar > 0) two boundaries per reference segment.  kRasterLanes lanes
// share an item and stride over the words its range [t0, t1) touches.
__global__ __launch_bounds__(kThreads) void der_raster(const DerArgs a, const int64_t items) {
    const int64_t item = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / kRasterLanes;
    const int sub = threadIdx.x % kRasterLanes;
    if (item >= items) return;
    const bool is_hyp = item >= a.n_ref && item < a.n_ref + a.n_hyp;
    const bool is_collar = item >= a.n_ref + a.n_hyp;
    const int64_t si = is_collar ? (item - a.n_ref - a.n_hyp) / 2 : (is_hyp ? item - a.n_ref : item);
    const fa_der_segment s = is_hyp ? a.hyp[si] : a.ref[si];
    if (!(s.end > s.start)) return;
    const DerRec r = a.rec[recording_of(a.rec, a.B, si, is_hyp)];
    int32_t t0, t1, plane;
    if (is_collar) {
        const double half = a.collar / 2.0;
        const double b = ((item - a.n_ref - a.n_hyp) & 1) ? s.end : s.start;
        t0 = clamp_frame(floor((b - half) / a.step), r.num_frames);
        t1 = clamp_frame(ceil((b + half) / a.step), r.num_frames);
        plane = r.R + r.H;
    } else {
        t0 = clamp_frame(ceil(s.start / a.step - 0.5), r.num_frames);
        t1 = clamp_frame(ceil(s.end / a.step - 0.5), r.num_frames);
        plane = is_hyp ? r.R + s.label : s.label;
    }
    if (t1 <= t0) return;
    unsigned long long *p = a.planes + r.plane_off + static_cast<int64_t>(plane) * r.words;
    const int32_t w0 = t0 >> 6, w1 = (t1 - 1) >> 6;   // w1 < r.words: t1 <= num_frames
    for (int32_t w = w0 + sub; w <= w1; w += kRasterLanes) {
        unsigned long long m = ~0ull;
        if (w == w0) m &= ~0ull << (t0 & 63);
        if (w == w1) m &= ~0ull >> (63 - ((t1 - 1) & 63));
        atomicOr(p + w, m);
    }
}

__device__ inline int32_t wave_sum(int32_t v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (tiles, B).  Wavefront k of a workgroup owns words [tile * 256 + 64 k, + 64): lane = word, so a (h, r) pair costs two coalesced
// loads, a popc and a wave sum.  Counted over all frames, before the collar (:96-110).
__global__ __launch_bounds__(kThreads) void der_overlap(const DerArgs a) {
    __shared__ int32_t table[kMaxLabels * kMaxLabels];   // a tile holds 2^14 frames: no entry overflows
    const DerRec r = a.rec[blockIdx.y];
    const int32_t P = r.H * r.R;
    const int32_t tile0 = static_cast<int32_t>(blockIdx.x) * kOverlapTileWords;
    if (P == 0 || tile0 >= r.words) return;
    for (int32_t p = threadIdx.x; p < P; p += kThreads) table[p] = 0;
    __syncthreads();
    const int lane = threadIdx.x % kWave;
    const int32_t w = tile0 + (threadIdx.x / kWave) * kWave + lane;
    const bool in = w < r.words;
    const unsigned long long *ref = a.planes + r.plane_off, *hyp = ref + static_cast<int64_t>(r.R) * r.words;
    if (tile0 + (threadIdx.x / kWave) * kWave < r.words) {   // wave-uniform
        for (int32_t h = 0; h < r.H; ++h) {
            const unsigned long long hw = in ? hyp[static_cast<int64_t>(h) * r.words + w] : 0ull;
            if (!__any(hw != 0ull)) continue;
            for (int32_t q = 0; q < r.R; ++q) {
                const unsigned long long rw = in ? ref[static_cast<int64_t>(q) * r.words + w] : 0ull;
                const int32_t c = wave_sum(__popcll(hw & rw));
                if (lane == 0 && c) atomicAdd(&table[h * r.R + q], c);
            }
        }
    }
    __syncthreads();
    for (int32_t p = threadIdx.x; p < P; p += kThreads)
        if (table[p]) atomicAdd(a.overlap + r.ov_off + p, static_cast<unsigned long long>(table[p]));
}

__device__ inline int64_t wave_min64(int64_t v) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const int lo = __shfl_xor(static_cast<int>(v & 0xffffffffll), o), hi = __shfl_xor(static_cast<int>(v >> 32), o);
        const int64_t x = (static_cast<int64_t>(hi) << 32) | static_cast<uint32_t>(lo);
        v = x < v ? x : v;
    }
    return v;
}

// HungarianAssignment.solve (:8-61) on cost = maxO - O padded to n x n with maxO (:114-123), one wavefront per recording.  Lane j - 1 holds
// column j's v, p, way, minv and used; column 0 (v[0] is never read), p[0] and the row potentials' index are wave-uniform, u lives in LDS.
// The sequential scan keeps the LOWEST j among equal minv (strict <): the wave minimum, then the lowest lane that holds it.
__global__ __launch_bounds__(kWave) void der_assign(const DerArgs a) {
    __shared__ int64_t u[kMaxLabels + 1];
    __shared__ int32_t col_of_row[kMaxLabels + 1];
    const DerRec r = a.rec[blockIdx.x];
    const int lane = threadIdx.x;
    int32_t *map = a.mapping + static_cast<int64_t>(blockIdx.x) * kMaxLabels;
    const int32_t n = max(r.H, r.R);
    const int64_t *O = reinterpret_cast<const int64_t *>(a.overlap) + r.ov_off;
    if (n == 0) return;
    int64_t maxO = 0;   // overlap.max() ?? 0
    for (int32_t p = lane; p < r.H * r.R; p += kWave) maxO = max(maxO, O[p]);
    maxO = -wave_min64(-maxO);
    const int64_t INF = INT64_MAX / 4;
    const bool col = lane < n;   // this lane owns column lane + 1
    int64_t v = 0, minv = 0;
    int32_t p = 0, way = 0, p0 = 0;
    bool used = false;
    u[lane] = 0;
    if (lane == 0) u[kMaxLabels] = 0;
    __syncthreads();
    for (int32_t i = 1; i <= n; ++i) {
        p0 = i;
        int32_t j0 = 0;
        minv = INF;
        used = false;
        int32_t pj0, pass = 0;   // a row's search uses a new column per pass, its walk back visits each at most once: `pass` only bounds a corrupted state
        do {
            if (j0 > 0 && lane == j0 - 1) used = true;
            const int32_t i0 = j0 == 0 ? p0 : __shfl(p, j0 - 1);
            const int64_t ui0 = u[i0];
            if (col && !used) {
                const int64_t c = (i0 - 1 < r.H && lane < r.R) ? maxO - O[static_cast<int64_t>(i0 - 1) * r.R + lane] : maxO;
                const int64_t cur = c - ui0 - v;
                if (cur < minv) { minv = cur; way = j0; }
            }
            const int64_t mine = (col && !used) ? minv : INT64_MAX;
            const int64_t delta = wave_min64(mine);
            const int32_t j1 = __ffsll(static_cast<unsigned long long>(__ballot(mine == delta)));   // lowest lane + 1 = its column
            __syncthreads();   // every lane has read u[i0]
            if (lane == 0) u[p0] += delta;   // column 0 is used from the first pass on
            if (col) {
                if (used) { u[p] += delta; v -= delta; } else minv -= delta;   // used columns hold distinct rows: no two lanes share a u
            }
            __syncthreads();
            j0 = j1;
            pj0 = __shfl(p, j0 - 1);
        } while (pj0 != 0 && ++pass <= n);
        pass = 0;
        do {
            const int32_t j1 = __shfl(way, j0 - 1);
            const int32_t pj1 = j1 == 0 ? p0 : __shfl(p, j1 - 1);
            if (lane == j0 - 1) p = pj1;
            j0 = j1;
        } while (j0 != 0 && ++pass <= n);
    }
    // assign[p[j] - 1] = j - 1; the pair is kept when r < R and O[h][r] > 0 (:125-130)
    if (col) col_of_row[p] = lane;   // a perfect matching: every row 1 ... n is some column's p
    __syncthreads();
    if (lane < r.H) {
        const int32_t c = col_of_row[lane + 1];
        map[lane] = (c < r.R && O[static_cast<int64_t>(lane) * r.R + c] > 0) ? c : -1;
    }
}

// grid (tiles, B); a wavefront takes kAccWordsPerWave consecutive words, lane = frame.  The R + H + 1 plane words of a word are
// wave-uniform loads; a lane collects its reference set, its hypothesis set and the set of references its active hypotheses map to.
__global__ __launch_bounds__(kThreads) void der_accumulate(const DerArgs a) {
    const DerRec r = a.rec[blockIdx.y];
    const int lane = threadIdx.x % kWave;
    const int32_t w_begin = (static_cast<int32_t>(blockIdx.x) * (kThreads / kWave) + threadIdx.x / kWave) * kAccWordsPerWave;
    if (w_begin >= r.words) return;   // wave-uniform
    const int32_t w_end = min(w_begin + kAccWordsPerWave, r.words);
    const unsigned long long *ref = a.planes + r.plane_off, *hyp = ref + static_cast<int64_t>(r.R) * r.words;
    const unsigned long long *excl = hyp + static_cast<int64_t>(r.H) * r.words;
    const int32_t *map = a.mapping + static_cast<int64_t>(blockIdx.y) * kMaxLabels;
    int32_t miss = 0, fa = 0, conf = 0, nref_sum = 0;
    for (int32_t w = w_begin; w < w_end; ++w) {
        if ((excl[w] >> lane) & 1ull) continue;   // bits at and beyond numFrames are never set in any plane: those lanes add zeros
        unsigned long long ref_set = 0, hyp_set = 0, mapped = 0;
        for (int32_t q = 0; q < r.R; ++q) ref_set |= ((ref[static_cast<int64_t>(q) * r.words + w] >> lane) & 1ull) << q;
        for (int32_t h = 0; h < r.H; ++h) {
            const unsigned long long on = (hyp[static_cast<int64_t>(h) * r.words + w] >> lane) & 1ull;
            const int32_t m = map[h];
            hyp_set |= on << h;
            if (on && m >= 0) mapped |= 1ull << m;
        }
        const int32_t n_ref = __popcll(ref_set), n_sys = __popcll(hyp_set), n_correct = __popcll(ref_set & mapped);
        miss += max(0, n_ref - n_sys);
        fa += max(0, n_sys - n_ref);
        conf += min(n_ref, n_sys) - n_correct;
        nref_sum += n_ref;
    }
    miss = wave_sum(miss);
    fa = wave_sum(fa);
    conf = wave_sum(conf);
    nref_sum = wave_sum(nref_sum);
    if (lane == 0) {
        unsigned long long *acc = a.acc + static_cast<int64_t>(blockIdx.y) * 4;
        if (miss) atomicAdd(acc + 0, static_cast<unsigned long long>(miss));
        if (fa) atomicAdd(acc + 1, static_cast<unsigned long long>(fa));
        if (conf) atomicAdd(acc + 2, static_cast<unsigned long long>(conf));
        if (nref_sum) atomicAdd(acc + 3, static_cast<unsigned long long>(nref_sum));
    }
}

}  // namespace

namespace fa {
namespace der {

void launch_raster(hipStream_t stream, const DerArgs &a, const Plan &plan) {
    if (plan.items > 0) hipLaunchKernelGGL(der_raster, dim3(static_cast<unsigned>(plan.raster_blocks)), dim3(kThreads), 0, stream, a, plan.items);
}

void launch_overlap(hipStream_t stream, const DerArgs &a, const Plan &plan) {
    if (plan.ov_entries > 0)
        hipLaunchKernelGGL(der_overlap, dim3((plan.max_words + kOverlapTileWords - 1) / kOverlapTileWords, a.B), dim3(kThreads), 0, stream, a);
}

void launch_assign(hipStream_t stream, const DerArgs &a) { hipLaunchKernelGGL(der_assign, dim3(a.B), dim3(kWave), 0, stream, a); }

void launch_accumulate(hipStream_t stream, const DerArgs &a, const Plan &plan) {
    hipLaunchKernelGGL(der_accumulate, dim3((plan.max_words + kAccTileWords - 1) / kAccTileWords, a.B), dim3(kThreads), 0, stream, a);
}

}  // namespace der
}  // namespace fa
