// der.hip — frame-wise diarization error rate with the optimal speaker mapping, batched over recordings: DiarizationDER.compute
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
#include <algorithm>
#include <cmath>

#include "fa_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxLabels = FA_DER_MAX_LABELS;
constexpr int kRasterLanes = 8;          // lanes that share one range in der_raster
constexpr int kOverlapTileWords = 256;   // words per workgroup of der_overlap: one 64-word chunk per wavefront
constexpr int kAccWordsPerWave = 8;      // consecutive words a wavefront of der_accumulate sums before it reduces
constexpr int kAccTileWords = kAccWordsPerWave * (kThreads / kWave);

static_assert(kMaxLabels == kWave, "der_assign gives every column a lane and der_accumulate keeps a label set in one 64-bit word");

struct DerRec {
    int64_t ref_begin, ref_end, hyp_begin, hyp_end;   // the recording's segments in the concatenated lists
    int64_t plane_off;                                // first word of its planes: R ref planes, H hyp planes, the excluded plane
    int64_t ov_off;                                   // first entry of its [H][R] overlap table
    int32_t words, num_frames, R, H;
};

struct DerArgs {
    const fa_der_segment *ref, *hyp;
    const DerRec *rec;
    unsigned long long *planes;
    unsigned long long *overlap;   // int64 counts, added as unsigned
    unsigned long long *acc;       // [B][4]: miss, false alarm, confusion, ref
    int32_t *mapping;              // [B][kMaxLabels]
    int64_t n_ref, n_hyp;
    int32_t B;
    double step, collar;
};

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

// The argument pass: labels, times, and with them the geometry of :61-86.  Nothing here touches the device.
fa_status der_geometry(fa_ctx *ctx, const fa_der_config *cfg, const fa_der_segment *ref, const int64_t *ref_range, const fa_der_segment *hyp,
                       const int64_t *hyp_range, int32_t B, std::vector<DerRec> &rec, int64_t &plane_words, int64_t &ov_entries) {
    plane_words = 0;
    ov_entries = 0;
    for (int32_t b = 0; b < B; ++b) {
        DerRec &r = rec[b];
        r = DerRec{ref_range[b], ref_range[b + 1], hyp_range[b], hyp_range[b + 1], plane_words, ov_entries, 0, 0, 0, 0};
        if (r.ref_begin < 0 || r.ref_end < r.ref_begin || r.hyp_begin < 0 || r.hyp_end < r.hyp_begin)
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: the segment ranges of recording %d do not ascend", b);
        if ((r.ref_end > r.ref_begin && !ref) || (r.hyp_end > r.hyp_begin && !hyp)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: segments are required");
        double max_end = 0.0;
        int32_t labels[2] = {0, 0};
        for (int side = 0; side < 2; ++side) {
            const fa_der_segment *s = side ? hyp : ref;
            for (int64_t i = side ? r.hyp_begin : r.ref_begin, e = side ? r.hyp_end : r.ref_end; i < e; ++i) {
                if (!std::isfinite(s[i].start) || !std::isfinite(s[i].end))
                    return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: recording %d has a segment with a non-finite time", b);
                if (s[i].label < 0 || s[i].label >= kMaxLabels)
                    return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: recording %d has label %d; a side holds at most %d labels, numbered from 0", b, s[i].label,
                                         kMaxLabels);
                labels[side] = std::max(labels[side], s[i].label + 1);
                max_end = std::max(max_end, s[i].end);   // degenerate segments count too (:72, :79)
            }
        }
        r.R = labels[0];
        r.H = labels[1];
        if (r.R == 0 && r.H == 0) continue;   // :82-86: every output is zero
        const double frames = std::ceil(max_end / cfg->frame_step) + 1.0;
        if (!(frames < 2147483584.0)) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "der: recording %d has 2^31 frames or more", b);
        r.num_frames = static_cast<int32_t>(frames);
        r.words = (r.num_frames + 63) / 64;
        plane_words += static_cast<int64_t>(r.words) * (r.R + r.H + 1);
        ov_entries += static_cast<int64_t>(r.R) * r.H;
    }
    return FA_SUCCESS;
}

fa_status der_score(fa_ctx *ctx, const fa_der_config *cfg, const fa_der_segment *ref, const int64_t *ref_range, const fa_der_segment *hyp,
                    const int64_t *hyp_range, int32_t B, fa_der_counts *counts, int32_t *mapping, const int64_t *mapping_range, int64_t *overlap,
                    int64_t overlap_capacity) {
    if (!ctx || !cfg) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: ctx and config are required");
    if (!(cfg->frame_step > 0.0) || !std::isfinite(cfg->frame_step) || !(cfg->collar >= 0.0) || !std::isfinite(cfg->collar))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: frame_step must be positive and finite, collar non-negative and finite");
    if (B < 0 || overlap_capacity < 0 || (B > 0 && (!ref_range || !hyp_range || !counts || !mapping_range)))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: bad arguments");
    if (B == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "der", [&]() -> fa_status {
    std::vector<DerRec> rec(static_cast<size_t>(B));
    int64_t plane_words = 0, ov_entries = 0;
    FA_TRY(der_geometry(ctx, cfg, ref, ref_range, hyp, hyp_range, B, rec, plane_words, ov_entries));
    int32_t max_words = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t room = mapping_range[b + 1] - mapping_range[b];
        if (mapping_range[b] < 0 || room < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: the mapping range of recording %d does not ascend", b);
        if (room < rec[b].H) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "der: recording %d has %d hypothesis labels, its mapping range holds %lld", b, rec[b].H, (long long)room);
        if (room > 0 && !mapping) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: mapping is required");
        max_words = std::max(max_words, rec[b].words);
    }
    if (overlap && overlap_capacity < ov_entries)
        return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "der: the overlap tables take %lld entries, the output holds %lld", (long long)ov_entries, (long long)overlap_capacity);
    const int64_t n_ref = ref_range[B], n_hyp = hyp_range[B], r0 = ref_range[0], h0 = hyp_range[0];
    for (int32_t b = 0; b < B; ++b) {
        counts[b] = fa_der_counts{rec[b].num_frames, 0, 0, 0, 0, rec[b].R, rec[b].H};
        for (int64_t i = mapping_range[b]; i < mapping_range[b + 1]; ++i) mapping[i] = -1;
        rec[b].ref_begin -= r0; rec[b].ref_end -= r0; rec[b].hyp_begin -= h0; rec[b].hyp_end -= h0;   // the upload starts at the first segment used
    }
    if (plane_words == 0) return FA_SUCCESS;   // no recording has a label
    const int64_t items = (n_ref - r0) + (n_hyp - h0) + (cfg->collar > 0.0 ? 2 * (n_ref - r0) : 0);
    const int64_t raster_blocks = (items * kRasterLanes + kThreads - 1) / kThreads;
    if (raster_blocks >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "der: %lld segments", (long long)items);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_ref, b_hyp, b_rec, b_planes, b_work;
    auto alloc = [&](fa::DevBuf &b, size_t bytes) { return b.alloc(ctx, bytes) == hipSuccess; };
    // b_work: the overlap tables, the accumulators, then the mappings — what comes back to the host, in one buffer
    const size_t ov_bytes = sizeof(int64_t) * ov_entries, acc_bytes = sizeof(int64_t) * 4 * B, map_bytes = sizeof(int32_t) * kMaxLabels * static_cast<size_t>(B);
    if (!alloc(b_ref, sizeof(fa_der_segment) * (n_ref - r0)) || !alloc(b_hyp, sizeof(fa_der_segment) * (n_hyp - h0)) || !alloc(b_rec, sizeof(DerRec) * B) ||
        !alloc(b_planes, sizeof(uint64_t) * plane_words) || !alloc(b_work, ov_bytes + acc_bytes + map_bytes)) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "der: device allocation failed");
    }
    if (n_ref > r0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_ref.p, ref + r0, sizeof(fa_der_segment) * (n_ref - r0), hipMemcpyHostToDevice, st));
    if (n_hyp > h0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_hyp.p, hyp + h0, sizeof(fa_der_segment) * (n_hyp - h0), hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_rec.p, rec.data(), sizeof(DerRec) * B, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_planes.p, 0, sizeof(uint64_t) * plane_words, st));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_work.p, 0, ov_bytes + acc_bytes, st));   // der_assign writes every mapping entry it owns
    char *work = b_work.as<char>();
    DerArgs a{b_ref.as<fa_der_segment>(), b_hyp.as<fa_der_segment>(), b_rec.as<DerRec>(), b_planes.as<unsigned long long>(),
              reinterpret_cast<unsigned long long *>(work), reinterpret_cast<unsigned long long *>(work + ov_bytes),
              reinterpret_cast<int32_t *>(work + ov_bytes + acc_bytes), n_ref - r0, n_hyp - h0, B, cfg->frame_step, cfg->collar};
    if (items > 0) hipLaunchKernelGGL(der_raster, dim3(static_cast<unsigned>(raster_blocks)), dim3(kThreads), 0, st, a, items);
    if (ov_entries > 0)
        hipLaunchKernelGGL(der_overlap, dim3((max_words + kOverlapTileWords - 1) / kOverlapTileWords, B), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(der_assign, dim3(B), dim3(kWave), 0, st, a);
    hipLaunchKernelGGL(der_accumulate, dim3((max_words + kAccTileWords - 1) / kAccTileWords, B), dim3(kThreads), 0, st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int64_t> h_acc(static_cast<size_t>(4) * B);
    std::vector<int32_t> h_map(static_cast<size_t>(kMaxLabels) * B);
    if (overlap && ov_entries > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(overlap, work, ov_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(h_acc.data(), work + ov_bytes, acc_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(h_map.data(), work + ov_bytes + acc_bytes, map_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    for (int32_t b = 0; b < B; ++b) {
        counts[b].miss = h_acc[4 * b + 0];
        counts[b].false_alarm = h_acc[4 * b + 1];
        counts[b].confusion = h_acc[4 * b + 2];
        counts[b].ref = h_acc[4 * b + 3];
        for (int32_t h = 0; h < rec[b].H; ++h) mapping[mapping_range[b] + h] = h_map[static_cast<size_t>(kMaxLabels) * b + h];
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_der_default_config(fa_der_config *cfg) {
    if (!cfg) return;
    cfg->frame_step = 0.01;   // DiarizationDER.compute's defaults (:55-56)
    cfg->collar = 0.0;
}

fa_status fa_der_score_batch(fa_ctx *ctx, const fa_der_config *cfg, const fa_der_segment *ref_segs, const int64_t *ref_range, const fa_der_segment *hyp_segs,
                             const int64_t *hyp_range, int32_t batch, fa_der_counts *counts, int32_t *mapping, const int64_t *mapping_range, int64_t *overlap,
                             int64_t overlap_capacity) {
    return der_score(ctx, cfg, ref_segs, ref_range, hyp_segs, hyp_range, batch, counts, mapping, mapping_range, overlap, overlap_capacity);
}

}  // extern "C"
