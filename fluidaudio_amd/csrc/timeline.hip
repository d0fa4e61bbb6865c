// timeline.hip — the timeline shared by the frame-based diarizers (offline and streaming Sortformer, LS-EEND), on the device.
//
// Timeline segments (reference: Sources/FluidAudio/Diarizer/DiarizerTimeline.swift:945-1003, 1169-1336): rebuild(finalizedPredictions:
// tentativePredictions:keepingSpeakers:false,isComplete:).  The onset / offset hysteresis is a map {silent, speaking} -> {silent, speaking}
// per frame; maps compose associatively, so the state before every frame is a scan over 2-bit maps (exact).  Onset frames are compacted
// with block_scan.h in (recording, speaker, frame) order, one lane per raw run walks it for its sequential fp32 activity sum, and one lane
// per (recording, speaker) runs the reference's merge logic over its raw runs.  fluidaudio_amd/der.py scores the records this unit writes.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "block_scan.h"
#include "fa_common.h"

namespace {

using fa::grid_for;
using fa::scan::block_exclusive;
constexpr int kThreads = fa::scan::kThreads;
constexpr int kPer = 8;             // frames per thread of the state scan
constexpr int kTile = kThreads * kPer;

struct TlRec { int64_t fin_off, tent_off; int32_t nf, nt; };   // frame offsets into the two prediction arrays; frames of this recording

struct TlArgs {
    const float *fin, *tent;
    const TlRec *rec;          // [B]
    uint8_t *tile;             // [Q][max_tiles]: the composed map of a tile, then (tl_tile_state) the state at its start
    int32_t *bsum;             // [Q * max_tiles] onsets of a tile, then their exclusive offsets
    int32_t S, max_tiles;
    float onset, offset;
};

// a map {silent, speaking} -> {silent, speaking}: bit 0 = image of silent, bit 1 = image of speaking
constexpr unsigned kIdentity = 2u;
__device__ inline unsigned frame_map(float a, float onset, float offset) { return (a > onset ? 1u : 0u) | (a >= offset ? 2u : 0u); }   // NaN: neither
__device__ inline unsigned then(unsigned f, unsigned g) { return ((g >> (f & 1u)) & 1u) | (((g >> ((f >> 1) & 1u)) & 1u) << 1); }   // g after f

__device__ inline float tl_value(const TlArgs &a, const TlRec &rc, int s, int64_t i) {
    return i < rc.nf ? a.fin[(rc.fin_off + i) * a.S + s] : a.tent[(rc.tent_off + (i - rc.nf)) * a.S + s];
}

// The workgroup's tile of one (recording, speaker): each thread loads its kPer frames into v (n of them) and gets the map of everything
// in the tile before its first frame; *tile_map = the whole tile's map.
__device__ inline unsigned tile_prefix(const TlArgs &a, const TlRec &rc, int s, int64_t i0, float *v, int *n, unsigned *tile_map) {
    __shared__ unsigned wmap[kThreads / 64];
    const int64_t len = static_cast<int64_t>(rc.nf) + rc.nt;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned m = kIdentity;
    int cnt = 0;
    for (int k = 0; k < kPer; ++k) {
        if (i0 + k < len) { v[k] = tl_value(a, rc, s, i0 + k); m = then(m, frame_map(v[k], a.onset, a.offset)); ++cnt; }
    }
    *n = cnt;
    unsigned x = m;   // inclusive scan over the wavefront
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned y = __shfl_up(x, off); if (lane >= off) x = then(y, x); }
    if (lane == 63) wmap[wid] = x;
    unsigned ex = __shfl_up(x, 1);
    if (lane == 0) ex = kIdentity;
    __syncthreads();
    unsigned base = kIdentity, tot = kIdentity;
    for (int w = 0; w < kThreads / 64; ++w) { if (w < wid) base = then(base, wmap[w]); tot = then(tot, wmap[w]); }
    __syncthreads();
    *tile_map = tot;
    return then(base, ex);
}

// workgroup (q, t): mode 0 writes the tile's map; mode 1 counts its onsets (state at the tile's start known); mode 2 writes them
__global__ __launch_bounds__(kThreads) void tl_tiles(TlArgs a, int mode, int32_t *__restrict__ starts) {
    const int64_t blk = blockIdx.x;
    const int64_t q = blk / a.max_tiles;
    const int t = static_cast<int>(blk - q * a.max_tiles);
    const int r = static_cast<int>(q / a.S), s = static_cast<int>(q - static_cast<int64_t>(r) * a.S);
    const TlRec rc = a.rec[r];
    const int64_t len = static_cast<int64_t>(rc.nf) + rc.nt;
    const bool live = static_cast<int64_t>(t) * kTile < len;   // uniform over the workgroup
    float v[kPer];
    int n = 0;
    unsigned tile_map = kIdentity, pre = kIdentity;
    const int64_t i0 = static_cast<int64_t>(t) * kTile + static_cast<int64_t>(threadIdx.x) * kPer;
    if (live) pre = tile_prefix(a, rc, s, i0, v, &n, &tile_map);
    if (mode == 0) {
        if (threadIdx.x == 0) a.tile[blk] = static_cast<uint8_t>(tile_map);
        return;
    }
    unsigned st = live ? (pre >> a.tile[blk]) & 1u : 0u;   // the state before this thread's first frame
    unsigned flags = 0;
    int cnt = 0;
    for (int k = 0; k < n; ++k) {
        const unsigned fm = frame_map(v[k], a.onset, a.offset);
        if (!st && (fm & 1u)) { flags |= 1u << k; ++cnt; }
        st = (fm >> st) & 1u;
    }
    int tot;
    const int ex = block_exclusive(cnt, &tot);
    if (mode == 1) {
        if (threadIdx.x == 0) a.bsum[blk] = tot;
        return;
    }
    int pos = a.bsum[blk] + ex;
    for (int k = 0; k < n; ++k) if (flags & (1u << k)) starts[pos++] = static_cast<int32_t>(i0 + k);
}

// one thread per (recording, speaker): the state at the start of each of its tiles
__global__ __launch_bounds__(kThreads) void tl_tile_state(TlArgs a, int64_t Q) {
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (q >= Q) return;
    uint8_t *tm = a.tile + q * a.max_tiles;
    unsigned st = 0;
    for (int t = 0; t < a.max_tiles; ++t) { const unsigned m = tm[t]; tm[t] = static_cast<uint8_t>(st); st = (m >> st) & 1u; }
}

struct TlRun { int32_t on, off; float sum; };   // frames [on, off) speaking; off == frames of the recording: still speaking at the end

// one lane per raw run: unmergedActivitySum starts at the onset frame's value and adds the following frames' in order (:1205, :1231)
__global__ __launch_bounds__(kThreads) void tl_run_walk(TlArgs a, const int32_t *__restrict__ starts, int64_t Q, TlRun *__restrict__ runs) {
    const int32_t *boff = a.bsum;   // exclusive onset offsets per (q, tile); boff[Q * max_tiles] = the total
    const int64_t n = boff[Q * a.max_tiles];
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        int64_t lo = 0, hi = Q;   // the last q whose first run is <= i
        while (hi - lo > 1) { const int64_t m = (lo + hi) >> 1; if (boff[m * a.max_tiles] <= i) lo = m; else hi = m; }
        const int r = static_cast<int>(lo / a.S), s = static_cast<int>(lo - static_cast<int64_t>(r) * a.S);
        const TlRec rc = a.rec[r];
        const int64_t len = static_cast<int64_t>(rc.nf) + rc.nt;
        const int32_t on = starts[i];
        float sum = tl_value(a, rc, s, on);
        int64_t f = static_cast<int64_t>(on) + 1;
        for (; f < len; ++f) {
            const float x = tl_value(a, rc, s, f);
            if (!(x >= a.offset)) break;
            sum += x;
        }
        runs[i] = TlRun{on, static_cast<int32_t>(f), sum};
    }
}

struct WalkArgs {
    const TlRec *rec;
    const int32_t *boff;       // as tl_run_walk
    const TlRun *runs;
    int32_t *count;            // [Q] segments of each (recording, speaker)
    const int32_t *seg_off;    // [Q] exclusive offsets of count (fill pass)
    fa_diarizer_segment *out;  // fill pass: capacity records
    int64_t capacity, Q;
    int32_t S, max_tiles, pad_on, pad_off, min_on, min_off, complete;
};

// one lane per (recording, speaker): updateSegments (:1169-1294) twice over the raw runs instead of the frames, then finalize()
__global__ __launch_bounds__(kThreads) void tl_segment_walk(WalkArgs a, int fill) {
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (q >= a.Q) return;
    const int r = static_cast<int>(q / a.S), s = static_cast<int>(q - static_cast<int64_t>(r) * a.S);
    const TlRec rc = a.rec[r];
    const int64_t nf = rc.nf, len = nf + rc.nt;
    const int64_t run0 = a.boff[q * a.max_tiles], run1 = a.boff[(q + 1) * a.max_tiles];
    const int64_t pad = static_cast<int64_t>(a.pad_on) + a.pad_off, min_len = pad + a.min_on;
    // SegmentScratch (:649-661)
    bool speaking = false, has = false;
    int64_t start = INT64_MIN, end = INT64_MIN, ustart = INT64_MIN, acount = 0, ucount = 0;
    float asum = 0.0f, usum = 0.0f;
    int64_t emitted = 0;
    const int64_t base = fill ? a.seg_off[q] : 0;
    auto commit = [&](bool finalized) {   // commitSegment (:1297-1336)
        if (!has) return;
        if (fill && base + emitted < a.capacity) {
            fa_diarizer_segment seg;
            seg.recording = r;
            seg.speaker = s;
            seg.start_frame = start;
            seg.end_frame = end;
            seg.activity = acount > 0 ? asum / static_cast<float>(acount) : 0.0f;
            seg.finalized = finalized ? 3 : (a.complete ? 2 : 0);
            a.out[base + emitted] = seg;
        }
        ++emitted;
        has = false;
        asum = 0.0f;
        acount = 0;
    };
    bool fin = true;   // the finalized pass
    auto end_finalized_pass = [&]() {   // :1255-1264 with isFinalized
        if (has && end < nf - a.min_off - pad) commit(true);
        fin = false;
    };
    for (int64_t i = run0; i < run1; ++i) {
        const TlRun run = a.runs[i];
        if (fin && run.on >= nf) end_finalized_pass();
        {   // not speaking -> speaking (:1224-1252)
            const int64_t st = static_cast<int64_t>(run.on) - a.pad_on;
            speaking = true;
            ustart = st;
            if (has && !(st > end + a.min_off)) {
                has = false;
            } else {
                commit(fin);
                start = st;
            }
        }
        usum = run.sum;
        ucount = static_cast<int64_t>(run.off) - run.on;
        if (run.off >= len) break;   // still speaking at the end
        if (fin && run.off >= nf) end_finalized_pass();
        {   // speaking -> not speaking (:1210-1223)
            speaking = false;
            const int64_t e = static_cast<int64_t>(run.off) + a.pad_off;
            if (!(e >= ustart + min_len)) {
                has = end >= start + min_len;
            } else {
                end = e;
                asum += usum;
                acount += ucount;
                has = true;
            }
        }
    }
    if (fin) end_finalized_pass();
    commit(false);   // the tentative pass's pending segment (:1256 with isFinalized false)
    if (speaking) {  // the trailing segment (:1272-1292)
        const int64_t padded_end = len + a.pad_off;
        if (padded_end >= start + min_len) {
            has = true;
            if (padded_end >= ustart + min_len) {
                end = padded_end;
                asum += usum;
                acount += ucount;
            }
            commit(false);
        }
    }
    if (!fill) a.count[q] = static_cast<int32_t>(emitted);
}

fa_status timeline_segments(fa_ctx *ctx, const fa_timeline_config *cfg, const float *finalized, const int64_t *fin_frames, const float *tentative,
                            const int64_t *tent_frames, int32_t B, int32_t is_complete, fa_diarizer_segment *segs, int64_t capacity, int64_t *count,
                            int64_t *rec_counts, bool device) {
    if (!ctx || !cfg || !count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "timeline: ctx, config and count are required");
    *count = 0;
    if (B < 0 || capacity < 0 || cfg->speakers < 1 || (B > 0 && !fin_frames) || cfg->onset_pad_frames < 0 || cfg->offset_pad_frames < 0 ||
        cfg->min_frames_on < 0 || cfg->min_frames_off < 0)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "timeline: bad arguments");
    if (cfg->activity_type != FA_ACTIVITY_SIGMOIDS)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "timeline: only the sigmoid activity type is supported");
    if (rec_counts) for (int32_t b = 0; b < B; ++b) rec_counts[b] = 0;
    if (B == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "timeline", [&]() -> fa_status {
    const int32_t S = cfg->speakers;
    std::vector<TlRec> rec(static_cast<size_t>(B));
    int64_t fsum = 0, tsum = 0, max_len = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t nf = fin_frames[b], nt = tent_frames ? tent_frames[b] : 0;
        if (nf < 0 || nt < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "timeline: recording %d has a negative frame count", b);
        if (nf + nt >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "timeline: recording %d has 2^31 frames or more", b);
        rec[b] = TlRec{fsum, tsum, static_cast<int32_t>(nf), static_cast<int32_t>(nt)};
        fsum += nf;
        tsum += nt;
        max_len = std::max(max_len, nf + nt);
    }
    if ((fsum > 0 && !finalized) || (tsum > 0 && !tentative)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "timeline: predictions are required");
    const int64_t Q = static_cast<int64_t>(B) * S;
    const int32_t max_tiles = static_cast<int32_t>(std::max<int64_t>(1, (max_len + kTile - 1) / kTile));
    const int64_t blocks = Q * max_tiles;
    if (blocks >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "timeline: %lld tiles", (long long)blocks);

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_fin, b_tent, b_rec, b_tile, b_bsum, b_starts, b_runs, b_count, b_off, b_total, b_out;
    auto alloc = [&](fa::DevBuf &b, size_t bytes) { return b.alloc(ctx, bytes) == hipSuccess; };
    const auto fail = [&]() { (void)hipGetLastError(); return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "timeline: device allocation failed"); };
    if (!alloc(b_rec, sizeof(TlRec) * B) || !alloc(b_tile, static_cast<size_t>(blocks)) || !alloc(b_bsum, sizeof(int32_t) * (blocks + 1)) ||
        !alloc(b_count, sizeof(int32_t) * Q) || !alloc(b_off, sizeof(int32_t) * Q) || !alloc(b_total, sizeof(int32_t)))
        return fail();
    const float *d_fin = finalized, *d_tent = tentative;
    if (!device) {
        if ((fsum > 0 && !alloc(b_fin, sizeof(float) * fsum * S)) || (tsum > 0 && !alloc(b_tent, sizeof(float) * tsum * S))) return fail();
        if (fsum > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_fin.p, finalized, sizeof(float) * fsum * S, hipMemcpyHostToDevice, st));
        if (tsum > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(b_tent.p, tentative, sizeof(float) * tsum * S, hipMemcpyHostToDevice, st));
        d_fin = b_fin.as<float>();
        d_tent = b_tent.as<float>();
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_rec.p, rec.data(), sizeof(TlRec) * B, hipMemcpyHostToDevice, st));
    TlArgs ta{d_fin, d_tent, b_rec.as<TlRec>(), b_tile.as<uint8_t>(), b_bsum.as<int32_t>(), S, max_tiles, cfg->onset_threshold, cfg->offset_threshold};
    const unsigned tgrid = static_cast<unsigned>(blocks);
    hipLaunchKernelGGL(tl_tiles, dim3(tgrid), dim3(kThreads), 0, st, ta, 0, static_cast<int32_t *>(nullptr));
    hipLaunchKernelGGL(tl_tile_state, dim3(grid_for(Q, kThreads)), dim3(kThreads), 0, st, ta, Q);
    hipLaunchKernelGGL(tl_tiles, dim3(tgrid), dim3(kThreads), 0, st, ta, 1, static_cast<int32_t *>(nullptr));
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(kThreads), 0, st, b_bsum.as<int32_t>(), blocks, b_bsum.as<int32_t>() + blocks);
    FA_HIP_TRY(ctx, hipGetLastError());
    int32_t n_runs = 0;
    FA_HIP_TRY(ctx, hipMemcpyAsync(&n_runs, b_bsum.as<int32_t>() + blocks, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the raw run count sizes the run buffers
    if (!alloc(b_starts, sizeof(int32_t) * std::max(n_runs, 1)) || !alloc(b_runs, sizeof(TlRun) * std::max(n_runs, 1))) return fail();
    if (n_runs > 0) {
        hipLaunchKernelGGL(tl_tiles, dim3(tgrid), dim3(kThreads), 0, st, ta, 2, b_starts.as<int32_t>());
        hipLaunchKernelGGL(tl_run_walk, dim3(std::min<unsigned>(grid_for(n_runs, kThreads), 4096)), dim3(kThreads), 0, st, ta, b_starts.as<int32_t>(), Q,
                           b_runs.as<TlRun>());
    }
    WalkArgs wa{b_rec.as<TlRec>(), b_bsum.as<int32_t>(), b_runs.as<TlRun>(), b_count.as<int32_t>(), b_off.as<int32_t>(), nullptr, 0, Q, S, max_tiles,
                cfg->onset_pad_frames, cfg->offset_pad_frames, cfg->min_frames_on, cfg->min_frames_off, is_complete ? 1 : 0};
    hipLaunchKernelGGL(tl_segment_walk, dim3(grid_for(Q, kThreads)), dim3(kThreads), 0, st, wa, 0);
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_off.p, b_count.p, sizeof(int32_t) * Q, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(kThreads), 0, st, b_off.as<int32_t>(), Q, b_total.as<int32_t>());
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> counts(static_cast<size_t>(Q));
    FA_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), b_count.p, sizeof(int32_t) * Q, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the segment counts
    int64_t total = 0;
    for (int64_t q = 0; q < Q; ++q) {
        total += counts[q];
        if (rec_counts) rec_counts[q / S] += counts[q];
    }
    *count = total;
    if (!segs || total == 0) return FA_SUCCESS;
    const int64_t n_out = std::min(total, capacity);
    if (n_out > 0) {
        if (!alloc(b_out, sizeof(fa_diarizer_segment) * n_out)) return fail();
        wa.out = b_out.as<fa_diarizer_segment>();
        wa.capacity = n_out;
        hipLaunchKernelGGL(tl_segment_walk, dim3(grid_for(Q, kThreads)), dim3(kThreads), 0, st, wa, 1);
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipMemcpyAsync(segs, b_out.p, sizeof(fa_diarizer_segment) * n_out, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    if (capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "timeline: output holds %lld of %lld segments", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_timeline_default_config(fa_timeline_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->onset_threshold = 0.5f;        // DiarizerTimelineConfig.sortformerDefault (DiarizerTimeline.swift:72-87)
    cfg->offset_threshold = 0.5f;
    cfg->frame_duration = 0.08f;
    cfg->speakers = 4;
    cfg->activity_type = FA_ACTIVITY_SIGMOIDS;
}

fa_status fa_timeline_segments_dev(fa_ctx *ctx, const fa_timeline_config *cfg, const float *d_finalized, const int64_t *finalized_frames,
                                   const float *d_tentative, const int64_t *tentative_frames, int32_t batch, int32_t is_complete,
                                   fa_diarizer_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts) {
    return timeline_segments(ctx, cfg, d_finalized, finalized_frames, d_tentative, tentative_frames, batch, is_complete, segs, capacity, count,
                             recording_counts, true);
}

fa_status fa_timeline_segments(fa_ctx *ctx, const fa_timeline_config *cfg, const float *finalized, const int64_t *finalized_frames, const float *tentative,
                               const int64_t *tentative_frames, int32_t batch, int32_t is_complete, fa_diarizer_segment *segs, int64_t capacity,
                               int64_t *count, int64_t *recording_counts) {
    return timeline_segments(ctx, cfg, finalized, finalized_frames, tentative, tentative_frames, batch, is_complete, segs, capacity, count,
                             recording_counts, false);
}

}  // extern "C"
