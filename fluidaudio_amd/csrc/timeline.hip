// timeline.hip — the kernels of the timeline shared by the frame-based diarizers (offline and streaming Sortformer, LS-EEND), on the
// device (entries: timeline_host.hip, operands and plan: timeline_launch.h).
//
// Timeline segments (reference: Sources/FluidAudio/Diarizer/DiarizerTimeline.swift:945-1003, 1169-1336): rebuild(finalizedPredictions:
// tentativePredictions:keepingSpeakers:false,isComplete:).  The onset / offset hysteresis is a map {silent, speaking} -> {silent, speaking}
// per frame; maps compose associatively, so the state before every frame is a scan over 2-bit maps (exact).  Onset frames are compacted
// with block_scan.h in (recording, speaker, frame) order, one lane per raw run walks it for its sequential fp32 activity sum, and one lane
// per (recording, speaker) runs the reference's merge logic over its raw runs.  fluidaudio_amd/der.py scores the records this unit writes.
#include "block_scan.h"
#include "fa_common.h"
#include "timeline_launch.h"

namespace {

using namespace fa::timeline;
using fa::grid_for;
using fa::scan::block_exclusive;
static_assert(kThreads == fa::scan::kThreads, "the kernels call block_exclusive");

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

}  // namespace

namespace fa {
namespace timeline {

void launch_tiles(hipStream_t stream, const TlArgs &a, const int64_t blocks, const int mode, int32_t *starts) {
    hipLaunchKernelGGL(tl_tiles, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, a, mode, starts);
}

void launch_tile_state(hipStream_t stream, const TlArgs &a, const int64_t Q) {
    hipLaunchKernelGGL(tl_tile_state, dim3(grid_for(Q, kThreads)), dim3(kThreads), 0, stream, a, Q);
}

void launch_scan_totals(hipStream_t stream, int32_t *bsum, const int64_t nb, int32_t *total) {
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(kThreads), 0, stream, bsum, nb, total);
}

void launch_run_walk(hipStream_t stream, const TlArgs &a, const int32_t *starts, const int64_t Q, const int32_t n_runs, TlRun *runs) {
    hipLaunchKernelGGL(tl_run_walk, dim3(std::min<unsigned>(grid_for(n_runs, kThreads), 4096)), dim3(kThreads), 0, stream, a, starts, Q, runs);
}

void launch_segment_walk(hipStream_t stream, const WalkArgs &a, const int fill) {
    hipLaunchKernelGGL(tl_segment_walk, dim3(grid_for(a.Q, kThreads)), dim3(kThreads), 0, stream, a, fill);
}

}  // namespace timeline
}  // namespace fa
