// sortformer.hip — the offline Sortformer diarizer around its network, and the timeline shared by the frame-based diarizers, on the device.
//
//   * window geometry and packing (reference: Sources/FluidAudio/Diarizer/Sortformer/Offline/OfflineSortformerDiarizer.swift:98-119,
//     303-363): a recording's mel is tiled into windows of windowOutputFrames * subsampling mel frames that overlap by
//     overlapOutputFrames output frames; each window becomes one model input [n_mels, windowMel] with a zero tail and its mel_length.
//   * stitching (:321-358, SortformerSpeakerStitcher.swift:27-77): per window the S x S correlation of the global timeline's overlap
//     region with the window's first frames (a += g * w: a multiply and an add, this file is built with -ffp-contract=off), the best of
//     the S! bijections in the reference's enumeration order (the swap recursion :80-90), and the merge into the global timeline
//     (first writer stores, later ones average).
//     With 2 * overlap <= window the overlap region has been written by the previous window only and never averaged: it is that
//     window's values moved by its mapping.  So the correlations of all windows are independent (one wavefront each, against the
//     previous window's own columns), the mappings are a short chain per recording over 16 numbers per window, and the merge is
//     parallel over global frames.  Any other geometry runs window by window, one workgroup per recording (stitch_serial): slow.
//   * timeline segments (Diarizer/DiarizerTimeline.swift:945-1003, 1169-1336): rebuild(finalizedPredictions:tentativePredictions:
//     keepingSpeakers:false,isComplete:).  The onset / offset hysteresis is a map {silent, speaking} -> {silent, speaking} per frame;
//     maps compose associatively, so the state before every frame is a scan over 2-bit maps (exact).  Onset frames are compacted with
//     block_scan.h in (recording, speaker, frame) order, one lane per raw run walks it for its sequential fp32 activity sum, and one
//     lane per (recording, speaker) runs the reference's merge logic over its raw runs.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "block_scan.h"
#include "fa_common.h"

namespace {

using fa::scan::block_exclusive;
constexpr int kThreads = fa::scan::kThreads;
constexpr int kMaxSpeakers = 4;     // stitching: S! bijections, 24 for 4 (the reference fixes 4)
constexpr int kMaxPerms = 24;
constexpr int kPer = 8;             // timeline: frames per thread of the state scan
constexpr int kTile = kThreads * kPer;

unsigned grid_for(int64_t n, int per_block) { return static_cast<unsigned>((n + per_block - 1) / per_block); }

// ---------------------------------------------------------------- window geometry (:303-363)

struct Geometry {
    std::vector<fa_sortformer_window> win;
    std::vector<int64_t> total_out, range;   // per recording; range[B + 1]
    int32_t overlap_out = 0, hop_out = 0;
};

bool config_ok(const fa_sortformer_offline_config *c) {
    return c && c->window_output_frames >= 1 && c->subsampling >= 1 && c->speakers >= 1 && c->n_mels >= 1 &&
           static_cast<int64_t>(c->window_output_frames) * c->subsampling <= INT32_MAX / 2;
}

// false: a recording's length is negative or its windows overflow 32-bit frame indices
bool geometry(const fa_sortformer_offline_config &c, const int64_t *n_mel, int32_t B, Geometry &g) {
    const int64_t window = c.window_output_frames, sub = c.subsampling, window_mel = window * sub;
    const int64_t overlap = std::max<int64_t>(0, std::min<int64_t>(c.overlap_output_frames, window - 1));
    const int64_t hop_out = window - overlap, hop_mel = hop_out * sub;
    g.overlap_out = static_cast<int32_t>(overlap);
    g.hop_out = static_cast<int32_t>(hop_out);
    g.total_out.assign(static_cast<size_t>(B), 0);
    g.range.assign(static_cast<size_t>(B) + 1, 0);
    for (int32_t b = 0; b < B; ++b) {
        const int64_t n = n_mel[b];
        if (n < 0 || n > INT32_MAX - window_mel) return false;
        g.total_out[b] = (n + sub - 1) / sub;
        int64_t mel_start = 0;
        bool first = true;
        while (mel_start < n) {
            const int64_t valid_mel = std::min(window_mel, n - mel_start);
            fa_sortformer_window w;
            w.recording = b;
            w.valid_mel = static_cast<int32_t>(valid_mel);
            w.valid_out = static_cast<int32_t>(std::min(window, (valid_mel + sub - 1) / sub));
            w.first = first ? 1 : 0;
            w.mel_start = mel_start;
            w.g_start = mel_start / sub;
            g.win.push_back(w);
            first = false;
            if (valid_mel < window_mel) break;
            mel_start += hop_mel;
        }
        g.range[b + 1] = static_cast<int64_t>(g.win.size());
    }
    return true;
}

// ---------------------------------------------------------------- packing

struct PackArgs {
    const float *mel;
    const fa_sortformer_window *win;
    float *out;
    int32_t *mel_length;
    int64_t rec_stride, frame_stride;
    int32_t n_mels, window_mel;
};

// mel-major [n_mels][frame_stride] rows: one workgroup per (window, mel row) copies the row slice and zero-fills the tail.  Stores are
// 16 bytes when the output rows are 16-byte aligned; a group of four loads as 16 bytes when its source is aligned and wholly valid.
__global__ __launch_bounds__(kThreads) void pack_rows(PackArgs a, int vec) {
    const int64_t row = blockIdx.x;
    const int64_t w = row / a.n_mels;
    const int m = static_cast<int>(row - w * a.n_mels);
    const fa_sortformer_window win = a.win[w];
    const float *src = a.mel + win.recording * a.rec_stride + m * a.frame_stride + win.mel_start;
    float *dst = a.out + row * a.window_mel;
    const int valid = win.valid_mel;
    if (m == 0 && threadIdx.x == 0) a.mel_length[w] = valid;
    if (vec) {
        const bool src_al = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
        for (int t = 4 * threadIdx.x; t < a.window_mel; t += 4 * kThreads) {
            float4 v;
            if (src_al && t + 4 <= valid) {
                v = *reinterpret_cast<const float4 *>(src + t);
            } else {
                v.x = t < valid ? src[t] : 0.0f;
                v.y = t + 1 < valid ? src[t + 1] : 0.0f;
                v.z = t + 2 < valid ? src[t + 2] : 0.0f;
                v.w = t + 3 < valid ? src[t + 3] : 0.0f;
            }
            *reinterpret_cast<float4 *>(dst + t) = v;
        }
    } else {
        for (int t = threadIdx.x; t < a.window_mel; t += kThreads) dst[t] = t < valid ? src[t] : 0.0f;
    }
}

// time-major [T][n_mels]: 64 frames x 64 mels through LDS, coalesced along the mels on the way in and along the frames on the way out
__global__ __launch_bounds__(kThreads) void pack_transpose(PackArgs a, int t_tiles, int m_tiles) {
    __shared__ float tile[64][65];
    int64_t b = blockIdx.x;
    const int mt = static_cast<int>(b % m_tiles);
    b /= m_tiles;
    const int tt = static_cast<int>(b % t_tiles);
    const int64_t w = b / t_tiles;
    const fa_sortformer_window win = a.win[w];
    const int valid = win.valid_mel, t0 = tt * 64, m0 = mt * 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    if (tt == 0 && mt == 0 && threadIdx.x == 0) a.mel_length[w] = valid;
    const float *src = a.mel + win.recording * a.rec_stride + win.mel_start * a.n_mels;
    for (int k = 0; k < 16; ++k) {
        const int t = t0 + 4 * k + ly, m = m0 + lx;
        tile[4 * k + ly][lx] = (t < valid && m < a.n_mels) ? src[static_cast<int64_t>(t) * a.n_mels + m] : 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        const int m = m0 + 4 * k + ly, t = t0 + lx;
        if (m < a.n_mels && t < a.window_mel) a.out[(w * a.n_mels + m) * a.window_mel + t] = tile[lx][4 * k + ly];
    }
}

// ---------------------------------------------------------------- stitching

struct Perms { uint8_t p[kMaxPerms][kMaxSpeakers]; int32_t n; };

// the reference's enumeration (SortformerSpeakerStitcher.swift:80-90): swap recursion, not lexicographic
void enumerate(int *arr, int k, int S, Perms &out) {
    if (k == S) {
        for (int i = 0; i < S; ++i) out.p[out.n][i] = static_cast<uint8_t>(arr[i]);
        ++out.n;
        return;
    }
    for (int i = k; i < S; ++i) {
        std::swap(arr[k], arr[i]);
        enumerate(arr, k + 1, S, out);
        std::swap(arr[k], arr[i]);
    }
}

Perms make_perms(int S) {
    Perms p;
    memset(&p, 0, sizeof(p));
    int arr[kMaxSpeakers] = {0, 1, 2, 3};
    enumerate(arr, 0, S, p);
    return p;
}

// alignment's search (:56-76) on one wavefront: lane p scores permutation p over corr[g][w] (row g already in global order).  Returns
// the winning permutation's index in every lane, -1 when no score exceeds -Float.greatestFiniteMagnitude (the identity stays).
__device__ inline int best_perm(const Perms &perms, const float *corr, int S, int lane) {
    float score = 0.0f;
    bool ok = lane < perms.n;
    if (ok) {
        for (int g = 0; g < S; ++g) score += corr[g * S + perms.p[lane][g]];
        ok = score > -3.40282347e38f;
    }
    int idx = ok ? lane : INT_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(score, off);
        const int oi = __shfl_xor(idx, off);
        if (oi != INT_MAX && (idx == INT_MAX || os > score || (os == score && oi < idx))) { score = os; idx = oi; }
    }
    return idx == INT_MAX ? -1 : idx;
}

struct StitchArgs {
    const float *preds;                 // [W][window][S]
    const fa_sortformer_window *win;    // [W]
    const int64_t *range;               // [B + 1] windows of each recording
    const int64_t *gofs;                // [B + 1] first global frame of each recording
    float *corr;                        // [W][S][S]: rows in the PREVIOUS window's own columns
    int32_t *ov;                        // [W] overlap frames compared
    float *global;                      // [sum totalOut][S]
    int32_t *mapping;                   // [W][S]
    int32_t B, S, window, overlap, hop;
};

__device__ inline int overlap_frames(const StitchArgs &a, const fa_sortformer_window &w) {
    if (w.first || a.overlap <= 0) return 0;
    const int64_t total = a.gofs[w.recording + 1] - a.gofs[w.recording];
    const int64_t room = total - w.g_start > 0 ? total - w.g_start : 0;
    const int64_t ov = a.overlap < w.valid_out ? a.overlap : w.valid_out;
    return static_cast<int>(ov < room ? ov : room);
}

// One wavefront per window: the overlap region of the global timeline is the previous window's frames hop .. hop + ov in that window's
// own columns.  Lanes < S * S carry one sequential chain each, in frame order; all lanes stage the frames through LDS.
__global__ __launch_bounds__(64) void stitch_corr(StitchArgs a) {
    __shared__ float sp[64 * kMaxSpeakers], sc[64 * kMaxSpeakers];
    const int64_t w = blockIdx.x;
    const fa_sortformer_window win = a.win[w];
    const int lane = threadIdx.x, S = a.S;
    const int ov = overlap_frames(a, win);
    if (lane == 0) a.ov[w] = ov;
    if (ov == 0) return;
    const float *prev = a.preds + ((w - 1) * a.window + a.hop) * S;
    const float *cur = a.preds + w * a.window * S;
    const int g = lane / S, c = lane - g * S;
    float acc = 0.0f;
    for (int f0 = 0; f0 < ov; f0 += 64) {
        const int nf = ov - f0 < 64 ? ov - f0 : 64;
        for (int i = lane; i < nf * S; i += 64) { sp[i] = prev[f0 * S + i]; sc[i] = cur[f0 * S + i]; }
        __syncthreads();
        if (lane < S * S) {
            for (int f = 0; f < nf; ++f) {
                const float gv = sp[f * S + g];
                if (gv != 0.0f) acc += gv * sc[f * S + c];   // guard gv != 0 (:49); multiply, then add
            }
        }
        __syncthreads();
    }
    if (lane < S * S) a.corr[w * S * S + lane] = acc;
}

// One wavefront per recording walks its windows: correlation rows re-indexed through the previous window's inverse mapping, the search,
// and mapping[w] = g.
__global__ __launch_bounds__(64) void stitch_chain(StitchArgs a, Perms perms) {
    __shared__ float corr[kMaxSpeakers * kMaxSpeakers];
    const int r = blockIdx.x, lane = threadIdx.x, S = a.S;
    int inv[kMaxSpeakers] = {0, 1, 2, 3};   // inv[g] = the previous window's column that went to global column g (its winning permutation)
    for (int64_t w = a.range[r]; w < a.range[r + 1]; ++w) {
        int best = -1;
        if (a.ov[w] > 0) {
            if (lane < S * S) { const int g = lane / S, c = lane - g * S; corr[lane] = a.corr[w * S * S + inv[g] * S + c]; }
            __syncthreads();
            best = best_perm(perms, corr, S, lane);
            __syncthreads();
        }
        for (int g = 0; g < S; ++g) inv[g] = best >= 0 ? perms.p[best][g] : g;
        if (lane < S) { int m = 0; for (int g = 0; g < S; ++g) if (inv[g] == lane) m = g; a.mapping[w * S + lane] = m; }
    }
}

// One thread per (global frame, global column): its covering windows in window order (:342-358)
__global__ __launch_bounds__(kThreads) void stitch_merge(StitchArgs a, int64_t items, int reach) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= items) return;
    const int S = a.S;
    const int64_t gf_all = e / S;
    const int g = static_cast<int>(e - gf_all * S);
    int lo = 0, hi = a.B;   // the recording: last r with gofs[r] <= gf_all
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (a.gofs[m] <= gf_all) lo = m; else hi = m; }
    const int r = lo;
    const int64_t gf = gf_all - a.gofs[r], w0 = a.range[r], nw = a.range[r + 1] - w0;
    float v = 0.0f;
    bool filled = false;
    if (nw > 0) {
        const int64_t last = gf / a.hop < nw - 1 ? gf / a.hop : nw - 1;
        for (int64_t i = last > reach ? last - reach : 0; i <= last; ++i) {
            const fa_sortformer_window win = a.win[w0 + i];
            if (gf < win.g_start || gf >= win.g_start + win.valid_out) continue;
            int c = 0;
            for (int k = 0; k < S; ++k) if (a.mapping[(w0 + i) * S + k] == g) c = k;
            const float p = a.preds[((w0 + i) * a.window + (gf - win.g_start)) * S + c];
            v = filled ? (v + p) * 0.5f : p;
            filled = true;
        }
    }
    a.global[e] = v;
}

// Any geometry, as the reference walks it: one workgroup per recording, window by window against the global timeline itself.
__global__ __launch_bounds__(kThreads) void stitch_serial(StitchArgs a, Perms perms) {
    __shared__ float corr[kMaxSpeakers * kMaxSpeakers];
    __shared__ int map[kMaxSpeakers];
    const int r = blockIdx.x, tid = threadIdx.x, S = a.S;
    const int64_t total = a.gofs[r + 1] - a.gofs[r];
    float *global = a.global + a.gofs[r] * S;
    int64_t prev_end = 0;
    for (int64_t w = a.range[r]; w < a.range[r + 1]; ++w) {
        const fa_sortformer_window win = a.win[w];
        const float *cur = a.preds + w * a.window * S;
        const int ov = overlap_frames(a, win);
        if (tid < S) map[tid] = tid;
        if (ov > 0 && tid < S * S) {
            const int g = tid / S, c = tid - g * S;
            float acc = 0.0f;
            for (int f = 0; f < ov; ++f) {
                const float gv = global[(win.g_start + f) * S + g];
                if (gv != 0.0f) acc += gv * cur[f * S + c];
            }
            corr[tid] = acc;
        }
        __syncthreads();
        if (ov > 0 && tid < 64) {
            const int best = best_perm(perms, corr, S, tid);
            if (best >= 0 && tid < S) map[perms.p[best][tid]] = tid;   // mapping[bestPerm[g]] = g
        }
        __syncthreads();
        if (tid < S) a.mapping[w * S + tid] = map[tid];
        for (int i = tid; i < win.valid_out * S; i += kThreads) {
            const int j = i / S, c = i - j * S;
            const int64_t gf = win.g_start + j;
            if (gf >= total) continue;
            const int64_t idx = gf * S + map[c];
            const float p = cur[i];
            global[idx] = (!win.first && gf < prev_end) ? (global[idx] + p) * 0.5f : p;
        }
        prev_end = win.g_start + win.valid_out;
        __syncthreads();
    }
}

// the host twin of the alignment (SortformerSpeakerStitcher.alignment :27-77)
void alignment_host(const float *global, const float *window, int64_t frames, int S, int32_t *mapping) {
    float corr[kMaxSpeakers][kMaxSpeakers] = {};
    for (int64_t f = 0; f < frames; ++f) {
        for (int g = 0; g < S; ++g) {
            const float gv = global[f * S + g];
            if (!(gv != 0.0f)) continue;
            for (int w = 0; w < S; ++w) corr[g][w] += gv * window[f * S + w];
        }
    }
    const Perms perms = make_perms(S);
    int best = -1;
    float best_score = -3.40282347e38f;
    for (int p = 0; p < perms.n; ++p) {
        float score = 0.0f;
        for (int g = 0; g < S; ++g) score += corr[g][perms.p[p][g]];
        if (score > best_score) { best_score = score; best = p; }
    }
    for (int g = 0; g < S; ++g) mapping[best >= 0 ? perms.p[best][g] : g] = g;
}

// ---------------------------------------------------------------- timeline

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

void fa_sortformer_offline_default_config(fa_sortformer_offline_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->window_output_frames = 384;    // OfflineSortformerDiarizer.swift:17-43
    cfg->subsampling = 8;
    cfg->speakers = 4;
    cfg->n_mels = 128;
    cfg->overlap_output_frames = 100;
}

fa_status fa_sortformer_offline_windows(const fa_sortformer_offline_config *cfg, const int64_t *n_mel_frames, int32_t batch, fa_sortformer_window *windows,
                                        int64_t capacity, int64_t *count, int64_t *total_out, int64_t *window_range) {
    if (!config_ok(cfg) || !count || batch < 0 || capacity < 0 || (batch > 0 && !n_mel_frames)) return FA_INVALID_ARGUMENT;
    *count = 0;
    return fa::no_throw(nullptr, "sortformer windows", [&]() -> fa_status {
        Geometry g;
        if (!geometry(*cfg, n_mel_frames, batch, g)) return FA_INVALID_ARGUMENT;
        *count = static_cast<int64_t>(g.win.size());
        if (total_out) std::copy(g.total_out.begin(), g.total_out.end(), total_out);
        if (window_range) std::copy(g.range.begin(), g.range.end(), window_range);
        if (!windows) return FA_SUCCESS;
        if (capacity < *count) return FA_OUTPUT_TOO_SMALL;
        std::copy(g.win.begin(), g.win.end(), windows);
        return FA_SUCCESS;
    });
}

fa_status fa_sortformer_pack_windows_dev(fa_ctx *ctx, const fa_sortformer_offline_config *cfg, const float *d_mel, int32_t layout, int64_t rec_stride,
                                         int64_t frame_stride, const int64_t *n_mel_frames, int32_t batch, int64_t windows, float *d_out,
                                         int32_t *d_mel_length) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!config_ok(cfg) || batch < 0 || windows < 0 || (batch > 0 && !n_mel_frames) || rec_stride < 0 || frame_stride < 0 ||
        (layout != FA_MEL_LAYOUT_MEL_MAJOR && layout != FA_MEL_LAYOUT_FRAME_MAJOR))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: bad arguments");
    return fa::no_throw(ctx, "sortformer pack", [&]() -> fa_status {
    Geometry g;
    if (!geometry(*cfg, n_mel_frames, batch, g)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: bad recording lengths");
    const int64_t W = static_cast<int64_t>(g.win.size());
    if (W != windows) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: %lld windows given, the geometry has %lld", (long long)windows, (long long)W);
    if (W == 0) return FA_SUCCESS;
    if (!d_mel || !d_out || !d_mel_length) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: mel, output and mel_length are required");
    const int32_t n_mels = cfg->n_mels, window_mel = cfg->window_output_frames * cfg->subsampling;
    for (int32_t b = 0; b < batch; ++b) {   // every recording's frames lie inside its slot of the mel buffer
        const int64_t n = n_mel_frames[b];
        const bool fits = layout == FA_MEL_LAYOUT_MEL_MAJOR ? (n <= frame_stride && (batch == 1 || static_cast<int64_t>(n_mels) * frame_stride <= rec_stride))
                                                            : (batch == 1 || n * n_mels <= rec_stride);
        if (!fits) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: recording %d does not fit its strides", b);
    }
    const int64_t rows = W * n_mels;
    const int t_tiles = (window_mel + 63) / 64, m_tiles = (n_mels + 63) / 64;
    if (rows >= INT32_MAX || W * t_tiles * m_tiles >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "sortformer pack: %lld windows", (long long)W);
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_win;
    if (b_win.alloc(ctx, sizeof(fa_sortformer_window) * W) != hipSuccess) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "sortformer pack: device allocation failed");
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_win.p, g.win.data(), sizeof(fa_sortformer_window) * W, hipMemcpyHostToDevice, st));
    PackArgs pa{d_mel, b_win.as<fa_sortformer_window>(), d_out, d_mel_length, rec_stride, frame_stride, n_mels, window_mel};
    if (layout == FA_MEL_LAYOUT_MEL_MAJOR) {
        const int vec = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 && window_mel % 4 == 0;
        hipLaunchKernelGGL(pack_rows, dim3(static_cast<unsigned>(rows)), dim3(kThreads), 0, st, pa, vec);
    } else {
        hipLaunchKernelGGL(pack_transpose, dim3(static_cast<unsigned>(W * t_tiles * m_tiles)), dim3(kThreads), 0, st, pa, t_tiles, m_tiles);
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the staged window table is released with this call
    return FA_SUCCESS;
    });
}

fa_status fa_sortformer_stitch_dev(fa_ctx *ctx, const fa_sortformer_offline_config *cfg, const float *d_preds, const int64_t *n_mel_frames, int32_t batch,
                                   int64_t windows, float *d_global, int32_t *d_mapping) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!config_ok(cfg) || batch < 0 || windows < 0 || (batch > 0 && !n_mel_frames) || cfg->speakers > kMaxSpeakers)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer stitch: bad arguments (1 to %d speakers)", kMaxSpeakers);
    return fa::no_throw(ctx, "sortformer stitch", [&]() -> fa_status {
    Geometry g;
    if (!geometry(*cfg, n_mel_frames, batch, g)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer stitch: bad recording lengths");
    const int64_t W = static_cast<int64_t>(g.win.size());
    if (W != windows) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer stitch: %lld windows given, the geometry has %lld", (long long)windows, (long long)W);
    if (W == 0) return FA_SUCCESS;
    if (!d_preds || !d_global || !d_mapping) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer stitch: predictions, timeline and mapping are required");
    const int32_t S = cfg->speakers, window = cfg->window_output_frames;
    std::vector<int64_t> gofs(static_cast<size_t>(batch) + 1, 0);
    for (int32_t b = 0; b < batch; ++b) gofs[b + 1] = gofs[b] + g.total_out[b];
    const int64_t items = gofs[batch] * S;
    if (W >= INT32_MAX || items / kThreads >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "sortformer stitch: %lld windows", (long long)W);
    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_win, b_range, b_gofs, b_corr, b_ov;
    if (b_win.alloc(ctx, sizeof(fa_sortformer_window) * W) != hipSuccess || b_range.alloc(ctx, sizeof(int64_t) * (batch + 1)) != hipSuccess ||
        b_gofs.alloc(ctx, sizeof(int64_t) * (batch + 1)) != hipSuccess || b_corr.alloc(ctx, sizeof(float) * W * S * S) != hipSuccess ||
        b_ov.alloc(ctx, sizeof(int32_t) * W) != hipSuccess) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "sortformer stitch: device allocation failed");
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_win.p, g.win.data(), sizeof(fa_sortformer_window) * W, hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_range.p, g.range.data(), sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_gofs.p, gofs.data(), sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice, st));
    StitchArgs sa{d_preds, b_win.as<fa_sortformer_window>(), b_range.as<int64_t>(), b_gofs.as<int64_t>(), b_corr.as<float>(), b_ov.as<int32_t>(),
                  d_global, d_mapping, batch, S, window, g.overlap_out, g.hop_out};
    const Perms perms = make_perms(S);
    if (2 * g.overlap_out <= window) {
        hipLaunchKernelGGL(stitch_corr, dim3(static_cast<unsigned>(W)), dim3(64), 0, st, sa);
        hipLaunchKernelGGL(stitch_chain, dim3(static_cast<unsigned>(batch)), dim3(64), 0, st, sa, perms);
        if (items > 0) {
            const int reach = (window + g.hop_out - 1) / g.hop_out;   // windows that can cover one frame
            hipLaunchKernelGGL(stitch_merge, dim3(grid_for(items, kThreads)), dim3(kThreads), 0, st, sa, items, reach);
        }
    } else {
        if (items > 0) FA_HIP_TRY(ctx, hipMemsetAsync(d_global, 0, sizeof(float) * items, st));
        hipLaunchKernelGGL(stitch_serial, dim3(static_cast<unsigned>(batch)), dim3(kThreads), 0, st, sa, perms);
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the staged geometry is released with this call
    return FA_SUCCESS;
    });
}

fa_status fa_sortformer_stitcher_alignment(const float *global, const float *window, int64_t frames, int32_t speakers, int32_t *mapping) {
    if (speakers < 1 || speakers > kMaxSpeakers || !mapping) return FA_INVALID_ARGUMENT;
    for (int32_t s = 0; s < speakers; ++s) mapping[s] = s;
    if (frames <= 0) return FA_SUCCESS;           // nothing to align on: identity (:34-39)
    if (!global || !window) return FA_INVALID_ARGUMENT;
    alignment_host(global, window, frames, speakers, mapping);
    return FA_SUCCESS;
}

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
