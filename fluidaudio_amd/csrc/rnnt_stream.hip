// rnnt_stream.hip — the kernels of the Nemotron streaming session (host side: rnnt_stream_host.hip; operands and launchers:
// rnnt_stream_launch.h; the integers and the RMS order: rnnt_stream_core.h).
//   gate_kernel        one workgroup of four wavefronts per stream: the chunk's RMS in the core's order, the hangover counter, the skip.
//   run_list_kernel    the active streams that run, ascending, by one workgroup's scan (block_scan.h).
//   mel_rows_kernel    one wavefront per (listed stream, mel row): the old cache into registers, the encoder's row, the new cache.
//   mel_count_kernel   the cache's frame count, after every row has read the old one.
//   advance_kernel     the frame base of the streams that ran.
//   track_decide       one wavefront per stream: every window's RMS by all lanes, the silent word, the span machine over it without a
//                      write to the state, the closing test over the stream's tokens; leaves the silent and wanted words and the counts.
//   track_place        the requests' and the arena's offsets by one workgroup's scan, in slot order.
//   track_copy         the machine again over the silent word, now with its copies (chunk -> slab / ring, ring -> slab, slab -> arena),
//                      the request records and the state.  The decisions are taken before the first copy, so a span that closes and
//                      reopens inside one chunk has its audio in the arena before the slab is written again.
//   merge_kernel       one wavefront per stream: its requests in order; tags dropped, frames clamped, the suffix moved from its end.
// No float atomics; every store is a vector store of plain C++.
#include "block_scan.h"
#include "rnnt_stream_launch.h"

namespace fa {
namespace rns {
namespace {

__device__ inline float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
    return x;
}

// the writes of this wavefront's other lanes are seen, and its reads are done, before what follows
__device__ inline void wave_fence() { __threadfence_block(); }

__device__ inline float add4(const float4 v, float a) {
    a = square_add(v.x, a); a = square_add(v.y, a); a = square_add(v.z, a);
    return square_add(v.w, a);
}

// this lane's share of x[0, n) in the core's order.  wide: x is 16-byte aligned
__device__ inline float lane_squares(const float *__restrict__ x, const int64_t n, const int wave, const int lane, const int waves, const bool wide) {
    float a = 0.0f;
    for (int64_t k = 0;; ++k) {
        const int64_t i0 = lane_group(k, wave, lane, waves) * 4;
        if (i0 >= n) break;
        if (wide && i0 + 4 <= n) {
            a = add4(*reinterpret_cast<const float4 *>(x + i0), a);
        } else {
            for (int64_t i = i0; i < i0 + 4 && i < n; ++i) a = square_add(x[i], a);
        }
    }
    return a;
}

// one window of W <= 8 * 256 samples, W % 4 == 0, 16-byte aligned: every load before the first use
constexpr int kWindowLoads = 8;
__device__ inline float window_squares_wide(const float *__restrict__ x, const int32_t W, const int lane) {
    float4 v[kWindowLoads];
#pragma unroll
    for (int k = 0; k < kWindowLoads; ++k) {
        const int32_t i0 = (k * kLanes + lane) * 4;
        v[k] = i0 < W ? *reinterpret_cast<const float4 *>(x + i0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < kWindowLoads; ++k)
        if ((k * kLanes + lane) * 4 < W) a = add4(v[k], a);
    return a;
}

// n floats, n % 4 == 0, dst 16-byte aligned; src 16-byte aligned when wide
__device__ inline void copy_floats(float *__restrict__ dst, const float *__restrict__ src, const int32_t n, const int lane, const bool wide) {
    for (int32_t i = lane * 4; i < n; i += kLanes * 4) {
        float4 v;
        if (wide) v = *reinterpret_cast<const float4 *>(src + i);
        else v = make_float4(src[i], src[i + 1], src[i + 2], src[i + 3]);
        *reinterpret_cast<float4 *>(dst + i) = v;
    }
}

__device__ inline void zero_floats(float *__restrict__ dst, const int64_t n, const int lane) {
    for (int64_t i = lane * 4; i < n; i += kLanes * 4) *reinterpret_cast<float4 *>(dst + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- gate
__global__ __launch_bounds__(kGateBlock) void gate_kernel(const GateArgs a, const bool wide) {
    __shared__ float part[kGateWaves];
    const int32_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (a.active && a.active[b] == 0) {
        if (threadIdx.x == 0) a.status[b] = kInactive;
        return;
    }
    const int64_t n = a.chunk_samples;
    const bool on = a.c.vad_rms_threshold > 0.0f;
    if (on) {
        const float s = wave_sum(lane_squares(a.chunks + static_cast<int64_t>(b) * n, n, wave, lane, kGateWaves, wide));
        if (lane == 0) part[wave] = s;
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float r = 0.0f;
    if (on) {
        float total = part[0];
        for (int w = 1; w < kGateWaves; ++w) total = total + part[w];
        r = rms_of_sum(total, n);
    }
    int32_t *sc = a.st.scalars + static_cast<int64_t>(b) * kScalars;
    int32_t low = sc[kVadLow], skips = sc[kVadSkips], base = sc[kFrameBase];
    const int32_t skip = gate_step(a.c, n <= 0 || r < a.c.vad_rms_threshold, a.chunk_samples, low, skips, base);   // isAudioSilent: an empty chunk is silent
    sc[kVadLow] = low; sc[kVadSkips] = skips; sc[kFrameBase] = base;
    a.rms[b] = r; a.skip[b] = skip; a.status[b] = kOk;
}

__global__ __launch_bounds__(scan::kThreads) void run_list_kernel(const GateArgs a) {
    const int total = scan::workgroup_exclusive(
        a.st.B, [&](const int32_t b) { return (!a.active || a.active[b] != 0) && a.skip[b] == 0 ? 1 : 0; },
        [&](const int32_t b, const int v, const int at) { if (v) a.run_list[at] = b; });
    if (threadIdx.x == 0) *a.run_count = total;
}

// ---- the listed streams of mel_inputs, advance and finalize
__device__ inline int32_t listed(const int32_t *count, const int32_t max_count) {
    const int32_t n = *count;
    return n < 0 ? 0 : n > max_count ? max_count : n;
}

__global__ __launch_bounds__(kWaveBlock) void mel_rows_kernel(const MelArgs a) {
    const int32_t k = blockIdx.y, f = blockIdx.x, lane = threadIdx.x;
    if (k >= listed(a.count, a.max_count)) return;
    const int32_t b = a.streams[k];
    if (b < 0 || b >= a.st.B) {
        if (f == 0 && lane == 0) a.status[k] = kBadOperand;
        return;
    }
    const int32_t pre = a.c.pre_encode_cache, total = a.c.total_mel_frames, F = a.c.mel_features;
    const int32_t have = a.st.scalars[static_cast<int64_t>(b) * kScalars + kMelFrames];
    float *cache = a.st.mel_cache + (static_cast<int64_t>(b) * F + f) * (pre > 0 ? pre : 1);
    const float old = lane < have ? cache[lane] : 0.0f;                            // before any store
    const int32_t copy = a.chunk_frames < total - pre ? a.chunk_frames : total - pre;
    const float *src = a.mel + b * a.stream_stride + f * a.row_stride;
    float *out = a.rows + (static_cast<int64_t>(k) * F + f) * total;
    for (int32_t t = lane; t < total; t += kLanes)
        out[t] = t < pre ? old : t - pre < copy ? src[(t - pre) * a.frame_stride] : 0.0f;
    const int32_t keep = pre < a.chunk_frames ? pre : a.chunk_frames;
    if (lane < pre) cache[lane] = lane < keep ? src[(a.chunk_frames - keep + lane) * a.frame_stride] : 0.0f;
    if (f == 0 && lane == 0) a.status[k] = kOk;
}

__global__ __launch_bounds__(kListBlock) void mel_count_kernel(const MelArgs a) {
    const int32_t k = blockIdx.x * kListBlock + threadIdx.x;
    if (k >= listed(a.count, a.max_count)) return;
    const int32_t b = a.streams[k];
    if (b < 0 || b >= a.st.B) return;
    a.st.scalars[static_cast<int64_t>(b) * kScalars + kMelFrames] = a.c.pre_encode_cache < a.chunk_frames ? a.c.pre_encode_cache : a.chunk_frames;
}

__global__ __launch_bounds__(kListBlock) void advance_kernel(const AdvanceArgs a) {
    const int32_t k = blockIdx.x * kListBlock + threadIdx.x;
    if (k >= listed(a.count, a.max_count)) return;
    const int32_t b = a.streams[k], frames = a.d_frames ? a.d_frames[k] : a.frames;
    if (b < 0 || b >= a.st.B || frames <= 0) return;
    a.st.scalars[static_cast<int64_t>(b) * kScalars + kFrameBase] += frames;
}

// ---- track
// the stream of a slot, or -1 with the slot's status decided
__device__ inline int32_t slot_stream(const TrackArgs &a, const int32_t slot, int32_t *status) {
    *status = kOk;
    if (a.finalize) {
        if (slot >= listed(a.count, a.slots)) { *status = -1; return -1; }        // not listed: no status either
        const int32_t b = a.streams[slot];
        if (b < 0 || b >= a.st.B) { *status = kBadOperand; return -1; }
        return b;
    }
    if (a.active && a.active[slot] == 0) { *status = kInactive; return -1; }
    return slot;
}

__device__ inline Span load_span(const int32_t *sc, const int32_t W) {
    return Span{sc[kOpen], sc[kStart], sc[kLast], sc[kSpeech], sc[kPreFrames], sc[kRun], sc[kOverflowed], sc[kSpanLen], sc[kPreHead], sc[kPreLen] / W};
}

__device__ inline int64_t padded_floats(const int32_t samples, const int32_t chunk) { return static_cast<int64_t>(decode_chunks(samples, chunk)) * chunk; }

// closeSpanAndMaybeRescue's test (:138-157): true when the span asks for a rescue
__device__ inline bool wants_rescue(const TrackArgs &a, const Closure &k, const int32_t b, const int32_t tokens, const int lane) {
    if (!qualifies(a.c, k)) return false;
    const int64_t row = static_cast<int64_t>(b) * a.token_capacity;
    bool emitted = false;
    for (int32_t j0 = 0; j0 < tokens; j0 += kLanes) {
        const int32_t j = j0 + lane;
        const bool hit = j < tokens && in_span_window(a.c, k, a.tok_frame[row + j]) && (class_of(a.class_of, a.vocab, a.tok_id[row + j]) & kLexical);
        emitted = emitted || __ballot(hit) != 0;
    }
    return !emitted;
}

__global__ __launch_bounds__(kWaveBlock) void track_decide(const TrackArgs a, const bool wide) {
    const int32_t slot = blockIdx.x, lane = threadIdx.x;
    int32_t verdict;
    const int32_t b = slot_stream(a, slot, &verdict);
    int32_t tokens = 0;
    if (b >= 0) {
        tokens = a.tok_count[b];
        if (tokens < 0 || tokens > a.token_capacity) verdict = kBadOperand;
    }
    if (b < 0 || verdict != kOk || !(a.c.rescue_rms_threshold > 0.0f)) {          // nothing to track: no request, the state as it is
        if (lane == 0) {
            a.st.found[slot] = 0; a.st.floats[slot] = 0;
            if (verdict >= 0) a.status[slot] = verdict;
        }
        return;
    }
    const int32_t W = a.c.window_samples, windows = a.finalize ? 0 : a.chunk_samples / W;
    const int32_t *sc = a.st.scalars + static_cast<int64_t>(b) * kScalars;
    Span s = load_span(sc, W);
    const int32_t cursor = sc[kCursor];
    const float *x = a.chunks + static_cast<int64_t>(b) * a.chunk_samples;
    uint64_t *silent = a.st.silent + static_cast<int64_t>(b) * a.st.words, *wanted = a.st.wanted + static_cast<int64_t>(b) * a.st.words;
    int32_t found = 0;
    int64_t floats = 0;
    for (int32_t w0 = 0; w0 < windows; w0 += 64) {
        const int32_t n = windows - w0 < 64 ? windows - w0 : 64;
        uint64_t quiet = 0, want = 0;
        for (int32_t j = 0; j < n; ++j) {                                          // phase 1: every lane takes part in every window
            const float *p = x + static_cast<int64_t>(w0 + j) * W;
            const float sum = wave_sum(wide && W <= kWindowLoads * 256 ? window_squares_wide(p, W, lane) : lane_squares(p, W, 0, lane, 1, wide));
            if (rms_of_sum(sum, W) < a.c.rescue_rms_threshold) quiet |= uint64_t{1} << j;
        }
        for (int32_t j = 0; j < n; ++j) {                                          // phase 2: wave-uniform
            const Step r = window_step(a.c, s, (quiet >> j) & 1u, cursor + w0 + j);
            if (r.closed && wants_rescue(a, r.closure, b, tokens, lane)) {
                want |= uint64_t{1} << j; ++found; floats += padded_floats(r.closure.len, a.rescue_chunk_samples);
            }
        }
        if (lane == 0) { silent[w0 / 64] = quiet; wanted[w0 / 64] = want; }
    }
    if (a.finalize) {
        uint64_t want = 0;
        if (s.open) {
            const Closure k = close_span(s);
            if (wants_rescue(a, k, b, tokens, lane)) { want = 1; ++found; floats += padded_floats(k.len, a.rescue_chunk_samples); }
        }
        if (lane == 0) wanted[0] = want;
    }
    if (lane == 0) { a.st.found[slot] = found; a.st.floats[slot] = floats; }
}

__device__ inline int64_t block_exclusive64(const int64_t v, int64_t *total) {
    __shared__ int64_t wsum[scan::kThreads / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int64_t y = __shfl_up(x, off); if (lane >= off) x += y; }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    int64_t base = 0, tot = 0;
    for (int w = 0; w < scan::kThreads / 64; ++w) { if (w < wid) base += wsum[w]; tot += wsum[w]; }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(scan::kThreads) void track_place(const TrackArgs a) {
    const int total = scan::workgroup_exclusive(
        a.slots, [&](const int32_t i) { return a.st.found[i]; }, [&](const int32_t i, int, const int at) { a.st.found[i] = at; });
    if (threadIdx.x == 0) *a.request_count = total;
    int64_t base = 0;
    for (int32_t i0 = 0; i0 < a.slots; i0 += scan::kThreads) {
        const int32_t i = i0 + static_cast<int32_t>(threadIdx.x);
        const int64_t v = i < a.slots ? a.st.floats[i] : 0;
        int64_t tot;
        const int64_t at = base + block_exclusive64(v, &tot);
        if (i < a.slots) a.st.floats[i] = at;
        base += tot;
    }
}

__global__ __launch_bounds__(kWaveBlock) void track_copy(const TrackArgs a, const bool wide) {
    const int32_t slot = blockIdx.x, lane = threadIdx.x;
    int32_t verdict;
    const int32_t b = slot_stream(a, slot, &verdict);
    if (b < 0 || !(a.c.rescue_rms_threshold > 0.0f)) return;
    const int32_t tokens = a.tok_count[b];
    if (tokens < 0 || tokens > a.token_capacity) return;
    const int32_t W = a.c.window_samples, P = a.c.pre_roll_windows, windows = a.finalize ? 0 : a.chunk_samples / W;
    int32_t *sc = a.st.scalars + static_cast<int64_t>(b) * kScalars;
    Span s = load_span(sc, W);
    const int32_t cursor = sc[kCursor];
    const float *x = a.chunks + static_cast<int64_t>(b) * a.chunk_samples;
    float *span = a.st.span + static_cast<int64_t>(b) * span_capacity(a.c), *ring = a.st.ring + static_cast<int64_t>(b) * pre_roll_capacity(a.c);
    const uint64_t *silent = a.st.silent + static_cast<int64_t>(b) * a.st.words, *wanted = a.st.wanted + static_cast<int64_t>(b) * a.st.words;
    int32_t at = a.st.found[slot], detected = 0;
    int64_t room = a.st.floats[slot];
    bool small = false;

    const auto request = [&](const Closure &k) {
        const int32_t chunks = decode_chunks(k.len, a.rescue_chunk_samples);
        const int64_t padded = static_cast<int64_t>(chunks) * a.rescue_chunk_samples;
        const bool recorded = at < a.request_capacity, placed = recorded && room + padded <= a.arena_capacity;
        if (placed) {
            wave_fence();                                                          // the slab's windows were written by other lanes
            copy_floats(a.arena + room, span, k.len, lane, true);
            zero_floats(a.arena + room + k.len, padded - k.len, lane);
            wave_fence();                                                          // read before the slab is written again
        }
        if (recorded && lane == 0)
            a.requests[at] = fa_rnnt_stream_request{b, k.start - k.pre_frames, k.last + 1, k.speech, k.len, chunks, placed ? kOk : kOutputTooSmall, 0, placed ? room : -1};
        small = small || !placed;
        ++at; ++detected; room += padded;
    };

    for (int32_t w = 0; w < windows; ++w) {
        const Step r = window_step(a.c, s, (silent[w / 64] >> (w % 64)) & 1u, cursor + w);
        const float *p = x + static_cast<int64_t>(w) * W;
        if (r.ring_windows > 0) {
            wave_fence();                                                          // the ring's slots may have been written in this launch
            for (int32_t i = 0; i < r.ring_windows; ++i) copy_floats(span + static_cast<int64_t>(i) * W, ring + static_cast<int64_t>((r.ring_head + i) % P) * W, W, lane, true);
        }
        if (r.dest == kToSpan) copy_floats(span + r.offset, p, W, lane, wide);
        else if (r.dest == kToRing) copy_floats(ring + static_cast<int64_t>(r.offset) * W, p, W, lane, wide);
        if (r.closed && ((wanted[w / 64] >> (w % 64)) & 1u)) request(r.closure);
    }
    if (a.finalize && s.open) {
        const Closure k = close_span(s);
        if (wanted[0] & 1u) request(k);
    }
    if (lane == 0) {
        sc[kCursor] = cursor + windows;
        sc[kOpen] = s.open; sc[kStart] = s.start; sc[kLast] = s.last; sc[kSpeech] = s.speech; sc[kPreFrames] = s.pre_frames; sc[kRun] = s.run;
        sc[kOverflowed] = s.overflowed; sc[kSpanLen] = s.len; sc[kPreLen] = s.pre_count * W; sc[kPreHead] = s.pre_head;
        sc[kDetected] += detected;
        a.status[slot] = small ? kOutputTooSmall : kOk;
    }
}

// ---- merge
// arr[from, to) moves up by m, from its end: an iteration reads 64 entries into registers before it writes them, and what it writes lies
// above everything still to be read
__device__ inline void shift_up(int32_t *arr, const int32_t from, const int32_t to, const int32_t m, const int lane) {
    for (int32_t p = to; p > from; p -= kLanes) {
        const int32_t j = p - 1 - lane;
        const int32_t v = j >= from ? arr[j] : 0;
        if (j >= from) arr[j + m] = v;
    }
}

__global__ __launch_bounds__(kWaveBlock) void merge_kernel(const MergeArgs a) {
    const int32_t b = blockIdx.x, lane = threadIdx.x;
    const int32_t requests = listed(a.request_count, a.request_capacity), cap = a.live_capacity;
    int32_t ids_n = a.live_id_count[b], timed_n = a.live_timed_count[b], rescued = 0;
    const bool sound = ids_n >= 0 && ids_n <= cap && timed_n >= 0 && timed_n <= cap;
    int32_t *ids = a.live_ids + static_cast<int64_t>(b) * cap, *frames = a.live_frames + static_cast<int64_t>(b) * cap;
    int32_t *timed = a.live_timed_ids ? a.live_timed_ids + static_cast<int64_t>(b) * cap : nullptr;
    const uint64_t below = (uint64_t{1} << lane) - 1;

    const auto merge_one = [&](const int32_t r) -> int32_t {
        const fa_rnnt_stream_request q = a.requests[r];
        if (q.status != kOk) return q.status;
        const int32_t ni = a.staged_id_count[r], nf = a.staged_frame_count[r];
        if (!sound || ni < 0 || ni > a.staged_capacity || nf < 0 || nf > a.staged_capacity) return kBadOperand;
        const int32_t *sid = a.staged_ids + static_cast<int64_t>(r) * a.staged_capacity, *sfr = a.staged_frames + static_cast<int64_t>(r) * a.staged_capacity;
        int32_t m = 0;
        bool lexical = false;
        for (int32_t j0 = 0; j0 < ni; j0 += kLanes) {                              // :264-265, :285-287
            const int32_t j = j0 + lane;
            const uint8_t cls = j < ni ? class_of(a.class_of, a.vocab, sid[j]) : static_cast<uint8_t>(kLangTag);
            m += popcount64(__ballot(!(cls & kLangTag)));
            lexical = lexical || __ballot(!(cls & kLangTag) && (cls & kLexical)) != 0;
        }
        if (m != nf) return kBadOperand;                                           // ids and timings are 1:1 behind the filter
        if (!lexical) return kNoLexical;
        if (ids_n + m > cap || timed_n + m > cap) return kOutputTooSmall;
        const int32_t first = sfr[0];
        const int32_t key = m > 0 ? (first <= q.span_end_frame ? first : q.span_end_frame) : (q.span_start_frame > 0 ? q.span_start_frame : 0);   // :331
        int32_t t_at = timed_n, i_at = ids_n, need;
        for (int32_t j0 = 0; j0 < timed_n; j0 += kLanes) {                         // :332-333
            const int32_t j = j0 + lane;
            const int32_t p = timing_word(__ballot(j < timed_n && frames[j] > key), j0);
            if (p >= 0) { t_at = p; break; }
        }
        need = t_at;
        for (int32_t j0 = 0; j0 < ids_n; j0 += kLanes) {                           // :337-347
            const int32_t j = j0 + lane;
            const int32_t p = ids_word(__ballot(j < ids_n && !(class_of(a.class_of, a.vocab, ids[j]) & kLangTag)), j0, need);
            if (p >= 0) { i_at = p; break; }
        }
        shift_up(ids, i_at, ids_n, m, lane);
        shift_up(frames, t_at, timed_n, m, lane);
        if (timed) shift_up(timed, t_at, timed_n, m, lane);
        int32_t base = 0;
        for (int32_t j0 = 0; j0 < ni; j0 += kLanes) {                              // :349-352, the frames clamped (:270-278)
            const int32_t j = j0 + lane;
            const int32_t id = j < ni ? sid[j] : 0;
            const bool plain = j < ni && !(class_of(a.class_of, a.vocab, id) & kLangTag);
            const uint64_t word = __ballot(plain);
            if (plain) {
                const int32_t pos = base + popcount64(word & below), f = sfr[pos];
                ids[i_at + pos] = id;
                frames[t_at + pos] = f <= q.span_end_frame ? f : q.span_end_frame;
                if (timed) timed[t_at + pos] = id;
            }
            base += popcount64(word);
        }
        ids_n += m; timed_n += m; ++rescued;
        wave_fence();                                                              // the next request of this stream reads what other lanes wrote
        return kOk;
    };

    for (int32_t r0 = 0; r0 < requests; r0 += kLanes) {
        const int32_t r = r0 + lane;
        uint64_t mine = __ballot(r < requests && a.requests[r].stream == b);
        for (; mine; mine &= mine - 1) {
            const int32_t at = r0 + __builtin_ctzll(mine);
            const int32_t verdict = merge_one(at);
            if (lane == 0) a.request_status[at] = verdict;
        }
    }
    if (lane == 0 && sound && rescued > 0) {
        a.live_id_count[b] = ids_n; a.live_timed_count[b] = timed_n;
        a.st.scalars[static_cast<int64_t>(b) * kScalars + kRescued] += rescued;
    }
}

// a request of a stream outside the state has no wavefront: it is refused here
__global__ __launch_bounds__(kListBlock) void merge_strays_kernel(const MergeArgs a) {
    const int32_t r = blockIdx.x * kListBlock + threadIdx.x;
    if (r >= listed(a.request_count, a.request_capacity)) return;
    const int32_t b = a.requests[r].stream;
    if (b < 0 || b >= a.st.B) a.request_status[r] = kBadOperand;
}

}  // namespace

void launch_gate(hipStream_t stream, const GateArgs &a) {
    const bool wide = (reinterpret_cast<uintptr_t>(a.chunks) & 15u) == 0 && a.chunk_samples % 4 == 0;
    hipLaunchKernelGGL(gate_kernel, dim3(a.st.B), dim3(kGateBlock), 0, stream, a, wide);
    hipLaunchKernelGGL(run_list_kernel, dim3(1), dim3(scan::kThreads), 0, stream, a);
}

void launch_mel(hipStream_t stream, const MelArgs &a) {
    hipLaunchKernelGGL(mel_rows_kernel, dim3(a.c.mel_features, a.max_count), dim3(kWaveBlock), 0, stream, a);
    hipLaunchKernelGGL(mel_count_kernel, dim3(grid_for(a.max_count, kListBlock)), dim3(kListBlock), 0, stream, a);
}

void launch_advance(hipStream_t stream, const AdvanceArgs &a) {
    hipLaunchKernelGGL(advance_kernel, dim3(grid_for(a.max_count, kListBlock)), dim3(kListBlock), 0, stream, a);
}

void launch_track(hipStream_t stream, const TrackArgs &a) {
    const bool wide = (reinterpret_cast<uintptr_t>(a.chunks) & 15u) == 0 && a.chunk_samples % 4 == 0;
    hipLaunchKernelGGL(track_decide, dim3(a.slots), dim3(kWaveBlock), 0, stream, a, wide);
    hipLaunchKernelGGL(track_place, dim3(1), dim3(scan::kThreads), 0, stream, a);
    hipLaunchKernelGGL(track_copy, dim3(a.slots), dim3(kWaveBlock), 0, stream, a, wide);
}

void launch_merge(hipStream_t stream, const MergeArgs &a) {
    hipLaunchKernelGGL(merge_kernel, dim3(a.st.B), dim3(kWaveBlock), 0, stream, a);
    hipLaunchKernelGGL(merge_strays_kernel, dim3(grid_for(a.request_capacity, kListBlock)), dim3(kListBlock), 0, stream, a);
}

}  // namespace rns
}  // namespace fa
