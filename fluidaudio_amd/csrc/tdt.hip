// tdt.hip — Parakeet-TDT greedy decoding: frame navigation + the token/duration control loop (gfx950).
//
// Restates the control flow of TdtDecoderV3.decodeWithTimings (reference:
// Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/Decoder/TdtDecoderV3.swift:103-607) and its helpers
// (TdtFrameNavigation.swift:20-105, TdtDurationMapping.swift:17-31, TdtConfig.swift:13-26).
//
// In the reference every step of that loop crosses into CoreML: the decoder LSTM (one call per emitted token) and the
// joint network, which already returns the ARG-MAXED (token id, token probability, duration bin)
// (TdtModelInference.swift:107-138).  Those networks are not part of the reference tree, so what can be reproduced is
// the integer control flow.  The device entry therefore consumes the joint's decisions as tables indexed by
// (u = decoder steps taken so far in this chunk, t = encoder frame) — exactly the values the reference would see along
// its greedy path — and replays the loop for a whole batch of chunks, one thread per chunk (the loop is a serial walk of
// <= T + maxTokens table look-ups; the batch is the parallel axis).  PARITY of token outputs against the real models is
// UNPINNED (models absent); the navigation helpers are pinned by TdtRefactoredComponentsTests.swift:12-195.
//
// The loop is a STATE MACHINE with ONE joint evaluation per iteration (phase = outer step / blank-advance / last-chunk flush), not the reference's
// three nested loops.  Written as those, the joint is called from three places; inlined three times with its state captured by reference, the
// compiler kept token / duration in scratch memory and, in the wavefront walk, the time / step counters in vector registers (every branch an
// exec-mask save + restore, every row address 64-bit per-lane arithmetic: the round-4 listing).  One call site leaves the state a handful of
// integers: scalar registers and scalar branches where a wavefront walks a chunk, no scratch where a thread does.
//
// This unit: the kernels and one launcher per kernel family.  Host side (navigation helpers, argument checks, C ABI): tdt_host.hip; shared: tdt_launch.h.
// The language mode (transcribe(..., language:): the script filter and the blocklist at the walk's decision site, the top-K list): tdt_lang.h, included below.
#include <hip/hip_fp16.h>

#include <type_traits>

#include "tdt_launch.h"

namespace {

using namespace fa::tdt;

// Who walks a chunk: a wavefront through wave-uniform control flow (the logits kernels; what is loaded or decided is forced uniform, so the state
// lives in scalar registers), or one thread of its own (the table walk).
struct WaveWalk { static __device__ __forceinline__ int uni(const int x) { return __builtin_amdgcn_readfirstlane(x); } };
struct ThreadWalk { static __device__ __forceinline__ int uni(const int x) { return x; } };

// The control loop for chunk b.  `decide(u, frame, tok, bin)` supplies one joint decision — the token and the duration bin, which decide the next
// cell —, `prob_of_last()` the probability of the token of the MOST RECENT decision, asked for only when that token is emitted (the reference's
// joint returns it with every decision, TdtModelInference.swift:107-138, but only an emitted token's confidence is ever used, :409-463): three of
// four decisions are blanks, and the soft-max denominator is most of a decision's arithmetic.  `writer` is true for the thread that stores the outputs.
// LANG (the language mode, tdt_lang.h): `filter(u, frame, tok, score)` sees every main-loop and blank-advance decision — never a flush decision
// (TdtDecoderV3.swift:602-605) — before anything is derived from its token; it returns FA_TDT_ROUTE_* bits and, where one is set, has replaced
// tok and set score, the replaced token's confidence.  out_route [max_out] takes the bits of every emitted token.  Without LANG there is no hook.
template <class Walker, bool LANG = false, class Decide, class Prob, class Filter = int>
__device__ __forceinline__ void tdt_walk(const TdtArgs &a, const int b, const bool writer, Decide &&decide, Prob &&prob_of_last, Filter &&filter = 0,
                                         int32_t *out_route = nullptr) {
    auto uni = [](const int x) { return Walker::uni(x); };
    const fa_tdt_config &c = a.cfg;
    int32_t *otok = a.out_tok + static_cast<int64_t>(b) * a.max_out, *otime = a.out_time + static_cast<int64_t>(b) * a.max_out;
    int32_t *odur = a.out_dur + static_cast<int64_t>(b) * a.max_out;
    float *oconf = a.out_conf + static_cast<int64_t>(b) * a.max_out;
    int count = 0, st = FA_SUCCESS, u = 0;
    const int enc_len = uni(a.enc_len[b]);
    const int goff = uni(a.global_offset ? a.global_offset[b] : 0);
    const int emit_after = uni(a.emit_after ? a.emit_after[b] : -1);
    const int is_last = uni(a.is_last ? a.is_last[b] : 0);
    int t = uni(a.t0 ? a.t0[b] : 0);
    if (writer) a.final_time[b] = INT32_MIN;  // "timeJump not updated" (early returns, :110-112,:150-152)
    auto finish = [&]() { if (writer) { a.out_count[b] = count; a.final_u[b] = u; a.status[b] = st; } };
    if (enc_len <= 1) { finish(); return; }                        // :110-112
    const int Teff = min(enc_len, uni(a.audio_frames ? a.audio_frames[b] : enc_len));  // TdtFrameNavigation.swift:59-78
    if (t >= Teff) { finish(); return; }                           // :150-152
    const int last = Teff - 1;
    enum { OUTER = 0, INNER = 1, FLUSH = 2 };
    int phase = OUTER, last_emit_t = -1, n_at_t = 0, processed = 0, t_label = t;
    int steps = 0, blanks = 0, fp = 0;                             // last-chunk flush (:472-571)
    int route = 0;                                                 // LANG: what the filters did to the present decision
    float filtered_score = 0.0f;
    auto emit = [&](const int ts, const int tok, const int dur) {
        if (emit_after >= 0 && ts < emit_after) return;           // shouldEmitToken (:600-606)
        if (count < a.max_out) {
            float score;
            if constexpr (LANG) score = route ? filtered_score : clamp_probability(prob_of_last());
            else score = clamp_probability(prob_of_last());
            if (writer) { otok[count] = tok; otime[count] = ts; odur[count] = dur; oconf[count] = score; }
            if constexpr (LANG) { if (writer) out_route[count] = route; }
        } else st = FA_OUTPUT_TOO_SMALL;
        ++count;
    };
    for (;;) {
        int frame;
        if (phase == FLUSH) {
            if (!(steps < c.max_symbols_per_step && blanks < c.consecutive_blank_limit)) break;
            const int sel = steps % 3;                             // the three boundary-frame variants (:487-499)
            frame = sel == 0 ? min(fp, enc_len - 1) : (sel == 1 ? min(Teff - 1, enc_len - 1) : min(max(0, Teff - 2), enc_len - 1));
        } else {
            if (phase == INNER) t_label = t;                       // :349: the blank-advance loop labels the frame it is about to look at
            frame = min(t, last);
        }
        // ---- one joint decision (the single call site)
        if (u >= a.U || frame < 0 || frame >= a.T) { st = FA_OUTPUT_TOO_SMALL; finish(); return; }
        int tok = 0, bi = 0;
        decide(u, frame, tok, bi);
        tok = uni(tok); bi = uni(bi);
        if constexpr (LANG) {
            route = 0;
            if (phase != FLUSH) { route = uni(filter(u, frame, tok, filtered_score)); tok = uni(tok); }
        }
        if (bi < 0 || bi >= c.n_duration_bins) { st = FA_RUNTIME_ERROR; finish(); return; }  // mapDurationBin throws (TdtDurationMapping.swift:17-22)
        int dur = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) dur = bi == q ? c.duration_bins[q] : dur;   // (selects on the uniform bin: an indexed copy of the config would sit in scratch)
        const bool blank = tok == c.blank_id;
        if (phase == FLUSH) {
            if (blank) ++blanks;
            else { blanks = 0; emit(min(fp, Teff - 1) + goff, tok, dur); ++u; }
            fp = min(fp + max(1, dur), Teff);
            ++steps;
            continue;
        }
        if (phase == OUTER) {
            if (!blank && dur == 0 && t == last_emit_t && n_at_t >= 1) dur = 1;  // :318-323
            t_label = t;
        }
        if (blank && dur == 0) dur = 1;                                           // :327-329 / :377-379
        t += dur;
        bool active = t < Teff;
        if (active && blank) { phase = INNER; continue; }                         // :348-405: same predictor state, blanks only move the frame pointer
        bool stop = false;
        if (active && !blank) {                                                   // :409-463
            if (++processed > c.max_tokens_per_chunk) stop = true;
            else {
                emit(t_label + goff, tok, dur);
                ++u;                                                              // decoder LSTM step on the emitted token (:433-444)
                if (t_label == last_emit_t) ++n_at_t; else { last_emit_t = t_label; n_at_t = 1; }
                if (n_at_t >= c.max_symbols_per_step) {                           // force-advance (:453-462)
                    t = min(t + 1, last);
                    n_at_t = 0;
                    last_emit_t = -1;
                }
            }
        }
        active = t < Teff;
        if (active && !stop) { phase = OUTER; continue; }
        if (!is_last) break;
        phase = FLUSH; steps = 0; blanks = 0; fp = t;
    }
    if (writer) a.final_time[b] = t;
    finish();
}

__global__ void tdt_kernel(const TdtArgs a) {   // joint decisions from tables [B][U][T], one thread per chunk
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const int64_t tb = static_cast<int64_t>(b) * a.U * a.T;
    int64_t last = 0;
    tdt_walk<ThreadWalk>(a, b, true, [&](const int u, const int frame, int &tok, int &bin) {
        last = tb + static_cast<int64_t>(u) * a.T + frame;
        tok = a.tok[last]; bin = a.bin[last];
    }, [&]() -> float { return a.prob[last]; });
}

// Joint decisions computed on the fly from joint LOGITS [B][U][T][row_stride] (token logits [0, V1), duration logits [V1, V1 + nd)):
// what the reference's JointDecision model hands back (TdtModelInference.swift:84-188: token_id, token_prob, duration) —
// token = first-index argmax over the V1 token logits (strict '>', NaN never wins: the rule of LogitsArgmax.swift:16-55),
// probability = softmax probability of that token, duration bin = first-index argmax over the nd duration logits.  One
// wavefront per chunk walks the greedy path and touches ONLY the rows on it (~T + tokens rows of V1 + nd logits) instead of the
// U x T x (V1 + nd) grid a table-building pre-pass would need.  The models themselves are not in the reference tree: PARITY UNPINNED.
//
// Round 4: ONE WAVEFRONT per chunk (round 3: a 256-thread workgroup per chunk, three workgroup barriers and two passes over the row per
// decision — 4.2 us per decision, 3 % of the HBM roofline on 256 chunks).  A decision is latency, not work: ~4 KB of logits, an argmax and a
// soft-max denominator.  Within a wavefront both reductions stay in the VALU (DPP row shifts + row broadcasts; the first version used
// __shfl_xor: 36 LDS round trips per decision), the row is read ONCE (the denominator is accumulated against the running maximum, one
// rescale per batch of sixteen values), its loads are requested sixteen 256-byte pieces at a time and one batch ahead, and four times as
// many chunks fit a CU — the batch of chunks is the parallel axis of this kernel.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float tdt_dpp(const float old, const float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, ROWMASK, 0xf, false));
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int tdt_dpp(const int old, const int src) { return __builtin_amdgcn_update_dpp(old, src, CTRL, ROWMASK, 0xf, false); }
template <int CTRL, int ROWMASK>
__device__ __forceinline__ unsigned tdt_dpp(const unsigned old, const unsigned src) {
    return static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(old), static_cast<int>(src), CTRL, ROWMASK, 0xf, false));
}
template <int LANE> __device__ __forceinline__ float tdt_readlane(const float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), LANE)); }
template <int LANE> __device__ __forceinline__ int tdt_readlane(const int v) { return __builtin_amdgcn_readlane(v, LANE); }
template <int LANE> __device__ __forceinline__ unsigned tdt_readlane(const unsigned v) { return static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v), LANE)); }

// THE reduction of this unit, as the shifts it is made of: step(shift) runs once per shift, and shift(identity, v) is v of the lane 1, 2, 4 (, 8) to
// the left in its row of sixteen — row_shr; a lane without such a neighbour sees `identity` —, which leaves lane 15 of every row with the row's
// result (lane 7 with that of lanes 0 .. 7: LANES = 8 stops here, values elsewhere are ignored); then row_bcast15 into rows 1 and 3 and
// row_bcast31 into rows 2 and 3, after which lane 63 holds it all.
template <int CTRL, int ROWMASK>
struct TdtShift {
    template <class T> __device__ __forceinline__ T operator()(const T identity, const T v) const { return tdt_dpp<CTRL, ROWMASK>(identity, v); }
};
template <int LANES, class Step>
__device__ __forceinline__ void tdt_shifts(Step &&step) {
    static_assert(LANES == 64 || LANES == 8, "the 64 lanes of a wavefront, or its lanes 0 .. 7");
    step(TdtShift<0x111, 0xf>{}); step(TdtShift<0x112, 0xf>{}); step(TdtShift<0x114, 0xf>{});
    if constexpr (LANES == 64) { step(TdtShift<0x118, 0xf>{}); step(TdtShift<0x142, 0xa>{}); step(TdtShift<0x143, 0xc>{}); }
}
// one value per lane: v = combine(v, shifted v) at every step; every lane gets the result (uniform)
template <int LANES, class T, class Combine>
__device__ __forceinline__ T tdt_reduce(T v, const T identity, Combine &&combine) {
    tdt_shifts<LANES>([&](const auto shift) { v = combine(v, shift(identity, v)); });
    return tdt_readlane<LANES - 1>(v);
}
// first maximum of (value, index): lower index on equal values, NaN never present (callers keep it out); every lane gets the result
template <int LANES>
__device__ __forceinline__ void tdt_argmax(float &v, int &i) {
    tdt_shifts<LANES>([&](const auto shift) {
        const float ov = shift(-INFINITY, v);
        const int oi = shift(0x7fffffff, i);
        const bool t = (ov > v) | ((ov == v) & (oi < i));
        v = t ? ov : v; i = t ? oi : i;
    });
    v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), LANES - 1));
    i = __builtin_amdgcn_readlane(i, LANES - 1);
}
__device__ __forceinline__ void tdt_wave_argmax(float &v, int &i) { tdt_argmax<64>(v, i); }
__device__ __forceinline__ void tdt_low8_argmax(float &v, int &i) { tdt_argmax<8>(v, i); }   // the <= 8 duration logits
__device__ __forceinline__ float tdt_wave_max(const float v) { return tdt_reduce<64>(v, -INFINITY, [](const float x, const float o) { return __builtin_fmaxf(x, o); }); }
__device__ __forceinline__ float tdt_low8_max(const float v) { return tdt_reduce<8>(v, -INFINITY, [](const float x, const float o) { return __builtin_fmaxf(x, o); }); }
__device__ __forceinline__ unsigned tdt_wave_umin(const unsigned v) { return tdt_reduce<64>(v, 0xffffffffu, [](const unsigned x, const unsigned o) { return o < x ? o : x; }); }
// soft-max partials (m = maximum, s = sum of exp(x - m)) of the 64 lanes -> the wavefront's, in every lane: the maximum first (six DPP steps of
// one v_max), ONE rescale per lane, then the sum (six DPP adds) — the pairwise form spent two exp per step on the decision's dependent chain
__device__ __forceinline__ void tdt_wave_softmax(float &m, float &s) {
    const float M = tdt_reduce<64>(m, -INFINITY, [](const float x, const float o) { return o > x ? o : x; });
    const float t = m == -INFINITY ? 0.0f : s * __expf(m - M);     // a lane without a finite value holds s = 0
    m = M;
    s = tdt_reduce<64>(t, 0.0f, [](const float x, const float o) { return x + o; });
}

#include "tdt_lang.h"   // the language mode's filters and the top-K kernel, on the helpers above

// ---- rows of at most 17 x 64 logits (Parakeet-TDT's 1 025 + 5, the CTC-sized heads): the row stays in registers, in its own element type, from
// the decision until the next one.  A decision is: 17 + 1 requests from a scalar row address (the lane's byte offsets are loop invariants; offsets
// beyond the row are clamped to its last element — a duplicate of a real element can tie with it but never beat it, and the true holder has the
// lower index), the lane maximum (v_max: a NaN operand is dropped), six DPP steps for the row maximum M, and the FIRST index holding M as 17
// compares whose lane masks the scalar unit searches (piece j before piece j + 1, lowest lane within a piece: index = lane + 64 j) — ~90 vector
// instructions where the (value, index) scan + (value, index) DPP reduction of round 4 took ~250.  The soft-max runs from the registers, and only
// when the token is emitted.
//
// W = logits per request and lane (round 6).  A request of one HALF per lane moves 128 bytes per wavefront, and with those the fp16 walk was SLOWER than
// the fp32 walk of the same chunks (0.179 against 0.155 ms for 1 024 chunks) although it reads half the bytes.  fp16 rows whose every start is 4-byte
// aligned are therefore read as PAIRS (W = 2: nine requests of 256 bytes instead of seventeen of 128; 0.142 ms, 4 096 chunks 33 -> 40 % of HBM): logit e
// of piece j of lane l is W (l + 64 j) + e.  The first logit of a piece is a token logit or a clamped duplicate of one (as above); the others are masked
// to -inf by their index when they lie behind the last token logit (a duration logit or the next row's first; the masks are loop invariants).  Pieces of
// 512 bytes and more per wavefront (fp32 pairs / quads, fp16 quads / octets) measured SLOWER than 256: profiles/r06_tdt_piece_probe.txt.
typedef unsigned tdt_v2u __attribute__((ext_vector_type(2)));
typedef unsigned tdt_v4u __attribute__((ext_vector_type(4)));
template <bool F16, int W, bool LANG>
__device__ __forceinline__ void tdt_logits_fits_body(const TdtArgs &a, const TdtLogitArgs &g, const TdtLangArgs &l) {
    using E = std::conditional_t<F16, __half, float>;
    constexpr int kBytes = W * static_cast<int>(sizeof(E));   // per request and lane
    static_assert(W == 1 || kBytes == 4 || kBytes == 8 || kBytes == 16, "a request is one element or 1 / 2 / 4 dwords");
    constexpr int kReq = (kFitsPieces + W - 1) / W;   // requests per lane: 64 W kReq >= kFitsLogits (1 088) logits
    constexpr int kP = kReq * W;                 // logits per lane
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t tb = static_cast<int64_t>(b) * a.U * a.T;
    const int last_k = g.V1 - 1;
    auto index_of = [lane](const int j) { return W * (lane + 64 * (j / W)) + (j % W); };
    unsigned off[kReq];
#pragma unroll
    for (int j = 0; j < kReq; ++j) {
        const int k = W * (lane + 64 * j);
        const int lim = W == 1 ? last_k : last_k / W * W;                      // beyond the row: its last request again
        off[j] = static_cast<unsigned>(k < lim ? k : lim) * static_cast<unsigned>(sizeof(E));
    }
    const unsigned doff = static_cast<unsigned>(g.V1 + (lane < g.nd ? lane : g.nd - 1)) * static_cast<unsigned>(sizeof(E));
    const int row_bytes = (g.V1 + g.nd) * static_cast<int>(sizeof(E));
    int n_script = 0, n_block = 0;   // LANG: decisions the script filter / the blocklist replaced
    auto filter = [&](const int u, const int frame, int &tok, float &score) -> int {
        const void *row = static_cast<const char *>(g.logits) + (tb + static_cast<int64_t>(u) * a.T + frame) * g.row_stride * static_cast<int64_t>(sizeof(E));
        return tdt_lang_filter<F16>(l, row, g.V1, a.cfg.blank_id, tok, score, n_script, n_block);
    };
    float v[kP];   // fp16 rows are widened as they arrive (LogitsArgmax.swift:31-55 widens fp16 logits before the scan): one conversion per element —
                   // half-precision maxima (__hmax) compile to a NaN-handling branch per element
    tdt_walk<WaveWalk, LANG>(a, b, lane == 0, [&](const int u, const int frame, int &tok, int &bin) {
        // the row through a buffer descriptor: scalar base (the walk's state is scalar) + the lane's 32-bit byte offset = ONE instruction per
        // request (a flat global load of scalar base + lane offset is compiled as a 64-bit per-lane add and the load)
        char *rp = const_cast<char *>(static_cast<const char *>(g.logits)) + (tb + static_cast<int64_t>(u) * a.T + frame) * g.row_stride * static_cast<int64_t>(sizeof(E));
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(rp, 0, row_bytes, 0x00020000);
        auto fetch = [&](const unsigned byte_off) -> float {
            if constexpr (F16) return __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(rsrc, static_cast<int>(byte_off), 0, 0)));
            else return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, static_cast<int>(byte_off), 0, 0));
        };
        const float dve = fetch(doff);                                         // the duration logits travel with the row
        if constexpr (W == 1) {
#pragma unroll
            for (int j = 0; j < kReq; ++j) v[j] = fetch(off[j]);
        } else {
            constexpr int kDw = kBytes / 4;
            unsigned raw[kReq][kDw];
#pragma unroll
            for (int j = 0; j < kReq; ++j) {
                if constexpr (kDw == 1) raw[j][0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, static_cast<int>(off[j]), 0, 0);
                else if constexpr (kDw == 2) { const tdt_v2u q = __builtin_amdgcn_raw_buffer_load_b64(rsrc, static_cast<int>(off[j]), 0, 0); raw[j][0] = q.x; raw[j][1] = q.y; }
                else { const tdt_v4u q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, static_cast<int>(off[j]), 0, 0); raw[j][0] = q.x; raw[j][1] = q.y; raw[j][2] = q.z; raw[j][3] = q.w; }
            }
#pragma unroll
            for (int j = 0; j < kP; ++j) {
                float x;
                if constexpr (F16) {
                    const unsigned dw = raw[j / W][(j % W) / 2];
                    x = __half2float(__ushort_as_half(static_cast<unsigned short>((j & 1) ? dw >> 16 : dw & 0xffffu)));
                } else x = __uint_as_float(raw[j / W][j % W]);
                v[j] = (j % W == 0 || index_of(j) <= last_k) ? x : -INFINITY;
            }
        }
        float dv = lane < g.nd ? dve : -INFINITY;
        dv = dv != dv ? -INFINITY : dv;                                          // NaN never wins the first-maximum scan
        float me = v[0];
#pragma unroll
        for (int j = 1; j < kP; ++j) me = __builtin_fmaxf(me, v[j]);            // a NaN operand is dropped
        const float M = tdt_wave_max(me);                                         // all NaN: NaN; nothing above -inf: -inf
        // the FIRST index holding M: per lane the lowest of its logits that equals M (compares + selects, walked downwards so the lowest index is written
        // last), then the minimum of those indices over the wavefront — six v_min_u32 with a DPP operand.  Round 5 searched the 17 lane
        // masks on the scalar unit (ballot, compare, find-first, select per piece: 11 scalar instructions each, 318 per decision in r05_tdt_pmc.json).
        unsigned key = 0xffffffffu;
#pragma unroll
        for (int j = kP - 1; j >= 0; --j) key = v[j] == M ? static_cast<unsigned>(index_of(j)) : key;
        key = tdt_wave_umin(key);
        tok = (M > -INFINITY && key != 0xffffffffu) ? static_cast<int>(key) : 0;   // all NaN / -inf: index 0 (LogitsArgmax semantics: nothing beats the -inf seed)
        const float DM = tdt_low8_max(dv);
        const unsigned long long dmask = __builtin_amdgcn_ballot_w64(lane < g.nd && dv == DM);
        bin = (DM > -INFINITY && dmask != 0) ? __ffsll(static_cast<long long>(dmask)) - 1 : 0;   // first maximum; nothing above -inf: bin 0 (the scan's initial value)
    }, [&]() -> float {
        // soft-max of the row in the registers: lane maximum (NaN dropped), one exp per in-row value, then the wavefront's partials
        float m = -INFINITY, ssum = 0.0f;
        bool nan_seen = false;                     // a NaN logit anywhere in the row: probability 0 after the clamp
#pragma unroll
        for (int j = 0; j < kP; ++j) { const float x = v[j]; m = x > m ? x : m; nan_seen = nan_seen | (x != x); }
        const bool finite_max = m > -INFINITY;
#pragma unroll
        for (int j = 0; j < kP; ++j) { const float e = __expf(v[j] - m); ssum += (finite_max & (index_of(j) <= last_k)) ? e : 0.0f; }
        tdt_wave_softmax(m, ssum);
        return __builtin_amdgcn_ballot_w64(nan_seen) ? NAN : 1.0f / ssum;
    }, filter, LANG ? l.out_route + static_cast<int64_t>(b) * a.max_out : nullptr);
    if constexpr (LANG) { if (lane == 0) { l.swap_counts[2 * static_cast<int64_t>(b)] = n_script; l.swap_counts[2 * static_cast<int64_t>(b) + 1] = n_block; } }
}
template <bool F16, int W = 1>
__global__ __launch_bounds__(64) void tdt_logits_fits_kernel(const TdtArgs a, const TdtLogitArgs g) { tdt_logits_fits_body<F16, W, false>(a, g, TdtLangArgs{}); }
template <bool F16, int W = 1>
__global__ __launch_bounds__(64) void tdt_logits_fits_lang_kernel(const TdtArgs a, const TdtLogitArgs g, const TdtLangArgs l) { tdt_logits_fits_body<F16, W, true>(a, g, l); }

// ---- longer rows (8 198 logits: Parakeet-TDT v3): one pass, the soft-max partials (m, ssum) accumulated against the running maximum while the
// row streams through sixteen 256-byte pieces at a time, the NEXT sixteen requested before the present ones are looked at
template <bool F16, bool LANG>
__device__ __forceinline__ void tdt_logits_body(const TdtArgs &a, const TdtLogitArgs &g, const TdtLangArgs &l) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t tb = static_cast<int64_t>(b) * a.U * a.T;
    auto at = [&](const int64_t row, const int k) -> float {   // row: wave-uniform (a scalar base address), k: the lane's element
        if (F16) return __half2float((static_cast<const __half *>(g.logits) + row * g.row_stride)[k]);
        return (static_cast<const float *>(g.logits) + row * g.row_stride)[k];
    };
    constexpr int kBatch = 16;
    float m_on = -INFINITY, s_on = 0.0f;              // one-pass partials of the present row
    bool nan_seen = false;                            // a NaN logit anywhere in the row: probability 0 after the clamp (what the two-pass sum of round 3 gave)
    int n_script = 0, n_block = 0;                    // LANG: decisions the script filter / the blocklist replaced
    auto filter = [&](const int u, const int frame, int &tok, float &score) -> int {
        const void *row = static_cast<const char *>(g.logits) + (tb + static_cast<int64_t>(u) * a.T + frame) * g.row_stride * static_cast<int64_t>(F16 ? 2 : 4);
        return tdt_lang_filter<F16>(l, row, g.V1, a.cfg.blank_id, tok, score, n_script, n_block);
    };
    tdt_walk<WaveWalk, LANG>(a, b, lane == 0, [&](const int u, const int frame, int &tok, int &bin) {
        const int64_t row = tb + static_cast<int64_t>(u) * a.T + frame;
        float dvl = lane < g.nd ? at(row, g.V1 + lane) : -INFINITY;            // the duration logits travel with the first batch of the row
        if (dvl != dvl) dvl = -INFINITY;                                       // NaN never wins the first-maximum scan
        // per-lane: first maximum over k = lane, lane + 64, ... (ascending, strict '>': NaN never wins) and the soft-max partials (m, ssum)
        float bv = -INFINITY, m = -INFINITY, ssum = 0.0f, v[kBatch], vn[kBatch];
        int bi = 0x7fffffff;
        nan_seen = false;
        auto request = [&](float (&dst)[kBatch], const int k0) {
#pragma unroll
            for (int j = 0; j < kBatch; ++j) { const int k = k0 + 64 * j; dst[j] = k < g.V1 ? at(row, k) : -INFINITY; }
        };
        request(v, lane);
        for (int k0 = lane; k0 < g.V1; k0 += 64 * kBatch) {
            request(vn, k0 + 64 * kBatch);                                          // (beyond the row: no loads, -inf)
            const int kbase = k0 - lane;                                             // wave-uniform: pieces at or beyond the row's end are skipped by a scalar branch
            float bm = -INFINITY;                                                    // maximum of the batch first: one exp per value, one rescale per batch
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {                                       // selects, no per-lane branches: the decision is a dependent chain
                if (kbase + 64 * j >= g.V1) break;
                const bool t = v[j] > bv;                                            // (slots beyond the row hold -inf and never win)
                bv = t ? v[j] : bv; bi = t ? k0 + 64 * j : bi;
                bm = v[j] > bm ? v[j] : bm;
            }
            {
                const bool up = bm > m;
                const float rescaled = m == -INFINITY ? 0.0f : ssum * __expf(m - bm);
                ssum = up ? rescaled : ssum; m = up ? bm : m;
            }
            const bool finite_max = m > -INFINITY;
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                if (kbase + 64 * j >= g.V1) break;
                const bool in_row = k0 + 64 * j < g.V1;
                nan_seen = nan_seen | (in_row & (v[j] != v[j]));
                const float e = __expf(v[j] - m);
                ssum += (in_row & finite_max) ? e : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) v[j] = vn[j];
        }
        m_on = m; s_on = ssum;
        tdt_wave_argmax(bv, bi);
        tok = bi == 0x7fffffff ? 0 : bi;           // all NaN / -inf: index 0 (LogitsArgmax semantics)
        float dv = dvl;
        int di = lane < g.nd ? lane : 0x7fffffff;
        tdt_low8_argmax(dv, di);                                                // the <= 8 duration logits sit in lanes 0 .. 7: three DPP steps
        bin = (di == 0x7fffffff || !(dv > -INFINITY)) ? 0 : di;                 // first maximum; nothing above -inf: bin 0 (the scan's initial value)
    }, [&]() -> float {
        float m = m_on, ssum = s_on;
        tdt_wave_softmax(m, ssum);
        return __builtin_amdgcn_ballot_w64(nan_seen) ? NAN : 1.0f / ssum;
    }, filter, LANG ? l.out_route + static_cast<int64_t>(b) * a.max_out : nullptr);
    if constexpr (LANG) { if (lane == 0) { l.swap_counts[2 * static_cast<int64_t>(b)] = n_script; l.swap_counts[2 * static_cast<int64_t>(b) + 1] = n_block; } }
}
template <bool F16>
__global__ __launch_bounds__(64) void tdt_logits_kernel(const TdtArgs a, const TdtLogitArgs g) { tdt_logits_body<F16, false>(a, g, TdtLangArgs{}); }
template <bool F16>
__global__ __launch_bounds__(64) void tdt_logits_lang_kernel(const TdtArgs a, const TdtLogitArgs g, const TdtLangArgs l) { tdt_logits_body<F16, true>(a, g, l); }

}  // namespace

namespace fa {
namespace tdt {

void launch_tables(hipStream_t stream, const TdtArgs &a) { hipLaunchKernelGGL(tdt_kernel, dim3((a.B + 63) / 64), dim3(64), 0, stream, a); }

void launch_logits(hipStream_t stream, const TdtArgs &a, const TdtLogitArgs &g) {
    const Route route = logits_route(g.f16 != 0, g.V1, g.row_stride, reinterpret_cast<uintptr_t>(g.logits));
    const dim3 grid(a.B), block(64);
    if (g.f16) {
        if (route == kStream) hipLaunchKernelGGL(tdt_logits_kernel<true>, grid, block, 0, stream, a, g);
        else if (route == kFitsPairs) hipLaunchKernelGGL((tdt_logits_fits_kernel<true, 2>), grid, block, 0, stream, a, g);
        else hipLaunchKernelGGL((tdt_logits_fits_kernel<true, 1>), grid, block, 0, stream, a, g);
    } else {
        if (route == kStream) hipLaunchKernelGGL(tdt_logits_kernel<false>, grid, block, 0, stream, a, g);
        else hipLaunchKernelGGL((tdt_logits_fits_kernel<false, 1>), grid, block, 0, stream, a, g);
    }
}

void launch_logits_lang(hipStream_t stream, const TdtArgs &a, const TdtLogitArgs &g, const TdtLangArgs &l) {
    const Route route = logits_route(g.f16 != 0, g.V1, g.row_stride, reinterpret_cast<uintptr_t>(g.logits));
    const dim3 grid(a.B), block(64);
    if (g.f16) {
        if (route == kStream) hipLaunchKernelGGL(tdt_logits_lang_kernel<true>, grid, block, 0, stream, a, g, l);
        else if (route == kFitsPairs) hipLaunchKernelGGL((tdt_logits_fits_lang_kernel<true, 2>), grid, block, 0, stream, a, g, l);
        else hipLaunchKernelGGL((tdt_logits_fits_lang_kernel<true, 1>), grid, block, 0, stream, a, g, l);
    } else {
        if (route == kStream) hipLaunchKernelGGL(tdt_logits_lang_kernel<false>, grid, block, 0, stream, a, g, l);
        else hipLaunchKernelGGL((tdt_logits_fits_lang_kernel<false, 1>), grid, block, 0, stream, a, g, l);
    }
}

void launch_topk(hipStream_t stream, const TdtTopkArgs &k) {
    const dim3 grid(static_cast<unsigned>(k.R)), block(64);
    if (k.f16) hipLaunchKernelGGL(tdt_topk_kernel<true>, grid, block, 0, stream, k);
    else hipLaunchKernelGGL(tdt_topk_kernel<false>, grid, block, 0, stream, k);
}

}  // namespace tdt
}  // namespace fa
