// rnnt.hip — streaming RNN-T greedy decoding with decode-time hotword biasing (gfx950).
//
// Restates the greedy loop of RnntDecoder.decodeWithEOU (reference: Sources/FluidAudio/ASR/Parakeet/Streaming/RnntDecoder.swift:73-127;
// StreamingNemotronMultilingualAsrManager+Decode.swift:189-251, 278-440 is the same loop behind a speculative scan) with the biased
// selection of NemotronVocabularyBias.swift:55-340 (the matcher) and :465-498 (selectToken / pickBiased) at its one decision site.
//
// As in the TDT walk (tdt.hip), the decoder and joint networks are CoreML models outside the reference tree: the entry consumes joint
// LOGITS indexed by (u = decoder steps taken so far in this chunk, t = encoder frame), and one wavefront per stream walks the greedy path
// through wave-uniform control flow, reading only the rows on it.  A decision is the first-index argmax of the row (LogitsArgmax's rule:
// fp16 widened, NaN never wins, nothing above -inf gives 0) and, with a vocabulary, the best boosted candidate: logit[id] + boost, one
// fp32 add (this unit is built with -ffp-contract=off), taken when it is STRICTLY above logit[plain].  Among candidates of equal score
// the lowest token id wins — the reference iterates a Dictionary there, whose order is unspecified; this library defines it.
//
// THE MATCHER.  The reference re-walks every suffix of the emitted tail through its trie after each emission.  Here a lane holds suffix
// starts (slot = lane + 64 pass of a ring of tail_cap scalars in LDS) and, per start, the trie node its suffix has reached, or "dead", in
// registers together with that node's candidate list.  An emitted scalar advances every live suffix by one child look-up — a bounded
// binary search in the blob's sorted edge arrays — and opens one new suffix at the root.  A suffix as long as the longest form has no
// child, so the ring overwriting its oldest start never drops a live match.  Between emissions the live set is fixed: a decision costs
// the gathers of logit[id] for the depth-0 list and the live nodes' lists, and one wave maximum on (score, id).
//
// MEMORY SAFETY OF THE BLOB.  It sits in device memory the host entry cannot inspect: the header is checked against the launch arguments
// (rnnt_bias_core.h: read_header), every offset and length taken from it is compared with bias_words before it forms an address, and a
// violation ends the stream with RUNTIME_ERROR.  Loop bounds are launch arguments or lengths checked against them.
//
// This unit: the kernel and its launcher.  Host side (argument checks, bias tables, C ABI): rnnt_host.hip; shared: rnnt_launch.h.
#include <hip/hip_fp16.h>

#include "rnnt_launch.h"

namespace {

using namespace fa::rnnt;
namespace rb = fa::rnnt_bias;

__device__ __forceinline__ int uni(const int x) { return __builtin_amdgcn_readfirstlane(x); }

// ---- the wave reduction (restated from tdt.hip): row_shr 1, 2, 4, 8 leave lane 15 of every row of sixteen with the row's result, row_bcast15
// carries it into rows 1 and 3, row_bcast31 into rows 2 and 3; lane 63 holds it all.  A lane without a left neighbour sees `old`.
template <int CTRL, int ROWMASK> __device__ __forceinline__ float rnnt_dpp(const float old, const float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, ROWMASK, 0xf, false));
}
template <int CTRL, int ROWMASK> __device__ __forceinline__ int rnnt_dpp(const int old, const int src) { return __builtin_amdgcn_update_dpp(old, src, CTRL, ROWMASK, 0xf, false); }
// first maximum of (value, index) over the wavefront: the higher value, the lower index among equal values; NaN never present (callers keep it
// out); every lane gets the result
__device__ __forceinline__ void rnnt_wave_argmax(float &v, int &i) {
    auto step = [&](const float ov, const int oi) {
        const bool t = (ov > v) | ((ov == v) & (oi < i));
        v = t ? ov : v; i = t ? oi : i;
    };
    step(rnnt_dpp<0x111, 0xf>(-INFINITY, v), rnnt_dpp<0x111, 0xf>(0x7fffffff, i));
    step(rnnt_dpp<0x112, 0xf>(-INFINITY, v), rnnt_dpp<0x112, 0xf>(0x7fffffff, i));
    step(rnnt_dpp<0x114, 0xf>(-INFINITY, v), rnnt_dpp<0x114, 0xf>(0x7fffffff, i));
    step(rnnt_dpp<0x118, 0xf>(-INFINITY, v), rnnt_dpp<0x118, 0xf>(0x7fffffff, i));
    step(rnnt_dpp<0x142, 0xa>(-INFINITY, v), rnnt_dpp<0x142, 0xa>(0x7fffffff, i));
    step(rnnt_dpp<0x143, 0xc>(-INFINITY, v), rnnt_dpp<0x143, 0xc>(0x7fffffff, i));
    v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    i = __builtin_amdgcn_readlane(i, 63);
}
__device__ __forceinline__ bool wave_any(const bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

template <bool F16>
__global__ __launch_bounds__(64) void rnnt_greedy_kernel(const RnntArgs a) {
    __shared__ int32_t ring[kMaxTail];                    // the tail's scalars; logical position j is ring[(head + j) % cap]
    const int b = blockIdx.x, lane = threadIdx.x;
    const fa_rnnt_config &c = a.cfg;
    const int V1 = a.V1, cap = a.tail_cap;
    const int32_t *const blob = a.bias;
    const bool biased = blob != nullptr;
    int32_t *otok = a.out_tok + static_cast<int64_t>(b) * a.max_out, *oframe = a.out_frame + static_cast<int64_t>(b) * a.max_out;
    int32_t *oplain = a.out_plain + static_cast<int64_t>(b) * a.max_out;
    int count = 0, u = 0, st = FA_SUCCESS, eou = 0;
    auto finish = [&]() { if (lane == 0) { a.out_count[b] = count; a.final_u[b] = u; a.eou[b] = eou; a.status[b] = st; } };
    auto at = [&](const int64_t row, const int k) -> float {   // row: wave-uniform, k: the lane's element, inside the row
        if (F16) return __half2float((static_cast<const __half *>(a.logits) + row * a.row_stride)[k]);
        return (static_cast<const float *>(a.logits) + row * a.row_stride)[k];
    };

    // ---- the match state
    rb::Header h = {};
    int node[kTailPasses], cfirst[kTailPasses], ccount[kTailPasses];   // per suffix start of this lane: its trie node (-1: dead) and that node's list
    int root_first = 0, root_count = 0, head = 0, len = 0;
#pragma unroll
    for (int p = 0; p < kTailPasses; ++p) { node[p] = -1; cfirst[p] = 0; ccount[p] = 0; }
    // the candidate list of every live suffix start of this lane; false: the blob broke its own bounds
    auto lists = [&]() -> bool {
        bool ok = true;
#pragma unroll
        for (int p = 0; p < kTailPasses; ++p) {
            if (64 * p >= cap) break;
            ccount[p] = 0;
            if (node[p] >= 0) { ok = rb::node_candidates(blob, h, node[p], cfirst[p], ccount[p]) && ok; if (!ok) ccount[p] = 0; }
        }
        return !wave_any(!ok);
    };
    // one scalar behind the tail: the oldest start makes room when the ring is full, the new start opens at the root, every live start advances
    auto append = [&](const uint32_t scalar) -> bool {
        int slot;
        if (len == cap) { slot = head; head = head + 1 == cap ? 0 : head + 1; }
        else { slot = head + len; slot = slot >= cap ? slot - cap : slot; ++len; }
        if (lane == 0) ring[slot] = static_cast<int32_t>(scalar);
        bool ok = true;
#pragma unroll
        for (int p = 0; p < kTailPasses; ++p) {
            if (64 * p >= cap) break;
            const int mine = lane + 64 * p;
            int n = mine == slot ? 0 : node[p];
            if (n >= 0) { int child; ok = rb::node_child(blob, h, n, scalar, child) && ok; n = child; }
            node[p] = n;
        }
        return !wave_any(!ok);
    };
    if (biased) {
        const rb::HeaderVerdict verdict = rb::read_header(blob, a.bias_words, V1, cap, h);   // (uniform: every lane reads the same words)
        if (verdict != rb::kHeaderOk) { st = verdict == rb::kHeaderMismatch ? FA_INVALID_ARGUMENT : FA_RUNTIME_ERROR; finish(); return; }
        if (!rb::node_candidates(blob, h, 0, root_first, root_count)) { st = FA_RUNTIME_ERROR; finish(); return; }
        root_first = uni(root_first); root_count = uni(root_count);
        len = uni(a.tail_len[b]);
        len = len < 0 ? 0 : (len > cap ? cap : len);
        const int32_t *tin = a.tail + static_cast<int64_t>(b) * cap;
        for (int j = lane; j < len; j += 64) ring[j] = tin[j];
        __syncthreads();
        // the carried state is the scalars: every lane walks its own suffixes through the trie, as the reference's candidates() does (:285-301)
        bool ok = true;
#pragma unroll
        for (int p = 0; p < kTailPasses; ++p) {
            if (64 * p >= cap) break;
            const int mine = lane + 64 * p;
            int n = mine < len ? 0 : -1;
            for (int j = mine; j < len && n >= 0 && ok; ++j) { int child; ok = rb::node_child(blob, h, n, static_cast<uint32_t>(ring[j]), child); n = child; }
            node[p] = n;
        }
        if (wave_any(!ok) || !lists()) { st = FA_RUNTIME_ERROR; finish(); return; }
    }
    // observe (:254-261): the scalars of the token's folded piece go behind the tail; a token without a piece leaves it alone
    auto observe = [&](const int tok) -> bool {
        int first = 0, n = 0;
        if (!rb::piece_span(blob, h, tok, first, n)) return false;
        first = uni(first); n = uni(n);
        for (int base = 0; base < n; base += 64) {
            const int here = min(64, n - base);
            const int mine = lane < here ? static_cast<int>(rb::piece_scalar(blob, h, first + base + lane)) : 0;
            for (int j = 0; j < here; ++j)
                if (!append(static_cast<uint32_t>(__shfl(mine, j)))) return false;
        }
        return n == 0 || lists();
    };
    auto write_back = [&]() {
        if (!biased) return;
        __syncthreads();
        int32_t *tout = a.tail + static_cast<int64_t>(b) * cap;
        for (int j = lane; j < len; j += 64) { int s = head + j; s = s >= cap ? s - cap : s; tout[j] = ring[s]; }
        if (lane == 0) a.tail_len[b] = len;
    };

    const int frames = uni(a.frames[b]);
    const int maxT = max(0, min(frames, a.T));                                   // RnntDecoder.swift:85
    const int start = min(max(0, uni(a.skip ? a.skip[b] : 0)), maxT);            // :88
    const int64_t tb = static_cast<int64_t>(b) * a.U * a.T;
    constexpr int kBatch = 8;
    bool done = false;
    for (int t = start; t < maxT && !done; ++t) {
        for (int symbols = 0; symbols < c.max_symbols_per_step; ++symbols) {      // :98
            if (u >= a.U) { st = FA_OUTPUT_TOO_SMALL; done = true; break; }
            const int64_t row = tb + static_cast<int64_t>(u) * a.T + t;
            // ---- plain: per lane the first maximum over k = lane, lane + 64, ... (ascending, strict '>': NaN never wins), kBatch loads in flight
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int k0 = lane; k0 - lane < V1; k0 += 64 * kBatch) {
                float v[kBatch];
#pragma unroll
                for (int j = 0; j < kBatch; ++j) { const int k = k0 + 64 * j; v[j] = k < V1 ? at(row, k) : -INFINITY; }
#pragma unroll
                for (int j = 0; j < kBatch; ++j) { const bool up = v[j] > bv; bv = up ? v[j] : bv; bi = up ? k0 + 64 * j : bi; }
            }
            rnnt_wave_argmax(bv, bi);
            const int plain = bi == 0x7fffffff ? 0 : bi;       // all NaN / -inf: index 0 (LogitsArgmax semantics)
            int tok = plain, displaced = -1;
            if (biased) {                                      // pickBiased (:482-498)
                float best = -INFINITY;
                int best_id = 0x7fffffff;
                auto offer = [&](const int index) {
                    int id;
                    float boost;
                    rb::candidate(blob, h, index, id, boost);
                    if (id < 0 || id >= V1) return;            // `where candidate.tokenId < count`: never read
                    const float score = at(row, id) + boost;   // NaN: no comparison below holds
                    const bool up = (score > best) | ((score == best) & (id < best_id));
                    best = up ? score : best; best_id = up ? id : best_id;
                };
                for (int i = lane; i < root_count; i += 64) offer(root_first + i);
#pragma unroll
                for (int p = 0; p < kTailPasses; ++p) {
                    if (64 * p >= cap) break;
                    for (int i = 0; i < ccount[p]; ++i) offer(cfirst[p] + i);
                }
                rnnt_wave_argmax(best, best_id);
                const float plain_logit = __int_as_float(uni(__float_as_int(at(row, plain))));
                if (best > plain_logit && best_id != plain) { displaced = plain; tok = best_id; }
            }
            if (tok == c.blank_id) break;                      // :106
            if (tok == c.eou_id) { eou = 1; done = true; break; }   // :108-111
            if (count < a.max_out) { if (lane == 0) { otok[count] = tok; oframe[count] = t; oplain[count] = displaced; } }
            else st = FA_OUTPUT_TOO_SMALL;
            ++count;
            ++u;                                               // the predictor state advances on a non-blank only (:117-119)
            if (biased && !observe(tok)) { st = FA_RUNTIME_ERROR; done = true; break; }
        }
    }
    write_back();
    finish();
}

}  // namespace

namespace fa {
namespace rnnt {

void launch_greedy(hipStream_t stream, const RnntArgs &a) {
    const Plan p = plan_of(a.B);
    if (a.f16) hipLaunchKernelGGL(rnnt_greedy_kernel<true>, dim3(p.grid), dim3(p.block), 0, stream, a);
    else hipLaunchKernelGGL(rnnt_greedy_kernel<false>, dim3(p.grid), dim3(p.block), 0, stream, a);
}

}  // namespace rnnt
}  // namespace fa
