// tdt_lang.h — the language mode of the TDT walk on joint logits: the row's top-K list as this library defines it, the script filter and the
// blocklist pass (TdtDecoderV3.swift:635-703, Shared/TokenLanguageFilter.swift:136-186).  Part of tdt.hip: included there, inside its unnamed
// namespace, behind the wavefront helpers it is made of.  Everything here runs with all 64 lanes of ONE wavefront in wave-uniform control flow.
//
// THE LIST (fa_tdt_topk_rows_dev hands it out): the min(K, V1) tokens of a row in order of descending key, then ascending id; key = the logit
// widened to float32, NaN counting as -inf, compared BY VALUE (-0.0 == +0.0: a selection on raw bit patterns would rank +0.0 first).
//
// The walk never materialises it.  A filter asks for the list's first entry of some class.  The list is sorted, so that entry is the best token of
// the class in the whole row (greatest key, lowest id) if that token's rank — the tokens with a greater key, or an equal key and a lower id — is
// below K, and there is none otherwise: one pass for the best token and the row's maximum, one counting pass for its rank.  The confidence needs
// the sum of exp(x - M) over the list.  Equal keys have equal terms, so WHICH of the tokens tied at the K-th key the list admits does not matter,
// only how many: the K-th greatest key tau by exact selection over the four bytes of an order-preserving key, most significant first (the method
// of paraformer.hip's pf_floor, the histogram in 1 KiB of LDS), then one pass adding the terms above tau, and the ties' term times their number.
// Seven passes over a row (tdt_row_each: eight requests in flight per lane), re-read from L2 by every route (the register routes' copy of the
// row is left alone: one code path, and the plain decision keeps its registers); only a decision whose winner is in the wrong script or on the
// blocklist pays them.
#pragma once

constexpr int kNoToken = 0x7fffffff;

template <bool F16>
struct TdtRow {
    const void *p;
    int V1;
    __device__ __forceinline__ float key(const int k) const {   // widened; NaN counts as -inf
        const float x = F16 ? __half2float(static_cast<const __half *>(p)[k]) : static_cast<const float *>(p)[k];
        return x != x ? -INFINITY : x;
    }
};

// f(k, key, in) for the lane's tokens k = lane, lane + 64, ...: eight loads are requested before the first is looked at (a pass is a chain of L2
// round trips, not arithmetic).  The calls of a batch are unconditional: in == false marks a slot behind the row, whose k and key are the last
// token's and which f must not count.
template <bool F16, class F>
__device__ __forceinline__ void tdt_row_each(const TdtRow<F16> row, const int lane, F &&f) {
    constexpr int kBatch = 8;
    for (int k0 = lane; k0 < row.V1; k0 += 64 * kBatch) {
        float x[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) x[j] = row.key(min(k0 + 64 * j, row.V1 - 1));
#pragma unroll
        for (int j = 0; j < kBatch; ++j) f(min(k0 + 64 * j, row.V1 - 1), x[j], k0 + 64 * j < row.V1);
    }
}

// ascending as unsigned where the keys ascend; -0.0 and +0.0 are one key
__device__ __forceinline__ unsigned tdt_order_key(const float v) {
    const unsigned u = __float_as_uint(v == 0.0f ? 0.0f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tdt_order_value(const unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ int tdt_wave_count(const int v) { return tdt_reduce<64>(v, 0, [](const int x, const int o) { return x + o; }); }

// tau = the Kc-th greatest key of the row (1 <= Kc <= V1), ties = how many of the list's Kc entries hold it (>= 1).  hist: 256 counters in LDS.
template <bool F16>
__device__ __forceinline__ void tdt_select(const TdtRow<F16> row, const int Kc, unsigned *hist, const int lane, float &tau, int &ties) {
    unsigned prefix = 0, mask = 0;
    int need = Kc;
    for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
        for (int q = 0; q < 4; ++q) hist[lane + 64 * q] = 0;
        __syncthreads();
        tdt_row_each(row, lane, [&](const int, const float x, const bool in) {
            const unsigned u = tdt_order_key(x);
            if (in && (u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        });
        __syncthreads();
        // lane l looks at the digits 255 - 4 l ... 252 - 4 l, greatest first; an inclusive sum over the lanes finds the lane, then the digit, at
        // which the count from the top reaches `need`
        int h[4], mine = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { h[q] = static_cast<int>(hist[255 - (4 * lane + q)]); mine += h[q]; }
        int incl = mine;
        tdt_shifts<64>([&](const auto shr) { incl += shr(0, incl); });
        const unsigned long long reached = __builtin_amdgcn_ballot_w64(incl >= need);   // never empty: the candidates of this digit are >= need
        const int L = __ffsll(static_cast<long long>(reached)) - 1;
        int above = __builtin_amdgcn_readlane(incl - mine, L), digit = 255 - 4 * L;
        bool found = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int hq = __builtin_amdgcn_readlane(h[q], L);
            if (!found) {
                if (above + hq >= need) { digit = 255 - (4 * L + q); found = true; }
                else above += hq;
            }
        }
        need -= above;
        prefix |= static_cast<unsigned>(digit) << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    tau = tdt_order_value(prefix);
    ties = need;
}

// The first entry of the row's list whose class byte has every bit of `need`, none of `forbid`, and whose id is not `skip` (-1: nothing to skip):
// its id and key, and the row's greatest key M.  false: the list has no such entry.
template <bool F16>
__device__ __forceinline__ bool tdt_list_first(const TdtRow<F16> row, const uint8_t *classes, const unsigned need, const unsigned forbid, const int skip,
                                               const int Kc, const int lane, int &id, float &xb, float &M) {
    float bv = -INFINITY, m = -INFINITY;
    int bi = kNoToken;
    tdt_row_each(row, lane, [&](const int k, const float x, const bool in) {   // ascending ids: the first of equal keys stays; the first match wins even at -inf
        const unsigned c = classes[k];
        const bool take = in & ((c & need) == need) & ((c & forbid) == 0) & (k != skip) & ((bi == kNoToken) | (x > bv));
        m = x > m ? x : m;                                         // (a slot behind the row repeats the last token's key)
        bv = take ? x : bv; bi = take ? k : bi;
    });
    tdt_wave_argmax(bv, bi);                                       // (-inf, kNoToken) of a lane without a match loses to any match
    M = tdt_wave_max(m);
    if (bi == kNoToken) return false;
    int rank = 0;
    tdt_row_each(row, lane, [&](const int k, const float x, const bool in) { rank += (in & ((x > bv) | ((x == bv) & (k < bi)))) ? 1 : 0; });
    if (tdt_wave_count(rank) >= Kc) return false;
    id = bi; xb = bv;
    return true;
}

// sum over the list of exp(x - M), M the row's greatest key and finite
template <bool F16>
__device__ __forceinline__ float tdt_list_sum(const TdtRow<F16> row, const int Kc, const float M, unsigned *hist, const int lane) {
    float tau;
    int ties;
    tdt_select(row, Kc, hist, lane, tau, ties);
    float s = 0.0f;
    tdt_row_each(row, lane, [&](const int, const float x, const bool in) { s += (in & (x > tau)) ? __expf(x - M) : 0.0f; });
    s = tdt_reduce<64>(s, 0.0f, [](const float x, const float o) { return x + o; });
    return s + static_cast<float>(ties) * __expf(tau - M);
}

// The two filters on a decision that one of them may change.  NOT inlined: a call keeps the seven passes' registers and code out of the walk's
// loop, whose plain decision — the common case — is a chain of dependent instructions that slows down with every register the loop carries
// (inlined, the never-firing walk of 1 024 chunks took 0.231 ms against 0.164 ms with the call).  Operands and result by value.
struct TdtSwap { int tok; float score; int route; };
template <bool F16>
__device__ __attribute__((noinline)) TdtSwap tdt_lang_replace(const uint8_t *classes, const unsigned script_bit, const int use_blocklist, const int top_k,
                                                              const void *row_ptr, const int V1, const int blank, const int tok0, unsigned *hist) {
    const int lane = threadIdx.x;
    const TdtRow<F16> row{row_ptr, V1};
    const int Kc = min(top_k, V1);
    TdtSwap r{tok0, 0.0f, 0};
    float S = 0.0f;
    bool have_sum = false;
    auto replace = [&](const unsigned need, const unsigned forbid, const int skip, const int bit) {
        int id = 0;
        float xb = 0.0f, M = 0.0f;
        if (!tdt_list_first(row, classes, need, forbid, skip, Kc, lane, id, xb, M)) return;
        r.tok = id;
        r.route |= bit;
        if (!(M - M == 0.0f)) { r.score = 0.0f; return; }           // the list's maximum is not finite (TokenLanguageFilter.swift:176)
        if (!have_sum) { S = tdt_list_sum(row, Kc, M, hist, lane); have_sum = true; }
        r.score = fa::tdt::clamp_probability(__expf(xb - M) / S);
    };
    unsigned c = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(classes[tok0]));
    if ((c & FA_TDT_CLASS_IN_VOCAB) && !(c & script_bit)) {                                     // TdtDecoderV3.swift:676-703
        replace(FA_TDT_CLASS_IN_VOCAB | script_bit, 0u, -1, FA_TDT_ROUTE_SCRIPT_SWAP);
        if (r.route) c = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(classes[r.tok]));
    }
    if (use_blocklist && r.tok != blank && (c & FA_TDT_CLASS_BLOCKLISTED))                      // :635-667, on the possibly replaced label
        replace(FA_TDT_CLASS_IN_VOCAB | FA_TDT_CLASS_LATIN_OK, FA_TDT_CLASS_BLOCKLISTED, blank, FA_TDT_ROUTE_BLOCKLIST_SWAP);
    return r;
}

// The hook of the walk: one class byte per non-blank decision; the call only for a winner in the wrong script or on the blocklist.  Returns the
// FA_TDT_ROUTE_* bits; where one is set, tok is the replacement and score its confidence.  n_script / n_block count the replacements.
template <bool F16>
__device__ __forceinline__ int tdt_lang_filter(const fa::tdt::TdtLangArgs &l, const void *row_ptr, const int V1, const int blank, int &tok, float &score,
                                               int &n_script, int &n_block) {
    __shared__ unsigned hist[256];
    if (tok == blank) return 0;
    const unsigned c = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(l.classes[tok]));
    const bool wrong_script = (c & FA_TDT_CLASS_IN_VOCAB) && !(c & static_cast<unsigned>(l.script_bit));
    if (!wrong_script && !(l.use_blocklist && (c & FA_TDT_CLASS_BLOCKLISTED))) return 0;
    const TdtSwap r = tdt_lang_replace<F16>(l.classes, static_cast<unsigned>(l.script_bit), l.use_blocklist, l.top_k, row_ptr, V1, blank, tok, hist);
    const int route = __builtin_amdgcn_readfirstlane(r.route);
    if (route) { tok = __builtin_amdgcn_readfirstlane(r.tok); score = r.score; }
    n_script += route & FA_TDT_ROUTE_SCRIPT_SWAP;
    n_block += (route >> 1) & 1;
    return route;
}

// fa_tdt_topk_rows_dev: the list itself, one wavefront per row.  The selection names the survivors — the keys above tau and, in ascending id, as
// many of those at tau as the list admits —; they are packed into LDS in id order and every lane finds the rank of its own among the at most 64.
template <bool F16>
__global__ __launch_bounds__(64) void tdt_topk_kernel(const fa::tdt::TdtTopkArgs t) {
    __shared__ unsigned hist[256];
    __shared__ float sv[64];
    __shared__ int si[64];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const TdtRow<F16> row{static_cast<const char *>(t.rows) + r * t.row_stride * static_cast<int64_t>(F16 ? 2 : 4), t.V1};
    const int Kc = min(t.K, t.V1);
    float tau;
    int ties;
    tdt_select(row, Kc, hist, lane, tau, ties);
    const unsigned long long lower = (1ull << lane) - 1ull;
    int n = 0, ties_seen = 0;
    for (int k0 = 0; k0 < t.V1; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < t.V1;
        const float x = in ? row.key(k) : -INFINITY;
        const bool eq = in & (x == tau);
        const unsigned long long eqs = __builtin_amdgcn_ballot_w64(eq);
        const bool admit = (in & (x > tau)) | (eq & (ties_seen + __popcll(eqs & lower) < ties));
        const unsigned long long adm = __builtin_amdgcn_ballot_w64(admit);
        const int slot = n + __popcll(adm & lower);
        if (admit && slot < 64) { sv[slot] = x; si[slot] = k; }
        n += __popcll(adm);
        ties_seen += __popcll(eqs);
    }
    n = min(n, 64);
    __syncthreads();
    const float v = lane < n ? sv[lane] : 0.0f;
    const int id = lane < n ? si[lane] : 0;
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float vj = sv[j];
        const int ij = si[j];
        rank += ((vj > v) | ((vj == v) & (ij < id))) ? 1 : 0;
    }
    int32_t *ids = t.ids + r * t.K;
    float *lg = t.logits + r * t.K;
    if (lane < n) { ids[rank] = id; lg[rank] = v; }
    else if (lane < t.K) { ids[lane] = -1; lg[lane] = -INFINITY; }
    if (lane == 0 && t.counts) t.counts[r] = n;
}
