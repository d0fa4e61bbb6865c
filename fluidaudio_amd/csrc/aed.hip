// aed.hip — the kernels of the AED (attention encoder-decoder) greedy decoder for gfx950: the decode step of Cohere Transcribe
// (CoherePipeline.swift:728-803, 924-969: repetition penalty, no-repeat n-gram, first-index argmax, the history and the next
// step's inputs) and of Canary (CanaryManager.swift:212-275), the two attention masks (:817-876), Canary's strided encoder
// transpose and hidden-row gather (CanaryManager.swift:187-209, 251-256) and the longest-common-substring seam merge of the
// long-form path (mergeTokenStreams).  Host side: aed_host.hip; operands and plans: aed_launch.h; shared integers: aed_core.h.
//
// The step is one workgroup per utterance.  The row is read ONCE with 16-byte loads and never written: the ids of the history
// (the only logits the penalty and the ban can change) are marked in a V-bit map in LDS and left out of the streaming maximum;
// one thread per history position — the first occurrence owns the id — computes the id's penalised / banned value, and both
// maxima meet on (value, lowest index).  Built with -ffp-contract=off: the penalty is one IEEE divide or multiply.
#include <cfloat>
#include <climits>

#include <hip/hip_fp16.h>

#include "fa_common.h"
#include "aed_launch.h"

namespace fa {
namespace aed {
void launch_begin(hipStream_t stream, const BeginArgs &a, int32_t batch);
void launch_step(hipStream_t stream, const StepArgs &a, const StepPlan &p);
void launch_finish(hipStream_t stream, const FinishArgs &a);
void launch_cross_mask(hipStream_t stream, const int32_t *valid, int32_t batch, int32_t len, int32_t f16, void *mask);
void launch_context(hipStream_t stream, const StridedArgs &a, const int32_t *len, float *emb, float *mask);
void launch_gather(hipStream_t stream, const StridedArgs &a, const Layout &lay, const int32_t *state, float *hidden);
void launch_merge(hipStream_t stream, const MergeArgs &a);
}  // namespace aed
}  // namespace fa

namespace {

using namespace fa::aed;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 stream_load(const void *p) {   // the row is read once: nontemporal, as the CTC argmax reads its rows
    const u32x4 v = __builtin_nontemporal_load(static_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float widen(const unsigned short h) { return __half2float(__ushort_as_half(h)); }

// (value, lowest index): a greater value wins, an equal one with the lower index; a NaN is never a candidate
struct Best {
    float v;
    int i;
};
template <bool SEQ>
__device__ __forceinline__ void offer(Best &b, const float x, const int idx, const unsigned skip = 0u) {
    const bool ok = (SEQ ? x > -FLT_MAX : x == x) & (skip == 0u);   // Canary: strict '>' from -greatestFiniteMagnitude; Cohere: every number
    const bool t = ok & ((x > b.v) | ((x == b.v) & (idx < b.i)));
    b.v = t ? x : b.v;
    b.i = t ? idx : b.i;
}
__device__ __forceinline__ void meet(Best &b, const float ov, const int oi) {
    const bool t = (ov > b.v) | ((ov == b.v) & (oi < b.i));
    b.v = t ? ov : b.v;
    b.i = t ? oi : b.i;
}
__device__ __forceinline__ void wave_meet(Best &b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) meet(b, __shfl_xor(b.v, off), __shfl_xor(b.i, off));
}

template <bool F16>
__device__ __forceinline__ float load_logit(const void *row, const int id) {
    return F16 ? widen(static_cast<const unsigned short *>(row)[id]) : static_cast<const float *>(row)[id];
}

// The streaming maximum over the ids whose bit is clear (bits == nullptr: over all), in two halves so that the row's loads are in flight
// while the bit map is built: preload() issues the first kPre 16-byte loads of a thread (a whole row of 16 384 fp16 logits, half a row of fp32, over 256 threads),
// finish() takes them and streams what is left.  Only `vocab` elements are read.
constexpr int kPre = 8;
template <bool F16>
struct RowStream {
    static constexpr int kPer = F16 ? 8 : 4;
    const void *row;
    int vocab, nvec, tid;
    uint4 q[kPre];
    __device__ __forceinline__ RowStream(const void *r, const int v, const int t) : row(r), vocab(v), tid(t) {
        nvec = (reinterpret_cast<uintptr_t>(r) & 15u) == 0 ? v / kPer : 0;   // a row off the 16-byte grid is read element by element
    }
    __device__ __forceinline__ void preload() {
        if (nvec <= 0) return;   // uniform over the workgroup: nothing may be read 16 bytes at a time
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const int i = tid + k * kStepThreads;
            q[k] = stream_load(static_cast<const char *>(row) + 16 * static_cast<size_t>(i < nvec ? i : nvec - 1));   // past the end: the last group again, not used
        }
    }
    template <bool SEQ>
    __device__ __forceinline__ void take(Best &b, const uint4 v, const int i, const unsigned *bits) const {
        const int base = i * kPer;
        const unsigned m = bits ? (bits[base >> 5] >> (base & 31)) : 0u;   // kPer divides 32: the group's bits sit in one word
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (F16) {
                offer<SEQ>(b, widen(static_cast<unsigned short>(w[e] & 0xffffu)), base + 2 * e, (m >> (2 * e)) & 1u);
                offer<SEQ>(b, widen(static_cast<unsigned short>(w[e] >> 16)), base + 2 * e + 1, (m >> (2 * e + 1)) & 1u);
            } else {
                offer<SEQ>(b, __uint_as_float(w[e]), base + e, (m >> e) & 1u);
            }
        }
    }
    template <bool SEQ>
    __device__ __forceinline__ Best finish(const unsigned *bits) const {
        Best b{-INFINITY, INT_MAX};
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const int i = tid + k * kStepThreads;
            if (i < nvec) take<SEQ>(b, q[k], i, bits);
        }
#pragma unroll 4
        for (int i = tid + kPre * kStepThreads; i < nvec; i += kStepThreads) take<SEQ>(b, stream_load(static_cast<const char *>(row) + 16 * static_cast<size_t>(i)), i, bits);
        for (int i = nvec * kPer + tid; i < vocab; i += kStepThreads) offer<SEQ>(b, load_logit<F16>(row, i), i, bits ? (bits[i >> 5] >> (i & 31)) & 1u : 0u);
        return b;
    }
};

// Whether the token at history position k is one applyNoRepeatNgram bans: n == 1 every history token; n >= 2 the token that follows an
// earlier occurrence of the last n - 1 tokens (at i = k - (n - 1) < H - (n - 1), so k < H).  h: the history (H tokens) in LDS.
__device__ __forceinline__ bool follows_the_suffix(const int *h, const int H, const int k, const int n) {
    if (n == 1) return true;
    if (n < 1 || H < n - 1 || k < n - 1) return false;
    bool match = true;
    for (int j = 0; j < n - 1 && match; ++j) match = h[k - (n - 1) + j] == h[H - (n - 1) + j];
    return match;
}

// the mask row of `step`: 0 up to and including it, -1e4 beyond (buildSelfAttentionMask's static path)
__device__ __forceinline__ void write_self_mask(void *mask, const int f16, const int64_t b, const int max_seq, const int step, const int tid, const int nthreads) {
    if (!mask) return;
    if (f16) {
        unsigned short *m = static_cast<unsigned short *>(mask) + b * max_seq;
        for (int i = tid; i < max_seq; i += nthreads) m[i] = i <= step ? static_cast<unsigned short>(0) : kMaskedF16;
    } else {
        float *m = static_cast<float *>(mask) + b * max_seq;
        for (int i = tid; i < max_seq; i += nthreads) m[i] = i <= step ? 0.0f : kMasked;
    }
}

template <bool F16, bool SEQ>
__global__ __launch_bounds__(kStepThreads) void aed_step_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float red_v[kStepThreads / kWave];
    __shared__ int red_i[kStepThreads / kWave];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    int32_t *st = a.lay.utt(a.state, b);
    if (st[kReason] != FA_AED_RUNNING) return;   // a finished utterance: its row is not read, nothing of it is touched
    const int max_seq = a.lay.max_seq, V = a.cfg.vocab;
    const int32_t *hist = st + a.lay.hist();
    // one round trip: the header and this thread's first history token (inside the state whatever the history's length)
    const int h0 = (!SEQ && a.marked && tid < max_seq) ? hist[tid] : -1;
    const int step = st[kStep], P = st[kPromptLen], cur = st[kCur], out_count = st[kOutCount];
    int H = st[kHistLen];
    H = H < 0 ? 0 : (H > max_seq ? max_seq : H);
    const bool decides = SEQ || token_decides(step, P);
    __syncthreads();   // every wavefront has read the header before thread 0 rewrites it
    const void *row = static_cast<const char *>(a.logits) + static_cast<size_t>(b) * static_cast<size_t>(a.row_stride) * (F16 ? 2 : 4);

    int next = 0;
    if (decides) {   // uniform over the workgroup
        Best best;
        RowStream<F16> rs(row, V, tid);
        rs.preload();   // the second round trip: the row, and below the logit of this thread's history id
        if (!SEQ && a.marked && H > 0) {
            // LDS: the history, the banned tokens by position (-1: not banned), both padded to a multiple of 4 with -1, then the bit map
            const int S4 = (max_seq + 3) & ~3, H4 = (H + 3) & ~3;
            int *h = reinterpret_cast<int *>(lds_raw), *hb = h + S4;
            unsigned *bits = reinterpret_cast<unsigned *>(hb + S4);
            const int words = (V + 31) / 32;
            const bool mine = tid < H && h0 >= 0 && h0 < V;
            const float v0 = mine ? load_logit<F16>(row, h0) : 0.0f;
            for (int i = tid; i < words; i += kStepThreads) bits[i] = 0u;
            if (tid < H4) h[tid] = tid < H ? h0 : -1;
            for (int j = tid + kStepThreads; j < H4; j += kStepThreads) h[j] = j < H ? hist[j] : -1;
            __syncthreads();
            for (int j = tid; j < H4; j += kStepThreads) {
                const int id = h[j];
                if (j < H && id >= 0 && id < V) atomicOr(&bits[id >> 5], 1u << (id & 31));
                hb[j] = (j < H && follows_the_suffix(h, H, j, a.cfg.no_repeat_ngram)) ? id : -1;
            }
            __syncthreads();
            best = rs.template finish<false>(bits);
            for (int j = tid; j < H; j += kStepThreads) {   // lane = history position; the first occurrence owns the id
                const int id = h[j];
                if (id < 0 || id >= V) continue;
                bool seen = false, banned = false;           // no early exit: the LDS reads of the scan are independent and go out together
                for (int k = 0; k < H4; k += 4) {
                    const int4 t = *reinterpret_cast<const int4 *>(h + k), u = *reinterpret_cast<const int4 *>(hb + k);
                    seen |= ((t.x == id) & (k < j)) | ((t.y == id) & (k + 1 < j)) | ((t.z == id) & (k + 2 < j)) | ((t.w == id) & (k + 3 < j));
                    banned |= (u.x == id) | (u.y == id) | (u.z == id) | (u.w == id);
                }
                if (seen) continue;
                float v = j == tid ? v0 : load_logit<F16>(row, id);
                if (a.cfg.repetition_penalty != 1.0f) v = (v >= 0.0f) ? v / a.cfg.repetition_penalty : v * a.cfg.repetition_penalty;   // H > 0 here
                offer<false>(best, banned ? kBanned : v, id);
            }
        } else {
            best = rs.template finish<SEQ>(nullptr);
        }
        wave_meet(best);
        if ((tid & (kWave - 1)) == 0) { red_v[tid / kWave] = best.v; red_i[tid / kWave] = best.i; }
        __syncthreads();
        Best all{red_v[0], red_i[0]};
#pragma unroll
        for (int w = 1; w < kStepThreads / kWave; ++w) meet(all, red_v[w], red_i[w]);
        next = all.i == INT_MAX ? 0 : all.i;
    }

    if (SEQ) {
        if (tid != 0) return;
        if (next == a.cfg.eos_id) { st[kReason] = FA_AED_END_EOS; return; }
        const int pos = step;   // begin and the previous step keep 1 <= pos < max_seq while the utterance runs
        if (out_count < a.lay.max_out) st[a.lay.out() + out_count] = next;
        st[kOutCount] = out_count + 1;
        if (pos >= 0 && pos < max_seq) {
            a.input_ids[b * max_seq + pos] = next;
            a.decoder_mask[b * max_seq + pos] = 1.0f;
        }
        st[kStep] = pos + 1;
        if (pos + 1 >= max_seq) st[kReason] = FA_AED_END_CAP;
        return;
    }

    // the token feed: the consumed token joins the history AFTER the decision
    const int last = token_last_step(a.cfg.max_new, P, max_seq);
    const bool eos = decides && next == a.cfg.eos_id;
    const bool goes_on = !eos && step < last;
    if (tid == 0) {
        if (H < max_seq) st[a.lay.hist() + H] = cur;
        st[kHistLen] = H + 1;
        if (eos) {
            st[kReason] = FA_AED_END_EOS;
        } else {
            if (decides) {
                if (out_count < a.lay.max_out) st[a.lay.out() + out_count] = next;
                st[kOutCount] = out_count + 1;
            }
            const int fed = step < P - 1 ? st[a.lay.prompt() + step + 1] : next;
            st[kCur] = fed;
            st[kStep] = step + 1;   // the steps that ran
            if (!goes_on) {
                st[kReason] = FA_AED_END_CAP;
            } else {
                a.input_id[b] = fed;
                a.position_id[b] = step + 1;
            }
        }
    }
    if (goes_on) write_self_mask(a.self_mask, a.mask_f16, b, max_seq, step + 1, tid, kStepThreads);
}

__global__ __launch_bounds__(kStepThreads) void aed_begin_kernel(const BeginArgs a) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    int32_t *st = a.lay.utt(a.state, b);
    const int max_seq = a.lay.max_seq;
    const int P = a.prompt_lens[b];   // 1 ... min(prompt_stride, max_seq): the host pass
    const int32_t *prompt = a.prompts + b * a.prompt_stride;
    const bool seq = a.cfg.mode == FA_AED_FEED_SEQUENCE;
    for (int64_t i = kHead + tid; i < a.lay.words(); i += kStepThreads) st[i] = 0;
    __syncthreads();
    for (int i = tid; i < P; i += kStepThreads) st[a.lay.prompt() + i] = prompt[i];
    if (tid == 0) {
        st[kHistLen] = 0;
        st[kStep] = seq ? P : 0;
        st[kCur] = prompt[0];
        st[kOutCount] = 0;
        st[kReason] = (seq && P >= max_seq) ? FA_AED_END_CAP : FA_AED_RUNNING;   // `while pos < s` never runs
        st[kPromptLen] = P;
        st[6] = 0;
        st[7] = 0;
        if (!seq) {
            a.input_id[b] = prompt[0];
            a.position_id[b] = 0;
        }
    }
    if (seq) {
        for (int i = tid; i < max_seq; i += kStepThreads) {
            a.input_ids[b * max_seq + i] = i < P ? prompt[i] : 0;
            a.decoder_mask[b * max_seq + i] = i < P ? 1.0f : 0.0f;
        }
    } else {
        write_self_mask(a.self_mask, a.mask_f16, b, max_seq, 0, tid, kStepThreads);
    }
}

__global__ __launch_bounds__(kWave) void aed_finish_kernel(const FinishArgs a) {
    const int64_t b = blockIdx.x;
    const int32_t *st = a.lay.utt(a.state, b);
    int n = st[kOutCount];
    n = n < 0 ? 0 : (n > a.lay.max_out ? a.lay.max_out : n);
    for (int i = threadIdx.x; i < a.max_out; i += kWave) a.tokens[b * a.max_out + i] = i < n ? st[a.lay.out() + i] : 0;
    if (threadIdx.x == 0) {
        a.counts[b] = n;
        if (a.reasons) a.reasons[b] = st[kReason];
        if (a.steps) a.steps[b] = st[kStep];
    }
}

__global__ __launch_bounds__(kStepThreads) void aed_cross_mask_kernel(const int32_t *valid, const int64_t cells, const int len, const int f16, void *mask) {
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kStepThreads + threadIdx.x;
    if (at >= cells) return;
    const int64_t b = at / len;
    const int i = static_cast<int>(at - b * len);
    int v = valid[b];
    v = v < 0 ? 0 : (v > len ? len : v);   // max(0, min(encoderValid, encoderSeqLen))
    if (f16) static_cast<unsigned short *>(mask)[at] = i < v ? static_cast<unsigned short>(0) : kMaskedF16;
    else static_cast<float *>(mask)[at] = i < v ? 0.0f : kMasked;
}

// [D][T] at strides -> [T][D] dense through a 32 x 32 LDS tile (one padding column: the transposed read is conflict-free)
template <bool F16>
__global__ __launch_bounds__(kTileThreads) void aed_context_kernel(const StridedArgs a, const int32_t *len, float *emb, float *mask) {
    __shared__ float tile[kTile][kTile + 1];
    const int64_t b = blockIdx.z;
    const int D = a.rows, T = a.cols;
    const int t0 = blockIdx.x * kTile, d0 = blockIdx.y * kTile;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;   // 32 x 8
    const char *src = static_cast<const char *>(a.src);
#pragma unroll
    for (int r = ty; r < kTile; r += kTileThreads / kTile) {
        const int d = d0 + r, t = t0 + tx;
        if (d < D && t < T) {
            const int64_t at = b * a.sb + d * a.sr + t * a.sc;
            tile[r][tx] = F16 ? widen(reinterpret_cast<const unsigned short *>(src)[at]) : reinterpret_cast<const float *>(src)[at];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < kTile; r += kTileThreads / kTile) {
        const int t = t0 + r, d = d0 + tx;
        if (t < T && d < D) emb[(b * T + t) * D + d] = tile[tx][r];
    }
    if (blockIdx.y == 0 && threadIdx.x < kTile) {
        const int t = t0 + threadIdx.x;
        if (t < T) {
            int v = len[b];
            v = v < 1 ? 1 : v;
            v = v > T ? T : v;   // min(max(encoderLength, 1), t)
            mask[b * T + t] = t < v ? 1.0f : 0.0f;
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(kStepThreads) void aed_gather_kernel(const StridedArgs a, const Layout lay, const int32_t *state, float *hidden) {
    const int64_t b = blockIdx.x;
    const int32_t *st = lay.utt(state, b);
    if (st[kReason] != FA_AED_RUNNING) return;
    const int pos = st[kStep];
    if (pos < 1 || pos > a.rows) return;   // row pos - 1 of S rows
    const char *src = static_cast<const char *>(a.src);
    const int64_t base = b * a.sb + static_cast<int64_t>(pos - 1) * a.sr;
    for (int d = threadIdx.x; d < a.cols; d += kStepThreads) {
        const int64_t at = base + d * a.sc;
        hidden[b * a.cols + d] = F16 ? widen(reinterpret_cast<const unsigned short *>(src)[at]) : reinterpret_cast<const float *>(src)[at];
    }
}

// mergeTokenStreams folded over a recording's windows by one wavefront, in the recording's output slice.  Lane j holds sHead[j]
// (column j + 1 of the reference's table); the rows are the tokens of pTail, each broadcast to the wavefront; dp[i-1][j-1] comes
// from lane j - 1 by a DPP wave shift; a lane keeps its first strict maximum and the wavefront picks the longest run, then the
// lowest row, then the lowest column — the first cell in row-major order that reaches the maximum, the reference's strict '>'.
constexpr int kWaveShr1 = 0x138;   // DPP wave_shr:1: lane l reads lane l - 1, lane 0 keeps the old value (0)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__global__ __launch_bounds__(kWave) void aed_merge_kernel(const MergeArgs a) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const MergeRec rec = a.recs[r];
    int32_t *out = a.out + rec.out_off;
    int n = 0;   // tokens merged so far: check_merge keeps a recording within INT32_MAX
    for (int64_t w = rec.w_lo; w < rec.w_hi; ++w) {
        const int32_t *s = a.tokens + a.win_off[w];
        const int len = static_cast<int>(a.win_off[w + 1] - a.win_off[w]);
        int best_len = 0, best_send = 0, drop = 0;
        if (n > 0 && len > 0) {
            const int m = n < a.window_tokens ? n : a.window_tokens, cols = len < a.window_tokens ? len : a.window_tokens;
            const int32_t *p_tail = out + (n - m);
            const int sj = lane < cols ? s[lane] : 0;
            int dp = 0, mine = 0, mine_row = 0;
            for (int i = 0; i < m; ++i) {
                const int p = p_tail[i];
                const int prev = __builtin_amdgcn_update_dpp(0, dp, kWaveShr1, 0xf, 0xf, false);
                dp = (lane < cols && p == sj) ? prev + 1 : 0;
                if (dp > mine) { mine = dp; mine_row = i; }
            }
            // the longest run; among its lanes the lowest (row, column)
            int top = mine;
#pragma unroll
            for (int d = kWave / 2; d > 0; d >>= 1) top = max(top, __shfl_xor(top, d));
            int key = (mine == top && top > 0) ? mine_row * kWave + lane : INT_MAX;
#pragma unroll
            for (int d = kWave / 2; d > 0; d >>= 1) key = min(key, __shfl_xor(key, d));
            best_len = top;
            best_send = top > 0 ? (key % kWave) + 1 : 0;
            if (best_len >= a.min_match) drop = best_send;
        }
        for (int i = drop + lane; i < len; i += kWave) out[n + i - drop] = s[i];
        n += len - drop;
        if (lane == 0) {
            if (a.best_len) a.best_len[w] = best_len;
            if (a.best_send) a.best_send[w] = best_send;
        }
        wave_sync();   // the next seam reads the tail other lanes wrote
    }
    if (lane == 0) a.counts[r] = n;
}

template <bool F16>
void launch_step_mode(hipStream_t stream, const StepArgs &a, const StepPlan &p) {
    if (a.cfg.mode == FA_AED_FEED_SEQUENCE) hipLaunchKernelGGL((aed_step_kernel<F16, true>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
    else hipLaunchKernelGGL((aed_step_kernel<F16, false>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
}

}  // namespace

void fa::aed::launch_begin(hipStream_t stream, const BeginArgs &a, const int32_t batch) {
    hipLaunchKernelGGL(aed_begin_kernel, dim3(static_cast<unsigned>(batch)), dim3(kStepThreads), 0, stream, a);
}
void fa::aed::launch_step(hipStream_t stream, const StepArgs &a, const StepPlan &p) {
    if (a.f16) launch_step_mode<true>(stream, a, p);
    else launch_step_mode<false>(stream, a, p);
}
void fa::aed::launch_finish(hipStream_t stream, const FinishArgs &a) {
    hipLaunchKernelGGL(aed_finish_kernel, dim3(static_cast<unsigned>(a.batch)), dim3(kWave), 0, stream, a);
}
void fa::aed::launch_cross_mask(hipStream_t stream, const int32_t *valid, const int32_t batch, const int32_t len, const int32_t f16, void *mask) {
    const int64_t cells = static_cast<int64_t>(batch) * len;
    hipLaunchKernelGGL(aed_cross_mask_kernel, dim3(fa::grid_for(cells, kStepThreads)), dim3(kStepThreads), 0, stream, valid, cells, len, f16, mask);
}
void fa::aed::launch_context(hipStream_t stream, const StridedArgs &a, const int32_t *len, float *emb, float *mask) {
    const TilePlan p = tile_plan(a.batch, a.rows, a.cols);
    if (a.f16) hipLaunchKernelGGL(aed_context_kernel<true>, dim3(p.gx, p.gy, p.gz), dim3(p.block), 0, stream, a, len, emb, mask);
    else hipLaunchKernelGGL(aed_context_kernel<false>, dim3(p.gx, p.gy, p.gz), dim3(p.block), 0, stream, a, len, emb, mask);
}
void fa::aed::launch_gather(hipStream_t stream, const StridedArgs &a, const Layout &lay, const int32_t *state, float *hidden) {
    if (a.f16) hipLaunchKernelGGL(aed_gather_kernel<true>, dim3(static_cast<unsigned>(a.batch)), dim3(kStepThreads), 0, stream, a, lay, state, hidden);
    else hipLaunchKernelGGL(aed_gather_kernel<false>, dim3(static_cast<unsigned>(a.batch)), dim3(kStepThreads), 0, stream, a, lay, state, hidden);
}
void fa::aed::launch_merge(hipStream_t stream, const MergeArgs &a) {
    if (a.n_recs <= 0) return;
    hipLaunchKernelGGL(aed_merge_kernel, dim3(static_cast<unsigned>(a.n_recs)), dim3(kWave), 0, stream, a);
}
