// sortformer_stream.hip — the kernels of the streaming Sortformer state (SortformerStateUpdater.swift:43-164, 175-212, 220-578), batched over
// streams; the host side is sortformer_stream_host.hip, the operands sortformer_stream_launch.h, the integers sortformer_stream_core.h.
// One update is four launches whatever the streams do; a stream that is refused, inactive, does not pop or does not compress leaves
// the later kernels at their first instruction.
//   sfs_control  one workgroup per stream.  Validates before the first write, hands out the confirmed / tentative rows, replaces the
//                FIFO's preds, marks the silent popped frames, and for a compressing stream runs everything up to the selection in LDS:
//                base scores, disableLowScores, the latest-frames boost, the strong and the weak boost — each "the first min(k, frames) in
//                the order (score descending, frame ascending)", found by an exact rank count per speaker column —, the +inf placeholder
//                rows and the global selection, again an exact rank count over 64-bit keys (score descending, permuted index ascending);
//                the selected indices come out ascending through a prefix sum over the selection's flags in index order.
//   sfs_move     a lane owns four columns of one stream for the whole call: the append, the silence profile over the popped rows in frame
//                order, the popped rows' way into the cache (or, compressing, into scratch), and the FIFO's shift in place — row j takes row
//                j + pop, ascending, so within a column every read lies ahead of every write.
//   sfs_gather   (stream, row tile): the compressed cache into scratch — its source rows are neither monotone nor distinct, so nothing
//                reads the slab that is being written;  sfs_replace: scratch into the model-facing slab.
// The unit is built with -ffp-contract=off: (mean * n + x) / newN and every add of the scores stay unfused, as in the reference.
// Every store is a plain C++ assignment.  The chunk rows the model reads are row_pack.h's copy, instantiated here (launch_pack).
#include <hip/hip_fp16.h>

#include "row_pack.h"
#include "sortformer_stream_launch.h"

namespace fa {
namespace sfs {
namespace {

constexpr uint32_t kNegInfBits = 0xFF800000u, kPosInfBits = 0x7F800000u;

__device__ inline float bits_float(const uint32_t u) { return __uint_as_float(u); }

// ascending integer key of "score descending": the smaller key comes first.  -0 and +0 compare equal as floats, so both map to +0.
__device__ inline uint32_t desc_key(const float v) {
    uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

__global__ __launch_bounds__(kControlBlock) void sfs_control(const UpdateArgs a) {
    extern __shared__ __align__(8) unsigned char lds_raw[];
    __shared__ Plan s_plan;
    __shared__ int s_pos[kMaxSpeakers];
    __shared__ int s_sil;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int S = a.c.speakers, cap = a.c.spkcache_len;
    uint64_t *keys = reinterpret_cast<uint64_t *>(lds_raw);                    // [slabs.keys]; its first bytes double as the boosts' second score array
    float *P = reinterpret_cast<float *>(keys + a.slabs.keys);                 // [score_rows][S] the preds of the scored rows
    float *sc = P + a.slabs.score_rows * S;                                    // [score_rows][S] their scores
    float *C = sc + a.slabs.score_rows * S;                                    // [fifo_pred_rows][S] the FIFO's preds with the core rows appended
    int32_t *flag = reinterpret_cast<int32_t *>(C + a.slabs.fifo_pred_rows * S);   // [slabs.keys]
    int32_t *part = flag + a.slabs.keys;                                       // [kControlBlock]
    float *tmp = reinterpret_cast<float *>(keys);

    const float *preds = a.preds + static_cast<int64_t>(b) * a.pred_stride * S;
    int32_t *meta = a.st.meta + static_cast<int64_t>(b) * kMetaInts;
    if (tid == 0) {
        Plan p{};
        if (a.active && a.active[b] == 0) { p.status = kInactive; p.mode = kSkip; }
        else p = plan_update(a.c, a.st.spk_len[b], a.st.fifo_len[b], meta[kMetaSpkPreds], a.emb_len[b], a.pred_rows[b], a.pred_stride, a.left[b], a.right[b]);
        p.sil_before = meta[kMetaSilCount];
        s_plan = p;
        s_sil = 0;
        for (int s = 0; s < kMaxSpeakers; ++s) s_pos[s] = 0;
    }
    __syncthreads();
    Plan p = s_plan;
    const int chunk_end = p.chunk_start + p.core;
    // a pred that is NaN or outside [0, 1] among the rows this update reads: the FIFO's, the core's and the tentative ones, and the cache's at its first overflow
    int bad = 0;
    if (p.status == kOk) {
        const bool prefix = p.mode == kCompress && p.first_overflow;
        for (int e = tid; e < (chunk_end + p.rc) * S; e += kControlBlock) {
            const int r = e / S;
            const bool read = (p.old_fifo > 0 && r >= p.old_spk && r < p.old_spk + p.old_fifo) || r >= p.chunk_start || (prefix && r < p.old_spk);
            if (!read) continue;
            const float v = preds[e];
            if (!(v >= 0.0f && v <= 1.0f)) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);
    if (bad) { p.status = kBadPred; p.mode = kSkip; }
    if (tid == 0) {
        a.status[b] = p.status;
        a.st.plan[b] = p;
        a.counts[2 * b] = p.mode == kSkip ? 0 : p.core;
        a.counts[2 * b + 1] = p.mode == kSkip ? 0 : p.rc;
    }
    if (p.mode == kSkip) return;   // nothing of the stream has been written

    // :93-94 the rows handed out
    float *confirmed = a.confirmed + static_cast<int64_t>(b) * a.c.max_chunk_frames * S, *tentative = a.tentative + static_cast<int64_t>(b) * a.c.max_chunk_frames * S;
    for (int e = tid; e < p.core * S; e += kControlBlock) confirmed[e] = preds[p.chunk_start * S + e];
    for (int e = tid; e < p.rc * S; e += kControlBlock) tentative[e] = preds[chunk_end * S + e];
    // :47-55, :100-104 the FIFO's preds: this call's rows of the FIFO, then the core's
    const int context = p.old_fifo + p.core;
    for (int e = tid; e < p.old_fifo * S; e += kControlBlock) C[e] = preds[p.old_spk * S + e];
    for (int e = tid; e < p.core * S; e += kControlBlock) C[p.old_fifo * S + e] = preds[p.chunk_start * S + e];
    __syncthreads();
    float *fifo_preds = a.st.fifo_preds + static_cast<int64_t>(b) * a.slabs.fifo_pred_rows * S;
    for (int e = tid; e < p.new_fifo * S; e += kControlBlock) fifo_preds[e] = C[p.pop * S + e];
    if (tid == 0) {
        a.st.fifo_len[b] = p.new_fifo;
        a.st.spk_len[b] = p.new_spk;
        meta[kMetaFifoPreds] = 1;
    }
    (void)context;
    if (p.mode == kAppend) return;

    // :185-195 which popped frames enter the silence profile
    uint8_t *silent = a.st.silent + static_cast<int64_t>(b) * a.slabs.max_pop;
    for (int r = tid; r < p.pop; r += kControlBlock) {
        float sum = 0.0f;
        for (int s = 0; s < S; ++s) sum += C[r * S + s];
        const bool sil = sum < a.c.silence_threshold;
        silent[r] = sil ? 1 : 0;
        if (sil) atomicAdd(&s_sil, 1);
    }
    float *spk_preds = a.st.spk_preds + static_cast<int64_t>(b) * a.slabs.score_rows * S;
    const bool present = meta[kMetaSpkPreds] != 0;   // read by every thread before thread 0 sets it behind the barriers below
    if (p.mode == kPop) {
        if (present)   // :145-147
            for (int e = tid; e < p.pop * S; e += kControlBlock) spk_preds[p.old_spk * S + e] = C[e];
        __syncthreads();
        if (tid == 0) meta[kMetaSilCount] = p.sil_before + s_sil;
        return;
    }

    // ---- compressSpkcache (:220-305) on N rows: the cache's preds (at the first overflow this call's, :150-158), then the popped ones
    const int N = p.old_spk + p.pop;
    for (int e = tid; e < p.old_spk * S; e += kControlBlock) P[e] = p.first_overflow ? preds[e] : spk_preds[e];
    for (int e = tid; e < p.pop * S; e += kControlBlock) P[p.old_spk * S + e] = C[e];
    __syncthreads();
    if (tid == 0) { meta[kMetaSilCount] = p.sil_before + s_sil; meta[kMetaSpkPreds] = 1; }

    // getLogPredScores (:311-348)
    const float thr = a.c.pred_score_threshold, hi = 1.0f - thr, ln2 = bits_float(kLn2Bits);
    float *log_scores = a.log_scores ? a.log_scores + static_cast<int64_t>(b) * a.slabs.score_rows * S : nullptr;
    for (int e = tid; e < N * S; e += kControlBlock) {
        const int f = e / S;
        float sum = 0.0f, own = 0.0f;
        for (int s = 0; s < S; ++s) {
            const float l = log1pf(-fminf(fmaxf(P[f * S + s], 0.0f), hi));
            sum += l;
            if (f * S + s == e) own = l;
        }
        float v = logf(fminf(fmaxf(P[e], thr), 3.402823466e+38f));
        v = v - own;
        v = ln2 + v;
        v = v + sum;
        sc[e] = v;
        if (log_scores) log_scores[e] = v;
    }
    __syncthreads();
    // disableLowScores (:351-390), then the latest rows' boost (:246-252)
    for (int e = tid; e < N * S; e += kControlBlock)
        if (P[e] > 0.5f && sc[e] > 0.0f) atomicAdd(&s_pos[e % S], 1);
    __syncthreads();
    for (int e = tid; e < N * S; e += kControlBlock) {
        float v = sc[e];
        if (P[e] <= 0.5f) v = bits_float(kNegInfBits);
        else if (v <= 0.0f && s_pos[e % S] >= a.q.min_pos) v = bits_float(kNegInfBits);
        if (e / S >= cap) v = v + a.c.scores_boost_latest;
        sc[e] = v;
    }
    __syncthreads();
    // boostTopKScores (:393-457), strong then weak: the first min(k, N) of a speaker's finite scores in the order (score descending, frame ascending)
    for (int pass = 0; pass < 2; ++pass) {
        const int k = pass == 0 ? a.q.strong : a.q.weak;
        if (k <= 0) continue;
        const int k_eff = imin(k, N);
        const float delta = (pass == 0 ? 2.0f : 1.0f) * ln2;
        for (int e = tid; e < N * S; e += kControlBlock) {
            const float v = sc[e];
            float out = v;
            if (v != bits_float(kNegInfBits)) {
                const int f = e / S, s = e % S;
                int rank = 0;   // no early exit: the reads of a straight loop are issued eight at a time instead of one per LDS round trip
#pragma unroll 8
                for (int g = 0; g < N; ++g) {
                    const float w = sc[g * S + s];
                    rank += (w > v || (w == v && g < f)) ? 1 : 0;
                }
                if (rank < k_eff) out = v + delta;
            }
            tmp[e] = out;
        }
        __syncthreads();
        for (int e = tid; e < N * S; e += kControlBlock) sc[e] = tmp[e];
        __syncthreads();
    }
    // getTopKIndices (:465-578): the sil +inf rows per speaker, keys in permuted order
    const int frames = N + a.c.sil_frames_per_spk, M = frames * S, k_eff = imin(cap, M);
    for (int i = tid; i < M; i += kControlBlock) {
        const int s = i / frames, f = i % frames;
        const float v = f < N ? sc[f * S + s] : bits_float(kPosInfBits);
        keys[i] = (static_cast<uint64_t>(desc_key(v)) << 32) | static_cast<uint32_t>(i);
    }
    __syncthreads();
    const uint32_t neg_inf_key = desc_key(bits_float(kNegInfBits));
    // four keys of a lane are ranked against every key it reads: a quarter of the LDS reads; a selected -inf becomes the sentinel
    // max_index, which sorts behind every live index
    constexpr int kBatch = 4;
    for (int base = 0; base < M; base += kBatch * kControlBlock) {
        uint64_t own[kBatch];
        int rank[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kControlBlock + tid;
            own[u] = keys[i < M ? i : 0];
            rank[u] = 0;
        }
#pragma unroll 4
        for (int j = 0; j < M; ++j) {
            const uint64_t k = keys[j];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) rank[u] += k < own[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kControlBlock + tid;
            if (i < M) flag[i] = (rank[u] < k_eff && static_cast<uint32_t>(own[u] >> 32) != neg_inf_key) ? 1 : 0;
        }
    }
    __syncthreads();
    // ascending sort of the live indices = their prefix count in index order
    const int seg = (M + kControlBlock - 1) / kControlBlock, lo = imin(tid * seg, M), up = imin(lo + seg, M);
    int mine = 0;
    for (int i = lo; i < up; ++i) mine += flag[i];
    part[tid] = mine;
    __syncthreads();
    int pos = 0, live_count = 0;   // every lane adds up the partial counts before its own: no second barrier, no single lane's loop
#pragma unroll 8
    for (int t = 0; t < kControlBlock; ++t) {
        const int n = part[t];
        pos += t < tid ? n : 0;
        live_count += n;
    }
    int32_t *sel = a.st.sel + static_cast<int64_t>(b) * cap;
    for (int i = lo; i < up; ++i) {
        if (!flag[i]) continue;
        const int f = i % frames;
        const bool live = f < N;   // :566-570 a placeholder row is disabled
        sel[pos] = live ? f : -1;
        for (int s = 0; s < S; ++s) spk_preds[pos * S + s] = live ? P[f * S + s] : 0.0f;
        ++pos;
    }
    for (int i = live_count + tid; i < cap; i += kControlBlock) {   // the sentinels, and the slots past k_eff
        sel[i] = -1;
        for (int s = 0; s < S; ++s) spk_preds[i * S + s] = 0.0f;
    }
}

template <bool kHalf>
__device__ inline float4 load_row4(const void *base, const int64_t element) {
    if (kHalf) {
        const uint2 raw = *reinterpret_cast<const uint2 *>(static_cast<const __half *>(base) + element);
        const __half2 lo = *reinterpret_cast<const __half2 *>(&raw.x), hi2 = *reinterpret_cast<const __half2 *>(&raw.y);
        const float2 a = __half22float2(lo), c = __half22float2(hi2);
        return make_float4(a.x, a.y, c.x, c.y);
    }
    return *reinterpret_cast<const float4 *>(static_cast<const float *>(base) + element);
}

template <bool kHalf>
__global__ __launch_bounds__(kMoveBlock) void sfs_move(const UpdateArgs a) {
    const int b = blockIdx.y, g = blockIdx.x * kMoveBlock + threadIdx.x, D = a.c.d_model, D4 = D / 4;
    if (g >= D4) return;
    const Plan p = a.st.plan[b];
    if (p.mode == kSkip) return;
    float4 *fifo = reinterpret_cast<float4 *>(a.st.fifo + static_cast<int64_t>(b) * a.c.fifo_len * D) + g;
    const int64_t chunk0 = (static_cast<int64_t>(b) * a.c.max_chunk_frames + p.lc) * D + 4 * g;
    const auto core_row = [&](const int i) { return load_row4<kHalf>(a.chunk_embs, chunk0 + static_cast<int64_t>(i) * D); };
    if (p.mode == kAppend) {   // :97-98
        for (int i = 0; i < p.core; ++i) fifo[static_cast<int64_t>(p.old_fifo + i) * D4] = core_row(i);
        return;
    }
    // row r of the FIFO with the core rows appended
    const auto row = [&](const int r) { return r < p.old_fifo ? fifo[static_cast<int64_t>(r) * D4] : core_row(r - p.old_fifo); };
    const bool compress = p.mode == kCompress;
    float4 *mean_at = reinterpret_cast<float4 *>(a.st.mean + static_cast<int64_t>(b) * D) + g;
    float4 *popped = compress ? reinterpret_cast<float4 *>(a.st.popped + static_cast<int64_t>(b) * a.slabs.max_pop * D) + g
                              : reinterpret_cast<float4 *>(a.st.spkcache + (static_cast<int64_t>(b) * a.c.spkcache_len + p.old_spk) * D) + g;
    const uint8_t *silent = a.st.silent + static_cast<int64_t>(b) * a.slabs.max_pop;
    float4 mean = *mean_at;
    int count = p.sil_before;
    for (int r = 0; r < p.pop; ++r) {   // :128-142: the silence profile in frame order, the popped rows to the cache
        const float4 v = row(r);
        if (silent[r]) {
            const float n = static_cast<float>(count), new_n = n + 1.0f;
            mean.x = (mean.x * n + v.x) / new_n;
            mean.y = (mean.y * n + v.y) / new_n;
            mean.z = (mean.z * n + v.z) / new_n;
            mean.w = (mean.w * n + v.w) / new_n;
            ++count;
        }
        popped[static_cast<int64_t>(r) * D4] = v;
    }
    *mean_at = mean;
    // removeFirst in place: ascending, a column private to this lane
    for (int j = 0; j < p.new_fifo; ++j) fifo[static_cast<int64_t>(j) * D4] = row(j + p.pop);
    for (int j = p.new_fifo; j < p.old_fifo; ++j) fifo[static_cast<int64_t>(j) * D4] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(128) void sfs_gather(const UpdateArgs a) {
    const int b = blockIdx.y, D4 = a.c.d_model / 4, cap = a.c.spkcache_len;
    const Plan p = a.st.plan[b];
    if (p.mode != kCompress) return;
    const float4 *slab = reinterpret_cast<const float4 *>(a.st.spkcache + static_cast<int64_t>(b) * cap * a.c.d_model);
    const float4 *popped = reinterpret_cast<const float4 *>(a.st.popped + static_cast<int64_t>(b) * a.slabs.max_pop * a.c.d_model);
    const float4 *mean = reinterpret_cast<const float4 *>(a.st.mean + static_cast<int64_t>(b) * a.c.d_model);
    float4 *out = reinterpret_cast<float4 *>(a.st.gathered + static_cast<int64_t>(b) * cap * a.c.d_model);
    const int r1 = imin(cap, (blockIdx.x + 1) * kGatherRows);
    for (int i = blockIdx.x * kGatherRows; i < r1; ++i) {
        const int src = a.st.sel[static_cast<int64_t>(b) * cap + i];
        // :277-299: a disabled slot takes the mean silence embedding, a live one its row
        const float4 *from = src < 0 ? mean : (src < p.old_spk ? slab + static_cast<int64_t>(src) * D4 : popped + static_cast<int64_t>(src - p.old_spk) * D4);
        for (int g = threadIdx.x; g < D4; g += 128) out[static_cast<int64_t>(i) * D4 + g] = from[g];
    }
}

__global__ __launch_bounds__(128) void sfs_replace(const UpdateArgs a) {
    const int b = blockIdx.y, D4 = a.c.d_model / 4, cap = a.c.spkcache_len;
    if (a.st.plan[b].mode != kCompress) return;
    const float4 *from = reinterpret_cast<const float4 *>(a.st.gathered + static_cast<int64_t>(b) * cap * a.c.d_model);
    float4 *slab = reinterpret_cast<float4 *>(a.st.spkcache + static_cast<int64_t>(b) * cap * a.c.d_model);
    const int64_t e1 = static_cast<int64_t>(imin(cap, (blockIdx.x + 1) * kGatherRows)) * D4;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kGatherRows * D4 + threadIdx.x; e < e1; e += 128) slab[e] = from[e];
}

}  // namespace

void launch_update(hipStream_t stream, const UpdateArgs &a) {
    const LaunchPlan lp = launch_plan_of(a.c, a.slabs);
    const unsigned B = static_cast<unsigned>(a.st.B);
    hipLaunchKernelGGL(sfs_control, dim3(B), dim3(kControlBlock), lp.lds_bytes, stream, a);
    if (a.embs_f16) hipLaunchKernelGGL(sfs_move<true>, dim3(lp.move_grid_x, B), dim3(kMoveBlock), 0, stream, a);
    else hipLaunchKernelGGL(sfs_move<false>, dim3(lp.move_grid_x, B), dim3(kMoveBlock), 0, stream, a);
    hipLaunchKernelGGL(sfs_gather, dim3(lp.gather_grid_x, B), dim3(128), 0, stream, a);
    hipLaunchKernelGGL(sfs_replace, dim3(lp.gather_grid_x, B), dim3(128), 0, stream, a);
}

void launch_pack(hipStream_t stream, const float *mel, const rows::Group &g, const int64_t row_samples, float *out, const bool wide) {
    rows::launch_pack<false>(stream, mel, g, row_samples, out, nullptr, wide);
}

}  // namespace sfs
}  // namespace fa
