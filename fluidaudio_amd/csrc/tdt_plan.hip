// tdt_plan.hip — the kernels of the TDT window planner (host side: tdt_plan_host.hip; operands, plans and the argument pass:
// tdt_plan_launch.h; the integer arithmetic shared with the host: tdt_plan_core.h; the restated reference lines: include/fluidaudio_hip.h).
//
// ordered_sum    every energy of the reference is `sum += sample * sample` over consecutive samples in fp32: one rounded product and one
//                rounded addition per sample, in order (the unit is built with -ffp-contract=off).  One lane owns one run and adds it in
//                order; the workgroup's runs pass through LDS kStage samples a run at a time, so that consecutive lanes load consecutive
//                addresses (rows of kStage + 1: the lanes' reads fall into different banks).  What lies outside a run or the recording is
//                staged as +0: a non-negative sum is unchanged by adding +0 * +0.
// tp_energy      the boundary table of a recording: entry f is the mean square over [f F - F, f F + F) clipped to the recording, for every
//                frame f whose window holds a sample.  Every boundary score of the chain is centred on a multiple of F (the candidates,
//                targetStart, the forced next boundary), so the table serves the whole chain.  The sum of window f continues the finished sum
//                of frame f - 1, so a lane adds frame f - 1 first — which is also that frame's sum from offset 0, what the gate wants —
//                and then frame f: a sample is staged twice, by two neighbouring lanes, and no partial sum is shared.
// tp_speech_end  speechEndSamples: one wavefront per recording, 64 tail frames per pass counted back from the end, the first frame at or
//                above the floor from a ballot; the common file ends in speech and leaves after one pass.
// tp_chain       silenceAlignedChunkStarts: one wavefront per recording, serial over the targets.  Lane = candidate frame, in two passes
//                over the +-50; the strict minimum with the lowest frame is a wave minimum over (score bits, frame) — scores are not
//                negative, so their bits order as unsigned; the median is the exact rank count / 2 among the keys kept in LDS.  The quiet
//                probe has lane = 20 ms window, and the loop's exits are read off three ballots.
// tp_count /     the window loop: lane = window, each turn of the loop is independent given the start (tdt_plan_core.h: turn), the first
// tp_write       terminating window comes from a ballot.  The windows of the recordings are placed by scan_totals (block_scan.h).
// rows::pack     the preprocessor's rows (row_pack.h); tp_threshold the gate's percentile by exact rank selection over the bits of the kept frames'
//                sums (sqrt and the division are monotone, and the selected element alone is converted); tp_spans the speech-like frames.
// No kernel reads a sample of another recording than its own, and there are no float atomics.
#include "fa_common.h"
#include "block_scan.h"
#include "row_pack.h"
#include "tdt_plan_launch.h"

namespace fa {
namespace tdt_plan {
namespace {

constexpr uint32_t kGreatestFiniteBits = 0x7f7fffffu;   // Float.greatestFiniteMagnitude
constexpr uint64_t kNoKey = ~uint64_t{0};

// Lane `tid` of the first `nf` lanes adds the squares of x[base + tid * stride + p], p = 0 ... len - 1, to `sum`, in order; positions
// outside [0, hi) count as +0.  Every thread of the workgroup calls it with the same arguments but `sum`.
template <int kBlock>
__device__ inline float ordered_sum(float *__restrict__ tile, const float *__restrict__ x, const int64_t hi, const int64_t base, const int64_t stride, const int len,
                                    const int nf, float sum) {
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < len; k0 += kStage) {
#pragma unroll 4
        for (int j = 0; j < kStage; ++j) {
            const int e = j * kBlock + tid, fr = e / kStage, s = e % kStage;
            const int64_t pos = base + fr * stride + k0 + s;
            float v = 0.0f;
            if (fr < nf && k0 + s < len && pos >= 0 && pos < hi) v = x[pos];
            tile[fr * (kStage + 1) + s] = v;
        }
        __syncthreads();
        if (tid < nf) {
#pragma unroll
            for (int s = 0; s < kStage; ++s) {
                const float v = tile[tid * (kStage + 1) + s];
                sum += v * v;
            }
        }
        __syncthreads();
    }
    return sum;
}

// the last recording whose first workgroup is not behind `tile`: recordings without a table have no workgroup
__device__ inline int32_t recording_of_tile(const Recording *__restrict__ rec, const int32_t batch, const int64_t tile) {
    int32_t lo = 0, hi = batch;
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (rec[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kEnergyBlock) void tp_energy(const PlanArgs a) {
    __shared__ float tile[kEnergyBlock * (kStage + 1)];
    const int tid = threadIdx.x;
    const int32_t b = recording_of_tile(a.rec, a.batch, blockIdx.x);
    const Recording r = a.rec[b];
    const int64_t F = a.g.frame, entries = table_entries(F, r.n);
    const int64_t f0 = (static_cast<int64_t>(blockIdx.x) - r.tile0) * kEnergyBlock;
    if (f0 >= entries) return;               // the whole workgroup
    const int nf = static_cast<int>(lesser<int64_t>(kEnergyBlock, entries - f0));
    const float *__restrict__ x = a.audio + r.audio0;
    const int64_t f = f0 + tid;
    float sum = ordered_sum<kEnergyBlock>(tile, x, r.n, (f0 - 1) * F, F, static_cast<int>(F), nf, 0.0f);
    if (tid < nf && a.sums && f >= 1 && f * F <= r.n) a.sums[r.sums0 + f - 1] = sum;     // frame f - 1 is whole
    sum = ordered_sum<kEnergyBlock>(tile, x, r.n, f0 * F, F, static_cast<int>(F), nf, sum);
    if (tid < nf) {
        const int64_t count = lesser(r.n, (f + 1) * F) - greater<int64_t>(0, (f - 1) * F);
        a.table[r.table0 + f] = sum / static_cast<float>(count);
        if (!isfinite(sum)) a.bad[b] = 1;    // every writer writes the same value
    }
}

__global__ __launch_bounds__(kWave) void tp_speech_end(const PlanArgs a) {
    __shared__ float tile[kWave * (kStage + 1)];
    const int b = blockIdx.x, lane = threadIdx.x;
    const Recording r = a.rec[b];
    const int64_t F = a.g.frame;
    int64_t answer = r.n;                    // an all-quiet recording answers totalSamples
    if (a.g.end_aligned && !a.bad[b]) {
        const float *__restrict__ x = a.audio + r.audio0;
        for (int64_t end = r.n; end > 0; end -= kWave * F) {
            const int nf = static_cast<int>(lesser<int64_t>(kWave, (end + F - 1) / F));
            // frame `lane` of the pass is [end - (lane + 1) F, end - lane F), the first block of the recording possibly short
            const float sum = ordered_sum<kWave>(tile, x, r.n, end - F, -F, static_cast<int>(F), nf, 0.0f);
            const int64_t hi = end - lane * F, lo = greater<int64_t>(0, hi - F);
            const bool loud = lane < nf && sqrtf(sum / static_cast<float>(hi - lo)) >= 0.0005f;   // speechRmsFloor
            const uint64_t m = __ballot(loud);
            if (m) {
                answer = end - static_cast<int64_t>(__builtin_ctzll(m)) * F;
                break;
            }
        }
    }
    if (lane == 0) a.speech_end[b] = answer;
}

__device__ inline uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), off);
        v = o < v ? o : v;
    }
    return v;
}

struct Candidate {
    int64_t start;
    float score, median;
};

// bestBoundaryCandidate (:270-310).  keys: 2 * kWave slots of LDS.
__device__ inline Candidate best_boundary(uint64_t *__restrict__ keys, const float *__restrict__ table, const int64_t n, const int64_t F, const int64_t target_frame,
                                          const int32_t radius, const int64_t previous_start, const int64_t latest, const int64_t target_start) {
    const int lane = threadIdx.x;
    const int64_t lower = greater<int64_t>(1, target_frame - radius), upper = lesser((n - 1) / F, target_frame + radius);
    uint64_t mine[2], least = kNoKey;
    int count = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int64_t frame = lower + p * kWave + lane, candidate = frame * F;
        const bool valid = frame <= upper && candidate > previous_start && candidate <= latest;
        mine[p] = valid ? (static_cast<uint64_t>(__float_as_uint(table[frame])) << 32) | static_cast<uint64_t>(frame - lower) : kNoKey;
        keys[p * kWave + lane] = mine[p];
        least = mine[p] < least ? mine[p] : least;
        count += __popcll(__ballot(valid));
    }
    __syncthreads();
    Candidate c{target_start, __uint_as_float(kGreatestFiniteBits), 0.0f};
    if (count > 0) {                         // wave-uniform
        least = wave_min_u64(least);
        const uint32_t bits = static_cast<uint32_t>(least >> 32);
        c.score = __uint_as_float(bits < kGreatestFiniteBits ? bits : kGreatestFiniteBits);
        if (bits < kGreatestFiniteBits) c.start = (lower + static_cast<int64_t>(least & 0xffffffffu)) * F;   // `score < bestScore` is strict
        // sorted()[count / 2]: the key with exactly count / 2 keys below it
        uint32_t median_bits = 0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int below = 0;
            for (int k = 0; k < 2 * kWave; ++k) below += keys[k] < mine[p] ? 1 : 0;
            const uint64_t hit = __ballot(mine[p] != kNoKey && below == count / 2);
            if (hit) median_bits = static_cast<uint32_t>(__shfl(static_cast<unsigned long long>(mine[p]), __builtin_ctzll(hit)) >> 32);
        }
        c.median = __uint_as_float(median_bits);
    }
    __syncthreads();                         // the keys are free again
    return c;
}

__device__ inline float threshold_of(const float median, const float ratio) { return median > 0.0f ? median * ratio : 0.0f; }   // :320-323

__global__ __launch_bounds__(kWave) void tp_chain(const PlanArgs a) {
    __shared__ float tile[kWave * (kStage + 1)];
    __shared__ uint64_t keys[2 * kWave];
    const int b = blockIdx.x, lane = threadIdx.x;
    const Recording r = a.rec[b];
    if (r.n == 0 || a.bad[b]) return;
    const Geometry g = a.g;
    const int64_t F = g.frame, n = r.n, entries = table_entries(F, n), minimum_overlap = F * kMinOverlapFrames;
    const float *__restrict__ x = a.audio + r.audio0;
    const float *__restrict__ table = a.table + r.table0;
    int64_t *__restrict__ starts = a.starts + r.starts0;
    const auto score_at = [&](const int64_t center) {                // boundaryEnergyScore at a multiple of F; 0 where the window is empty
        const int64_t f = center / F;
        return f < entries ? table[f] : 0.0f;
    };
    const int windows = static_cast<int>((g.lookahead + g.probe_window - 1) / g.probe_window);
    // shouldUseWarmupPrefix (:350-382)
    const auto should_use_warmup = [&](const int64_t center) {
        const int64_t hi = lesser(n, center + g.lookahead);
        const float sum = ordered_sum<kWave>(tile, x, hi, center, g.probe_window, static_cast<int>(g.probe_window), windows, 0.0f);
        const int64_t start = center + lane * g.probe_window;
        const int64_t count = lesser(lesser(g.probe_window, n - start), g.lookahead - lane * g.probe_window);
        const bool in = lane < windows;
        const bool past = in && (start >= n || count <= 0);                                      // :361, :364
        const bool loud = in && !past && !(sqrtf(sum / static_cast<float>(count)) < 0.003f);     // :372
        const int64_t quiet = lesser(start + g.probe_window, hi) - center;                       // quietSamples with this window, all before it quiet
        const bool stable = in && quiet >= g.stable_quiet;                                       // :375
        const uint64_t m_break = __ballot(past || loud), m_stable = __ballot(stable);
        const uint64_t any = m_break | m_stable;
        if (!any) return true;                                                                   // the look-ahead ran out
        return ((m_break >> __builtin_ctzll(any)) & 1) != 0;                                     // a window's break comes before its quiet count
    };

    if (lane == 0) starts[0] = 0;
    int64_t previous_start = 0, k = 1;
    for (int64_t target = g.stride; target < n; target += g.stride, ++k) {
        const int64_t target_frame = target / F, latest = previous_start + g.chunk - minimum_overlap;
        const int64_t target_start = lesser(greater(target_frame * F, previous_start + F), latest);
        const Candidate silence = best_boundary(keys, table, n, F, target_frame, g.silence_radius, previous_start, latest, target_start);
        int64_t best_start;
        bool use_warmup = false;
        if (silence.score <= threshold_of(silence.median, 0.05f)) {                              // isNearSilenceBoundary
            const bool should_warmup = g.can_warmup ? should_use_warmup(silence.start) : false;
            bool compresses = false;
            if (should_warmup && silence.start < target_start && silence.median > 0.0f) {        // wouldCompressSpeechTail (:325-348)
                const int64_t forced = silence.start + g.chunk - minimum_overlap;
                if (forced < n) {
                    const float speech_like = silence.median * 0.8f;
                    compresses = score_at(target_start) > speech_like && score_at(forced) > speech_like;
                }
            }
            if (compresses) {
                best_start = target_start;
            } else {
                best_start = silence.start;
                use_warmup = should_warmup;
            }
        } else {
            const Candidate valley = best_boundary(keys, table, n, F, target_frame, g.valley_radius, previous_start, latest, target_start);
            best_start = valley.score <= threshold_of(valley.median, 0.35f) ? valley.start : target_start;   // isUsableValleyBoundary
        }
        if (best_start <= previous_start) best_start = lesser(previous_start + g.stride, n);    // :253-255
        if (lane == 0) starts[k] = (best_start << 1) | (use_warmup ? 1 : 0);
        previous_start = best_start;
    }
}

// The window loop of recording b: f(index, turn) for every window that leaves a record; the number of them is returned.
template <class Emit>
__device__ inline int32_t walk(const PlanArgs &a, const int b, const Emit &emit) {
    const int lane = threadIdx.x;
    const Recording r = a.rec[b];
    if (r.n == 0 || a.bad[b]) return 0;
    const Geometry g = a.g;
    const int64_t speech_end = a.speech_end[b];
    const int64_t *__restrict__ starts = a.starts + r.starts0;
    const int64_t last_listed = g.aligned ? starts[r.listed - 1] >> 1 : (r.listed - 1) * g.stride;
    for (int64_t i0 = 0;; i0 += kWave) {
        const int64_t i = i0 + lane;
        int64_t start;
        bool use_warmup = false;
        if (i < r.listed) {
            start = g.aligned ? starts[i] >> 1 : i * g.stride;
            use_warmup = g.aligned && (starts[i] & 1);
        } else {
            start = last_listed + (i - (r.listed - 1)) * g.stride;                               // :634-635
        }
        const Turn t = turn(g, b, r.n, speech_end, start, use_warmup, i);
        const uint64_t ends = __ballot(t.ends);
        const int first = ends ? __builtin_ctzll(ends) : kWave;
        if (lane <= first && t.record) emit(i, t);
        if (ends) return static_cast<int32_t>(i0 + first + ((__ballot(t.record) >> first) & 1));
    }
}

__global__ __launch_bounds__(kWave) void tp_count(const PlanArgs a) {
    const int b = blockIdx.x;
    const int32_t n = walk(a, b, [](const int64_t, const Turn &) {});
    if (threadIdx.x == 0) { a.counts[b] = n; a.counts_kept[b] = n; }
}

__global__ __launch_bounds__(kWave) void tp_write(const PlanArgs a) {
    const int b = blockIdx.x;
    if (*a.total > a.capacity) return;       // nothing is planned into an output that is too small
    const int64_t at = a.counts[b];          // the windows of the recordings before this one
    (void)walk(a, b, [&](const int64_t i, const Turn &t) {
        const int64_t slot = at + i;
        a.out[slot] = t.w;
        if (a.audio_frames) a.audio_frames[slot] = t.w.actual_audio_frames;
        if (a.t0) a.t0[slot] = t.w.context_frames;                   // calculateInitialTimeIndices without a time jump; 0 behind a suppressed prefix
        if (a.is_last) a.is_last[slot] = t.w.is_last;
        if (a.global_offset) a.global_offset[slot] = t.w.global_frame_offset;
        if (a.emit_after) a.emit_after[slot] = t.w.emit_after_frame;
    });
}

// adaptiveSpeechRmsThreshold (:1252-1276).  sqrt(sum / F) ascends with sum, and equal sums give equal values, so the element of rank k
// among the RMS values is the RMS of the sum of rank k: the selection runs over the bits of the kept sums (positive floats order as
// unsigned), four passes of one byte each, most significant first, and the chosen sum alone goes through the division and the root.
__global__ __launch_bounds__(256) void tp_threshold(const GateArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t pick[2];
    __shared__ uint32_t kept_total;
    const int tid = threadIdx.x, b = blockIdx.x;
    const Recording r = a.plan.rec[b];
    const int64_t frames = r.n / a.plan.g.frame;
    const uint32_t *__restrict__ sums = reinterpret_cast<const uint32_t *>(a.plan.sums) + r.sums0;
    if (a.plan.bad[b]) {
        if (tid == 0) a.thresholds[b] = __builtin_nanf("");
        return;
    }
    if (tid == 0) kept_total = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int64_t i = tid; i < frames; i += 256) mine += __uint_as_float(sums[i]) > 0.0f ? 1 : 0;   // `if sum > 0`
    atomicAdd(&kept_total, mine);
    __syncthreads();
    const uint32_t kept = kept_total;
    float answer = 0.008f;                   // speechRmsCeiling when no frame is left
    if (kept > 0) {
        const uint32_t at = static_cast<uint32_t>(static_cast<double>(kept) * 0.75);             // Int(Double(count) * 0.75)
        uint32_t k = at < kept - 1 ? at : kept - 1, prefix = 0, mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < frames; i += 256) {
                const uint32_t u = sums[i];
                if (__uint_as_float(u) > 0.0f && (u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 0xffu], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t byte = 0, below = 0;
                while (below + hist[byte] <= k) below += hist[byte++];
                pick[0] = byte; pick[1] = k - below;
            }
            __syncthreads();
            prefix |= pick[0] << shift; mask |= 0xffu << shift; k = pick[1];
            __syncthreads();
        }
        const float reference = sqrtf(__uint_as_float(prefix) / static_cast<float>(a.plan.g.frame));
        const float scaled = reference * 0.3f, floored = scaled >= 0.0005f ? scaled : 0.0005f;   // max(floor, x)
        answer = floored < 0.008f ? floored : 0.008f;                                            // min(ceiling, x)
    }
    if (tid == 0) a.thresholds[b] = answer;
}

// speechLikeSeconds' count (:1518-1532): one wavefront per span, 64 frames a pass.
__global__ __launch_bounds__(kWave) void tp_spans(const GateArgs a) {
    __shared__ float tile[kWave * (kStage + 1)];
    const int lane = threadIdx.x;
    const Span s = a.spans[blockIdx.x];
    const int64_t F = a.plan.g.frame;
    int64_t count = 0;
    if (!a.plan.bad[s.recording]) {
        const float threshold = a.override_thresholds ? a.override_thresholds[s.recording] : a.thresholds[s.recording];
        const float *__restrict__ x = a.plan.audio + s.audio0;
        for (int64_t f0 = 0; f0 < s.frames; f0 += kWave) {
            const int nf = static_cast<int>(lesser<int64_t>(kWave, s.frames - f0));
            const float sum = ordered_sum<kWave>(tile, x, s.frames * F, f0 * F, F, static_cast<int>(F), nf, 0.0f);
            count += __popcll(__ballot(lane < nf && sqrtf(sum / static_cast<float>(F)) > threshold));
        }
    }
    if (lane == 0) a.span_frames[blockIdx.x] = count;
}

}  // namespace

void launch_plan(hipStream_t stream, const PlanArgs &a) {
    if (a.tiles > 0) tp_energy<<<a.tiles, kEnergyBlock, 0, stream>>>(a);
    tp_speech_end<<<a.batch, kWave, 0, stream>>>(a);
    if (a.g.aligned) tp_chain<<<a.batch, kWave, 0, stream>>>(a);
    tp_count<<<a.batch, kWave, 0, stream>>>(a);
    scan::scan_totals<<<1, scan::kThreads, 0, stream>>>(a.counts, static_cast<int64_t>(a.batch), a.total);
    tp_write<<<a.batch, kWave, 0, stream>>>(a);
}

void launch_pack(hipStream_t stream, const float *audio, const rows::Group &g, const int64_t row_samples, float *out, int32_t *lengths, const bool wide) {
    rows::launch_pack<false>(stream, audio, g, row_samples, out, lengths, wide);
}

void launch_gate(hipStream_t stream, const GateArgs &a) {
    if (a.plan.tiles > 0) tp_energy<<<a.plan.tiles, kEnergyBlock, 0, stream>>>(a.plan);
    tp_threshold<<<a.plan.batch, 256, 0, stream>>>(a);
    if (a.n_spans > 0) tp_spans<<<a.n_spans, kWave, 0, stream>>>(a);
}

}  // namespace tdt_plan
}  // namespace fa
