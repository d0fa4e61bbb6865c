// vad.hip — the kernels of the VAD stages (host side: vad_host.hip; operands, plans and the restated reference lines: vad_launch.h).
//
// vad_machine   detectSpeechSampleRanges' state machine (VadManager+SpeechSegmentation.swift:102-201), one wavefront per recording,
//               lane = frame, 64 frames a step.  The two classes of a step (p >= threshold, p < negativeThreshold) are 64-bit ballots;
//               the machine itself is wave-uniform and visits only the frames at which the reference's loop body can do anything:
//                 not triggered                  the next frame at or above the threshold;
//                 triggered, no silence open     the next frame below the negative threshold, or the first frame whose distance from
//                                                the speech's start exceeds maxSpeechSamples;
//                 triggered, a silence open      the next frame at or above the threshold (it closes the silence and may record it as a
//                                                candidate), the first low frame at which the silence has lasted minSilenceSamples (only a
//                                                low frame runs the end-of-speech test), or the max-duration frame.
//               Every other frame changes nothing but tempSilenceMinProb, which is folded in as a masked wave minimum over the low
//               lanes the jump passes.  The event frame itself goes through the reference's body, statement by statement.  possibleEnds
//               needs no storage: the cut reads the longest qualifying candidate, the longest one or the last one, each the first of
//               equal lengths (Sequence.max(by:) replaces its result only by a strictly greater element), so three running registers
//               stand for the list and are cleared where it is cleared.  The chain over the steps is serial, so the probabilities of
//               the next four steps are in flight while one is walked.
// vad_count /   the padding pass (:205-224: iteration i writes end[i] and start[i + 1], neither written before, so every gap is
// vad_write     independent), the clamps (:228-233, :43-50), the end > start filter and the times, lane = raw speech; the kept records
//               are placed by block_scan.h: block_exclusive counts a recording's, scan_totals places the recordings and
//               workgroup_exclusive the records within one.
// vad_pack      the model rows; vad_gather the ragged copy of the segments' audio; vad_stream the streaming machine, lane = stream.
// No kernel reads a frame or a sample of another recording than its own, and there are no float atomics.
#include "fa_common.h"
#include "block_scan.h"
#include "vad_launch.h"

namespace fa {
namespace vad {
namespace {

constexpr int64_t kFar = int64_t{1} << 44;   // samples no frame index below 2^31 can reach

template <class T> __device__ inline T least(const T x, const T y) { return y < x ? y : x; }
template <class T> __device__ inline T most(const T x, const T y) { return x < y ? y : x; }

__device__ inline float wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// the lowest set bit of m at or above `from` (0 ... 64), 64 when there is none
__device__ inline int next_bit(const uint64_t m, const int64_t from) {
    if (from >= 64) return 64;
    const uint64_t r = m >> from;
    return r ? static_cast<int>(from) + __builtin_ctzll(r) : 64;
}

// bits lo ... hi - 1, 0 <= lo < hi <= 64
__device__ inline uint64_t bit_range(const int64_t lo, const int64_t hi) {
    const uint64_t below_hi = hi >= 64 ? ~uint64_t{0} : (uint64_t{1} << hi) - 1;
    return below_hi & ~((uint64_t{1} << lo) - 1);
}

__global__ __launch_bounds__(kWave) void vad_machine(const SegArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const SegRecording r = a.rec[b];
    const int64_t F = r.frames;
    if (F == 0) {
        if (lane == 0) a.raw_counts[b] = 0;
        return;
    }
    const float *__restrict__ p = a.probs + r.frame0;
    RawSpeech *__restrict__ raw = a.raw + r.raw0;
    const Operands o = a.o;
    const float kInf = __builtin_inff(), kNan = __builtin_nanf("");
    // frames from a silence's first frame to the first one with frameStart - tempEnd >= minSilenceSamples
    const int64_t need = o.min_silence >= kFar ? kFar : (o.min_silence + kChunk - 1) / kChunk;
    const bool bounded = o.max_speech != kNone;

    bool triggered = false;
    int64_t speech_start = 0;                // currentSpeechStart, samples
    int64_t temp_end = -1;                   // tempEnd, samples; -1: nil
    float min_prob = kInf;                   // tempSilenceMinProb; inf: nil
    bool any = false, any_below = false;     // possibleEnds: is there one; one with minProbability <= silenceThresholdForSplit
    int64_t below_start = 0, below_len = 0, long_start = 0, long_len = 0, last_start = 0, last_len = 0;
    int32_t n = 0;                           // speeches.count

    // flushCurrentSpeechEnd: end_frame -1 stands for audioLengthSamples
    const auto flush = [&](const int64_t end_sample, const int32_t end_frame) {
        if (!(end_sample > speech_start)) return;
        if (end_sample - speech_start >= o.min_speech) {
            if (lane == 0 && n < F) raw[n] = RawSpeech{static_cast<int32_t>(speech_start / kChunk), end_frame};
            ++n;
        }
    };
    // a lane beyond the recording holds a NaN, which is in neither class
    const auto load = [&](const int64_t step) {
        const int64_t i = step * kWave + lane;
        return i < F ? p[i] : kNan;
    };

    const int64_t steps = (F + kWave - 1) / kWave;
    float q0 = load(0), q1 = load(1), q2 = load(2), q3 = load(3);
    for (int64_t k = 0; k < steps; ++k) {
        const float cur = q0;
        q0 = q1; q1 = q2; q2 = q3; q3 = load(k + 4);
        const uint64_t high = __ballot(cur >= o.threshold), low = __ballot(cur < o.negative_threshold);
        const int64_t b0 = k * kWave, bend = b0 + kWave < F ? b0 + kWave : F;
        int64_t c = b0;                      // frames below c are done
        for (;;) {
            int64_t e;                       // the next frame at which the body can do anything, b0 + 64 or beyond: not in this step
            if (!triggered) {
                e = b0 + next_bit(high, c - b0);
            } else {
                int64_t e_max = INT64_MAX;   // the first frame >= c with frameStart - currentSpeechStart > maxSpeechSamples
                if (bounded && o.max_speech < kFar) e_max = most(c, (speech_start + o.max_speech) / kChunk + 1);
                if (temp_end < 0) {
                    e = least(b0 + next_bit(low, c - b0), e_max);
                } else {
                    const int64_t from = most(c, temp_end / kChunk + need);
                    e = least(least(b0 + next_bit(high, c - b0), b0 + next_bit(low, from - b0)), e_max);
                }
            }
            const int64_t stop = e < bend ? e : bend;
            if (triggered && temp_end >= 0 && stop > c) {               // the low frames passed over: tempSilenceMinProb = min(..., prob)
                const uint64_t m = low & bit_range(c - b0, stop - b0);
                if (m) min_prob = fminf(min_prob, wave_min(((m >> lane) & 1) ? cur : kInf));
            }
            if (e >= bend) break;
            const int at = static_cast<int>(e - b0);
            const float prob = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur), at));
            const bool is_high = (high >> at) & 1, is_low = (low >> at) & 1;
            const int64_t frame_start = e * kChunk;
            c = e + 1;
            if (is_high) {                                                                       // :120-140
                if (temp_end >= 0) {
                    const int64_t silence = frame_start - temp_end;
                    if (silence > o.min_silence_at_max) {
                        const float mp = min_prob == kInf ? 1.0f : min_prob;
                        if (mp <= o.split_threshold && (!any_below || below_len < silence)) { below_start = temp_end; below_len = silence; any_below = true; }
                        if (!any || long_len < silence) { long_start = temp_end; long_len = silence; }
                        last_start = temp_end; last_len = silence; any = true;
                    }
                }
                temp_end = -1; min_prob = kInf;
                if (!triggered) { triggered = true; speech_start = frame_start; continue; }
            }
            if (triggered && bounded && frame_start - speech_start > o.max_speech) {             // :142-183
                int64_t s = last_start, d = last_len;
                if (any_below) { s = below_start; d = below_len; }
                else if (o.use_max) { s = long_start; d = long_len; }
                const int64_t split_end = any ? s : frame_start;
                flush(split_end, static_cast<int32_t>(split_end / kChunk));
                if (any && s + d < frame_start) { speech_start = s + d; triggered = true; }
                else triggered = false;
                any = any_below = false;
                temp_end = -1; min_prob = kInf;
                if (!triggered) continue;
            }
            if (is_low && triggered) {                                                           // :185-196
                if (temp_end < 0) temp_end = frame_start;
                min_prob = fminf(min_prob, prob);
                if (frame_start - temp_end >= o.min_silence) {
                    flush(temp_end, static_cast<int32_t>(temp_end / kChunk));
                    triggered = false;
                    temp_end = -1; min_prob = kInf;
                    any = any_below = false;
                }
            }
        }
    }
    if (triggered) flush(r.total, -1);                                                           // :199-201
    if (lane == 0) a.raw_counts[b] = n;
}

struct Finished {
    int64_t start, end;
    bool keep;
};

// Raw speech i of n behind the padding pass, the clamps and the filter.
__device__ inline Finished finish(const RawSpeech *__restrict__ raw, const int32_t i, const int32_t n, const int64_t total, const int64_t pad) {
    const auto start_of = [&](const int32_t j) { return static_cast<int64_t>(raw[j].start) * kChunk; };
    const auto end_of = [&](const int32_t j) {                         // min(endSample, audioLengthSamples) of the flush
        const int32_t f = raw[j].end;
        const int64_t e = f < 0 ? total : static_cast<int64_t>(f) * kChunk;
        return e < total ? e : total;
    };
    const auto share = [&](const int64_t silence) { return silence < 2 * pad ? silence / 2 : pad; };
    int64_t s = start_of(i), e = end_of(i);
    const int64_t back = i == 0 ? pad : share(s - end_of(i - 1));
    const int64_t ahead = i < n - 1 ? share(start_of(i + 1) - e) : pad;
    s = most(int64_t{0}, s - back);
    e = total - e <= ahead ? total : e + ahead;                        // min(audioLengthSamples, end + ahead), where end <= audioLengthSamples
    const int64_t cs = most(int64_t{0}, least(s, total)), ce = most(cs, least(e, total));              // :228-233, and :43-50 again
    return Finished{cs, ce, ce > cs};
}

__global__ __launch_bounds__(scan::kThreads) void vad_count(const SegArgs a) {
    const int b = blockIdx.x;
    const SegRecording r = a.rec[b];
    const int32_t n = least(a.raw_counts[b], r.frames);
    int mine = 0;
    for (int32_t i = threadIdx.x; i < n; i += scan::kThreads) mine += finish(a.raw + r.raw0, i, n, r.total, a.o.pad).keep ? 1 : 0;
    int total;
    (void)scan::block_exclusive(mine, &total);
    if (threadIdx.x == 0) { a.kept[b] = total; a.kept_counts[b] = total; }
}

__global__ __launch_bounds__(scan::kThreads) void vad_write(const SegArgs a) {
    const int b = blockIdx.x;
    const SegRecording r = a.rec[b];
    const int32_t n = least(a.raw_counts[b], r.frames);
    const int64_t first = a.kept[b];         // the records of the recordings before this one
    Finished f{0, 0, false};                 // raw speech i of this thread, from value_of(i) to place(i, ...)
    const auto keep_of = [&](const int32_t i) { f = finish(a.raw + r.raw0, i, n, r.total, a.o.pad); return f.keep ? 1 : 0; };
    (void)scan::workgroup_exclusive(n, keep_of, [&](int32_t, const int keep, const int at) {
        if (keep && first + at < a.out_slots)
            a.out[first + at] = fa_vad_segment{b, 0, f.start, f.end, static_cast<double>(f.start) / kRate, static_cast<double>(f.end) / kRate};
    });
}

// One workgroup per row: 1040 groups of four elements.
template <bool kWide>
__global__ __launch_bounds__(256) void vad_pack(const uint32_t *__restrict__ audio, const PackGroup g, uint32_t *__restrict__ rows) {
    const int64_t row = blockIdx.x;
    int rec = 0;
    while (rec + 1 < g.count && g.row_off[rec + 1] <= row) ++rec;
    const int64_t k = row - g.row_off[rec], n = g.audio_off[rec + 1] - g.audio_off[rec];
    const uint32_t *__restrict__ src = audio + g.audio_off[rec];
    uint32_t *__restrict__ out = rows + row * kRow;
    const auto element = [&](const int e) -> uint32_t {
        if (e < kContext) return k == 0 ? 0u : src[(k - 1) * kChunk + (kChunk - kContext) + e];  // the chunk before this one is a full one
        const int64_t s = k * kChunk + (e - kContext);
        return src[s < n ? s : n - 1];                                                           // a short chunk repeats its last sample
    };
    for (int j = threadIdx.x; j < kRow / 4; j += 256) {
        const uint32_t v0 = element(4 * j), v1 = element(4 * j + 1), v2 = element(4 * j + 2), v3 = element(4 * j + 3);
        if (kWide) {
            reinterpret_cast<uint4 *>(out)[j] = make_uint4(v0, v1, v2, v3);
        } else {
            out[4 * j] = v0; out[4 * j + 1] = v1; out[4 * j + 2] = v2; out[4 * j + 3] = v3;
        }
    }
}
static_assert(kRow % 4 == 0, "a row is whole groups of four");

__global__ __launch_bounds__(256) void vad_gather(const GatherArgs a) {
    const int64_t tile = blockIdx.x;
    int64_t lo = 0, hi = a.n_segments;       // the last segment with tile_off <= tile: segments without samples have no tile
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.tile_off[mid] <= tile) lo = mid; else hi = mid;
    }
    const int64_t len = a.out_range[lo + 1] - a.out_range[lo], first = (tile - a.tile_off[lo]) * kGatherTile;
    const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(a.audio) + a.src[lo] + first;
    uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(a.out) + a.out_range[lo] + first;
    const int64_t m = len - first < kGatherTile ? len - first : kGatherTile;
    for (int64_t j = threadIdx.x; j < m; j += 256) dst[j] = src[j];
}

__global__ __launch_bounds__(kWave) void vad_stream(const StreamArgs a) {
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kWave + threadIdx.x;
    if (s >= a.streams) return;
    fa_vad_stream_state st = a.states[s];
    const int32_t count = a.chunk_counts[s];
    for (int32_t k = 0; k < a.max_chunks; ++k) {
        const int64_t at = s * a.max_chunks + k;
        fa_vad_stream_event ev{static_cast<int32_t>(s), k, -1, 0, 0, __builtin_nan("")};
        if (k < count) {
            const float prob = a.probs[at];
            const int64_t chunk = a.chunk_samples ? a.chunk_samples[at] : kChunk;
            st.processed_samples += chunk;
            if (prob >= a.o.threshold) {
                st.has_temp_end = 0; st.temp_end_sample = 0;
                if (!st.triggered) {
                    st.triggered = 1;
                    ev.kind = FA_VAD_SPEECH_START;
                    ev.sample_index = most(int64_t{0}, st.processed_samples - a.o.pad - chunk);
                }
            } else if (prob < a.o.negative_threshold && st.triggered) {
                if (!st.has_temp_end) { st.has_temp_end = 1; st.temp_end_sample = st.processed_samples; }
                if (st.processed_samples - st.temp_end_sample >= a.o.min_silence) {
                    ev.kind = FA_VAD_SPEECH_END;
                    ev.sample_index = most(int64_t{0}, st.temp_end_sample + a.o.pad - chunk);
                    st.triggered = 0; st.has_temp_end = 0; st.temp_end_sample = 0;
                }
            }
            if (ev.kind >= 0 && a.return_seconds) {                     // makeStreamEvent
                const double seconds = static_cast<double>(ev.sample_index) / kRate;
                ev.time = round(seconds * a.factor) / a.factor;
            }
        }
        a.events[at] = ev;
    }
    a.states[s] = st;
}

}  // namespace

void launch_segments(hipStream_t stream, const SegArgs &a) {
    vad_machine<<<a.batch, kWave, 0, stream>>>(a);
    vad_count<<<a.batch, scan::kThreads, 0, stream>>>(a);
    scan::scan_totals<<<1, scan::kThreads, 0, stream>>>(a.kept, static_cast<int64_t>(a.batch), a.total);
    vad_write<<<a.batch, scan::kThreads, 0, stream>>>(a);
}

void launch_pack(hipStream_t stream, const float *audio, const PackGroup &g, float *rows, const bool wide) {
    const unsigned blocks = static_cast<unsigned>(g.row_off[g.count]);
    if (blocks == 0) return;
    if (wide) vad_pack<true><<<blocks, 256, 0, stream>>>(reinterpret_cast<const uint32_t *>(audio), g, reinterpret_cast<uint32_t *>(rows));
    else vad_pack<false><<<blocks, 256, 0, stream>>>(reinterpret_cast<const uint32_t *>(audio), g, reinterpret_cast<uint32_t *>(rows));
}

void launch_gather(hipStream_t stream, const GatherArgs &a) {
    if (a.tiles > 0) vad_gather<<<a.tiles, 256, 0, stream>>>(a);
}

void launch_stream(hipStream_t stream, const StreamArgs &a) {
    if (a.streams > 0) vad_stream<<<grid_for(a.streams, kWave), kWave, 0, stream>>>(a);
}

}  // namespace vad
}  // namespace fa
