// fsmn_vad_core.h — the integers and the bit steps of FSMN-VAD that the host (fsmn_vad_launch.h), the kernel (fsmn_vad.hip) and the
// stand-alone program tests/cpu/fsmn_vad_core_main.cpp share: the preprocessor's geometry (FsmnVadManager.swift:25-34, 113-117), and
// decide (:159-201) as a machine that advances 64 frames a step on 64-bit words.
//
// decide, restated.  Per frame t: cur = p <= threshold; the window count w over the last window_frames values of cur (a zero-filled ring);
//     if !preSpeech && w >= on   { preSpeech = true; if !inSeg { inSeg = true; segStart = max(0, t - on - lookback); contSil = 0 } }
//     else if preSpeech && w <= off { preSpeech = false }
//     contSil = inSeg && !preSpeech ? contSil + 1 : 0
//     if inSeg && contSil >= maxEndSilence        close(at: t - maxEndSilence + lookahead)
//     else if inSeg && t - segStart >= maxSegment { close(at: t); preSpeech = false }
// and close(at: T) behind the loop when a segment is open.
//
// The word step.  What a frame does to preSpeech is a function on {false, true} that its count alone decides (classes below): set,
// clear, toggle or hold.  A composition of such functions is the last set / clear among them, xor the parity of the toggles behind it —
// or the carry-in xor the parity of all toggles where there is none.  So the state behind every lane of a step follows from three words
// with a find-last-set and a masked population count (state_at).  A segment's bookkeeping touches preSpeech in one place only, the
// maximal-length close, which clears it: the walk recomputes the word behind that frame with carry-in false.  Outside a segment
// preSpeech is false (an end-silence close needs contSil >= 1, which needs it false at that frame; the other close clears it), so the next
// segment opens at the first set bit of the word.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FA_FV_HD __host__ __device__
#else
#define FA_FV_HD
#endif

namespace fa {
namespace fsmnvad {

constexpr int kWave = 64;
constexpr int kHop = 160, kFbankWindow = 400, kLfrPad = 2, kLfrWidth = 5;   // hopSamples, fbankWindowSamples, lfrPadFrames, lfrWidth
constexpr int kFeatureDim = 400;
constexpr int kBuckets[4] = {512, 1024, 2048, 3072};
constexpr int kChunkWindowFrames = 20;                                      // the windowFrames of chunkSamples (:95): the reference's constant, not the config's
constexpr int64_t kChunkSamples = static_cast<int64_t>(kBuckets[3] - kChunkWindowFrames) * kHop;
constexpr int32_t kEndSilence = 0, kMaxLength = 1, kEndOfAudio = 2;         // fa_fsmn_vad_segment.reason

// lfrFrameCount (:113-117)
FA_FV_HD constexpr int64_t frame_count(const int64_t samples) {
    if (samples < kFbankWindow) return 0;
    const int64_t fbank = (samples - kFbankWindow) / kHop + 1, n = fbank + kLfrPad - kLfrWidth + 1;
    return n > 0 ? n : 0;
}

// buckets.first(where: { $0 >= t }) ?? buckets.last! (:131)
FA_FV_HD constexpr int32_t bucket_for(const int64_t frames) {
    return frames <= kBuckets[0] ? kBuckets[0] : frames <= kBuckets[1] ? kBuckets[1] : frames <= kBuckets[2] ? kBuckets[2] : kBuckets[3];
}

struct Params {                              // a checked fa_fsmn_vad_config
    float threshold;
    int32_t window, on, off, max_end_silence, lookback, lookahead, max_segment, frame_ms;
};

// bits lo ... hi - 1, 0 <= lo <= hi <= 64
FA_FV_HD inline uint64_t bit_range(const int lo, const int hi) {
    const uint64_t below_hi = hi >= 64 ? ~uint64_t{0} : (uint64_t{1} << hi) - 1;
    const uint64_t below_lo = lo >= 64 ? ~uint64_t{0} : (uint64_t{1} << lo) - 1;
    return below_hi & ~below_lo;
}

// the lowest set bit of m at or above `from` (0 ... 64), 64 when there is none
FA_FV_HD inline int next_bit(const uint64_t m, const int from) {
    if (from >= 64) return 64;
    const uint64_t r = m >> from;
    return r ? from + __builtin_ctzll(r) : 64;
}

// The window count of lane `lane`: the speech bits of frames lane - window + 1 ... lane, from this step's ballot and the one before it
// (zero in front of a recording, as the reference's ring is).  1 <= window <= 64, so the two words always hold them.
FA_FV_HD inline int window_count(const uint64_t prev, const uint64_t cur, const int window, const int lane) {
    const int lo = lane - window + 1;
    if (lo >= 0) return __builtin_popcountll(cur & bit_range(lo, lane + 1));
    return __builtin_popcountll(cur & bit_range(0, lane + 1)) + __builtin_popcountll(prev >> (64 + lo));   // 64 + lo is 1 ... 63
}

// The classes of a step's frames, two ballots: at_on = (w >= on), above_off = (w > off).
//   set = at_on & above_off, clear = ~at_on & ~above_off, toggle = at_on & ~above_off, hold = ~at_on & above_off
struct Classes {
    uint64_t fixed;                          // set or clear
    uint64_t value;                          // set (within fixed)
    uint64_t toggle;
};
FA_FV_HD inline Classes classes(const uint64_t at_on, const uint64_t above_off) {
    return Classes{~(at_on ^ above_off), at_on & above_off, at_on & ~above_off};
}

// preSpeech behind lane `lane` when it was `carry` in front of lane `from` and only the lanes from ... lane acted; false below from
FA_FV_HD inline bool state_at(const Classes &c, const int from, const bool carry, const int lane) {
    if (lane < from) return false;
    const uint64_t span = bit_range(from, lane + 1);
    const uint64_t fixed = c.fixed & span;
    bool s = carry;
    uint64_t toggles = c.toggle & span;
    if (fixed) {
        const int j = 63 - __builtin_clzll(fixed);
        s = (c.value >> j) & 1;
        toggles &= bit_range(j + 1, 64);
    }
    return s != ((__builtin_popcountll(toggles) & 1) != 0);
}

struct Machine {                             // what decide carries from frame to frame, between two steps
    uint64_t prev;                           // the speech ballot of the step before
    bool pre_speech, in_seg;
    int64_t seg_start;
    int64_t max_at;                          // the frame of the segment's maximal-length close
    int64_t silence;                         // contSil
    int64_t count;                           // segments closed so far
};
FA_FV_HD inline Machine machine_start() { return Machine{0, false, false, 0, 0, 0, 0}; }

// The first lane e in [c, v) at which a run of clear bits of P, begun `*silence` frames in front of lane c, reaches `need` frames; 64 when
// none does, and then *silence is the run in front of lane v: the carry plus the leading zeros when no bit is set, else the trailing ones.
FA_FV_HD inline int silence_close(const uint64_t P, int c, const int v, const int64_t need, int64_t *silence) {
    const uint64_t valid = bit_range(0, v);
    if (*silence + (v - c) < need) {         // no run can reach it in this step
        const uint64_t ones = P & bit_range(c, v);
        *silence = ones ? v - 1 - (63 - __builtin_clzll(ones)) : *silence + (v - c);
        return 64;
    }
    int64_t run = *silence;
    while (c < v) {
        const int one = next_bit(P & valid, c);                         // the run's end
        const int stop = one < v ? one : v;
        if (run + (stop - c) >= need) return c + static_cast<int>(need - run) - 1;
        if (stop == v) { run += stop - c; break; }
        const int zero = next_bit(~P & valid, stop);                    // behind the ones
        c = zero < v ? zero : v;
        run = 0;
    }
    *silence = run;
    return 64;
}

// One step of decide: frames b0 ... b0 + v - 1 (1 <= v <= 64), whose preSpeech word with the machine's carry-in is P.  recompute(from)
// answers the word with carry-in false in front of lane `from` (lanes below it clear); emit(start_frame, end_frame, reason) takes a closed
// segment.  Everything here is uniform over a wavefront.
template <class Recompute, class Emit>
FA_FV_HD inline void walk_step(Machine &m, const Params &o, const int64_t b0, const int v, uint64_t P, const Recompute &recompute, const Emit &emit) {
    const uint64_t valid = bit_range(0, v);
    int c = 0;                               // lanes below c are done
    while (c < v) {
        if (!m.in_seg) {
            const int e = next_bit(P & valid, c);
            if (e >= v) break;
            const int64_t t = b0 + e, back = t - o.on - o.lookback;
            m.in_seg = true;
            m.seg_start = back > 0 ? back : 0;
            m.max_at = m.seg_start + o.max_segment > t ? m.seg_start + o.max_segment : t;
            m.silence = 0;
            c = e + 1;
            if (m.max_at == t) {             // contSil is 0 at the opening frame, so only the maximal length can close it there
                emit(m.seg_start, t, kMaxLength);
                m.in_seg = false;
                P = recompute(c);
            }
            continue;
        }
        const int64_t at_max = m.max_at - b0;                           // >= c: an earlier frame would have closed the segment
        const int e = silence_close(P, c, v, o.max_end_silence, &m.silence);
        if (e < v && e <= at_max) {
            emit(m.seg_start, b0 + e - o.max_end_silence + o.lookahead, kEndSilence);
            m.in_seg = false;
            c = e + 1;
        } else if (at_max < v) {
            emit(m.seg_start, m.max_at, kMaxLength);
            m.in_seg = false;
            c = static_cast<int>(at_max) + 1;
            P = recompute(c);
        } else {
            break;
        }
    }
    m.pre_speech = (P >> (v - 1)) & 1;
}

}  // namespace fsmnvad
}  // namespace fa
