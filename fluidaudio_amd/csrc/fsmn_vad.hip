// fsmn_vad.hip — the kernels of FSMN-VAD (host side: fsmn_vad_host.hip; plans, operands and the restated reference lines:
// fsmn_vad_launch.h; the word step: fsmn_vad_core.h).
//
// fsmn_vad_machine  decide (FsmnVadManager.swift:159-201), one wavefront per recording, lane = frame, 64 frames a step.  A step is the
//                   speech ballot (p <= threshold: a NaN, and a lane beyond the recording, is not speech), every lane's window count from
//                   that ballot and the one before it, two ballots for the four classes of a frame's effect on preSpeech, every lane's
//                   state in closed form (state_at: a find-last-set and a masked population count) and its ballot, and then walk_step:
//                   wave-uniform code that jumps from a segment's opening to its close on that word.  The chain over the steps is
//                   serial, so the probabilities of the next four steps are in flight while one is walked.
// fsmn_vad_write    the records of every recording's slice, placed in the call's output by scan_totals (block_scan.h) of the slices' fill.
// rows::pack        the scorer-side rows: the scaled waveform of a chunk (row_pack.h, with its scale); fsmn_vad_feats the zero-padded bucket of features;
//                   fsmn_vad_gather column 0 of the scores, onto the recording's frame grid.
// No kernel reads a frame or a sample of another recording than its own, and there are no atomics.
#include <hip/hip_fp16.h>

#include "fa_common.h"
#include "block_scan.h"
#include "fsmn_vad_launch.h"
#include "row_pack.h"

namespace fa {
namespace fsmnvad {
namespace {

__global__ __launch_bounds__(kWave) void fsmn_vad_machine(const SegArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const SegRecording r = a.rec[b];
    const int64_t F = r.frames;
    const float *__restrict__ p = a.probs + r.frame0;
    RawSegment *__restrict__ slice = a.arena + r.slot0;
    const Params o = a.o;
    const float kNan = __builtin_nanf("");

    Machine m = machine_start();
    const auto emit = [&](const int64_t start, const int64_t end, const int32_t reason) {
        if (lane == 0 && m.count < r.slots) slice[m.count] = RawSegment{static_cast<int32_t>(start), static_cast<int32_t>(end), reason};
        ++m.count;
    };
    const auto load = [&](const int64_t step) {
        const int64_t i = step * kWave + lane;
        return i < F ? p[i] : kNan;
    };

    const int64_t steps = (F + kWave - 1) / kWave;
    float q0 = load(0), q1 = load(1), q2 = load(2), q3 = load(3);
    for (int64_t k = 0; k < steps; ++k) {
        const float cur = q0;
        q0 = q1; q1 = q2; q2 = q3; q3 = load(k + 4);
        const uint64_t speech = __ballot(cur <= o.threshold);
        const int w = window_count(m.prev, speech, o.window, lane);
        const Classes c = classes(__ballot(w >= o.on), __ballot(w > o.off));
        const uint64_t P = __ballot(state_at(c, 0, m.pre_speech, lane));
        const int64_t b0 = k * kWave;
        const int v = F - b0 < kWave ? static_cast<int>(F - b0) : kWave;
        walk_step(m, o, b0, v, P, [&](const int from) -> uint64_t { return __ballot(state_at(c, from, false, lane)); }, emit);
        m.prev = speech;
    }
    if (m.in_seg) emit(m.seg_start, F, kEndOfAudio);                  // :199
    if (lane == 0) {
        a.counts[b] = static_cast<int32_t>(m.count);                  // at most F: every segment opens at a frame of its own
        a.kept[b] = static_cast<int32_t>(m.count < r.slots ? m.count : r.slots);
    }
}

__global__ __launch_bounds__(scan::kThreads) void fsmn_vad_write(const SegArgs a) {
    const int b = blockIdx.x;
    const SegRecording r = a.rec[b];
    const int32_t n = a.counts[b] < r.slots ? a.counts[b] : r.slots;
    const int64_t at = a.kept[b];            // the records of the recordings before this one
    const RawSegment *__restrict__ slice = a.arena + r.slot0;
    for (int32_t i = threadIdx.x; i < n; i += scan::kThreads) {
        const int64_t slot = at + i;
        if (slot >= a.out_slots) break;
        const RawSegment s = slice[i];
        a.out[slot] = fa_fsmn_vad_segment{b, s.reason, s.start, s.end, static_cast<int64_t>(s.start) * a.o.frame_ms, static_cast<int64_t>(s.end) * a.o.frame_ms};
    }
}

// blockIdx.y: the chunk; a thread per group of four elements of its [bucket][400] output
template <bool kHalf, bool kWide>
__global__ __launch_bounds__(256) void fsmn_vad_feats(const void *__restrict__ feats, const int64_t feat_stride, const FeatGroup g, const int32_t bucket, float *__restrict__ out) {
    const int chunk = blockIdx.y;
    const int64_t quads = static_cast<int64_t>(bucket) * (kFeatureDim / 4), copied = static_cast<int64_t>(g.frames[chunk]) * (kFeatureDim / 4);
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j >= quads) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                   // :134: the rows behind the chunk's frames
    if (j < copied) {
        const int64_t at = (chunk * feat_stride * kFeatureDim) + 4 * j;
        if (kHalf) {
            const __half *__restrict__ s = static_cast<const __half *>(feats) + at;
            if (kWide) {
                const uint2 w = *reinterpret_cast<const uint2 *>(s);
                v = make_float4(__half2float(__ushort_as_half(static_cast<unsigned short>(w.x & 0xffffu))), __half2float(__ushort_as_half(static_cast<unsigned short>(w.x >> 16))),
                                __half2float(__ushort_as_half(static_cast<unsigned short>(w.y & 0xffffu))), __half2float(__ushort_as_half(static_cast<unsigned short>(w.y >> 16))));
            } else {
                v = make_float4(__half2float(s[0]), __half2float(s[1]), __half2float(s[2]), __half2float(s[3]));
            }
        } else {
            const float *__restrict__ s = static_cast<const float *>(feats) + at;
            v = kWide ? *reinterpret_cast<const float4 *>(s) : make_float4(s[0], s[1], s[2], s[3]);
        }
    }
    float *__restrict__ dst = out + (chunk * quads + j) * 4;
    if (kWide) {
        *reinterpret_cast<float4 *>(dst) = v;
    } else {
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
}

// blockIdx.y: the chunk; a thread per frame of the bucket
template <bool kHalf>
__global__ __launch_bounds__(256) void fsmn_vad_gather(const void *__restrict__ scores, const int32_t bucket, const int32_t vocab, const GatherGroup g, float *__restrict__ silence) {
    const int chunk = blockIdx.y;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < g.keep_from[chunk] || i >= g.frames[chunk]) return;
    const int64_t at = (static_cast<int64_t>(chunk) * bucket + i) * vocab;                       // :150: col 0 = silence prob
    silence[g.dst[chunk] + (i - g.keep_from[chunk])] = kHalf ? __half2float(static_cast<const __half *>(scores)[at]) : static_cast<const float *>(scores)[at];
}

}  // namespace

void launch_segments(hipStream_t stream, const SegArgs &a) {
    fsmn_vad_machine<<<a.batch, kWave, 0, stream>>>(a);
    scan::scan_totals<<<1, scan::kThreads, 0, stream>>>(a.kept, static_cast<int64_t>(a.batch), a.total);
    if (a.out_slots > 0) fsmn_vad_write<<<a.batch, scan::kThreads, 0, stream>>>(a);
}

void launch_pack(hipStream_t stream, const float *audio, const rows::Group &g, float *out, const int64_t row_stride, const bool wide) {
    rows::launch_pack<true>(stream, audio, g, row_stride, out, nullptr, wide, 32768.0f);   // :123: one fp32 multiply
}

void launch_feats(hipStream_t stream, const void *feats, const int32_t dtype, const int64_t feat_stride, const FeatGroup &g, const int32_t bucket, float *out, const bool wide) {
    if (g.count == 0 || bucket == 0) return;
    const dim3 grid(grid_for(static_cast<int64_t>(bucket) * (kFeatureDim / 4), 256), static_cast<unsigned>(g.count));
    const bool half = dtype == FA_DTYPE_F16;
    if (half && wide) fsmn_vad_feats<true, true><<<grid, 256, 0, stream>>>(feats, feat_stride, g, bucket, out);
    else if (half) fsmn_vad_feats<true, false><<<grid, 256, 0, stream>>>(feats, feat_stride, g, bucket, out);
    else if (wide) fsmn_vad_feats<false, true><<<grid, 256, 0, stream>>>(feats, feat_stride, g, bucket, out);
    else fsmn_vad_feats<false, false><<<grid, 256, 0, stream>>>(feats, feat_stride, g, bucket, out);
}

void launch_gather(hipStream_t stream, const void *scores, const int32_t dtype, const int32_t bucket, const int32_t vocab, const GatherGroup &g, float *silence) {
    if (g.count == 0 || bucket == 0) return;
    const dim3 grid(grid_for(bucket, 256), static_cast<unsigned>(g.count));
    if (dtype == FA_DTYPE_F16) fsmn_vad_gather<true><<<grid, 256, 0, stream>>>(scores, bucket, vocab, g, silence);
    else fsmn_vad_gather<false><<<grid, 256, 0, stream>>>(scores, bucket, vocab, g, silence);
}

}  // namespace fsmnvad
}  // namespace fa
