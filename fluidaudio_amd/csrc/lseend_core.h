// lseend_core.h — the integers of the LS-EEND front end (kernels: lseend.hip, host code: lseend_host.hip), restated from the two
// StreamingChunkQueues of Diarizer/LS-EEND/LSEENDPreprocessor.swift:52-61,94-105,158-180,362-376, and the one definition of the
// cumulative mean's summation order.  Everything the queues decide depends on sample counts only, so the host computes it before a
// launch and no kernel counts, waits or allocates.  Plain C++: no HIP type appears here; tests/test_lseend_cpu.py checks it
// through fa_lseend_plan_file / fa_lseend_plan_push against a literal restatement of the two queues.
//
// Positions.  The audio queue is one endless array: n_fft / 2 zeros, then every sample pushed (flush zeros included).  Its head only
// moves by whole chunks of hop * subsampling * chunk_size samples, so mel frame f always covers queue positions [f hop, f hop + n_fft).
// The mel queue is one endless array of rows: context_size literal zero rows, then normalised frame f at row context_size + f.
// Window c is rows [c chunk_mels, c chunk_mels + mel_frames).  The decoder mask end is min(windows chunk_size, conv_delay + chunk_size).
//
// The cumulative mean.  mu_k = float(S_k / k), y_k = x_k - mu_k in fp32, where S_k is the fp64 sum of x_1 .. x_k taken as: the carried
// sum, plus the sums of the call's whole tiles in front of frame k's tile (each a sum over kTileFrames frames in ascending order from
// 0.0, added to the running total in ascending tile order), plus the frames of its own tile up to k added one by one to that total.
// The reference runs mu_k = mu_(k-1) + (x_k - mu_(k-1)) / k in fp32 (:268-275); the two are equal in exact arithmetic.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FA_LSEEND_HD __host__ __device__ __forceinline__
#else
#define FA_LSEEND_HD inline
#endif

namespace fa {
namespace lseend {

constexpr int kTileFrames = 32;   // consecutive frames of one item a workgroup owns
constexpr int kThreads = 256;     // 16 groups of 16 lanes: one frame per group and pass, two passes per tile
constexpr int kGroups = kThreads / 16;
constexpr int kPasses = kTileFrames / kGroups;
constexpr int kNfft = 256;        // the radix-16 x radix-16 route; every other n_fft is refused (FA_INVALID_ARGUMENT)
constexpr int kBins = kNfft / 2 + 1;
constexpr int kMaxMels = 128;     // the carry kernel: lane = mel bin, two bins per lane beyond 64

struct Geometry {
    int n_fft, hop, win, n_mels, context, subsampling, conv_delay, chunk;
    int chunk_mels;       // subsampling * chunk
    int chunk_samples;    // hop * chunk_mels
    int audio_context;    // n_fft - hop: left n_fft / 2 plus right n_fft / 2 - hop (:53-56)
    int mel_context;      // 2 context + 1 - subsampling: left context plus right context + 1 - subsampling (:97)
    int mel_frames;       // (chunk - 1) subsampling + 2 context + 1 = chunk_mels + mel_context (LSEENDTypes.swift:53)
    int flush_samples;    // (context + conv_delay subsampling) hop + n_fft / 2 (:59-61)
    int audio_tail_cap;   // unread samples a stream can carry: chunk_samples + audio_context - 1
    int mel_tail_cap;     // unread rows a stream can carry: mel_frames - 1
    int mask_len;         // conv_delay + chunk
};

// false: a geometry the queues cannot run (or this library refuses: a negative mel context would let the head pass the rows written)
FA_LSEEND_HD bool make_geometry(int n_fft, int hop, int win, int n_mels, int context, int subsampling, int conv_delay, int chunk, Geometry &g) {
    if (n_fft < 2 || hop < 1 || hop > n_fft / 2 || win < 2 || win > n_fft || n_mels < 1 || context < 0 || subsampling < 1 || conv_delay < 0 || chunk < 1) return false;
    if (context > 4096 || subsampling > 4096 || conv_delay > 4096 || chunk > 4096) return false;
    g.n_fft = n_fft; g.hop = hop; g.win = win; g.n_mels = n_mels; g.context = context; g.subsampling = subsampling; g.conv_delay = conv_delay; g.chunk = chunk;
    g.chunk_mels = subsampling * chunk;
    g.chunk_samples = hop * g.chunk_mels;
    g.audio_context = n_fft - hop;
    g.mel_context = 2 * context + 1 - subsampling;
    if (g.mel_context < 0) return false;
    g.mel_frames = g.chunk_mels + g.mel_context;
    g.flush_samples = (context + conv_delay * subsampling) * hop + n_fft / 2;
    g.audio_tail_cap = g.chunk_samples + g.audio_context - 1;
    g.mel_tail_cap = g.mel_frames - 1;
    g.mask_len = conv_delay + chunk;
    return true;
}

// What a stream has seen so far.  A fresh stream (and every recording of the offline call) starts from fresh().
struct Counters {
    int64_t audio;     // audio queue length: n_fft / 2 + samples pushed
    int64_t frames;    // mel frames computed = the CMN count
    int64_t windows;   // windows emitted
};
FA_LSEEND_HD Counters fresh(const Geometry &g) { return Counters{g.n_fft / 2, 0, 0}; }

// popAllChunks (:370-376): the whole chunks in front of the context, all at once; frames = chunks * chunk_mels
FA_LSEEND_HD int64_t frames_of(const Geometry &g, const int64_t audio) {
    const int64_t over = audio - g.audio_context;
    return over < g.chunk_samples ? 0 : over / g.chunk_samples * g.chunk_mels;
}
// popNextChunk (:362-367) until it fails: every window whose mel_frames rows are there
FA_LSEEND_HD int64_t windows_of(const Geometry &g, const int64_t frames) {
    const int64_t over = g.context + frames - g.mel_context;
    return over < g.chunk_mels ? 0 : over / g.chunk_mels;
}
FA_LSEEND_HD int64_t unread_audio(const Geometry &g, const Counters &c) { return c.audio - c.frames * g.hop; }
FA_LSEEND_HD int64_t unread_mel(const Geometry &g, const Counters &c) { return g.context + c.frames - c.windows * g.chunk_mels; }
// drainRightContextWithSilence (:158-174): the zeros a flush appends behind `audio` queue positions
FA_LSEEND_HD int64_t flush_zeros(const Geometry &g, const Counters &c, const int64_t audio) {
    const int64_t unread = audio + g.flush_samples - c.frames * g.hop;
    const int64_t over = unread > g.audio_context ? unread - g.audio_context : 0;
    return g.flush_samples + (g.chunk_samples - over % g.chunk_samples) % g.chunk_samples;
}

// emitNextChunk (:192-199) for the window with index c of its stream: the mask end behind it, its warm-up rows, and the rows
// [warmup, chunk) every window in front of it has kept (the offset of its own rows in the dense probabilities)
FA_LSEEND_HD int mask_end_of(const Geometry &g, const int64_t windows) {
    return windows * g.chunk < g.mask_len ? static_cast<int>(windows * g.chunk) : g.mask_len;
}
FA_LSEEND_HD int warmup_of(const Geometry &g, const int64_t c) {
    const int left = g.mask_len - mask_end_of(g, c + 1);
    return left < g.chunk ? left : g.chunk;
}
FA_LSEEND_HD int64_t rows_before(const Geometry &g, const int64_t c) {
    const int64_t r = c * g.chunk - g.conv_delay;
    return r > 0 ? r : 0;
}

// One call on one item: `samples` new samples, then (flush) the zeros of flush_zeros.  Advances c and says what the kernels do.
struct Step {
    int64_t frames0, windows0;      // the counters before
    int32_t tail_in, tail_out;      // unread audio before / after
    int32_t mel_in, mel_out;        // unread mel rows before / after
    int64_t zeros;                  // flush zeros appended
    int64_t frames, windows;        // computed / emitted by this call
    int64_t out_rows;               // rows [warmup, chunk) of the emitted windows
};
FA_LSEEND_HD Step advance(const Geometry &g, Counters &c, const int64_t samples, const bool flush) {
    Step s;
    s.frames0 = c.frames; s.windows0 = c.windows;
    s.tail_in = static_cast<int32_t>(unread_audio(g, c));
    s.mel_in = static_cast<int32_t>(unread_mel(g, c));
    s.zeros = flush ? flush_zeros(g, c, c.audio + samples) : 0;
    c.audio += samples + s.zeros;
    c.frames = frames_of(g, c.audio);
    c.windows = windows_of(g, c.frames);
    s.frames = c.frames - s.frames0; s.windows = c.windows - s.windows0;
    s.tail_out = static_cast<int32_t>(unread_audio(g, c));
    s.mel_out = static_cast<int32_t>(unread_mel(g, c));
    s.out_rows = rows_before(g, c.windows) - rows_before(g, s.windows0);
    return s;
}

// Which (window, row) slots take mel-queue row q, among the windows [w0, w1) a call emits: fn(window, row), windows ascending.
template <class F>
FA_LSEEND_HD void for_each_slot(const Geometry &g, const int64_t q, const int64_t w0, const int64_t w1, F &&fn) {
    int64_t lo = q - g.mel_frames + 1;
    lo = lo <= 0 ? 0 : (lo + g.chunk_mels - 1) / g.chunk_mels;
    int64_t hi = q / g.chunk_mels + 1;
    if (lo < w0) lo = w0;
    if (hi > w1) hi = w1;
    for (int64_t c = lo; c < hi; ++c) fn(c, static_cast<int>(q - c * g.chunk_mels));
}

}  // namespace lseend
}  // namespace fa
