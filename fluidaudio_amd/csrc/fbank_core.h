// fbank_core.h — the integers and the summation order the Kaldi fbank + LFR + CMVN kernel (fbank.hip) shares with its host code
// (fbank_host.hip) and with tests/cpu/fbank_core_main.cpp: frame and row counts, the tile geometry, and the enumeration "which
// (row, slot) of the stacked output does fbank frame t write", which is what lets the kernel store every feature straight into
// its final place with no intermediate [T, n_mels] tensor, no atomics and no second pass.  Plain C++: no HIP type appears here.
#pragma once
#include <stdint.h>

#include "mel_core.h"   // FA_HD, the 16-lane frame group and the radix-16 phases the kernel reuses

namespace fa {
namespace fbank {

constexpr int kTileFrames = 32;   // consecutive frames of one utterance a workgroup owns
constexpr int kThreads = 256;     // 16 groups of 16 lanes: one frame per group and pass, two passes per tile
constexpr int kGroups = kThreads / fa::melcore::kGroup;
constexpr int kPasses = kTileFrames / kGroups;
constexpr int kMaxMels = 256;
constexpr int kMaxLfr = 64;       // largest m of LFR(m, n)
constexpr int kTailReplicate = 0, kTailValid = 1;   // FA_FBANK_TAIL_*

// snip-edges frame count: no padding, no partial frame
FA_HD int64_t num_frames(const int64_t n, const int win, const int hop) { return n < win ? 0 : 1 + (n - win) / hop; }

FA_HD int lfr_lpad(const int m) { return (m - 1) / 2; }

// rows of LFR(m, n) over T frames.  REPLICATE (WavFrontend): ceil(T / n), the last rows repeat frame T - 1.  VALID (the FSMN-VAD
// preprocessor as converted): only rows whose last slot is a real frame, max(0, floor((T + lpad - m) / n) + 1).
FA_HD int64_t num_rows(const int64_t T, const int m, const int n, const int tail) {
    if (T <= 0) return 0;
    if (tail == kTailValid) { const int64_t u = T + lfr_lpad(m) - m; return u < 0 ? 0 : u / n + 1; }
    return (T + n - 1) / n;
}

// Row i, slot k of the output takes frame clamp(i n + k - lpad, 0, T - 1).  Seen from the frame: frame t is written to
//   (a) every slot k with (t + lpad - k) divisible by n and row (t + lpad - k) / n in [0, R)        — its own place,
//   (b) t == 0:     every (i, k) with i n + k - lpad < 0                                            — the replicated head,
//   (c) t == T - 1: every (i, k) with i n + k - lpad > T - 1                                        — the replicated tail,
// and (a), (b), (c) are disjoint, so over t = 0 .. T - 1 every (i, k) of the R x m output is visited exactly once.
// fn(row, slot) is called in ascending slot order, rows ascending inside a slot.
template <class F>
FA_HD void for_each_target(const int t, const int T, const int R, const int m, const int n, F &&fn) {
    const int lpad = lfr_lpad(m);
    for (int k = 0; k < m; ++k) {
        if (t == 0)
            for (int i = 0; i < R && i * n + k - lpad < 0; ++i) fn(i, k);
        const int u = t + lpad - k;
        if (u >= 0 && u % n == 0 && u / n < R) fn(u / n, k);
        if (t == T - 1) {
            const int v = T - 1 + lpad - k;
            for (int i = v < 0 ? 0 : v / n + 1; i < R; ++i) fn(i, k);
        }
    }
}

// ---- the frame mean (remove_dc): its summation order is part of the result ----------------------------------------------------
// Lane l of the frame's 16-lane group holds the samples at frame positions 32 n1 + 2 l and 32 n1 + 2 l + 1, n1 = 0 .. 15 (positions
// >= win hold 0).  It adds them to 0.0f in ascending position order: this is lane_partial().  The 16 partials are then combined by
// a butterfly, s_l <- s_l + s_(l ^ d) for d = 1, 2, 4, 8 in that order; fp32 addition commutes, so all 16 lanes end with the same
// bits.  The mean is that sum divided (not multiplied by a reciprocal) by win: a constant frame whose sum is exact has an exact mean.
FA_HD float lane_partial(const float (&re)[16], const float (&im)[16]) {
    float s = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int n1 = 0; n1 < 16; ++n1) { s += re[n1]; s += im[n1]; }
    return s;
}

}  // namespace fbank
}  // namespace fa
