// vocab_rescore_launch.h — what the vocabulary rescorer's host unit (vocab_rescore_host.hip: the argument passes, staging, launches, the
// one synchronisation, the C ABI) and its kernel unit (vocab_rescore.hip) share beyond the plain C++ of vocab_rescore_core.h: the
// tiling constants, the kernels' operands and their launchers.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"
#include "vocab_rescore_core.h"

namespace fa {
namespace vr {

constexpr int kWave = 64;
// A wavefront takes kStarts consecutive word starts of one utterance; its last two lanes walk the two words behind them only as the
// neighbours the compound guards of lanes 60 and 61 ask about (does word i + 1 / i + 2 match a single-word form at >= 0.9 on its own),
// so no lane needs a value of another wavefront.
constexpr int kHalo = 2;
constexpr int kStarts = kWave - kHalo;
constexpr int64_t kDefaultArena = 65536;

struct Block { int32_t utterance, first_word; };   // first_word: within the utterance

struct WalkArgs {
    const int32_t *blob;            // validated on the host before the upload
    Header h;
    const uint16_t *syms;           // dense ids of every word, back to back
    const int64_t *word_off;        // [words + 1]
    const int64_t *utt_words;       // [batch + 1]
    const uint8_t *flags;           // [words]
    int32_t *sid;                   // [words][4]: the sid of the phrase of 1 ... 4 words from a word (spaced), -1 none, -2 empty or past the utterance
    int64_t n_words;
    int32_t batch;
    const Block *blocks;
    int32_t n_blocks;
    float min_similarity;
    fa_vr_candidate *arena;
    int64_t arena_cap;
    unsigned long long *cursor;     // survivors so far, whether they fitted or not
};

// the pre-pass: lane = (word, span length)
void launch_sids(hipStream_t stream, const WalkArgs &a);
// the walk: one wavefront per (block, term); a.h.A * 8 bytes of LDS
void launch_walk(hipStream_t stream, const WalkArgs &a);

}  // namespace vr
}  // namespace fa
