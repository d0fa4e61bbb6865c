// beam_launch.h — what beam search's host code (beam_host.hip: the ARPA reader, the language model's hash tables, the vocabulary, the launch
// plan, the C ABI) and its kernel translation unit (beam.hip) share: the limits, the records of the tables in HBM, the operands of the two
// kernel families, the model's scoring — the same functions serve fa_arpa_score on the host and the frame walk on the device — and one
// launcher per kernel family with the query that says which instance serves a call.  Template arguments are named in beam.hip only.
// Internal; not part of the C ABI.  Launch errors surface through hipGetLastError().
#pragma once
#include "fa_common.h"

namespace fa {
namespace beam {

constexpr int kMaxBeam = 128;
constexpr int kMaxTop = 64;
constexpr uint64_t kHashBase = 0x100000001b3ull;   // odd: multiplication by it is a bijection mod 2^64
constexpr float kUnkLogProb = -23.026f;            // ARPALanguageModel.unkLogProb (:33)

struct UniEntry { uint64_t h; int32_t len; float logp, backoff; int32_t used; };
struct BiEntry { uint64_t hp, hw; int32_t lp, lw; float logp; int32_t used; };
struct TokInfo { uint64_t mult, add; int32_t len, boundary; };   // stripped piece: h' = h * mult + add, len' = len + this len

struct LmView {
    const UniEntry *uni; const BiEntry *bi;
    uint32_t uni_mask, bi_mask;   // capacity - 1
};

struct TopEntry { int32_t tok; float lp; };   // tok: token id, bit 31 = the piece starts a word (TokInfo::boundary)

struct TopArgs {
    const float *logp; const int32_t *valid; const TokInfo *tok;
    TopEntry *top;                             // [utterance of the launch][frame][top_k + 1]: the K best tokens, then (lp) the blank's log-probability
    int64_t row_stride, matrix_stride, rows;
    int32_t frames, vocab, blank, top_k, first, use_lm;
};

struct BeamArgs {
    const float *logp; const int32_t *valid; const TokInfo *tok; LmView lm;
    unsigned long long *arena;   // [B][arena_stride] trie = hash table of (parent node << 32 | token), node id = slot; -1 = empty prefix
    int32_t *tokens, *lens; float *scores;
    int64_t row_stride, matrix_stride, arena_stride;
    int32_t frames, vocab, blank, beam_width, top_k, use_lm, first;
    float lm_weight, word_bonus;
    const TopEntry *top;   // the pre-pass' table (ctc_topk_kernel): [workgroup][frame][top_k + 1]
};

__host__ __device__ inline uint64_t mix64(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }

// First slot of a word (h, len) in the unigram table, of a pair (context, word) in the bigram table; probing is linear.  The table builder
// (beam_host.hip) and every prober go through these two: a builder and a prober that disagree make every word of the model unknown.
__host__ __device__ inline uint32_t uni_slot(uint64_t h, int32_t len, uint32_t mask) { return static_cast<uint32_t>(mix64(h + static_cast<uint64_t>(len))) & mask; }
__host__ __device__ inline uint32_t bi_slot(uint64_t hp, int32_t lp, uint64_t hw, int32_t lw, uint32_t mask) {
    return static_cast<uint32_t>(mix64(mix64(hp + static_cast<uint64_t>(lp)) ^ (hw + static_cast<uint64_t>(lw) * 0x9e3779b97f4a7c15ull))) & mask;
}

__host__ __device__ inline bool uni_find(const LmView &lm, uint64_t h, int32_t len, float &logp, float &backoff) {
    if (!lm.uni) return false;
    for (uint32_t s = uni_slot(h, len, lm.uni_mask);; s = (s + 1) & lm.uni_mask) {
        const UniEntry e = lm.uni[s];
        if (!e.used) return false;
        if (e.h == h && e.len == len) { logp = e.logp; backoff = e.backoff; return true; }
    }
}

__host__ __device__ inline bool bi_find(const LmView &lm, uint64_t hp, int32_t lp, uint64_t hw, int32_t lw, float &logp) {
    if (!lm.bi) return false;
    for (uint32_t s = bi_slot(hp, lp, hw, lw, lm.bi_mask);; s = (s + 1) & lm.bi_mask) {
        const BiEntry e = lm.bi[s];
        if (!e.used) return false;
        if (e.hp == hp && e.hw == hw && e.lp == lp && e.lw == lw) { logp = e.logp; return true; }
    }
}

// ARPALanguageModel.score (:98-103); plen < 0 encodes prev == nil
__host__ __device__ inline float lm_score(const LmView &lm, uint64_t hw, int32_t lw, uint64_t hp, int32_t plen) {
    float logp, bo;
    if (plen >= 0 && bi_find(lm, hp, plen, hw, lw, logp)) return logp;
    float backoff = 0.0f;
    if (plen >= 0 && uni_find(lm, hp, plen, logp, bo)) backoff = bo;
    const float uni = uni_find(lm, hw, lw, logp, bo) ? logp : kUnkLogProb;
    return backoff + uni;
}

// the polynomial hash of a word's bytes and the multiplier that appends a word of that length (TokInfo: mult, add)
inline void hash_bytes(const char *s, size_t n, uint64_t &h, uint64_t &mult) {
    h = 0; mult = 1;
    for (size_t i = 0; i < n; ++i) { h = h * kHashBase + static_cast<unsigned char>(s[i]); mult *= kHashBase; }
}

// ctc_topk_kernel<NREG> on the a.rows (utterance, frame) rows of a launch, one wavefront per row.  top_regs: the keys per lane the instance
// for a vocabulary holds in registers (0: the instance that reads the row again in every pass).
int top_regs(int vocab);
void launch_top(hipStream_t stream, const TopArgs &a);
// ctc_beam_kernel<MAXE> on `utterances` workgroups from utterance a.first on.  walk_keys: the extension keys per thread (MAXE) of the instance
// that serves ntop = min(top_k, tokens of the vocabulary other than the blank) top tokens per frame.
int walk_keys(int ntop);
void launch_walk(hipStream_t stream, const BeamArgs &a, int utterances, int ntop);

}  // namespace beam
}  // namespace fa
