// vocab_rescore.hip — the vocabulary rescorer's candidate discovery on the device: the two loops of
// rescoreWithConstrainedCTCTermCentric (Sources/FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/Rescorer/
// VocabularyRescorer+TokenRescoring.swift:755-1033) for every (utterance, term, word start), without the CTC verdict behind them.
// Integer edit distances, one correctly rounded fp32 divide and one subtraction per similarity, strict compares: the records are the
// reference's bit for bit (this unit is built with -ffp-contract=off like the other restatements).
//
// One wavefront takes one (block of word starts, term); the lane is the word start.  A form is a 64-bit pattern and the lane's words are
// the text of the bit-vector recurrence of vocab_rescore_core.h: the score after j text symbols is the distance of the form to the
// text's first j symbols, so ONE pass over the words i, i + 1, i + 2 — they lie back to back — gives the single word and both compounds,
// and one pass with a space between the non-empty words gives the spans 2 ... 4 of the multi-word path.  The form's masks (A < 1024
// dense ids, 8 bytes each) are staged in LDS by the wavefront; lanes diverge only in the length of their text.  The guards (the phrase
// is the canonical form / a form of another term) are integer compares on the sids a pre-pass found by binary search with exact symbol
// compare.  The last two lanes of a wavefront repeat the first two word starts of the next block: they only answer the compound guard of
// the lanes before them ("does word i + 1 / i + 2 match a single-word form at >= 0.9 alone"), through a wave shift.
// Survivors go to a bounded arena behind an atomic cursor; the host sorts them into the reference's order (vocab_rescore_host.hip).
#include "vocab_rescore_launch.h"

namespace fa {
namespace vr {
namespace {

constexpr int kSidThreads = 256;

__global__ __launch_bounds__(kSidThreads) void vr_sids(const WalkArgs a) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kSidThreads + threadIdx.x;
    const int64_t g = t / kMaxSpan;
    const int32_t span = static_cast<int32_t>(t % kMaxSpan) + 1;
    if (g >= a.n_words) return;
    int32_t lo = 0, hi = a.batch;   // the utterance of word g: the last u with utt_words[u] <= g
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (a.utt_words[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t end = a.utt_words[lo + 1];
    int32_t out = -2;
    if (g + span <= end) {
        uint16_t phrase[kMaxForm];
        int32_t len = 0;
        bool fits = true;
        for (int32_t k = 0; k < span; ++k) {
            const int64_t p0 = a.word_off[g + k], p1 = a.word_off[g + k + 1];
            if (p1 == p0) continue;
            if (len > 0) { if (len < kMaxForm) phrase[len] = static_cast<uint16_t>(a.h.space_id); ++len; }
            if (len + (p1 - p0) > kMaxForm) { fits = false; len = kMaxForm + 1; break; }
            for (int64_t p = p0; p < p1; ++p) phrase[len++] = a.syms[p];
        }
        if (len > kMaxForm) fits = false;
        if (len > 0) out = fits ? find_sid(a.blob, a.h, phrase, len) : -1;
    }
    a.sid[g * kMaxSpan + (span - 1)] = out;
}

__global__ __launch_bounds__(kWave) void vr_walk(const WalkArgs a) {
    extern __shared__ uint64_t masks[];   // [A] of the form being walked
    const int lane = threadIdx.x;
    const int64_t job = blockIdx.x;
    const Block blk = a.blocks[job / a.h.n_terms];
    const int32_t t = static_cast<int32_t>(job % a.h.n_terms);
    const Term tm = term_at(a.blob, a.h, t);
    const float term_min = tm.has_min ? tm.min_similarity : a.min_similarity;   // :729

    int32_t min_words = INT32_MAX, max_words = 0, n_single = 0;
    for (int32_t f = 0; f < tm.n_forms; ++f) {
        const int32_t w = form_at(a.blob, a.h, tm.first_form + f).words;
        if (w > 1) { min_words = min(min_words, w); max_words = max(max_words, w); }
        if (w == 1) ++n_single;
    }
    int32_t min_span = 0, max_span = -1;
    if (max_words > 0 && !multi_spans(min_words, max_words, min_span, max_span)) return;   // :762 leaves the term (wave-uniform, before any barrier)

    const int64_t g0 = a.utt_words[blk.utterance];
    const int32_t W = static_cast<int32_t>(a.utt_words[blk.utterance + 1] - g0);
    const int32_t i = blk.first_word + lane;
    const bool in = i < W;
    const bool emits = in && lane < kStarts;
    const int64_t g = g0 + (in ? i : W);
    int64_t o[kMaxSpan + 1];   // the symbols of the words i ... i + 3, clipped to the utterance
#pragma unroll
    for (int k = 0; k <= kMaxSpan; ++k) o[k] = a.word_off[min(g + k, g0 + W)];
    int32_t n[kMaxSpan];
#pragma unroll
    for (int k = 0; k < kMaxSpan; ++k) n[k] = static_cast<int32_t>(o[k + 1] - o[k]);

    const auto emit = [&](const int32_t span, const int32_t origin, const int32_t form, const float sim) {
        const unsigned long long at = atomicAdd(a.cursor, 1ull);
        if (at < static_cast<unsigned long long>(a.arena_cap)) a.arena[at] = fa_vr_candidate{blk.utterance, tm.src, i, span, origin, form, sim};
    };
    const auto stage = [&](const int32_t f) {   // every lane of the wavefront comes here
        __syncthreads();
        for (int32_t c = lane; c < a.h.A; c += kWave) masks[c] = mask_at(a.blob, a.h, f, c);
        __syncthreads();
    };
    // the phrase is the canonical form, or a form of another term (:789-800, :867-877)
    const auto guarded = [&](const int32_t sid) { return sid >= 0 && (sid == tm.canon_sid || !term_has_sid(a.blob, a.h, tm, sid)); };

    if (max_words > 0) {   // :755-855
        int32_t plen[kMaxSpan];   // the phrase of k + 1 words: the non-empty ones joined by one space
        int32_t len = 0;
#pragma unroll
        for (int k = 0; k < kMaxSpan; ++k) {
            if (n[k] > 0) len += n[k] + (len > 0 ? 1 : 0);
            plen[k] = len;
        }
        float best[kMaxSpan] = {0.0f, 0.0f, 0.0f, 0.0f};
        int32_t alias[kMaxSpan] = {-1, -1, -1, -1};
        for (int32_t f = 0; f < tm.n_forms; ++f) {
            const Form fm = form_at(a.blob, a.h, tm.first_form + f);
            if (fm.words <= 1) continue;
            stage(tm.first_form + f);
            BitDp s;
            bitdp_begin(s, fm.len);
            bool any = false;
#pragma unroll
            for (int k = 0; k < kMaxSpan; ++k) {
                if (k + 1 <= max_span && i + k < W) {
                    if (n[k] > 0) {
                        if (any) bitdp_step(s, masks[a.h.space_id]);
                        for (int64_t p = o[k]; p < o[k + 1]; ++p) bitdp_step(s, masks[a.syms[p]]);
                        any = true;
                    }
                    if (k + 1 >= min_span && any) {
                        const float sim = similarity(s.score, plen[k], fm.len);
                        if (sim > best[k]) { best[k] = sim; alias[k] = f; }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 1; k < kMaxSpan; ++k) {
            const int32_t span = k + 1;
            if (!emits || span < min_span || span > max_span || i + span > W || plen[k] == 0) continue;
            if (guarded(a.sid[g * kMaxSpan + k])) continue;
            if (best[k] < required_similarity(term_min, span)) continue;
            emit(span, FA_VR_ORIGIN_MULTI_WORD, alias[k], best[k]);
        }
    }

    if (n_single == 0) return;   // wave-uniform
    // :857-1033
    const bool has2 = i + 1 < W && n[1] > 0, has3 = i + 2 < W && n[2] > 0;
    const bool try2 = has2 && tm.char_count >= kMinCharsFor2Words, try3 = has2 && has3 && tm.char_count >= kMinCharsFor3Words;
    const int64_t text_end = try3 ? o[3] : (try2 ? o[2] : o[1]);
    float m[3] = {0.0f, 0.0f, 0.0f};   // the best similarity of the word and of the compounds of 2 and 3 words, each with its first form
    int32_t al[3] = {-1, -1, -1};
    int alone = 0;                     // the word matches a single-word form at >= 0.9 on its own
    for (int32_t f = 0; f < tm.n_forms; ++f) {
        const Form fm = form_at(a.blob, a.h, tm.first_form + f);
        if (fm.words != 1) continue;
        stage(tm.first_form + f);
        if (in && n[0] > 0) {
            BitDp s;
            bitdp_begin(s, fm.len);
            int32_t d[3] = {fm.len, fm.len, fm.len};
            for (int64_t p = o[0]; p < text_end; ++p) {
                bitdp_step(s, masks[a.syms[p]]);
                if (p + 1 == o[1]) d[0] = s.score;
                if (p + 1 == o[2]) d[1] = s.score;
                if (p + 1 == o[3]) d[2] = s.score;
            }
            const float s1 = similarity(d[0], n[0], fm.len);
            if (s1 > m[0]) { m[0] = s1; al[0] = f; }
            if (s1 >= kCompoundGuard) alone = 1;
            if (try2) {
                const float s2 = similarity(d[1], n[0] + n[1], fm.len);
                if (s2 > m[1]) { m[1] = s2; al[1] = f; }
            }
            if (try3) {
                const float s3 = similarity(d[2], n[0] + n[1] + n[2], fm.len);
                if (s3 > m[2]) { m[2] = s3; al[2] = f; }
            }
        }
    }
    const int alone1 = __shfl_down(alone, 1), alone2 = __shfl_down(alone, 2);   // the words i + 1 and i + 2: lanes of this wavefront for every lane that emits
    if (!emits || n[0] == 0) return;
    if (guarded(a.sid[g * kMaxSpan])) return;
    float best = m[0];
    int32_t span = 1, alias = al[0];
    if (try2 && !alone1 && m[1] > best) { best = m[1]; span = 2; alias = al[1]; }
    if (try3 && !(alone1 || alone2) && m[2] > best) { best = m[2]; span = 3; alias = al[2]; }
    float thr;
    if (!single_threshold(term_min, span, n[0], tm.char_count, a.flags + g, thr)) return;
    if (best < thr) return;
    emit(span, FA_VR_ORIGIN_SINGLE_WORD, alias, best);
}

}  // namespace

void launch_sids(hipStream_t stream, const WalkArgs &a) {
    if (a.n_words <= 0) return;
    hipLaunchKernelGGL(vr_sids, dim3(grid_for(a.n_words * kMaxSpan, kSidThreads)), dim3(kSidThreads), 0, stream, a);
}

void launch_walk(hipStream_t stream, const WalkArgs &a) {
    const int64_t jobs = static_cast<int64_t>(a.n_blocks) * a.h.n_terms;
    if (jobs <= 0) return;
    hipLaunchKernelGGL(vr_walk, dim3(static_cast<unsigned>(jobs)), dim3(kWave), sizeof(uint64_t) * static_cast<size_t>(a.h.A), stream, a);
}

}  // namespace vr
}  // namespace fa
