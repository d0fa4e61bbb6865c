// vocab_rescore_core.h — the vocabulary rescorer's plain C++ (kernels: vocab_rescore.hip, entries: vocab_rescore_host.hip, operands:
// vocab_rescore_launch.h): the vocabulary blob's layout with its checked reader and — host only — its builder, the fp32 similarity and
// threshold arithmetic, the bit-vector step of the edit distance, the frame window, the boost and the arbitration, and the host's
// reference walk of the candidate loops with the plain DP.  tests/cpu/vocab_rescore_core_main.cpp drives all of it under the sanitizers;
// the arithmetic and the reader are __host__ __device__ under hipcc.
//
// Restated from FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/: Rescorer/VocabularyRescorer+TokenRescoring.swift :272-307
// (arbitration) and :723-1033 (the term-centric loops), +TokenEvaluation.swift :37-42 (window), :319-377 (stopword and length-ratio
// rules), +Utilities.swift :8-17 (stringSimilarity), :43-62 (normalizedForms), :87-96 (requiredSimilarity), :321-339 (the normalized
// set), VocabularyRescorer.swift :111-129 (adaptiveCbw), Shared/StringUtils.swift :12-41.  normalizeForSimilarity, the tokenizers and the
// stopword lists are the caller's: a word or a form is a row of int32 symbols, one per Character, FA_VR_SPACE for the space.
//
// THE BLOB: int32 words, position independent (every reference is an index into one of its sections).
//   [0] magic  [1] version  [2] total words  [3] n_terms  [4] off_terms  [5] n_forms  [6] off_forms  [7] n_strings  [8] off_strings
//   [9] n_string_syms  [10] off_string_syms  [11] A  [12] off_alphabet  [13] off_masks  [14] space id  [15] input terms  [16 ... 23] 0
//   terms        [n_terms][8]     input index, char_count, min_similarity bits, has a min_similarity, first form, form count, canonical sid
//                                 (-1: the canonical form is empty), 0.  Only the terms that are kept, in file order.
//   forms        [n_forms][4]     sid, symbols, words, 0.  A term's kept forms in buildNormalizedForms' order.
//   strings      [n_strings][2]   first symbol, symbols: the vocabulary's normalized set — every distinct non-empty form of every input term,
//                                 kept or not — ascending (symbol by symbol as dense ids, a prefix before its extensions); sid = the index
//   string syms  [n_string_syms]  dense ids
//   alphabet     [A - 1]          the symbols that occur in a form, ascending: dense id = index + 1; id 0 is every other symbol and matches nothing
//   masks        [n_forms][A][2]  per form and dense id the 64-bit set of the form's positions that hold it, low word first
// validate() checks every offset, count and index of a blob once; the readers below take a blob that passed it.
#pragma once
#include <cstdint>

#include "../../include/fluidaudio_hip.h"

#if defined(__HIPCC__)
#define FA_VR_HD __host__ __device__
#else
#define FA_VR_HD
#endif

namespace fa {
namespace vr {

constexpr int32_t kMagic = 0x52564146;   // "FAVR"
constexpr int32_t kVersion = 1;
constexpr int32_t kHeaderWords = 24;
constexpr int32_t kTermWords = 8, kFormWords = 4, kStringWords = 2;
constexpr int32_t kMaxForm = FA_VR_MAX_FORM;            // a form is one 64-bit pattern
constexpr int32_t kMaxAlphabet = FA_VR_MAX_ALPHABET;    // A < 1024: a form's masks are at most 8 KB of LDS
constexpr int32_t kMaxSpan = 4;

struct Header {
    int32_t total, n_terms, off_terms, n_forms, off_forms, n_strings, off_strings, n_string_syms, off_string_syms, A, off_alphabet, off_masks, space_id,
        input_terms;
};

struct Term { int32_t src, char_count; float min_similarity; int32_t has_min, first_form, n_forms, canon_sid; };
struct Form { int32_t sid, len, words; };

FA_VR_HD inline bool section_ok(const int64_t off, const int64_t count, const int64_t per, const int64_t words) {
    return off >= kHeaderWords && count >= 0 && count <= words && off <= words && off + count * per <= words;
}

FA_VR_HD inline float bits_float(const int32_t i) { union { int32_t i; float f; } u; u.i = i; return u.f; }
FA_VR_HD inline int32_t float_bits(const float f) { union { int32_t i; float f; } u; u.f = f; return u.i; }

// the header of blob[words]: false for no header, another magic or version, or a section that leaves the blob
FA_VR_HD inline bool read_header(const int32_t *blob, const int64_t words, Header &h) {
    if (!blob || words < kHeaderWords || blob[0] != kMagic || blob[1] != kVersion) return false;
    h.total = blob[2]; h.n_terms = blob[3]; h.off_terms = blob[4]; h.n_forms = blob[5]; h.off_forms = blob[6]; h.n_strings = blob[7]; h.off_strings = blob[8];
    h.n_string_syms = blob[9]; h.off_string_syms = blob[10]; h.A = blob[11]; h.off_alphabet = blob[12]; h.off_masks = blob[13]; h.space_id = blob[14];
    h.input_terms = blob[15];
    if (h.total < kHeaderWords || h.total > words) return false;
    const int64_t w = h.total;
    if (h.A < 1 || h.A >= kMaxAlphabet || h.space_id < 0 || h.space_id >= h.A || h.input_terms < 0) return false;
    return section_ok(h.off_terms, h.n_terms, kTermWords, w) && section_ok(h.off_forms, h.n_forms, kFormWords, w) &&
           section_ok(h.off_strings, h.n_strings, kStringWords, w) && section_ok(h.off_string_syms, h.n_string_syms, 1, w) &&
           section_ok(h.off_alphabet, h.A - 1, 1, w) && section_ok(h.off_masks, static_cast<int64_t>(h.n_forms) * h.A, 2, w);
}

// ---- readers of a validated blob
FA_VR_HD inline Term term_at(const int32_t *blob, const Header &h, const int32_t t) {
    const int32_t *r = blob + h.off_terms + static_cast<int64_t>(t) * kTermWords;
    return Term{r[0], r[1], bits_float(r[2]), r[3], r[4], r[5], r[6]};
}
FA_VR_HD inline Form form_at(const int32_t *blob, const Header &h, const int32_t f) {
    const int32_t *r = blob + h.off_forms + static_cast<int64_t>(f) * kFormWords;
    return Form{r[0], r[1], r[2]};
}
FA_VR_HD inline const int32_t *string_at(const int32_t *blob, const Header &h, const int32_t sid, int32_t &len) {
    const int32_t *r = blob + h.off_strings + static_cast<int64_t>(sid) * kStringWords;
    len = r[1];
    return blob + h.off_string_syms + r[0];
}
FA_VR_HD inline uint64_t mask_at(const int32_t *blob, const Header &h, const int32_t form, const int32_t id) {
    const int32_t *r = blob + h.off_masks + 2 * (static_cast<int64_t>(form) * h.A + id);
    return static_cast<uint64_t>(static_cast<uint32_t>(r[0])) | (static_cast<uint64_t>(static_cast<uint32_t>(r[1])) << 32);
}
// the dense id of a caller's symbol: 1 ... A - 1, or 0 for a symbol no form holds
FA_VR_HD inline int32_t dense_id(const int32_t *blob, const Header &h, const int32_t symbol) {
    const int32_t *keys = blob + h.off_alphabet;
    int32_t lo = 0, hi = h.A - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] == symbol) return mid + 1;
        if (keys[mid] < symbol) lo = mid + 1; else hi = mid;
    }
    return 0;
}
// The sid of a phrase of dense ids: its index in the sorted string table, or -1.  Exact symbol compare; a phrase longer than a form can be
// is in no table.
template <class Sym>
FA_VR_HD inline int32_t find_sid(const int32_t *blob, const Header &h, const Sym *phrase, const int32_t len) {
    if (len < 1 || len > kMaxForm) return -1;
    int32_t lo = 0, hi = h.n_strings;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        int32_t n;
        const int32_t *s = string_at(blob, h, mid, n);
        int cmp = 0;   // the string against the phrase
        for (int32_t i = 0; i < n && i < len && cmp == 0; ++i) cmp = s[i] < static_cast<int32_t>(phrase[i]) ? -1 : (s[i] > static_cast<int32_t>(phrase[i]) ? 1 : 0);
        if (cmp == 0) cmp = n < len ? -1 : (n > len ? 1 : 0);
        if (cmp == 0) return mid;
        if (cmp < 0) lo = mid + 1; else hi = mid;
    }
    return -1;
}
// normalizedCurrentSet.contains: the sid among the term's forms
FA_VR_HD inline bool term_has_sid(const int32_t *blob, const Header &h, const Term &t, const int32_t sid) {
    for (int32_t f = 0; f < t.n_forms; ++f)
        if (form_at(blob, h, t.first_form + f).sid == sid) return true;
    return false;
}

// ---- the fp32 arithmetic
FA_VR_HD inline float max_f(const float a, const float b) { return b >= a ? b : a; }
// stringSimilarity (+Utilities.swift:8-17): one correctly rounded divide, one subtraction
FA_VR_HD inline float similarity(const int32_t distance, const int32_t len_a, const int32_t len_b) {
    const int32_t longest = len_a > len_b ? len_a : len_b;
    if (longest <= 0) return 1.0f;
    return 1.0f - static_cast<float>(distance) / static_cast<float>(longest);
}
FA_VR_HD inline float required_similarity(const float min_similarity, const int32_t span) {   // :87-96
    return span >= 2 ? max_f(min_similarity, 0.55f) : min_similarity;
}
FA_VR_HD inline float length_ratio_rule(const int32_t word_len, const int32_t char_count, const float min_similarity) {   // +TokenEvaluation.swift:357-377
    const float ratio = static_cast<float>(word_len) / static_cast<float>(char_count);
    return (ratio < 0.75f && word_len <= 4) ? max_f(min_similarity, 0.8f) : min_similarity;
}
constexpr float kStopwordSpanSimilarity = 0.85f, kCompoundGuard = 0.9f;
constexpr int32_t kMinCharsFor2Words = 4, kMinCharsFor3Words = 8;

// The threshold of the single-word path behind the match (:949-980): false when the stopword rule drops the word.  flags: the span's
// words, bit 0 stopwords, bit 1 multiWordStopwords.
FA_VR_HD inline bool single_threshold(const float term_min, const int32_t span, const int32_t word_len, const int32_t char_count, const uint8_t *flags, float &thr) {
    thr = required_similarity(term_min, span);
    if (span == 1) thr = length_ratio_rule(word_len, char_count, thr);
    if (span == 1 && (flags[0] & 1)) return false;
    if (span >= 2) {
        bool any = false;
        for (int32_t k = 0; k < span; ++k) any = any || (flags[k] & 2);
        if (any) thr = max_f(thr, kStopwordSpanSimilarity);
    }
    return true;
}

// The spans of the multi-word path of a term (:757-762): false when it has none — the reference then leaves the TERM, its single-word forms
// included (the `continue` of :762).
FA_VR_HD inline bool multi_spans(const int32_t min_words, const int32_t max_words, int32_t &min_span, int32_t &max_span) {
    max_span = max_words + 1 < kMaxSpan ? max_words + 1 : kMaxSpan;
    min_span = min_words > 2 ? min_words : 2;
    return min_span <= max_span;
}

// ---- the bit-vector step (Myers 1999 as Hyyro's global variant): the form is the pattern of m <= 64 symbols, `eq` the mask of the
// text's next symbol.  After j steps `score` is the Levenshtein distance of the form to the text's first j symbols.
struct BitDp {
    uint64_t pv, mv, last;
    int32_t score;
};
FA_VR_HD inline void bitdp_begin(BitDp &s, const int32_t m) { s.pv = ~uint64_t{0}; s.mv = 0; s.last = uint64_t{1} << (m - 1); s.score = m; }
FA_VR_HD inline void bitdp_step(BitDp &s, const uint64_t eq) {
    const uint64_t xv = eq | s.mv;
    const uint64_t xh = (((eq & s.pv) + s.pv) ^ s.pv) | eq;
    uint64_t ph = s.mv | ~(xh | s.pv);
    uint64_t mh = s.pv & xh;
    if (ph & s.last) ++s.score;
    else if (mh & s.last) --s.score;
    ph = (ph << 1) | 1;   // the global distance: row 0 grows by one per text symbol
    mh <<= 1;
    s.pv = mh | ~(xv | ph);
    s.mv = ph & xv;
}

// ---- the frame window (+TokenEvaluation.swift:37-42): fp64 quotients truncated like Int(_:), clamped to [0, valid].  false where Int(_:)
// would trap (a quotient that is not finite or leaves the integers).
FA_VR_HD inline bool frame_window(const double start_time, const double end_time, const double frame_duration, const double margin_seconds, const int32_t valid,
                                  int32_t &start, int32_t &end) {
    const double q[3] = {margin_seconds / frame_duration, start_time / frame_duration, end_time / frame_duration};
    int64_t v[3];
    for (int i = 0; i < 3; ++i) {
        if (!(q[i] > -4.0e18 && q[i] < 4.0e18)) return false;   // NaN fails both
        v[i] = static_cast<int64_t>(q[i]);
    }
    int64_t a = v[1] - v[0], b = v[2] + v[0];
    a = a < 0 ? 0 : a;
    b = b > valid ? valid : b;
    start = static_cast<int32_t>(a > valid ? valid : a);
    end = static_cast<int32_t>(b < 0 ? 0 : b);
    return true;
}

}  // namespace vr
}  // namespace fa

// ---- host only: the plain DP, the boost, the arbitration, the builder, the validation and the reference walk
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "fa_verdict.h"

namespace fa {
namespace vr {

// StringUtils.levenshteinDistance (:12-41) with two rows
template <class SymA, class SymB>
inline int32_t levenshtein(const SymA *a, const int32_t m, const SymB *b, const int32_t n) {
    if (m <= 0) return n;
    if (n <= 0) return m;
    std::vector<int32_t> prev(static_cast<size_t>(n) + 1), cur(static_cast<size_t>(n) + 1);
    for (int32_t j = 0; j <= n; ++j) prev[j] = j;
    for (int32_t i = 1; i <= m; ++i) {
        cur[0] = i;
        for (int32_t j = 1; j <= n; ++j) {
            const int32_t cost = static_cast<int64_t>(a[i - 1]) == static_cast<int64_t>(b[j - 1]) ? 0 : 1;
            cur[j] = std::min(std::min(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + cost);
        }
        prev.swap(cur);
    }
    return prev[n];
}

// adaptiveCbw (VocabularyRescorer.swift:111-129).  log2 and pow are evaluated in fp64 and rounded once to fp32: the library's definition
// of the two libm calls, the same on every host; everything round them is the reference's fp32 arithmetic.
inline float boost(const float cbw, const int32_t tokens, const fa_vr_boost_config &c) {
    if (!c.use_adaptive_thresholds) return cbw;
    if (c.short_term_taper_pivot > 1 && tokens < c.short_term_taper_pivot) {
        const float ratio = static_cast<float>(std::max(1, tokens)) / static_cast<float>(c.short_term_taper_pivot);
        return cbw * static_cast<float>(std::pow(static_cast<double>(ratio), static_cast<double>(c.short_term_taper_exponent)));
    }
    if (!(tokens > c.reference_token_count)) return cbw;
    const float ratio = static_cast<float>(tokens) / static_cast<float>(c.reference_token_count);
    const float l = static_cast<float>(std::log2(static_cast<double>(ratio)));
    const float scaled = l * 0.3f;
    const float grown = 1.0f + scaled;
    return cbw * grown;
}

// the bucket of arbitratePendingReplacements (:276): Int((sim / 0.05).rounded()) in fp32, halves away from zero
inline int32_t bucket(const float similarity) { return static_cast<int32_t>(std::round(similarity / 0.05f)); }
inline bool bucket_ok(const float similarity) { return std::isfinite(similarity) && std::fabs(similarity) <= 1.0e6f; }

// arbitratePendingReplacements (:272-307) over the pending replacements of one utterance, given in candidate order: the order is bucket
// descending, span ascending, similarity descending, ties in candidate order (a stable sort: this library's definition); then the greedy
// pass over the word indices.  occupied[words] is read and extended.  applied: indices into the arrays in application order;
// superseded[i] set for the others.
inline void arbitrate(const int32_t n, const float *similarity, const int32_t *first_word, const int32_t *span, uint8_t *occupied, std::vector<int32_t> &applied,
                      std::vector<uint8_t> &superseded) {
    std::vector<int32_t> order(static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](const int32_t a, const int32_t b) {
        const int32_t qa = bucket(similarity[a]), qb = bucket(similarity[b]);
        if (qa != qb) return qa > qb;
        if (span[a] != span[b]) return span[a] < span[b];
        return similarity[a] > similarity[b];
    });
    applied.clear();
    superseded.assign(static_cast<size_t>(n), 0);
    for (const int32_t i : order) {
        bool free_span = true;
        for (int32_t k = 0; k < span[i]; ++k) free_span = free_span && !occupied[first_word[i] + k];
        if (!free_span) { superseded[i] = 1; continue; }
        applied.push_back(i);
        for (int32_t k = 0; k < span[i]; ++k) occupied[first_word[i] + k] = 1;
    }
}

typedef std::vector<int32_t> Symbols;

// fa_vocab_rescore_build without the context: term t has the rows [term_rows[t], term_rows[t + 1]) of the ragged symbol table, its
// canonical form first (possibly empty), then its aliases in buildNormalizedForms' order.
inline Verdict build(const int32_t *char_counts, const float *min_similarities, const int64_t *term_rows, const int64_t *row_offsets, const int32_t *symbols,
                     const int32_t terms, const int32_t min_term_length, int32_t *blob, const int64_t capacity_words, int64_t *words_needed) {
    if (words_needed) *words_needed = 0;
    if (!words_needed || terms < 0 || capacity_words < 0 || (capacity_words > 0 && !blob)) return refuse(FA_INVALID_ARGUMENT, "words_needed is required, sizes >= 0, a blob with a capacity");
    if (terms > 0 && (!char_counts || !term_rows)) return refuse(FA_INVALID_ARGUMENT, "char_counts and term_rows are required");
    if (terms > 0 && term_rows[0] < 0) return refuse(FA_INVALID_ARGUMENT, "term_rows starts below 0");
    for (int32_t t = 0; t < terms; ++t)
        if (term_rows[t + 1] < term_rows[t]) return refuse(FA_INVALID_ARGUMENT, "term_rows does not ascend at term %d", t);
    const int64_t r0 = terms > 0 ? term_rows[0] : 0, r1 = terms > 0 ? term_rows[terms] : 0;
    if (r1 > r0 && !row_offsets) return refuse(FA_INVALID_ARGUMENT, "row_offsets is required");
    if (r1 - r0 > INT32_MAX / 8) return refuse(FA_INVALID_ARGUMENT, "too many forms");
    if (r1 > r0 && row_offsets[r0] < 0) return refuse(FA_INVALID_ARGUMENT, "row_offsets starts below 0");
    for (int64_t r = r0; r < r1; ++r)
        if (row_offsets[r + 1] < row_offsets[r]) return refuse(FA_INVALID_ARGUMENT, "row_offsets does not ascend at row %lld", (long long)r);
    if (r1 > r0 && row_offsets[r1] > row_offsets[r0] && !symbols) return refuse(FA_INVALID_ARGUMENT, "symbols is required");
    for (int32_t t = 0; t < terms; ++t) {
        if (min_similarities && min_similarities[t] != min_similarities[t]) return refuse(FA_INVALID_ARGUMENT, "term %d: min_similarity is not a number", t);
        for (int64_t r = term_rows[t]; r < term_rows[t + 1]; ++r)
            if (row_offsets[r + 1] - row_offsets[r] > kMaxForm)
                return refuse(FA_INVALID_ARGUMENT, "term %d form %lld has %lld symbols, at most %d are supported", t, (long long)(r - term_rows[t]),
                              (long long)(row_offsets[r + 1] - row_offsets[r]), kMaxForm);
    }
    // the alphabet and the normalized set, over every non-empty form of every input term
    std::map<int32_t, int32_t> alphabet;
    for (int64_t r = r0; r < r1; ++r)
        for (int64_t i = row_offsets[r]; i < row_offsets[r + 1]; ++i) alphabet[symbols[i]] = 0;
    const int64_t A = static_cast<int64_t>(alphabet.size()) + 1;
    if (A >= kMaxAlphabet) return refuse(FA_INVALID_ARGUMENT, "the forms use %lld distinct symbols, at most %d are supported", (long long)(A - 1), kMaxAlphabet - 2);
    int32_t next = 0;
    for (auto &kv : alphabet) kv.second = ++next;   // (a map: ascending symbols)
    std::map<Symbols, int32_t> strings;
    auto dense_row = [&](const int64_t r) {
        Symbols s;
        for (int64_t i = row_offsets[r]; i < row_offsets[r + 1]; ++i) s.push_back(alphabet[symbols[i]]);
        return s;
    };
    for (int64_t r = r0; r < r1; ++r)
        if (row_offsets[r + 1] > row_offsets[r]) strings[dense_row(r)] = 0;
    next = 0;
    for (auto &kv : strings) kv.second = next++;    // (a map: ascending strings, a prefix before its extensions)
    const auto space = alphabet.find(FA_VR_SPACE);
    const int32_t space_id = space == alphabet.end() ? 0 : space->second;

    std::vector<int32_t> term_words, form_words, mask_words;
    std::vector<Symbols> kept_forms;
    for (int32_t t = 0; t < terms; ++t) {
        if (char_counts[t] < min_term_length) continue;                                  // :732
        std::vector<int32_t> sids;
        for (int64_t r = term_rows[t]; r < term_rows[t + 1]; ++r) {                      // normalizedForms (:43-62)
            if (row_offsets[r + 1] == row_offsets[r]) continue;
            const int32_t sid = strings[dense_row(r)];
            if (std::find(sids.begin(), sids.end(), sid) == sids.end()) sids.push_back(sid);
        }
        if (sids.empty()) continue;                                                      // :746
        const int64_t first = term_rows[t];
        const bool has_canon = term_rows[t + 1] > first && row_offsets[first + 1] > row_offsets[first];
        const bool has_min = min_similarities && min_similarities[t] >= 0.0f;
        const int32_t rec[kTermWords] = {t, char_counts[t], float_bits(has_min ? min_similarities[t] : 0.0f), has_min ? 1 : 0, static_cast<int32_t>(kept_forms.size()),
                                         static_cast<int32_t>(sids.size()), has_canon ? strings[dense_row(first)] : -1, 0};
        term_words.insert(term_words.end(), rec, rec + kTermWords);
        for (const int32_t sid : sids) {
            auto it = strings.begin();
            std::advance(it, sid);
            const Symbols &s = it->first;
            int32_t words = 0;
            for (size_t i = 0; i < s.size(); ++i)
                if (s[i] != space_id && (i == 0 || s[i - 1] == space_id)) ++words;         // split(separator: " "): the non-empty runs
            const int32_t frec[kFormWords] = {sid, static_cast<int32_t>(s.size()), words, 0};
            form_words.insert(form_words.end(), frec, frec + kFormWords);
            kept_forms.push_back(s);
        }
    }
    for (const Symbols &s : kept_forms) {
        std::vector<uint64_t> masks(static_cast<size_t>(A), 0);
        for (size_t i = 0; i < s.size(); ++i) masks[s[i]] |= uint64_t{1} << i;
        for (const uint64_t m : masks) { mask_words.push_back(static_cast<int32_t>(static_cast<uint32_t>(m))); mask_words.push_back(static_cast<int32_t>(static_cast<uint32_t>(m >> 32))); }
    }
    std::vector<int32_t> string_words, string_syms, alphabet_words;
    for (const auto &kv : strings) {
        string_words.push_back(static_cast<int32_t>(string_syms.size()));
        string_words.push_back(static_cast<int32_t>(kv.first.size()));
        string_syms.insert(string_syms.end(), kv.first.begin(), kv.first.end());
    }
    for (const auto &kv : alphabet) alphabet_words.push_back(kv.first);
    const int64_t total = static_cast<int64_t>(kHeaderWords) + static_cast<int64_t>(term_words.size()) + static_cast<int64_t>(form_words.size()) +
                          static_cast<int64_t>(string_words.size()) + static_cast<int64_t>(string_syms.size()) + static_cast<int64_t>(alphabet_words.size()) +
                          static_cast<int64_t>(mask_words.size());
    if (total > INT32_MAX) return refuse(FA_INVALID_ARGUMENT, "the blob would have %lld words", (long long)total);
    *words_needed = total;
    if (capacity_words == 0) return Verdict{};
    if (capacity_words < total) return refuse(FA_OUTPUT_TOO_SMALL, "the blob needs %lld words, the buffer holds %lld", (long long)total, (long long)capacity_words);
    int32_t at = kHeaderWords;
    auto put = [&](const std::vector<int32_t> &v) { const int32_t off = at; std::copy(v.begin(), v.end(), blob + at); at += static_cast<int32_t>(v.size()); return off; };
    std::fill(blob, blob + kHeaderWords, 0);
    blob[0] = kMagic; blob[1] = kVersion; blob[2] = static_cast<int32_t>(total);
    blob[3] = static_cast<int32_t>(term_words.size() / kTermWords); blob[4] = put(term_words);
    blob[5] = static_cast<int32_t>(kept_forms.size()); blob[6] = put(form_words);
    blob[7] = static_cast<int32_t>(strings.size()); blob[8] = put(string_words);
    blob[9] = static_cast<int32_t>(string_syms.size()); blob[10] = put(string_syms);
    blob[11] = static_cast<int32_t>(A); blob[12] = put(alphabet_words);
    blob[13] = put(mask_words); blob[14] = space_id; blob[15] = terms;
    return Verdict{};
}

// Everything a reader or a kernel will index with, checked once; `h` is filled for a blob that passes.
inline Verdict validate(const int32_t *blob, const int64_t words, Header &h) {
    if (!read_header(blob, words, h)) return refuse(FA_INVALID_ARGUMENT, "not a vocabulary blob, or a section leaves it");
    for (int32_t s = 0; s < h.n_strings; ++s) {
        const int32_t *r = blob + h.off_strings + static_cast<int64_t>(s) * kStringWords;
        if (r[0] < 0 || r[1] < 1 || r[1] > kMaxForm || static_cast<int64_t>(r[0]) + r[1] > h.n_string_syms) return refuse(FA_INVALID_ARGUMENT, "blob: string %d leaves its section", s);
    }
    for (int32_t i = 0; i < h.n_string_syms; ++i) {
        const int32_t v = blob[h.off_string_syms + static_cast<int64_t>(i)];
        if (v < 1 || v >= h.A) return refuse(FA_INVALID_ARGUMENT, "blob: symbol %d is outside the alphabet", i);
    }
    for (int32_t i = 1; i + 1 < h.A; ++i)
        if (blob[h.off_alphabet + static_cast<int64_t>(i)] <= blob[h.off_alphabet + static_cast<int64_t>(i) - 1]) return refuse(FA_INVALID_ARGUMENT, "blob: the alphabet does not ascend");
    for (int32_t f = 0; f < h.n_forms; ++f) {
        const Form fm = form_at(blob, h, f);
        if (fm.sid < 0 || fm.sid >= h.n_strings || fm.words < 0 || fm.words > kMaxForm) return refuse(FA_INVALID_ARGUMENT, "blob: form %d names string %d", f, fm.sid);
        int32_t n;
        string_at(blob, h, fm.sid, n);
        if (n != fm.len) return refuse(FA_INVALID_ARGUMENT, "blob: form %d has %d symbols, its string %d", f, fm.len, n);
    }
    for (int32_t t = 0; t < h.n_terms; ++t) {
        const Term tm = term_at(blob, h, t);
        if (tm.src < 0 || tm.src >= h.input_terms || tm.first_form < 0 || tm.n_forms < 1 || static_cast<int64_t>(tm.first_form) + tm.n_forms > h.n_forms ||
            tm.canon_sid < -1 || tm.canon_sid >= h.n_strings || tm.min_similarity != tm.min_similarity)
            return refuse(FA_INVALID_ARGUMENT, "blob: term %d leaves its sections", t);
    }
    return Verdict{};
}

// ---- the words of a call, as dense ids: utterance u has the words [utt_words[u], utt_words[u + 1]), word w the symbols
// [word_off[w], word_off[w + 1]) — back to back in word order — and the flag byte flags[w]
struct Words {
    int32_t batch = 0;
    std::vector<int64_t> utt_words;     // [batch + 1], from 0
    std::vector<int64_t> word_off;      // [words + 1], from 0
    std::vector<uint16_t> syms;         // dense ids
    std::vector<uint8_t> flags;
    int64_t n_words() const { return static_cast<int64_t>(word_off.size()) - 1; }
};

inline Verdict check_words(const int32_t *blob, const Header &h, const int64_t *utterance_offsets, const int32_t batch, const int64_t *word_offsets, const int32_t *symbols,
                           const uint8_t *flags, const float min_similarity, Words &w) {
    if (batch < 0) return refuse(FA_INVALID_ARGUMENT, "negative batch");
    if (min_similarity != min_similarity) return refuse(FA_INVALID_ARGUMENT, "min_similarity is not a number");
    if (batch > 0 && !utterance_offsets) return refuse(FA_INVALID_ARGUMENT, "utterance_offsets is required");
    w.batch = batch;
    w.utt_words.assign(static_cast<size_t>(batch) + 1, 0);
    if (batch > 0 && utterance_offsets[0] < 0) return refuse(FA_INVALID_ARGUMENT, "utterance_offsets starts below 0");
    for (int32_t u = 0; u < batch; ++u) {
        if (utterance_offsets[u + 1] < utterance_offsets[u]) return refuse(FA_INVALID_ARGUMENT, "utterance_offsets does not ascend at utterance %d", u);
        w.utt_words[u + 1] = utterance_offsets[u + 1] - utterance_offsets[0];
    }
    const int64_t n = w.utt_words[batch];
    if (n >= INT32_MAX / 8) return refuse(FA_INDEX_OVERFLOW, "2^28 words or more");
    if (n > 0 && (!word_offsets || !flags)) return refuse(FA_INVALID_ARGUMENT, "word_offsets and word_flags are required");
    const int64_t w0 = batch > 0 ? utterance_offsets[0] : 0;
    w.word_off.assign(static_cast<size_t>(n) + 1, 0);
    w.flags.assign(flags ? flags + w0 : nullptr, flags ? flags + w0 + n : nullptr);
    if (n > 0 && word_offsets[w0] < 0) return refuse(FA_INVALID_ARGUMENT, "word_offsets starts below 0");
    for (int64_t i = 0; i < n; ++i) {
        if (word_offsets[w0 + i + 1] < word_offsets[w0 + i]) return refuse(FA_INVALID_ARGUMENT, "word_offsets does not ascend at word %lld", (long long)i);
        w.word_off[i + 1] = word_offsets[w0 + i + 1] - word_offsets[w0];
    }
    if (w.word_off[n] >= INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "2^31 symbols or more");
    if (w.word_off[n] > 0 && !symbols) return refuse(FA_INVALID_ARGUMENT, "word_symbols is required");
    w.syms.resize(static_cast<size_t>(w.word_off[n]));
    const int32_t *src = n > 0 ? symbols + word_offsets[w0] : symbols;
    for (int64_t i = 0; i < w.word_off[n]; ++i) w.syms[i] = static_cast<uint16_t>(dense_id(blob, h, src[i]));
    return Verdict{};
}

// The phrase of `span` words from word g (global index) of its utterance: the non-empty words joined by the space id (multi: what
// normalizeForSimilarity makes of the joined words) or by nothing (the compounds of the single-word path).
inline void phrase_of(const Words &w, const int64_t g, const int32_t span, const bool spaced, const int32_t space_id, std::vector<uint16_t> &out) {
    out.clear();
    for (int32_t k = 0; k < span; ++k) {
        const int64_t a = w.word_off[g + k], b = w.word_off[g + k + 1];
        if (b > a && spaced && !out.empty()) out.push_back(static_cast<uint16_t>(space_id));
        out.insert(out.end(), w.syms.begin() + a, w.syms.begin() + b);
    }
}

// The host's reference walk: the two loops of :755-1033 with the plain DP, one (utterance, term) after the other.  The records come in
// the reference's append order.
inline void walk_candidates(const int32_t *blob, const Header &h, const Words &w, const float min_similarity, std::vector<fa_vr_candidate> &out) {
    std::vector<uint16_t> phrase, other;
    auto sim_to = [&](const Form &fm, const std::vector<uint16_t> &text) {
        int32_t n;
        const int32_t *s = string_at(blob, h, fm.sid, n);
        return similarity(levenshtein(text.data(), static_cast<int32_t>(text.size()), s, n), static_cast<int32_t>(text.size()), n);
    };
    for (int32_t u = 0; u < w.batch; ++u) {
        const int64_t g0 = w.utt_words[u];
        const int32_t W = static_cast<int32_t>(w.utt_words[u + 1] - g0);
        for (int32_t t = 0; t < h.n_terms; ++t) {
            const Term tm = term_at(blob, h, t);
            const float term_min = tm.has_min ? tm.min_similarity : min_similarity;   // :729
            int32_t min_words = INT32_MAX, max_words = 0, n_single = 0;
            for (int32_t f = 0; f < tm.n_forms; ++f) {
                const Form fm = form_at(blob, h, tm.first_form + f);
                if (fm.words > 1) { min_words = std::min(min_words, fm.words); max_words = std::max(max_words, fm.words); }
                if (fm.words == 1) ++n_single;
            }
            if (max_words > 0) {                                                       // :755-855
                int32_t min_span, max_span;
                if (!multi_spans(min_words, max_words, min_span, max_span)) continue;  // :762 leaves the term
                for (int32_t span = min_span; span <= max_span; ++span) {
                    if (span > W) break;
                    for (int32_t i = 0; i + span <= W; ++i) {
                        phrase_of(w, g0 + i, span, true, h.space_id, phrase);
                        if (phrase.empty()) continue;
                        float best = 0.0f;
                        int32_t alias = -1;
                        for (int32_t f = 0; f < tm.n_forms; ++f) {
                            const Form fm = form_at(blob, h, tm.first_form + f);
                            if (fm.words <= 1) continue;
                            const float s = sim_to(fm, phrase);
                            if (s > best) { best = s; alias = f; }
                        }
                        const int32_t sid = find_sid(blob, h, phrase.data(), static_cast<int32_t>(phrase.size()));
                        if (sid >= 0 && sid == tm.canon_sid) continue;
                        if (sid >= 0 && !term_has_sid(blob, h, tm, sid)) continue;
                        if (best < required_similarity(term_min, span)) continue;
                        out.push_back(fa_vr_candidate{u, tm.src, i, span, FA_VR_ORIGIN_MULTI_WORD, alias, best});
                    }
                }
            }
            if (n_single == 0) continue;
            for (int32_t i = 0; i < W; ++i) {                                          // :857-1033
                phrase_of(w, g0 + i, 1, false, 0, phrase);
                if (phrase.empty()) continue;
                const int32_t n1 = static_cast<int32_t>(phrase.size());
                const int32_t sid = find_sid(blob, h, phrase.data(), n1);
                if (sid >= 0 && sid == tm.canon_sid) continue;
                if (sid >= 0 && !term_has_sid(blob, h, tm, sid)) continue;
                float best = 0.0f;
                int32_t span = 1, alias = -1;
                auto over_forms = [&](const std::vector<uint16_t> &text, const int32_t as_span) {
                    for (int32_t f = 0; f < tm.n_forms; ++f) {
                        const Form fm = form_at(blob, h, tm.first_form + f);
                        if (fm.words != 1) continue;
                        const float s = sim_to(fm, text);
                        if (s > best) { best = s; span = as_span; alias = f; }
                    }
                };
                auto matches_alone = [&](const int64_t g) {
                    phrase_of(w, g, 1, false, 0, other);
                    for (int32_t f = 0; f < tm.n_forms; ++f) {
                        const Form fm = form_at(blob, h, tm.first_form + f);
                        if (fm.words == 1 && sim_to(fm, other) >= kCompoundGuard) return true;
                    }
                    return false;
                };
                over_forms(phrase, 1);
                const bool has2 = i + 1 < W && w.word_off[g0 + i + 2] > w.word_off[g0 + i + 1];
                const bool has3 = i + 2 < W && w.word_off[g0 + i + 3] > w.word_off[g0 + i + 2];
                if (has2 && tm.char_count >= kMinCharsFor2Words && !matches_alone(g0 + i + 1)) {
                    phrase_of(w, g0 + i, 2, false, 0, phrase);
                    over_forms(phrase, 2);
                }
                if (has2 && has3 && tm.char_count >= kMinCharsFor3Words && !(matches_alone(g0 + i + 1) || matches_alone(g0 + i + 2))) {
                    phrase_of(w, g0 + i, 3, false, 0, phrase);
                    over_forms(phrase, 3);
                }
                float thr;
                if (!single_threshold(term_min, span, n1, tm.char_count, w.flags.data() + g0 + i, thr)) continue;
                if (best < thr) continue;
                out.push_back(fa_vr_candidate{u, tm.src, i, span, FA_VR_ORIGIN_SINGLE_WORD, alias, best});
            }
        }
    }
}

// the order of the records: utterance, term, multi-word before single-word, multi-word by span length then start, single-word by word
inline bool candidate_before(const fa_vr_candidate &a, const fa_vr_candidate &b) {
    if (a.utterance != b.utterance) return a.utterance < b.utterance;
    if (a.term != b.term) return a.term < b.term;
    if (a.origin != b.origin) return a.origin < b.origin;
    if (a.origin == FA_VR_ORIGIN_MULTI_WORD && a.span_len != b.span_len) return a.span_len < b.span_len;
    return a.first_word < b.first_word;
}

// The delivery of fa_ctc_kws_spot_batch's capacity contract: *count and the utterance counts are whole, min(total, capacity) records are written.
inline Verdict deliver(const std::vector<fa_vr_candidate> &recs, const int32_t batch, fa_vr_candidate *out, const int64_t capacity, int64_t *count, int64_t *utt_counts) {
    const int64_t total = static_cast<int64_t>(recs.size());
    *count = total;
    if (utt_counts)
        for (const fa_vr_candidate &r : recs)
            if (r.utterance >= 0 && r.utterance < batch) ++utt_counts[r.utterance];
    if (out) std::copy(recs.begin(), recs.begin() + std::min(total, capacity), out);
    if (out && total > capacity) return refuse(FA_OUTPUT_TOO_SMALL, "output holds %lld of %lld candidates", (long long)capacity, (long long)total);
    return Verdict{};
}

}  // namespace vr
}  // namespace fa
