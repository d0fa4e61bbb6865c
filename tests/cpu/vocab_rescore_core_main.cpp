// vocab_rescore_core_main.cpp — fluidaudio_amd/csrc/vocab_rescore_core.h driven on the CPU: a stand-alone program (built by
// tests/test_vocab_rescore_cpu.py with the address and undefined-behaviour sanitizers, by scripts/vocab_rescore_timing.py with -O2).
// It reads one command and its integers from standard input (a float as its 32 bits, a double as its 64 bits) and prints what the
// header's functions answer, one tagged line per fact:
//   bitdp                                  the bit-vector step against the plain DP: every pair of strings of up to 6 symbols over 3
//                                          letters, and random patterns of 31, 32, 33, 63 and 64 symbols against random texts, at every
//                                          prefix of the text
//   build   <vocabulary>                   the blob's contents (ALPHABET, STRING, TERM, FORM lines), or the refusal
//   corrupt <vocabulary>                   every header word and every index of the blob damaged in turn: validate() refuses each
//   walk    <vocabulary> <min bits> <words> [time]   the reference walk's records (CAND lines) — or only its wall time
//   arbitrate n (sim bits, first, span)* W occupied*  APPLIED / SUPERSEDED
//   window  start end frame_duration margin valid    WINDOW start end, or WINDOW none
//   boost   n (cbw_bits tokens adaptive reference pivot exponent_bits)*   a BOOST bits line each
// <vocabulary>: min_term_length terms, per term char_count has_min min_bits rows, per row length symbols*
// <words>:      batch, per utterance words, per word flags length symbols*
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../fluidaudio_amd/csrc/vocab_rescore_core.h"

namespace vr = fa::vr;

static int64_t next_int() {
    long long v = 0;
    if (!(std::cin >> v)) { std::printf("INPUT short\n"); std::exit(2); }
    return v;
}
static float next_float() { return vr::bits_float(static_cast<int32_t>(static_cast<uint32_t>(next_int()))); }
static double next_double() {
    const uint64_t b = static_cast<uint64_t>(next_int());
    double d;
    std::memcpy(&d, &b, sizeof(d));
    return d;
}

struct Vocabulary {
    int32_t min_term_length = 0, terms = 0;
    std::vector<int32_t> char_counts, symbols;
    std::vector<float> mins;
    std::vector<int64_t> term_rows{0}, row_offsets{0};
};

static Vocabulary read_vocabulary() {
    Vocabulary v;
    v.min_term_length = static_cast<int32_t>(next_int());
    v.terms = static_cast<int32_t>(next_int());
    for (int32_t t = 0; t < v.terms; ++t) {
        v.char_counts.push_back(static_cast<int32_t>(next_int()));
        const bool has_min = next_int() != 0;
        const float m = next_float();
        v.mins.push_back(has_min ? m : -1.0f);
        const int64_t rows = next_int();
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t n = next_int();
            for (int64_t i = 0; i < n; ++i) v.symbols.push_back(static_cast<int32_t>(next_int()));
            v.row_offsets.push_back(static_cast<int64_t>(v.symbols.size()));
        }
        v.term_rows.push_back(static_cast<int64_t>(v.row_offsets.size()) - 1);
    }
    return v;
}

static fa::Verdict build_blob(const Vocabulary &v, std::vector<int32_t> &blob) {
    int64_t need = 0;
    const int32_t none = 0;
    const int32_t *syms = v.symbols.empty() ? &none : v.symbols.data();
    fa::Verdict verdict = vr::build(v.char_counts.data(), v.mins.data(), v.term_rows.data(), v.row_offsets.data(), syms, v.terms, v.min_term_length, nullptr, 0, &need);
    if (verdict.status != FA_SUCCESS) return verdict;
    blob.assign(static_cast<size_t>(need), -1);
    if (need > 1) {   // a buffer that is one word short is refused and left alone
        int64_t again = 0;
        const fa::Verdict small = vr::build(v.char_counts.data(), v.mins.data(), v.term_rows.data(), v.row_offsets.data(), syms, v.terms, v.min_term_length, blob.data(), need - 1, &again);
        if (small.status != FA_OUTPUT_TOO_SMALL || again != need || blob[0] != -1) std::printf("SMALL wrong %d\n", static_cast<int>(small.status));
    }
    return vr::build(v.char_counts.data(), v.mins.data(), v.term_rows.data(), v.row_offsets.data(), syms, v.terms, v.min_term_length, blob.data(), need, &need);
}

static void print_verdict(const fa::Verdict &v) { std::printf("VERDICT %d %s\n", static_cast<int>(v.status), v.text); }

static int cmd_bitdp() {
    long long pairs = 0, prefixes = 0, wrong = 0;
    const auto check = [&](const std::vector<int32_t> &pattern, const std::vector<int32_t> &text, const int alphabet) {
        std::vector<uint64_t> masks(static_cast<size_t>(alphabet), 0);
        for (size_t i = 0; i < pattern.size(); ++i) masks[pattern[i]] |= uint64_t{1} << i;
        vr::BitDp s;
        vr::bitdp_begin(s, static_cast<int32_t>(pattern.size()));
        ++pairs;
        for (size_t j = 0; j <= text.size(); ++j) {
            if (j > 0) vr::bitdp_step(s, masks[text[j - 1]]);
            ++prefixes;
            if (s.score != vr::levenshtein(pattern.data(), static_cast<int32_t>(pattern.size()), text.data(), static_cast<int32_t>(j))) ++wrong;
        }
    };
    std::vector<std::vector<int32_t>> all;   // every string of 0 ... 6 symbols over {1, 2, 3}
    for (int n = 0; n <= 6; ++n) {
        int count = 1;
        for (int i = 0; i < n; ++i) count *= 3;
        for (int c = 0; c < count; ++c) {
            std::vector<int32_t> s;
            for (int i = 0, v = c; i < n; ++i, v /= 3) s.push_back(1 + v % 3);
            all.push_back(s);
        }
    }
    for (const auto &p : all)
        if (!p.empty())
            for (const auto &t : all) check(p, t, 4);
    std::mt19937 rng(7);
    for (const int m : {31, 32, 33, 63, 64})
        for (int rep = 0; rep < 200; ++rep) {
            const int alphabet = rep % 2 ? 3 : 5;   // id 0 occurs in the text only: a symbol no form holds
            std::vector<int32_t> p(static_cast<size_t>(m)), t(static_cast<size_t>(rng() % 90));
            for (auto &x : p) x = 1 + static_cast<int32_t>(rng() % (alphabet - 1));
            for (auto &x : t) x = static_cast<int32_t>(rng() % alphabet);
            if (rep % 5 == 0) { t = p; if (!t.empty()) t[rng() % t.size()] = 0; }   // a near match
            check(p, t, alphabet);
        }
    std::printf("BITDP %lld %lld %lld\n", pairs, prefixes, wrong);
    return 0;
}

static void dump(const std::vector<int32_t> &blob) {
    vr::Header h;
    print_verdict(vr::validate(blob.data(), static_cast<int64_t>(blob.size()), h));
    std::printf("ALPHABET");
    for (int32_t i = 0; i + 1 < h.A; ++i) std::printf(" %d", blob[h.off_alphabet + i]);
    std::printf("\n");
    const auto raw = [&](const int32_t id) { return blob[h.off_alphabet + id - 1]; };
    for (int32_t s = 0; s < h.n_strings; ++s) {
        int32_t n;
        const int32_t *p = vr::string_at(blob.data(), h, s, n);
        std::printf("STRING %d", s);
        for (int32_t i = 0; i < n; ++i) std::printf(" %d", raw(p[i]));
        std::printf("\n");
    }
    for (int32_t t = 0; t < h.n_terms; ++t) {
        const vr::Term tm = vr::term_at(blob.data(), h, t);
        std::printf("TERM %d %d %d %u %d %d\n", tm.src, tm.char_count, tm.has_min, static_cast<uint32_t>(vr::float_bits(tm.min_similarity)), tm.canon_sid, tm.n_forms);
        for (int32_t f = 0; f < tm.n_forms; ++f) {
            const vr::Form fm = vr::form_at(blob.data(), h, tm.first_form + f);
            std::printf("FORM %d %d %d", fm.sid, fm.len, fm.words);
            for (int32_t id = 0; id < h.A; ++id) {
                const uint64_t m = vr::mask_at(blob.data(), h, tm.first_form + f, id);
                if (m) std::printf(" %d:%" PRIx64, id == 0 ? -1 : raw(id), m);
            }
            std::printf("\n");
        }
    }
}

static int cmd_corrupt(std::vector<int32_t> blob) {
    vr::Header h;
    if (vr::validate(blob.data(), static_cast<int64_t>(blob.size()), h).status != FA_SUCCESS) { std::printf("CORRUPT the blob itself is refused\n"); return 1; }
    int tried = 0, refused = 0;
    const auto attempt = [&](const size_t at, const int32_t value) {
        const int32_t kept = blob[at];
        if (kept == value) return;
        blob[at] = value;
        vr::Header g;
        ++tried;
        if (vr::validate(blob.data(), static_cast<int64_t>(blob.size()), g).status == FA_INVALID_ARGUMENT) ++refused;
        else std::printf("ACCEPTED word %zu = %d\n", at, value);
        blob[at] = kept;
    };
    const int32_t big = static_cast<int32_t>(blob.size());
    for (const size_t at : {0, 1, 2, 4, 6, 8, 10, 12, 13})                      // magic, version, the total, every offset
        for (const int32_t v : {-1, big + 1, INT32_MAX, INT32_MIN}) attempt(at, v);
    for (const size_t at : {3, 5, 7, 9, 11})                                    // every count
        for (const int32_t v : {-1, big + 1, INT32_MAX}) attempt(at, v);
    attempt(14, -1); attempt(14, h.A);                                          // the space id
    attempt(11, 0); attempt(11, vr::kMaxAlphabet);
    for (int32_t t = 0; t < h.n_terms; ++t) {                                   // a term's form range and canonical sid
        const size_t r = static_cast<size_t>(h.off_terms) + static_cast<size_t>(t) * vr::kTermWords;
        attempt(r + 0, -1); attempt(r + 0, h.input_terms);
        attempt(r + 4, -1); attempt(r + 4, h.n_forms); attempt(r + 5, 0); attempt(r + 5, h.n_forms + 1); attempt(r + 6, -2); attempt(r + 6, h.n_strings);
    }
    for (int32_t f = 0; f < h.n_forms; ++f) {                                   // a form's sid and length
        const size_t r = static_cast<size_t>(h.off_forms) + static_cast<size_t>(f) * vr::kFormWords;
        attempt(r + 0, -1); attempt(r + 0, h.n_strings); attempt(r + 1, 0); attempt(r + 1, vr::kMaxForm + 1);
    }
    for (int32_t s = 0; s < h.n_strings; ++s) {                                 // a string's span
        const size_t r = static_cast<size_t>(h.off_strings) + static_cast<size_t>(s) * vr::kStringWords;
        attempt(r + 0, -1); attempt(r + 0, h.n_string_syms); attempt(r + 1, 0); attempt(r + 1, vr::kMaxForm + 1);
    }
    for (int32_t i = 0; i < h.n_string_syms; ++i) { attempt(static_cast<size_t>(h.off_string_syms) + i, 0); attempt(static_cast<size_t>(h.off_string_syms) + i, h.A); }
    vr::Header g;
    ++tried;
    if (vr::validate(blob.data(), static_cast<int64_t>(blob.size()) - 1, g).status == FA_INVALID_ARGUMENT) ++refused;   // the last word missing
    ++tried;
    if (vr::validate(nullptr, 0, g).status == FA_INVALID_ARGUMENT) ++refused;
    std::printf("CORRUPT %d %d\n", tried, refused);
    return 0;
}

static int cmd_walk(const std::vector<int32_t> &blob) {
    const float min_similarity = next_float();
    const int32_t batch = static_cast<int32_t>(next_int());
    std::vector<int64_t> utt{0}, off{0};
    std::vector<int32_t> syms;
    std::vector<uint8_t> flags;
    for (int32_t u = 0; u < batch; ++u) {
        const int64_t W = next_int();
        for (int64_t w = 0; w < W; ++w) {
            flags.push_back(static_cast<uint8_t>(next_int()));
            const int64_t n = next_int();
            for (int64_t i = 0; i < n; ++i) syms.push_back(static_cast<int32_t>(next_int()));
            off.push_back(static_cast<int64_t>(syms.size()));
        }
        utt.push_back(static_cast<int64_t>(off.size()) - 1);
    }
    std::string tail;
    const bool timed = static_cast<bool>(std::cin >> tail) && tail == "time";
    vr::Header h;
    fa::Verdict v = vr::validate(blob.data(), static_cast<int64_t>(blob.size()), h);
    if (v.status != FA_SUCCESS) { print_verdict(v); return 0; }
    vr::Words words;
    const int32_t none = 0;
    const uint8_t no_flag = 0;
    v = vr::check_words(blob.data(), h, utt.data(), batch, off.data(), syms.empty() ? &none : syms.data(), flags.empty() ? &no_flag : flags.data(), min_similarity, words);
    print_verdict(v);
    if (v.status != FA_SUCCESS) return 0;
    std::vector<fa_vr_candidate> out;
    const auto t0 = std::chrono::steady_clock::now();
    vr::walk_candidates(blob.data(), h, words, min_similarity, out);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (timed) { std::printf("TIME %.3f %zu\n", ms, out.size()); return 0; }
    std::vector<fa_vr_candidate> sorted = out;
    std::sort(sorted.begin(), sorted.end(), vr::candidate_before);
    for (size_t i = 0; i < out.size(); ++i)   // the walk's append order is the order of the keys
        if (std::memcmp(&sorted[i], &out[i], sizeof(fa_vr_candidate)) != 0) { std::printf("ORDER differs at %zu\n", i); break; }
    for (const fa_vr_candidate &c : out)
        std::printf("CAND %d %d %d %d %d %d %u\n", c.utterance, c.term, c.first_word, c.span_len, c.origin, c.form, static_cast<uint32_t>(vr::float_bits(c.similarity)));
    return 0;
}

int main() {
    std::string cmd;
    if (!(std::cin >> cmd)) return 2;
    if (cmd == "bitdp") return cmd_bitdp();
    if (cmd == "build" || cmd == "corrupt" || cmd == "walk") {
        const Vocabulary v = read_vocabulary();
        std::vector<int32_t> blob;
        const fa::Verdict verdict = build_blob(v, blob);
        if (verdict.status != FA_SUCCESS) { print_verdict(verdict); return 0; }
        if (cmd == "build") { dump(blob); return 0; }
        if (cmd == "corrupt") return cmd_corrupt(blob);
        return cmd_walk(blob);
    }
    if (cmd == "arbitrate") {
        const int32_t n = static_cast<int32_t>(next_int());
        std::vector<float> sim;
        std::vector<int32_t> first, span;
        for (int32_t i = 0; i < n; ++i) { sim.push_back(next_float()); first.push_back(static_cast<int32_t>(next_int())); span.push_back(static_cast<int32_t>(next_int())); }
        const int64_t W = next_int();
        std::vector<uint8_t> occupied;
        for (int64_t i = 0; i < W; ++i) occupied.push_back(static_cast<uint8_t>(next_int()));
        occupied.push_back(0);
        std::vector<int32_t> applied;
        std::vector<uint8_t> superseded;
        vr::arbitrate(n, sim.data(), first.data(), span.data(), occupied.data(), applied, superseded);
        std::printf("APPLIED");
        for (const int32_t i : applied) std::printf(" %d", i);
        std::printf("\nSUPERSEDED");
        for (int32_t i = 0; i < n; ++i)
            if (superseded[i]) std::printf(" %d", i);
        std::printf("\nBUCKETS");
        for (int32_t i = 0; i < n; ++i) std::printf(" %d", vr::bucket(sim[i]));
        std::printf("\n");
        return 0;
    }
    if (cmd == "window") {
        const double a = next_double(), b = next_double(), fd = next_double(), margin = next_double();
        const int32_t valid = static_cast<int32_t>(next_int());
        int32_t s = 0, e = 0;
        if (vr::frame_window(a, b, fd, margin, valid, s, e)) std::printf("WINDOW %d %d\n", s, e);
        else std::printf("WINDOW none\n");
        return 0;
    }
    if (cmd == "boost") {
        const int64_t queries = next_int();
        for (int64_t q = 0; q < queries; ++q) {
            const float cbw = next_float();
            const int32_t tokens = static_cast<int32_t>(next_int());
            fa_vr_boost_config c;
            c.use_adaptive_thresholds = static_cast<int32_t>(next_int());
            c.reference_token_count = static_cast<int32_t>(next_int());
            c.short_term_taper_pivot = static_cast<int32_t>(next_int());
            c.short_term_taper_exponent = next_float();
            std::printf("BOOST %u\n", static_cast<uint32_t>(vr::float_bits(vr::boost(cbw, tokens, c))));
        }
        return 0;
    }
    std::printf("UNKNOWN %s\n", cmd.c_str());
    return 2;
}
