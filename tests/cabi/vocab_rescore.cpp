// A C++ caller of VocabularyRescorer (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by tests/test_cabi_vocab_rescore.py.
//   vocab_rescore args      no GPU needed: the build's refusals with their texts, every entry's answer to a missing context
//   vocab_rescore rescore   a six-word utterance on the device: candidates, verdicts and the applied list through ctcTokenRescore
// Floats are printed as their bit patterns.
#include <cstdio>
#include <cstring>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;
using VR = fl::VocabularyRescorer;

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

static VR::Symbols sym(const char *text) {
    VR::Symbols s;
    for (; *text; ++text) s.push_back(static_cast<unsigned char>(*text));
    return s;
}

static std::vector<VR::Term> vocabulary() {
    VR::Term a, b, c;
    a.charCount = 8; a.forms = {sym("livmarli")}; a.ctcTokenIds = {1, 2}; a.altTokenIds = {2};
    b.charCount = 6; b.minSimilarity = 0.6f; b.forms = {sym("newrez"), sym("new rez")}; b.ctcTokenIds = {3, 4, 5, 6};
    c.charCount = 2; c.forms = {sym("ab")}; c.ctcTokenIds = {1};
    return {a, b, c};
}

static int args() {
    const auto refusal = [](std::vector<VR::Term> terms) {
        try {
            VR r(std::move(terms));
        } catch (const fl::Error &e) {
            std::printf("BUILD %d %s\n", static_cast<int>(e.status), e.what());
            return;
        }
        std::printf("BUILD 0\n");
    };
    refusal(vocabulary());
    VR::Term wide;
    wide.charCount = 65; wide.forms = {sym("x"), VR::Symbols(65, 7)};
    refusal({wide});
    VR::Term many;
    many.charCount = 9;
    for (int32_t i = 0; i < 1023; i += 33) {
        VR::Symbols row;
        for (int32_t k = i; k < i + 33 && k < 1023; ++k) row.push_back(100 + k);
        many.forms.push_back(row);
    }
    refusal({many});
    const VR r(vocabulary());
    std::printf("BLOB %zu\n", r.blob.size());
    int64_t count = 7, need = 7;
    fa_vr_candidate cand{};
    fa_vr_verdict verdict{};
    const int64_t two[2] = {0, 0};
    const int a = (int)fa_vocab_rescore_candidates(nullptr, r.blob.data(), (int64_t)r.blob.size(), two, 1, two, nullptr, nullptr, 0.5f, &cand, 1, &count, nullptr);
    const int b = (int)fa_vocab_rescore_decide(nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, &cand, 1, two, nullptr, nullptr, 0, nullptr, two, nullptr, nullptr, nullptr, two, nullptr, &verdict, nullptr, nullptr);
    const int c = (int)fa_vocab_rescore_decide_dev(nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    const int d = (int)fa_vocab_rescore_build(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, nullptr, 0, nullptr, nullptr, 0);
    const int e = (int)fa_vocab_rescore_build(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, nullptr, 0, &need, nullptr, 0);
    std::printf("ST %d %d %d %d %d\nCOUNT %lld %lld\n", a, b, c, d, e, (long long)count, (long long)need);
    fa_vr_decide_config cfg;
    fa_vocab_rescore_default_config(&cfg);
    fa_vocab_rescore_default_config(nullptr);
    std::printf("CFG %.3f %.3f %08x %d %d %d %d %08x\n", cfg.frame_duration, cfg.margin_seconds, bits(cfg.cbw), cfg.blank_id, cfg.boost.use_adaptive_thresholds,
                cfg.boost.reference_token_count, cfg.boost.short_term_taper_pivot, bits(cfg.boost.short_term_taper_exponent));
    std::printf("BOOST %08x %08x %08x\n", bits(fa_vocab_rescore_boost(3.0f, 3, nullptr)), bits(fa_vocab_rescore_boost(3.0f, 6, nullptr)), bits(fa_vocab_rescore_boost(3.0f, 12, &cfg.boost)));
    return 0;
}

static int rescore() {
    fl::Context ctx(0);
    VR r(vocabulary());
    r.config.blank_id = 7;
    const char *text[6] = {"liv", "marli", "", "new", "res", "the"};
    std::vector<VR::Word> words;
    for (int i = 0; i < 6; ++i) {
        VR::Word w;
        w.symbols = sym(text[i]);
        w.stopword = w.multiWordStopword = i == 5;
        w.startTime = 0.16 * i;
        w.endTime = 0.16 * (i + 1);
        words.push_back(w);
    }
    VR::LogProbs lp;   // 12 frames of 8 columns on a coarse grid
    for (int t = 0; t < 12; ++t) {
        std::vector<float> row;
        for (int v = 0; v < 8; ++v) row.push_back(-0.5f * static_cast<float>((t * 5 + v * 3) % 7));
        lp.push_back(row);
    }
    int asked = 0;
    const VR::Decision d = r.ctcTokenRescore(ctx.handle(), lp, words, [&](int32_t first, int32_t span) {
        ++asked;
        std::vector<int32_t> tokens;
        for (int32_t k = 0; k < span; ++k) tokens.push_back((first + k) % 7);
        return tokens;
    });
    for (size_t i = 0; i < d.candidates.size(); ++i) {
        const fa_vr_candidate &c = d.candidates[i];
        const fa_vr_verdict &v = d.verdicts[i];
        std::printf("CAND %d %d %d %d %d %08x VERDICT %08x %08x %08x %08x %d %d %d %d %d %d\n", c.term, c.first_word, c.span_len, c.origin, c.form, bits(c.similarity),
                    bits(v.term_score), bits(v.original_score), bits(v.boost), bits(v.boosted_score), v.alt_won, v.compared, v.should_replace, v.outcome, v.start_frame, v.end_frame);
    }
    std::printf("APPLIED");
    for (const int32_t i : d.applied) std::printf(" %d", i);
    std::printf("\nASKED %d\n", asked);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
        if (argc == 2 && !std::strcmp(argv[1], "rescore")) return rescore();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
