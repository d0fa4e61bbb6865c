// A C++ caller of RnntConfig / NemotronVocabularyBias (include/fluidaudio.hpp) and of the fa_rnnt_* entries, built with -Wall -Wextra
// -Werror by tests/test_cabi_rnnt.py.  No device: the bias tables are host work, and the decoding entry is only asked for its refusals.
#include <cstdio>
#include <optional>
#include <string>
#include <vector>

#include "fluidaudio.hpp"

using namespace fluidaudio;

static void show(const char *tag, const NemotronVocabularyBias &b) {
    std::printf("%s", tag);
    for (const NemotronVocabularyBias::Candidate &c : b.candidates()) std::printf(" %d=%g", c.tokenId, static_cast<double>(c.boost));
    std::printf("\n");
}

int main() {
    const std::string m = "\xE2\x96\x81";
    // the toy table of NemotronVocabularyBiasTests.swift:11-20, folded
    std::vector<std::optional<std::string>> pieces(25);
    const std::pair<int, std::string> table[] = {{0, m}, {1, m + "to"}, {2, "r"}, {3, "vane"}, {4, m + "tor"}, {5, m + "torvane"}, {6, m + "the"}, {7, m + "the"},
                                                 {8, m + "ran"}, {9, m + "t"}, {10, m + "cr"}, {11, "an"}, {18, "<unk>"}, {19, "<en-us>"}, {21, m + "ab"},
                                                 {22, m + "c"}, {23, "v"}, {24, m + "vor"}};
    for (const auto &p : table) pieces[static_cast<size_t>(p.first)] = p.second;

    RnntConfig cfg;
    fa_rnnt_config raw;
    fa_rnnt_default_config(&raw);
    fa_rnnt_default_config(nullptr);
    std::printf("CFG %d %d %d %d %d %d %zu\n", cfg.blankId, cfg.eouId, cfg.maxSymbolsPerStep, raw.blank_id, raw.eou_id, raw.max_symbols_per_step, sizeof(fa_rnnt_config));
    std::printf("BOOST %g %g %g %g %g\n", static_cast<double>(NemotronVocabularyBias::effectiveBoost({"x", std::nullopt, {}})),
                static_cast<double>(NemotronVocabularyBias::effectiveBoost({"x", 10.0f, {}})), static_cast<double>(NemotronVocabularyBias::effectiveBoost({"x", 6.0f, {}})),
                static_cast<double>(NemotronVocabularyBias::effectiveBoost({"x", 5.5f, {}}, 3.0f)), static_cast<double>(NemotronVocabularyBias::effectiveBoost({"x", std::nullopt, {}}, 3.0f)));

    std::optional<NemotronVocabularyBias> bias = NemotronVocabularyBias::make({{"torvane", std::nullopt, {"vortane"}}, {"ab ab c", 5.5f, {}}}, pieces);
    if (!bias) return 1;
    std::printf("CAP %d %d\n", bias->tailCap(), bias->blob().empty() ? 0 : 1);
    show("FRESH", *bias);
    bias->observe(4);
    bias->observe(19);      // a special piece, then ids outside the table: the match state stays
    bias->observe(12);
    bias->observe(99);
    bias->observe(-1);
    show("TOR", *bias);
    bias->observe(7);
    show("THE", *bias);
    for (int i = 0; i < 40; ++i) bias->observe(21);     // more emissions than the tail holds
    show("ABAB", *bias);
    bias->resetMatchState();
    show("RESET", *bias);
    std::printf("NONE %d %d %d\n", NemotronVocabularyBias::make({}, pieces).has_value(), NemotronVocabularyBias::make({{"torvane", 0.0f, {}}}, pieces).has_value(),
                NemotronVocabularyBias::make({{"torvane", -1.0f, {}}}, pieces).has_value());
    int thrown = 0;
    try { NemotronVocabularyBias::make({{"\xC0\x80", std::nullopt, {}}}, pieces); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    try { NemotronVocabularyBias::make({{std::string(300, 'a'), std::nullopt, {}}}, pieces); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    try { NemotronVocabularyBias::make({{std::string("a\0b", 3), std::nullopt, {}}}, pieces); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    std::printf("THROWN %d\n", thrown);

    // every refusal of the host entries is a status
    const char *p1[] = {"ab"};
    const char *s1[] = {"ab"};
    const float b1[] = {4.5f}, b0[] = {0.0f};
    int64_t need = -7;
    int32_t cap = -7, blob[4], count = -7;
    std::printf("ST build %d %d %d %d %d %d", fa_rnnt_bias_build(p1, 1, s1, b1, 1, nullptr, 0, nullptr, &cap), fa_rnnt_bias_build(p1, 1, s1, b1, 1, nullptr, 0, &need, nullptr),
                fa_rnnt_bias_build(nullptr, 1, s1, b1, 1, nullptr, 0, &need, &cap), fa_rnnt_bias_build(p1, 1, nullptr, b1, 1, nullptr, 0, &need, &cap),
                fa_rnnt_bias_build(p1, 1, s1, b0, 1, nullptr, 0, &need, &cap), fa_rnnt_bias_build(p1, -1, s1, b1, 1, nullptr, 0, &need, &cap));
    std::printf(" %lld %d", static_cast<long long>(need), cap);                                                  // a refusal writes nothing
    std::printf(" %d", fa_rnnt_bias_build(p1, 1, s1, b1, 1, blob, 4, &need, &cap));                              // too small
    const fa_status none = fa_rnnt_bias_build(p1, 1, s1, b1, 0, nullptr, 0, &need, &cap);                         // no surface: no bias
    std::printf(" %d %lld\n", none, static_cast<long long>(need));
    std::printf("ST candidates %d %d %d %d\n", fa_rnnt_bias_candidates(nullptr, 0, nullptr, 0, nullptr, nullptr, 0, &count), fa_rnnt_bias_candidates(blob, 4, nullptr, 0, nullptr, nullptr, 0, &count),
                fa_rnnt_bias_candidates(bias->blob().data(), static_cast<int64_t>(bias->blob().size()), nullptr, 0, nullptr, nullptr, 0, nullptr),
                fa_rnnt_bias_candidates(bias->blob().data(), static_cast<int64_t>(bias->blob().size()) - 1, nullptr, 0, nullptr, nullptr, 0, &count));
    std::printf("ST greedy %d %d\n", fa_rnnt_greedy_logits_dev(nullptr, &raw, nullptr, FA_DTYPE_F32, 1, 1, 1, 1, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr,
                                                               nullptr, nullptr, nullptr, nullptr, nullptr),
                fa_rnnt_greedy_logits_dev(nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr));
    return 0;
}
