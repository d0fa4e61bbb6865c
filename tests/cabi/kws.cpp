// A C++ caller of CtcKeywordSpotter (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by tests/test_cabi_kws.py.
//   kws args     no GPU needed: every argument error is a status / an Error, nothing crashes; the threshold rule by its bits
//   kws spot     a five-frame utterance on the device: the per-term loop, ctcWordSpotMultiple and ctcWordSpotConstrained
// Floats are printed as their bit patterns.
#include <cstdio>
#include <cstring>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;
using KS = fl::CtcKeywordSpotter;

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class F>
static int status_of(F &&f) {
    try {
        f();
    } catch (const fl::Error &e) {
        return static_cast<int>(e.status);
    }
    return 0;
}

static KS::LogProbs utterance() {   // token 0, three frames of blank (3), token 1 — CtcDPAlgorithmTests.testBlankEmissionCostIsAccumulated
    const float hi = -0.1f, bl = -0.5f, cold = -10.0f;
    return {{hi, cold, cold, bl}, {cold, cold, cold, bl}, {cold, cold, cold, bl}, {cold, cold, cold, bl}, {cold, hi, cold, bl}};
}

static int args() {
    fa_ctx *none = nullptr;
    const KS::LogProbs lp = utterance();
    const std::vector<int32_t> wide(128, 1);
    KS::LogProbs ragged = lp;
    ragged[2].pop_back();
    std::printf("ST %d %d %d %d\n", status_of([&] { KS::ctcWordSpotMultiple(none, lp, wide); }), status_of([&] { KS::ctcWordSpotMultiple(none, ragged, {0, 1}); }),
                status_of([&] { KS::ctcWordSpotConstrained(none, lp, {0, 1}, 0, 5, 3); }), status_of([&] { KS::spotKeywordsFromLogProbs(none, lp, 0.08, {{"ab", {0, 1}}}); }));
    int64_t count = 7;
    const int64_t off[2] = {0, 128};
    const fa_kws_window w{0, 0, 0, 1};
    fa_kws_detection d{};
    const int a = (int)fa_ctc_kws_spot_batch(nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, &count, nullptr);
    const int b = (int)fa_ctc_kws_spot_batch_dev(nullptr, nullptr, 1, 1, 4, 4, 4, nullptr, wide.data(), off, 1, nullptr, 3, 1, nullptr, 0, nullptr, nullptr);
    const int c = (int)fa_ctc_kws_score_windows_dev(nullptr, nullptr, 1, 1, 4, 4, 4, nullptr, wide.data(), off, 1, &w, 1, 3, &d);
    const int e = (int)fa_ctc_kws_score_windows(nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr);
    std::printf("ST %d %d %d %d\n", a, b, c, e);
    std::printf("COUNT %lld\n", (long long)count);
    std::printf("THR %08x %08x %08x %08x %08x\n", bits(fa_kws_adjusted_threshold(0, -3.0f, 9)), bits(fa_kws_adjusted_threshold(1, -8.5f, 3)),
                bits(fa_kws_adjusted_threshold(1, -8.5f, 10)), bits(fa_kws_adjusted_threshold(1, -0.1f, 4)), bits(fa_kws_adjusted_threshold(1, 16777216.0f, 4)));
    return 0;
}

static int spot() {
    fl::Context ctx(0);
    const KS::LogProbs lp = utterance();
    const std::vector<KS::Term> terms = {{"ab", {0, 1}}, {"", {}}, {"a*b", {0, KS::wildcardTokenId, 1}}, {"ba", {1, 0}}, {"abab", {0, 1, 0, 1}}};
    for (const auto &d : KS::spotKeywordsFromLogProbs(ctx, lp, 0.08, terms, -6.0f, 3))
        std::printf("DET %zu %08x %d %d %d %016llx %016llx\n", d.term, bits(d.score), d.totalFrames, d.startFrame, d.endFrame, bits(d.startTime), bits(d.endTime));
    for (const auto &s : KS::ctcWordSpotMultiple(ctx.handle(), lp, {0}, -100.0f, false, 3)) std::printf("MUL %08x %d %d\n", bits(s.score), s.startFrame, s.endFrame);
    const KS::Spot c = KS::ctcWordSpotConstrained(ctx.handle(), lp, {0, 1}, 0, 5, 3), e = KS::ctcWordSpotConstrained(ctx.handle(), lp, {0, 1}, 4, 9, 3);
    std::printf("CON %08x %d %d\nCON %08x %d %d\n", bits(c.score), c.startFrame, c.endFrame, bits(e.score), e.startFrame, e.endFrame);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
        if (argc == 2 && !std::strcmp(argv[1], "spot")) return spot();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
