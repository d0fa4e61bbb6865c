// A C++ caller of WERCalculator / StringUtils (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by tests/test_cabi_wer.py.
//   wer args                 no GPU needed: every argument error is a status / an Error, nothing crashes
//   wer score <m> <n>        a word pair, and a pair of m x n tokens over three words drawn by the generator below, on the device
// Doubles are printed as their bit patterns.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

static int status_of(const fl::WERCalculator::Tokens &hyp, const fl::WERCalculator::Tokens &ref) {
    try {
        fl::WERCalculator::editDistance(static_cast<fa_ctx *>(nullptr), hyp, ref);
    } catch (const fl::Error &e) {
        return static_cast<int>(e.status);
    }
    return 0;
}

static int args() {
    const int32_t sym[4] = {1, 2, 3, 4};
    const int64_t ok[3] = {0, 2, 4}, down[3] = {0, 3, 2}, below[3] = {-1, 2, 4}, huge[2] = {0, int64_t{1} << 31};
    fa_edit_counts out[2];
    std::memset(out, 0x55, sizeof(out));
    // no context: a well-formed call, empty sides included, still ends in INVALID_ARGUMENT
    std::printf("ST %d %d %d\n", status_of({"a"}, {"a", "b"}), status_of({}, {"a"}), status_of({}, {}));
    std::printf("ST %d %d %d %d %d %d %d %d\n", (int)fa_edit_distance_batch(nullptr, sym, ok, sym, ok, -1, out), (int)fa_edit_distance_batch(nullptr, sym, nullptr, sym, ok, 2, out),
                (int)fa_edit_distance_batch(nullptr, sym, ok, sym, ok, 2, nullptr), (int)fa_edit_distance_batch(nullptr, sym, down, sym, ok, 2, out),
                (int)fa_edit_distance_batch_dev(nullptr, sym, ok, sym, below, 2, out), (int)fa_edit_distance_batch(nullptr, nullptr, ok, sym, ok, 2, out),
                (int)fa_edit_distance_batch(nullptr, sym, ok, sym, ok, 2, out), (int)fa_edit_distance_batch(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    std::printf("ST %d %d %d\n", (int)fa_edit_distance_batch(nullptr, sym, huge, sym, ok, 1, out), (int)fa_edit_distance_batch_dev(nullptr, sym, ok, sym, huge, 1, out),
                (int)fa_edit_distance_batch(nullptr, sym, ok, sym, ok, INT32_MAX, out));
    const unsigned char *p = reinterpret_cast<const unsigned char *>(out);
    int untouched = 1;
    for (size_t i = 0; i < sizeof(out); ++i) untouched &= p[i] == 0x55;
    std::printf("OUT %d\n", untouched);
    return 0;
}

static void print(const char *tag, const fl::WERCalculator::EditDistanceResult &d) { std::printf("%s %d %d %d %d\n", tag, d.total, d.insertions, d.deletions, d.substitutions); }

static int score(int m, int n) {
    fl::Context ctx(0);
    const fl::WERCalculator::Tokens ref = {"the", "quick", "brown", "fox", "jumps", "over", "the", "lazy", "dog"},
                                    hyp = {"the", "fast", "brown", "fox", "jumped", "over", "a", "lazy", "dog"};
    print("WORDS", fl::WERCalculator::editDistance(ctx, hyp, ref));
    const fl::WERCalculator::WERMetrics w = fl::WERCalculator::calculateWERMetrics(ctx.handle(), hyp, ref);
    std::printf("WER %016llx %d %d %d %d\n", bits(w.wer), w.insertions, w.deletions, w.substitutions, w.totalWords);
    const fl::WERCalculator::WERMetrics e = fl::WERCalculator::calculateWERMetrics(ctx.handle(), hyp, {});
    std::printf("WER %016llx %d %d %d %d\n", bits(e.wer), e.insertions, e.deletions, e.substitutions, e.totalWords);
    std::printf("LEV %d %d\n", fl::StringUtils::levenshteinDistance(ctx, {1, 2, 3}, {1, 3, 3}), fl::StringUtils::levenshteinDistance(ctx, {}, {1, 2}));
    // x <- (1103515245 x + 12345) mod 2^31 from 1; a token is word (x >> 16) % 3, the hypothesis first
    unsigned long long x = 1;
    const char *words[3] = {"ja", "nein", "doch"};
    fl::WERCalculator::Tokens a, b;
    for (int i = 0; i < m + n; ++i) {
        x = (1103515245ull * x + 12345ull) % 2147483648ull;
        (i < m ? a : b).push_back(words[(x >> 16) % 3]);
    }
    const auto both = fl::WERCalculator::editDistance(ctx.handle(), {{a, b}, {hyp, ref}, {b, a}});
    print("LONG", both[0]);
    print("WORDS", both[1]);
    print("SWAPPED", both[2]);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
        if (argc == 4 && !std::strcmp(argv[1], "score")) return score(std::atoi(argv[2]), std::atoi(argv[3]));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
