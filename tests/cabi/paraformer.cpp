// A C++ caller of ParaformerCif / ParaformerManager (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by
// tests/test_cabi_paraformer.py.
//   paraformer args              no GPU needed: every argument error is a status / an Error, nothing crashes, nothing is written
//   paraformer cif <T> <D>       integrateAndFireWithFireFrames on rows and alphas drawn by the generator below, on the device
//   paraformer stamps <T>        decodeWithTimestamps on generated alphas and a gated noise signal, on the device
// Floats and doubles are printed as their bit patterns.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

// x <- (1103515245 x + 12345) mod 2^31 from 1; a draw is (x >> 16) % m
struct Lcg {
    unsigned long long x = 1;
    int next(int m) {
        x = (1103515245ull * x + 12345ull) % 2147483648ull;
        return static_cast<int>((x >> 16) % static_cast<unsigned long long>(m));
    }
};

static int args() {
    float enc[64], alphas[8], ac[2 * 128 * 8];
    int32_t tc[2], fc[2], ff[10];
    std::memset(enc, 0, sizeof(enc));
    std::memset(alphas, 0, sizeof(alphas));
    std::memset(ac, 0x55, sizeof(ac));
    std::memset(tc, 0x55, sizeof(tc));
    std::memset(fc, 0x55, sizeof(fc));
    std::memset(ff, 0x55, sizeof(ff));
    fa_paraformer_cif_config cfg;
    fa_paraformer_cif_default_config(&cfg);
    std::printf("CFG %08x %08x %d %d\n", bits(cfg.threshold), bits(cfg.tail_threshold), cfg.max_tokens, cfg.enc_frames);
    const auto cif = [&](int32_t batch, int32_t frames, int32_t dim, int64_t rs, const void *e, float *out) {
        return static_cast<int>(fa_paraformer_cif(nullptr, &cfg, e, FA_DTYPE_F32, batch, frames, dim, rs, 32, alphas, 4, nullptr, out, nullptr, tc, fc, ff));
    };
    std::printf("ST %d %d %d %d %d %d %d\n", cif(-1, 4, 8, 8, enc, ac), cif(2, -1, 8, 8, enc, ac), cif(2, 4, 0, 8, enc, ac), cif(2, 4, 8, 7, enc, ac), cif(2, 4, 8, 8, nullptr, ac),
                cif(2, 4, 8, 8, enc, nullptr), cif(2, 4, 8, 8, enc, ac));
    std::printf("ST %d\n", static_cast<int>(fa_paraformer_cif_dev(nullptr, &cfg, enc, FA_DTYPE_F32, 1 << 25, 4, 8, 8, 32, alphas, 4, nullptr, ac, nullptr, tc, fc, ff)));
    int32_t ids[256], counts[2] = {3, 128}, over[2] = {3, 129};
    std::memset(ids, 0, sizeof(ids));
    const uint8_t keep[4] = {0, 0, 0, 1};
    const int64_t off[3] = {0, 40, 64}, down[3] = {0, 50, 40}, huge[3] = {0, 40, int64_t{1} << 32};
    fa_paraformer_span spans[4];
    std::memset(spans, 0x55, sizeof(spans));
    int64_t count = 0x5555, utt[2] = {0x5555, 0x5555};
    const auto stamps = [&](int32_t batch, const int32_t *c, const int64_t *o, int64_t cap, int64_t *n) {
        return static_cast<int>(fa_paraformer_timestamps(nullptr, &cfg, alphas, 4, batch, 4, nullptr, ids, c, keep, 4, enc, o, spans, cap, n, utt));
    };
    std::printf("ST %d %d %d %d %d %d\n", stamps(-1, counts, off, 4, &count), stamps(2, over, off, 4, &count), stamps(2, counts, down, 4, &count), stamps(2, counts, off, -1, &count),
                stamps(2, counts, off, 4, nullptr), stamps(2, counts, off, 4, &count));
    std::printf("ST %d\n", stamps(2, counts, huge, 4, &count));
    // the mirror: a well-formed call without a context ends in an Error carrying INVALID_ARGUMENT
    int thrown = 0;
    try {
        fl::ParaformerCif::integrateAndFire(static_cast<fa_ctx *>(nullptr), {{1.0f, 2.0f}}, {0.5f});
    } catch (const fl::Error &e) {
        thrown = static_cast<int>(e.status);
    }
    int ragged = 0;
    try {
        fl::ParaformerCif::integrateAndFire(static_cast<fa_ctx *>(nullptr), {{1.0f, 2.0f}, {1.0f}}, {0.5f, 0.5f});
    } catch (const fl::Error &e) {
        ragged = static_cast<int>(e.status);
    }
    std::printf("ST %d %d\n", thrown, ragged);
    int untouched = count == 0x5555 && utt[0] == 0x5555 && utt[1] == 0x5555;
    const auto same = [&](const void *p, size_t n) {
        for (size_t i = 0; i < n; ++i) untouched &= static_cast<const unsigned char *>(p)[i] == 0x55;
    };
    same(ac, sizeof(ac));
    same(tc, sizeof(tc));
    same(fc, sizeof(fc));
    same(ff, sizeof(ff));
    same(spans, sizeof(spans));
    std::printf("OUT %d\n", untouched);
    // the text side needs no device
    const fl::ParaformerManager::Vocabulary vocab = {{0, "<blank>"}, {1, "<s>"}, {2, "</s>"}, {3, "\xE2\x96\x81he"}, {4, "llo"}, {5, "cu@@"}, {6, "t"}, {7, "\xE2\x96\x81"}};
    std::printf("TEXT [%s]\n", fl::ParaformerManager::decode({1, 3, 4, 0, 7, 5, 6, 2, 99}, vocab).c_str());
    const std::vector<fa_paraformer_span> raw = {{0, 0, -0.5, 0.1}, {0, 1, 0.1, 0.2}, {0, 2, 0.2, 0.3}, {0, 3, 0.3, 0.4}, {0, 4, 0.4, 0.5}, {0, 5, 0.5, 0.6}};
    for (const fl::TimestampedSegment &s : fl::ParaformerManager::segments({"\xE2\x96\x81he", "llo", "cu@@", "t", "\xE2\x96\x81", "x@@"}, raw))
        std::printf("SEG %016llx %016llx %s\n", bits(s.startTime), bits(s.endTime), s.text.c_str());
    return 0;
}

static int cif(int T, int D) {
    fl::Context ctx(0);
    Lcg g;
    fl::ParaformerCif::Rows rows(static_cast<size_t>(T), std::vector<float>(static_cast<size_t>(D)));
    std::vector<float> alphas(static_cast<size_t>(T));
    for (auto &row : rows)
        for (float &v : row) v = static_cast<float>(g.next(2001) - 1000) / 250.0f;
    for (float &a : alphas) a = static_cast<float>(g.next(500)) / 1000.0f;
    const fl::ParaformerCif::Fired f = fl::ParaformerCif::integrateAndFireWithFireFrames(ctx, rows, alphas);
    std::printf("FIRES");
    for (const int t : f.fireFrames) std::printf(" %d", t);
    std::printf("\n");
    for (const auto &e : f.embeds) {
        std::printf("EMBED");
        for (const float v : e) std::printf(" %08x", bits(v));
        std::printf("\n");
    }
    std::printf("NONE %zu %zu\n", fl::ParaformerCif::integrateAndFire(ctx, {}, {}).size(), fl::ParaformerCif::integrateAndFire(ctx, rows, alphas).size());
    return 0;
}

static int stamps(int T) {
    fl::Context ctx(0);
    Lcg g;
    std::vector<float> alphas(static_cast<size_t>(T));
    for (float &a : alphas) a = static_cast<float>(g.next(450)) / 1000.0f;
    // 60 ms of audio per frame: bursts of 0.1 s every 0.2 s over a noise floor
    std::vector<float> audio(static_cast<size_t>(T) * 960);
    for (size_t i = 0; i < audio.size(); ++i) {
        const float noise = static_cast<float>(g.next(21) - 10) / 100000.0f, burst = static_cast<float>(g.next(2001) - 1000) / 4000.0f;
        audio[i] = (i / 1600) % 2 == 0 ? burst : noise;
    }
    const fl::ParaformerManager::Vocabulary vocab = {{0, "<blank>"}, {1, "<s>"}, {2, "</s>"}, {3, "\xE2\x96\x81he"}, {4, "llo"}, {5, "cu@@"}, {6, "t"}, {7, "\xE2\x96\x81"}, {8, ""}};
    const std::vector<int> ids = {1, 3, 4, 0, 5, 6, 7, 8, 40, 4, 5, 6, 3, 2};
    for (const fa_paraformer_span &s : fl::ParaformerManager::rawSpans(ctx.handle(), ids, vocab, alphas, audio))
        std::printf("SPAN %d %d %016llx %016llx\n", s.utterance, s.token_index, bits(s.start), bits(s.end));
    for (const fl::TimestampedSegment &s : fl::ParaformerManager::decodeWithTimestamps(ctx, ids, vocab, alphas, audio))
        std::printf("SEG %016llx %016llx %s\n", bits(s.startTime), bits(s.endTime), s.text.c_str());
    std::printf("EMPTY %zu %zu\n", fl::ParaformerManager::decodeWithTimestamps(ctx, {0, 1, 2}, vocab, alphas, audio).size(),
                fl::ParaformerManager::decodeWithTimestamps(ctx, {}, vocab, alphas, audio).size());
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
        if (argc == 4 && !std::strcmp(argv[1], "cif")) return cif(std::atoi(argv[2]), std::atoi(argv[3]));
        if (argc == 3 && !std::strcmp(argv[1], "stamps")) return stamps(std::atoi(argv[2]));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
