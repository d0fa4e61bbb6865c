// A C++ caller of fa_tdt_merge_windows(_dev) and ChunkProcessor (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by
// tests/test_cabi_tdt_merge.py.
//   tdt_merge args           no GPU needed: every argument error is a status / an Error, nothing crashes, nothing is written
//   tdt_merge merge          two of the reference's literal cases through ChunkProcessor, on the device
#include <cmath>
#include <cstdio>
#include <cstring>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;

static int32_t tok[8] = {1, 2, 3, 4, 5, 6, 7, 8}, cnt[2] = {2, 2};
static float conf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static int32_t o_tok[8], o_cnt[2], o_st[2], o_rt[2];
static float o_conf[8];

static int call(const fa_tdt_merge_config *cfg, const int32_t *t, const int32_t *c, int32_t max_out, const int64_t *wr, int64_t n, int32_t vocab, int32_t *out,
                const int64_t *orng, int32_t *counts, int32_t *statuses, bool dev = false) {
    return static_cast<int>((dev ? fa_tdt_merge_windows_dev : fa_tdt_merge_windows)(nullptr, cfg, t, t, t, conf, c, max_out, wr, n, nullptr, nullptr, vocab, out, out, out, o_conf,
                                                                                    orng, counts, statuses, o_rt));
}

static int args() {
    const int64_t ok[2] = {0, 2}, down[2] = {2, 0}, below[2] = {-1, 2}, out_ok[2] = {0, 6}, huge[2] = {0, int64_t{1} << 31};
    std::memset(o_tok, 0x55, sizeof(o_tok));
    std::memset(o_cnt, 0x55, sizeof(o_cnt));
    std::memset(o_st, 0x55, sizeof(o_st));
    std::memset(o_rt, 0x55, sizeof(o_rt));
    fa_tdt_merge_config d;
    fa_tdt_merge_default_config(&d);
    fa_tdt_merge_default_config(nullptr);
    std::printf("CFG %d %d\n", d.frame_seconds == 1280.0 / 16000.0, d.overlap_seconds == 2.0);
    fa_tdt_merge_config neg = d, zero = d, nan = d;
    neg.overlap_seconds = -1.0;
    zero.frame_seconds = 0.0;
    nan.overlap_seconds = std::nan("");
    // a well-formed call without a context ends in INVALID_ARGUMENT too; zero recordings without a context as well
    std::printf("ST %d %d %d\n", call(&d, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st), call(nullptr, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st, true),
                call(nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr));
    std::printf("ST %d %d %d %d %d %d %d %d %d %d %d %d %d\n", call(&d, tok, cnt, 4, ok, -1, 0, o_tok, out_ok, o_cnt, o_st), call(&d, tok, cnt, 4, nullptr, 1, 0, o_tok, out_ok, o_cnt, o_st),
                call(&d, tok, cnt, 4, ok, 1, 0, o_tok, nullptr, o_cnt, o_st), call(&d, tok, cnt, 4, down, 1, 0, o_tok, out_ok, o_cnt, o_st),
                call(&d, tok, cnt, 4, ok, 1, 0, o_tok, down, o_cnt, o_st, true), call(&d, tok, cnt, 4, below, 1, 0, o_tok, out_ok, o_cnt, o_st),
                call(&d, nullptr, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st), call(&d, tok, nullptr, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st),
                call(&d, tok, cnt, 4, ok, 1, 0, nullptr, out_ok, o_cnt, o_st), call(&d, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, nullptr, o_st),
                call(&d, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, nullptr), call(&d, tok, cnt, -1, ok, 1, 0, o_tok, out_ok, o_cnt, o_st),
                call(&d, tok, cnt, 4, ok, 1, -1, o_tok, out_ok, o_cnt, o_st));
    std::printf("ST %d %d %d\n", call(&neg, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st), call(&zero, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st),
                call(&nan, tok, cnt, 4, ok, 1, 0, o_tok, out_ok, o_cnt, o_st));
    std::printf("ST %d %d\n", call(&d, tok, cnt, 4, ok, 1, 0, o_tok, huge, o_cnt, o_st), call(&d, tok, cnt, 4, ok, INT32_MAX, 0, o_tok, out_ok, o_cnt, o_st));
    int untouched = 1;
    const auto same = [&untouched](const void *p, size_t n) { for (size_t i = 0; i < n; ++i) untouched &= static_cast<const unsigned char *>(p)[i] == 0x55; };
    same(o_tok, sizeof(o_tok)); same(o_cnt, sizeof(o_cnt)); same(o_st, sizeof(o_st)); same(o_rt, sizeof(o_rt));
    std::printf("OUT %d\n", untouched);
    int thrown = 0;
    try {
        fl::ChunkProcessor cp;
        cp.mergeRecording(static_cast<fa_ctx *>(nullptr), {{{1, 2, 1, 0.5f}}, {{1, 2, 1, 0.5f}}});
    } catch (const fl::Error &e) {
        thrown = static_cast<int>(e.status);
    }
    std::printf("THROWN %d\n", thrown);
    return 0;
}

static void print(const char *tag, const fl::ChunkProcessor::Merged &m) {
    std::printf("%s %d", tag, static_cast<int>(m.status));
    for (const auto &t : m.tokens) std::printf(" %d@%d", t.token, t.timestamp);
    std::printf(" |");
    for (const int32_t r : m.seamRoutes) std::printf(" %d", r);
    std::printf("\n");
}

static int merge() {
    fl::Context ctx(0);
    using W = fl::ChunkProcessor::Window;
    // testPostMatchTailAdoptsRightSegmentationOfSeamWord and testMidpointMergeLegacyBehaviorWithoutVocabulary (ChunkProcessorTests.swift:636-664, 768-786)
    const W left = {{10, 120, 1, 0.98f}, {24, 130, 1, 0.97f}, {25, 131, 1, 0.96f}, {26, 132, 1, 0.95f}};
    const W right = {{27, 130, 1, 0.97f}, {25, 131, 1, 0.96f}, {28, 132, 1, 0.95f}, {30, 134, 1, 0.97f}};
    fl::ChunkProcessor cp;
    cp.hasSpliceSafe = true;
    cp.spliceSafe.assign(64, 0);
    for (const int id : {10, 20, 24, 27, 30, 40, 60}) cp.spliceSafe[static_cast<size_t>(id)] = 1;
    print("ADOPT", cp.mergeRecording(ctx, {left, right}));
    const W ml = {{10, 120, 1, 0.98f}, {20, 133, 1, 0.97f}, {21, 135, 1, 0.96f}}, mr = {{60, 134, 1, 0.90f}, {50, 136, 1, 0.91f}, {30, 138, 1, 0.97f}};
    const fl::ChunkProcessor legacy;
    const auto both = legacy.mergeRecordings(ctx.handle(), {{ml, mr}, {}, {ml}});
    print("MIDPOINT", both[0]);
    print("NONE", both[1]);
    print("ONE", both[2]);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
        if (argc == 2 && !std::strcmp(argv[1], "merge")) return merge();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
