// A C++ caller of AedConfig / AedLongForm / CoherePipeline / CanaryManager (include/fluidaudio.hpp) and of the fa_aed_* entries, built with
// -Wall -Wextra -Werror by tests/test_cabi_aed.py.  Without an argument no device is touched: the defaults, the host integer functions, the
// window plan and every refusal.  With "merge" the seam merge runs on the device, on groups of recordings read from stdin (one window
// per line).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fluidaudio.hpp"

using namespace fluidaudio;

static void show(const char *tag, const AedConfig &a) {
    std::printf("%s %d %d %d %d %d %d %g %d %d %lld %lld %d %lld\n", tag, a.mode, a.vocab, a.eosId, a.maxSeq, a.maxNew, a.noRepeatNgram, static_cast<double>(a.repetitionPenalty),
                a.windowTokens, a.minMatch, static_cast<long long>(a.chunkSamples), static_cast<long long>(a.hopSamples), a.maxOut(), static_cast<long long>(a.stateBytes(3)));
}

static int merge_on_device() {
    Context ctx(0);
    std::string line;
    while (std::getline(std::cin, line)) {               // "group <windowTokens> <minMatch>", then windows, "end" after a recording, "run" after the group
        int windowTokens = 32, minMatch = 4;
        std::string word;
        std::istringstream(line) >> word >> windowTokens >> minMatch;
        std::vector<std::vector<std::vector<int32_t>>> recordings(1);
        while (std::getline(std::cin, line) && line != "run") {
            if (line == "end") { recordings.emplace_back(); continue; }
            std::istringstream in(line);
            std::vector<int32_t> w;
            for (int32_t t; in >> t;) w.push_back(t);
            recordings.back().push_back(w);
        }
        recordings.pop_back();
        for (const auto &m : AedLongForm::mergeRecordings(ctx, recordings, windowTokens, minMatch)) {
            std::printf("MERGED");
            for (const int32_t t : m) std::printf(" %d", t);
            std::printf("\n");
        }
    }
    std::printf("ONE");
    for (const int32_t t : CoherePipeline::mergeTokenStreams(ctx, {1, 2, 3, 7, 8, 9, 10}, {7, 8, 9, 10, 11, 12})) std::printf(" %d", t);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "merge") == 0) return merge_on_device();

    show("COHERE", AedConfig::cohere());
    show("CANARY", AedConfig::canary());
    show("PLAIN", AedConfig());
    fa_aed_config raw;
    fa_aed_default_config(&raw, 7);      // an unknown model: Cohere
    fa_aed_default_config(nullptr, 0);
    std::printf("RAW %d %d %zu\n", raw.mode, raw.max_seq, sizeof(fa_aed_config));
    AedConfig small;
    small.maxSeq = 16; small.maxNew = 4;
    AedConfig bad;
    bad.vocab = 0;
    std::printf("SIZES %d %lld %d %lld %d %lld\n", small.maxOut(), static_cast<long long>(small.stateBytes(2)), bad.maxOut(), static_cast<long long>(bad.stateBytes(2)),
                fa_aed_max_out(nullptr), static_cast<long long>(AedConfig().stateBytes(0)));
    std::printf("VALID");
    for (const long long f : {0LL, 1LL, 8LL, 1000LL, 3499LL, 3500LL, 9000LL}) std::printf(" %d", CoherePipeline::encoderValidFrames(f, 438));
    std::printf(" %d %d %d %d\n", CoherePipeline::encoderValidFrames(3500, 400), CoherePipeline::encoderValidFrames(10, 5, 0, 3), CoherePipeline::encoderValidFrames(-1, 5),
                CoherePipeline::encoderValidFrames(5, 9, 7, 3));
    std::printf("DYNAMIC %zu %zu\n", CoherePipeline::buildDynamicSelfAttentionMask(4).size(), CoherePipeline::buildDynamicSelfAttentionMask(0).size());
    const std::vector<int64_t> samples = {0, 560000, 560001, 1040000, 1040001, 240000, 300000, 432001};
    for (int model = 0; model < 2; ++model) {
        const auto plans = model == 0 ? CoherePipeline::planWindows(samples) : CanaryManager::planWindows(samples);
        for (size_t r = 0; r < plans.size(); ++r) {
            std::printf("PLAN %d %lld", model, static_cast<long long>(samples[r]));
            for (const auto &w : plans[r]) std::printf(" %lld %lld", static_cast<long long>(w.start), static_cast<long long>(w.length));
            std::printf("\n");
        }
    }
    int thrown = 0;
    AedConfig noHop;
    noHop.hopSamples = 0;
    try { AedLongForm::planWindows(noHop, samples); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    try { AedLongForm::planWindows(AedConfig(), {5, -1}); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    std::printf("THROWN %d\n", thrown);

    // every refusal of the entries is a status, answered without a device (no context exists here)
    const fa_aed_config ok = AedConfig().c(), seq = AedConfig::canary().c();
    int32_t lens[2] = {1, 2}, zero[2] = {1, 0}, word = 0, counts[2];
    int64_t range[3], count = -7, two[2] = {5, 700000}, starts[1], lengths[1];
    void *p = &word;
    int32_t *q = &word;
    float f = 0.0f;
    std::printf("ST begin %d %d %d %d\n", fa_aed_begin_dev(nullptr, &ok, 2, q, 2, lens, p, q, q, nullptr, 0, nullptr, nullptr), fa_aed_begin_dev(nullptr, &ok, 2, q, 2, zero, p, q, q, nullptr, 0, nullptr, nullptr),
                fa_aed_begin_dev(nullptr, nullptr, 2, q, 2, lens, p, q, q, nullptr, 0, nullptr, nullptr), fa_aed_begin_dev(nullptr, &seq, 2, q, 2, lens, p, nullptr, nullptr, nullptr, 0, nullptr, &f));
    std::printf("ST step %d %d %d %d\n", fa_aed_step_dev(nullptr, &ok, 1, p, p, FA_DTYPE_F32, 16384, q, q, nullptr, 0, nullptr, nullptr), fa_aed_step_dev(nullptr, &ok, 1, p, p, FA_DTYPE_F32, 16383, q, q, nullptr, 0, nullptr, nullptr),
                fa_aed_step_dev(nullptr, &ok, 1, p, p, 5, 16384, q, q, nullptr, 0, nullptr, nullptr), fa_aed_step_dev(nullptr, &seq, 1, p, p, FA_DTYPE_F16, 16384, nullptr, nullptr, nullptr, 0, q, nullptr));
    std::printf("ST finish %d %d %d %d\n", fa_aed_finish(nullptr, &ok, 1, p, 108, q, q, nullptr, nullptr), fa_aed_finish(nullptr, &ok, 1, p, 107, q, q, nullptr, nullptr),
                fa_aed_finish_dev(nullptr, &ok, 1, nullptr, 108, q, q, nullptr, nullptr), fa_aed_finish_dev(nullptr, &ok, 0, p, 108, q, q, nullptr, nullptr));
    std::printf("ST masks %d %d %d %d %d %d\n", fa_aed_cross_mask_dev(nullptr, q, 1, 438, FA_DTYPE_F16, p), fa_aed_cross_mask_dev(nullptr, q, 1, 0, FA_DTYPE_F16, p), fa_aed_cross_mask_dev(nullptr, q, 1, 438, 3, p),
                fa_aed_encoder_context_dev(nullptr, p, FA_DTYPE_F32, 1, 1024, 188, 1024 * 192, 192, 1, q, &f, &f), fa_aed_encoder_context_dev(nullptr, p, FA_DTYPE_F32, 1, 0, 188, 0, 192, 1, q, &f, &f),
                fa_aed_encoder_context_dev(nullptr, p, FA_DTYPE_F32, 1, 1024, 188, 0, 192, 1, nullptr, &f, &f));
    std::printf("ST gather %d %d %d\n", fa_aed_gather_hidden_dev(nullptr, &seq, 1, p, p, FA_DTYPE_F32, 128, 1024, 0, 1024, 1, &f), fa_aed_gather_hidden_dev(nullptr, &ok, 1, p, p, FA_DTYPE_F32, 128, 1024, 0, 1024, 1, &f),
                fa_aed_gather_hidden_dev(nullptr, &seq, 1, p, p, FA_DTYPE_F32, 0, 1024, 0, 1024, 1, &f));
    const fa_status counted = fa_aed_plan_windows(&ok, two, 2, range, nullptr, nullptr, 0, &count);
    const fa_status tooSmall = fa_aed_plan_windows(&ok, two, 2, range, starts, lengths, 1, &count);
    std::printf("ST plan %d %d %lld %lld", counted, tooSmall, static_cast<long long>(count), static_cast<long long>(range[2]));
    std::printf(" %d %d\n", fa_aed_plan_windows(nullptr, two, 2, range, nullptr, nullptr, 0, &count), fa_aed_plan_windows(&ok, two, 2, range, nullptr, nullptr, 0, nullptr));
    const int64_t woff[3] = {0, 2, 4}, rr[2] = {0, 2}, room[2] = {0, 4}, tight[2] = {0, 3};
    fa_aed_config wide = ok;
    wide.window_tokens = 65;
    std::printf("ST merge %d %d %d %d %d\n", fa_aed_merge_windows(nullptr, &ok, q, woff, rr, 1, q, room, counts, nullptr, nullptr), fa_aed_merge_windows(nullptr, &ok, q, woff, rr, 1, q, tight, counts, nullptr, nullptr),
                fa_aed_merge_windows(nullptr, &wide, q, woff, rr, 1, q, room, counts, nullptr, nullptr), fa_aed_merge_windows_dev(nullptr, &ok, q, nullptr, rr, 1, q, room, counts, nullptr, nullptr),
                fa_aed_merge_windows_dev(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    return 0;
}
