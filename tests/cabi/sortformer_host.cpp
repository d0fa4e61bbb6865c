// A C++ caller of the offline Sortformer / timeline mirrors of include/fluidaudio.hpp (built with -Wall -Wextra -Werror by
// tests/test_cabi_sortformer.py).
//   sortformer_host host <file>      no GPU needed: window geometry, stitcher alignment, the seconds initialiser, statuses
//   sortformer_host timeline <file>  DiarizerTimeline::rebuild on the device
// Floats are printed as their bit patterns.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

static int host(std::istream &in) {
    fl::OfflineSortformerConfig cfg;
    size_t n = 0;
    in >> cfg.windowOutputFrames >> cfg.subsamplingFactor >> cfg.overlapOutputFrames >> n;
    std::vector<int64_t> lengths(n);
    for (auto &v : lengths) in >> v;
    const auto w = cfg.windows(lengths);
    for (const auto &x : w.windows)
        std::printf("WIN %d %d %d %d %lld %lld\n", x.recording, x.valid_mel, x.valid_out, x.first, (long long)x.mel_start, (long long)x.g_start);
    for (size_t b = 0; b < n; ++b) std::printf("REC %lld %lld %lld\n", (long long)w.totalOut[b], (long long)w.windowRange[b], (long long)w.windowRange[b + 1]);
    std::printf("CFG %d %08x\n", cfg.windowMelFrames(), bits(cfg.frameDurationSeconds()));
    int frames = 0, speakers = 0;
    while (in >> frames >> speakers) {
        std::vector<float> g(static_cast<size_t>(frames) * speakers), x(g.size());
        for (auto &v : g) in >> v;
        for (auto &v : x) in >> v;
        std::printf("MAP");
        for (int m : fl::SortformerSpeakerStitcher::alignment(g, x, frames, speakers)) std::printf(" %d", m);
        std::printf("\n");
    }
    const auto t = fl::DiarizerTimelineConfig::fromSeconds(1, 0.08f, 0.5f, 0.5f, 0.12f, 0.2f, 0.04f, 0.36f);
    std::printf("SEC %d %d %d %d\n", t.onsetPadFrames, t.offsetPadFrames, t.minFramesOn, t.minFramesOff);
    // statuses: nothing here may throw or crash without a device
    fa_sortformer_offline_config c = cfg.c();
    int64_t cnt = 0;
    const int64_t bad = -1;
    std::printf("ST %d %d %d\n", (int)fa_sortformer_offline_windows(nullptr, lengths.data(), 1, nullptr, 0, &cnt, nullptr, nullptr),
                (int)fa_sortformer_offline_windows(&c, &bad, 1, nullptr, 0, &cnt, nullptr, nullptr),
                (int)fa_sortformer_stitch_dev(nullptr, &c, nullptr, lengths.data(), 1, 0, nullptr, nullptr));
    fa_timeline_config tc = t.c();
    std::printf("ST %d %d\n", (int)fa_timeline_segments_dev(nullptr, &tc, nullptr, nullptr, nullptr, nullptr, 0, 1, nullptr, 0, &cnt, nullptr),
                (int)fa_sortformer_pack_windows_dev(nullptr, &c, nullptr, 0, 0, 0, lengths.data(), 1, 0, nullptr, nullptr));
    try {
        fl::SortformerSpeakerStitcher::alignment(std::vector<float>(10), std::vector<float>(10), 2, 5);
        std::printf("ST none\n");
    } catch (const fl::Error &e) {
        std::printf("ST %d\n", (int)e.status);
    }
    return 0;
}

static int timeline(std::istream &in) {
    fl::DiarizerTimelineConfig cfg;
    size_t nf = 0, nt = 0;
    int complete = 1;
    in >> cfg.numSpeakers >> cfg.onsetThreshold >> cfg.offsetThreshold >> cfg.onsetPadFrames >> cfg.offsetPadFrames >> cfg.minFramesOn >> cfg.minFramesOff >>
        complete >> nf >> nt;
    std::vector<float> fin(nf * cfg.numSpeakers), tent(nt * cfg.numSpeakers);
    for (auto &v : fin) in >> v;
    for (auto &v : tent) in >> v;
    fl::Context ctx(0);
    for (const auto &s : fl::DiarizerTimeline(cfg).rebuild(ctx, fin, tent, complete != 0))
        std::printf("SEG %d %lld %lld %08x %d %08x %08x\n", s.speakerIndex, (long long)s.startFrame, (long long)s.endFrame, bits(s.activity), s.isFinalized ? 1 : 0,
                    bits(s.startTime()), bits(s.endTime()));
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[2]);
    if (!in) return 2;
    try {
        if (!std::strcmp(argv[1], "host")) return host(in);
        if (!std::strcmp(argv[1], "timeline")) return timeline(in);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
