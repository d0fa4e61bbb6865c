// A C++ host of fluidaudio::OfflineReconstruction (include/fluidaudio.hpp), driven by tests/test_cabi_reconstruct.py:
//   reconstruct_host db <file>        buildSpeakerDatabase only (host code, no GPU)
//   reconstruct_host segments <file>  build(): buildSegments on the device + buildSpeakerDatabase
// <file>: whitespace-separated "C F S K D fd minSegment minGap exclusive nOffsets nHardRows nSegments", the weights [C][F][S], the
// offsets, the hard-cluster rows (each its length, then its entries: a ragged [[Int]]), the centroids [K][D], and for `db` the
// segments as "id start end quality".  Output: "SEG <id> <start> <end> <quality>" and "DB <id> <values>", floats as hex bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "fluidaudio.hpp"

static unsigned bitsOf(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: reconstruct_host db|segments <file>\n"); return 2; }
    const std::string mode = argv[1];
    std::ifstream in(argv[2]);
    int64_t C, F, S, K, D, nOff, nHard, nSeg;
    double fd, minSeg, minGap;
    int exclusive;
    in >> C >> F >> S >> K >> D >> fd >> minSeg >> minGap >> exclusive >> nOff >> nHard >> nSeg;
    std::vector<std::vector<std::vector<float>>> w(C, std::vector<std::vector<float>>(F, std::vector<float>(S)));
    for (auto &chunk : w) for (auto &frame : chunk) for (float &v : frame) in >> v;
    std::vector<double> offsets(nOff);
    for (double &o : offsets) in >> o;
    std::vector<std::vector<int>> hard(nHard);
    for (auto &row : hard) { int64_t n; in >> n; row.resize(n); for (int &k : row) in >> k; }
    fluidaudio::Matrix centroids(K, std::vector<double>(D));
    for (auto &row : centroids) for (double &v : row) in >> v;
    if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
    fa_reconstruct_config cfg = fluidaudio::OfflineReconstruction::defaultConfig();
    cfg.frame_duration = fd;
    cfg.min_segment_duration = minSeg;
    cfg.min_gap_duration = minGap;
    cfg.exclusive = exclusive;
    fluidaudio::OfflineReconstruction::Result r;
    try {
        if (mode == "db") {
            for (int64_t i = 0; i < nSeg; ++i) {
                fa_rttm_segment s{};
                std::string id;
                in >> id >> s.start_seconds >> s.end_seconds >> s.quality;
                std::snprintf(s.speaker_id, sizeof(s.speaker_id), "%s", id.c_str());
                r.segments.push_back(s);
            }
            r.speakerDatabase = fluidaudio::OfflineReconstruction::buildSpeakerDatabase(r.segments, centroids);
        } else {
            fluidaudio::Context ctx(0);
            r = fluidaudio::OfflineReconstruction(cfg).build(ctx, w, offsets, hard, centroids);
        }
    } catch (const std::exception &e) {
        std::printf("ERROR %s\n", e.what());
        return 1;
    }
    for (const auto &s : r.segments) std::printf("SEG %s %08x %08x %08x\n", s.speaker_id, bitsOf(s.start_seconds), bitsOf(s.end_seconds), bitsOf(s.quality));
    for (const auto &kv : r.speakerDatabase) {
        std::printf("DB %s", kv.first.c_str());
        for (float v : kv.second) std::printf(" %08x", bitsOf(v));
        std::printf("\n");
    }
    return 0;
}
