// A C++ host of fluidaudio::OfflineEmbeddingPlanner (include/fluidaudio.hpp), driven by tests/test_cabi_embedding.py:
//   embedding_host <file>   plan() on the device
// <file>: whitespace-separated "C F S W batch skip threshold exclude total nOffsets", the weights [C][F][S], the offsets.
// Output: "REC chunk speaker first last startbits endbits run" per job, "WIN chunk start" per planned window, "RUN window rowbits..." per
// run, "MASK bits..." per job, "INFO evaluated empty fallback skipped"; floats / doubles as hex bits.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "fluidaudio.hpp"

static unsigned bitsOf(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static unsigned long long bitsOfD(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: embedding_host <file>\n"); return 2; }
    std::ifstream in(argv[1]);
    int64_t C, F, S, W, batch, skip, exclude, total, nOff;
    float threshold;
    in >> C >> F >> S >> W >> batch >> skip >> threshold >> exclude >> total >> nOff;
    std::vector<std::vector<std::vector<float>>> w(C, std::vector<std::vector<float>>(F, std::vector<float>(S)));
    for (auto &chunk : w) for (auto &frame : chunk) for (float &v : frame) in >> v;
    std::vector<double> offsets(nOff);
    for (double &o : offsets) in >> o;
    if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
    fa_embedding_config cfg = fluidaudio::OfflineEmbeddingPlanner::defaultConfig();
    cfg.weight_frames = static_cast<int32_t>(W);
    cfg.batch_size = static_cast<int32_t>(batch);
    cfg.skip_enabled = static_cast<int32_t>(skip);
    cfg.skip_threshold = threshold;
    cfg.exclude_overlap = static_cast<int32_t>(exclude);
    fluidaudio::OfflineEmbeddingPlanner::Plan p;
    try {
        fluidaudio::Context ctx(0);
        p = fluidaudio::OfflineEmbeddingPlanner(cfg).plan(ctx, w, offsets, total, 0.0, true);
    } catch (const std::exception &e) {
        std::printf("ERROR %s\n", e.what());
        return 1;
    }
    for (size_t j = 0; j < p.records.size(); ++j) {
        const fa_export_embedding &r = p.records[j];
        std::printf("REC %d %d %d %d %016llx %016llx %d\n", r.chunk_index, r.speaker_index, r.start_frame, r.end_frame, bitsOfD(r.start_time),
                    bitsOfD(r.end_time), p.runOfJob[j]);
    }
    for (size_t i = 0; i < p.windowStart.size(); ++i) std::printf("WIN %d %" PRId64 "\n", p.windowChunk[i], p.windowStart[i]);
    for (size_t r = 0; r < p.runWeights.size(); ++r) {
        std::printf("RUN %d", p.windowOfRun[r]);
        for (float v : p.runWeights[r]) std::printf(" %08x", bitsOf(v));
        std::printf("\n");
    }
    for (const auto &m : p.frameWeights) {
        std::printf("MASK");
        for (float v : m) std::printf(" %08x", bitsOf(v));
        std::printf("\n");
    }
    std::printf("INFO %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", p.info.evaluated_masks, p.info.empty_masks, p.info.fallback_masks,
                p.info.skipped_embeddings);
    return 0;
}
