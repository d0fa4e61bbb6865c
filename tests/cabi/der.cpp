// A C++ caller of DiarizationDER::compute (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by tests/test_cabi_der.py.
//   der args                        no GPU needed: every argument error is a status / an Error, nothing crashes
//   der score <step> <collar>       the two-speaker case of tests/test_der_cpu.py on the device
// Doubles are printed as their bit patterns.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "fluidaudio.hpp"

namespace fl = fluidaudio;

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

static int status_of(const std::vector<fl::DERSpeakerSegment> &ref, const std::vector<fl::DERSpeakerSegment> &hyp, double step, double collar) {
    try {
        fl::DiarizationDER::compute(static_cast<fa_ctx *>(nullptr), ref, hyp, step, collar);
    } catch (const fl::Error &e) {
        return static_cast<int>(e.status);
    }
    return 0;
}

static int args() {
    const std::vector<fl::DERSpeakerSegment> ok = {{"A", 0.0, 1.0}};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<fl::DERSpeakerSegment> many;
    for (int i = 0; i < 65; ++i) many.push_back({"s" + std::to_string(i), 0.0, 1.0});
    std::printf("ST %d %d %d %d %d %d %d\n", status_of({{"A", nan, 1.0}}, ok, 0.01, 0.0), status_of(ok, {{"x", 0.0, inf}}, 0.01, 0.0), status_of(ok, ok, 0.0, 0.0),
                status_of(ok, ok, -1.0, 0.0), status_of(ok, ok, 0.01, -0.5), status_of(many, ok, 0.01, 0.0), status_of(ok, ok, 0.01, 0.0));
    fa_der_config cfg;
    fa_der_default_config(&cfg);
    fa_der_default_config(nullptr);
    std::printf("CFG %016llx %016llx\n", bits(cfg.frame_step), bits(cfg.collar));
    std::printf("ST %d %d\n", (int)fa_der_score_batch(nullptr, &cfg, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0),
                (int)fa_der_score_batch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, 0));
    return 0;
}

static int score(double step, double collar) {
    fl::Context ctx(0);
    const std::vector<fl::DERSpeakerSegment> ref = {{"A", 0.0, 10.0}, {"B", 10.0, 20.0}}, hyp = {{"x", 0.0, 12.0}, {"y", 12.0, 20.0}};
    const fl::DERResult r = fl::DiarizationDER::compute(ctx, ref, hyp, step, collar);
    std::printf("DER %016llx %016llx %016llx %016llx %016llx\n", bits(r.der), bits(r.confusion), bits(r.falseAlarm), bits(r.miss), bits(r.totalRefSpeech));
    std::printf("CNT %lld %lld %lld %lld %lld %d %d\n", (long long)r.counts.frames, (long long)r.counts.miss, (long long)r.counts.false_alarm,
                (long long)r.counts.confusion, (long long)r.counts.ref, r.counts.ref_labels, r.counts.hyp_labels);
    for (const auto &kv : r.mapping) std::printf("MAP %s %s\n", kv.first.c_str(), kv.second.c_str());
    std::printf("OV");
    for (const int64_t v : r.overlap) std::printf(" %lld", (long long)v);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
        if (argc == 4 && !std::strcmp(argv[1], "score")) return score(std::atof(argv[2]), std::atof(argv[3]));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
