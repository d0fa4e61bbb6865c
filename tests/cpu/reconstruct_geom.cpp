// The host arithmetic of the reconstruction (fluidaudio_amd/csrc/reconstruct_geom.h, the code reconstruct_host.hip plans with) driven over
// stdin: one plan per command, numbers as scanf reads them (hex floats, nan, inf).  Test infrastructure: built by
// tests/test_reconstruct_geom.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   plan C F S K fd_cfg window n_offsets offsets... has_hard [C*S labels] n_overrides (lo hi k)...
//       -> "error index frames fd", then (error 0 or 3) "sorted T Kc maxc smax", then (error 0) the lines start, first_g, last_g, hard, ovr
//   masks -> powerset_mask(0..7)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/reconstruct_geom.h"

using namespace fa::reconstruct;

template <class T>
static void line(const std::vector<T> &v, const char *fmt) {
    for (const T &x : v) printf(fmt, x);
    printf("\n");
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "masks")) {
            for (int c = 0; c < 8; ++c) printf("%u ", powerset_mask(c));
            printf("\n");
            continue;
        }
        if (strcmp(cmd, "plan")) return 2;
        int64_t C, n_off, n_ovr;
        int32_t F, S, K, has_hard;
        double fd_cfg, window;
        if (scanf("%" SCNd64 " %d %d %d %lf %lf %" SCNd64, &C, &F, &S, &K, &fd_cfg, &window, &n_off) != 7) return 2;
        std::vector<double> off(static_cast<size_t>(n_off));
        for (double &v : off) if (scanf("%lf", &v) != 1) return 2;
        if (scanf("%d", &has_hard) != 1) return 2;
        std::vector<int32_t> hard(has_hard ? static_cast<size_t>(C * S) : 0);
        for (int32_t &v : hard) if (scanf("%d", &v) != 1) return 2;
        if (scanf("%" SCNd64, &n_ovr) != 1) return 2;
        std::vector<int64_t> ovr(static_cast<size_t>(3 * n_ovr));
        for (int64_t &v : ovr) if (scanf("%" SCNd64, &v) != 1) return 2;
        const double fd = frame_duration(fd_cfg, window, F);
        const FramePlan p = frame_plan(C, F, S, K, fd, window, off.data(), n_off, has_hard ? hard.data() : nullptr, ovr.data(), n_ovr);
        printf("%d %" PRId64 " %a %a\n", static_cast<int>(p.error), p.index, p.frames, fd);
        if (p.error != PlanError::kNone && p.error != PlanError::kOverride) continue;
        printf("%d %d %d %d %d\n", p.sorted ? 1 : 0, p.T, p.Kc, p.maxc, p.smax);
        if (p.error != PlanError::kNone) continue;
        line(p.start, "%a ");
        line(p.first_g, "%d ");
        line(p.last_g, "%d ");
        line(p.hard, "%d ");
        line(p.ovr, "%d ");
    }
    return 0;
}
