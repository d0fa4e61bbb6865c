// The host arithmetic of the embedding inputs (fluidaudio_amd/csrc/embedding_geom.h, the code embedding_host.hip plans with) driven over
// stdin: one command per line, numbers as scanf reads them (hex floats, nan, inf).  Test infrastructure: built by
// tests/test_embedding_geom.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   windows rate window_duration spw batch W fd_cfg min_seg F C total n_offsets offsets...
//       -> "spw W B fd min_frames nw", then nw lines "chunk start offset"
//   spans rate window_duration spw W total n (t0 t1)...   -> n lines "ok start len active"
//   slice start total                                       -> "0" or "1"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/embedding_geom.h"

using namespace fa::embedding;

static bool config(fa_embedding_config &cfg, bool full) {
    memset(&cfg, 0, sizeof(cfg));
    cfg.overlap_threshold = 1e-3f;
    cfg.min_segment_duration = 1.0;
    cfg.batch_size = 32;
    if (scanf("%d %lf %d", &cfg.sample_rate, &cfg.window_duration, &cfg.samples_per_window) != 3) return false;
    if (full && scanf("%d %d %lf %lf", &cfg.batch_size, &cfg.weight_frames, &cfg.frame_duration, &cfg.min_segment_duration) != 4) return false;
    if (!full && scanf("%d", &cfg.weight_frames) != 1) return false;
    return config_ok(&cfg);
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        fa_embedding_config cfg;
        if (!strcmp(cmd, "windows")) {
            int32_t F;
            int64_t C, total, n_off;
            if (!config(cfg, true) || scanf("%d %" SCNd64 " %" SCNd64 " %" SCNd64, &F, &C, &total, &n_off) != 4) return 2;
            std::vector<double> off(static_cast<size_t>(n_off));
            for (double &v : off) if (scanf("%lf", &v) != 1) return 2;
            const Geometry g = geometry(cfg, F);
            const Windows w = plan_windows(cfg, g, C, off.data(), n_off, total);
            printf("%d %d %d %a %d %zu\n", g.spw, g.W, g.B, g.fd, g.min_frames, w.chunk.size());
            for (size_t i = 0; i < w.chunk.size(); ++i) printf("%d %" PRId64 " %a\n", w.chunk[i], w.start[i], w.offset[i]);
        } else if (!strcmp(cmd, "spans")) {
            int64_t total, n;
            if (!config(cfg, false) || scanf("%" SCNd64 " %" SCNd64, &total, &n) != 2) return 2;
            const Geometry g = geometry(cfg, 0);
            for (int64_t i = 0; i < n; ++i) {
                double t0, t1;
                if (scanf("%lf %lf", &t0, &t1) != 2) return 2;
                const Span s = span_geometry(t0, t1, cfg.sample_rate, g, total);
                printf("%d %" PRId64 " %" PRId64 " %d\n", s.ok ? 1 : 0, s.start, s.len, s.active);
            }
        } else if (!strcmp(cmd, "slice")) {
            int64_t start, total;
            if (scanf("%" SCNd64 " %" SCNd64, &start, &total) != 2) return 2;
            printf("%d\n", slice_ok(start, total) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
