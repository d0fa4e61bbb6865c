// The shared integer arithmetic of the TDT window planner (fluidaudio_amd/csrc/tdt_plan_core.h, the same text the GPU compiles) and the
// geometry of tdt_plan_launch.h, walked on the host the way the kernel tp_count / tp_write walks it: 64 windows a pass, every turn of the
// loop on its own, the first ending window of a pass found as a ballot would find it.  Built by tests/test_tdt_plan_core_emul.py with g++.
#include <cstdint>

#include "../../fluidaudio_amd/csrc/tdt_plan_launch.h"

namespace tp = fa::tdt_plan;

extern "C" {

// 0 and the four layout values, or the refusal's status
int tp_emul_layout(const fa_tdt_window_config *cfg, int64_t *out) {
    tp::Geometry g{};
    const fa::Verdict v = tp::derive(*cfg, &g);
    if (v.status != FA_SUCCESS) return v.status;
    out[0] = g.chunk; out[1] = g.stride; out[2] = g.mel_context; out[3] = g.warmup_prefix;
    out[4] = g.silence_radius; out[5] = g.valley_radius; out[6] = g.lookahead; out[7] = g.stable_quiet; out[8] = g.probe_window; out[9] = g.aligned;
    return 0;
}

int64_t tp_emul_last_chunk_warmup(int64_t chunk_start, int64_t default_warmup, int64_t chunk, int64_t total, int64_t speech_end, int64_t frame) {
    return tp::last_chunk_warmup(chunk_start, default_warmup, chunk, total, speech_end, frame);
}

int64_t tp_emul_bound(const fa_tdt_window_config *cfg, int64_t n) {
    tp::Geometry g{};
    return tp::derive(*cfg, &g).status == FA_SUCCESS ? tp::window_count_bound(g, n) : -1;
}

// The windows of one recording from its listed starts (start << 1 | useWarmupPrefix); returns their number, writes at most `capacity`.
int64_t tp_emul_walk(const fa_tdt_window_config *cfg, int32_t recording, int64_t total, int64_t speech_end, const int64_t *starts, int64_t listed, fa_tdt_window *out,
                     int64_t capacity) {
    tp::Geometry g{};
    if (tp::derive(*cfg, &g).status != FA_SUCCESS) return -1;
    if (total == 0) return 0;
    if (listed != tp::listed_starts(g, total)) return -2;
    const int64_t last_listed = starts[listed - 1] >> 1;
    for (int64_t i0 = 0;; i0 += tp::kWave) {
        tp::Turn turns[tp::kWave];
        int first = tp::kWave;
        for (int lane = 0; lane < tp::kWave; ++lane) {
            const int64_t i = i0 + lane;
            const int64_t start = i < listed ? starts[i] >> 1 : last_listed + (i - (listed - 1)) * g.stride;
            turns[lane] = tp::turn(g, recording, total, speech_end, start, i < listed && (starts[i] & 1), i);
            if (turns[lane].ends && first == tp::kWave) first = lane;
        }
        for (int lane = 0; lane < tp::kWave && lane <= first; ++lane)
            if (turns[lane].record && i0 + lane < capacity) out[i0 + lane] = turns[lane].w;
        if (first < tp::kWave) return i0 + first + (turns[first].record ? 1 : 0);
    }
}

}  // extern "C"
