// The argument pass and the plan of the timeline (fluidaudio_amd/csrc/timeline_launch.h: what timeline_host.hip sizes every buffer and
// every grid of a call with) driven over stdin: one call per line.
// Test infrastructure: built by tests/test_timeline_plan.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   call S activity pad_on pad_off min_on min_off capacity have_fin have_tent B fin_frames[B] tent_frames[B] ('-' in place of tent_frames: none)
// -> "status | text" for a refusal, else "0 | fsum tsum Q max_tiles blocks | B x (fin_off tent_off nf nt)"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/timeline_launch.h"

namespace tl = fa::timeline;

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (strcmp(cmd, "call")) return 2;
        fa_timeline_config cfg;
        memset(&cfg, 0, sizeof(cfg));
        int64_t capacity;
        int32_t have_fin, have_tent, B;
        if (scanf("%d %d %d %d %d %d %" SCNd64 " %d %d %d", &cfg.speakers, &cfg.activity_type, &cfg.onset_pad_frames, &cfg.offset_pad_frames, &cfg.min_frames_on,
                  &cfg.min_frames_off, &capacity, &have_fin, &have_tent, &B) != 10)
            return 2;
        // exactly B counts a side: the sanitizers watch the plan's reads
        std::vector<int64_t> fin(static_cast<size_t>(B > 0 ? B : 0)), tent(fin.size());
        bool tent_given = true;
        for (size_t side = 0; side < 2; ++side)
            for (size_t b = 0; b < fin.size() && tent_given; ++b) {
                char w[32];
                if (scanf("%31s", w) != 1) return 2;
                if (side == 1 && b == 0 && !strcmp(w, "-")) { tent_given = false; break; }
                (side ? tent : fin)[b] = strtoll(w, nullptr, 10);
            }
        int dummy = 0;
        fa::Verdict v = tl::check_config(cfg, B, capacity, B > 0 ? fin.data() : nullptr);
        tl::Plan plan;
        if (v.status == FA_SUCCESS && B > 0)
            v = tl::make_plan(cfg.speakers, fin.data(), tent_given ? tent.data() : nullptr, B, have_fin ? &dummy : nullptr, have_tent ? &dummy : nullptr, plan);
        if (v.status != FA_SUCCESS) {
            printf("%d | %s\n", static_cast<int>(v.status), v.text);
            continue;
        }
        printf("0 | %" PRId64 " %" PRId64 " %" PRId64 " %d %" PRId64 " |", plan.fsum, plan.tsum, plan.Q, plan.max_tiles, plan.blocks);
        for (const tl::TlRec &r : plan.rec) printf(" %" PRId64 " %" PRId64 " %d %d", r.fin_off, r.tent_off, r.nf, r.nt);
        printf("\n");
    }
    return 0;
}
