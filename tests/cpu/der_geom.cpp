// The argument pass and the plan of the DER scorer (fluidaudio_amd/csrc/der_geom.h: what der_host.hip sizes every buffer and every grid
// of a call with) driven over stdin: one call per `call` block.
// Test infrastructure: built by tests/test_der_geom.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   call frame_step collar B n_ref n_hyp have_mapping have_overlap overlap_capacity
//   ref_range[B + 1]  hyp_range[B + 1]  mapping_range[B + 1]
//   n_ref x (label start end)   n_hyp x (label start end)         times as C hexadecimal or decimal floats, inf and nan admitted
// -> "status | text" for a refusal, else
//    "0 | plane_words ov_entries max_words items raster_blocks raster_status | B x (num_frames R H words plane_off ov_off ref_begin ref_end hyp_begin hyp_end)"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/der_geom.h"

static bool read_segments(std::vector<fa_der_segment> &v) {
    for (fa_der_segment &s : v) {
        char a[64], b[64];
        if (scanf("%d %63s %63s", &s.label, a, b) != 3) return false;
        s.start = strtod(a, nullptr);
        s.end = strtod(b, nullptr);
    }
    return true;
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (strcmp(cmd, "call")) return 2;
        char fs[64], fc[64];
        int32_t B, have_mapping, have_overlap;
        int64_t n_ref, n_hyp, capacity;
        if (scanf("%63s %63s %d %" SCNd64 " %" SCNd64 " %d %d %" SCNd64, fs, fc, &B, &n_ref, &n_hyp, &have_mapping, &have_overlap, &capacity) != 8) return 2;
        if (n_ref < 0 || n_hyp < 0) return 2;
        const fa_der_config cfg{strtod(fs, nullptr), strtod(fc, nullptr)};
        std::vector<int64_t> range[3];
        for (auto &r : range) {
            r.resize(static_cast<size_t>(B > 0 ? B : 0) + 1);   // a negative B is a case too
            for (int64_t &x : r) if (scanf("%" SCNd64, &x) != 1) return 2;
        }
        // exactly as many segments as the caller says: the sanitizers watch the pass's reads
        std::vector<fa_der_segment> ref(static_cast<size_t>(n_ref)), hyp(static_cast<size_t>(n_hyp));
        if (!read_segments(ref) || !read_segments(hyp)) return 2;
        int dummy = 0;
        fa::der::Plan plan;
        const fa::Verdict v = fa::der::make_plan(cfg, n_ref ? ref.data() : nullptr, range[0].data(), n_hyp ? hyp.data() : nullptr, range[1].data(), B, &dummy,
                                                 have_mapping ? &dummy : nullptr, range[2].data(), have_overlap ? &dummy : nullptr, capacity, plan);
        if (v.status != FA_SUCCESS) {
            printf("%d | %s\n", static_cast<int>(v.status), v.text);
            continue;
        }
        printf("0 | %" PRId64 " %" PRId64 " %d %" PRId64 " %" PRId64 " %d |", plan.plane_words, plan.ov_entries, plan.max_words, plan.items, plan.raster_blocks,
               static_cast<int>(fa::der::check_raster(plan).status));
        for (const fa::der::DerRec &r : plan.rec)
            printf(" %d %d %d %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64, r.num_frames, r.R, r.H, r.words, r.plane_off, r.ov_off, r.ref_begin,
                   r.ref_end, r.hyp_begin, r.hyp_end);
        printf("\n");
    }
    return 0;
}
