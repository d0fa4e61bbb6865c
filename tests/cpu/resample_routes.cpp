// The route of a fa_resample_poly_dev call (fluidaudio_amd/csrc/resample_route.h: pick_route, the plain C++ part of resample_host.hip) driven over
// stdin, one call per line, on synthetic plan facts.  Test infrastructure: built by tests/test_resample_routes.py with g++ and the address /
// undefined-behaviour sanitizers, no GPU.
//   route up down n_taps pre_remove decim_tiles decim_regs interp has_rows tile_rows m_begin k_begin groups ppg sld smax share lds_bytes
//         simple no_decim no_decim_tiles no_rows x_addr y_addr frames n_out
//       -> "kind lo hi split count" (kind: 0 DECIM, 1 INTERP, 2 ROWS, 3 LDS, 4 SIMPLE)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../fluidaudio_amd/csrc/resample_route.h"

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (strcmp(cmd, "route")) return 2;
        fa::resample::PlanFacts P;
        fa::PolyRowsGeom &G = P.rows_geom;
        int decim_tiles, decim_regs, interp, has_rows, simple, no_decim, no_decim_tiles, no_rows;
        uint64_t lds_bytes, x_addr, y_addr;
        int64_t frames, n_out;
        if (scanf("%d %d %" SCNd64 " %" SCNd64 " %d %d %d %d %d", &P.up, &P.down, &P.n_taps, &P.pre_remove, &decim_tiles, &decim_regs, &interp, &has_rows, &P.tile_rows) != 9) return 2;
        if (scanf("%" SCNd64 " %" SCNd64 " %d %d %d %d %d %" SCNu64, &G.m_begin, &G.k_begin, &G.groups, &G.ppg, &G.sld, &G.smax, &G.share, &lds_bytes) != 8) return 2;
        if (scanf("%d %d %d %d %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64, &simple, &no_decim, &no_decim_tiles, &no_rows, &x_addr, &y_addr, &frames, &n_out) != 8) return 2;
        P.decim_tiles = decim_tiles != 0; P.decim_regs = decim_regs != 0; P.interp = interp != 0; P.has_rows = has_rows != 0;
        P.lds_bytes = static_cast<size_t>(lds_bytes);
        G.up = P.up; G.down = P.down;
        const fa::resample::Switches sw = {simple != 0, no_decim != 0, no_decim_tiles != 0, no_rows != 0};
        const fa::resample::Route r = fa::resample::pick_route(P, sw, static_cast<uintptr_t>(x_addr), static_cast<uintptr_t>(y_addr), frames, n_out);
        printf("%d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", static_cast<int>(r.kind), r.lo, r.hi, r.split, r.count);
    }
    return 0;
}
