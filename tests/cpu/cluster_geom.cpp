// The host arithmetic of the clustering stage's kernels (fluidaudio_amd/csrc/vbx_geom.h and post_geom.h: what vbx.hip's kernels and
// launchers, vbx_host.hip's shard entries and post_host.hip's constrained assignment decide with) driven over stdin: one command per line.
// Test infrastructure: built by tests/test_cluster_geom.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   slices Tg                      -> "lo hi" of the 64 slices, on one line
//   shard Tg rank world            -> "lo hi"
//   chunk S D world                -> doubles of a rank's records (0: refused)
//   tiled S allowed                -> "0" or "1"
//   dim D                          -> "fits lds_bytes"
//   cen n                          -> "0" or "1" (the tiled centroid kernel)
//   groups K n ids...              -> "n_chunks max_rows side slabs slab_bytes | order... | starts..."
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/post_geom.h"
#include "../../fluidaudio_amd/csrc/vbx_geom.h"

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        int64_t Tg, n;
        int32_t a, b, c;
        if (!strcmp(cmd, "slices")) {
            if (scanf("%" SCNd64, &Tg) != 1) return 2;
            for (int z = 0; z < fa::vbx::kSplit; ++z) {
                const fa::vbx::FrameRange r = fa::vbx::slice_range(Tg, z);
                printf("%" PRId64 " %" PRId64 "%c", r.lo, r.hi, z + 1 < fa::vbx::kSplit ? ' ' : '\n');
            }
        } else if (!strcmp(cmd, "shard")) {
            if (scanf("%" SCNd64 " %d %d", &Tg, &a, &b) != 3) return 2;
            const fa::vbx::FrameRange r = fa::vbx::shard_range(Tg, a, b);
            printf("%" PRId64 " %" PRId64 "\n", r.lo, r.hi);
        } else if (!strcmp(cmd, "chunk")) {
            if (scanf("%d %d %d", &a, &b, &c) != 3) return 2;
            printf("%" PRId64 "\n", fa::vbx::chunk_doubles(a, b, c));
        } else if (!strcmp(cmd, "tiled")) {
            if (scanf("%d %d", &a, &b) != 2) return 2;
            printf("%d\n", fa::vbx::tiled_route(a, b != 0) ? 1 : 0);
        } else if (!strcmp(cmd, "dim")) {
            if (scanf("%d", &a) != 1) return 2;
            printf("%d %zu\n", fa::vbx::dim_fits(a) ? 1 : 0, fa::vbx::estep_lds_bytes(a));
        } else if (!strcmp(cmd, "cen")) {
            if (scanf("%" SCNd64, &n) != 1) return 2;
            printf("%d\n", fa::post::centroids_tiled(n) ? 1 : 0);
        } else if (!strcmp(cmd, "groups")) {
            if (scanf("%d %" SCNd64, &a, &n) != 2 || n < 0) return 2;
            std::vector<int32_t> ids(static_cast<size_t>(n));   // exactly n ids: the sanitizers watch the grouping's reads
            for (int32_t &x : ids) if (scanf("%d", &x) != 1) return 2;
            const fa::post::ChunkGroups g = fa::post::group_by_chunk(ids.data(), n);
            const int side = fa::post::hung_side(g.max_rows, a);
            printf("%d %d %d %d %zu |", g.n_chunks(), g.max_rows, side, fa::post::hung_in_slabs(side) ? 1 : 0, fa::post::hung_slab_bytes(side));
            for (const int32_t x : g.order) printf(" %d", x);
            printf(" |");
            for (const int32_t x : g.starts) printf(" %d", x);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
