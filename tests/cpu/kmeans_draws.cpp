// The host decisions of the k-means fallback (fluidaudio_amd/csrc/kmeans_draws.h: the seeded generator and the Swift-stdlib draws on
// it, the shuffle that seeds a run, the pre-drawn re-seeding picks, the guards of clusterWithCentroids and SpeakerCountConstraints.resolve)
// driven over stdin: one command per line.
// Test infrastructure: built by tests/test_kmeans_draws.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   next seed count                -> count values of next()
//   below seed bound count         -> count values of below(bound)
//   draws seed n k                 -> "the first k shuffled indices | the kPicks picks", one generator through both as in a run
//   guards n d k                   -> "finished out_k | labels[n] | centroids" on embeddings e[i][j] = 100 i + j, labels preset to -7
//   resolve n ns|- min|- max|-     -> "count min max"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/kmeans_draws.h"

namespace km = fa::kmeans;

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        uint64_t seed, bound;
        int64_t n;
        int32_t count, d, k;
        if (!strcmp(cmd, "next") || !strcmp(cmd, "below")) {
            const bool bounded = cmd[0] == 'b';
            bound = 0;
            if (scanf("%" SCNu64, &seed) != 1 || (bounded && scanf("%" SCNu64, &bound) != 1) || scanf("%d", &count) != 1) return 2;
            km::Rng rng{seed};
            for (int32_t i = 0; i < count; ++i) printf("%" PRIu64 "%c", bounded ? rng.below(bound) : rng.next(), i + 1 < count ? ' ' : '\n');
        } else if (!strcmp(cmd, "draws")) {
            if (scanf("%" SCNu64 " %" SCNd64 " %d", &seed, &n, &k) != 3 || n < 1 || k < 0 || k > n) return 2;
            km::Rng rng{seed};
            std::vector<int64_t> idx(static_cast<size_t>(n));
            km::shuffled_indices(rng, idx);
            std::vector<int32_t> picks(km::kPicks);   // exactly kPicks: the sanitizers watch the writes
            km::draw_picks(rng, n, picks.data());
            for (int32_t c = 0; c < k; ++c) printf("%" PRId64 " ", idx[c]);
            printf("|");
            for (const int32_t p : picks) printf(" %d", p);
            printf("\n");
        } else if (!strcmp(cmd, "guards")) {
            if (scanf("%" SCNd64 " %d %d", &n, &d, &k) != 3 || n < 0) return 2;
            const size_t cells = static_cast<size_t>(n) * static_cast<size_t>(d > 0 ? d : 0);
            std::vector<double> emb(cells), cen(cells, -1.0);
            for (size_t i = 0; i < cells; ++i) emb[i] = 100.0 * static_cast<double>(i / d) + static_cast<double>(i % d);
            std::vector<int32_t> labels(static_cast<size_t>(n), -7);
            int32_t out_k = -7;
            const bool finished = km::degenerate(emb.data(), n, d, k, labels.data(), cen.data(), &out_k);
            printf("%d %d |", finished ? 1 : 0, out_k);
            for (const int32_t l : labels) printf(" %d", l);
            printf(" |");
            for (const double c : cen) printf(" %g", c);
            printf("\n");
        } else if (!strcmp(cmd, "resolve")) {
            char w[3][32];
            if (scanf("%" SCNd64 " %31s %31s %31s", &n, w[0], w[1], w[2]) != 4) return 2;
            int64_t v[3], out[3];
            const int64_t *p[3];
            for (int i = 0; i < 3; ++i) {
                v[i] = strtoll(w[i], nullptr, 10);
                p[i] = strcmp(w[i], "-") ? &v[i] : nullptr;
            }
            km::resolve_constraints(n, p[0], p[1], p[2], out);
            printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", out[0], out[1], out[2]);
        } else {
            return 2;
        }
    }
    return 0;
}
