// kmeans_draws.h — everything of the k-means fallback that is decided on the host without the data's values (kernels: kmeans.hip,
// entries: kmeans_host.hip): the reference's LCG (SeededRNG, KMeansClustering.swift:212-223) pushed through the Swift standard
// library's `next(upperBound:)` (Lemire's method), `shuffle(using:)` and `randomElement(using:)` — restated because that library is the
// only specification of the draw sequence (third-party, unpinned) — the guards of clusterWithCentroids and
// SpeakerCountConstraints.resolve.  Plain C++ without a HIP call, walked on the host by tests/cpu/kmeans_draws.cpp.  Internal; not part
// of the C ABI.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace fa {
namespace kmeans {

constexpr int kPicks = 1024;   // re-seeding draws a run has before km_step_end raises status[1]

struct Rng {   // SeededRNG (:212-223) + Swift stdlib draws
    uint64_t s;
    uint64_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s; }
    uint64_t below(uint64_t bound) {
        uint64_t r = next();
        unsigned __int128 m = static_cast<unsigned __int128>(r) * bound;
        if (static_cast<uint64_t>(m) < bound) {
            const uint64_t t = (0 - bound) % bound;
            while (static_cast<uint64_t>(m) < t) { r = next(); m = static_cast<unsigned __int128>(r) * bound; }
        }
        return static_cast<uint64_t>(m >> 64);
    }
};

// initializeCentroids (:144-152): indices.shuffled(using:) over 0 ... n - 1, idx.size() = n; the first k entries seed the run.  The
// whole walk is made whatever k is: the run's later draws continue the same stream.
inline void shuffled_indices(Rng &rng, std::vector<int64_t> &idx) {
    const int64_t n = static_cast<int64_t>(idx.size());
    for (int64_t i = 0; i < n; ++i) idx[i] = i;
    int64_t amount = n, cur = 0;
    while (amount > 1) {
        const int64_t j = static_cast<int64_t>(rng.below(static_cast<uint64_t>(amount)));
        amount -= 1;
        std::swap(idx[cur], idx[cur + j]);
        cur += 1;
    }
}

// The re-seeding of empty clusters (randomElement, :196-199) draws below(n) on the run's generator whatever the data is, so the
// sequence is drawn ahead: picks[0 .. kPicks), behind the shuffle.
inline void draw_picks(Rng &rng, const int64_t n, int32_t *picks) {
    for (int j = 0; j < kPicks; ++j) picks[j] = static_cast<int32_t>(rng.below(static_cast<uint64_t>(n)));
}

// the guards of clusterWithCentroids (:46-59); returns true when the call is finished without device work
inline bool degenerate(const double *emb, int64_t n, int32_t d, int32_t num_clusters, int32_t *labels, double *centroids, int32_t *out_k) {
    if (out_k) *out_k = 0;
    if (n <= 0) return true;
    const int64_t k = std::min<int64_t>(num_clusters, n);
    if (d <= 0 || k <= 0) { std::fill(labels, labels + n, 0); return true; }
    if (n <= k) {
        for (int64_t i = 0; i < n; ++i) labels[i] = static_cast<int32_t>(i);
        if (centroids) std::memcpy(centroids, emb, sizeof(double) * n * d);
        if (out_k) *out_k = static_cast<int32_t>(n);
        return true;
    }
    return false;
}

// SpeakerCountConstraints.resolve (SpeakerCountConstraints.swift:25-62): out = { the count when it is decided or -1, min, max }
inline void resolve_constraints(int64_t num_embeddings, const int64_t *num_speakers, const int64_t *min_speakers, const int64_t *max_speakers, int64_t out[3]) {
    int64_t rmin = num_speakers ? *num_speakers : (min_speakers ? *min_speakers : 1);
    rmin = std::max<int64_t>(1, std::min(num_embeddings, rmin));
    int64_t rmax = num_speakers ? *num_speakers : (max_speakers ? *max_speakers : num_embeddings);
    rmax = std::max<int64_t>(1, std::min(num_embeddings, rmax));
    if (rmin > rmax) rmin = rmax;
    out[0] = rmin == rmax ? rmin : (num_speakers ? *num_speakers : -1);
    out[1] = rmin;
    out[2] = rmax;
}

}  // namespace kmeans
}  // namespace fa
