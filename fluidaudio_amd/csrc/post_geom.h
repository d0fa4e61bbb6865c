// post_geom.h — the host arithmetic of the centroid / assignment kernels (post.hip) in plain C++: the rows of a recording grouped by
// segmentation chunk, the scratch a Hungarian problem beyond the LDS arrays needs, and the two routes (LDS or slab; the tiled centroid
// kernel).  post_host.hip, post.hip and tests/cpu/cluster_geom.cpp — which walks it under the sanitizers without a GPU — take it from here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define FA_POST_HD __host__ __device__ inline
#else
#define FA_POST_HD inline
#endif

namespace fa {
namespace post {

constexpr int kHungMaxN = 256;   // rows of a chunk / clusters whose potentials, matching and slack arrays fit a wavefront's LDS slice
constexpr int kCenTile = 128;    // rows of one LDS tile of the tiled centroid kernel

// rows grouped by chunk, ascending row order inside a chunk (rowsByChunk[chunk].append(row), ConstrainedClusterAssignment.swift:27-30);
// chunks in ascending id order.  starts: n_chunks + 1 offsets into order.
struct ChunkGroups {
    std::vector<int32_t> order, starts;
    int max_rows = 0;            // rows of the largest chunk
    int n_chunks() const { return static_cast<int>(starts.size()) - 1; }
};
inline ChunkGroups group_by_chunk(const int32_t *chunk_indices, const int64_t n) {
    ChunkGroups g;
    g.order.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) g.order[i] = static_cast<int32_t>(i);
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t a, int32_t b) { return chunk_indices[a] < chunk_indices[b]; });
    for (int64_t i = 0; i < n; ++i)
        if (i == 0 || chunk_indices[g.order[i]] != chunk_indices[g.order[i - 1]]) g.starts.push_back(static_cast<int32_t>(i));
    g.starts.push_back(static_cast<int32_t>(n));
    for (int c = 0; c < g.n_chunks(); ++c) g.max_rows = std::max(g.max_rows, g.starts[c + 1] - g.starts[c]);
    return g;
}

// the side of the largest (square, padded) assignment problem, and whether its arrays leave LDS for per-wavefront slabs of HBM scratch
// (rare: more than 256 clusters survive VBx, or a chunk holds more than 256 rows — the reference solves any size, HungarianAssignment.swift:8-62)
FA_POST_HD int hung_side(const int max_rows, const int K) { return max_rows > K ? max_rows : K; }
FA_POST_HD bool hung_in_slabs(const int side) { return side > kHungMaxN; }

// bytes of one wavefront's slab for problems of side n: u, v, minv (long long), p, way (int), used (a byte), n + 1 entries each; 16-byte aligned
FA_POST_HD size_t hung_slab_bytes(const int n) {
    const size_t e = static_cast<size_t>(n) + 1;
    return (e * (3 * sizeof(long long) + 2 * sizeof(int) + 1) + 15) & ~static_cast<size_t>(15);
}

// long recordings take the tiled centroid kernel: at least four tiles of rows
FA_POST_HD bool centroids_tiled(const int64_t n) { return n >= 4 * kCenTile; }

}  // namespace post
}  // namespace fa
