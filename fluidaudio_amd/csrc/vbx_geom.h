// vbx_geom.h — the index arithmetic of the VBx refinement in plain C++, for host and device: the kernels (vbx.hip), the host code
// (vbx_host.hip: set-up, the shard entries of the C ABI) and tests/cpu/cluster_geom.cpp — which walks it under the sanitizers without
// a GPU — all take it from here.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FA_VBX_HD __host__ __device__ inline
#else
#define FA_VBX_HD inline
#endif

namespace fa {
namespace vbx {

constexpr int kSplit = 64;          // fixed split of the frame axis: one record per slice, summed in slice order
constexpr int kTiledMinS = 48;      // speakers from which the two contractions run as tiled products
constexpr int kEstepWaves = 4;      // frames (one per wavefront) of an E-step workgroup: that many rho rows in LDS
constexpr size_t kEstepLdsLimit = 64 * 1024;

struct FrameRange { int64_t lo, hi; };   // [lo, hi); empty when lo == hi

// the frames of slice z (0 .. kSplit - 1) of a problem of Tg frames: ceil(Tg / kSplit) frames each, the last ones short or empty
FA_VBX_HD FrameRange slice_range(const int64_t Tg, const int z) {
    const int64_t per = (Tg + kSplit - 1) / kSplit;
    const int64_t lo = z * per, hi = lo + per;
    return {lo < Tg ? lo : Tg, hi < Tg ? hi : Tg};
}

// world sizes that divide the slices; a rank's slices are zn = kSplit / world consecutive ones from rank * zn on
FA_VBX_HD bool shard_ok(const int32_t rank, const int32_t world) { return world > 0 && kSplit % world == 0 && rank >= 0 && rank < world; }

// the frames a rank holds = the union of its slices; (0, 0) for an empty problem or a (rank, world) that shard_ok refuses
FA_VBX_HD FrameRange shard_range(const int64_t Tg, const int32_t rank, const int32_t world) {
    if (Tg <= 0 || !shard_ok(rank, world)) return {0, 0};
    const int zn = kSplit / world;
    return {slice_range(Tg, rank * zn).lo, slice_range(Tg, (rank + 1) * zn - 1).hi};
}

// doubles of one slice record: [S][D + 1] (column D carries sum_t gamma), then the slice's sum of the per-frame log-likelihoods
FA_VBX_HD int64_t record_stride(const int32_t S, const int32_t D) { return static_cast<int64_t>(S) * (D + 1) + 1; }

// doubles a rank contributes to the all-gather of an iteration; 0 for arguments the shard entries refuse
FA_VBX_HD int64_t chunk_doubles(const int32_t S, const int32_t D, const int32_t world) {
    if (S < 1 || D < 1 || world < 1 || kSplit % world != 0) return 0;
    return (kSplit / world) * record_stride(S, D);
}

// the tiled products serve many speakers, unless the switch (FA_VBX_NO_TILED, read once per refinement) turns them off
FA_VBX_HD bool tiled_route(const int32_t S, const bool tiled_allowed) { return S >= kTiledMinS && tiled_allowed; }

// LDS of an E-step workgroup, and the feature dimensions it can hold
FA_VBX_HD size_t estep_lds_bytes(const int32_t D) { return sizeof(double) * kEstepWaves * static_cast<size_t>(D); }
FA_VBX_HD bool dim_fits(const int32_t D) { return estep_lds_bytes(D) <= kEstepLdsLimit; }

}  // namespace vbx
}  // namespace fa
