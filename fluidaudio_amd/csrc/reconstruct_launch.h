// reconstruct_launch.h — what the reconstruction's host code (reconstruct_host.hip: the frame plan's staging, the segment passes, the
// C ABI) and its kernel translation unit (reconstruct.hip) share: the limits, the operands of the frame kernel, the raw run record and one
// launcher per stage, each of which owns its route choice.  The host arithmetic is reconstruct_geom.h.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"
#include "reconstruct_geom.h"

namespace fa {
namespace reconstruct {

constexpr int kTileG = 64;        // global frames per workgroup of the frame kernel (16 per wavefront)
constexpr int kListCap = 1024;    // chunks of a tile listed in LDS (irregular offsets); more: every wavefront scans all chunks
constexpr int kSelBits = 15;      // per-frame word: [0, 15) clusters active, [15, 30) speakerCountPerFrame, bit 30 zero-vote
constexpr int kSelMask = (1 << kSelBits) - 1;
constexpr int kZeroVote = 1 << 30;

struct FrameArgs {
    const float *w;          // [C][F][S] speaker weights
    const double *start;     // [C] chunk start times
    const int32_t *first_g;  // [C] global frame of chunk frame 0 / F-1
    const int32_t *last_g;
    const int32_t *hard;     // [C][S] cluster of each local speaker, -1 = none (host-mapped from anything outside [0, K))
    const int32_t *ovr;      // [T] zero-vote override cluster or -1; nullptr: none
    int32_t *word;           // [T] kSelBits fields (see above)
    int32_t *sel;            // [T][smax] active clusters, by rank
    double *avg;             // [T][smax] their activation averages
    int32_t *bad;            // set when a weight is not finite
    double *esum_out;        // [T] the fp64 expected-count sum of each frame, or nullptr (fa_reconstruct_info.expected_count_sums)
    int64_t C;
    int32_t F, S, K, T, smax, maxc, sorted;
    double fd;
};

struct RawRun {
    int32_t g0, g1, k, frames;   // frames [g0, g1) of cluster k
    double score;                // sequential fp64 sum of the per-frame averages (:207-213)
};

// Launch errors surface through hipGetLastError().
// 7 classes and 16-byte-aligned x, w and lp: powerset_decode7 on the rows / 4 groups of four rows, powerset_decode_rows on the tail; anything
// else: powerset_decode_rows on every row.  lp may be nullptr.
void launch_powerset(hipStream_t stream, const float *x, int64_t rows, int32_t classes, float *w, float *lp);
// workgroups of the run-start compaction over T * smax items: the length of `bsum`
int64_t run_blocks(int64_t items);
// recon_frames (<1> for K <= 64 clusters, else <4>) on tiles of kTileG global frames, then the compaction of the run starts: starts[0, *total)
// holds the items g * smax + j that start a run
void launch_frames(hipStream_t stream, const FrameArgs &a, int32_t *bsum, int32_t *total, int64_t *starts);
// run_walk over the n_raw runs that start at `starts` (at most 4096 workgroups), one RawRun each
void launch_walk(hipStream_t stream, const FrameArgs &a, const int64_t *starts, const int32_t *total, int64_t n_raw, RawRun *out);

}  // namespace reconstruct
}  // namespace fa
