// sortformer_launch.h — what the offline Sortformer's host code (sortformer_host.hip: window geometry, the window plan, the enumeration of
// the bijections, the host twin of the alignment, the C ABI) and its kernel translation unit (sortformer.hip) share: the limits, the
// operands of the two kernel families and one launcher per family.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"

namespace fa {
namespace sortformer {

constexpr int kMaxSpeakers = 4;     // stitching: S! bijections, 24 for 4 (the reference fixes 4)
constexpr int kMaxPerms = 24;
constexpr int kPackTile = 64;       // pack_transpose: frames x mels of one workgroup
constexpr int kMergeItems = 256;    // stitch_merge: (global frame, column) items of one workgroup

struct Perms { uint8_t p[kMaxPerms][kMaxSpeakers]; int32_t n; };

struct PackArgs {
    const float *mel;
    const fa_sortformer_window *win;
    float *out;
    int32_t *mel_length;
    int64_t rec_stride, frame_stride;
    int32_t n_mels, window_mel;
};

struct StitchArgs {
    const float *preds;                 // [W][window][S]
    const fa_sortformer_window *win;    // [W]
    const int64_t *range;               // [B + 1] windows of each recording
    const int64_t *gofs;                // [B + 1] first global frame of each recording
    float *corr;                        // [W][S][S]: rows in the PREVIOUS window's own columns
    int32_t *ov;                        // [W] overlap frames compared
    float *global;                      // [sum totalOut][S]
    int32_t *mapping;                   // [W][S]
    int32_t B, S, window, overlap, hop;
};

// pack_rows (FA_MEL_LAYOUT_MEL_MAJOR: W * n_mels workgroups; 16-byte stores when a.out and the window length allow them) or pack_transpose
// (FA_MEL_LAYOUT_FRAME_MAJOR: kPackTile x kPackTile tiles) on W windows.  Launch errors surface through hipGetLastError().
void launch_pack(hipStream_t stream, const PackArgs &a, int32_t layout, int64_t W);
// The global timeline (items = global frames * S) and the mappings of W windows.  2 * overlap <= window: stitch_corr, stitch_chain and
// stitch_merge; any other geometry: a.global zeroed, then stitch_serial.  Returns the memset's error; the launches' as launch_pack.
hipError_t launch_stitch(hipStream_t stream, const StitchArgs &a, const Perms &perms, int64_t W, int64_t items);

}  // namespace sortformer
}  // namespace fa
