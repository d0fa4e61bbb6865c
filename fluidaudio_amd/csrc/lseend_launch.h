// lseend_launch.h — what the host code of the LS-EEND front end (lseend_host.hip: tables, plans, stream state, entries) and its
// kernel unit (lseend.hip) share: the per-item record, the kernels' operands, the LDS carve-up, the launches.  Internal.
#pragma once
#include "fa_common.h"
#include "lseend_core.h"
#include "mel_core.h"   // fft16, cmul and the transpose geometry of the 16-lane frame group

namespace fa {
namespace lseend {

// One item of a call: a whole recording from a fresh state, or one stream's newly pushed audio behind its carried state.  The call's
// sample sequence of the item is: tail_in carried samples | n_new samples at pcm + pcm_off | zeros; frame j covers [j hop, j hop + n_fft).
struct Item {
    const float *tail_src;    // carried audio (nullptr: zeros, the n_fft / 2 seed of a fresh state)
    float *tail_dst;          // the samples behind the last frame, tail_out of them (nullptr: dropped)
    const float *mel_src;     // carried normalised rows [mel_in][n_mels] (nullptr: zeros, the context seed of a fresh state)
    float *mel_dst;           // rows behind the last emitted window, [mel_out][n_mels] (nullptr: dropped)
    const double *sum_src;    // carried per-mel sum (nullptr: 0)
    double *sum_dst;          // (nullptr: dropped)
    int64_t pcm_off;
    int64_t frames0;          // frames before this call: the CMN count
    int64_t windows0, windows1;   // the windows this call emits, as indices of the stream
    int64_t row0;             // first row of the item in the call's raw-row array
    int64_t win0;             // first window of the item in the call's arena
    int64_t out_row0;         // first row of the item in the dense probabilities
    int32_t n_new, tail_in, tail_out, mel_in, frames, tile0, tiles;
};

struct Args {
    const Item *items;
    const int32_t *tile_item;   // [tiles] the item of every tile
    const float *pcm;
    int64_t pcm_total;          // floats behind pcm: 16-byte loads stay inside
    float *rows;                // [total frames][n_mels] un-normalised log10-mel rows: the caller's array or the workspace
    double *tile_sums;          // [tiles][n_mels]
    double *tile_prefix;        // [tiles][n_mels] exclusive, the carried sum included
    float *windows;             // [total windows][mel_frames][n_mels]
    float *masks;               // [total windows][chunk]
    int32_t *warmups;           // [total windows]
    int64_t *out_rows;          // [total windows] first row of the window's kept rows in the dense probabilities
    const float *windowz;       // 256: the periodic Hann of `win` centred in n_fft
    const float2 *tw256;        // 256  exp(-2 pi i k / 256)
    const int32_t *mel_tab;     // 2 n_mels: (first bin | bins << 16, offset of the row's weights)
    const float *mel_w;         // n_weights
    Geometry g;
    int32_t n_items, n_tiles, n_weights, stage_alloc, vec;   // vec: pcm 16-byte aligned
    float log_floor, log10_scale;
};

struct GatherArgs {
    const float *probs;         // [windows][chunk][row_stride >= speakers], window_stride floats apart
    const int32_t *warmups;
    const int64_t *out_rows;
    float *out;                 // dense [rows][speakers]
    int64_t window_stride, row_stride;
    int64_t out_capacity;       // rows behind `out`
    int32_t windows, chunk, speakers;
};

// floats of dynamic LDS of the mel-tile kernel: staged samples | 16 transpose regions | the tile's rows | filterbank rows | weights
inline size_t lds_bytes(const Args &a) {
    return sizeof(float) * (static_cast<size_t>(a.stage_alloc) + kGroups * fa::melcore::kRegionFloats + static_cast<size_t>(kTileFrames) * a.g.n_mels +
                            2 * static_cast<size_t>(a.g.n_mels) + static_cast<size_t>(a.n_weights));
}

// lseend.hip; errors surface through hipGetLastError().  run(): the three launches of a call, whatever the batch.
void run(const Args &a, hipStream_t stream);
void gather(const GatherArgs &a, hipStream_t stream);

}  // namespace lseend
}  // namespace fa
