// fbank_launch.h — what the host code of the Kaldi fbank front end (fbank_host.hip: tables, plan, entries) and its kernel unit
// (fbank.hip) share: the kernel's operands, the LDS carve-up, the launch.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"
#include "fbank_core.h"

namespace fa {
namespace fbank {

using fa::melcore::kRegionFloats;                            // per 16-lane group: transpose buffer, then the 257 power bins, then ...
constexpr int kRegionOut = 288;                              // ... the frame's n_mels log energies at [288, 288 + n_mels)
static_assert(28 + fa::melcore::kBins <= kRegionOut && kRegionOut + kMaxMels <= kRegionFloats, "power bins, then the log energies, inside one region");

struct FbankArgs {
    const float *pcm;          // packed utterances
    const int64_t *offsets;    // B + 1
    float *out;                // [B][row_stride][lfr_m * n_mels]
    int32_t *rows;             // B or nullptr
    const float *shift;        // [lfr_m * n_mels] or nullptr   (AddShift)
    const float *scale;        // [lfr_m * n_mels] or nullptr   (Rescale)
    const float *windowz;      // 512: the window at frame positions [0, win), zeros behind it
    const float2 *tw256;       // 256  exp(-2 pi i k / 256)
    const float2 *tw512;       // 129  exp(-2 pi i k / 512)
    const int32_t *mel_tab;    // 2 n_mels: (first bin | bins << 16, offset of the row's weights)
    const float *mel_w;        // n_weights
    int64_t utt_stride;        // row_stride * row_floats
    int32_t row_stride, row_floats;
    int32_t tiles_per_utt;
    int32_t n_mels, n_weights, win, hop, stage_alloc;
    int32_t lfr_m, lfr_n, tail, remove_dc, vec;   // vec: n_mels % 4 == 0 and `out` 16-byte aligned -> 16-byte stores
    float wave_scale, preemph, log_floor, log_of_floor;   // log_of_floor: log(log_floor) rounded once on the host
};

// floats of dynamic LDS: staged samples | 16 regions | filterbank rows | filterbank weights
inline size_t lds_bytes(const FbankArgs &a) {
    return sizeof(float) * (static_cast<size_t>(a.stage_alloc) + kGroups * kRegionFloats + 2 * static_cast<size_t>(a.n_mels) + static_cast<size_t>(a.n_weights));
}

// fbank.hip; errors surface through hipGetLastError()
void launch(const FbankArgs &a, int64_t grid, hipStream_t stream);

}  // namespace fbank
}  // namespace fa
