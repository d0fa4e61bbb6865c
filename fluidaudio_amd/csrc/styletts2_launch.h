// styletts2_launch.h — what the host code of the StyleTTS2 session (styletts2_host.hip: tables, plan, session, entries) and its kernel
// unit (styletts2.hip) share: the per-item records, the kernels' operands, the launch geometry.  Internal.
#pragma once
#include "fa_common.h"
#include "mel_core.h"   // fft16, cmul
#include "styletts2_core.h"

namespace fa {
namespace styletts2 {

// ---- the reference mel: a workgroup of kMelThreads = 4 wavefronts owns kTileFrames consecutive frames of one item (a mel row leaves the
// tile as kTileFrames floats = 64 bytes); a wavefront takes a frame per pass, 16 complex points per lane
constexpr int kMelThreads = 256;
constexpr int kMelWaves = kMelThreads / 64;
constexpr int kTileFrames = 16;
constexpr int kTileStride = kTileFrames + 1;           // floats per mel row of the output tile in LDS: odd, a frame's 80 stores spread over the banks
constexpr int kRowStride = 68;                         // complex elements per k1 row of the transpose buffer: 64 + 4, as luxtts.hip
constexpr int kRegionFloats = 2 * 16 * kRowStride;     // a wavefront's region: the transpose buffer, then Z (quarters 16 complex apart), then the power bins

// ---- the element-wise kernels
constexpr int kThreads = 256;
constexpr int kAlignFrames = 64;                       // frames of an alignment tile
constexpr int kAlignChannels = 64;                     // channels of an alignment tile
constexpr int kAlignStride = kAlignChannels + 4;       // floats per token row of the tile of d in LDS: 16-byte rows, a column's reads 4 banks apart

using Item = fa_styletts2_item_plan;
using Slabs = fa_styletts2_slabs;

struct MelArgs {
    const Item *items;
    const int64_t *offsets;    // [B] first sample of the item in pcm (device copy)
    const float *pcm;
    float *mel;                // [B][n_mels][stride]
    const float *window;       // win
    const float2 *tw2048;      // 2049: exp(-2 pi i k / 2048); the 1024-point twiddles are the even entries
    const int32_t *mel_tab;    // 2 n_mels: (first bin | bins << 16, offset of the row's weights)
    const float *mel_w;
    int32_t n_mels, hop, win, lead, stride, vec;   // lead = (n_fft - win) / 2; vec: pcm 16-byte aligned
    float log_eps, log_mean, log_std;
};

struct InputArgs {
    const Item *items;
    const int32_t *token_ids;  // ragged, item b at token_offsets[b]
    const int64_t *token_offsets;
    const uint64_t *seeds;
    Slabs s;
    int32_t batch, token_stride, aux_steps;
};

struct BlendArgs {
    const float *s_pred, *ref_s;   // [B][>= 256]
    const float *alphas, *betas;   // [B] device copies
    int64_t s_pred_stride, ref_s_stride;
    Slabs s;
};

struct DurationArgs {
    const Item *items;
    const float *logits;
    int64_t item_stride, token_stride, channel_stride;
    Slabs s;
    int32_t channels, token_stride_out, max_frames;
};

struct AlignArgs {
    const Item *items;
    const float *d, *t_en;     // [B][n][d_row_stride >= d_channels], [B][asr_channels][t_row_stride >= n]
    int64_t d_row_stride, d_item_stride, t_row_stride, t_item_stride;
    float *en, *asr;           // [B][d_channels][frame_stride], [B][asr_channels][frame_stride]
    Slabs s;
    int32_t d_channels, asr_channels, d_slabs, frame_stride, token_stride, shift, vec_d, vec_out;
};

struct FinishArgs {
    const float *audio;        // [B][row_stride]
    const int64_t *ranges;     // [B + 1] device copy of the output offsets
    float *out;
    int64_t row_stride;
    int32_t vec;
};

inline size_t mel_lds_bytes(const MelArgs &a) {
    return sizeof(float) * (static_cast<size_t>((kTileFrames - 1) * a.hop + a.win) + kMelWaves * kRegionFloats + 2 * static_cast<size_t>(a.n_mels) + static_cast<size_t>(a.n_mels) * kTileStride);
}

// styletts2.hip; errors surface through hipGetLastError()
void run_reference_mel(const MelArgs &a, int batch, hipStream_t stream);
void run_inputs(const InputArgs &a, hipStream_t stream);
void run_blend(const BlendArgs &a, int batch, hipStream_t stream);
void run_durations(const DurationArgs &a, int batch, hipStream_t stream);
void run_align(const AlignArgs &a, int batch, hipStream_t stream);
void run_finish(const FinishArgs &a, int batch, int64_t longest, hipStream_t stream);

}  // namespace styletts2
}  // namespace fa
