// luxtts_launch.h — what the host code of the LuxTTS session (luxtts_host.hip: tables, plan, session, entries) and its kernel unit
// (luxtts.hip) share: the per-item records, the kernels' operands, the launch geometry.  Internal.
#pragma once
#include "fa_common.h"
#include "luxtts_core.h"
#include "mel_core.h"   // fft16, cmul

namespace fa {
namespace luxtts {

// ---- the fused prompt mel: a workgroup of kMelThreads = 4 wavefronts owns kTileFrames consecutive frames of one item; a wavefront takes
// a frame per pass, 16 points per lane
constexpr int kMelThreads = 256;
constexpr int kMelWaves = kMelThreads / 64;
constexpr int kTileFrames = 2 * kMelWaves;
constexpr int kRowStride = 68;                         // complex elements per k1 row of the transpose buffer: 64 + 4, see luxtts.hip
constexpr int kTransposeFloats = 2 * 16 * kRowStride;
constexpr int kRegionFloats = kTransposeFloats + 520;   // floats of a wavefront's region: the transpose buffer, then the kBins magnitudes
constexpr int kSplit = 256;                             // bins below come from the frame's transform, the others from its first difference's

// ---- the element-wise kernels: 256 threads, four floats of a row each
constexpr int kThreads = 256;
constexpr int kVocTile = 64;                           // frames of a vocoder-input tile
constexpr int kVocStride = kVocTile + 1;               // floats per mel row of the tile in LDS: odd, so a column's stores spread over the banks

using Item = fa_luxtts_item_plan;     // the plan of one item, uploaded by fa_luxtts_session_begin
using Record = fa_luxtts_record;      // what fa_luxtts_prompt_dev leaves per item: 0, kSilentPrompt, or the plan's status of a refused item
using Slabs = fa_luxtts_slabs;

struct MelArgs {
    const Item *items;
    const int64_t *offsets;    // [B] first sample of the item in pcm (device copy)
    const float *pcm;
    Slabs s;
    const float *window;       // 1024
    const float2 *tw1024;      // 1024 exp(-2 pi i k / 1024)
    const float *undo;         // 513: 1 / (2 sin(pi k / 1024)), what the first difference did to bin k (read from kSplit on)
    const int32_t *mel_tab;    // 2 n_mels: (first bin | bins << 16, offset of the row's weights)
    const float *mel_w;
    int32_t n_weights, n_mels, hop, max_frames, vec;   // vec: pcm 16-byte aligned
    float log_floor, feat_scale, target_rms;
};

struct InputArgs {
    const Item *items;
    const int32_t *token_ids;  // ragged, item b at token_offsets[b]
    const int64_t *token_offsets;
    const uint64_t *seeds;
    Slabs s;
    int32_t n_mels, max_tokens, max_frames;
};

struct RowArgs {               // text condition and solver step: a strided [B][rows][row_stride] operand beside a slab
    const Item *items;
    const float *src;
    int64_t row_stride, item_stride;
    Slabs s;
    StepTimes times;
    int32_t n_mels, max_frames, vec;   // vec: src rows 16-byte aligned
};

struct VocoderArgs {
    const Item *items;
    const int32_t *list;       // [n] the items of this bucket
    Slabs s;
    float *mel;                // [n][n_mels][bucket]
    int32_t bucket, n_mels, max_frames, vec;
    float floor_value, inv_scale;
};

struct FinishArgs {
    const Item *items;
    const float *audio;        // [B][row_stride]
    const int64_t *sample_offsets;
    float *out;
    Slabs s;
    int64_t row_stride;
    int32_t vec;               // audio and out 16-byte aligned
    float target_rms;
};

inline size_t mel_lds_bytes(const MelArgs &a) {
    return sizeof(float) * (static_cast<size_t>((kTileFrames - 1) * a.hop + kNfft) + kMelWaves * kRegionFloats + 2 * static_cast<size_t>(a.n_mels) + static_cast<size_t>(a.n_weights));
}

// luxtts.hip; errors surface through hipGetLastError()
void run_prompt(const MelArgs &a, int batch, hipStream_t stream);            // two launches: loudness, mel
void run_inputs(const InputArgs &a, int batch, hipStream_t stream);
void run_text_condition(const RowArgs &a, int batch, hipStream_t stream);
void run_step(const RowArgs &a, int batch, hipStream_t stream);
void run_vocoder_input(const VocoderArgs &a, int n, hipStream_t stream);
void run_finish(const FinishArgs &a, int batch, int64_t max_samples, hipStream_t stream);

}  // namespace luxtts
}  // namespace fa
