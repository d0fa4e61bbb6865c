// pockettts_launch.h — what the host code of the PocketTTS session (pockettts_host.hip: tables, plans, session, entries) and its kernel
// unit (pockettts.hip) share: the kernels' operands and the launch geometry.  Internal.
#pragma once
#include "fa_common.h"
#include "pockettts_core.h"
#include "row_pack_launch.h"

namespace fa {
namespace pockettts {

// ---- the re-projection: a workgroup of kCloneThreads = 4 wavefronts owns kTileFrames frames of one clone.  The 1024 dims pass through
// LDS in kSteps slices of kSliceDims; of a slice a wavefront multiplies its own kSliceDims / 4 dims (32x32x2 fp32 matrix instruction, 2
// dims an issue), so the K axis of stage one is split four ways and every wavefront keeps one 32 x 32 partial in registers over all
// slices.  The partials meet in LDS, wavefront 0 first; stage two reads the latents from there and a wavefront makes kDim / 4 columns.
constexpr int kCloneThreads = 256;
constexpr int kTileFrames = 32;
constexpr int kSliceDims = 256;
constexpr int kSteps = kDim / kSliceDims;
constexpr int kSliceStride = kSliceDims + 4;        // floats per frame row of the slice in LDS: 16-byte rows, a column's reads 4 banks apart
constexpr int kLatStride = kLatent + 1;             // floats per frame row of the latents in LDS
constexpr int kThreads = 256;
constexpr int kKvUnits = 8;                         // 16-byte stores a thread of the reset makes

struct CloneItem {
    int32_t voice, projection, usable, pad;
};

struct CloneArgs {
    const CloneItem *items;
    const void *cond;          // element (b, f, d) at b item_stride + f frame_stride + d dim_stride
    int64_t item_stride, frame_stride, dim_stride;
    const float *projections;  // per slot: Pinv [1024][32], then W [1024][32]
    float *voice_rows;         // [voices][125][1024]
    int32_t vec;               // dim_stride 1 and every row 16-byte aligned
};

struct KvItem {
    int32_t stream, voice, src_seq, pad;   // voice -1: zeros, position 0
};

struct KvArgs {
    const KvItem *items;
    void *kv;
    float *positions;
    float *voice_kv;           // [voices][layers][2][voice_plane]
    float *voice_offsets;      // [voices][kMaxLayers]
    int64_t voice_plane;       // voice_seq * 1024
    int32_t format, streams, layers, n_positions;
};

struct PrefillArgs {
    const Window *windows;
    const int32_t *ids;
    const float *table, *bos_before_voice, *voice_rows, *positions;
    float *arena, *valid_len, *window_position;
    int32_t vocab, n_positions;
};

struct AdvanceItem {
    int32_t stream, rows;
};

struct StepArgs {
    StreamState *state;
    const float *eos_logit, *latent;
    float *sequence, *positions;
    int32_t *running, *n_running;
    int32_t streams, n_positions;
};

struct BeginItem {
    int32_t stream, max_gen, after, pad;
};

// pockettts.hip; errors surface through hipGetLastError()
void run_encoder_rows(const float *pcm, const rows::Group &g, float *rows, bool wide, hipStream_t stream);
void run_clone(const CloneArgs &a, int32_t dtype, int n, hipStream_t stream);
void run_kv_reset(const KvArgs &a, int n, hipStream_t stream);
void run_kv_capture(const KvArgs &a, hipStream_t stream);                 // items[0]: the stream, the voice and the rows to keep
void run_prefill(const PrefillArgs &a, int n_windows, const AdvanceItem *advance, float *positions, int n_streams, hipStream_t stream);
void run_position_set(float *positions, int n_positions, float value, hipStream_t stream);
void run_step_begin(const BeginItem *items, int n, StreamState *state, float *sequence, const float *bos_embedding, int use_bos, hipStream_t stream);
void run_step(const StepArgs &a, hipStream_t stream);
void run_append_audio(const StreamState *state, const float *samples, float *audio, int streams, int max_frames, hipStream_t stream);

}  // namespace pockettts
}  // namespace fa
