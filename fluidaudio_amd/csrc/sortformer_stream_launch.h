// sortformer_stream_launch.h — what the host side of the streaming Sortformer state (sortformer_stream_host.hip: the handle, the argument
// checks, the C ABI) and its kernel unit (sortformer_stream.hip) share: the state's device arrays, the operands of one update, the launch
// plan and the launcher.  The integers: sortformer_stream_core.h.  Internal; not part of the C ABI.  Launch errors surface through
// hipGetLastError().
#pragma once
#include "fa_common.h"
#include "row_pack_launch.h"
#include "sortformer_stream_core.h"

namespace fa {
namespace sfs {

constexpr int kControlBlock = 256;   // one workgroup per stream: validation, preds, scores, the two rank selections, the global selection
constexpr int kMoveBlock = 64;       // a lane owns four columns of one stream for the whole of the FIFO shift
constexpr int kGatherRows = 8;       // rows of the compressed cache one workgroup of the gather fills

// per-stream scalars beside the model-facing lengths: the cache's preds present, the FIFO's preds present, silenceFrameCount
constexpr int kMetaInts = 4;
enum { kMetaSpkPreds = 0, kMetaFifoPreds = 1, kMetaSilCount = 2 };

// The whole state on the device, per stream.  spkcache, spk_len, fifo, fifo_len are what the network reads: fixed for the handle's lifetime.
struct StateArrays {
    float *spkcache;        // [B][spkcache_len][d_model], rows past the length zero
    int32_t *spk_len;       // [B]
    float *fifo;            // [B][fifo_len][d_model], rows past the length zero
    int32_t *fifo_len;      // [B]
    float *spk_preds;       // [B][score_rows][S]
    float *fifo_preds;      // [B][fifo_pred_rows][S]
    float *mean;            // [B][d_model] meanSilenceEmbedding
    int32_t *meta;          // [B][kMetaInts]
    // the library's scratch of one update
    Plan *plan;             // [B]
    uint8_t *silent;        // [B][max_pop]: 1 where the popped frame enters the silence profile
    int32_t *sel;           // [B][spkcache_len]: the source row of every slot of the compressed cache, -1: disabled
    float *popped;          // [B][max_pop][d_model]: the popped rows of a compressing stream
    float *gathered;        // [B][spkcache_len][d_model]: the compressed cache before it replaces the slab
    int32_t B;
};

struct UpdateArgs {
    StateArrays st;
    Config c;
    Slabs slabs;
    Quotas q;
    const void *chunk_embs;     // [B][max_chunk_frames][d_model] fp32 or fp16
    int32_t embs_f16;
    const int32_t *emb_len;     // [B]
    const float *preds;         // [B][pred_stride][S]
    int32_t pred_stride;
    const int32_t *pred_rows;   // [B]
    const int32_t *left, *right;// [B]
    const int32_t *active;      // [B] or null
    float *confirmed;           // [B][max_chunk_frames][S]
    float *tentative;           // [B][max_chunk_frames][S]
    int32_t *counts;            // [B][2]: confirmed rows, tentative rows
    int32_t *status;            // [B]
    float *log_scores;          // [B][score_rows][S] or null
};

struct LaunchPlan {
    unsigned control_grid, move_grid_x, gather_grid_x;
    size_t lds_bytes;
};
inline LaunchPlan launch_plan_of(const Config &c, const Slabs &s) {
    return LaunchPlan{0u, grid_for(c.d_model / 4, kMoveBlock), grid_for(c.spkcache_len, kGatherRows), static_cast<size_t>(s.lds_bytes)};
}

// control, move, gather, replace: four launches whatever the streams do
void launch_update(hipStream_t stream, const UpdateArgs &a);

// the model's chunk rows: a group of streams' mel rows copied as bits, zeros behind them (row_pack.h).  rows: the group's first row
void launch_pack(hipStream_t stream, const float *mel, const rows::Group &g, int64_t row_samples, float *rows, bool wide);

}  // namespace sfs
}  // namespace fa
