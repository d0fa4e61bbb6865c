// embedding_launch.h — what the embedding inputs' host code (embedding_host.hip: the plan, the staging, the records, the C ABI) and their
// kernel translation unit (embedding.hip) share: the limits, the per-item record, the operands of the kernel families and one launcher
// per stage.  The host arithmetic is embedding_geom.h.  Internal; not part of the C ABI.
#pragma once
#include "embedding_geom.h"
#include "fa_common.h"

namespace fa {
namespace embedding {

constexpr int kValid = 1, kFallback = 2, kEmpty = 4;   // ItemRec.flags

struct ItemRec {   // one (planned window, local speaker)
    int32_t flags, first, last, pad;
};

struct StatsArgs {
    const float *w;            // [C][F][S]
    const int32_t *win_chunk;  // [nw] chunk of each planned window
    ItemRec *rec;              // [nw][S]
    float *masks;              // [nw][S][F] chosen masks (skip chain only) or nullptr
    int32_t *bad;
    int32_t nw, F, S, W, exclude;
    float thr, min_frames, min_active;   // Float(minFrames), Float(frames) * 0.2
};

// the index arrays of the selection stage, `items` = nw * S entries each but bsum (select_blocks(items))
struct SelectArgs {
    int32_t *flags;            // [4], zeroed by the caller: [0] a weight is not finite, [1] jobs, [2] runs
    int32_t *bsum;
    int32_t *job_of_item, *item_of_job;   // valid masks -> jobs
    int32_t *is_run, *src;                // job runs the model / the job whose embedding it carries
    int32_t *run_of_src, *job_of_run;     // jobs that run the model -> runs
    int32_t *run_of_job, *window_of_run;  // the outputs
    int32_t B, skip;
    float skip_threshold;
};

struct RowArgs {
    const float *w;
    const int32_t *win_chunk, *item_of_job, *job_of_run;
    const ItemRec *rec;
    int32_t F, S, W, exclude;
    float thr;
};

// Launch errors surface through hipGetLastError().
// workgroups of one compaction over `items` items: the length of SelectArgs.bsum
int64_t select_blocks(int64_t items);
// emb_stats (chunks of up to 8192 weights staged in LDS), the valid-mask compaction, runs_init, skip_chain when s.skip, the run compaction
// and runs_finish; s.flags[1] / [2] hold the job / run counts afterwards
void launch_select(hipStream_t stream, const StatsArgs &a, const SelectArgs &s);
// run_rows -> rows [runs][W] when runs > 0; mask_rows -> mrows [jobs][F] when mrows and jobs > 0
void launch_rows(hipStream_t stream, const RowArgs &a, int64_t runs, float *rows, int64_t jobs, float *mrows);
// out [count][spw]: audio[start[r], start[r] + len[r]) then zeros
void launch_windows(hipStream_t stream, const float *audio, const int64_t *start, const int64_t *len, int64_t count, int32_t spw, float *out);
// out [count][W]: 1 for the first active[r] frames
void launch_spans(hipStream_t stream, const int32_t *active, int64_t count, int32_t W, float *out);
// WeightInterpolation.resample2D: in [rows][n_in] -> out [rows][n_out]
void launch_resample(hipStream_t stream, const float *in, int64_t rows, int32_t n_in, int32_t n_out, float *out);

}  // namespace embedding
}  // namespace fa
