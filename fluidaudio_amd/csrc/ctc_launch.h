// ctc_launch.h — what the CTC decoder's host code (ctc_host.hip: the argument checks, the rows contract, the staging of the host-pointer
// entries, the C ABI) and its kernel translation unit (ctc.hip) share: the launch geometry and the routes (ctc_route.h), the operands of the
// three kernel families and one launcher per family.  Template arguments are named in ctc.hip only.  Internal; not part of the C ABI.
// Launch errors surface through hipGetLastError().
#pragma once
#include "ctc_route.h"
#include "fa_common.h"

namespace fa {
namespace ctc {

struct CtcArgs {
    const void *logits;
    const int32_t *valid_frames;
    int32_t *frame_ids;
    int32_t *token_ids;
    int32_t *token_lens;
    int64_t row_stride, matrix_stride;
    int32_t frames, vocab, blank_id;
};

struct CtcRowsArgs {
    const float *values;
    const int64_t *row_offsets;   // [total_rows + 1], non-decreasing
    const int64_t *utt_rows;      // [batch + 1], non-decreasing; NULL: one utterance of `total_rows` rows
    int32_t *frame_ids;           // [total_rows] or NULL: argmax per frame, -1 for an empty frame
    int32_t *token_ids;           // [total_rows]: utterance u writes from token_ids[utt_rows[u]]
    int32_t *token_lens;          // [batch]
    int64_t total_rows;
    int32_t blank_id;
};

struct LsmArgs {
    const void *logits;
    float *out;
    int64_t row_stride, matrix_stride, out_row_stride, out_matrix_stride, rows_total;
    int32_t frames, vocab, blank_id;
    float inv_temp_unused, temperature, blank_bias;
};

// ctc_greedy_kernel<F16, MODE> on `batch` matrices, one workgroup each: the instance greedy_mode names for the operands
void launch_greedy(hipStream_t stream, const CtcArgs &a, bool f16, int batch);
// ctc_greedy_rows_kernel on `batch` utterances, one workgroup each
void launch_greedy_rows(hipStream_t stream, const CtcRowsArgs &a, int batch);
// the log-softmax of a.rows_total rows, one wavefront per row: ctc_log_softmax_vec4_kernel where log_softmax_vec4 allows it
void launch_log_softmax(hipStream_t stream, const LsmArgs &a, bool f16);

}  // namespace ctc
}  // namespace fa
