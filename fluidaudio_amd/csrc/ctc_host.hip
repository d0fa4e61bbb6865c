// ctc_host.hip — the host side of the CTC decoder (kernels and launchers: ctc.hip, through ctc_launch.h): the argument checks, the contract
// of the rows entries (ctc_route.h), the staging of the two host-pointer entries and the C ABI.  A host-pointer entry is its checks, the
// staging of its inputs, the _dev entry on the staged buffers, and the copies back.
#include "ctc_launch.h"

namespace {

using namespace fa::ctc;

// a copy or synchronisation of a host-pointer entry: failures are reported under the entry's name
#define FA_CTC_HIP(ctx, entry, expr) FA_TRY(::fa::hip_status((ctx), (expr), (entry)))

fa_status check_args(fa_ctx *ctx, const void *logits, int dtype, int batch, int frames, int vocab, int64_t row_stride,
                     int64_t matrix_stride, const int32_t *token_ids, const int32_t *token_lens) {
    if (!ctx || !token_ids || !token_lens) return FA_INVALID_ARGUMENT;
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "ctc: bad dtype");
    if (batch < 0 || frames < 0 || vocab < 1 || row_stride < vocab) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "ctc: bad shape");
    if (batch > 0 && frames > 0 && (!logits || matrix_stride < static_cast<int64_t>(frames - 1) * row_stride + vocab))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "ctc: bad strides");
    return FA_SUCCESS;
}

// the contract both rows entries share (rows_call_error), wherever the arrays live
fa_status check_rows(fa_ctx *ctx, const int64_t *row_offsets, int64_t total_rows, const int64_t *utt_rows, int32_t batch, const int32_t *token_ids,
                     const int32_t *token_lens) {
    if (!ctx || !token_lens) return FA_INVALID_ARGUMENT;
    const char *err = rows_call_error(batch, total_rows, utt_rows != nullptr, row_offsets != nullptr, token_ids != nullptr);
    return err ? fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s", err) : FA_SUCCESS;
}

// ---------------------------------------------------------------- fa_ctc_greedy_batch

struct BatchBuffers {
    fa::DevBuf in, valid, fid, tok, len;
    size_t in_bytes = 0, id_bytes = 0, len_bytes = 0;
};

fa_status stage_batch(fa_ctx *ctx, const char *entry, const void *logits, int32_t dtype, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride,
                      int64_t matrix_stride, const int32_t *valid_frames, bool want_frame_ids, BatchBuffers &b) {
    const size_t esz = dtype == FA_DTYPE_F16 ? 2 : 4;
    b.in_bytes = frames > 0 ? (static_cast<size_t>(batch - 1) * matrix_stride + static_cast<size_t>(frames - 1) * row_stride + vocab) * esz : 0;
    b.id_bytes = sizeof(int32_t) * static_cast<size_t>(batch) * (frames > 0 ? frames : 1);
    b.len_bytes = sizeof(int32_t) * batch;
    FA_TRY(fa::take_once(ctx, entry, {{&b.in, b.in_bytes}, {&b.tok, b.id_bytes}, {&b.len, b.len_bytes}, {&b.fid, b.id_bytes, want_frame_ids},
                                      {&b.valid, b.len_bytes, valid_frames != nullptr}}));
    if (b.in_bytes) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(b.in.p, logits, b.in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (valid_frames) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(b.valid.p, valid_frames, b.len_bytes, hipMemcpyHostToDevice, ctx->stream));
    return FA_SUCCESS;
}

fa_status collect_batch(fa_ctx *ctx, const char *entry, const BatchBuffers &b, int32_t frames, int32_t *frame_ids, int32_t *token_ids, int32_t *token_lens) {
    if (frames > 0) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(token_ids, b.tok.p, b.id_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (frames > 0 && frame_ids) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(frame_ids, b.fid.p, b.id_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FA_CTC_HIP(ctx, entry, hipMemcpyAsync(token_lens, b.len.p, b.len_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FA_CTC_HIP(ctx, entry, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

// ---------------------------------------------------------------- fa_ctc_greedy_rows

struct RowsBuffers {
    fa::DevBuf val, off, utt, fid, tok, len;
};

fa_status stage_rows(fa_ctx *ctx, const char *entry, const float *values, int64_t n_values, const int64_t *row_offsets, int64_t total_rows,
                     const int64_t *utt_rows, int32_t batch, bool want_frame_ids, RowsBuffers &b) {
    const size_t id_bytes = sizeof(int32_t) * static_cast<size_t>(total_rows > 0 ? total_rows : 1);
    const size_t off_bytes = sizeof(int64_t) * static_cast<size_t>(total_rows + 1), utt_bytes = sizeof(int64_t) * (static_cast<size_t>(batch) + 1);
    FA_TRY(fa::take_once(ctx, entry, {{&b.val, sizeof(float) * static_cast<size_t>(n_values > 0 ? n_values : 1)}, {&b.off, off_bytes}, {&b.tok, id_bytes},
                                      {&b.len, sizeof(int32_t) * batch}, {&b.fid, id_bytes, want_frame_ids}, {&b.utt, utt_bytes, utt_rows != nullptr}}));
    if (n_values > 0) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(b.val.p, values, sizeof(float) * static_cast<size_t>(n_values), hipMemcpyHostToDevice, ctx->stream));
    if (total_rows > 0) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(b.off.p, row_offsets, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (utt_rows) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(b.utt.p, utt_rows, utt_bytes, hipMemcpyHostToDevice, ctx->stream));
    return FA_SUCCESS;
}

fa_status collect_rows(fa_ctx *ctx, const char *entry, const RowsBuffers &b, int64_t total_rows, int32_t batch, int32_t *frame_ids, int32_t *token_ids,
                       int32_t *token_lens) {
    const size_t id_bytes = sizeof(int32_t) * static_cast<size_t>(total_rows);
    if (total_rows > 0) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(token_ids, b.tok.p, id_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (total_rows > 0 && frame_ids) FA_CTC_HIP(ctx, entry, hipMemcpyAsync(frame_ids, b.fid.p, id_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FA_CTC_HIP(ctx, entry, hipMemcpyAsync(token_lens, b.len.p, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, ctx->stream));
    FA_CTC_HIP(ctx, entry, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

fa_status fa_ctc_greedy_batch_dev(fa_ctx *ctx, const void *d_logits, int32_t dtype, int32_t batch, int32_t frames,
                                  int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                                  const int32_t *d_valid_frames, int32_t blank_id, int32_t *d_frame_ids,
                                  int32_t *d_token_ids, int32_t *d_token_lens) {
    FA_TRY(check_args(ctx, d_logits, dtype, batch, frames, vocab, row_stride, matrix_stride, d_token_ids, d_token_lens));
    if (batch == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    CtcArgs a;
    a.logits = d_logits; a.valid_frames = d_valid_frames; a.frame_ids = d_frame_ids; a.token_ids = d_token_ids;
    a.token_lens = d_token_lens; a.row_stride = row_stride; a.matrix_stride = matrix_stride; a.frames = frames;
    a.vocab = vocab; a.blank_id = blank_id;
    launch_greedy(ctx->stream, a, dtype == FA_DTYPE_F16, batch);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_ctc_greedy_batch(fa_ctx *ctx, const void *logits, int32_t dtype, int32_t batch, int32_t frames, int32_t vocab,
                              int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames, int32_t blank_id,
                              int32_t *frame_ids, int32_t *token_ids, int32_t *token_lens) {
    FA_TRY(check_args(ctx, logits, dtype, batch, frames, vocab, row_stride, matrix_stride, token_ids, token_lens));
    if (batch == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    BatchBuffers b;
    FA_TRY(stage_batch(ctx, __func__, logits, dtype, batch, frames, vocab, row_stride, matrix_stride, valid_frames, frame_ids != nullptr, b));
    FA_TRY(fa_ctc_greedy_batch_dev(ctx, b.in.p, dtype, batch, frames, vocab, row_stride, matrix_stride, valid_frames ? b.valid.as<int32_t>() : nullptr,
                                   blank_id, frame_ids ? b.fid.as<int32_t>() : nullptr, b.tok.as<int32_t>(), b.len.as<int32_t>()));
    return collect_batch(ctx, __func__, b, frames, frame_ids, token_ids, token_lens);
}

fa_status fa_ctc_greedy_rows_dev(fa_ctx *ctx, const float *d_values, const int64_t *d_row_offsets, int64_t total_rows, const int64_t *d_utt_rows,
                                 int32_t batch, int32_t blank_id, int32_t *d_frame_ids, int32_t *d_token_ids, int32_t *d_token_lens) {
    FA_TRY(check_rows(ctx, d_row_offsets, total_rows, d_utt_rows, batch, d_token_ids, d_token_lens));
    if (batch == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    CtcRowsArgs a;
    a.values = d_values; a.row_offsets = d_row_offsets; a.utt_rows = d_utt_rows; a.frame_ids = d_frame_ids; a.token_ids = d_token_ids;
    a.token_lens = d_token_lens; a.total_rows = total_rows; a.blank_id = blank_id;
    launch_greedy_rows(ctx->stream, a, batch);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_ctc_greedy_rows(fa_ctx *ctx, const float *values, const int64_t *row_offsets, int64_t total_rows, const int64_t *utt_rows, int32_t batch,
                             int32_t blank_id, int32_t *frame_ids, int32_t *token_ids, int32_t *token_lens) {
    FA_TRY(check_rows(ctx, row_offsets, total_rows, utt_rows, batch, token_ids, token_lens));
    if (batch == 0) return FA_SUCCESS;
    // the offsets are the caller's, and readable here
    if (const char *err = rows_offsets_error(row_offsets, total_rows, utt_rows, batch)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s", err);
    const int64_t n_values = total_rows > 0 ? row_offsets[total_rows] : 0;
    if (n_values > 0 && !values) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "ctc rows: null values");
    fa::DeviceGuard guard(ctx->device);
    RowsBuffers b;
    FA_TRY(stage_rows(ctx, __func__, values, n_values, row_offsets, total_rows, utt_rows, batch, frame_ids != nullptr, b));
    FA_TRY(fa_ctc_greedy_rows_dev(ctx, b.val.as<float>(), b.off.as<int64_t>(), total_rows, utt_rows ? b.utt.as<int64_t>() : nullptr, batch, blank_id,
                                  frame_ids ? b.fid.as<int32_t>() : nullptr, b.tok.as<int32_t>(), b.len.as<int32_t>()));
    return collect_rows(ctx, __func__, b, total_rows, batch, frame_ids, token_ids, token_lens);
}

fa_status fa_ctc_log_softmax_batch_dev(fa_ctx *ctx, const void *d_logits, int32_t dtype, int32_t batch, int32_t frames, int32_t vocab,
                                       int64_t row_stride, int64_t matrix_stride, float temperature, float blank_bias, int32_t blank_id,
                                       float *d_log_probs) {
    if (!ctx || !d_log_probs) return FA_INVALID_ARGUMENT;
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "log_softmax: bad dtype");
    if (batch < 0 || frames < 0 || vocab < 1 || row_stride < vocab || !(temperature > 0.0f)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "log_softmax: bad shape");
    if (batch == 0 || frames == 0) return FA_SUCCESS;
    if (!d_logits || matrix_stride < static_cast<int64_t>(frames - 1) * row_stride + vocab) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "log_softmax: bad strides");
    fa::DeviceGuard guard(ctx->device);
    LsmArgs a{};
    a.logits = d_logits; a.out = d_log_probs; a.row_stride = row_stride; a.matrix_stride = matrix_stride;
    a.out_row_stride = vocab; a.out_matrix_stride = static_cast<int64_t>(frames) * vocab;
    a.rows_total = static_cast<int64_t>(batch) * frames; a.frames = frames; a.vocab = vocab; a.blank_id = blank_id;
    a.temperature = temperature; a.blank_bias = blank_bias;
    launch_log_softmax(ctx->stream, a, dtype == FA_DTYPE_F16);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // extern "C"
