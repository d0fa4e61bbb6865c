// aed_host.hip — the host side of the AED unit (kernels: aed.hip, plans and argument passes: aed_launch.h, shared integers:
// aed_core.h): the defaults, the C ABI, the uploads and the one synchronisation of the entries that have one.  The step entry
// allocates nothing and does not synchronise: it is one launch in the caller's decode loop.
#include <algorithm>

#include "fa_common.h"
#include "aed_launch.h"

namespace fa {
namespace aed {
void launch_begin(hipStream_t stream, const BeginArgs &a, int32_t batch);
void launch_step(hipStream_t stream, const StepArgs &a, const StepPlan &p);
void launch_finish(hipStream_t stream, const FinishArgs &a);
void launch_cross_mask(hipStream_t stream, const int32_t *valid, int32_t batch, int32_t len, int32_t f16, void *mask);
void launch_context(hipStream_t stream, const StridedArgs &a, const int32_t *len, float *emb, float *mask);
void launch_gather(hipStream_t stream, const StridedArgs &a, const Layout &lay, const int32_t *state, float *hidden);
void launch_merge(hipStream_t stream, const MergeArgs &a);
}  // namespace aed
}  // namespace fa

namespace {

namespace ad = fa::aed;

fa_status refused(fa_ctx *ctx, const char *entry, const fa::Verdict &v) { return fa::set_error(ctx, v.status, "%s: %s", entry, v.text); }

fa_status finish(fa_ctx *ctx, const fa_aed_config *cfg, const int32_t batch, const void *d_state, const int32_t max_out, int32_t *tokens, int32_t *counts,
                 int32_t *reasons, int32_t *steps, const bool device) {
    const char *entry = device ? "aed_finish_dev" : "aed_finish";
    const fa::Verdict v = ad::check_finish(cfg, batch, d_state, max_out, tokens, counts);
    if (v.status != FA_SUCCESS) return refused(ctx, entry, v);
    if (!ctx) return FA_INVALID_ARGUMENT;
    return fa::no_throw(ctx, entry, [&]() -> fa_status {
        fa::DeviceGuard guard(ctx->device);
        const size_t B = static_cast<size_t>(batch), cells = B * static_cast<size_t>(max_out);
        fa::DevBuf b_out;
        if (!device) FA_TRY(fa::take(ctx, entry, {{&b_out, sizeof(int32_t) * (cells + 3 * B)}}));
        ad::FinishArgs a{ad::layout_of(*cfg), static_cast<const int32_t *>(d_state), batch, max_out, tokens, counts, reasons, steps};
        if (!device) {
            a.tokens = b_out.as<int32_t>();
            a.counts = a.tokens + cells;
            a.reasons = a.counts + B;
            a.steps = a.reasons + B;
        }
        ad::launch_finish(ctx->stream, a);
        FA_HIP_TRY(ctx, hipGetLastError());
        if (device) return FA_SUCCESS;
        FA_HIP_TRY(ctx, hipMemcpyAsync(tokens, a.tokens, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(counts, a.counts, sizeof(int32_t) * B, hipMemcpyDeviceToHost, ctx->stream));
        if (reasons) FA_HIP_TRY(ctx, hipMemcpyAsync(reasons, a.reasons, sizeof(int32_t) * B, hipMemcpyDeviceToHost, ctx->stream));
        if (steps) FA_HIP_TRY(ctx, hipMemcpyAsync(steps, a.steps, sizeof(int32_t) * B, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the call's one synchronisation
        return FA_SUCCESS;
    });
}

fa_status merge(fa_ctx *ctx, const fa_aed_config *cfg, const int32_t *tokens, const int64_t *window_offsets, const int64_t *recording_range, const int64_t n,
                int32_t *out, const int64_t *out_range, int32_t *out_counts, int32_t *seam_best_len, int32_t *seam_best_send, const bool device) {
    const char *entry = device ? "aed_merge_windows_dev" : "aed_merge_windows";
    const fa::Verdict v = ad::check_merge(cfg, tokens, window_offsets, recording_range, n, out, out_range, out_counts);
    if (v.status != FA_SUCCESS) return refused(ctx, entry, v);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, entry, [&]() -> fa_status {
        const size_t N = static_cast<size_t>(n), w0 = static_cast<size_t>(recording_range[0]), W = static_cast<size_t>(recording_range[n]) - w0;
        const int64_t t0 = window_offsets[w0], o0 = out_range[0];
        const size_t T = static_cast<size_t>(window_offsets[w0 + W] - t0), O = static_cast<size_t>(out_range[n] - o0);
        std::vector<ad::MergeRec> recs(N);
        for (size_t r = 0; r < N; ++r) recs[r] = ad::MergeRec{recording_range[r] - recording_range[0], recording_range[r + 1] - recording_range[0], out_range[r] - o0};
        std::vector<int64_t> offs(W + 1);
        for (size_t w = 0; w <= W; ++w) offs[w] = window_offsets[w0 + w] - t0;

        fa::DeviceGuard guard(ctx->device);
        hipStream_t st = ctx->stream;
        fa::DevBuf b_recs, b_offs, b_res, b_tok, b_out;
        FA_TRY(fa::take(ctx, entry, {{&b_recs, sizeof(ad::MergeRec) * N, true, recs.data()}, {&b_offs, sizeof(int64_t) * (W + 1), true, offs.data()},
                                     {&b_res, sizeof(int32_t) * (N + 2 * W)}, {&b_tok, sizeof(int32_t) * T, !device, tokens ? tokens + t0 : nullptr},
                                     {&b_out, sizeof(int32_t) * O, !device}}));
        ad::MergeArgs a{};
        a.tokens = device ? tokens + t0 : b_tok.as<int32_t>();
        a.win_off = b_offs.as<int64_t>();
        a.recs = b_recs.as<ad::MergeRec>();
        a.n_recs = static_cast<int32_t>(n);
        a.window_tokens = cfg ? cfg->window_tokens : 32;
        a.min_match = cfg ? cfg->min_match : 4;
        a.out = device ? out + o0 : b_out.as<int32_t>();
        a.counts = b_res.as<int32_t>();
        a.best_len = a.counts + N;
        a.best_send = a.best_len + W;
        ad::launch_merge(st, a);
        FA_HIP_TRY(ctx, hipGetLastError());
        std::vector<int32_t> res(N + 2 * W);
        FA_HIP_TRY(ctx, hipMemcpyAsync(res.data(), b_res.p, sizeof(int32_t) * res.size(), hipMemcpyDeviceToHost, st));
        if (!device && O) FA_HIP_TRY(ctx, hipMemcpyAsync(out + o0, a.out, sizeof(int32_t) * O, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
        std::copy(res.begin(), res.begin() + n, out_counts);
        if (seam_best_len) std::copy(res.begin() + N, res.begin() + N + W, seam_best_len + w0);
        if (seam_best_send) std::copy(res.begin() + N + W, res.end(), seam_best_send + w0);
        return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_aed_default_config(fa_aed_config *cfg, int32_t model) {
    if (cfg) *cfg = ad::default_config(model);
}

int32_t fa_aed_max_out(const fa_aed_config *cfg) { return ad::check_decode_config(cfg).status == FA_SUCCESS ? ad::max_out_of(*cfg) : 0; }

int64_t fa_aed_state_bytes(const fa_aed_config *cfg, int32_t batch) {
    if (ad::check_decode_config(cfg).status != FA_SUCCESS || batch < 1) return 0;
    return static_cast<int64_t>(sizeof(int32_t)) * ad::layout_of(*cfg).words() * batch;
}

int32_t fa_aed_encoder_valid_frames(int64_t feature_length, int32_t encoder_seq_len, int32_t mel_frames, int32_t encoder_frames) {
    if (feature_length < 0 || encoder_seq_len < 0 || mel_frames < 1 || encoder_frames < 0 || feature_length > INT64_MAX / std::max(encoder_frames, 1)) return 0;
    return static_cast<int32_t>(ad::encoder_valid_frames(feature_length, encoder_seq_len, mel_frames, encoder_frames));
}

fa_status fa_aed_begin_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const int32_t *d_prompts, int32_t prompt_stride, const int32_t *prompt_lens,
                           void *d_state, int32_t *d_input_id, int32_t *d_position_id, void *d_self_mask, int32_t mask_dtype, int32_t *d_input_ids,
                           float *d_decoder_mask) {
    const fa::Verdict v = ad::check_begin(cfg, batch, d_prompts, prompt_stride, prompt_lens, d_state, d_input_id, d_position_id, d_self_mask, mask_dtype, d_input_ids,
                                          d_decoder_mask);
    if (v.status != FA_SUCCESS) return refused(ctx, "aed_begin_dev", v);
    if (!ctx) return FA_INVALID_ARGUMENT;
    return fa::no_throw(ctx, "aed_begin_dev", [&]() -> fa_status {
        fa::DeviceGuard guard(ctx->device);
        fa::DevBuf b_lens;
        FA_TRY(fa::take(ctx, "aed_begin_dev", {{&b_lens, sizeof(int32_t) * static_cast<size_t>(batch), true, prompt_lens}}));
        const ad::BeginArgs a{*cfg, ad::layout_of(*cfg), static_cast<int32_t *>(d_state), d_prompts, b_lens.as<int32_t>(), prompt_stride, d_input_id, d_position_id,
                              d_self_mask, mask_dtype == FA_DTYPE_F16 ? 1 : 0, d_input_ids, d_decoder_mask};
        ad::launch_begin(ctx->stream, a, batch);
        FA_HIP_TRY(ctx, hipGetLastError());
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the uploaded lengths live until here
        return FA_SUCCESS;
    });
}

fa_status fa_aed_step_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, void *d_state, const void *d_logits, int32_t dtype, int64_t row_stride,
                          int32_t *d_input_id, int32_t *d_position_id, void *d_self_mask, int32_t mask_dtype, int32_t *d_input_ids, float *d_decoder_mask) {
    const fa::Verdict v = ad::check_step(cfg, batch, d_state, d_logits, dtype, row_stride, d_input_id, d_position_id, d_self_mask, mask_dtype, d_input_ids, d_decoder_mask);
    if (v.status != FA_SUCCESS) return refused(ctx, "aed_step_dev", v);
    if (!ctx) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    const ad::StepPlan p = ad::step_plan(*cfg, batch);
    const ad::StepArgs a{*cfg, ad::layout_of(*cfg), static_cast<int32_t *>(d_state), d_logits, dtype == FA_DTYPE_F16 ? 1 : 0, p.marked, row_stride, d_input_id, d_position_id,
                         d_self_mask, mask_dtype == FA_DTYPE_F16 ? 1 : 0, d_input_ids, d_decoder_mask};
    ad::launch_step(ctx->stream, a, p);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_aed_finish_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const void *d_state, int32_t max_out, int32_t *d_tokens, int32_t *d_counts,
                            int32_t *d_reasons, int32_t *d_steps) {
    return finish(ctx, cfg, batch, d_state, max_out, d_tokens, d_counts, d_reasons, d_steps, true);
}
fa_status fa_aed_finish(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const void *d_state, int32_t max_out, int32_t *tokens, int32_t *counts, int32_t *reasons,
                        int32_t *steps) {
    return finish(ctx, cfg, batch, d_state, max_out, tokens, counts, reasons, steps, false);
}

fa_status fa_aed_cross_mask_dev(fa_ctx *ctx, const int32_t *d_valid, int32_t batch, int32_t encoder_seq_len, int32_t mask_dtype, void *d_mask) {
    if (batch < 1 || encoder_seq_len < 1 || !d_valid || !d_mask || !ad::mask_dtype_ok(mask_dtype))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "aed_cross_mask_dev: batch and encoder_seq_len >= 1, d_valid and d_mask required, an fp32 or fp16 mask");
    if (!ctx) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    ad::launch_cross_mask(ctx->stream, d_valid, batch, encoder_seq_len, mask_dtype == FA_DTYPE_F16 ? 1 : 0, d_mask);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_aed_encoder_context_dev(fa_ctx *ctx, const void *d_enc, int32_t dtype, int32_t batch, int32_t D, int32_t T, int64_t stride_b, int64_t stride_d,
                                     int64_t stride_t, const int32_t *d_len, float *d_emb, float *d_mask) {
    const fa::Verdict v = ad::check_strided(batch, D, T, stride_b, stride_d, stride_t, dtype);
    if (v.status != FA_SUCCESS) return refused(ctx, "aed_encoder_context_dev", v);
    if (!d_enc || !d_len || !d_emb || !d_mask || batch > 65535) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "aed_encoder_context_dev: every array is required; batch <= 65535");
    if (!ctx) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    ad::launch_context(ctx->stream, ad::StridedArgs{d_enc, dtype == FA_DTYPE_F16 ? 1 : 0, batch, D, T, stride_b, stride_d, stride_t}, d_len, d_emb, d_mask);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_aed_gather_hidden_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const void *d_state, const void *d_dec, int32_t dtype, int32_t S, int32_t D,
                                   int64_t stride_b, int64_t stride_s, int64_t stride_d, float *d_hidden) {
    const fa::Verdict c = ad::check_decode_config(cfg);
    if (c.status != FA_SUCCESS) return refused(ctx, "aed_gather_hidden_dev", c);
    const fa::Verdict v = ad::check_strided(batch, S, D, stride_b, stride_s, stride_d, dtype);
    if (v.status != FA_SUCCESS) return refused(ctx, "aed_gather_hidden_dev", v);
    if (!d_state || !d_dec || !d_hidden || cfg->mode != FA_AED_FEED_SEQUENCE)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "aed_gather_hidden_dev: every array is required; the state is a sequence feed's");
    if (!ctx) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    ad::launch_gather(ctx->stream, ad::StridedArgs{d_dec, dtype == FA_DTYPE_F16 ? 1 : 0, batch, S, D, stride_b, stride_s, stride_d}, ad::layout_of(*cfg),
                      static_cast<const int32_t *>(d_state), d_hidden);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_aed_plan_windows(const fa_aed_config *cfg, const int64_t *samples, int64_t n, int64_t *window_range, int64_t *starts, int64_t *lens, int64_t capacity,
                              int64_t *count) {
    if (ad::check_windows(cfg, samples, n, window_range, starts, lens, capacity, count).status != FA_SUCCESS) return FA_INVALID_ARGUMENT;
    const fa::Verdict v = ad::count_windows(*cfg, samples, n, window_range, count);
    if (v.status != FA_SUCCESS) return v.status;
    if (!starts) return FA_SUCCESS;
    if (*count > capacity) return FA_OUTPUT_TOO_SMALL;
    for (int64_t r = 0; r < n; ++r) ad::plan_windows_one(samples[r], cfg->chunk_samples, cfg->hop_samples, starts + window_range[r], lens + window_range[r]);
    return FA_SUCCESS;
}

fa_status fa_aed_merge_windows_dev(fa_ctx *ctx, const fa_aed_config *cfg, const int32_t *d_tokens, const int64_t *window_offsets, const int64_t *recording_range,
                                   int64_t n_recordings, int32_t *d_out, const int64_t *out_range, int32_t *out_counts, int32_t *seam_best_len, int32_t *seam_best_send) {
    return merge(ctx, cfg, d_tokens, window_offsets, recording_range, n_recordings, d_out, out_range, out_counts, seam_best_len, seam_best_send, true);
}
fa_status fa_aed_merge_windows(fa_ctx *ctx, const fa_aed_config *cfg, const int32_t *tokens, const int64_t *window_offsets, const int64_t *recording_range,
                               int64_t n_recordings, int32_t *out, const int64_t *out_range, int32_t *out_counts, int32_t *seam_best_len, int32_t *seam_best_send) {
    return merge(ctx, cfg, tokens, window_offsets, recording_range, n_recordings, out, out_range, out_counts, seam_best_len, seam_best_send, false);
}

}  // extern "C"
