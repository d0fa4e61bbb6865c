// tdt_host.hip — the host side of the TDT decoder (kernels and launchers: tdt.hip, through tdt_launch.h): the navigation helpers
// (TdtFrameNavigation.swift:20-105, TdtDurationMapping.swift:17-31, TdtConfig.swift:13-26), the argument checks and the C ABI.  The tables
// entry and the logits entry share one body: the same checks, the same operands, another source of joint decisions; the language entry is the
// logits entry with the filters' operands.  The class bytes of a vocabulary (no device): tdt_lang_host.hip.
#include "tdt_launch.h"

namespace {

using namespace fa::tdt;

struct Logits {   // the joint logits of fa_tdt_greedy_logits_dev
    const void *p;
    int32_t dtype, vocab_with_blank;
    int64_t row_stride;
};

struct Lang {     // what fa_tdt_greedy_logits_lang_dev adds
    const uint8_t *classes;
    int32_t script, use_blocklist, top_k;
    int32_t *out_route, *swap_counts;
};

// lg: the walk decides on joint logits; otherwise on the tables tok / bin / prob.  lang (with lg only): the language mode
fa_status greedy(fa_ctx *ctx, const fa_tdt_config *cfg, const Logits *lg, const Lang *lang, const int32_t *tok, const int32_t *bin, const float *prob, int32_t batch,
                 int32_t U, int32_t T, const int32_t *enc_len, const int32_t *audio_frames, const int32_t *t0, const int32_t *is_last,
                 const int32_t *global_offset, const int32_t *emit_after, int32_t max_out, int32_t *out_tok, int32_t *out_time, int32_t *out_dur,
                 float *out_conf, int32_t *out_count, int32_t *final_time, int32_t *final_u, int32_t *status) {
    if (!ctx || !cfg) return FA_INVALID_ARGUMENT;
    if (batch == 0) return FA_SUCCESS;
    const bool decisions = lg ? lg->vocab_with_blank >= 1 && lg->row_stride >= static_cast<int64_t>(lg->vocab_with_blank) + cfg->n_duration_bins &&
                                    (lg->dtype == FA_DTYPE_F32 || lg->dtype == FA_DTYPE_F16) && lg->p
                              : tok && bin && prob;
    if (batch < 0 || U < 1 || T < 1 || max_out < 0 || cfg->n_duration_bins < 1 || cfg->n_duration_bins > 8 || !decisions || !enc_len || !out_count ||
        !final_time || !final_u || !status || (max_out > 0 && (!out_tok || !out_time || !out_dur || !out_conf)))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "tdt: bad arguments");
    if (lang && (!lang->classes || !lang->swap_counts || (max_out > 0 && !lang->out_route) || lang->script < FA_TDT_SCRIPT_LATIN ||
                 lang->script > FA_TDT_SCRIPT_GREEK || lang->top_k < 1 || lang->top_k > FA_TDT_MAX_TOP_K))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "tdt: bad language arguments (script 0 .. 2, top_k 1 .. 64, class bytes, route and swap-count outputs)");
    fa::DeviceGuard guard(ctx->device);
    TdtArgs a;
    a.tok = tok; a.bin = bin; a.prob = prob; a.enc_len = enc_len; a.audio_frames = audio_frames; a.t0 = t0;
    a.is_last = is_last; a.global_offset = global_offset; a.emit_after = emit_after;
    a.out_tok = out_tok; a.out_time = out_time; a.out_dur = out_dur; a.out_conf = out_conf; a.out_count = out_count;
    a.final_time = final_time; a.final_u = final_u; a.status = status;
    a.B = batch; a.U = U; a.T = T; a.max_out = max_out; a.cfg = *cfg;
    static_assert((FA_TDT_CLASS_LATIN_OK << FA_TDT_SCRIPT_CYRILLIC) == FA_TDT_CLASS_CYRILLIC_OK && (FA_TDT_CLASS_LATIN_OK << FA_TDT_SCRIPT_GREEK) == FA_TDT_CLASS_GREEK_OK,
                  "script s matches by class bit s");
    if (lang) launch_logits_lang(ctx->stream, a, TdtLogitArgs{lg->p, lg->dtype == FA_DTYPE_F16 ? 1 : 0, lg->vocab_with_blank, cfg->n_duration_bins, lg->row_stride},
                                 TdtLangArgs{lang->classes, FA_TDT_CLASS_LATIN_OK << lang->script, lang->use_blocklist != 0, lang->top_k, lang->out_route, lang->swap_counts});
    else if (lg) launch_logits(ctx->stream, a, TdtLogitArgs{lg->p, lg->dtype == FA_DTYPE_F16 ? 1 : 0, lg->vocab_with_blank, cfg->n_duration_bins, lg->row_stride});
    else launch_tables(ctx->stream, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

void fa_tdt_default_config(fa_tdt_config *c) {  // TdtConfig.swift:13-26
    if (!c) return;
    c->blank_id = 8192; c->max_symbols_per_step = 10; c->max_tokens_per_chunk = 150; c->consecutive_blank_limit = 5;
    c->n_duration_bins = 5;
    for (int i = 0; i < 8; ++i) c->duration_bins[i] = i < 5 ? i : 0;
}

int32_t fa_tdt_initial_time_index(int32_t has_time_jump, int32_t time_jump, int32_t context_frame_adjustment) {
    // TdtFrameNavigation.calculateInitialTimeIndices (TdtFrameNavigation.swift:20-49)
    if (!has_time_jump) return context_frame_adjustment;
    if (time_jump == 0 && context_frame_adjustment == 0) return kStandardOverlapFrames;
    const int32_t v = time_jump + context_frame_adjustment;
    return v > 0 ? v : 0;
}

void fa_tdt_navigation_state(int32_t time_indices, int32_t encoder_sequence_length, int32_t actual_audio_frames,
                             int32_t *effective_length, int32_t *safe_time_indices, int32_t *last_timestep, int32_t *active) {
    // TdtFrameNavigation.initializeNavigationState (:59-78)
    const int32_t eff = encoder_sequence_length < actual_audio_frames ? encoder_sequence_length : actual_audio_frames;
    if (effective_length) *effective_length = eff;
    if (safe_time_indices) *safe_time_indices = time_indices < eff - 1 ? time_indices : eff - 1;
    if (last_timestep) *last_timestep = eff - 1;
    if (active) *active = time_indices < eff;
}

int32_t fa_tdt_final_time_jump(int32_t current_time_indices, int32_t effective_length, int32_t is_last_chunk, int32_t *has_value) {
    // TdtFrameNavigation.calculateFinalTimeJump (:91-105): nil for the last chunk
    if (has_value) *has_value = !is_last_chunk;
    return is_last_chunk ? 0 : current_time_indices - effective_length;
}

fa_status fa_tdt_map_duration_bin(const fa_tdt_config *cfg, int32_t bin_index, int32_t *duration) {
    if (!cfg || !duration) return FA_INVALID_ARGUMENT;
    if (bin_index < 0 || bin_index >= cfg->n_duration_bins) return FA_RUNTIME_ERROR;  // "Duration bin index out of range" (:19-21)
    *duration = cfg->duration_bins[bin_index];
    return FA_SUCCESS;
}

float fa_tdt_clamp_probability(float v) { return clamp_probability(v); }

fa_status fa_tdt_greedy_tables_dev(fa_ctx *ctx, const fa_tdt_config *cfg, const int32_t *d_tok, const int32_t *d_bin, const float *d_prob,
                                   int32_t batch, int32_t U, int32_t T, const int32_t *d_enc_len, const int32_t *d_audio_frames,
                                   const int32_t *d_t0, const int32_t *d_is_last, const int32_t *d_global_offset,
                                   const int32_t *d_emit_after, int32_t max_out, int32_t *d_out_tok, int32_t *d_out_time,
                                   int32_t *d_out_dur, float *d_out_conf, int32_t *d_out_count, int32_t *d_final_time,
                                   int32_t *d_final_u, int32_t *d_status) {
    return greedy(ctx, cfg, nullptr, nullptr, d_tok, d_bin, d_prob, batch, U, T, d_enc_len, d_audio_frames, d_t0, d_is_last, d_global_offset, d_emit_after,
                  max_out, d_out_tok, d_out_time, d_out_dur, d_out_conf, d_out_count, d_final_time, d_final_u, d_status);
}

fa_status fa_tdt_greedy_logits_dev(fa_ctx *ctx, const fa_tdt_config *cfg, const void *d_logits, int32_t dtype, int32_t batch, int32_t U, int32_t T,
                                   int32_t vocab_with_blank, int64_t row_stride, const int32_t *d_enc_len, const int32_t *d_audio_frames,
                                   const int32_t *d_t0, const int32_t *d_is_last, const int32_t *d_global_offset, const int32_t *d_emit_after,
                                   int32_t max_out, int32_t *d_out_tok, int32_t *d_out_time, int32_t *d_out_dur, float *d_out_conf,
                                   int32_t *d_out_count, int32_t *d_final_time, int32_t *d_final_u, int32_t *d_status) {
    const Logits lg{d_logits, dtype, vocab_with_blank, row_stride};
    return greedy(ctx, cfg, &lg, nullptr, nullptr, nullptr, nullptr, batch, U, T, d_enc_len, d_audio_frames, d_t0, d_is_last, d_global_offset, d_emit_after,
                  max_out, d_out_tok, d_out_time, d_out_dur, d_out_conf, d_out_count, d_final_time, d_final_u, d_status);
}

fa_status fa_tdt_greedy_logits_lang_dev(fa_ctx *ctx, const fa_tdt_config *cfg, const void *d_logits, int32_t dtype, int32_t batch, int32_t U, int32_t T,
                                        int32_t vocab_with_blank, int64_t row_stride, const int32_t *d_enc_len, const int32_t *d_audio_frames,
                                        const int32_t *d_t0, const int32_t *d_is_last, const int32_t *d_global_offset, const int32_t *d_emit_after,
                                        int32_t max_out, int32_t *d_out_tok, int32_t *d_out_time, int32_t *d_out_dur, float *d_out_conf,
                                        int32_t *d_out_count, int32_t *d_final_time, int32_t *d_final_u, int32_t *d_status, const uint8_t *d_classes,
                                        int32_t script, int32_t use_blocklist, int32_t top_k, int32_t *d_out_route, int32_t *d_swap_counts) {
    const Logits lg{d_logits, dtype, vocab_with_blank, row_stride};
    const Lang lang{d_classes, script, use_blocklist, top_k, d_out_route, d_swap_counts};
    return greedy(ctx, cfg, &lg, &lang, nullptr, nullptr, nullptr, batch, U, T, d_enc_len, d_audio_frames, d_t0, d_is_last, d_global_offset, d_emit_after,
                  max_out, d_out_tok, d_out_time, d_out_dur, d_out_conf, d_out_count, d_final_time, d_final_u, d_status);
}

fa_status fa_tdt_topk_rows_dev(fa_ctx *ctx, const void *d_rows, int32_t dtype, int64_t R, int32_t vocab_with_blank, int64_t row_stride, int32_t K,
                               int32_t *d_ids, float *d_logits, int32_t *d_counts) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (R == 0) return FA_SUCCESS;
    if (R < 0 || R > INT32_MAX || vocab_with_blank < 1 || row_stride < vocab_with_blank || K < 1 || K > FA_TDT_MAX_TOP_K ||
        (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) || !d_rows || !d_ids || !d_logits)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "tdt top-k: bad arguments (1 <= K <= 64, fp32 / fp16 rows of at least vocab_with_blank logits)");
    fa::DeviceGuard guard(ctx->device);
    launch_topk(ctx->stream, TdtTopkArgs{d_rows, dtype == FA_DTYPE_F16 ? 1 : 0, vocab_with_blank, K, R, row_stride, d_ids, d_logits, d_counts});
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // extern "C"
