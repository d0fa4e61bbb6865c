// rnnt_host.hip — the host side of the streaming RNN-T walk (kernel and launcher: rnnt.hip, through rnnt_launch.h): the defaults,
// the argument checks and the C ABI of the walk, and the C entries of the hotword-bias tables
// (rnnt_bias_core.h: NemotronVocabularyBias.swift:126-339) — those need no context and no device.
#include "rnnt_launch.h"

extern "C" {

void fa_rnnt_default_config(fa_rnnt_config *c) {
    if (!c) return;   // the Nemotron streaming defaults: blankIdx (NemotronStreamingConfig.swift:45), no end-of-utterance token, ten symbols per frame
    c->blank_id = 1024; c->eou_id = -1; c->max_symbols_per_step = 10;
}

float fa_rnnt_bias_effective_boost(int32_t has_weight, float weight, float default_boost) {
    return fa::rnnt_bias::effective_boost(has_weight, weight, default_boost);
}

fa_status fa_rnnt_bias_build(const char *const *folded_pieces, int32_t vocab, const char *const *folded_surfaces, const float *boosts, int32_t n_surfaces,
                             int32_t *blob, int64_t capacity_words, int64_t *words_needed, int32_t *tail_cap) {
    return fa::no_throw(nullptr, "fa_rnnt_bias_build", [&]() {
        return static_cast<fa_status>(fa::rnnt_bias::build(folded_pieces, vocab, folded_surfaces, boosts, n_surfaces, blob, capacity_words, words_needed, tail_cap));
    });
}

fa_status fa_rnnt_bias_candidates(const int32_t *blob, int64_t words, const int32_t *observed, int32_t n_observed, int32_t *ids, float *boosts,
                                  int32_t capacity, int32_t *count) {
    return fa::no_throw(nullptr, "fa_rnnt_bias_candidates", [&]() {
        return static_cast<fa_status>(fa::rnnt_bias::candidates(blob, words, observed, n_observed, ids, boosts, capacity, count));
    });
}

fa_status fa_rnnt_greedy_logits_dev(fa_ctx *ctx, const fa_rnnt_config *cfg, const void *d_logits, int32_t dtype, int32_t batch, int32_t U, int32_t T,
                                    int32_t vocab_with_blank, int64_t row_stride, const int32_t *d_frames, const int32_t *d_skip, const int32_t *d_bias,
                                    int64_t bias_words, int32_t tail_cap, int32_t *d_tail, int32_t *d_tail_len, int32_t max_out, int32_t *d_out_tok,
                                    int32_t *d_out_frame, int32_t *d_out_plain, int32_t *d_out_count, int32_t *d_final_u, int32_t *d_eou, int32_t *d_status) {
    if (!ctx || !cfg) return FA_INVALID_ARGUMENT;
    if (batch <= 0 || U <= 0 || T <= 0 || vocab_with_blank <= 0 || row_stride < vocab_with_blank || max_out < 0 || tail_cap < 0 ||
        tail_cap > FA_RNNT_BIAS_MAX_FORM || (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) || !d_logits || !d_frames || !d_out_count || !d_final_u ||
        !d_eou || !d_status || (max_out > 0 && (!d_out_tok || !d_out_frame || !d_out_plain)) || (d_bias && (!d_tail || !d_tail_len || bias_words < 0)))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "rnnt: bad arguments (sizes >= 1, row_stride >= vocab_with_blank, 0 <= tail_cap <= %d, fp32 / fp16 logits, a tail with a bias)",
                             FA_RNNT_BIAS_MAX_FORM);
    fa::DeviceGuard guard(ctx->device);
    fa::rnnt::RnntArgs a;
    a.logits = d_logits; a.f16 = dtype == FA_DTYPE_F16 ? 1 : 0; a.B = batch; a.U = U; a.T = T; a.V1 = vocab_with_blank; a.max_out = max_out;
    a.row_stride = row_stride; a.frames = d_frames; a.skip = d_skip; a.bias = d_bias; a.bias_words = d_bias ? bias_words : 0; a.tail_cap = tail_cap;
    a.tail = d_tail; a.tail_len = d_tail_len; a.out_tok = d_out_tok; a.out_frame = d_out_frame; a.out_plain = d_out_plain; a.out_count = d_out_count;
    a.final_u = d_final_u; a.eou = d_eou; a.status = d_status; a.cfg = *cfg;
    fa::rnnt::launch_greedy(ctx->stream, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // extern "C"
