// paraformer_host.hip — the host side of the Paraformer stages (kernels: paraformer.hip, shared operands: paraformer_launch.h): the
// argument pass, the uploads of the host-pointer entries, the workspace, the one synchronisation of a call and the C ABI.  No
// arithmetic of the reference lives here: what is decided here is decided from the arguments alone, before any device work.
#include <algorithm>

#include "paraformer_launch.h"

namespace {

namespace pf = fa::paraformer;

std::vector<int32_t> clamped(const int32_t *valid_frames, const int32_t batch, const int32_t frames) {
    std::vector<int32_t> v(static_cast<size_t>(batch), frames);
    if (valid_frames)
        for (int32_t b = 0; b < batch; ++b) v[b] = std::min(frames, std::max(0, valid_frames[b]));
    return v;
}

fa_status cif(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const void *enc, int32_t dtype, int32_t batch, int32_t frames, int32_t dim, int64_t row_stride,
              int64_t matrix_stride, const float *alphas, int64_t alpha_stride, const int32_t *valid_frames, float *ac, float *enc_packed, int32_t *token_counts,
              int32_t *fire_counts, int32_t *fire_frames, const bool device) {
    const fa_paraformer_cif_config c = pf::config_or_default(cfg);
    const pf::CifShape s{dtype, batch, frames, dim, row_stride, matrix_stride, alpha_stride};
    const fa::Verdict v = pf::check_cif(c, s, enc, alphas, ac, token_counts, fire_counts, fire_frames);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "paraformer_cif: %s", v.text);
    // a workgroup per (utterance, row, slice of 64 elements) at the narrowest load
    const int64_t rows = static_cast<int64_t>(batch) * std::max(c.max_tokens, enc_packed ? c.enc_frames : 0);
    if (rows * ((dim + pf::kWave - 1) / pf::kWave) > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "paraformer_cif: more than INT32_MAX workgroups");
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "paraformer_cif", [&]() -> fa_status {
    const std::vector<int32_t> valid = clamped(valid_frames, batch, frames);
    const size_t B = static_cast<size_t>(batch), per_utt = static_cast<size_t>(frames) + 1, esz = dtype == FA_DTYPE_F16 ? 2 : 4;
    const size_t enc_bytes = device ? 0 : esz * static_cast<size_t>(pf::enc_extent(s));
    const size_t alpha_bytes = (device || frames == 0) ? 0 : sizeof(float) * ((B - 1) * static_cast<size_t>(alpha_stride) + static_cast<size_t>(frames));
    const size_t ac_bytes = sizeof(float) * B * static_cast<size_t>(c.max_tokens) * static_cast<size_t>(dim);
    const size_t packed_bytes = enc_packed ? sizeof(float) * B * static_cast<size_t>(c.enc_frames) * static_cast<size_t>(dim) : 0;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_valid, b_w, b_seed, b_fires, b_counts, b_enc, b_alphas, b_ac, b_packed;
    FA_TRY(fa::take(ctx, "paraformer_cif", {{&b_valid, sizeof(int32_t) * B, true, valid.data()}, {&b_w, sizeof(float) * B * per_utt}, {&b_seed, sizeof(float) * B * per_utt},
                                            {&b_fires, sizeof(int32_t) * B * per_utt}, {&b_counts, sizeof(int32_t) * 2 * B}, {&b_enc, enc_bytes, !device, enc},
                                            {&b_alphas, alpha_bytes, !device, alphas}, {&b_ac, ac_bytes, !device}, {&b_packed, packed_bytes, !device && enc_packed}}));

    pf::CifArgs a{};
    a.enc = device ? enc : b_enc.p;
    a.batch = batch; a.frames = frames; a.dim = dim; a.row_stride = row_stride; a.matrix_stride = matrix_stride;
    a.alphas = device ? alphas : b_alphas.as<float>();
    a.alpha_stride = alpha_stride;
    a.valid = b_valid.as<int32_t>();
    a.threshold = c.threshold; a.tail = c.tail_threshold; a.max_tokens = c.max_tokens; a.enc_frames = c.enc_frames;
    a.w = b_w.as<float>(); a.seed = b_seed.as<float>(); a.fires = b_fires.as<int32_t>(); a.counts = b_counts.as<int32_t>();
    a.ac = device ? ac : b_ac.as<float>();
    a.enc_packed = !enc_packed ? nullptr : (device ? enc_packed : b_packed.as<float>());
    fa::DeviceTiming tim{ctx};
    FA_TRY(tim.begin());
    pf::launch_cif(st, a, pf::vector_width(s, a.enc, a.ac, a.enc_packed), dtype == FA_DTYPE_F16);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_TRY(tim.end());
    std::vector<int32_t> counts(2 * B);
    FA_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), b_counts.p, sizeof(int32_t) * 2 * B, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(fire_frames, b_fires.p, sizeof(int32_t) * B * per_utt, hipMemcpyDeviceToHost, st));
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(ac, b_ac.p, ac_bytes, hipMemcpyDeviceToHost, st));
        if (packed_bytes) FA_HIP_TRY(ctx, hipMemcpyAsync(enc_packed, b_packed.p, packed_bytes, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    FA_TRY(tim.read());
    std::copy(counts.begin(), counts.begin() + batch, token_counts);
    std::copy(counts.begin() + batch, counts.end(), fire_counts);
    return FA_SUCCESS;
    });
}

fa_status timestamps(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const float *alphas, int64_t alpha_stride, int32_t batch, int32_t frames,
                     const int32_t *valid_frames, const int32_t *token_ids, const int32_t *token_counts, const uint8_t *keep, int32_t vocab, const float *audio,
                     const int64_t *audio_offsets, fa_paraformer_span *spans, int64_t capacity, int64_t *count, int64_t *utterance_counts, const bool device) {
    const fa_paraformer_cif_config c = pf::config_or_default(cfg);
    const pf::StampShape s{batch, frames, vocab, alpha_stride};
    const fa::Verdict v = pf::check_stamps(c, s, alphas, token_ids, token_counts, keep, audio, audio_offsets, capacity, count);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "paraformer_timestamps: %s", v.text);
    int64_t max_env = 0;
    for (int32_t b = 0; b < batch; ++b) max_env = std::max(max_env, pf::env_frames(audio_offsets[b + 1] - audio_offsets[b]));
    const int64_t env_blocks = (max_env + pf::kEnvBlock - 1) / pf::kEnvBlock;
    if (env_blocks * batch > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "paraformer_timestamps: more than INT32_MAX workgroups");
    if (!ctx) return FA_INVALID_ARGUMENT;
    *count = 0;
    if (utterance_counts) std::fill(utterance_counts, utterance_counts + batch, int64_t{0});
    if (batch == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "paraformer_timestamps", [&]() -> fa_status {
    const std::vector<int32_t> valid = clamped(valid_frames, batch, frames);
    const size_t B = static_cast<size_t>(batch), mt = static_cast<size_t>(c.max_tokens);
    // the host-pointer entry uploads the audio from the first sample used on
    const int64_t a0 = device ? 0 : audio_offsets[0];
    std::vector<int64_t> audio_off(B + 1), env_off(B + 1, 0);
    for (size_t b = 0; b <= B; ++b) audio_off[b] = audio_offsets[b] - a0;
    for (size_t b = 0; b < B; ++b) env_off[b + 1] = env_off[b] + pf::env_frames(audio_off[b + 1] - audio_off[b]);
    const size_t n_env = static_cast<size_t>(env_off[B]), n_fires = B * (static_cast<size_t>(pf::kUpsample) * frames + 1);
    const size_t audio_bytes = device ? 0 : sizeof(float) * static_cast<size_t>(audio_off[B]);
    const size_t alpha_bytes = (device || frames == 0) ? 0 : sizeof(float) * ((B - 1) * static_cast<size_t>(alpha_stride) + static_cast<size_t>(frames));
    const size_t ids_bytes = (device || !token_ids) ? 0 : sizeof(int32_t) * B * mt;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_valid, b_tc, b_keep, b_aoff, b_eoff, b_raw, b_env, b_thr, b_kept, b_fires, b_spacing, b_spans, b_counts, b_audio, b_alphas, b_ids;
    FA_TRY(fa::take(ctx, "paraformer_timestamps",
                    {{&b_valid, sizeof(int32_t) * B, true, valid.data()}, {&b_tc, sizeof(int32_t) * B, true, token_counts}, {&b_keep, static_cast<size_t>(vocab), true, keep},
                     {&b_aoff, sizeof(int64_t) * (B + 1), true, audio_off.data()}, {&b_eoff, sizeof(int64_t) * (B + 1), true, env_off.data()}, {&b_raw, sizeof(float) * n_env},
                     {&b_env, sizeof(float) * n_env}, {&b_thr, sizeof(float) * B}, {&b_kept, sizeof(int32_t) * B * mt}, {&b_fires, sizeof(int32_t) * n_fires},
                     {&b_spacing, sizeof(float) * B * mt}, {&b_spans, sizeof(pf::Span) * B * mt}, {&b_counts, sizeof(int32_t) * B}, {&b_audio, audio_bytes, !device, audio + a0},
                     {&b_alphas, alpha_bytes, !device, alphas}, {&b_ids, ids_bytes, !device, token_ids}}));

    pf::StampArgs a{};
    a.alphas = device ? alphas : b_alphas.as<float>();
    a.alpha_stride = alpha_stride;
    a.valid = b_valid.as<int32_t>();
    a.batch = batch; a.frames = frames; a.vocab = vocab; a.max_tokens = c.max_tokens; a.tail = c.tail_threshold;
    a.token_ids = device ? token_ids : b_ids.as<int32_t>();
    a.token_counts = b_tc.as<int32_t>();
    a.keep = b_keep.as<uint8_t>();
    a.audio = device ? audio : b_audio.as<float>();
    a.audio_off = b_aoff.as<int64_t>(); a.env_off = b_eoff.as<int64_t>();
    a.env_blocks = static_cast<int32_t>(env_blocks);
    a.env_raw = b_raw.as<float>(); a.env = b_env.as<float>(); a.threshold = b_thr.as<float>();
    a.kept = b_kept.as<int32_t>(); a.fires = b_fires.as<int32_t>(); a.spacing = b_spacing.as<float>();
    a.spans = b_spans.as<pf::Span>(); a.span_counts = b_counts.as<int32_t>();
    fa::DeviceTiming tim{ctx};
    FA_TRY(tim.begin());
    pf::launch_stamps(st, a);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_TRY(tim.end());
    std::vector<int32_t> counts(B);
    std::vector<pf::Span> got(B * mt);
    FA_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), b_counts.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_spans.p, sizeof(pf::Span) * B * mt, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    FA_TRY(tim.read());
    int64_t total = 0;
    for (size_t b = 0; b < B; ++b) {
        if (counts[b] < 0 || static_cast<size_t>(counts[b]) > mt) return fa::set_error(ctx, FA_RUNTIME_ERROR, "paraformer_timestamps: utterance %zu reports %d spans", b, counts[b]);
        if (utterance_counts) utterance_counts[b] = counts[b];
        for (int32_t i = 0; i < counts[b]; ++i, ++total) {
            const pf::Span &r = got[b * mt + static_cast<size_t>(i)];
            if (spans && total < capacity) spans[total] = fa_paraformer_span{static_cast<int32_t>(b), r.token, r.start, r.end};
        }
    }
    *count = total;
    if (spans && capacity < total) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "paraformer_timestamps: output holds %lld of %lld spans", (long long)capacity, (long long)total);
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_paraformer_cif_default_config(fa_paraformer_cif_config *cfg) {
    if (cfg) *cfg = pf::config_or_default(nullptr);
}

fa_status fa_paraformer_cif_dev(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const void *d_enc, int32_t dtype, int32_t batch, int32_t frames, int32_t dim,
                                int64_t row_stride, int64_t matrix_stride, const float *d_alphas, int64_t alpha_stride, const int32_t *valid_frames, float *d_ac,
                                float *d_enc_packed, int32_t *token_counts, int32_t *fire_counts, int32_t *fire_frames) {
    return cif(ctx, cfg, d_enc, dtype, batch, frames, dim, row_stride, matrix_stride, d_alphas, alpha_stride, valid_frames, d_ac, d_enc_packed, token_counts, fire_counts,
               fire_frames, true);
}

fa_status fa_paraformer_cif(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const void *enc, int32_t dtype, int32_t batch, int32_t frames, int32_t dim, int64_t row_stride,
                            int64_t matrix_stride, const float *alphas, int64_t alpha_stride, const int32_t *valid_frames, float *ac, float *enc_packed,
                            int32_t *token_counts, int32_t *fire_counts, int32_t *fire_frames) {
    return cif(ctx, cfg, enc, dtype, batch, frames, dim, row_stride, matrix_stride, alphas, alpha_stride, valid_frames, ac, enc_packed, token_counts, fire_counts, fire_frames,
               false);
}

fa_status fa_paraformer_timestamps_dev(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const float *d_alphas, int64_t alpha_stride, int32_t batch, int32_t frames,
                                       const int32_t *valid_frames, const int32_t *d_token_ids, const int32_t *token_counts, const uint8_t *keep, int32_t vocab,
                                       const float *d_audio, const int64_t *audio_offsets, fa_paraformer_span *spans, int64_t capacity, int64_t *count,
                                       int64_t *utterance_counts) {
    return timestamps(ctx, cfg, d_alphas, alpha_stride, batch, frames, valid_frames, d_token_ids, token_counts, keep, vocab, d_audio, audio_offsets, spans, capacity, count,
                      utterance_counts, true);
}

fa_status fa_paraformer_timestamps(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const float *alphas, int64_t alpha_stride, int32_t batch, int32_t frames,
                                   const int32_t *valid_frames, const int32_t *token_ids, const int32_t *token_counts, const uint8_t *keep, int32_t vocab, const float *audio,
                                   const int64_t *audio_offsets, fa_paraformer_span *spans, int64_t capacity, int64_t *count, int64_t *utterance_counts) {
    return timestamps(ctx, cfg, alphas, alpha_stride, batch, frames, valid_frames, token_ids, token_counts, keep, vocab, audio, audio_offsets, spans, capacity, count,
                      utterance_counts, false);
}

}  // extern "C"
