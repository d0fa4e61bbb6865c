// aed_launch.h — the host plan of the AED unit (kernels: aed.hip, entries: aed_host.hip, shared integers: aed_core.h): the argument
// passes, the kernels' operands and their launch plans.  Plain C++ without a HIP call, shared with tests/cpu/aed_core_main.cpp.
// Internal; not part of the C ABI.
#pragma once
#include <cstdint>

#include "../../include/fluidaudio_hip.h"
#include "aed_core.h"
#include "fa_verdict.h"

namespace fa {
namespace aed {

constexpr int kWave = 64;
constexpr int kStepThreads = 256;   // one workgroup per utterance
constexpr int kTile = 32;           // the LDS tile of the context transpose
constexpr int kTileThreads = 256;

inline fa_aed_config default_config(const int32_t model) {
    fa_aed_config c{};
    c.vocab = 16384; c.eos_id = 3; c.window_tokens = 32; c.min_match = 4;
    if (model == FA_AED_MODEL_CANARY) {   // CanaryConfig: maxDecoderSteps 128, 15 s windows with a 3 s overlap, the plain argmax
        c.mode = FA_AED_FEED_SEQUENCE; c.max_seq = 128; c.max_new = 128; c.no_repeat_ngram = 0; c.repetition_penalty = 1.0f;
        c.chunk_samples = 240000; c.hop_samples = 192000;
    } else {                              // CohereAsrConfig: maxSeqLen 108, 35 s windows with a 5 s overlap; transcribe's defaults
        c.mode = FA_AED_FEED_TOKEN; c.max_seq = 108; c.max_new = 108; c.no_repeat_ngram = 3; c.repetition_penalty = 1.1f;
        c.chunk_samples = 560000; c.hop_samples = 480000;
    }
    return c;
}

// ---- the argument passes: nothing is written, no device is touched
inline Verdict check_decode_config(const fa_aed_config *c) {
    if (!c) return refuse(FA_INVALID_ARGUMENT, "a config is required");
    if (c->mode != FA_AED_FEED_TOKEN && c->mode != FA_AED_FEED_SEQUENCE) return refuse(FA_INVALID_ARGUMENT, "mode is neither the token nor the sequence feed");
    if (c->vocab < 1 || c->vocab > FA_AED_MAX_VOCAB) return refuse(FA_INVALID_ARGUMENT, "vocab must be 1 ... %d", static_cast<int>(FA_AED_MAX_VOCAB));
    if (c->max_seq < 1 || c->max_seq > FA_AED_MAX_SEQ) return refuse(FA_INVALID_ARGUMENT, "max_seq must be 1 ... %d", static_cast<int>(FA_AED_MAX_SEQ));
    if (c->max_new < 0) return refuse(FA_INVALID_ARGUMENT, "max_new is negative");
    if (!(c->repetition_penalty == c->repetition_penalty)) return refuse(FA_INVALID_ARGUMENT, "the repetition penalty is NaN");
    return Verdict{};
}
inline bool mask_dtype_ok(const int32_t d) { return d == FA_DTYPE_F32 || d == FA_DTYPE_F16; }

// the arrays a feed writes: token feed input_id + position_id (self mask optional), sequence feed input_ids + decoder_mask
inline Verdict check_feed_arrays(const fa_aed_config &c, const void *input_id, const void *position_id, const void *self_mask, const int32_t mask_dtype,
                                 const void *input_ids, const void *decoder_mask) {
    if (c.mode == FA_AED_FEED_TOKEN) {
        if (!input_id || !position_id) return refuse(FA_INVALID_ARGUMENT, "the token feed writes d_input_id and d_position_id");
        if (self_mask && !mask_dtype_ok(mask_dtype)) return refuse(FA_INVALID_ARGUMENT, "the mask is fp32 or fp16");
    } else if (!input_ids || !decoder_mask) {
        return refuse(FA_INVALID_ARGUMENT, "the sequence feed writes d_input_ids and d_decoder_mask");
    }
    return Verdict{};
}

inline Verdict check_begin(const fa_aed_config *c, const int32_t batch, const void *prompts, const int32_t prompt_stride, const int32_t *prompt_lens,
                           const void *state, const void *input_id, const void *position_id, const void *self_mask, const int32_t mask_dtype,
                           const void *input_ids, const void *decoder_mask) {
    const Verdict v = check_decode_config(c);
    if (v.status != FA_SUCCESS) return v;
    if (batch < 1 || prompt_stride < 1 || !prompts || !prompt_lens || !state) return refuse(FA_INVALID_ARGUMENT, "batch and prompt_stride >= 1; prompts, prompt_lens and the state are required");
    const Verdict f = check_feed_arrays(*c, input_id, position_id, self_mask, mask_dtype, input_ids, decoder_mask);
    if (f.status != FA_SUCCESS) return f;
    for (int32_t b = 0; b < batch; ++b)
        if (prompt_lens[b] < 1 || prompt_lens[b] > prompt_stride || prompt_lens[b] > c->max_seq)
            return refuse(FA_INVALID_ARGUMENT, "utterance %d has a prompt of %d tokens (1 ... min(prompt_stride, max_seq))", static_cast<int>(b), static_cast<int>(prompt_lens[b]));
    return Verdict{};
}

inline Verdict check_step(const fa_aed_config *c, const int32_t batch, const void *state, const void *logits, const int32_t dtype, const int64_t row_stride,
                          const void *input_id, const void *position_id, const void *self_mask, const int32_t mask_dtype, const void *input_ids,
                          const void *decoder_mask) {
    const Verdict v = check_decode_config(c);
    if (v.status != FA_SUCCESS) return v;
    if (batch < 1 || !state || !logits) return refuse(FA_INVALID_ARGUMENT, "batch >= 1; the state and the logits are required");
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) return refuse(FA_INVALID_ARGUMENT, "the logits are fp32 or fp16");
    if (row_stride < c->vocab) return refuse(FA_INVALID_ARGUMENT, "row_stride is below vocab");
    return check_feed_arrays(*c, input_id, position_id, self_mask, mask_dtype, input_ids, decoder_mask);
}

inline Verdict check_finish(const fa_aed_config *c, const int32_t batch, const void *state, const int32_t max_out, const void *tokens, const void *counts) {
    const Verdict v = check_decode_config(c);
    if (v.status != FA_SUCCESS) return v;
    if (batch < 1 || !state || !tokens || !counts) return refuse(FA_INVALID_ARGUMENT, "batch >= 1; the state, tokens and counts are required");
    if (max_out < max_out_of(*c)) return refuse(FA_OUTPUT_TOO_SMALL, "max_out %d is below the %d tokens an utterance can emit", static_cast<int>(max_out), static_cast<int>(max_out_of(*c)));
    return Verdict{};
}

inline Verdict check_strided(const int32_t batch, const int32_t rows, const int32_t cols, const int64_t sb, const int64_t sr, const int64_t sc, const int32_t dtype) {
    if (batch < 1 || rows < 1 || cols < 1) return refuse(FA_INVALID_ARGUMENT, "the sizes are >= 1");
    if (sb < 0 || sr < 0 || sc < 0) return refuse(FA_INVALID_ARGUMENT, "a stride is negative");
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) return refuse(FA_INVALID_ARGUMENT, "the input is fp32 or fp16");
    return Verdict{};
}

// ---- the window plan for a batch of recordings
inline Verdict check_windows(const fa_aed_config *c, const int64_t *samples, const int64_t n, const int64_t *window_range, const int64_t *starts, const int64_t *lens,
                             const int64_t capacity, const int64_t *count) {
    if (!c || !count) return refuse(FA_INVALID_ARGUMENT, "a config and count are required");
    if (c->chunk_samples < 1 || c->hop_samples < 1 || c->hop_samples > c->chunk_samples) return refuse(FA_INVALID_ARGUMENT, "1 <= hop_samples <= chunk_samples");
    if (n < 0 || capacity < 0) return refuse(FA_INVALID_ARGUMENT, "a negative size");
    if (n > 0 && (!samples || !window_range)) return refuse(FA_INVALID_ARGUMENT, "samples and window_range are required");
    if ((starts == nullptr) != (lens == nullptr)) return refuse(FA_INVALID_ARGUMENT, "starts and lens come together");
    for (int64_t r = 0; r < n; ++r)
        if (samples[r] < 0) return refuse(FA_INVALID_ARGUMENT, "recording %lld has a negative length", static_cast<long long>(r));
    return Verdict{};
}
// window_range and the total; INDEX_OVERFLOW past int64
inline Verdict count_windows(const fa_aed_config &c, const int64_t *samples, const int64_t n, int64_t *window_range, int64_t *count) {
    int64_t total = 0;
    if (n > 0) window_range[0] = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t w = window_count(samples[r], c.chunk_samples, c.hop_samples);
        if (w > INT64_MAX - total) return refuse(FA_INDEX_OVERFLOW, "the windows are beyond int64");
        total += w;
        window_range[r + 1] = total;
    }
    *count = total;
    return Verdict{};
}

// ---- the seam merge
struct MergeRec {
    int64_t w_lo, w_hi;      // its windows
    int64_t out_off;         // its output slice, counted from the call's first output token
};
struct MergeArgs {
    const int32_t *tokens;   // the call's first token
    const int64_t *win_off;  // [windows + 1], counted from the call's first token
    const MergeRec *recs;
    int32_t n_recs;
    int32_t window_tokens, min_match;
    int32_t *out;
    int32_t *counts;         // [n_recs]
    int32_t *best_len, *best_send;   // [windows]
};
inline Verdict check_merge(const fa_aed_config *c, const void *tokens, const int64_t *window_offsets, const int64_t *recording_range, const int64_t n, const void *out,
                           const int64_t *out_range, const void *out_counts) {
    const int32_t wt = c ? c->window_tokens : 32;
    if (wt < 1 || wt > FA_AED_MAX_WINDOW_TOKENS) return refuse(FA_INVALID_ARGUMENT, "window_tokens must be 1 ... %d", static_cast<int>(FA_AED_MAX_WINDOW_TOKENS));
    if (n < 0) return refuse(FA_INVALID_ARGUMENT, "a negative size");
    if (n == 0) return Verdict{};
    if (n >= INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "2^31 - 1 recordings or more");
    if (!window_offsets || !recording_range || !out_range || !out_counts) return refuse(FA_INVALID_ARGUMENT, "the offsets, ranges and out_counts are required");
    if (recording_range[0] < 0 || out_range[0] < 0) return refuse(FA_INVALID_ARGUMENT, "a range starts below 0");
    for (int64_t r = 0; r < n; ++r)
        if (recording_range[r + 1] < recording_range[r] || out_range[r + 1] < out_range[r]) return refuse(FA_INVALID_ARGUMENT, "the ranges do not ascend");
    if (window_offsets[recording_range[0]] < 0) return refuse(FA_INVALID_ARGUMENT, "the window offsets start below 0");
    for (int64_t w = recording_range[0]; w < recording_range[n]; ++w)
        if (window_offsets[w + 1] < window_offsets[w]) return refuse(FA_INVALID_ARGUMENT, "the window offsets do not ascend");
    for (int64_t r = 0; r < n; ++r) {
        const int64_t need = window_offsets[recording_range[r + 1]] - window_offsets[recording_range[r]], room = out_range[r + 1] - out_range[r];
        if (need > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "recording %lld holds more than INT32_MAX tokens", static_cast<long long>(r));
        if (room < need) return refuse(FA_OUTPUT_TOO_SMALL, "recording %lld has %lld tokens, its output slice holds %lld", static_cast<long long>(r), static_cast<long long>(need), static_cast<long long>(room));
    }
    const int64_t total = window_offsets[recording_range[n]] - window_offsets[recording_range[0]];
    if (total > 0 && (!tokens || !out)) return refuse(FA_INVALID_ARGUMENT, "tokens and out are required");
    return Verdict{};
}

// ---- launch plans
struct StepPlan {
    unsigned grid, block;
    unsigned lds_bytes;      // the history and the banned tokens by position (each max_seq rounded up to 4 words), then the V-bit map; 0 when no id of the row can change
    int32_t marked;          // the row has penalised / banned ids: the bit map is built
};
inline StepPlan step_plan(const fa_aed_config &c, const int32_t batch) {
    StepPlan p{static_cast<unsigned>(batch), static_cast<unsigned>(kStepThreads), 0u, 0};
    p.marked = (c.mode == FA_AED_FEED_TOKEN && (c.repetition_penalty != 1.0f || c.no_repeat_ngram > 0)) ? 1 : 0;
    if (p.marked) p.lds_bytes = 8u * static_cast<unsigned>((c.max_seq + 3) & ~3) + 4u * static_cast<unsigned>((c.vocab + 31) / 32);
    return p;
}
struct TilePlan {
    unsigned gx, gy, gz, block;
};
inline TilePlan tile_plan(const int32_t batch, const int32_t D, const int32_t T) {
    return TilePlan{static_cast<unsigned>((T + kTile - 1) / kTile), static_cast<unsigned>((D + kTile - 1) / kTile), static_cast<unsigned>(batch), static_cast<unsigned>(kTileThreads)};
}

struct StepArgs {
    fa_aed_config cfg;
    Layout lay;
    int32_t *state;
    const void *logits;
    int32_t f16, marked;
    int64_t row_stride;
    int32_t *input_id, *position_id;
    void *self_mask;
    int32_t mask_f16;
    int32_t *input_ids;
    float *decoder_mask;
};
struct BeginArgs {
    fa_aed_config cfg;
    Layout lay;
    int32_t *state;
    const int32_t *prompts, *prompt_lens;
    int32_t prompt_stride;
    int32_t *input_id, *position_id;
    void *self_mask;
    int32_t mask_f16;
    int32_t *input_ids;
    float *decoder_mask;
};
struct FinishArgs {
    Layout lay;
    const int32_t *state;
    int32_t batch, max_out;
    int32_t *tokens, *counts, *reasons, *steps;
};
struct StridedArgs {      // [batch][rows][cols] at element strides; context: rows = D, cols = T; gather: rows = S, cols = D
    const void *src;
    int32_t f16, batch, rows, cols;
    int64_t sb, sr, sc;
};

}  // namespace aed
}  // namespace fa
