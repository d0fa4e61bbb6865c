// paraformer_launch.h — what the host side of the Paraformer stages (paraformer_host.hip: the C ABI, uploads, the one synchronisation
// of a call) and their kernels (paraformer.hip) share: the argument pass of both stages (plain C++: decided from the arguments alone,
// nothing is written), the vector width of the row loads, the layout of the workspace, the kernels' operands and their launchers.
// Internal; not part of the C ABI.
//
// CIF (ParaformerCif.swift:19-50).  The alpha chain of an utterance is serial — fp32 adds do not reassociate — but short (T + 1 steps),
// and it alone decides which rows go into which token with which weight.  So cif_scan walks it once per utterance (one wavefront) and
// leaves, per frame t = 0 ... T, the weight of row t in the token that is open at t (alpha, or `used` when t fires) and the weight of
// row t in the seed of the next token (alpha - used), and per token its fire frame.  Token l is then
//     frame = h[f(l-1)] * seed[f(l-1)]          (l > 0; zeros for l == 0)
//     frame += w[t] * h[t]                      for t = f(l-1) + 1 ... f(l), ascending
// which cif_gather evaluates with one accumulator per element: one wavefront per (utterance, token, slice of 64 V elements).
#pragma once
#include <algorithm>

#include "fa_common.h"
#include "fa_verdict.h"

namespace fa {
namespace paraformer {

constexpr int kWave = 64;
constexpr int kHop = 160;            // Int(0.01 * 16000): samples of one envelope frame
constexpr int kEnvBlock = 256;       // envelope frames of one workgroup
constexpr int kEnvChunk = 32;        // samples of every frame staged through LDS at a time (kHop is a multiple)
constexpr int kUpsample = 3;
constexpr int kMinRun = 3;
static_assert(kHop % kEnvChunk == 0, "the envelope kernel stages whole chunks");

inline fa_paraformer_cif_config config_or_default(const fa_paraformer_cif_config *cfg) {
    return cfg ? *cfg : fa_paraformer_cif_config{1.0f, 0.45f, 128, 512};   // ParaformerConfig.swift:19-20, 28-29
}

// ---- CIF
struct CifShape {
    int32_t dtype, batch, frames, dim;
    int64_t row_stride, matrix_stride, alpha_stride;
};

// elements of the encoder array up to the last one read
inline int64_t enc_extent(const CifShape &s) {
    return (s.batch < 1 || s.frames < 1) ? 0 : static_cast<int64_t>(s.batch - 1) * s.matrix_stride + static_cast<int64_t>(s.frames - 1) * s.row_stride + s.dim;
}

inline Verdict check_cif(const fa_paraformer_cif_config &c, const CifShape &s, const void *enc, const void *alphas, const void *ac, const void *token_counts,
                         const void *fire_counts, const void *fire_frames) {
    if (s.batch < 0 || s.frames < 0 || s.dim < 1 || s.row_stride < s.dim || s.alpha_stride < s.frames) return refuse(FA_INVALID_ARGUMENT, "bad shape");
    if (s.dtype != FA_DTYPE_F32 && s.dtype != FA_DTYPE_F16) return refuse(FA_INVALID_ARGUMENT, "dtype is FA_DTYPE_F32 or FA_DTYPE_F16");
    if (c.max_tokens < 1 || c.enc_frames < 0) return refuse(FA_INVALID_ARGUMENT, "bad config");
    if (s.batch > 1 && s.frames > 0 && s.matrix_stride < static_cast<int64_t>(s.frames - 1) * s.row_stride + s.dim) return refuse(FA_INVALID_ARGUMENT, "matrices overlap");
    if (s.batch > 0 && (!ac || !token_counts || !fire_counts || !fire_frames)) return refuse(FA_INVALID_ARGUMENT, "an output is NULL");
    if (s.batch > 0 && s.frames > 0 && (!enc || !alphas)) return refuse(FA_INVALID_ARGUMENT, "an input is NULL");
    const int64_t b = s.batch;
    if (b * (static_cast<int64_t>(s.frames) + 1) > INT32_MAX || b * c.max_tokens > INT32_MAX || b * std::max(c.enc_frames, 1) > INT32_MAX)
        return refuse(FA_INDEX_OVERFLOW, "more than INT32_MAX frames or tokens in the batch");
    return Verdict{};
}

// Elements a lane loads at once (16 bytes: 4 floats or 8 halves), as far as the dimension, both strides and the three addresses allow;
// a narrower width otherwise.  The store to ac / enc_packed ([..., dim] contiguous fp32) is 16 bytes per 4 elements.
inline int vector_width(const CifShape &s, const void *enc, const void *ac, const void *enc_packed) {
    const size_t esz = s.dtype == FA_DTYPE_F16 ? 2 : 4;
    const auto fits = [&](const int v) {
        return s.dim % v == 0 && s.row_stride % v == 0 && s.matrix_stride % v == 0 && reinterpret_cast<uintptr_t>(enc) % (esz * v) == 0 &&
               reinterpret_cast<uintptr_t>(ac) % 16 == 0 && reinterpret_cast<uintptr_t>(enc_packed) % 16 == 0;
    };
    if (s.dtype == FA_DTYPE_F16 && fits(8)) return 8;
    return fits(4) ? 4 : 1;
}

struct CifArgs {
    const void *enc;                 // matrix b at b * matrix_stride, row t at t * row_stride, dim elements read
    int32_t batch, frames, dim;
    int64_t row_stride, matrix_stride;
    const float *alphas;             // [batch][alpha_stride]
    int64_t alpha_stride;
    const int32_t *valid;            // [batch], in [0, frames]
    float threshold, tail;
    int32_t max_tokens, enc_frames;
    // the workspace, [batch][frames + 1] each: cif_scan writes entries 0 ... valid[b] of w and seed and every entry of fires
    float *w, *seed;
    int32_t *fires;                  // the fire frames, -1 behind the last one
    int32_t *counts;                 // [2][batch]: min(L, max_tokens), then L
    float *ac;                       // [batch][max_tokens][dim]
    float *enc_packed;               // [batch][enc_frames][dim] or nullptr
};

// cif_scan, cif_gather and (with enc_packed) cif_pack, in stream order; width from vector_width, fp16 from FA_DTYPE_F16
void launch_cif(hipStream_t stream, const CifArgs &a, int width, bool fp16);

// ---- timestamps
struct StampShape {
    int32_t batch, frames, vocab;
    int64_t alpha_stride;
};

inline Verdict check_stamps(const fa_paraformer_cif_config &c, const StampShape &s, const void *alphas, const void *token_ids, const int32_t *token_counts,
                            const void *keep, const void *audio, const int64_t *audio_offsets, const int64_t capacity, const void *count) {
    if (s.batch < 0 || s.frames < 0 || s.vocab < 0 || s.alpha_stride < s.frames || capacity < 0 || !count) return refuse(FA_INVALID_ARGUMENT, "bad shape, or count is NULL");
    if (c.max_tokens < 1) return refuse(FA_INVALID_ARGUMENT, "bad config");
    if (s.batch > 0 && (!token_counts || !audio_offsets || (s.vocab > 0 && !keep) || (s.frames > 0 && !alphas))) return refuse(FA_INVALID_ARGUMENT, "an input is NULL");
    if (s.batch > 0 && audio_offsets[0] < 0) return refuse(FA_INVALID_ARGUMENT, "audio_offsets starts below 0");
    bool tokens = false;
    for (int32_t b = 0; b < s.batch; ++b) {
        if (token_counts[b] < 0 || token_counts[b] > c.max_tokens) return refuse(FA_INVALID_ARGUMENT, "a token count outside [0, max_tokens]");
        if (audio_offsets[b + 1] < audio_offsets[b]) return refuse(FA_INVALID_ARGUMENT, "audio_offsets does not ascend");
        if (audio_offsets[b + 1] - audio_offsets[b] > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "an utterance of more than INT32_MAX samples");
        tokens = tokens || token_counts[b] > 0;
    }
    if (tokens && !token_ids) return refuse(FA_INVALID_ARGUMENT, "token_ids is NULL");
    if (s.batch > 0 && audio_offsets[s.batch] > audio_offsets[0] && !audio) return refuse(FA_INVALID_ARGUMENT, "audio is NULL");
    const int64_t b = s.batch;
    if (b * (static_cast<int64_t>(kUpsample) * s.frames + 1) > INT32_MAX || b * c.max_tokens > INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "more than INT32_MAX frames or tokens in the batch");
    return Verdict{};
}

// envelope frames of an utterance of n samples (energyEnvelope, ParaformerManager.swift:277-293: none unless n > hop)
constexpr int64_t env_frames(const int64_t n) { return n > kHop ? n / kHop : 0; }

struct Span {                        // a record of the device arena, slot [b][i]
    int32_t token;                   // position in the utterance's token_ids
    int32_t pad;
    double start, end;
};

struct StampArgs {
    const float *alphas;             // [batch][alpha_stride]
    int64_t alpha_stride;
    const int32_t *valid;            // [batch], in [0, frames]
    int32_t batch, frames, vocab, max_tokens;
    float tail;
    const int32_t *token_ids;        // [batch][max_tokens]
    const int32_t *token_counts;     // [batch]
    const uint8_t *keep;             // [vocab]
    const float *audio;              // utterance b's samples at audio_off[b] ... audio_off[b + 1]
    const int64_t *audio_off;        // [batch + 1], from the array the kernel is given
    const int64_t *env_off;          // [batch + 1]: utterance b's envelope frames in env_raw / env
    int32_t env_blocks;              // workgroups of kEnvBlock frames that cover the longest envelope of the batch
    // the workspace: pf_envelope writes env_raw, pf_smooth env, pf_floor threshold; pf_walk writes what it reads of the rest
    float *env_raw, *env;
    float *threshold;                // [batch]
    int32_t *kept;                   // [batch][max_tokens] positions of the kept tokens
    int32_t *fires;                  // [batch][3 frames + 1]
    float *spacing;                  // [batch][max_tokens]
    Span *spans;                     // [batch][max_tokens]
    int32_t *span_counts;            // [batch]
};

void launch_stamps(hipStream_t stream, const StampArgs &a);

}  // namespace paraformer
}  // namespace fa
