// tdt_launch.h — what the TDT decoder's host code (tdt_host.hip: the navigation helpers, the argument checks, the C ABI) and its kernel
// translation unit (tdt.hip) share: the operands of the walk, clamp_probability — the same function serves fa_tdt_clamp_probability on the
// host and every emitted token on the device —, the route of a logits call (tdt_route.h) and one launcher per kernel family.  Template
// arguments are named in tdt.hip only.  Internal; not part of the C ABI.  Launch errors surface through hipGetLastError().
// The language mode adds its operands (TdtLangArgs), the top-K entry its own (TdtTopkArgs), and a launcher each.
#pragma once
#include "fa_common.h"
#include "tdt_route.h"

namespace fa {
namespace tdt {

constexpr int kStandardOverlapFrames = 25;  // ASRConstants.standardOverlapFrames (Shared/ASRConstants.swift:49)

struct TdtArgs {
    const int32_t *tok, *bin;  // [B][U][T]
    const float *prob;         // [B][U][T]
    const int32_t *enc_len, *audio_frames, *t0, *is_last, *global_offset, *emit_after;  // [B]; emit_after < 0: emit all
    int32_t *out_tok, *out_time, *out_dur;  // [B][max_out]
    float *out_conf;                        // [B][max_out]
    int32_t *out_count, *final_time, *final_u, *status;  // [B]
    int32_t B, U, T, max_out;
    fa_tdt_config cfg;
};

// Joint LOGITS [B][U][T][row_stride]: token logits [0, V1), duration logits [V1, V1 + nd)
struct TdtLogitArgs {
    const void *logits;
    int32_t f16, V1, nd;
    int64_t row_stride;
};

// The language mode of the walk on logits (fa_tdt_greedy_logits_lang_dev): the filters of tdt_lang.h at the walk's decision site
struct TdtLangArgs {
    const uint8_t *classes;   // [V1] FA_TDT_CLASS_* bits
    int32_t script_bit;       // the FA_TDT_CLASS_*_OK bit of the target script
    int32_t use_blocklist, top_k;
    int32_t *out_route;       // [B][max_out]
    int32_t *swap_counts;     // [B][2]
};

// fa_tdt_topk_rows_dev: rows [R][row_stride] -> ids / logits [R][K], counts [R] (may be null)
struct TdtTopkArgs {
    const void *rows;
    int32_t f16, V1, K;
    int64_t R, row_stride;
    int32_t *ids;
    float *logits;
    int32_t *counts;
};

__host__ __device__ inline float clamp_probability(const float v) {  // TdtDurationMapping.swift:28-31
    if (!(v - v == 0.0f)) return 0.0f;  // NaN / +-inf
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

// tdt_kernel: a.B chunks on joint-decision tables, one thread per chunk
void launch_tables(hipStream_t stream, const TdtArgs &a);
// the walk on joint logits, one wavefront per chunk: the instance logits_route names for (g.f16, g.V1, g.row_stride, g.logits)
void launch_logits(hipStream_t stream, const TdtArgs &a, const TdtLogitArgs &g);
// the same instance with the language filters at its decision site
void launch_logits_lang(hipStream_t stream, const TdtArgs &a, const TdtLogitArgs &g, const TdtLangArgs &l);
// tdt_topk_kernel: one wavefront per row
void launch_topk(hipStream_t stream, const TdtTopkArgs &k);

}  // namespace tdt
}  // namespace fa
