// rnnt_launch.h — what the host side of the streaming RNN-T walk (rnnt_host.hip: the argument checks, the C ABI) and its kernel unit
// (rnnt.hip) share: the operands of the walk, its launch plan and the launcher.  The bias tables themselves: rnnt_bias_core.h.
// Internal; not part of the C ABI.  Launch errors surface through hipGetLastError().
#pragma once
#include "fa_common.h"
#include "rnnt_bias_core.h"

namespace fa {
namespace rnnt {

constexpr int kWave = 64;
constexpr int kMaxTail = FA_RNNT_BIAS_MAX_FORM;          // the ring of tail scalars in LDS
constexpr int kTailPasses = kMaxTail / kWave;            // suffix starts per lane

struct RnntArgs {
    const void *logits;              // [B][U][T][row_stride]
    int32_t f16, B, U, T, V1, max_out;
    int64_t row_stride;
    const int32_t *frames, *skip;    // [B]; skip may be null (0)
    const int32_t *bias;             // the blob of fa_rnnt_bias_build on the device, or null (unbiased)
    int64_t bias_words;
    int32_t tail_cap;
    int32_t *tail, *tail_len;        // [B][tail_cap], [B]: the match state, in and out
    int32_t *out_tok, *out_frame, *out_plain;   // [B][max_out]
    int32_t *out_count, *final_u, *eou, *status;   // [B]
    fa_rnnt_config cfg;
};

// One wavefront per stream, one workgroup per wavefront; no row-length switch: every row is streamed in pieces of kWave logits.
struct Plan {
    unsigned grid, block;
};
inline Plan plan_of(const int32_t batch) { return Plan{static_cast<unsigned>(batch), static_cast<unsigned>(kWave)}; }

void launch_greedy(hipStream_t stream, const RnntArgs &a);

}  // namespace rnnt
}  // namespace fa
