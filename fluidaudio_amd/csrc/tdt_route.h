// tdt_route.h — which kernel serves a call of the TDT walk on joint logits, as plain C++ (no HIP types: tests/cpu/decoder_routes.cpp walks it
// on the CPU).  Part of tdt_launch.h.
#pragma once
#include <cstdint>

namespace fa {
namespace tdt {

// Rows of at most 17 x 64 logits stay in a wavefront's registers from the decision until the (rare) request for its probability
// (tdt_logits_fits_kernel: 17 requests per lane of one logit, 9 of a pair); longer rows stream through tdt_logits_kernel.
constexpr int kFitsPieces = 17;
constexpr int kFitsLogits = 64 * kFitsPieces;

enum Route : int { kStream = 0, kFits = 1, kFitsPairs = 2 };   // kFits: W = 1; kFitsPairs: W = 2, fp16 rows read as pairs

// fp16 rows that all start on a 4-byte boundary (an even row stride behind a 4-byte aligned pointer) are read as pairs
inline Route logits_route(const bool f16, const int32_t vocab_with_blank, const int64_t row_stride, const uintptr_t logits) {
    if (vocab_with_blank > kFitsLogits) return kStream;
    return f16 && (row_stride * 2) % 4 == 0 && logits % 4 == 0 ? kFitsPairs : kFits;
}

}  // namespace tdt
}  // namespace fa
