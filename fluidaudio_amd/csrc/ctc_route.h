// ctc_route.h — the decisions of the CTC decoder's host side that need no device, as plain C++ (no HIP types: tests/cpu/decoder_routes.cpp
// walks them on the CPU): the launch geometry, which kernel instance serves a greedy call and a log-softmax call, and the contract of the
// rows entries.  Part of ctc_launch.h.
#pragma once
#include <cstdint>

namespace fa {
namespace ctc {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLsmRegs = 32;  // log-softmax: values per lane held in registers: V <= 2048 single pass

// ctc_greedy_kernel<F16, MODE>.  0: rows are 16-byte aligned and hold whole vectors (16-byte loads only); 1: the matrices are aligned to their
// element type and a row holds two vectors or more — at least one whole 16-byte piece behind any head —, so rows of any alignment are a head,
// a 16-byte body and a tail; 2: 4- / 2-byte loads (misaligned matrices, rows shorter than two vectors).
inline int greedy_mode(const bool f16, const int32_t vocab, const int64_t row_stride, const int64_t matrix_stride, const uintptr_t logits) {
    const int vw = f16 ? 8 : 4;   // elements of a 16-byte vector
    if (vocab % vw == 0 && row_stride % vw == 0 && matrix_stride % vw == 0 && logits % 16 == 0) return 0;
    return logits % (f16 ? 2 : 4) == 0 && vocab >= 2 * vw ? 1 : 2;
}

// ctc_log_softmax_vec4_kernel: fp32 rows that are 16-byte aligned on both sides (the output rows are `vocab` floats apart), whole float4 groups, one pass
inline bool log_softmax_vec4(const bool f16, const int32_t vocab, const int64_t row_stride, const int64_t matrix_stride, const uintptr_t logits,
                             const uintptr_t log_probs) {
    return !f16 && vocab % 4 == 0 && vocab <= 64 * kLsmRegs && row_stride % 4 == 0 && matrix_stride % 4 == 0 && logits % 16 == 0 && log_probs % 16 == 0;
}

// The contract of fa_ctc_greedy_rows and fa_ctc_greedy_rows_dev, wherever the arrays live: last_error's text, or nullptr for a well-formed
// call (batch == 0 is one, and needs nothing else).
inline const char *rows_call_error(const int32_t batch, const int64_t total_rows, const bool utt_rows, const bool row_offsets, const bool token_ids) {
    if (batch < 0 || total_rows < 0) return "ctc rows: bad shape";
    if (batch == 0) return nullptr;
    if (!utt_rows && batch != 1) return "ctc rows: a batch needs utt_rows";
    if (total_rows > 0 && (!row_offsets || !token_ids)) return "ctc rows: null buffer";
    return nullptr;
}

// What the host-pointer entry adds, for a call that passed rows_call_error with batch > 0: a walk over the caller's offsets — a decreasing
// pair would make the kernel read outside `values`.
inline const char *rows_offsets_error(const int64_t *row_offsets, const int64_t total_rows, const int64_t *utt_rows, const int32_t batch) {
    if (total_rows > 0) {
        if (row_offsets[0] < 0) return "ctc rows: negative offset";
        for (int64_t r = 0; r < total_rows; ++r)
            if (row_offsets[r + 1] < row_offsets[r]) return "ctc rows: row_offsets decrease";
    }
    if (utt_rows) {
        if (utt_rows[0] < 0 || utt_rows[batch] > total_rows) return "ctc rows: utt_rows out of range";
        for (int32_t u = 0; u < batch; ++u)
            if (utt_rows[u + 1] < utt_rows[u]) return "ctc rows: utt_rows decrease";
    }
    return nullptr;
}

}  // namespace ctc
}  // namespace fa
