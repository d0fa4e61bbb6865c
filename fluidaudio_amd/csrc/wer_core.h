// wer_core.h — the per-lane arithmetic of the edit-distance kernel (fluidaudio_amd/csrc/wer.hip): one cell of
// WERCalculator.editDistance (Sources/FluidAudioCLI/Utils/WERCalculator.swift:178-239) with the counts of its traceback carried forward,
// and one row of a lane's strip of columns.
//
// The reference fills the whole (m + 1) x (n + 1) table and walks it back with a fixed priority: a match when the symbols are equal,
// else a substitution when dp[i][j] == dp[i-1][j-1] + 1, else a deletion (dp[i-1][j] + 1), else an insertion (dp[i][j-1] + 1).  Which of
// the four the walk takes at (i, j) depends on that cell and its three neighbours only, so the counts of the path from (i, j) back to
// (0, 0) are a function of the neighbours' counts: a cell is (dp, substitutions, deletions), the insertions are dp - sub - del, and
// cell(m, n) is the reference's answer without a table and without a walk.  Rows are the hypothesis (seq1), columns the reference text
// (seq2); the two may not be swapped, which would exchange the deletion and insertion priorities on ties.
// Everything here is written against registers so the same code runs inside the kernel and inside tests/cpu/wer_emul.cpp, which replays
// the 64 lanes on the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FA_WER_HD __host__ __device__ __forceinline__
#else
#define FA_WER_HD inline
#endif

namespace fa {
namespace wercore {

struct Cell {
    int32_t dp, sub, del;
};

FA_WER_HD Cell row_zero(const int32_t j) { return Cell{j, 0, 0}; }   // cell(0, j): j insertions (:225-227)
FA_WER_HD Cell col_zero(const int32_t i) { return Cell{i, 0, i}; }   // cell(i, 0): i deletions (:222-224)

// cell(i, j) from cell(i-1, j-1), cell(i-1, j), cell(i, j-1) and a[i-1] == b[j-1] (:200-204, :215-227)
FA_WER_HD Cell cell(const bool equal, const Cell diag, const Cell up, const Cell left) {
    const int32_t lo = up.dp < left.dp ? up.dp : left.dp;
    const int32_t d = 1 + (diag.dp < lo ? diag.dp : lo);
    const bool by_sub = d == diag.dp + 1, by_del = d == up.dp + 1;
    Cell c;
    c.dp = equal ? diag.dp : d;
    c.sub = equal ? diag.sub : (by_sub ? diag.sub + 1 : (by_del ? up.sub : left.sub));
    c.del = equal ? diag.del : (by_sub ? diag.del : (by_del ? up.del + 1 : left.del));
    return c;
}

// One hypothesis row of a lane's strip of C consecutive reference columns.  `strip` holds the row above on entry and this row on
// return; `diag` and `left` are the cells of the column left of the strip in the row above and in this row; `token` is the row's
// hypothesis symbol and `ref` the strip's reference symbols.
template <int C>
FA_WER_HD void strip_row(Cell (&strip)[C], const int32_t (&ref)[C], const int32_t token, Cell diag, Cell left) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const Cell up = strip[c];
        left = cell(token == ref[c], diag, up, left);
        strip[c] = left;
        diag = up;
    }
}

}  // namespace wercore
}  // namespace fa
