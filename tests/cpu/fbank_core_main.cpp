// The store plan of the fbank kernel (fluidaudio_amd/csrc/fbank_core.h: for_each_target, the same source the GPU compiles) against
// the naive gather clamp(i n + k - lpad, 0, T - 1): for every T in 0 .. 40, four (m, n) and both tail modes, every element of the
// R x m output is written exactly once and by the frame the gather names.  Prints "ok <cases>" or the first difference.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fluidaudio_amd/csrc/fbank_core.h"

using namespace fa::fbank;

int main() {
    const int shapes[4][2] = {{1, 1}, {5, 1}, {7, 6}, {4, 3}};
    int cases = 0;
    for (const auto &mn : shapes)
        for (int tail = 0; tail < 2; ++tail)
            for (int T = 0; T <= 40; ++T, ++cases) {
                const int m = mn[0], n = mn[1], lpad = lfr_lpad(m), R = static_cast<int>(num_rows(T, m, n, tail));
                std::vector<int> source(static_cast<size_t>(R) * m, -1), writes(static_cast<size_t>(R) * m, 0);
                for (int t = 0; t < T; ++t)
                    for_each_target(t, T, R, m, n, [&](int row, int slot) {
                        if (row < 0 || row >= R || slot < 0 || slot >= m) { printf("out of range: T %d m %d n %d tail %d t %d -> (%d, %d)\n", T, m, n, tail, t, row, slot); exit(1); }
                        source[static_cast<size_t>(row) * m + slot] = t;
                        ++writes[static_cast<size_t>(row) * m + slot];
                    });
                for (int i = 0; i < R; ++i)
                    for (int k = 0; k < m; ++k) {
                        int want = i * n + k - lpad;
                        want = want < 0 ? 0 : (want > T - 1 ? T - 1 : want);
                        if (writes[static_cast<size_t>(i) * m + k] != 1 || source[static_cast<size_t>(i) * m + k] != want) {
                            printf("T %d m %d n %d tail %d: (%d, %d) written %d times by frame %d, the gather takes %d\n", T, m, n, tail, i, k,
                                   writes[static_cast<size_t>(i) * m + k], source[static_cast<size_t>(i) * m + k], want);
                            return 1;
                        }
                    }
                // REPLICATE covers every frame; VALID never replicates the tail
                const int last = R > 0 ? (R - 1) * n + m - 1 - lpad : -1;
                if (tail == kTailReplicate ? (T > 0 && R != (T + n - 1) / n) : last > T - 1) { printf("row count: T %d m %d n %d tail %d R %d\n", T, m, n, tail, R); return 1; }
            }
    printf("ok %d\n", cases);
    return 0;
}
