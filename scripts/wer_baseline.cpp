// The single-core baseline of scripts/wer_probe.py: WERCalculator.editDistance as the reference writes it — a full (m + 1) x (n + 1) table
// of 64-bit integers per pair, filled row by row and walked back — over a file of pairs.  Written for the probe only.
//   wer_baseline <file>      int64 n_pairs, int64 hyp_range[n_pairs + 1], int64 ref_range[n_pairs + 1], int32 hyp[], int32 ref[]
//   prints                   milliseconds, then the sums of total, insertions, deletions, substitutions over the pairs
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t P = 0;
    if (std::fread(&P, 8, 1, f) != 1 || P < 0) return 2;
    std::vector<int64_t> hr(P + 1), rr(P + 1);
    if (std::fread(hr.data(), 8, P + 1, f) != size_t(P + 1) || std::fread(rr.data(), 8, P + 1, f) != size_t(P + 1)) return 2;
    std::vector<int32_t> hyp(hr[P]), ref(rr[P]);
    if (std::fread(hyp.data(), 4, hyp.size(), f) != hyp.size() || std::fread(ref.data(), 4, ref.size(), f) != ref.size()) return 2;
    std::fclose(f);
    int64_t sum[4] = {0, 0, 0, 0};
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t k = 0; k < P; ++k) {
        const int32_t *a = hyp.data() + hr[k], *b = ref.data() + rr[k];
        const int64_t m = hr[k + 1] - hr[k], n = rr[k + 1] - rr[k];
        if (m == 0) { sum[0] += n; sum[1] += n; continue; }
        if (n == 0) { sum[0] += m; sum[2] += m; continue; }
        std::vector<std::vector<int64_t>> dp(m + 1, std::vector<int64_t>(n + 1, 0));   // Array(repeating: Array(repeating: 0, count: n + 1), count: m + 1)
        for (int64_t i = 0; i <= m; ++i) dp[i][0] = i;
        for (int64_t j = 0; j <= n; ++j) dp[0][j] = j;
        for (int64_t i = 1; i <= m; ++i)
            for (int64_t j = 1; j <= n; ++j)
                dp[i][j] = a[i - 1] == b[j - 1] ? dp[i - 1][j - 1] : 1 + std::min(dp[i - 1][j], std::min(dp[i][j - 1], dp[i - 1][j - 1]));
        int64_t i = m, j = n, ins = 0, del = 0, sub = 0;
        while (i > 0 || j > 0) {
            if (i > 0 && j > 0 && a[i - 1] == b[j - 1]) { --i; --j; }
            else if (i > 0 && j > 0 && dp[i][j] == dp[i - 1][j - 1] + 1) { ++sub; --i; --j; }
            else if (i > 0 && dp[i][j] == dp[i - 1][j] + 1) { ++del; --i; }
            else if (j > 0 && dp[i][j] == dp[i][j - 1] + 1) { ++ins; --j; }
            else break;
        }
        sum[0] += dp[m][n]; sum[1] += ins; sum[2] += del; sum[3] += sub;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%.3f %lld %lld %lld %lld\n", ms, (long long)sum[0], (long long)sum[1], (long long)sum[2], (long long)sum[3]);
    return 0;
}
