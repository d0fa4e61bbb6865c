// The route decisions of the CTC and TDT decoders' host side (fluidaudio_amd/csrc/ctc_route.h and tdt_route.h, the parts of ctc_launch.h /
// tdt_launch.h without HIP types: what ctc.hip's and tdt.hip's launchers and ctc_host.hip decide with) driven over stdin: one command per
// line.  Test infrastructure: built by tests/test_decoder_routes.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   tdt f16 vocab_with_blank row_stride pointer                      -> route (0 streaming, 1 fits W = 1, 2 fits W = 2) and "limit N"
//   greedy f16 vocab row_stride matrix_stride pointer                -> mode (0 aligned, 1 head + body + tail, 2 scalar loads)
//   lsm f16 vocab row_stride matrix_stride pointer out_pointer       -> "0" or "1" (the vec4 kernel)
//   rows batch total_rows has_utt has_offsets has_token_ids n_offsets offsets... n_utt utt...
//       -> the error text of the contract (rows_call_error, then — for arrays that are given — rows_offsets_error) or "ok"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/ctc_route.h"
#include "../../fluidaudio_amd/csrc/tdt_route.h"

static bool read_array(std::vector<int64_t> &v) {
    int64_t n;
    if (scanf("%" SCNd64, &n) != 1 || n < 0) return false;
    v.resize(static_cast<size_t>(n));
    for (int64_t &x : v) if (scanf("%" SCNd64, &x) != 1) return false;
    return true;
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        int f16;
        int32_t vocab;
        int64_t row_stride, matrix_stride;
        uint64_t p, q;
        if (!strcmp(cmd, "tdt")) {
            if (scanf("%d %d %" SCNd64 " %" SCNu64, &f16, &vocab, &row_stride, &p) != 4) return 2;
            printf("%d limit %d\n", static_cast<int>(fa::tdt::logits_route(f16 != 0, vocab, row_stride, static_cast<uintptr_t>(p))), fa::tdt::kFitsLogits);
        } else if (!strcmp(cmd, "greedy")) {
            if (scanf("%d %d %" SCNd64 " %" SCNd64 " %" SCNu64, &f16, &vocab, &row_stride, &matrix_stride, &p) != 5) return 2;
            printf("%d\n", fa::ctc::greedy_mode(f16 != 0, vocab, row_stride, matrix_stride, static_cast<uintptr_t>(p)));
        } else if (!strcmp(cmd, "lsm")) {
            if (scanf("%d %d %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64, &f16, &vocab, &row_stride, &matrix_stride, &p, &q) != 6) return 2;
            printf("%d\n", fa::ctc::log_softmax_vec4(f16 != 0, vocab, row_stride, matrix_stride, static_cast<uintptr_t>(p), static_cast<uintptr_t>(q)) ? 1 : 0);
        } else if (!strcmp(cmd, "rows")) {
            int32_t batch;
            int64_t total_rows;
            int has_utt, has_off, has_tok;
            std::vector<int64_t> off, utt;
            if (scanf("%d %" SCNd64 " %d %d %d", &batch, &total_rows, &has_utt, &has_off, &has_tok) != 5 || !read_array(off) || !read_array(utt)) return 2;
            const char *err = fa::ctc::rows_call_error(batch, total_rows, has_utt != 0, has_off != 0, has_tok != 0);
            // the walk reads row_offsets[0 .. total_rows] and utt_rows[0 .. batch]: the sanitizers watch those bounds
            if (!err && batch > 0) {
                if ((total_rows > 0 && off.size() != static_cast<size_t>(total_rows) + 1) || (has_utt && utt.size() != static_cast<size_t>(batch) + 1)) return 2;
                err = fa::ctc::rows_offsets_error(off.data(), total_rows, has_utt ? utt.data() : nullptr, batch);
            }
            printf("%s\n", err ? err : "ok");
        } else {
            return 2;
        }
    }
    return 0;
}
