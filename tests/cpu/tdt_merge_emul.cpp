// The TDT seam merge walked on the host: csrc/tdt_merge_core.h (the code the kernel is built from) over a wave of ONE lane, with the
// plan, the slot layout and the argument pass of csrc/tdt_merge_launch.h.  Stand-alone; tests/test_tdt_merge_emul.py builds it with the
// address and undefined-behaviour sanitizers and compares it with tests/tdt_merge_restatement.py; scripts/tdt_merge_timing.py builds it
// -O2 as the host fold a caller would otherwise run.  Every buffer has exactly the size the plan gives it (the LDS scratch: the size
// the call's LDS limit needs, array by array) and starts out poisoned, so an index beyond what the plan promises ends the program and
// a value read before it was written changes the answer.
//
// stdin:  n_recordings vocab has_safe has_canon lds_side max_out frame overlap (%la)   [safe: vocab ints] [canon: vocab ints]
//         per recording: capacity n_windows; per window: count n_stored, then n_stored lines "token timestamp duration confidence-bits"
// stdout: per recording: "R status count", count lines "token timestamp duration confidence-bits", "ROUTES" and a route per window
// argv[1] == "time": the folds are repeated argv[2] times and "SECONDS s" (the best repeat) is printed instead.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fluidaudio_amd/csrc/tdt_merge_launch.h"

namespace mg = fa::tdtmerge;

struct Wave1 {
    static constexpr int kLanes = 1;
    int lane() const { return 0; }
    static int first_bit(const unsigned long long m) { return __builtin_ctzll(m); }
    static int count_bits(const unsigned long long m) { return __builtin_popcountll(m); }
    unsigned long long ballot(const bool p) const { return p ? 1ull : 0ull; }
    int prefix(unsigned long long) const { return 0; }
    int32_t max_i32(const int32_t v) const { return v; }
    long long min_i64(const long long v) const { return v; }
    int32_t scan_max_incl(const int32_t v) const { return v; }
    int32_t shift_up(int32_t, const int32_t fill) const { return fill; }
    int32_t bcast(const int32_t v, int) const { return v; }
    void sync() const {}
};

template <class T>
static T *poisoned(const size_t n) {
    T *p = static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1));
    if (!p) std::abort();
    std::memset(p, 0xA5, n * sizeof(T));
    return p;
}

static void need(const bool ok) {
    if (!ok) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
}

int main(int argc, char **argv) {
    const bool timing = argc > 2 && std::strcmp(argv[1], "time") == 0;
    const int repeats = timing ? std::max(1, std::atoi(argv[2])) : 1;
    long long n = 0;
    int vocab = 0, has_safe = 0, has_canon = 0, lds_side = 0, max_out = 0;
    double frame = 0, overlap = 0;
    need(std::scanf("%lld %d %d %d %d %d %la %la", &n, &vocab, &has_safe, &has_canon, &lds_side, &max_out, &frame, &overlap) == 8);
    std::vector<uint8_t> safe(static_cast<size_t>(vocab) + 1);   // + 1: a table without entries is still a table
    std::vector<int32_t> canon(static_cast<size_t>(vocab) + 1);
    for (int i = 0; has_safe && i < vocab; ++i) { int v; need(std::scanf("%d", &v) == 1); safe[i] = static_cast<uint8_t>(v); }
    for (int i = 0; has_canon && i < vocab; ++i) need(std::scanf("%d", &canon[i]) == 1);

    std::vector<int64_t> window_range{0}, out_range{0};
    std::vector<int32_t> tok, tim, dur, counts;
    std::vector<float> conf;
    for (long long r = 0; r < n; ++r) {
        long long cap = 0, nw = 0;
        need(std::scanf("%lld %lld", &cap, &nw) == 2);
        for (long long k = 0; k < nw; ++k) {
            int count = 0, stored = 0;
            need(std::scanf("%d %d", &count, &stored) == 2 && stored <= max_out);
            const size_t at = tok.size();
            tok.resize(at + max_out, -77); tim.resize(at + max_out, -77); dur.resize(at + max_out, -77); conf.resize(at + max_out, -77.0f);
            for (int i = 0; i < stored; ++i) {
                unsigned bits = 0;
                need(std::scanf("%d %d %d %u", &tok[at + i], &tim[at + i], &dur[at + i], &bits) == 4);
                std::memcpy(&conf[at + i], &bits, 4);
            }
            counts.push_back(count);
        }
        window_range.push_back(window_range.back() + nw);
        out_range.push_back(out_range.back() + cap);
    }
    // exact-size copies of the windows, so that a read beyond them is seen
    int32_t *w_tok = poisoned<int32_t>(tok.size()), *w_tim = poisoned<int32_t>(tok.size()), *w_dur = poisoned<int32_t>(tok.size()), *w_cnt = poisoned<int32_t>(counts.size());
    float *w_conf = poisoned<float>(tok.size());
    if (!tok.empty()) {
        std::memcpy(w_tok, tok.data(), 4 * tok.size()); std::memcpy(w_tim, tim.data(), 4 * tok.size());
        std::memcpy(w_dur, dur.data(), 4 * tok.size()); std::memcpy(w_conf, conf.data(), 4 * tok.size());
    }
    if (!counts.empty()) std::memcpy(w_cnt, counts.data(), 4 * counts.size());

    const fa_tdt_merge_config cfg{frame, overlap};
    int32_t none = 0;
    const fa::Verdict v = mg::check(cfg, w_tok, w_tim, w_dur, w_conf, w_cnt, max_out, window_range.data(), n, vocab, &none, &none, &none, &none, out_range.data(), &none, &none);
    if (v.status != FA_SUCCESS) {
        std::printf("CHECK %d %s\n", static_cast<int>(v.status), v.text);
        std::free(w_tok); std::free(w_tim); std::free(w_dur); std::free(w_conf); std::free(w_cnt);
        return 0;
    }
    mg::Plan plan;
    if (n > 0) mg::make_plan(window_range.data(), out_range.data(), n, max_out, plan);
    const int32_t side = mg::small_side_of(lds_side >= 0 ? std::to_string(lds_side).c_str() : nullptr);
    const mg::Tables tb{has_safe ? safe.data() : nullptr, has_canon ? canon.data() : nullptr, vocab};
    const mg::Times tm{frame, overlap};
    const mg::Stream win{w_tok, w_tim, w_dur, w_conf};
    std::vector<int32_t> routes(counts.size(), 12345);

    struct Result { int32_t status, count; std::vector<int32_t> tok, tim, dur; std::vector<float> conf; };
    std::vector<Result> results(static_cast<size_t>(n));
    double best = 1e300;
    Wave1 w;
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        // one slot: the recordings are folded one after the other, as one wavefront of the grid would
        unsigned char *slot = n > 0 ? poisoned<unsigned char>(static_cast<size_t>(plan.slot_bytes)) : nullptr;
        mg::Scratch small;
        const size_t sl = static_cast<size_t>(side);
        small.l_idx = poisoned<int32_t>(sl); small.r_idx = poisoned<int32_t>(sl);
        small.l_key = poisoned<long long>(sl); small.r_key = poisoned<long long>(sl);
        small.l_start = poisoned<double>(sl); small.r_start = poisoned<double>(sl);
        small.row0 = poisoned<int32_t>(sl + 1); small.row1 = poisoned<int32_t>(sl + 1);
        small.bits = poisoned<unsigned long long>(sl * static_cast<size_t>(mg::words_per_row(side)));
        for (long long r = 0; r < n; ++r) {
            const mg::Rec rec = plan.recs[r];
            const size_t cap = static_cast<size_t>(rec.cap);
            mg::Fold f;
            f.out = mg::Stream{poisoned<int32_t>(cap), poisoned<int32_t>(cap), poisoned<int32_t>(cap), poisoned<float>(cap)};
            f.runmax = poisoned<int32_t>(cap);
            f.cap = rec.cap;
            f.n = 0;
            mg::Scratch big;
            mg::slot_views(slot, plan.big_l, plan.big_r, f.stage, big);
            Result &res = results[r];
            res.status = mg::fold_recording(w, f, win, w_cnt, max_out, rec.w_lo, rec.w_hi, tb, tm, small, side, big, routes.data(), &res.count);
            res.tok.assign(f.out.tok, f.out.tok + res.count); res.tim.assign(f.out.time, f.out.time + res.count);
            res.dur.assign(f.out.dur, f.out.dur + res.count); res.conf.assign(f.out.conf, f.out.conf + res.count);
            std::free(f.out.tok); std::free(f.out.time); std::free(f.out.dur); std::free(f.out.conf); std::free(f.runmax);
        }
        std::free(small.l_idx); std::free(small.r_idx); std::free(small.l_key); std::free(small.r_key); std::free(small.l_start); std::free(small.r_start);
        std::free(small.row0); std::free(small.row1); std::free(small.bits); std::free(slot);
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::free(w_tok); std::free(w_tim); std::free(w_dur); std::free(w_conf); std::free(w_cnt);
    if (timing) { std::printf("SECONDS %.9f\n", best); return 0; }
    for (long long r = 0; r < n; ++r) {
        const Result &res = results[r];
        std::printf("R %d %d\n", res.status, res.count);
        for (int32_t i = 0; i < res.count; ++i) {
            unsigned bits;
            std::memcpy(&bits, &res.conf[i], 4);
            std::printf("%d %d %d %u\n", res.tok[i], res.tim[i], res.dur[i], bits);
        }
        std::printf("ROUTES");
        for (int64_t k = window_range[r]; k < window_range[r + 1]; ++k) std::printf(" %d", routes[k]);
        std::printf("\n");
    }
    return 0;
}
