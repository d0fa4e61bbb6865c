// The host-compilable headers of the AED unit (csrc/aed_core.h, csrc/aed_launch.h) walked on the CPU: the window plan (the loop and
// its closed-form count), the valid-frame rule, the state layout, the step bookkeeping, the launch plans and every refusal of the
// argument passes.  Stand-alone: reads commands from stdin, one per line; built with the address and undefined-behaviour sanitizers
// by tests/test_aed_cpu.py.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fluidaudio_amd/csrc/aed_launch.h"

namespace ad = fa::aed;

static fa_aed_config token_config(int vocab, int max_seq, int max_new, int n, float p) {
    fa_aed_config c = ad::default_config(FA_AED_MODEL_COHERE);
    c.vocab = vocab; c.max_seq = max_seq; c.max_new = max_new; c.no_repeat_ngram = n; c.repetition_penalty = p;
    return c;
}

static void refusals() {
    int32_t lens_ok[2] = {1, 3}, lens_zero[2] = {1, 0}, lens_long[2] = {4, 1}, lens_past_seq[2] = {1, 9};
    int dummy = 0;
    const void *p = &dummy;
    fa_aed_config ok = token_config(16, 8, 4, 3, 1.1f), seq = ad::default_config(FA_AED_MODEL_CANARY);
    auto cfg = [&](auto edit) { fa_aed_config c = ok; edit(c); return ad::check_decode_config(&c).status; };
    std::printf("config %d %d %d %d %d %d %d %d %d %d %d\n", ad::check_decode_config(nullptr).status, ad::check_decode_config(&ok).status, ad::check_decode_config(&seq).status,
                cfg([](fa_aed_config &c) { c.mode = 2; }), cfg([](fa_aed_config &c) { c.vocab = 0; }), cfg([](fa_aed_config &c) { c.vocab = FA_AED_MAX_VOCAB + 1; }),
                cfg([](fa_aed_config &c) { c.max_seq = 0; }), cfg([](fa_aed_config &c) { c.max_seq = FA_AED_MAX_SEQ + 1; }), cfg([](fa_aed_config &c) { c.max_new = -1; }),
                cfg([](fa_aed_config &c) { c.repetition_penalty = std::nanf(""); }), cfg([](fa_aed_config &c) { c.vocab = FA_AED_MAX_VOCAB; c.max_seq = FA_AED_MAX_SEQ; }));
    auto begin = [&](const fa_aed_config *c, int batch, const void *prompts, int stride, const int32_t *lens, const void *state, const void *in, const void *pos,
                     const void *mask, int mdt, const void *ids, const void *dmask) {
        return static_cast<int>(ad::check_begin(c, batch, prompts, stride, lens, state, in, pos, mask, mdt, ids, dmask).status);
    };
    std::printf("begin %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", begin(&ok, 2, p, 3, lens_ok, p, p, p, nullptr, 0, nullptr, nullptr),
                begin(nullptr, 2, p, 3, lens_ok, p, p, p, nullptr, 0, nullptr, nullptr), begin(&ok, 0, p, 3, lens_ok, p, p, p, nullptr, 0, nullptr, nullptr),
                begin(&ok, 2, nullptr, 3, lens_ok, p, p, p, nullptr, 0, nullptr, nullptr), begin(&ok, 2, p, 0, lens_ok, p, p, p, nullptr, 0, nullptr, nullptr),
                begin(&ok, 2, p, 3, nullptr, p, p, p, nullptr, 0, nullptr, nullptr), begin(&ok, 2, p, 3, lens_ok, nullptr, p, p, nullptr, 0, nullptr, nullptr),
                begin(&ok, 2, p, 3, lens_ok, p, nullptr, p, nullptr, 0, nullptr, nullptr), begin(&ok, 2, p, 3, lens_ok, p, p, nullptr, nullptr, 0, nullptr, nullptr),
                begin(&ok, 2, p, 3, lens_ok, p, p, p, p, 7, nullptr, nullptr), begin(&ok, 2, p, 3, lens_zero, p, p, p, nullptr, 0, nullptr, nullptr),
                begin(&ok, 2, p, 3, lens_long, p, p, p, nullptr, 0, nullptr, nullptr), begin(&ok, 2, p, 16, lens_past_seq, p, p, p, nullptr, 0, nullptr, nullptr),
                begin(&seq, 2, p, 3, lens_ok, p, nullptr, nullptr, nullptr, 0, p, p), begin(&seq, 2, p, 3, lens_ok, p, p, p, nullptr, 0, nullptr, p));
    auto step = [&](const fa_aed_config *c, int batch, const void *state, const void *logits, int dt, int64_t stride, const void *in, const void *pos, const void *ids,
                    const void *dmask) { return static_cast<int>(ad::check_step(c, batch, state, logits, dt, stride, in, pos, nullptr, 0, ids, dmask).status); };
    std::printf("step %d %d %d %d %d %d %d %d %d %d\n", step(&ok, 1, p, p, FA_DTYPE_F16, 16, p, p, nullptr, nullptr), step(nullptr, 1, p, p, 0, 16, p, p, nullptr, nullptr),
                step(&ok, 0, p, p, 0, 16, p, p, nullptr, nullptr), step(&ok, 1, nullptr, p, 0, 16, p, p, nullptr, nullptr), step(&ok, 1, p, nullptr, 0, 16, p, p, nullptr, nullptr),
                step(&ok, 1, p, p, 2, 16, p, p, nullptr, nullptr), step(&ok, 1, p, p, 0, 15, p, p, nullptr, nullptr), step(&ok, 1, p, p, 0, 16, nullptr, p, nullptr, nullptr),
                step(&seq, 1, p, p, 0, 16384, nullptr, nullptr, p, p), step(&seq, 1, p, p, 0, 16384, nullptr, nullptr, p, nullptr));
    std::printf("finish %d %d %d %d %d %d\n", ad::check_finish(&ok, 1, p, 5, p, p).status, ad::check_finish(&ok, 1, p, 4, p, p).status, ad::check_finish(&ok, 0, p, 5, p, p).status,
                ad::check_finish(&ok, 1, nullptr, 5, p, p).status, ad::check_finish(&ok, 1, p, 5, nullptr, p).status, ad::check_finish(&ok, 1, p, 5, p, nullptr).status);
    std::printf("strided %d %d %d %d %d %d\n", ad::check_strided(1, 2, 3, 6, 3, 1, 0).status, ad::check_strided(0, 2, 3, 6, 3, 1, 0).status, ad::check_strided(1, 0, 3, 6, 3, 1, 0).status,
                ad::check_strided(1, 2, 0, 6, 3, 1, 0).status, ad::check_strided(1, 2, 3, 6, -3, 1, 0).status, ad::check_strided(1, 2, 3, 6, 3, 1, 2).status);
    int64_t samples[2] = {5, 700000}, bad_samples[2] = {5, -1}, range[3], count = 0, starts[4], lens[4];
    fa_aed_config w = ad::default_config(FA_AED_MODEL_COHERE);
    auto win = [&](auto edit, const int64_t *s, int64_t n, int64_t *r, int64_t *st, int64_t *ln, int64_t cap, int64_t *cnt) {
        fa_aed_config c = w;
        edit(c);
        return static_cast<int>(ad::check_windows(&c, s, n, r, st, ln, cap, cnt).status);
    };
    auto same = [](fa_aed_config &) {};
    std::printf("windows %d %d %d %d %d %d %d %d %d %d %d %d\n", win(same, samples, 2, range, starts, lens, 4, &count), static_cast<int>(ad::check_windows(nullptr, samples, 2, range, starts, lens, 4, &count).status),
                win(same, samples, 2, range, starts, lens, 4, nullptr), win([](fa_aed_config &c) { c.chunk_samples = 0; }, samples, 2, range, nullptr, nullptr, 0, &count),
                win([](fa_aed_config &c) { c.hop_samples = 0; }, samples, 2, range, nullptr, nullptr, 0, &count),
                win([](fa_aed_config &c) { c.hop_samples = c.chunk_samples + 1; }, samples, 2, range, nullptr, nullptr, 0, &count), win(same, samples, -1, range, nullptr, nullptr, 0, &count),
                win(same, nullptr, 2, range, nullptr, nullptr, 0, &count), win(same, samples, 2, nullptr, nullptr, nullptr, 0, &count), win(same, samples, 2, range, starts, nullptr, 4, &count),
                win(same, bad_samples, 2, range, nullptr, nullptr, 0, &count), win(same, samples, 0, nullptr, nullptr, nullptr, 0, &count));
    int64_t huge[2] = {INT64_MAX, INT64_MAX};
    fa_aed_config one = w;
    one.chunk_samples = one.hop_samples = 1;
    std::printf("overflow %d\n", ad::count_windows(one, huge, 2, range, &count).status);
    const int64_t woff[4] = {0, 3, 3, 8}, rr[3] = {0, 2, 3}, orange_ok[3] = {0, 3, 8}, orange_small[3] = {0, 3, 7}, rr_desc[3] = {0, 2, 1}, woff_desc[4] = {0, 3, 2, 8};
    fa_aed_config m = w;
    auto mrg = [&](const fa_aed_config *c, const void *tok, const int64_t *wo, const int64_t *r, int64_t n, const void *out, const int64_t *orr, const void *cnt) {
        return static_cast<int>(ad::check_merge(c, tok, wo, r, n, out, orr, cnt).status);
    };
    fa_aed_config m0 = m, m65 = m, m64 = m;
    m0.window_tokens = 0; m65.window_tokens = 65; m64.window_tokens = 64;
    std::printf("merge %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", mrg(&m, p, woff, rr, 2, p, orange_ok, p), mrg(nullptr, p, woff, rr, 2, p, orange_ok, p), mrg(&m64, p, woff, rr, 2, p, orange_ok, p),
                mrg(&m0, p, woff, rr, 2, p, orange_ok, p), mrg(&m65, p, woff, rr, 2, p, orange_ok, p), mrg(&m, p, woff, rr, -1, p, orange_ok, p), mrg(&m, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr),
                mrg(&m, p, nullptr, rr, 2, p, orange_ok, p), mrg(&m, p, woff, rr, 2, p, orange_ok, nullptr), mrg(&m, p, woff, rr_desc, 2, p, orange_ok, p),
                mrg(&m, p, woff_desc, rr, 2, p, orange_ok, p), mrg(&m, p, woff, rr, 2, p, orange_small, p), mrg(&m, nullptr, woff, rr, 2, p, orange_ok, p), mrg(&m, p, woff, rr, 2, nullptr, orange_ok, p));
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "windows") {
            int64_t chunk, hop, samples;
            in >> chunk >> hop >> samples;
            const int64_t n = ad::plan_windows_one(samples, chunk, hop, nullptr, nullptr);
            std::vector<int64_t> starts(static_cast<size_t>(n)), lens(static_cast<size_t>(n));
            ad::plan_windows_one(samples, chunk, hop, starts.data(), lens.data());
            std::printf("windows %lld %lld", static_cast<long long>(n), static_cast<long long>(ad::window_count(samples, chunk, hop)));
            for (int64_t i = 0; i < n; ++i) std::printf(" %lld %lld", static_cast<long long>(starts[i]), static_cast<long long>(lens[i]));
            std::printf("\n");
        } else if (cmd == "valid") {
            int64_t fl, seq, mel, enc;
            in >> fl >> seq >> mel >> enc;
            std::printf("valid %lld\n", static_cast<long long>(ad::encoder_valid_frames(fl, seq, mel, enc)));
        } else if (cmd == "layout") {
            int mode, vocab, max_seq, max_new;
            in >> mode >> vocab >> max_seq >> max_new;
            fa_aed_config c = token_config(vocab, max_seq, max_new, 3, 1.1f);
            c.mode = mode;
            const ad::Layout l = ad::layout_of(c);
            std::printf("layout %d %lld %lld %lld %lld %d\n", l.max_out, static_cast<long long>(l.words()), static_cast<long long>(l.hist()), static_cast<long long>(l.prompt()),
                        static_cast<long long>(l.out()), static_cast<int>(ad::kHead));
        } else if (cmd == "last") {
            int max_new, P, max_seq, step;
            in >> max_new >> P >> max_seq >> step;
            std::printf("last %d %d\n", ad::token_last_step(max_new, P, max_seq), ad::token_decides(step, P) ? 1 : 0);
        } else if (cmd == "stepplan") {
            int mode, vocab, max_seq, n, batch;
            float p;
            in >> mode >> vocab >> max_seq >> n >> p >> batch;
            fa_aed_config c = token_config(vocab, max_seq, 8, n, p);
            c.mode = mode;
            const ad::StepPlan s = ad::step_plan(c, batch);
            const ad::TilePlan t = ad::tile_plan(batch, vocab, max_seq);
            std::printf("stepplan %u %u %u %d %u %u %u %u\n", s.grid, s.block, s.lds_bytes, s.marked, t.gx, t.gy, t.gz, t.block);
        } else if (cmd == "defaults") {
            for (int model = 0; model < 2; ++model) {
                const fa_aed_config c = ad::default_config(model);
                std::printf("defaults %d %d %d %d %d %d %g %d %d %lld %lld %d\n", c.mode, c.vocab, c.eos_id, c.max_seq, c.max_new, c.no_repeat_ngram, static_cast<double>(c.repetition_penalty),
                            c.window_tokens, c.min_match, static_cast<long long>(c.chunk_samples), static_cast<long long>(c.hop_samples), ad::max_out_of(c));
            }
        } else if (cmd == "refusals") {
            refusals();
        }
    }
    return 0;
}
