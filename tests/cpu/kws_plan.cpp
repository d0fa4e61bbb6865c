// A stand-alone program over fluidaudio_amd/csrc/kws_plan.h, the word spotter's host plan, built with the address and
// undefined-behaviour sanitizers by tests/test_kws_plan.py.  It reads one case from stdin and stands in for the device: a spotting case
// carries the candidates of every (utterance, keyword), which the program serves pass by pass through an arena by the kernel's protocol
// (kws.hip: a job reserves kChunk records at a time from a cursor that advances whether or not the chunk fitted; a job that did not fit
// once writes nothing more and reports -1; otherwise it reports its candidates and marks the unused tail of its last chunk with job -1),
// the jobs of a pass taking their chunks in turn as concurrent wavefronts would.  Every array handed to the plan has exactly its size,
// on the heap.  It prints what the plan decided and delivered for the test to hold against tests/kws_restatement.py.
//
//   check  batch frames vocab row_stride matrix_stride has_lp has_off has_tokens keywords off[0 .. keywords]
//   spot   batch frames valid[batch] keywords len[keywords] merge capacity forced corrupt, then per (utterance, keyword) n and n x (score bits, start, end)
//          forced: the arena asked for, -1 none.  corrupt: 0 none; 1 / 2 a record naming job take / take + 5; 3 a status one too high;
//          4 a -1 in a later pass
//   window batch frames valid[batch] keywords len[keywords] n and n x (utterance keyword start end)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "../../fluidaudio_amd/csrc/kws_plan.h"

namespace kws = fa::kws;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
template <class T> static T read() { T v; if (!(std::cin >> v)) { std::fprintf(stderr, "short input\n"); std::exit(2); } return v; }
static int refused(const fa::Verdict &v) { std::printf("VERDICT %d %s\n", static_cast<int>(v.status), v.text); return 0; }

struct Case {   // the arrays of a problem, each exactly its size
    int32_t batch = 0, frames = 0, keywords = 0;
    int32_t *valid = nullptr, *tokens = nullptr;
    int64_t *off = nullptr;
    float *lp = nullptr;
    kws::Problem p;
    void read_shape() {
        batch = read<int32_t>(); frames = read<int32_t>();
        valid = new int32_t[batch];
        for (int32_t u = 0; u < batch; ++u) valid[u] = read<int32_t>();
        keywords = read<int32_t>();
        off = new int64_t[keywords + 1];
        off[0] = 0;
        for (int32_t k = 0; k < keywords; ++k) off[k + 1] = off[k] + read<int32_t>();
        tokens = new int32_t[off[keywords]]();
        lp = new float[1]();   // named, never read: the plan does no DP step
    }
    fa::Verdict check() { return kws::check_problem(lp, batch, frames, 1, 1, frames, valid, tokens, off, keywords, 0, p); }
    ~Case() { delete[] valid; delete[] tokens; delete[] off; delete[] lp; }
};

static int run_check() {
    const int32_t batch = read<int32_t>(), frames = read<int32_t>(), vocab = read<int32_t>();
    const int64_t row_stride = read<int64_t>(), matrix_stride = read<int64_t>();
    const int has_lp = read<int>(), has_off = read<int>(), has_tokens = read<int>();
    const int32_t keywords = read<int32_t>();
    const int32_t n_off = keywords > 0 ? keywords + 1 : 1;
    int64_t *off = new int64_t[n_off]();
    for (int32_t k = 0; has_off && keywords > 0 && k < n_off; ++k) off[k] = read<int64_t>();
    float *lp = new float[1]();
    int32_t *tokens = new int32_t[1]();
    kws::Problem p;
    const fa::Verdict v = kws::check_problem(has_lp ? lp : nullptr, batch, frames, vocab, row_stride, matrix_stride, nullptr, has_tokens ? tokens : nullptr,
                                             has_off ? off : nullptr, keywords, 0, p);
    delete[] off; delete[] lp; delete[] tokens;
    return refused(v);
}

struct Candidate { uint32_t score; int32_t start, end; };

static int run_spot() {
    Case c;
    c.read_shape();
    const int merge = read<int>();
    const int64_t capacity = read<int64_t>(), forced = read<int64_t>();
    const int corrupt = read<int>();
    std::vector<std::vector<Candidate>> cands(static_cast<size_t>(c.batch) * c.keywords);
    for (auto &list : cands) {
        list.resize(read<size_t>());
        for (Candidate &x : list) { x.score = read<uint32_t>(); x.start = read<int32_t>(); x.end = read<int32_t>(); }
    }
    fa::Verdict v = c.check();
    if (v.status != FA_SUCCESS) return refused(v);
    std::vector<kws::Job> jobs;
    int64_t worst_one = 0;
    v = kws::spot_jobs(c.p, jobs, worst_one);
    if (v.status != FA_SUCCESS) return refused(v);
    for (const kws::Job &j : jobs) std::printf("JOB %d %d %d %d %zu\n", j.utterance, j.keyword, j.t0, j.t1, cands[static_cast<size_t>(j.utterance) * c.keywords + j.keyword].size());
    const int64_t J = static_cast<int64_t>(jobs.size());
    const kws::Arena arena = kws::arena_of(J, capacity, forced, worst_one);
    std::printf("ARENA %" PRId64 " %" PRId64 " %" PRId64 "\n", arena.cap, arena.slice, worst_one);

    int64_t count = -1;
    int64_t *utt_counts = new int64_t[c.batch]();
    fa_kws_detection *dets = new fa_kws_detection[capacity];
    for (int64_t i = 0; i < capacity; ++i) dets[i] = fa_kws_detection{-7, -7, 0.0f, -7, -7};   // untouched: stays so
    kws::Passes passes;
    passes.begin(c.p, jobs, arena);
    std::vector<kws::Record> device(static_cast<size_t>(arena.cap));
    while (passes.next()) {
        const size_t take = passes.pass_jobs.size();
        bool by_class = true, reordered = false;
        for (size_t i = 0; i < take; ++i) {
            const kws::Job &j = passes.pass_jobs[i], &w = jobs[passes.ids[i]];
            if (std::memcmp(&j, &w, sizeof(j)) != 0) { std::fprintf(stderr, "pass job %zu is not jobs[ids]\n", i); return 3; }
            if (i > 0 && kws::class_of(c.p.len(j.keyword)) < kws::class_of(c.p.len(passes.pass_jobs[i - 1].keyword))) by_class = false;
            if (i > 0 && passes.ids[i] < passes.ids[i - 1]) reordered = true;
        }
        if (!by_class) { std::fprintf(stderr, "a pass is not ordered by class\n"); return 3; }
        // the device: the jobs take their chunks in turn
        unsigned long long cursor = 0;
        int32_t *status = new int32_t[take]();
        std::vector<size_t> written(take, 0);
        int overflowed = 0;
        for (bool any = true; any;) {
            any = false;
            for (size_t i = 0; i < take; ++i) {
                const kws::Job &j = passes.pass_jobs[i];
                const std::vector<Candidate> &mine = cands[static_cast<size_t>(j.utterance) * c.keywords + j.keyword];
                if (status[i] < 0 || written[i] == mine.size()) continue;
                const unsigned long long at = cursor;
                cursor += kws::kChunk;
                if (at + kws::kChunk > static_cast<unsigned long long>(arena.cap)) { status[i] = -1; ++overflowed; continue; }
                for (int s = 0; s < kws::kChunk; ++s) {
                    kws::Record &r = device[static_cast<size_t>(at) + s];
                    if (written[i] < mine.size()) {
                        const Candidate &x = mine[written[i]++];
                        r = kws::Record{static_cast<int32_t>(i), from_bits(x.score), x.start, x.end};
                    } else {
                        r = kws::Record{-1, 0.0f, 0, 0};
                    }
                }
                any = true;
            }
        }
        for (size_t i = 0; i < take; ++i)
            if (status[i] >= 0) status[i] = static_cast<int32_t>(written[i]);
        const int64_t n_rec = passes.records(cursor);
        kws::Record *recs = new kws::Record[n_rec];
        std::copy(device.begin(), device.begin() + n_rec, recs);
        if ((corrupt == 1 || corrupt == 2) && n_rec > 0) recs[n_rec / 2].job = static_cast<int32_t>(take) + (corrupt == 2 ? 5 : 0);
        if (corrupt == 3)
            for (size_t i = 0; i < take; ++i)
                if (status[i] >= 0) { status[i] += 1; break; }
        if (corrupt == 4 && passes.passes > 0) status[take - 1] = -1;
        std::printf("PASS %d %zu %d %d %d %d %llu %d\n", passes.passes, take, passes.n_class[0], passes.n_class[1], passes.n_class[2], overflowed, cursor, reordered ? 1 : 0);
        v = passes.absorb(cursor, status, recs, merge != 0);
        delete[] status; delete[] recs;
        if (v.status != FA_SUCCESS) break;
    }
    if (v.status == FA_SUCCESS) {
        v = kws::deliver(jobs, passes.done, dets, capacity, &count, utt_counts);
        std::printf("COUNT %" PRId64 "\nUTT", count);
        for (int32_t u = 0; u < c.batch; ++u) std::printf(" %" PRId64, utt_counts[u]);
        std::printf("\n");
        for (int64_t i = 0; i < capacity; ++i) std::printf("DET %d %d %08" PRIx32 " %d %d\n", dets[i].utterance, dets[i].keyword, bits(dets[i].score), dets[i].start_frame, dets[i].end_frame);
    }
    delete[] utt_counts; delete[] dets;
    return refused(v);
}

static int run_window() {
    Case c;
    c.read_shape();
    const int64_t n = read<int64_t>();
    fa_kws_window *windows = new fa_kws_window[n];
    for (int64_t w = 0; w < n; ++w) { windows[w].utterance = read<int32_t>(); windows[w].keyword = read<int32_t>(); windows[w].start_frame = read<int32_t>(); windows[w].end_frame = read<int32_t>(); }
    fa_kws_detection *out = new fa_kws_detection[n];
    fa::Verdict v = c.check();
    kws::WindowPlan plan;
    if (v.status == FA_SUCCESS) v = kws::window_jobs(c.p, windows, n, out, plan);
    if (v.status == FA_SUCCESS) {
        for (int64_t w = 0; w < n; ++w) std::printf("OUT %d %d %08" PRIx32 " %d %d\n", out[w].utterance, out[w].keyword, bits(out[w].score), out[w].start_frame, out[w].end_frame);
        for (size_t i = 0; i < plan.jobs.size(); ++i)
            std::printf("JOB %d %d %d %d %" PRId64 "\n", plan.jobs[i].utterance, plan.jobs[i].keyword, plan.jobs[i].t0, plan.jobs[i].t1, plan.window_of[i]);
        std::printf("CLASSES %d %d %d\n", plan.n_class[0], plan.n_class[1], plan.n_class[2]);
    }
    delete[] windows; delete[] out;
    return refused(v);
}

int main() {
    const std::string mode = read<std::string>();
    if (mode == "check") return run_check();
    if (mode == "spot") return run_spot();
    if (mode == "window") return run_window();
    std::fprintf(stderr, "unknown mode\n");
    return 2;
}
