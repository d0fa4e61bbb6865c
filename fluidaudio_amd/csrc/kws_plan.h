// kws_plan.h — the host plan of the CTC word spotter (kernel: kws.hip, entries: kws_host.hip, operands: kws_launch.h): the argument pass,
// the job lists of a spotting call and of a window call, the width classes, the arena rule, the passes over the arena with what each
// pass hands back (the records by job, the checks on what the device wrote, mergeOverlap: CtcDPAlgorithm.swift:372-391) and the
// delivery of the detections.  Plain C++ without a HIP call, shared by the two units and by tests/cpu/kws_plan.cpp, which stands in
// for the device and walks all of it under the sanitizers.  Internal; not part of the C ABI.
//
// A spotting call makes one job per (utterance, keyword) that can match at all (1 <= tokens <= valid frames), ordered by utterance, and
// launches them by width class (1, 2 or 4 states per lane).  The candidates come back through an arena of O(jobs + capacity) records.
// The first pass takes every job; a job whose chunk did not fit reports -1 and is walked again, by passes that take only as many jobs
// as fit the arena at the most candidates a job can have (every other sample of its scan), so each of those passes finishes all its
// jobs.  Whatever indexes a host array with a value the device wrote does so here, behind its check.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "fa_verdict.h"

namespace fa {
namespace kws {

constexpr int kWave = 64;
constexpr int kChunk = 8;           // arena records a job reserves with one atomic

// the widest keyword of a launch with R states per lane: 2N + 1 <= 64 R
constexpr int max_tokens(const int states_per_lane) { return (kWave * states_per_lane - 1) / 2; }
static_assert(max_tokens(4) == FA_KWS_MAX_TOKENS, "four states per lane serve the longest keyword the ABI admits");
inline int class_of(const int32_t tokens) { return tokens <= max_tokens(1) ? 0 : (tokens <= max_tokens(2) ? 1 : 2); }

struct Job {
    int32_t utterance, keyword;
    int32_t t0, t1;                 // the frames [t0, t1) the DP walks: 1 <= tokens <= t1 - t0
};

struct Record {                     // a candidate before sort-and-merge (spotting), or a window's answer (constrained)
    int32_t job;                    // index into the launch's job list; -1: the unused tail of a reserved chunk
    float score;
    int32_t start, end;
};

struct Problem {   // the validated arguments both entries share
    int32_t batch = 0, frames = 0, vocab = 0, keywords = 0, blank = 0;
    int64_t row_stride = 0, matrix_stride = 0;
    const int32_t *tokens = nullptr;
    const int64_t *off = nullptr;
    std::vector<int32_t> valid;   // frames of each utterance, clamped to [0, frames]
    int32_t len(const int32_t k) const { return static_cast<int32_t>(off[k + 1] - off[k]); }
};

// The argument pass; the texts go behind the entry's name.
inline Verdict check_problem(const float *lp, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames,
                             const int32_t *tokens, const int64_t *off, int32_t keywords, int32_t blank, Problem &p) {
    if (batch < 0 || frames < 0 || vocab < 1 || row_stride < vocab || keywords < 0) return refuse(FA_INVALID_ARGUMENT, "bad shape");
    if (batch > 0 && frames > 0 && (!lp || (batch > 1 && matrix_stride < static_cast<int64_t>(frames - 1) * row_stride + vocab)))
        return refuse(FA_INVALID_ARGUMENT, "bad log-prob pointer or strides");
    if (keywords > 0 && !off) return refuse(FA_INVALID_ARGUMENT, "keyword_offsets is required");
    if (keywords > 0 && off[0] < 0) return refuse(FA_INVALID_ARGUMENT, "keyword_offsets starts below 0");
    for (int32_t k = 0; k < keywords; ++k) {
        const int64_t n = off[k + 1] - off[k];
        if (n < 0) return refuse(FA_INVALID_ARGUMENT, "keyword_offsets does not ascend at keyword %d", k);
        if (n > FA_KWS_MAX_TOKENS) return refuse(FA_INVALID_ARGUMENT, "keyword %d has %lld tokens, at most %d are supported", k, (long long)n, (int)FA_KWS_MAX_TOKENS);
    }
    if (keywords > 0 && off[keywords] > off[0] && !tokens) return refuse(FA_INVALID_ARGUMENT, "keyword_tokens is required");
    p.batch = batch; p.frames = frames; p.vocab = vocab; p.keywords = keywords; p.blank = blank;
    p.row_stride = row_stride; p.matrix_stride = matrix_stride; p.tokens = tokens; p.off = off;
    p.valid.assign(static_cast<size_t>(batch), frames);
    if (valid_frames)
        for (int32_t b = 0; b < batch; ++b) p.valid[b] = std::min(frames, std::max(0, valid_frames[b]));
    return Verdict{};
}

// `ids` (indices into `jobs`) reordered by width class, each class in its former order; n[c] jobs in class c
inline void order_by_class(const Problem &p, const std::vector<Job> &jobs, std::vector<int32_t> &ids, int32_t (&n)[3]) {
    std::vector<int32_t> out;
    out.reserve(ids.size());
    for (int c = 0; c < 3; ++c) {
        n[c] = 0;
        for (const int32_t i : ids)
            if (class_of(p.len(jobs[i].keyword)) == c) { out.push_back(i); ++n[c]; }
    }
    ids.swap(out);
}

// the most candidates a job can have, rounded up to whole chunks: every other sample of its scan t = N ... T, or the one fallback
inline int64_t worst_records(const Problem &p, const Job &j) {
    const int64_t samples = static_cast<int64_t>(j.t1 - j.t0) - p.len(j.keyword) + 1;
    return ((samples + 1) / 2 + kChunk - 1) / kChunk * kChunk;
}

// The jobs of a spotting call, by utterance, then keyword; worst_one: the most records one of them can need (a chunk at the least).
inline Verdict spot_jobs(const Problem &p, std::vector<Job> &jobs, int64_t &worst_one) {
    jobs.clear();
    worst_one = kChunk;
    for (int32_t u = 0; u < p.batch; ++u)
        for (int32_t k = 0; k < p.keywords; ++k) {
            const int32_t n = p.len(k), T = p.valid[u];
            if (n == 0 || T == 0 || T < n) continue;   // :321-323, :336
            if (jobs.size() >= static_cast<size_t>(INT32_MAX - 1)) return refuse(FA_INDEX_OVERFLOW, "2^31 jobs or more");
            jobs.push_back(Job{u, k, 0, T});
            worst_one = std::max(worst_one, worst_records(p, jobs.back()));
        }
    return Verdict{};
}

// The one launch of a window call: the jobs by utterance (the workgroups share rows), then by class; job i answers window window_of[i].
struct WindowPlan {
    std::vector<Job> jobs;
    std::vector<int64_t> window_of;
    int32_t n_class[3] = {0, 0, 0};
};

// Every window's answer is pre-filled as the reference leaves it without a walk (ctcWordSpotConstrained :260-272); the others become jobs.
inline Verdict window_jobs(const Problem &p, const fa_kws_window *windows, const int64_t n_windows, fa_kws_detection *out, WindowPlan &plan) {
    for (int64_t w = 0; w < n_windows; ++w)
        if (windows[w].utterance < 0 || windows[w].utterance >= p.batch || windows[w].keyword < 0 || windows[w].keyword >= p.keywords)
            return refuse(FA_INVALID_ARGUMENT, "window %lld names utterance %d, keyword %d", (long long)w, windows[w].utterance, windows[w].keyword);
    std::vector<Job> jobs;
    std::vector<int32_t> ids;
    std::vector<int64_t> window_of;
    for (int64_t w = 0; w < n_windows; ++w) {
        const fa_kws_window &q = windows[w];
        const int32_t n = p.len(q.keyword), t0 = std::max(0, q.start_frame), t1 = std::min(p.valid[q.utterance], q.end_frame);   // :260-261
        out[w] = fa_kws_detection{q.utterance, q.keyword, -__builtin_huge_valf(), t0, t0};                                    // :263-272
        if (n == 0 || t1 <= t0 || t1 - t0 < n) continue;
        ids.push_back(static_cast<int32_t>(jobs.size()));
        jobs.push_back(Job{q.utterance, q.keyword, t0, t1});
        window_of.push_back(w);
    }
    std::stable_sort(ids.begin(), ids.end(), [&](const int32_t x, const int32_t y) { return jobs[x].utterance < jobs[y].utterance; });
    order_by_class(p, jobs, ids, plan.n_class);
    plan.jobs.resize(ids.size());
    plan.window_of.resize(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) { plan.jobs[i] = jobs[ids[i]]; plan.window_of[i] = window_of[ids[i]]; }
    return Verdict{};
}

// The arena: O(jobs + capacity) records, never less than one job can need, in whole chunks; `forced` (FA_KWS_ARENA, tests) asks for
// another size.  slice: the jobs of a pass after the first, each of which then fits at its worst.
struct Arena {
    int64_t cap, slice;
};
constexpr int64_t kArenaNotForced = -1;
inline Arena arena_of(const int64_t J, const int64_t capacity, const int64_t forced, const int64_t worst_one) {
    int64_t cap = std::max<int64_t>(65536, 2 * J + std::min<int64_t>(capacity, int64_t{1} << 26));
    if (forced != kArenaNotForced) cap = forced;
    cap = std::max(worst_one, (cap + kChunk - 1) / kChunk * kChunk);
    return Arena{cap, std::max<int64_t>(1, cap / worst_one)};
}

// mergeOverlap (:374-391) on one job's candidates, which arrive in the order of their end samples
inline void merge_overlap(std::vector<Record> &c) {
    std::stable_sort(c.begin(), c.end(), [](const Record &x, const Record &y) { return x.start < y.start; });
    size_t m = 0;
    for (size_t i = 0; i < c.size(); ++i) {
        if (m > 0 && c[i].start <= c[m - 1].end) {
            Record best = c[i].score > c[m - 1].score ? c[i] : c[m - 1];
            best.end = std::max(c[m - 1].end, c[i].end);
            c[m - 1] = best;
        } else {
            c[m++] = c[i];
        }
    }
    c.resize(m);
}

// The passes of a spotting call over its arena.  begin(); then, while next(): the device walks pass_jobs (ordered by class, n_class of
// each) and absorb() takes what it wrote.  The vectors are reused from pass to pass.
struct Passes {
    std::vector<int32_t> ids;       // this pass: indices into the call's jobs
    std::vector<Job> pass_jobs;     // this pass: jobs[ids[i]]
    int32_t n_class[3] = {0, 0, 0};
    std::vector<Record> done;       // finished candidates; .job is the index into the call's jobs
    int passes = 0;

    void begin(const Problem &problem, const std::vector<Job> &all, const Arena &a) {
        p = &problem; jobs = &all; arena = a;
        pending.resize(all.size());
        for (size_t i = 0; i < all.size(); ++i) pending[i] = static_cast<int32_t>(i);
        done.clear();
        passes = 0;
    }
    // false: nothing is pending
    bool next() {
        if (pending.empty()) return false;
        const size_t take = passes == 0 ? pending.size() : std::min<size_t>(pending.size(), static_cast<size_t>(arena.slice));
        ids.assign(pending.begin(), pending.begin() + static_cast<ptrdiff_t>(take));
        order_by_class(*p, *jobs, ids, n_class);
        pass_jobs.resize(take);
        for (size_t i = 0; i < take; ++i) pass_jobs[i] = (*jobs)[ids[i]];
        return true;
    }
    // the records to fetch from the head of the arena for a cursor the pass left
    int64_t records(const unsigned long long cursor) const {
        return static_cast<int64_t>(std::min<unsigned long long>(cursor, static_cast<unsigned long long>(arena.cap)));
    }
    // What the pass wrote: status[i] of pass job i (its candidates, or -1 when a chunk did not fit) and recs[0 .. records(cursor)).
    // The finished jobs' candidates go to `done`; the overflowed ones head the next passes, back in utterance order.
    Verdict absorb(const unsigned long long cursor, const int32_t *status, const Record *recs, const bool merge) {
        const size_t take = ids.size();
        const Record *const end = recs + records(cursor);
        // the records of each job, in arena order: a job's chunks were reserved one after the other
        first.assign(take + 1, 0);
        for (const Record *r = recs; r != end; ++r) {
            if (r->job < 0) continue;
            if (static_cast<size_t>(r->job) >= take) return refuse(FA_RUNTIME_ERROR, "a record names job %d of %zu", r->job, take);
            ++first[static_cast<size_t>(r->job) + 1];
        }
        for (size_t i = 0; i < take; ++i) first[i + 1] += first[i];
        sorted.resize(static_cast<size_t>(first[take]));
        at.assign(first.begin(), first.end() - 1);
        for (const Record *r = recs; r != end; ++r)
            if (r->job >= 0) sorted[static_cast<size_t>(at[static_cast<size_t>(r->job)]++)] = *r;
        again.clear();
        for (size_t i = 0; i < take; ++i) {
            if (status[i] < 0) {
                if (passes > 0) return refuse(FA_RUNTIME_ERROR, "a job overflowed an arena sized for it");
                again.push_back(ids[i]);
                continue;
            }
            if (first[i + 1] - first[i] != status[i]) return refuse(FA_RUNTIME_ERROR, "job %zu wrote %lld of %d records", i, (long long)(first[i + 1] - first[i]), status[i]);
            mine.assign(sorted.begin() + first[i], sorted.begin() + first[i + 1]);
            if (merge) merge_overlap(mine);
            for (Record r : mine) { r.job = ids[i]; done.push_back(r); }
        }
        std::sort(again.begin(), again.end());   // back in utterance order
        again.insert(again.end(), pending.begin() + static_cast<ptrdiff_t>(take), pending.end());
        pending.swap(again);
        ++passes;
        return Verdict{};
    }

private:
    const Problem *p = nullptr;
    const std::vector<Job> *jobs = nullptr;
    Arena arena{0, 1};
    std::vector<int32_t> pending, again;
    std::vector<Record> sorted, mine;
    std::vector<int64_t> first, at;
};

// The detections by utterance, then keyword (the job order), then as the reference's array holds them (one pass leaves them by class):
// the count, the counts by utterance (zeroed by the caller), and as many detections as the output holds.
inline Verdict deliver(const std::vector<Job> &jobs, std::vector<Record> &done, fa_kws_detection *dets, const int64_t capacity, int64_t *count, int64_t *utt_counts) {
    std::stable_sort(done.begin(), done.end(), [](const Record &x, const Record &y) { return x.job < y.job; });
    const int64_t total = static_cast<int64_t>(done.size());
    *count = total;
    if (utt_counts) for (const Record &r : done) ++utt_counts[jobs[r.job].utterance];
    if (!dets || total == 0) return Verdict{};
    for (int64_t i = 0, n = std::min(total, capacity); i < n; ++i) dets[i] = fa_kws_detection{jobs[done[i].job].utterance, jobs[done[i].job].keyword, done[i].score, done[i].start, done[i].end};
    if (capacity < total) return refuse(FA_OUTPUT_TOO_SMALL, "output holds %lld of %lld detections", (long long)capacity, (long long)total);
    return Verdict{};
}

}  // namespace kws
}  // namespace fa
