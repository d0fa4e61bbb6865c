// tdt_merge_core.h — the TDT long-form seam merge, one recording folded by one wavefront: ChunkProcessor.mergeChunks with tokensMatch,
// tokenIdsMatch, mergeUsingMatches, wordInitialIndex, popSeamWord and mergeByMidpoint (Sources/FluidAudio/ASR/Parakeet/SlidingWindow/
// TDT/ChunkProcessor.swift:952-1219), SequenceMatcher.findLongestCommonSubsequence and findContiguousMatches (Sources/FluidAudio/ASR/
// Parakeet/TokenDeduplication/SequenceMatcher.swift:127-225) and enforceMonotonicTimestamps (ChunkProcessor.swift:843-855), as
// __host__ __device__ code over a wave type W.  tdt_merge.hip instantiates it with the 64 lanes of a wavefront, tests/cpu/
// tdt_merge_emul.cpp with a wave of one lane on the host: the same indices, the same scratch layout, the same staging.
//
// OUT OF SCOPE: collapseSeamWordDuplicates (Unicode strings), repairSeamGaps (needs the networks), the planning of chunk starts and
// the streaming removeDuplicateTokenSequence.
//
// Control flow is uniform over the wave: every value that decides a branch is the same in all lanes.  A lane-strided loop does the
// element work; w.sync() stands between a phase that writes memory and a phase in which other lanes read it.
//
// The merged stream lives in the recording's output slice; its timestamps stay as merged (later seams compare them) and their running
// maximum is kept beside it (runmax): it is the clamp's output, and both the left overlap filter and mergeByMidpoint's firstIndex start
// from a lower bound found on it, so a seam costs O(the part behind that bound), never O(|merged|).  Both time predicates are monotone
// in the timestamp (the product with a positive frame and the sum with it do not decrease), so for every i below the first index
// whose RUNNING MAXIMUM satisfies the predicate the token itself (timestamp <= running maximum) fails it; and at that first index the
// token is the new maximum, so it is mergeByMidpoint's firstIndex exactly.
//
// The fp64 time arithmetic is the reference's own expressions; the units that include this header are built with -ffp-contract=off.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FA_TM_HD __host__ __device__
#else
#define FA_TM_HD
#endif

namespace fa {
namespace tdtmerge {

// a seam's route (include/fluidaudio_hip.h: FA_TDT_MERGE_*): base | tail << 4
constexpr int32_t kEmpty = 0, kConcat = 1, kContiguous = 2, kLcs = 3, kMidpoint = 4;
constexpr int32_t kTailVerbatim = 0, kTailAdoptRight = 1, kTailKeepLeft = 2;
constexpr int32_t kNoSeam = -1;
constexpr int32_t kOk = 0, kTooSmall = 3;   // FA_SUCCESS, FA_OUTPUT_TOO_SMALL

constexpr int kLdsSide = 128;               // overlap sides up to this long keep their scratch in LDS

struct Stream {        // four parallel arrays of tokens
    int32_t *tok, *time, *dur;
    float *conf;
};
struct Tables {
    const uint8_t *safe;      // nullable: spliceSafeTokenIds == nil
    const int32_t *canon;     // nullable: caseVariantIds == nil; -1: no entry
    int32_t vocab;
};
struct Times {
    double frame, overlap;
};

// Scratch of one seam for overlap sides of up to (l_cap, r_cap) tokens.
struct Scratch {
    int32_t *l_idx, *r_idx;          // index in merged / in the window
    long long *l_key, *r_key;        // what tokenIdsMatch compares
    double *l_start, *r_start;       // Double(timestamp) * frame
    int32_t *row0, *row1;            // r_cap + 1 each: two rows of the run / LCS tables, then the matches
    unsigned long long *bits;        // l_cap rows of words_per_row(r_cap): the traceback's dp[i-1][j] > dp[i][j-1]
};
constexpr int64_t words_per_row(const int64_t r) { return (r + 63) / 64; }
// bytes of a Scratch, each array at a multiple of 8
constexpr int64_t scratch_bytes(const int64_t l_cap, const int64_t r_cap) {
    return 8 * ((l_cap + 1) / 2 + (r_cap + 1) / 2) + 16 * (l_cap + r_cap) + 8 * (r_cap + 2) + 8 * l_cap * words_per_row(r_cap);
}
FA_TM_HD inline Scratch carve(unsigned char *p, const int64_t l_cap, const int64_t r_cap) {
    Scratch s;
    s.l_key = reinterpret_cast<long long *>(p); p += 8 * l_cap;
    s.r_key = reinterpret_cast<long long *>(p); p += 8 * r_cap;
    s.l_start = reinterpret_cast<double *>(p); p += 8 * l_cap;
    s.r_start = reinterpret_cast<double *>(p); p += 8 * r_cap;
    s.bits = reinterpret_cast<unsigned long long *>(p); p += 8 * l_cap * words_per_row(r_cap);
    s.l_idx = reinterpret_cast<int32_t *>(p); p += 8 * ((l_cap + 1) / 2);
    s.r_idx = reinterpret_cast<int32_t *>(p); p += 8 * ((r_cap + 1) / 2);
    s.row0 = reinterpret_cast<int32_t *>(p); p += 4 * (r_cap + 1);
    s.row1 = reinterpret_cast<int32_t *>(p);
    return s;
}

FA_TM_HD inline double start_of(const int32_t ts, const double frame) { return static_cast<double>(ts) * frame; }   // startTime(of:) :965-967
FA_TM_HD inline bool is_safe(const Tables &t, const int32_t id) { return id >= 0 && id < t.vocab && t.safe[id] != 0; }
// tokenIdsMatch (:1068-1074) as one comparison: equal ids give equal keys; different ids match only when both have an entry and the
// entries agree
FA_TM_HD inline long long key_of(const Tables &t, const int32_t id) {
    if (t.canon && id >= 0 && id < t.vocab && t.canon[id] >= 0) return (1LL << 40) | static_cast<long long>(t.canon[id]);
    return static_cast<long long>(static_cast<uint32_t>(id));
}
FA_TM_HD inline int32_t imax(const int32_t a, const int32_t b) { return a > b ? a : b; }
FA_TM_HD inline int32_t imin(const int32_t a, const int32_t b) { return a < b ? a : b; }

// tokensMatch (:1053-1064)
FA_TM_HD inline bool cell_match(const long long lk, const double ls, const long long rk, const double rs, const double half) {
    if (lk != rk) return false;
    const double d = ls - rs;
    return (d < 0 ? -d : d) < half;
}

// first index in [0, n) of the non-decreasing runmax whose end time is above thr (strict) / whose start time is at least thr.  The
// answer lies near the end (a seam looks at the last seconds of the merged stream), and every probe of a search in global memory is a
// round trip: the last two strips of the wave are probed with one load per lane each, and only a bound before them is bisected.
template <bool kEnd>
FA_TM_HD inline bool time_ok(const int32_t ts, const double thr, const double frame) {
    const double s = start_of(ts, frame);
    return kEnd ? (s + frame > thr) : (s >= thr);
}
template <bool kEnd, class W>
FA_TM_HD inline int32_t lower_bound(W &w, const int32_t *runmax, const int32_t n, const double thr, const double frame) {
    int32_t hi = n;
    for (int round = 0; round < 2 && hi > 0; ++round) {
        const int32_t i = hi - 1 - w.lane(), valid = imin(W::kLanes, hi);
        const int32_t above = W::count_bits(w.ballot(i >= 0 && time_ok<kEnd>(runmax[i], thr, frame)));   // monotone: the strip's top entries
        if (above < valid) return hi - above;
        hi -= valid;
    }
    int32_t lo = 0;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (time_ok<kEnd>(runmax[mid], thr, frame)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// first index in [from, n) whose token is splice-safe, n when there is none
template <class W>
FA_TM_HD inline int32_t first_safe(W &w, const Tables &t, const int32_t *tok, const int32_t from, const int32_t n) {
    for (int32_t base = from; base < n; base += W::kLanes) {
        const int32_t i = base + w.lane();
        const unsigned long long m = w.ballot(i < n && is_safe(t, tok[i]));
        if (m) return base + W::first_bit(m);
    }
    return n;
}
// last index in [0, at] whose token is splice-safe, -1 when there is none (wordInitialIndex :1157-1168, popSeamWord's scan :1174-1184)
template <class W>
FA_TM_HD inline int32_t last_safe(W &w, const Tables &t, const int32_t *tok, const int32_t at) {
    for (int32_t top = at; top >= 0; top -= W::kLanes) {
        const int32_t i = top - w.lane();
        const unsigned long long m = w.ballot(i >= 0 && is_safe(t, tok[i]));
        if (m) return top - W::first_bit(m);
    }
    return -1;
}

// cur + len tokens fit?  then copy src[from, from + len) behind cur
template <class W>
FA_TM_HD inline bool append(W &w, const Stream &out, int32_t &cur, const int64_t cap, const int32_t *tok, const int32_t *time, const int32_t *dur,
                            const float *conf, const int32_t from, const int32_t len) {
    if (len <= 0) return true;
    if (static_cast<int64_t>(cur) + len > cap) return false;
    for (int32_t x = w.lane(); x < len; x += W::kLanes) {
        out.tok[cur + x] = tok[from + x];
        out.time[cur + x] = time[from + x];
        out.dur[cur + x] = dur[from + x];
        out.conf[cur + x] = conf[from + x];
    }
    cur += len;
    return true;
}

// SequenceMatcher.findContiguousMatches (:188-225): r(i, j) = match ? 1 + r(i + 1, j + 1) : 0 is the run that starts at (i, j); the
// longest wins and, among equals, the first in row-major order.  Rows are walked last to first, lane = right column in strips.
template <class W>
FA_TM_HD inline int32_t best_run(W &w, const Scratch &s, const int32_t nl, const int32_t nr, const double half, int32_t &bi, int32_t &bj) {
    int32_t *prev = s.row0, *cur = s.row1;
    for (int32_t j = w.lane(); j <= nr; j += W::kLanes) prev[j] = 0;
    if (w.lane() == 0) cur[nr] = 0;
    w.sync();
    int32_t blen = 0, mi = 0, mj = 0;
    for (int32_t i = nl - 1; i >= 0; --i) {
        const long long lk = s.l_key[i];
        const double ls = s.l_start[i];
        for (int32_t j = w.lane(); j < nr; j += W::kLanes) {
            const int32_t v = cell_match(lk, ls, s.r_key[j], s.r_start[j], half) ? 1 + prev[j + 1] : 0;
            cur[j] = v;
            if (v > blen || (v == blen && v > 0 && i < mi)) { blen = v; mi = i; mj = j; }   // within a row a lane's columns ascend
        }
        w.sync();
        int32_t *t = prev; prev = cur; cur = t;
    }
    const int32_t best = w.max_i32(blen);
    const long long key = (blen == best && best > 0) ? ((static_cast<long long>(mi) << 32) | static_cast<long long>(mj)) : INT64_MAX;
    const long long first = w.min_i64(key);
    bi = best > 0 ? static_cast<int32_t>(first >> 32) : 0;
    bj = best > 0 ? static_cast<int32_t>(first & 0xffffffffLL) : 0;
    return best;
}

// SequenceMatcher.findLongestCommonSubsequence (:127-172).  Row i of the table is the prefix maximum of cand[j] = match ?
// dp[i-1][j-1] + 1 : dp[i-1][j] (a matched cell is never below its left neighbour: one more row adds at most one to a row's values),
// one wave scan per strip of a row.  The table itself is not kept: one bit per cell says whether the walk back goes up (dp[i-1][j] >
// dp[i][j-1]) where the cell does not match; the match is recomputed.  The matches go to the ends of row0 (left) and row1 (right):
// returns their count K, they are entries [nr - K, nr).
template <class W>
FA_TM_HD inline int32_t lcs(W &w, const Scratch &s, const int32_t nl, const int32_t nr, const double half) {
    int32_t *prev = s.row0, *cur = s.row1;
    const int64_t wpr = words_per_row(nr);
    for (int32_t j = w.lane(); j <= nr; j += W::kLanes) prev[j] = 0;
    if (w.lane() == 0) cur[0] = 0;
    w.sync();
    for (int32_t i = 1; i <= nl; ++i) {
        const long long lk = s.l_key[i - 1];
        const double ls = s.l_start[i - 1];
        int32_t carry = 0;   // dp[i][the column left of the strip]
        for (int32_t base = 0; base < nr; base += W::kLanes) {
            const int32_t j = base + w.lane() + 1;
            const bool valid = j <= nr;
            int32_t up = 0, cand = 0;
            if (valid) {
                up = prev[j];
                cand = cell_match(lk, ls, s.r_key[j - 1], s.r_start[j - 1], half) ? prev[j - 1] + 1 : up;
            }
            const int32_t incl = w.scan_max_incl(cand);
            const int32_t left = imax(carry, w.shift_up(incl, 0));   // dp[i][j - 1]
            const int32_t here = imax(carry, incl);                  // dp[i][j]
            const unsigned long long m = w.ballot(valid && up > left);
            if (valid) cur[j] = here;
            if (w.lane() == 0) {   // a strip of 64 lanes is one word; narrower waves fill it piece by piece
                unsigned long long *word = s.bits + (i - 1) * wpr + base / 64;
                *word = base % 64 == 0 ? m : (*word | (m << (base % 64)));
            }
            carry = w.bcast(here, W::kLanes - 1);
        }
        w.sync();
        int32_t *t = prev; prev = cur; cur = t;
    }
    // one walk back, the same in every lane; lane 0 writes
    int32_t i = nl, j = nr, pos = nr;
    while (i > 0 && j > 0) {
        if (cell_match(s.l_key[i - 1], s.l_start[i - 1], s.r_key[j - 1], s.r_start[j - 1], half)) {
            --pos;
            if (w.lane() == 0) { s.row0[pos] = i - 1; s.row1[pos] = j - 1; }
            --i; --j;
        } else if ((s.bits[(i - 1) * wpr + (j - 1) / 64] >> ((j - 1) % 64)) & 1ull) {
            --i;
        } else {
            --j;
        }
    }
    w.sync();
    return nr - pos;
}

struct Window {        // one window as the greedy walk left it
    const int32_t *tok, *time, *dur;
    const float *conf;
    int32_t n;
};

struct Fold {          // one recording's state
    Stream out;        // the output slice: merged[0, n)
    int32_t *runmax;   // running maximum of merged's timestamps
    int64_t cap;       // tokens the slice holds
    Stream stage;      // cap tokens: the left suffix a seam still reads while it rewrites the slice
    int32_t n;
};

// mergeByMidpoint (:1186-1219)
template <class W>
FA_TM_HD inline bool by_midpoint(W &w, Fold &f, const Window &r, const Tables &tb, const Times &tm, const double left_end, const double right_start,
                                 int32_t &dirty) {
    const double cutoff = (left_end + right_start) / 2;
    int32_t le = lower_bound<false>(w, f.runmax, f.n, cutoff, tm.frame);
    int32_t rs = r.n;
    for (int32_t base = 0; base < r.n; base += W::kLanes) {
        const int32_t j = base + w.lane();
        const unsigned long long m = w.ballot(j < r.n && start_of(r.time[j], tm.frame) >= cutoff);
        if (m) { rs = base + W::first_bit(m); break; }
    }
    if (tb.safe) {
        if (le > 0) le = first_safe(w, tb, f.out.tok, le, f.n);
        const int32_t scan = first_safe(w, tb, r.tok, rs, r.n);
        if (scan < r.n) rs = scan;
    }
    dirty = le;
    f.n = le;
    return append(w, f.out, f.n, f.cap, r.tok, r.time, r.dur, r.conf, rs, r.n - rs);
}

// mergeUsingMatches (:1076-1153) over the K matches at row0 / row1 [off, off + K) (indices into the overlap sides)
template <class W>
FA_TM_HD inline bool using_matches(W &w, Fold &f, const Window &r, const Tables &tb, const Scratch &s, const int32_t off, const int32_t K, int32_t &tail_route,
                                   int32_t &dirty) {
    for (int32_t k = w.lane(); k < K; k += W::kLanes) {   // to indices in merged and in the window
        s.row0[off + k] = s.l_idx[s.row0[off + k]];
        s.row1[off + k] = s.r_idx[s.row1[off + k]];
    }
    w.sync();
    const int32_t first_left = s.row0[off], old_n = f.n;
    // everything from the first matched left token on is rebuilt in place: what is still read of it is staged first
    for (int32_t x = first_left + w.lane(); x < old_n; x += W::kLanes) {
        f.stage.tok[x - first_left] = f.out.tok[x];
        f.stage.time[x - first_left] = f.out.time[x];
        f.stage.dur[x - first_left] = f.out.dur[x];
        f.stage.conf[x - first_left] = f.out.conf[x];
    }
    w.sync();
    const Stream &g = f.stage;
    int32_t cur = first_left;
    dirty = first_left;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t li = s.row0[off + k], ri = s.row1[off + k];
        if (!append(w, f.out, cur, f.cap, g.tok, g.time, g.dur, g.conf, li - first_left, 1)) return false;
        if (k == K - 1) break;
        const int32_t nli = s.row0[off + k + 1], nri = s.row1[off + k + 1];
        const int32_t gap_left = nli > li + 1 ? nli - li - 1 : 0, gap_right = nri > ri + 1 ? nri - ri - 1 : 0;
        if (gap_right > gap_left) {
            if (!append(w, f.out, cur, f.cap, r.tok, r.time, r.dur, r.conf, ri + 1, gap_right)) return false;
        } else if (!append(w, f.out, cur, f.cap, g.tok, g.time, g.dur, g.conf, li + 1 - first_left, gap_left)) {
            return false;
        }
    }
    const int32_t last_left = s.row0[off + K - 1], last_right = s.row1[off + K - 1];
    tail_route = kTailVerbatim;
    bool ok = true;
    if (last_right + 1 < r.n) {
        if (tb.safe && !is_safe(tb, r.tok[last_right + 1])) {
            w.sync();   // popSeamWord looks at what was just written
            const int32_t word_start = last_safe(w, tb, r.tok, last_right);
            const int32_t cursor = word_start >= 0 ? last_safe(w, tb, f.out.tok, cur - 1) : -1;
            if (cursor >= 0) {   // right heard the seam word from its start
                tail_route = kTailAdoptRight;
                cur = cursor;
                dirty = imin(dirty, cursor);
                ok = append(w, f.out, cur, f.cap, r.tok, r.time, r.dur, r.conf, word_start, r.n - word_start);
            } else {             // left keeps its word; right resumes at its next word-initial piece
                tail_route = kTailKeepLeft;
                const int32_t from = last_left + 1 - first_left, staged = old_n - first_left;
                const int32_t to = first_safe(w, tb, g.tok, from, staged);
                ok = append(w, f.out, cur, f.cap, g.tok, g.time, g.dur, g.conf, from, to - from);
                int32_t resume = first_safe(w, tb, r.tok, last_right + 1, r.n);
                if (resume == r.n) resume = last_right + 1;   // no word-initial piece in the tail: verbatim
                ok = ok && append(w, f.out, cur, f.cap, r.tok, r.time, r.dur, r.conf, resume, r.n - resume);
            }
        } else {
            ok = append(w, f.out, cur, f.cap, r.tok, r.time, r.dur, r.conf, last_right + 1, r.n - last_right - 1);
        }
    }
    f.n = cur;
    return ok;
}

// mergeChunks (:952-1051): merged <- merge(merged, r).  false: the slice ran out.  `small` serves overlap sides up to small_side
// tokens each, `big` any the slice and a window can hold.
template <class W>
FA_TM_HD inline bool seam(W &w, Fold &f, const Window &r, const Tables &tb, const Times &tm, const Scratch &small, const int32_t small_side, const Scratch &big,
                          int32_t &route) {
    int32_t dirty = f.n;
    bool ok = true;
    if (f.n == 0 || r.n == 0) {                              // :958-959
        route = kEmpty;
        ok = append(w, f.out, f.n, f.cap, r.tok, r.time, r.dur, r.conf, 0, r.n);
    } else {
        const double left_end = start_of(f.out.time[f.n - 1], tm.frame) + tm.frame;
        const double right_start = start_of(r.time[0], tm.frame);
        if (left_end <= right_start) {                       // :976-978
            route = kConcat;
            ok = append(w, f.out, f.n, f.cap, r.tok, r.time, r.dur, r.conf, 0, r.n);
        } else {
            const double thr_left = right_start - tm.overlap, thr_right = left_end + tm.overlap, half = tm.overlap / 2;
            const int32_t p = lower_bound<true>(w, f.runmax, f.n, thr_left, tm.frame);
            int32_t nl = 0, nr = 0;
            for (int32_t base = p; base < f.n; base += W::kLanes) {
                const int32_t i = base + w.lane();
                nl += W::count_bits(w.ballot(i < f.n && start_of(f.out.time[i], tm.frame) + tm.frame > thr_left));
            }
            for (int32_t base = 0; base < r.n; base += W::kLanes) {
                const int32_t j = base + w.lane();
                nr += W::count_bits(w.ballot(j < r.n && start_of(r.time[j], tm.frame) < thr_right));
            }
            if (nl < 2 || nr < 2) {                          // :993-997
                route = kMidpoint;
                ok = by_midpoint(w, f, r, tb, tm, left_end, right_start, dirty);
            } else {
                const Scratch &s = (nl <= small_side && nr <= small_side) ? small : big;
                int32_t at = 0;                              // overlapLeft (:980-985), overlapRight (:987-991)
                for (int32_t base = p; base < f.n; base += W::kLanes) {
                    const int32_t i = base + w.lane();
                    const double st = i < f.n ? start_of(f.out.time[i], tm.frame) : 0.0;
                    const bool in = i < f.n && st + tm.frame > thr_left;
                    const unsigned long long m = w.ballot(in);
                    if (in) {
                        const int32_t q = at + w.prefix(m);
                        s.l_idx[q] = i; s.l_key[q] = key_of(tb, f.out.tok[i]); s.l_start[q] = st;
                    }
                    at += W::count_bits(m);
                }
                at = 0;
                for (int32_t base = 0; base < r.n; base += W::kLanes) {
                    const int32_t j = base + w.lane();
                    const double st = j < r.n ? start_of(r.time[j], tm.frame) : 0.0;
                    const bool in = j < r.n && st < thr_right;
                    const unsigned long long m = w.ballot(in);
                    if (in) {
                        const int32_t q = at + w.prefix(m);
                        s.r_idx[q] = j; s.r_key[q] = key_of(tb, r.tok[j]); s.r_start[q] = st;
                    }
                    at += W::count_bits(m);
                }
                w.sync();
                const int32_t minimum = imax(nl / 2, 1);     // :999
                int32_t bi = 0, bj = 0, tail = kTailVerbatim;
                const int32_t run = best_run(w, s, nl, nr, half, bi, bj);
                if (run >= minimum) {                        // :1015-1024
                    for (int32_t k = w.lane(); k < run; k += W::kLanes) { s.row0[k] = bi + k; s.row1[k] = bj + k; }
                    w.sync();
                    ok = using_matches(w, f, r, tb, s, 0, run, tail, dirty);
                    route = kContiguous | (tail << 4);
                } else {
                    const int32_t K = lcs(w, s, nl, nr, half);
                    if (K == 0) {                            // :1033-1037
                        route = kMidpoint;
                        ok = by_midpoint(w, f, r, tb, tm, left_end, right_start, dirty);
                    } else {
                        ok = using_matches(w, f, r, tb, s, nr - K, K, tail, dirty);
                        route = kLcs | (tail << 4);
                    }
                }
            }
        }
    }
    if (!ok) return false;
    // the running maximum from the first rewritten token on
    w.sync();
    int32_t carry = dirty > 0 ? f.runmax[dirty - 1] : INT32_MIN;
    for (int32_t base = dirty; base < f.n; base += W::kLanes) {
        const int32_t i = base + w.lane();
        const int32_t v = imax(carry, w.scan_max_incl(i < f.n ? f.out.time[i] : INT32_MIN));
        if (i < f.n) f.runmax[i] = v;
        carry = w.bcast(v, W::kLanes - 1);
    }
    w.sync();
    return true;
}

// One recording: windows [w_lo, w_hi) of the greedy walk's arrays ([windows][max_out] and a count, min(count, max_out) used), folded
// into f.out; then the clamp.  routes (one per window of the whole call): kNoSeam for the first window and, when the slice runs out,
// for the seam that did not fit and those behind it.  Returns the status; *count: tokens of the merged stream (0 unless kOk).
template <class W>
FA_TM_HD inline int32_t fold_recording(W &w, Fold &f, const Stream &win, const int32_t *counts, const int32_t max_out, const int64_t w_lo, const int64_t w_hi,
                                       const Tables &tb, const Times &tm, const Scratch &small, const int32_t small_side, const Scratch &big, int32_t *routes,
                                       int32_t *count) {
    for (int64_t k = w_lo + w.lane(); k < w_hi; k += W::kLanes) routes[k] = kNoSeam;
    w.sync();
    f.n = 0;
    int32_t status = kOk;
    for (int64_t k = w_lo; k < w_hi; ++k) {
        const int64_t at = k * max_out;
        const Window r{win.tok + at, win.time + at, win.dur + at, win.conf + at, imax(0, imin(counts[k], max_out))};
        int32_t route = kNoSeam;
        if (!seam(w, f, r, tb, tm, small, small_side, big, route)) { status = kTooSmall; break; }
        if (k > w_lo && w.lane() == 0) routes[k] = route;
    }
    if (status != kOk) f.n = 0;
    for (int32_t i = w.lane(); i < f.n; i += W::kLanes) f.out.time[i] = f.runmax[i];   // enforceMonotonicTimestamps (:843-855)
    if (w.lane() == 0) *count = f.n;
    return status;
}

}  // namespace tdtmerge
}  // namespace fa
