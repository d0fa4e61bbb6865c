// ahc_route.h — the decisions of the linkage's host side that need no device, as plain C++ (no HIP types: tests/cpu/ahc_route.cpp walks them on the
// CPU): slots per thread, padded sizes, which build of the round serves a problem or a batch, rounds per replay and the replay budget, and the route the
// batch dispatcher takes.  A switch arrives parsed (ahc_launch.h: sw_int); the .hip units hold no copy of a threshold.  Part of ahc_ws.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/fluidaudio_hip.h"

namespace fa_ahc {

#ifndef FA_AHC_BLK
#define FA_AHC_BLK 256
#endif
constexpr int kBlk = FA_AHC_BLK;   // rows per block record == threads per round workgroup (512 measured: see profiles/r03_ahc_variants.txt)
constexpr int kMaxBlocks = 768;    // N <= 196 608 (N^2 * 8 B = 288 GB is reached at N ~ 190 000)
#ifndef FA_AHC_ROUNDS_PER_GRAPH
#define FA_AHC_ROUNDS_PER_GRAPH 512
#endif
constexpr int kRoundsPerGraph = FA_AHC_ROUNDS_PER_GRAPH;  // multiple of 4 (counter rotation) and of 2 (parity)

namespace route {

constexpr int kLaneRecords = 4;           // block records a lane of the first reduction holds at most: 4 x 64 blocks of one slot per thread = 65 536 points
constexpr int kInFlightMax = 4;           // chains in flight: at most this many problems ...
constexpr size_t kInFlightMinN = 16384;   // ... of at least this many points each
constexpr size_t kUniGroupsMinN = 4096;   // uniform batches side by side: the smallest problem of eight

inline bool valid_cpt(const int v) { return v == 1 || v == 2 || v == 4; }
inline size_t padded(const size_t N, const int cpt) { const size_t cols = static_cast<size_t>(kBlk) * cpt; return (N + cols - 1) / cols * cols; }
inline size_t blocks(const size_t N, const int cpt) { return padded(N, cpt) / (static_cast<size_t>(kBlk) * cpt); }
inline bool fits_matrix(const size_t N) { return blocks(N, 1) <= static_cast<size_t>(kMaxBlocks); }   // else: the matrix-free route

// slots per thread of the round: 1 for a chain of its own (the fewest dependent instructions per round: 5.09 us at 43 200 points against 5.60 / 6.69 with
// 2 / 4); 2 where that makes the problem ONE block (257 .. 512 points: all rounds of a replay inside one launch, no kernel boundary between them:
// 400 points 2.35 -> 2.08 ms per call; four slots per thread for <= 1 024 points lose to the multi-block chain, 5.0 against 4.9 ms at 900).
// FA_AHC_CPT forces a value (measurements: profiles/r05_cpt_probe_v2.json).
inline int single_cpt(const int forced, const bool no_single_block, const size_t N) {
    if (valid_cpt(forced)) return forced;
    return no_single_block || N <= static_cast<size_t>(kBlk) || N > 2 * static_cast<size_t>(kBlk) ? 1 : 2;
}

// rounds per replay for a problem of n points: one replay should finish a small problem (one round per merge + a few re-scans /
// window rounds) without hundreds of idle rounds behind it — at n = 50 the fixed 512-round graph cost 2.7 ms per call, five times the
// reference on a host core; large problems use the full length.  Multiple of 4 (counter rotation and parity).
inline int rounds_for(const size_t n) {
    const size_t want = n + n / 8 + 8;
    const size_t r = want < static_cast<size_t>(kRoundsPerGraph) ? want : static_cast<size_t>(kRoundsPerGraph);
    return static_cast<int>((r + 3) & ~static_cast<size_t>(3));
}
// replays a problem of N points may take: a bound on its rounds (merges + re-scans + windows)
inline long long replay_budget(const size_t N) { return 64 + 8 * static_cast<long long>(N) / rounds_for(N); }

// ---- the plan of the drive loop (ahc_launch.h: drive_rounds): how long the next replay is and whether it may be enqueued before the state of the
// replays in flight has been read.
// The ladder: a problem whose replay has the full length also keeps shorter ones, so that the last replays do not run hundreds of launches behind `done`
// (a launch behind `done` still crosses a kernel boundary and reduces every block record: ~4 us each, 352 of them per 8 h recording with one length).
// Each length is a multiple of 4 (counter rotation and parity).
constexpr int kRungs = 3;
constexpr int kLadder[kRungs] = {kRoundsPerGraph, 128, 32};
constexpr int kQueueDepth = 2;   // replays in flight at most
static_assert(kRoundsPerGraph % 4 == 0 && kLadder[1] % 4 == 0 && kLadder[2] % 4 == 0 && kLadder[1] < kRoundsPerGraph, "replay lengths: multiples of 4, descending");
struct DrivePlan {
    long long left = 0;         // merges still to do by the last state the host has read (N - 1 - step); meaningful for one problem only
    int per_round = 1;          // merges a round commits at most: 2 with the speculative round, 1 otherwise
    int full = kRoundsPerGraph; // rounds_for(N): the one length of the synchronous drive
    int depth = 1;              // replays in flight at most (1: the synchronous drive, every state is read before the next replay is enqueued)
    bool ladder = false;        // lengths from kLadder; otherwise always `full`
    long long budget = 0;       // rounds the loop may enqueue: replay_budget(N) replays of `full` rounds
    long long spent = 0;        // rounds enqueued so far
    int in_flight[kQueueDepth] = {0, 0};   // rounds of the replays whose state has not been read, oldest first
    int queued = 0;
};
inline int rungs_for(const size_t N) { return rounds_for(N) == kRoundsPerGraph && kLadder[0] == kRoundsPerGraph ? kRungs : 1; }   // small problems keep their single length
// one problem of N points with `step` merges done; synchronous: FA_AHC_SYNC_DRIVE (one replay of rounds_for(N) at a time, as before the look-ahead)
inline DrivePlan drive_plan(const size_t N, const long long step, const bool spec, const bool synchronous) {
    DrivePlan p;
    p.left = static_cast<long long>(N) - 1 - step;
    p.per_round = spec ? 2 : 1;
    p.full = rounds_for(N);
    p.depth = synchronous ? 1 : kQueueDepth;
    p.ladder = !synchronous && rungs_for(N) > 1;
    p.budget = replay_budget(N) * p.full;
    return p;
}
// a batch: `budget` replays of one length, each state read before the next replay (its callers may capture their graph again between two replays)
inline DrivePlan drive_plan_batch(const int full, const long long budget) {
    DrivePlan p;
    p.full = full;
    p.budget = budget * full;
    return p;
}
// merges that are certainly left when everything in flight has run: a round commits at most per_round merges
inline long long plan_floor(const DrivePlan &p) {
    long long rounds = 0;
    for (int i = 0; i < p.queued; ++i) rounds += p.in_flight[i];
    return p.left - p.per_round * rounds;
}
// Rounds of the replay to enqueue now, 0: none before the oldest state in flight has been read (or the budget is spent).  A replay goes behind others only
// while those cannot finish the problem (plan_floor > 0): the synchronous drive would have enqueued it as well.  Its length is the longest rung the merges
// certainly left fill even at per_round merges a round, the shortest rung when none does.
inline int plan_next(DrivePlan &p) {
    if (p.queued >= p.depth || p.queued >= kQueueDepth) return 0;
    const long long floor = plan_floor(p);
    if (p.queued > 0 && floor <= 0) return 0;
    int len = p.full;
    if (p.ladder) {
        len = kLadder[kRungs - 1];
        for (int r = 0; r < kRungs; ++r) if (static_cast<long long>(p.per_round) * kLadder[r] <= floor) { len = kLadder[r]; break; }
    }
    if (p.spent + len > p.budget) return 0;
    p.in_flight[p.queued++] = len;
    p.spent += len;
    return len;
}
// the state of the oldest replay in flight has been read: `left` merges were still to do behind it
inline void plan_retire(DrivePlan &p, const long long left) {
    for (int i = 1; i < p.queued; ++i) p.in_flight[i - 1] = p.in_flight[i];
    if (p.queued > 0) p.in_flight[--p.queued] = 0;
    p.left = left;
}

// ---- one problem: which of the 13 builds of ahc_round_t<false, ...> (the table in ahc_rounds.hip is in this order)
enum SingleKernel { kSpecK1, kSpecK2, kSpecK3, kSpecK4, kC4Big, kC4, kC2Big, kC2, kC1Big, kC1K1, kC1K2, kC1K3, kC1K4, kSingleKernels };
struct RoundForm {
    bool big;    // more than 65 536 points (four block records per lane at one slot per thread): the kernel with the many-record reduction
    int kc;      // records a lane of the first reduction owns: the one-slot-per-thread kernel exists per count (ahc_round_body: a request for a record the
                 // lane does not own is not free); the forms with 2 / 4 slots per thread hold all 2 / 1 of theirs
    bool spec;   // the speculative round (two merges per launch where the next merge was foreseen): one slot per thread, the register path of the first
                 // reduction, AUTO, even d <= 256 (the centroid pairs of one lane hold the whole centroid); FA_AHC_SPEC=0 keeps the one-merge round
    SingleKernel kernel;
};
inline RoundForm single_form(const int cpt, const int nblk, const int mode, const size_t d, const bool spec_on) {
    RoundForm f{};
    f.big = nblk > (kLaneRecords / cpt) * 64;
    f.kc = cpt == 1 && !f.big ? std::max(1, (nblk + 63) / 64) : kLaneRecords / cpt;
    f.spec = spec_on && cpt == 1 && !f.big && mode == FA_AHC_MODE_AUTO && d % 2 == 0 && d <= 256;
    if (cpt == 1 && !f.big) f.kernel = static_cast<SingleKernel>((f.spec ? kSpecK1 : kC1K1) + std::min(f.kc, kLaneRecords) - 1);
    else f.kernel = cpt == 4 ? (f.big ? kC4Big : kC4) : cpt == 2 ? (f.big ? kC2Big : kC2) : kC1Big;
    return f;
}

// ---- uniform batches
// Eligible: >= 2 problems of >= 2 points, no reference-order mode, the smallest padded size at least half the largest (a smaller problem only pays dead
// padding slots: start-up and HBM of the larger layout).
inline bool uniform_eligible(const int count, const size_t *n, const int mode, const bool no_uniform) {
    if (count < 2 || mode == FA_AHC_MODE_REFERENCE_ORDER || no_uniform) return false;
    size_t lo = SIZE_MAX, hi = 0;
    for (int k = 0; k < count; ++k) {
        if (n[k] < 2) return false;
        const size_t np = padded(n[k], 1);
        lo = std::min(lo, np); hi = std::max(hi, np);
    }
    return hi / kBlk >= 2 && lo * 2 >= hi && hi / kBlk <= kLaneRecords * 64;   // one-block problems keep their single-launch form; > 65 536 points: the many-record kernels
}
// Slots per thread of the round that serves a uniform batch of `count` problems of up to Nmax points (ahc_round_body's CPT): a launch over several problems
// is bound by instruction issue, and a thread that owns four slots leaves a quarter of the workgroups, wavefronts and block records per problem; small
// problems keep enough blocks to spread over.  FA_AHC_UNI_CPT forces 1 / 2 / 4.
// Measured (profiles/r05_cpt_probe_v2.json, us per round of 43 200-point problems, one batch): K = 2: 5.80 / 5.93 / 6.83 with 1 / 2 / 4 slots per thread,
// K = 4: 6.89 / 6.66 / 7.15, K = 8: 10.83 / 7.93 / 8.49, K = 12: 13.41 / 10.00 / 9.80; two batches side by side, K = 8: 8.82 / 7.59 / 8.12, K = 12: 11.17 /
// 8.18 / 8.90; 16 x 5 400: 6.74 / 6.88 / 7.90.  Two slots per thread pay once a launch holds more than ~2 workgroups per CU at one slot per thread.
// (Three batches side by side instead of two, profiles/r05_groups_probe.txt: K = 8: 145 -> 152 audio-hours/s linkage-only, K = 12: 187 -> 180: not adopted.)
inline int uniform_cpt(const int forced, const int count, const size_t Nmax) {
    if (valid_cpt(forced)) return forced;
    const size_t wgs1 = static_cast<size_t>(count) * blocks(Nmax, 1);
    return wgs1 >= 450 && Nmax >= 1024 ? 2 : 1;   // (three 8 h recordings: a batch of K = 6 splits into two of three that run side by side: 1 014 workgroups at one slot per thread)
}
// uniform batches side by side a dispatch of `count` problems uses; FA_AHC_UNI_GROUPS = 1 .. 4 overrides the choice (1: one batch)
inline int uniform_groups(const int count, const size_t *n, const int forced) {
    if (forced >= 1 && forced <= 4) return std::min(forced, count / 2 > 0 ? count / 2 : 1);
    size_t lo = SIZE_MAX;
    for (int k = 0; k < count; ++k) lo = std::min(lo, n[k]);
    // six long recordings, or eight medium ones (chains of >= 4 096 rounds: the second stream's thread + graph capture, ~2 ms, must be worth it)
    return (count >= 6 && lo >= kInFlightMinN) || (count >= 8 && lo >= kUniGroupsMinN) ? 2 : 1;
}
// Which of the nine ahc_round_uni* kernels (the table in ahc_batch.hip is in this order).  Co-residency: 256 CUs x 4 SIMDs x (waves per SIMD) / 4 waves
// per workgroup.  The round without the many-record path needs 94 VGPRs: 5 waves per SIMD = 1 280 resident workgroups (7 recordings of 8 h).  Capped at
// 80 / 64 VGPRs (52 / 120 bytes of scratch): 1 536 / 2 048.  FA_AHC_UNI_WAVES = 5 | 6 | 8 picks one (measurements: profiles/r04_uni_probe.json); the
// default budget has a build per count of block records a lane of the first reduction owns.
enum UniKernel { kUni, kUniW3, kUniW4, kUniC2, kUniC4, kUniK1, kUniK2, kUniK3, kUniC2K1, kUniKernels };
inline UniKernel uniform_kernel(const int cpt, const int nblk, const int waves) {
    const int lane_recs = (nblk + 63) / 64;
    if (cpt == 4) return kUniC4;
    if (cpt == 2) return lane_recs == 1 ? kUniC2K1 : kUniC2;
    if (waves == 8) return kUniW4;
    if (waves == 6) return kUniW3;
    return lane_recs == 1 ? kUniK1 : lane_recs == 2 ? kUniK2 : lane_recs == 3 ? kUniK3 : kUni;
}

// ---- the batch dispatcher (ahc_batch_host.hip: run_device_batch_impl), count >= 1
enum class Route {
    kOversize,   // a problem the matrix-based rounds cannot hold (N > 196 608) runs alone through the single-problem entry; the others stay a batch
    kGroups,     // uniform batches side by side, on the caller's context and its helpers
    kInFlight,   // a few large problems as chains of their own, one context each (only on request: FA_AHC_IN_FLIGHT)
    kUniform,    // one uniform-layout batch
    kBlockMap    // the block map / argument kernels; the reference-order mode: one problem after the other
};
struct BatchRoute { Route route; int groups; };
inline BatchRoute batch_route(const int count, const size_t *n, const int mode, const bool allow_groups, const bool capped, const bool in_flight_on,
                              const int forced_groups, const bool no_uniform) {
    if (count > 1 && mode != FA_AHC_MODE_REFERENCE_ORDER)
        for (int k = 0; k < count; ++k) if (!fits_matrix(n[k]) && n[k] >= 2) return {Route::kOversize, 1};
    const bool uniform = uniform_eligible(count, n, mode, no_uniform);
    if (allow_groups && uniform && !capped) {   // a capped context keeps its promise: ONE workspace within the cap
        const int groups = uniform_groups(count, n, forced_groups);
        if (groups > 1) return {Route::kGroups, groups};
    }
    bool large = count >= 2 && count <= kInFlightMax && in_flight_on;
    for (int k = 0; k < count && large; ++k) large = n[k] >= kInFlightMinN;
    if (large) return {Route::kInFlight, 1};
    return {uniform ? Route::kUniform : Route::kBlockMap, 1};
}

}  // namespace route
}  // namespace fa_ahc
