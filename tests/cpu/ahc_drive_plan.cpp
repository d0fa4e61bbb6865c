// The plan of the linkage's drive loop (fluidaudio_amd/csrc/ahc_route.h: drive_plan, plan_next, plan_retire — what ahc_launch.h's drive_rounds asks before
// every replay) walked against a model device, over stdin: one command per line.
// Test infrastructure: built by tests/test_ahc_drive_plan.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
// The model: replays run in the order they were enqueued; a round of a replay commits `rate` merges (0: no progress at all, 1, 2; 3: `per_round` merges
// until fewer than 64 are left, none from then on) until N - 1 are done.  The host is drive_rounds: it enqueues while plan_next hands out a length, then
// reads the oldest state, and stops enqueueing once a state it has read says done.
//   walk N spec sync rate          -> "replays rounds max_depth queued_behind_finishable started_behind_done bad_length done : length..."
//   sweep lo hi stride spec sync rate -> the same counters summed / maxed over N = lo, lo + stride, ... <= hi, then "over_rounds over_replays not_done not_sync over_stall"
//                                        (over_stall: walks of more than replay_budget(N) x rounds_for(N) / 32 replays, the worst case of a device that stalls)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/ahc_route.h"

using namespace fa_ahc;

struct Walk {
    long long replays = 0, rounds = 0, queued_behind_finishable = 0, started_behind_done = 0, bad_length = 0;
    int max_depth = 0;
    bool done = false;
    std::vector<int> lengths;
};

static Walk walk(const size_t N, const bool spec, const bool sync, const int rate) {
    Walk w;
    route::DrivePlan plan = route::drive_plan(N, 0, spec, sync);
    const long long total = static_cast<long long>(N) - 1, per_round = spec ? 2 : 1;
    long long dev_step = 0;              // merges the model device has done behind the last replay it ran
    long long read_step = 0;             // ... by the last state the host has read
    struct Flying { int rounds; long long step_after; };
    std::vector<Flying> fly;             // enqueued, state not read (the device has run them already: the model is infinitely fast, the worst case for a look-ahead)
    bool active = total > 0;
    if (!active) w.done = true;
    for (;;) {
        while (active) {
            const int len = route::plan_next(plan);
            if (!len) break;
            long long in_flight = 0;
            for (const Flying &f : fly) in_flight += f.rounds;
            if (!fly.empty() && total - read_step - per_round * in_flight <= 0) ++w.queued_behind_finishable;   // the issue's bound, kept by the walk itself
            if (dev_step >= total) ++w.started_behind_done;     // the synchronous drive would have read `done` and not enqueued this one
            if (len % 4 != 0 || len <= 0) ++w.bad_length;
            long long r = rate == 3 ? (total - dev_step >= 64 ? per_round : 0) : rate;
            if (r > per_round) r = per_round;
            dev_step += r * len;
            if (dev_step > total) dev_step = total;
            fly.push_back({len, dev_step});
            if (static_cast<int>(fly.size()) > w.max_depth) w.max_depth = static_cast<int>(fly.size());
            ++w.replays;
            w.rounds += len;
            w.lengths.push_back(len);
        }
        if (fly.empty()) break;
        read_step = fly.front().step_after;
        fly.erase(fly.begin());
        if (read_step >= total) { active = false; w.done = true; }
        route::plan_retire(plan, total - read_step);
    }
    return w;
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        size_t N, lo, hi, stride;
        int spec, sync, rate;
        if (!strcmp(cmd, "walk")) {
            if (scanf("%zu %d %d %d", &N, &spec, &sync, &rate) != 4) return 2;
            const Walk w = walk(N, spec != 0, sync != 0, rate);
            printf("%lld %lld %d %lld %lld %lld %d :", w.replays, w.rounds, w.max_depth, w.queued_behind_finishable, w.started_behind_done, w.bad_length, w.done ? 1 : 0);
            for (const int l : w.lengths) printf(" %d", l);
            printf("\n");
        } else if (!strcmp(cmd, "sweep")) {
            if (scanf("%zu %zu %zu %d %d %d", &lo, &hi, &stride, &spec, &sync, &rate) != 6 || stride == 0) return 2;
            Walk sum;
            long long over_rounds = 0, over_replays = 0, not_done = 0, not_sync = 0, over_stall = 0;
            for (N = lo; N <= hi; N += stride) {
                const Walk w = walk(N, spec != 0, sync != 0, rate);
                sum.replays += w.replays; sum.rounds += w.rounds; sum.queued_behind_finishable += w.queued_behind_finishable;
                sum.started_behind_done += w.started_behind_done; sum.bad_length += w.bad_length;
                if (w.max_depth > sum.max_depth) sum.max_depth = w.max_depth;
                const long long full = route::rounds_for(N), budget = route::replay_budget(N);
                if (w.rounds > budget * full) ++over_rounds;
                if (w.replays > budget) ++over_replays;
                if (w.replays > budget * full / route::kLadder[route::kRungs - 1] && w.replays > budget) ++over_stall;
                if (!w.done) ++not_done;
                bool one_length = w.max_depth <= 1;   // the synchronous drive: one replay of rounds_for(N) at a time
                for (const int l : w.lengths) one_length = one_length && l == full;
                if (!one_length) ++not_sync;
            }
            printf("%lld %lld %d %lld %lld %lld %lld %lld %lld %lld %lld\n", sum.replays, sum.rounds, sum.max_depth, sum.queued_behind_finishable, sum.started_behind_done,
                   sum.bad_length, over_rounds, over_replays, not_done, not_sync, over_stall);
        } else {
            return 2;
        }
    }
    return 0;
}
