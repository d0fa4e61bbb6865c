// kws.hip — the CTC word-spotting dynamic program on the device: CtcDPAlgorithm.fillDPTable with the scans of ctcWordSpotMultiple and
// ctcWordSpotConstrained behind it (Sources/FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/WordSpotting/CtcDPAlgorithm.swift:
// 121-229, 250-300, 311-370; NeMo's ctc_word_spotter.py, arXiv:2406.07096).  fp32 adds, strict compares and one correctly rounded divide
// per sample: scores and frames are the reference's bit for bit (this unit is built with -ffp-contract=off like the other restatements).
//
// One wavefront walks one job (utterance, keyword, frame range).  The lane is the blank-expanded state [B, t1, B, ..., tN, B]: R = 1, 2 or
// 4 consecutive states per lane serve 31, 63 and 127 tokens.  A state's score, start frame and last-token frame live in registers; the
// predecessors s - 1 and s - 2 come from the lane below through DPP wave shifts, nothing goes through LDS.  The emissions of a frame
// depend on (t, symbol) only, not on the DP state: a lane gathers its states' columns of the next kAhead frames while the serial chain
// works on the current ones.  The rows are shared through L2, not staged: the wavefronts of a workgroup and the workgroups next to it in
// the job list walk the same utterance (188 frames x 1025 columns are 0.77 MB of an XCD's 4 MiB), and the list is dealt to the
// workgroups so that neighbours in it share blockIdx % 8, the label of the L2 they are placed on.
//
// The end column (dp, backtrack, lastMatch at n = N) is never stored: the lane of the last blank projects it one step late — the token
// state it needs is the `advance` operand it fetches anyway — and feeds a three-sample window (local maxima), the first strict maximum
// (the fallback, and the constrained variant's answer) and nothing else.  Candidates go to a bounded arena in chunks of kChunk records,
// one integer atomic per chunk; a job whose chunk does not fit says so in its status and is walked again by a later pass (kws_host.hip).
#include <cfloat>

#include "kws_launch.h"

namespace fa {
namespace kws {
namespace {

constexpr int kThreads = kWavesPerGroup * kWave;
constexpr int kWaitVm0 = 0x0F70;   // s_waitcnt vmcnt(0) alone: expcnt and lgkmcnt at their maxima (gfx9 encoding)
constexpr int kWaveShr1 = 0x138;   // DPP wave_shr:1: lane l reads lane l - 1, lane 0 keeps `fill`

__device__ inline int below(const int v, const int fill) { return __builtin_amdgcn_update_dpp(fill, v, kWaveShr1, 0xf, 0xf, false); }
__device__ inline float below(const float v, const float fill) { return __int_as_float(below(__float_as_int(v), __float_as_int(fill))); }

template <int R>
__global__ __launch_bounds__(kThreads) void kws_walk(const WalkArgs a) {
    const int lane = threadIdx.x % kWave;
    const int64_t per = gridDim.x / kXcds;
    const int64_t group = static_cast<int64_t>(blockIdx.x % kXcds) * per + blockIdx.x / kXcds;
    const int64_t j = group * kWavesPerGroup + threadIdx.x / kWave;
    if (j >= a.n_jobs) return;   // wave-uniform; the kernel has no barrier
    const Job job = a.jobs[j];
    const int64_t k0 = a.kw_off[job.keyword];
    const int32_t *tok = a.tokens + k0;
    const int N = static_cast<int>(a.kw_off[job.keyword + 1] - k0);
    const int S = 2 * N + 1, WT = job.t1 - job.t0;
    const float neg = -FLT_MAX;

    // the lane's states: the column each reads (or the constant it emits), whether it is a match state, whether s - 2 may skip onto it
    int col[R];
    float cst[R], sc[R];
    bool match[R], skip[R];
    int st[R], la[R];
    int nf = 0;   // nonWildcardCount (:232-234)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = lane * R + r;
        col[r] = -1; cst[r] = 0.0f; match[r] = false; skip[r] = false;
        bool counted = false;
        if (s < S) {
            if (s & 1) {
                const int32_t id = tok[s >> 1];
                match[r] = true;
                counted = id != FA_KWS_WILDCARD;
                if (id >= 0 && id < a.vocab) col[r] = id;
                else if (id != FA_KWS_WILDCARD) cst[r] = neg;               // :56
                skip[r] = s >= 3 && id != tok[(s >> 1) - 1];                // canSkipBlank (:68-80)
            } else if (a.blank >= 0 && a.blank < a.vocab) {
                col[r] = a.blank;                                           // :54
            }
        }
        nf += __popcll(__ballot(counted));
        sc[r] = s == 0 ? 0.0f : neg;
        st[r] = 0;
        la[r] = 0;
    }
    const float nf_f = nf > 0 ? static_cast<float>(nf) : 1.0f;
    const int lane_end = (S - 1) / R, r_end = (S - 1) % R;   // the last blank, state 2N
    const bool spot = a.constrained == 0;
    const float min_score = spot ? a.kw_min[job.keyword] : 0.0f;

    // what the lane of the last blank keeps of the end column
    float prev_x = neg, cur_x = neg, best_x = neg;
    int cur_s = 0, cur_l = 0, best_s = 0, best_l = 0, ncand = 0;
    int64_t slot = 0, slot_end = 0;
    bool overflow = false;
    const auto emit = [&](const float x, const int s, const int l) {
        if (!overflow && slot == slot_end) {
            const unsigned long long at = atomicAdd(a.cursor, static_cast<unsigned long long>(kChunk));
            if (at + kChunk > static_cast<unsigned long long>(a.arena_cap)) overflow = true;
            else { slot = static_cast<int64_t>(at); slot_end = slot + kChunk; }
        }
        if (!overflow) a.arena[slot++] = Record{a.job_base + static_cast<int32_t>(j), x, s, l};
        // A store left pending beside the emission loads would make every wait in the walk a full drain (the counter orders loads among
        // themselves only).  Draining here, where a candidate is written, keeps the waits of all other steps counted.
        __builtin_amdgcn_s_waitcnt(kWaitVm0);
        ++ncand;
    };

    const float *base = a.lp + static_cast<int64_t>(job.utterance) * a.matrix_stride + static_cast<int64_t>(job.t0) * a.row_stride;
    const auto load = [&](float (&e)[kAhead][R], const int f0) {   // frames f0 ... of the window; past its end the last row again
#pragma unroll
        for (int d = 0; d < kAhead; ++d) {
            const float *row = base + static_cast<int64_t>(min(f0 + d, WT - 1)) * a.row_stride;
#pragma unroll
            for (int r = 0; r < R; ++r) e[d][r] = row[max(col[r], 0)];   // every lane loads (column 0 where the state emits a constant,
                                                                           // chosen in the step): straight-line loads, counted waits
        }
    };

    // Step `it` first looks at time it - 1 (the end column's sample), then moves the states to time it with the emissions of frame it - 1.
    const auto step = [&](const int it, const float (&e)[R]) {
        const float a_sc = below(sc[R - 1], neg);   // state s - 1 of the lane's first state
        const int a_st = below(st[R - 1], 0), a_la = below(la[R - 1], 0);
        constexpr int q = R > 1 ? R - 2 : 0;
        const float b_sc = below(R > 1 ? sc[q] : a_sc, neg);   // state s - 2 of it
        const int b_st = below(R > 1 ? st[q] : a_st, 0), b_la = below(R > 1 ? la[q] : a_la, 0);
        const int u = it - 1;
        if (lane == lane_end && u >= N) {
            float o_sc = sc[0], p_sc = a_sc;
            int o_st = st[0], o_la = la[0], p_st = a_st, p_la = a_la;
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (r == r_end) { o_sc = sc[r]; o_st = st[r]; o_la = la[r]; p_sc = sc[r - 1]; p_st = st[r - 1]; p_la = la[r - 1]; }
            const bool token = p_sc >= o_sc;   // :216
            const float raw = token ? p_sc : o_sc;
            const int ps = token ? p_st : o_st, pl = token ? p_la : o_la;
            const float x = spot ? raw / nf_f : raw;
            if (x > best_x) { best_x = x; best_s = ps; best_l = pl; }   // the first strict maximum (:283-288, :358-364)
            if (spot) {
                if (u > N) {
                    if (cur_x >= prev_x && cur_x > x && cur_x >= min_score) emit(cur_x, cur_s, cur_l);   // sample u - 1 (:345-352)
                    prev_x = cur_x;
                }
                cur_x = x; cur_s = ps; cur_l = pl;
            }
        }
        if (it <= WT) {
#pragma unroll
            for (int r = R - 1; r >= 0; --r) {
                const float s1 = r >= 1 ? sc[r >= 1 ? r - 1 : 0] : a_sc;
                const int t1 = r >= 1 ? st[r >= 1 ? r - 1 : 0] : a_st, l1 = r >= 1 ? la[r >= 1 ? r - 1 : 0] : a_la;
                const float s2 = r >= 2 ? sc[r >= 2 ? r - 2 : 0] : (r == 1 ? a_sc : b_sc);
                const int t2 = r >= 2 ? st[r >= 2 ? r - 2 : 0] : (r == 1 ? a_st : b_st), l2 = r >= 2 ? la[r >= 2 ? r - 2 : 0] : (r == 1 ? a_la : b_la);
                float best = sc[r];
                int bs = st[r], bl = la[r];
                if (s1 > best) { best = s1; bs = t1; bl = l1; }               // state 0 carries it - 1: advancing into state 1 starts there (:191-193)
                if (skip[r] && s2 > best) { best = s2; bs = t2; bl = l2; }
                if (best <= neg / 2) { sc[r] = neg; st[r] = 0; la[r] = 0; }    // :178-181: the row's zeroes, nothing inherited
                else { sc[r] = best + (col[r] >= 0 ? e[r] : cst[r]); st[r] = bs; la[r] = match[r] ? it : bl; }
                if (lane == 0 && r == 0) { sc[r] = 0.0f; st[r] = it; la[r] = 0; }   // the free start (:148-151)
            }
        }
    };
    const auto run = [&](const float (&e)[kAhead][R], const int f0) {
#pragma unroll
        for (int d = 0; d < kAhead; ++d)
            if (f0 + d <= WT) step(f0 + d + 1, e[d]);   // wave-uniform
    };

    float ea[kAhead][R], eb[kAhead][R];
    load(ea, 0);
    for (int f0 = 0; f0 <= WT; f0 += 2 * kAhead) {
        load(eb, f0 + kAhead);
        run(ea, f0);
        load(ea, f0 + 2 * kAhead);
        run(eb, f0 + kAhead);
    }

    if (lane != lane_end) return;
    const int32_t id = a.job_base + static_cast<int32_t>(j);
    if (!spot) {
        a.out[id] = Record{id, nf > 0 ? best_x / static_cast<float>(nf) : best_x, job.t0 + best_s, job.t0 + best_l};   // :290-299
        return;
    }
    if (cur_x >= prev_x && cur_x > neg && cur_x >= min_score) emit(cur_x, cur_s, cur_l);   // the last sample: nothing follows it
    if (ncand == 0 && best_x >= min_score) emit(best_x, best_s, best_l);                   // :355-370
    for (; slot < slot_end; ++slot) a.arena[slot] = Record{-1, 0.0f, 0, 0};
    a.status[id] = overflow ? -1 : ncand;
}

}  // namespace

void launch_walk(hipStream_t stream, const WalkArgs &a, const int states_per_lane) {
    const int64_t groups = (static_cast<int64_t>(a.n_jobs) + kWavesPerGroup - 1) / kWavesPerGroup;
    const dim3 grid(static_cast<unsigned>((groups + kXcds - 1) / kXcds * kXcds)), block(kThreads);
    if (a.n_jobs <= 0) return;
    if (states_per_lane == 1) hipLaunchKernelGGL(kws_walk<1>, grid, block, 0, stream, a);
    else if (states_per_lane == 2) hipLaunchKernelGGL(kws_walk<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(kws_walk<4>, grid, block, 0, stream, a);
}

}  // namespace kws
}  // namespace fa
