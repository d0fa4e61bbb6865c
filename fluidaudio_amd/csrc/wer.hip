// wer.hip — the kernel of the batched edit distance (entries: wer_host.hip, plan: wer_launch.h), with the reference's insertion /
// deletion / substitution breakdown on the device:
// WERCalculator.editDistance (Sources/FluidAudioCLI/Utils/WERCalculator.swift:178-239), whose total is StringUtils.levenshteinDistance
// (Sources/FluidAudio/Shared/StringUtils.swift:12-40).  Integers only, hence the reference's numbers exactly.
//
// One wavefront walks one pair; rows are the hypothesis, columns the reference text.  A cell carries (dp, sub, del) — the counts of the
// reference's traceback from that cell, carried forward (wer_core.h) — so there is no table and no walk back: O(m + n) memory.  Lane l
// owns a strip of C consecutive columns in registers (C = 1 ... 16 by the reference's length, wer_launch.h) and the rows are walked
// skewed: at step s lane l works on row s - l.  What a lane needs from its left neighbour — the last cell of the neighbour's strip in
// the same row, produced one step earlier, and the row's hypothesis symbol — comes by a DPP wave shift; nothing goes through LDS.  Lane
// 0 is fed from registers: every 64 steps the wavefront loads the next 64 hypothesis symbols (and, past the first panel, the next 64
// cells of the boundary column), one per lane, a block ahead of the steps that read them lane by lane.
// A reference of more than 1024 columns is walked by the same wavefront panel by panel: lane 63 stores its last cell of every row to
// the pair's boundary buffer, the next panel's lane 0 consumes them.  Writer and reader are one wavefront, ordered by a workgroup-scope
// fence between the panels; no wavefront ever waits for another.  Every boundary entry a panel reads was written by the panel before it
// in this call, so the content of the workspace at entry does not matter.
#include "fa_common.h"
#include "wer_core.h"
#include "wer_launch.h"

namespace {

using fa::wer::Job;
using fa::wer::WalkArgs;
using fa::wercore::Cell;
constexpr int kWave = fa::wer::kWave;
constexpr int kWavesPerGroup = fa::wer::kWavesPerGroup;
constexpr int kThreads = kWavesPerGroup * kWave;
constexpr int kWaveShr1 = 0x138;   // DPP wave_shr:1: lane l reads lane l - 1, lane 0 keeps `fill`

__device__ inline int32_t below(const int32_t v, const int32_t fill) { return __builtin_amdgcn_update_dpp(fill, v, kWaveShr1, 0xf, 0xf, false); }
__device__ inline Cell below(const Cell v, const Cell fill) { return Cell{below(v.dp, fill.dp), below(v.sub, fill.sub), below(v.del, fill.del)}; }
__device__ inline int32_t lane_value(const int32_t v, const int t) { return __builtin_amdgcn_readlane(v, t); }   // t is wave-uniform

template <int C>
__global__ __launch_bounds__(kThreads) void wer_walk(const WalkArgs a) {
    const int lane = threadIdx.x % kWave;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kWavesPerGroup + threadIdx.x / kWave;
    if (j >= a.n_jobs) return;   // wave-uniform; the kernel has no barrier
    const Job job = a.jobs[j];
    const int32_t *hyp = a.hyp + job.hyp_off, *ref = a.ref + job.ref_off;
    const uint32_t m = static_cast<uint32_t>(job.m);
    int32_t *ws = a.ws + job.ws_off;
    Cell strip[C];

    for (int32_t p = 0; p < job.panels; ++p) {
        const bool first = p == 0, last = p == job.panels - 1;
        const int64_t col0 = (static_cast<int64_t>(p) * kWave + lane) * C;   // the columns left of the strip; columns past n are walked and never looked at
        int32_t sym[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            sym[c] = col0 + c < job.n ? ref[col0 + c] : 0;
            strip[c] = fa::wercore::row_zero(static_cast<int32_t>(col0 + c + 1));
        }
        Cell diag = fa::wercore::row_zero(static_cast<int32_t>(col0));
        const int32_t *rd = ws + fa::wer::boundary_at(job.m, (p - 1) & 1, 0);
        int32_t *wr = ws + fa::wer::boundary_at(job.m, p & 1, 0);
        const uint32_t steps = fa::wer::steps_of(job.m, job.n, C, last);

        // rows r0 + lane of the hypothesis and of the boundary column left of this panel; agent-scope loads: served by L2, where the
        // panel before left them
        const auto load = [&](const uint32_t r0, int32_t &tok, Cell &bnd) {
            const uint32_t r = r0 + lane;
            tok = r < m ? hyp[r] : 0;
            bnd = Cell{0, 0, 0};
            if (!first && r < m) {
                bnd.dp = __hip_atomic_load(rd + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bnd.sub = __hip_atomic_load(rd + m + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bnd.del = __hip_atomic_load(rd + 2 * static_cast<int64_t>(m) + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        int32_t tok_blk, tok_next, tok = 0;
        Cell bnd_blk, bnd_next;
        load(0, tok_next, bnd_next);
        for (uint32_t s0 = 0; s0 < steps; s0 += kWave) {
            tok_blk = tok_next;
            bnd_blk = bnd_next;
            load(s0 + kWave, tok_next, bnd_next);
            const int t_end = static_cast<int>(min(static_cast<uint32_t>(kWave), steps - s0));
            for (int t = 0; t < t_end; ++t) {
                const uint32_t s = s0 + t;   // lane 0's row
                const Cell feed = first ? fa::wercore::col_zero(static_cast<int32_t>(s + 1))
                                        : Cell{lane_value(bnd_blk.dp, t), lane_value(bnd_blk.sub, t), lane_value(bnd_blk.del, t)};
                tok = below(tok, lane_value(tok_blk, t));
                const Cell left = below(strip[C - 1], feed);
                const uint32_t r = s - lane;   // wraps to a large value before the lane's first row
                if (r < m) {
                    fa::wercore::strip_row<C>(strip, sym, tok, diag, left);
                    diag = left;
                    if (!last && lane == kWave - 1) {
                        wr[r] = strip[C - 1].dp;
                        wr[m + r] = strip[C - 1].sub;
                        wr[2 * static_cast<int64_t>(m) + r] = strip[C - 1].del;
                    }
                }
            }
        }
        // lane 63's stores of this panel are performed before the loads of the next one are issued
        if (!last) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }

    Cell res = strip[0];
    const int slot = fa::wer::last_slot(job.n, C);
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (c == slot) res = strip[c];
    if (lane == fa::wer::last_lane(job.n, C)) {
        int32_t *o = a.out + 4 * j;
        o[0] = res.dp;
        o[1] = res.dp - res.sub - res.del;
        o[2] = res.del;
        o[3] = res.sub;
    }
}

}  // namespace

void fa::wer::launch_walk(hipStream_t stream, const WalkArgs &a, const int cls) {
    if (a.n_jobs <= 0) return;
    const dim3 grid(fa::grid_for(a.n_jobs, kWavesPerGroup)), block(kThreads);
    switch (cls) {
    case 0: hipLaunchKernelGGL(wer_walk<1>, grid, block, 0, stream, a); break;
    case 1: hipLaunchKernelGGL(wer_walk<2>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(wer_walk<4>, grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(wer_walk<8>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(wer_walk<16>, grid, block, 0, stream, a); break;
    }
}
