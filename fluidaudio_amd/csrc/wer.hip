// wer.hip — batched edit distance with the reference's insertion / deletion / substitution breakdown on the device:
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
using fa::wercore::Cell;
constexpr int kWave = fa::wer::kWave;
constexpr int kWavesPerGroup = fa::wer::kWavesPerGroup;
constexpr int kThreads = kWavesPerGroup * kWave;
constexpr int kWaveShr1 = 0x138;   // DPP wave_shr:1: lane l reads lane l - 1, lane 0 keeps `fill`

struct WalkArgs {
    const int32_t *hyp, *ref;
    const Job *jobs;
    int32_t n_jobs;
    int32_t *ws;       // boundary buffers
    int32_t *out;      // [n_jobs][4]: total, insertions, deletions, substitutions
};

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

void launch_walk(hipStream_t stream, const WalkArgs &a, const int cls) {
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

fa_status edit_distance(fa_ctx *ctx, const int32_t *hyp, const int64_t *hyp_range, const int32_t *ref, const int64_t *ref_range, const int64_t n_pairs,
                        fa_edit_counts *out, const bool device) {
    if (n_pairs < 0 || (n_pairs > 0 && (!hyp_range || !ref_range || !out))) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "edit_distance: bad arguments");
    if (n_pairs >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "edit_distance: 2^31 - 1 pairs or more");
    if (n_pairs > 0) {
        const fa::wer::Verdict v = fa::wer::check_ranges(hyp, hyp_range, ref, ref_range, n_pairs);
        if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "edit_distance: %s (pair %lld)", v.what, (long long)v.pair);
    }
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_pairs == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "edit_distance", [&]() -> fa_status {
    // the host-pointer entry uploads from the first symbol used on
    const int64_t h0 = device ? 0 : hyp_range[0], r0 = device ? 0 : ref_range[0];
    fa::wer::Plan plan;
    fa::wer::make_plan(hyp_range, ref_range, n_pairs, h0, r0, out, plan);
    const size_t J = plan.jobs.size();
    if (J == 0) return FA_SUCCESS;   // every pair has an empty side

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_hyp, b_ref, b_jobs, b_out, b_ws;
    const size_t hyp_bytes = device ? 0 : sizeof(int32_t) * static_cast<size_t>(hyp_range[n_pairs] - h0);
    const size_t ref_bytes = device ? 0 : sizeof(int32_t) * static_cast<size_t>(ref_range[n_pairs] - r0);
    auto alloc = [&](fa::DevBuf &b, size_t bytes) { return b.alloc(ctx, bytes) == hipSuccess; };
    if (!alloc(b_hyp, hyp_bytes) || !alloc(b_ref, ref_bytes) || !alloc(b_jobs, sizeof(Job) * J) || !alloc(b_out, sizeof(int32_t) * 4 * J) ||
        !alloc(b_ws, sizeof(int32_t) * static_cast<size_t>(plan.ws_ints))) {
        (void)hipGetLastError();
        return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "edit_distance: device allocation failed");
    }
    if (!device) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(b_hyp.p, hyp + h0, hyp_bytes, hipMemcpyHostToDevice, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(b_ref.p, ref + r0, ref_bytes, hipMemcpyHostToDevice, st));
    }
    FA_HIP_TRY(ctx, hipMemcpyAsync(b_jobs.p, plan.jobs.data(), sizeof(Job) * J, hipMemcpyHostToDevice, st));
    WalkArgs a{device ? hyp : b_hyp.as<int32_t>(), device ? ref : b_ref.as<int32_t>(), nullptr, 0, b_ws.as<int32_t>(), nullptr};
    if (ctx->timing) FA_HIP_TRY(ctx, hipEventRecord(ctx->tim_ev[0], st));
    size_t base = 0;
    for (int c = 0; c < fa::wer::kClasses; ++c) {   // one launch per class that has pairs
        a.jobs = b_jobs.as<Job>() + base;
        a.n_jobs = plan.n_class[c];
        a.out = b_out.as<int32_t>() + 4 * base;
        launch_walk(st, a, c);
        base += static_cast<size_t>(plan.n_class[c]);
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    if (ctx->timing) FA_HIP_TRY(ctx, hipEventRecord(ctx->tim_ev[1], st));
    std::vector<int32_t> got(4 * J);
    FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_out.p, sizeof(int32_t) * 4 * J, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    if (ctx->timing) {
        float ms = 0.0f;
        FA_HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->tim_ev[0], ctx->tim_ev[1]));
        ctx->last_device_ms = ms;
    }
    for (size_t i = 0; i < J; ++i) {
        fa_edit_counts &o = out[plan.jobs[i].pair];
        o.total = got[4 * i + 0];
        o.insertions = got[4 * i + 1];
        o.deletions = got[4 * i + 2];
        o.substitutions = got[4 * i + 3];
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

fa_status fa_edit_distance_batch(fa_ctx *ctx, const int32_t *hyp, const int64_t *hyp_range, const int32_t *ref, const int64_t *ref_range, int64_t n_pairs,
                                 fa_edit_counts *out) {
    return edit_distance(ctx, hyp, hyp_range, ref, ref_range, n_pairs, out, false);
}

fa_status fa_edit_distance_batch_dev(fa_ctx *ctx, const int32_t *d_hyp, const int64_t *hyp_range, const int32_t *d_ref, const int64_t *ref_range,
                                     int64_t n_pairs, fa_edit_counts *out) {
    return edit_distance(ctx, d_hyp, hyp_range, d_ref, ref_range, n_pairs, out, true);
}

}  // extern "C"
