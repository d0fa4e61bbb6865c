// tdt_merge.hip — the TDT long-form seam merge on the device: ChunkProcessor's fold of mergeChunks over a recording's windows and
// enforceMonotonicTimestamps (Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/ChunkProcessor.swift:843-855, 952-1219), batched
// over recordings.  The fold is serial by definition, so one wavefront folds one recording, seam after seam (tdt_merge_core.h, where
// the reference's rules and what is out of scope are stated), and a grid of wavefronts strides over the recordings; inside a seam
// the lanes are the tokens of the overlap sides and the columns of the run and LCS tables.
//
// What this file adds to the core is the wavefront: ballots and prefix popcounts for the compaction of the overlap sides, a
// butterfly for the reductions, a Hillis-Steele prefix maximum for a row of the LCS table with the left neighbour by a DPP wave
// shift, and the LDS scratch of a seam whose sides hold up to kLdsSide tokens (longer sides use the slot's workspace).  A workgroup is
// one wavefront and there is no barrier: between a phase that writes and a phase in which other lanes read stands a workgroup-scope
// fence, which orders the wavefront's own LDS and global accesses.
#include "fa_common.h"
#include "tdt_merge_launch.h"

namespace fa {
namespace tdtmerge {
void launch(hipStream_t stream, const Args &a, int32_t slots);
}
}  // namespace fa

namespace {

namespace mg = fa::tdtmerge;
constexpr int kWave = mg::kWave;
constexpr int kWaveShr1 = 0x138;   // DPP wave_shr:1: lane l reads lane l - 1, lane 0 keeps `fill`

struct Wave64 {
    static constexpr int kLanes = kWave;
    int l;
    __device__ int lane() const { return l; }
    __device__ static int first_bit(const unsigned long long m) { return __ffsll(static_cast<long long>(m)) - 1; }
    __device__ static int count_bits(const unsigned long long m) { return __popcll(m); }
    __device__ unsigned long long ballot(const bool p) const { return __ballot(p); }
    __device__ int prefix(const unsigned long long m) const { return __popcll(m & ((1ull << l) - 1ull)); }
    __device__ int32_t max_i32(int32_t v) const {
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
        return v;
    }
    __device__ long long min_i64(long long v) const {
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
        return v;
    }
    __device__ int32_t scan_max_incl(int32_t v) const {
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int32_t t = __shfl_up(v, d);
            if (l >= d) v = max(v, t);
        }
        return v;
    }
    __device__ int32_t shift_up(const int32_t v, const int32_t fill) const { return __builtin_amdgcn_update_dpp(fill, v, kWaveShr1, 0xf, 0xf, false); }
    __device__ int32_t bcast(const int32_t v, const int src) const { return __shfl(v, src); }
    __device__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
};

__global__ __launch_bounds__(kWave) void tdt_merge_fold(const mg::Args a) {
    __shared__ __attribute__((aligned(8))) unsigned char lds[mg::scratch_bytes(mg::kLdsSide, mg::kLdsSide)];
    Wave64 w{static_cast<int>(threadIdx.x)};
    const mg::Scratch small = mg::carve(lds, mg::kLdsSide, mg::kLdsSide);
    mg::Stream stage;
    mg::Scratch big;
    mg::slot_views(a.ws + static_cast<int64_t>(blockIdx.x) * a.slot_bytes, a.big_l, a.big_r, stage, big);
    for (int64_t r = blockIdx.x; r < a.n_recs; r += gridDim.x) {
        const mg::Rec rec = a.recs[r];
        mg::Fold f;
        f.out = mg::Stream{a.out.tok + rec.out_off, a.out.time + rec.out_off, a.out.dur + rec.out_off, a.out.conf + rec.out_off};
        f.runmax = a.runmax + rec.out_off;
        f.cap = rec.cap;
        f.stage = stage;
        f.n = 0;
        int32_t count = 0;
        const int32_t status = mg::fold_recording(w, f, a.win, a.counts, a.max_out, rec.w_lo, rec.w_hi, a.tb, a.tm, small, a.small_side, big, a.routes, &count);
        if (w.lane() == 0) {
            a.out_counts[r] = count;
            a.statuses[r] = status;
        }
        w.sync();   // the next recording reuses the slot
    }
}

}  // namespace

void fa::tdtmerge::launch(hipStream_t stream, const Args &a, const int32_t slots) {
    if (slots <= 0) return;
    hipLaunchKernelGGL(tdt_merge_fold, dim3(static_cast<unsigned>(slots)), dim3(kWave), 0, stream, a);
}
