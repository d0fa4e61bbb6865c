// mel.hip — batched STFT -> power -> Slaney mel -> log featurizer for gfx950.
//
// Replaces AudioMelSpectrogram.computeFlat / computeFlatTransposed / compute
// (reference: Sources/FluidAudio/Shared/AudioMelSpectrogram.swift:132-178,185-292,325-456).
//
// One workgroup (256 threads = 4 wavefronts) walks a contiguous range of 32-frame tiles.  Per tile the
// hop*31+512 pre-emphasised samples are staged in LDS once; then every wavefront runs its own 8 frames
// (two passes of 4 frames x 16 lanes) with NO workgroup barrier: window and twiddles sit in registers,
// the only LDS traffic of the FFT is one radix-16 transpose, the Z[k] <-> Z[256-k] exchange of the
// real-FFT recombination is a DPP lane permutation, and the 257 power bins go back to the wavefront's
// LDS region only to be gathered by the sparse triangular filterbank.  Log-mel values are staged in LDS
// and stored by the whole workgroup as full rows ([n_mels, T]: 128-byte runs; [T, n_mels]: contiguous).
// HBM traffic per 15 s utterance = 960 000 B read + 768 512 B written.
//
// Device code only, plus the two functions that have to see the kernel templates (raise_lds_limit, launch: the end of this file).
// Tables, plans, the plan cache and the host-pointer entry are in mel_host.hip; mel_launch.h is what the two share.
#include "mel_generic.h"
#include "mel_launch.h"

using namespace fa::mel;
using fa::melpk::f2;

namespace {

// lane l <- lane (16 - l) & 15 inside every row of 16 lanes: row_mirror (l <- 15 - l), then row_ror:1 (l <- l - 1)
__device__ __forceinline__ float dpp_partner(const float x) {
    int v = __float_as_int(x);
    v = __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);
    v = __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, true);
    return __int_as_float(v);
}

struct TileInfo {
    const float *x;  // utterance samples
    float *ob;       // utterance output
    int64_t len, n0;
    float lastv;
    int t0, T;
    bool stage;      // tile has frames to compute
    bool interior;   // the whole staged span (and the sample before it) lies inside the utterance
};

// global filterbank slot s -> (mel group i, slot j inside the group), resolved at compile time inside unrolled loops
template <class F>
__device__ __forceinline__ void constexpr_for_slot(const int s, F &&fn) {
#pragma unroll
    for (int i = 0; i < kFastGroups; ++i)
        if (s >= fast_slot_base(i) && s < fast_slot_base(i) + fast_slots(i)) fn(i, s - fast_slot_base(i));
}

// Both frames of a 16-lane group straight from the staged samples: v.re[n1] = (x[32 n1], x[32 n1 + hop]) and v.im[n1] the same
// one sample later, x = the lane's pointer (frame start + 2 lane).  One ds_read2_b32 per register pair.  Written in assembly
// because the load combiner pairs LDS reads by ascending offset — (x[32 n1], x[32 n1 + 32]) — which costs four register moves
// per pair to re-pair by frame; the wait for the 32 reads is part of the block (the compiler does not track them).
template <bool EZ>
__device__ __forceinline__ void load_frame_pair(const float *x, fa::melpk::LanePk &v) {
    static_assert(kPkHop == 160, "offsets below are written for hop 160");
    const unsigned a0 = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const float *)x));
#define FA_RD(i, b, o0, o1) "ds_read2_b32 %" #i ", %" #b " offset0:" #o0 " offset1:" #o1 "\n"
#define FA_RD4(i0, i1, i2, i3, b) FA_RD(i0, b, 0, 160) FA_RD(i1, b, 1, 161) FA_RD(i2, b, 32, 192) FA_RD(i3, b, 33, 193)
    if (EZ) {   // blocks n1 = 0 and n1 = 15 meet a zero window: literal zeros, 28 reads
        const fa::melpk::f2 zero = {0.0f, 0.0f};
        v.re[0] = zero; v.im[0] = zero; v.re[15] = zero; v.im[15] = zero;
        asm volatile(FA_RD(0, 28, 32, 192) FA_RD(1, 28, 33, 193) FA_RD4(2, 3, 4, 5, 29) FA_RD4(6, 7, 8, 9, 30) FA_RD4(10, 11, 12, 13, 31)
                     FA_RD4(14, 15, 16, 17, 32) FA_RD4(18, 19, 20, 21, 33) FA_RD4(22, 23, 24, 25, 34) FA_RD(26, 35, 0, 160) FA_RD(27, 35, 1, 161)
                     "s_waitcnt lgkmcnt(0)\n"
                     : "=&v"(v.re[1]), "=&v"(v.im[1]), "=&v"(v.re[2]), "=&v"(v.im[2]), "=&v"(v.re[3]), "=&v"(v.im[3]), "=&v"(v.re[4]), "=&v"(v.im[4]),
                       "=&v"(v.re[5]), "=&v"(v.im[5]), "=&v"(v.re[6]), "=&v"(v.im[6]), "=&v"(v.re[7]), "=&v"(v.im[7]), "=&v"(v.re[8]), "=&v"(v.im[8]),
                       "=&v"(v.re[9]), "=&v"(v.im[9]), "=&v"(v.re[10]), "=&v"(v.im[10]), "=&v"(v.re[11]), "=&v"(v.im[11]), "=&v"(v.re[12]), "=&v"(v.im[12]),
                       "=&v"(v.re[13]), "=&v"(v.im[13]), "=&v"(v.re[14]), "=&v"(v.im[14])
                     : "v"(a0), "v"(a0 + 256), "v"(a0 + 512), "v"(a0 + 768), "v"(a0 + 1024), "v"(a0 + 1280), "v"(a0 + 1536), "v"(a0 + 1792)
                     : "memory");
    } else {
        asm volatile(FA_RD4(0, 1, 2, 3, 32) FA_RD4(4, 5, 6, 7, 33) FA_RD4(8, 9, 10, 11, 34) FA_RD4(12, 13, 14, 15, 35)
                     FA_RD4(16, 17, 18, 19, 36) FA_RD4(20, 21, 22, 23, 37) FA_RD4(24, 25, 26, 27, 38) FA_RD4(28, 29, 30, 31, 39)
                     "s_waitcnt lgkmcnt(0)\n"
                     : "=&v"(v.re[0]), "=&v"(v.im[0]), "=&v"(v.re[1]), "=&v"(v.im[1]), "=&v"(v.re[2]), "=&v"(v.im[2]), "=&v"(v.re[3]), "=&v"(v.im[3]),
                       "=&v"(v.re[4]), "=&v"(v.im[4]), "=&v"(v.re[5]), "=&v"(v.im[5]), "=&v"(v.re[6]), "=&v"(v.im[6]), "=&v"(v.re[7]), "=&v"(v.im[7]),
                       "=&v"(v.re[8]), "=&v"(v.im[8]), "=&v"(v.re[9]), "=&v"(v.im[9]), "=&v"(v.re[10]), "=&v"(v.im[10]), "=&v"(v.re[11]), "=&v"(v.im[11]),
                       "=&v"(v.re[12]), "=&v"(v.im[12]), "=&v"(v.re[13]), "=&v"(v.im[13]), "=&v"(v.re[14]), "=&v"(v.im[14]), "=&v"(v.re[15]), "=&v"(v.im[15])
                     : "v"(a0), "v"(a0 + 256), "v"(a0 + 512), "v"(a0 + 768), "v"(a0 + 1024), "v"(a0 + 1280), "v"(a0 + 1536), "v"(a0 + 1792)
                     : "memory");
    }
#undef FA_RD4
#undef FA_RD
}

__device__ __forceinline__ void set_prio(const int p) {   // s_setprio takes an immediate
    if (p == 0) __builtin_amdgcn_s_setprio(0);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}

// PK: frame-pair packed arithmetic (mel_pk.h): one pass of 2 frames per 16-lane group instead of two passes of one; needs
// FAST and hop == kPkHop.  PK == 2: additionally the window is zero on the outer 32 positions of the frame (fft256<EZ>).
template <int LAYOUT, bool FAST, int PK>
__global__ __launch_bounds__(kThreads, 2) void mel_kernel(const MelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *samples = smem;
    float *regions = samples + a.stage_alloc;
    float *outs = regions + kRegions * (PK ? kRegionFloatsPk : kRegionFloats);
    int32_t *mtab = reinterpret_cast<int32_t *>(outs + a.out_alloc);
    float *mw = reinterpret_cast<float *>(mtab + kMaxMels);
    float *wtab = mw + ((a.n_weights + 24 + 3) & ~3);   // packed kernel: per-lane window rows (mel_pk.h)

    const int tid = threadIdx.x;
    const int l = tid & (kGroup - 1);   // lane inside the 16-lane frame group
    const int grp = tid >> 4;           // 0..15: LDS region == (wave, frame of the pass)

    for (int i = tid; i < a.n_mels; i += kThreads) mtab[i] = a.mel_tab[i];
    for (int i = tid; i < a.n_weights; i += kThreads) mw[i] = PK ? 0.25f * a.mel_w[i] : a.mel_w[i];  // PK power bins carry an exact factor 4

    LaneConst kc;
    fa::melpk::LaneConstPk kp;
    if (PK) {
        fa::melpk::lane_const_init(l, a.tw256, a.tw512, kp);
        fa::melpk::window_table_fill(tid, kThreads, a.windowz, wtab);
    } else {
        Tables c;
        c.windowz = a.windowz;
        c.tw256 = reinterpret_cast<const float *>(a.tw256);
        c.tw512 = reinterpret_cast<const float *>(a.tw512);
        lane_const_init(l, c, kc);
    }
    int mlo[(kFastGroups + 2) / 3];  // first power bin of the lane's mel in every group, 3 x 10 bits per register (fast path)
#pragma unroll
    for (int i = 0; i < (kFastGroups + 2) / 3; ++i) mlo[i] = 0;
#pragma unroll
    for (int i = 0; i < kFastGroups; ++i)
        if (FAST && l + 16 * i < a.n_mels) mlo[i / 3] |= (a.mel_tab[l + 16 * i] & 1023) << (10 * (i % 3));
    __syncthreads();

    const int64_t per = (a.total_tiles + gridDim.x - 1) / gridDim.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * per;
    const int64_t stop = first + per < a.total_tiles ? first + per : a.total_tiles;
    const int n_mels = a.n_mels;
    const bool hop_even = (a.hop & 1) == 0;
    const bool vec_stage = a.stage_alloc <= kStageVec * kThreads * 4;

    auto tile_info = [&](const int64_t tl) {
        TileInfo ti;
        // workgroup-uniform values, forced into SGPRs: the metadata loads below become scalar loads
        const int tli = __builtin_amdgcn_readfirstlane(static_cast<int>(tl));
        const int b = tli / a.tiles_per_utt;
        ti.t0 = (tli - b * a.tiles_per_utt) * kTileFrames;
        // The plan's tables are read-only for the kernel: read them through the constant address space so that they become
        // scalar loads (lgkmcnt).  As plain global loads they are vector loads, and the s_waitcnt vmcnt(0) in front of their
        // first use also sits out every output store and prefetch load still in flight — about 2 k cycles per tile.
        typedef const int32_t __attribute__((address_space(4))) *c_i32;
        typedef const int64_t __attribute__((address_space(4))) *c_i64;
        typedef const float __attribute__((address_space(4))) *c_f32;
        ti.T = ((c_i32)a.frames)[b];
        const int64_t base = ((c_i64)a.offsets)[b];
        ti.len = ((c_i64)a.offsets)[b + 1] - base;
        ti.x = a.pcm + base;
        ti.ob = a.out + static_cast<int64_t>(b) * a.utt_stride;
        ti.lastv = a.last ? ((c_f32)a.last)[b] : 0.0f;
        ti.n0 = static_cast<int64_t>(ti.t0) * a.hop - a.pad;
        ti.stage = ti.t0 < ti.T;
        ti.interior = ti.n0 >= 1 && ti.n0 + kStageVec * kThreads * 4 <= ti.len;
        if (ti.t0 == 0 && tid == 0 && a.lengths) a.lengths[b] = ti.T;
        return ti;
    };
    // raw samples of a tile: thread t owns the float4 groups t, t + 256, ... of the staged span, plus the sample before each
    float4 raw[kStageVec];
    float rprev[kStageVec];
    auto fetch = [&](const TileInfo &ti) {
        if (ti.interior) {  // workgroup-uniform: straight-line independent loads, one memory round trip for the whole tile
#pragma unroll
            for (int r = 0; r < kStageVec; ++r) {
                const float *src = ti.x + ti.n0 + 4 * (tid + kThreads * r);
                raw[r] = *reinterpret_cast<const float4 *>(src);
                // the sample before the group through an opaque index: seen together, the two loads are re-cut into
                // (x[-1..2], x[3]) and the pieces copied into place right behind the loads, i.e. behind an s_waitcnt vmcnt
                int before = -1;
                asm volatile("" : "+v"(before));
                rprev[r] = src[before];
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < kStageVec; ++r) {  // utterance edges (first / last tiles): unconditional loads from clamped indices
            const int64_t n = ti.n0 + 4 * (tid + kThreads * r);
            float t[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) {  // values outside [0, len) are replaced in stage(): no select (= no wait) behind the loads here
                const int64_t m = n - 1 + c;
                t[c] = ti.x[m < 0 ? 0 : (m < ti.len ? m : ti.len - 1)];
            }
            rprev[r] = t[0];
            raw[r] = make_float4(t[1], t[2], t[3], t[4]);
        }
    };
    auto stage = [&](const TileInfo &ti) {  // pre-emphasis (:211,:219-225: y[n] = x[n] - p x[n-1]); zero outside [0, len)
        int ts = tid;
        asm volatile("" : "+v"(ts));  // distinct from fetch()'s index arithmetic: shared, it would stay live (and spill) across the pass
        // Pin the prefetched values to this point.  The pre-emphasis below is vectorised into packed fma's whose operand pairs
        // (x[n - 1], x[n]) are assembled by register copies; without the pin those copies are scheduled right behind the loads
        // in fetch() — a whole pass earlier — together with the s_waitcnt vmcnt that makes the loads synchronous.
#pragma unroll
        for (int r = 0; r < kStageVec; ++r) asm volatile("" : "+v"(raw[r].x), "+v"(raw[r].y), "+v"(raw[r].z), "+v"(raw[r].w), "+v"(rprev[r]));
#pragma unroll
        for (int r = 0; r < kStageVec; ++r) {
            const int e = 4 * (ts + kThreads * r);
            if (e >= a.stage_alloc) continue;
            if (!ti.interior) {  // x[-1] = the carried last sample (:211), x = 0 elsewhere outside the utterance
                const int64_t n = ti.n0 + e;
                auto fix = [&](const float v, const int64_t m) { return m >= 0 && m < ti.len ? v : (m == -1 ? ti.lastv : 0.0f); };
                rprev[r] = fix(rprev[r], n - 1);
                raw[r].x = fix(raw[r].x, n); raw[r].y = fix(raw[r].y, n + 1); raw[r].z = fix(raw[r].z, n + 2); raw[r].w = fix(raw[r].w, n + 3);
            }
            float4 y;
            y.x = raw[r].x - a.preemph * rprev[r];
            y.y = raw[r].y - a.preemph * raw[r].x;
            y.z = raw[r].z - a.preemph * raw[r].y;
            y.w = raw[r].w - a.preemph * raw[r].z;
            if (!ti.interior) {
                const int64_t n = ti.n0 + e;
                if (n < 0 || n >= ti.len) y.x = 0.f;
                if (n + 1 < 0 || n + 1 >= ti.len) y.y = 0.f;
                if (n + 2 < 0 || n + 2 >= ti.len) y.z = 0.f;
                if (n + 3 < 0 || n + 3 >= ti.len) y.w = 0.f;
            }
            *reinterpret_cast<float4 *>(samples + e) = y;
        }
    };

    // All table / constant loads are complete from here on (vmcnt(0), expcnt/lgkmcnt untouched).  Without this explicit
    // instruction the wait-count pass keeps them "possibly pending" around the tile loop and guards the first LDS reads of
    // every pass with s_waitcnt vmcnt(<=3), which also drains the next tile's prefetch loads (vmcnt retires in order) and
    // exposes a full HBM round trip per tile.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    auto stage_tile = [&](const TileInfo &ti) {
        if (!ti.stage) return;
        if (vec_stage) stage(ti);
        else
            for (int i = tid; i < a.stage_count; i += kThreads) {  // large hops: plain staging loop
                const int64_t n = ti.n0 + i;
                float y = 0.0f;
                if (n >= 0 && n < ti.len) y = ti.x[n] - a.preemph * (n > 0 ? ti.x[n - 1] : ti.lastv);
                samples[i] = y;
            }
    };
    auto info_and_fetch = [&](const int64_t tl) {   // metadata + the 12 loads of tile tl (a no-op tile past the range)
        TileInfo ti{};
        ti.stage = false;
        if (tl < stop) { ti = tile_info(tl); if (ti.stage && vec_stage) fetch(ti); }
        return ti;
    };
    TileInfo cur = info_and_fetch(first);
    stage_tile(cur);
    TileInfo nxt = info_and_fetch(first + 1);   // always one tile ahead: its samples sit in registers during the pass

    // Per tile: barrier | compute | barrier | stage the next tile | store this tile | issue the loads of the tile after.  Staging
    // BEFORE the stores matters: the wait in front of the staging is vmcnt(0) (the wait-count pass cannot bound it across the
    // loop), and with the four output stores issued first it would sit out their write acknowledgements (~1.5 k cycles per
    // tile); in this order the only VMEM operations in flight are the loads issued a whole pass earlier.
    for (int64_t tl = first; tl < stop; ++tl) {
        __syncthreads();
        if (PK && cur.stage) {  // workgroup-uniform; group g computes the frames 2 g and 2 g + 1 of the tile in one pass
            using namespace fa::melpk;
            const int f = 2 * grp;
            LanePk v;
            float4 w4[8];
            set_prio(a.prio_rd);
#pragma unroll
            for (int q = 0; q < 8; ++q) w4[q] = reinterpret_cast<const float4 *>(wtab)[q * kGroup + l];
            load_frame_pair<PK == 2>(samples + f * kPkHop + 2 * l, v);
            f2 *P2 = reinterpret_cast<f2 *>(__builtin_assume_aligned(regions + grp * kRegionFloatsPk, 8));
            set_prio(a.prio_lo);   // VALU-bound stretch: yield issue slots to the co-resident wave's short latency-bound bursts
            fft256<PK == 2>(l, v, w4, kp, P2);
            set_prio(a.prio_pw);
            // power bins of both frames, pair k at P2[k], over the transpose buffer (its last reads are already issued)
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // Z[256 - (l + 16 j)]: lane (16 - l) & 15, register 15 - j (lane 0: own (16 - j) & 15)
                const f2 pr = partner(v.re[15 - j]), pi = partner(v.im[15 - j]);
                const f2 qr = l == 0 ? v.re[(16 - j) & 15] : pr;
                const f2 qi = l == 0 ? v.im[(16 - j) & 15] : pi;
                f2 plo, phi;
                pair_power4(v.re[j], v.im[j], qr, qi, kp.t2[j], plo, phi);
                P2[l + 16 * j] = plo;
                P2[kHalf - (l + 16 * j)] = phi;
            }
            if (l == 0) P2[128] = 4.0f * (v.re[8] * v.re[8] + v.im[8] * v.im[8]);  // k = 128: X = conj(Z[128])
            set_prio(a.prio_hi);   // LDS-latency-bound from here to the next pass: issue as soon as data arrives
            // sparse triangular filterbank (vDSP_mmul row, :270-283, zeros skipped): lane l owns the mels l + 16 i; weights are
            // fetched two global slots (2 p, 2 p + 1) per register pair, so a pair may straddle two mel groups
            f2 acc[kFastGroups];
            const f2 *P[kFastGroups];
#pragma unroll
            for (int i = 0; i < kFastGroups; ++i) {
                acc[i] = f2{0.0f, 0.0f};
                P[i] = P2 + ((mlo[i / 3] >> (10 * (i % 3))) & 1023);
            }
            // All LDS reads of a half are issued before its first fma (sched_barrier keeps the scheduler from re-serialising
            // them into load -> wait -> fma chains, which exposes one LDS round trip per slot): weights first, then the bins.
            constexpr int kSplit = fast_slot_base(6) & ~1;   // slots [0, kSplit): groups 0..5 (even, so weight pairs do not straddle the halves)
            {
                f2 w[kSplit / 2], pb[kSplit];
#pragma unroll
                for (int sp = 0; sp < kSplit / 2; ++sp) w[sp] = f2{mw[(2 * sp) * kGroup + l], mw[(2 * sp + 1) * kGroup + l]};
#pragma unroll
                for (int s = 0; s < kSplit; ++s) constexpr_for_slot(s, [&](const int i, const int j) { pb[s] = P[i][j]; });
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < kSplit; ++s)
                    constexpr_for_slot(s, [&](const int i, const int) { acc[i] = (s & 1) ? fma_hi(pb[s], w[s / 2], acc[i]) : fma_lo(pb[s], w[s / 2], acc[i]); });
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                constexpr int kRest = kFastSlots - kSplit;
                f2 w[(kRest + 1) / 2], pb[kRest];
#pragma unroll
                for (int sp = 0; sp < (kRest + 1) / 2; ++sp) w[sp] = f2{mw[(kSplit + 2 * sp) * kGroup + l], mw[(kSplit + 2 * sp + 1) * kGroup + l]};
#pragma unroll
                for (int s = kSplit; s < kFastSlots; ++s) constexpr_for_slot(s, [&](const int i, const int j) { pb[s - kSplit] = P[i][j]; });
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = kSplit; s < kFastSlots; ++s)
                    constexpr_for_slot(s, [&](const int i, const int) {
                        acc[i] = (s & 1) ? fma_hi(pb[s - kSplit], w[(s - kSplit) / 2], acc[i]) : fma_lo(pb[s - kSplit], w[(s - kSplit) / 2], acc[i]);
                    });
            }
            // :542-549: log(acc + floor) or log(max(acc, floor)) as log(max(acc + add, clamp)) with wave-uniform add / clamp.
            // The argument is >= floor > 0 and far from the denormal range, so the hardware log2 (1 ulp) times ln 2 replaces
            // logf's denormal pre-scaling and two-term ln 2 product: 2 instructions instead of 11.
            const float add_floor = a.floor_clamped ? 0.0f : a.log_floor, clamp_floor = a.floor_clamped ? a.log_floor : 0.0f;
#pragma unroll
            for (int i = 0; i < kFastGroups; ++i) {
                const int m = l + 16 * i;
                constexpr float kLn2 = 0.693147180559945309f;
                const f2 x = acc[i] + add_floor;
                f2 val;
                val.x = kLn2 * __builtin_amdgcn_logf(fmaxf(x.x, clamp_floor));
                val.y = kLn2 * __builtin_amdgcn_logf(fmaxf(x.y, clamp_floor));
                if (m < n_mels) {
                    if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR) *reinterpret_cast<f2 *>(outs + m * kMelPad + f) = val;
                    else { outs[f * (n_mels + kFramePad) + m] = val.x; outs[(f + 1) * (n_mels + kFramePad) + m] = val.y; }
                }
            }
        }
        if (!PK && cur.stage) {  // workgroup-uniform
            float *R = static_cast<float *>(__builtin_assume_aligned(regions + grp * kRegionFloats, 8));
#pragma unroll 1
            for (int pass = 0; pass < kPasses; ++pass) {
                // frame of this 16-lane group inside the tile: wave w owns frames [8w, 8w + 8)
                const int f = (grp >> 2) * (kWaveFrames * kPasses) + pass * kWaveFrames + (grp & 3);
                const float *fs = hop_even ? static_cast<const float *>(__builtin_assume_aligned(samples + f * a.hop, 8)) : samples + f * a.hop;
                Lane v;
                if (hop_even) {
#pragma unroll
                    for (int n1 = 0; n1 < 16; ++n1) {
                        const float2 s2 = *reinterpret_cast<const float2 *>(fs + 32 * n1 + 2 * l);
                        v.re[n1] = s2.x; v.im[n1] = s2.y;
                    }
                } else {
#pragma unroll
                    for (int n1 = 0; n1 < 16; ++n1) { v.re[n1] = fs[32 * n1 + 2 * l]; v.im[n1] = fs[32 * n1 + 2 * l + 1]; }
                }
                // Everything below exchanges data only between the 16 lanes of one frame group, i.e. inside one
                // wavefront: LDS operations of a wavefront complete in program order, no barrier is needed.
                phase_a2(l, v, kc, R);
                phase_b1(l, R, v);
                float qr[8], qi[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {  // Z[256 - (l + 16 j)]: lane (16 - l) & 15, register 15 - j (lane 0: own (16 - j) & 15)
                    const float pr = dpp_partner(v.re[15 - j]), pi = dpp_partner(v.im[15 - j]);
                    qr[j] = l == 0 ? v.re[(16 - j) & 15] : pr;
                    qi[j] = l == 0 ? v.im[(16 - j) & 15] : pi;
                }
                Power p;
                phase_c1v2(l, v, qr, qi, kc, p);
                // power bins at R + {0,14,28,10}[frame]: regions are 578 = 2 (mod 32) floats apart, so this puts the two frames
                // of a 32-lane LDS service group 16 banks apart and the gathers below stop colliding
                float *PR = R + ((0x0a1c0e00u >> (8 * (grp & 3))) & 0xff);
                phase_c2(l, p, PR);
                // sparse triangular filterbank + log for this group's frame: lane l owns mels l, l + 16, ...
                if (FAST) {
                    // weights zero-padded to the slot profile, [slot][16 lanes]: every read below is independent
                    float acc[kFastGroups];
#pragma unroll
                    for (int i = 0; i < kFastGroups; ++i) {
                        acc[i] = 0.0f;
#pragma unroll
                        for (int j = 0; j < fast_slots(i); ++j)
                            acc[i] += mw[(fast_slot_base(i) + j) * kGroup + l] * PR[((mlo[i / 3] >> (10 * (i % 3))) & 1023) + j];  // vDSP_mmul row (:270-283), zeros skipped
                    }
#pragma unroll
                    for (int i = 0; i < kFastGroups; ++i) {
                        const int m = l + 16 * i;
                        const float val = a.floor_clamped ? logf(fmaxf(acc[i], a.log_floor)) : logf(acc[i] + a.log_floor);  // :542-549
                        if (m < n_mels) {
                            if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR) outs[m * kMelPad + f] = val;
                            else outs[f * (n_mels + kFramePad) + m] = val;
                        }
                    }
                } else {
                    for (int m = l; m < n_mels; m += kGroup) {
                        const int packed = mtab[m];
                        const int lo = packed & 1023, cnt = (packed >> 10) & 1023, st = packed >> 20;
                        const float *P = PR + lo;
                        const float *wgt = mw + st;
                        float acc = 0.0f;
                        for (int j = 0; j < cnt; ++j) acc += wgt[j] * P[j];
                        const float val = a.floor_clamped ? logf(fmaxf(acc, a.log_floor)) : logf(acc + a.log_floor);
                        if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR) outs[m * kMelPad + f] = val;
                        else outs[f * (n_mels + kFramePad) + m] = val;
                    }
                }
            }
        }
        __syncthreads();
        stage_tile(nxt);   // `samples` has no reader left after the barrier

        const bool full_tile = cur.t0 + kTileFrames <= cur.T && cur.t0 + kTileFrames <= a.frame_stride;
        if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR && FAST && full_tile && n_mels == kFastGroups * kGroup) {
            // 8 threads per mel row, 4 consecutive frames each: 16-byte LDS reads, 16-byte global stores (:287); a fixed number
            // of stores per thread keeps the wait count for the next tile's prefetch exact (vmcnt(4) instead of vmcnt(0))
            int st = tid;
            asm volatile("" : "+v"(st));   // keep the store addresses loop-variant: hoisted, they sit in 12 registers across the whole tile loop
#pragma unroll
            for (int it = 0; it < kFastGroups * kGroup * (kTileFrames / 4) / kThreads; ++it) {
                const int idx = st + kThreads * it, m = idx >> 3, f = (idx & 7) * 4;   // every thread stores: no exec masking, exact vmcnt
                *reinterpret_cast<float4 *>(cur.ob + static_cast<int64_t>(m) * a.frame_stride + cur.t0 + f) =
                    *reinterpret_cast<const float4 *>(outs + m * kMelPad + f);
            }
        } else if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR) {
            for (int idx = tid; idx < n_mels * (kTileFrames / 4); idx += kThreads) {
                const int m = idx >> 3, f = (idx & 7) * 4, t = cur.t0 + f;
                if (t >= a.frame_stride) continue;
                float4 v4 = *reinterpret_cast<const float4 *>(outs + m * kMelPad + f);
                float *dst = cur.ob + static_cast<int64_t>(m) * a.frame_stride + t;
                if (t + 3 < cur.T && t + 3 < a.frame_stride) { *reinterpret_cast<float4 *>(dst) = v4; continue; }
                const float e[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (t + c < a.frame_stride) dst[c] = t + c < cur.T ? e[c] : 0.0f;  // padValue (:39) for t >= T
            }
        } else {
            const int work = kTileFrames * n_mels;
            for (int idx = tid; idx < work; idx += kThreads) {
                const int f = idx / n_mels, m = idx - f * n_mels;
                const int t = cur.t0 + f;
                if (t >= a.frame_stride) continue;
                cur.ob[static_cast<int64_t>(t) * n_mels + m] = t < cur.T ? outs[f * (n_mels + kFramePad) + m] : 0.0f;  // :451
            }
        }
        // the barrier at the top of the next iteration orders these `outs` reads before the next tile's writes
        cur = nxt;
        // the loads of the tile after the next travel from HBM during the barrier wait and the whole next pass
        nxt = info_and_fetch(tl + 2);
    }
}

#include "mel_v4.inc"
// Every kernel of this translation unit, once: the generic one and the 16 tuned instantiations, indexed by what a plan resolved.
#define FA_K3(L) {reinterpret_cast<const void *>(mel_kernel<L, false, 0>), reinterpret_cast<const void *>(mel_kernel<L, true, 0>), \
                  reinterpret_cast<const void *>(mel_kernel<L, true, 1>), reinterpret_cast<const void *>(mel_kernel<L, true, 2>)}
#define FA_K4(L, E) {reinterpret_cast<const void *>(mel_kernel_v4<L, E, false>), reinterpret_cast<const void *>(mel_kernel_v4<L, E, true>)}
const void *const kKernelV3[2][4] = {FA_K3(0), FA_K3(1)};                                             // [layout][fast + pk + (pk && edge_zero)]
const void *const kKernelV4[2][2][2] = {{FA_K4(0, false), FA_K4(0, true)}, {FA_K4(1, false), FA_K4(1, true)}};   // [layout][edge_zero][clamped]
#undef FA_K4
#undef FA_K3

const void *kernel_of(const Variant &v) {
    if (v.generic) return reinterpret_cast<const void *>(fa::melgen::mel_generic_kernel);
    if (v.v4) return kKernelV4[v.layout][v.edge_zero][v.clamped];
    return kKernelV3[v.layout][v.fast + v.pk + (v.pk && v.edge_zero)];
}

}  // namespace

namespace fa {
namespace mel {

void raise_lds_limit(const Variant &v, const size_t lds_bytes) {
    (void)hipFuncSetAttribute(kernel_of(v), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
}

void launch(const Variant &v, const int grid, const size_t lds_bytes, hipStream_t stream, const void *args) {
    static_assert(kThreads == fa::melgen::kThreads, "one block size for every kernel of the table");
    void *kargs[] = {const_cast<void *>(args)};
    (void)hipLaunchKernel(kernel_of(v), dim3(grid), dim3(kThreads), kargs, lds_bytes, stream);
}

}  // namespace mel
}  // namespace fa
