// mel_v4.inc — occupancy-first variant of the frame-pair packed STFT->mel kernel (included inside mel.hip's anonymous namespace).
//
// Same arithmetic as mel_kernel<.., PK> (mel_pk.h: two frames per lane, v_pk_* fp32, radix-16 x radix-16, DPP partner
// exchange, sparse filterbank, hardware log2), re-plumbed so that THREE workgroups (12 wavefronts) fit a CU instead of two:
// micro-benchmarks (profiles/r02_ubench_valu_lds.txt) show that one wavefront issues a VALU instruction every ~5.5 cycles
// whether 1 or 4 wavefronts share the SIMD, and that the LDS pipe of a CU still scales at 16 wavefronts — at 2 wavefronts per
// SIMD the v3 kernel is bound by the latency chain of ONE wavefront, not by VALU, LDS or HBM throughput.  What had to go:
//   * the register double-buffer of the next tile's samples across the whole pass (30 VGPRs): the loads of the next tile are
//     issued after the pass, fly during the store phase, and the other workgroups of the CU cover the rest of their latency;
//   * register-resident twiddles (46 VGPRs): two small LDS tables, read where they are used;
//   * the separate sample / transpose / output-tile areas (21.9 + 34.8 + 18.4 KB): ONE 34.8 KB area holds the staged samples
//     until every wavefront has read its frames (barrier), then the 16 transpose regions, then the log-mel tile (each group
//     writes its 128 x 2 values into its own region, rotated by 4 slots per frame quad so that the store phase reads them
//     conflict-free): 42.6 KB per workgroup.
// Staged samples are de-interleaved (even samples | odd samples) and a 32-lane LDS service group holds the frame pairs
// (f, f + 2) and (f + 1, f + 3): the two groups read banks 16 apart, which removes the 2-way conflict of the v3 sample reads
// (all frame starts are multiples of 160 = 5 x 32 floats).
// LDS instruction choice (scripts/ubench/ldsw.hip, profiles/r03_ubench_lds_width.txt, 12 wavefronts per CU): per 64 lanes x 16 bytes a
// ds_read2_b64 occupies the LDS pipe for 8.2 clocks, two ds_read_b64 for 4.8, one ds_read_b128 for 4.4 (conflict-free when the lane
// stride is 4 x odd dwords); ds_read2_b32 4.5 clocks per 8 bytes against 2.6 for ds_read_b64.  The compiler merges neighbouring 8-byte
// reads into ds_read2_b64, so every table / transpose / power read below is a VOLATILE 8- or 16-byte load (never merged), the
// transpose rows hold 18 pairs (144 bytes: 16-byte aligned rows, lane stride 36 dwords) and the twiddle tables are laid out by
// lane ([lane][k], 16-byte reads) instead of by k.  The sizes of this carve-up (kV4*) are in mel_launch.h: the host sizes the launch from them.
typedef float v4f __attribute__((ext_vector_type(4)));
// (explicit LDS address space: address-space inference leaves volatile accesses alone, they would become flat loads)
__device__ __forceinline__ fa::melpk::f2 lds_ld8(const fa::melpk::f2 *p) { return *(__attribute__((address_space(3))) const volatile fa::melpk::f2 *)p; }
__device__ __forceinline__ v4f lds_ld16(const float *p) { return *(__attribute__((address_space(3))) const volatile v4f *)p; }

// Both frames (f, f + 2) of a 16-lane group from the de-interleaved staged samples: v.re[n1] = (E[16 n1], E[16 n1 + 160]),
// v.im[n1] likewise from the odd samples; e = the lane's pointer into E (frame start / 2 + lane), o the same into O.
template <bool EZ>
__device__ __forceinline__ void load_frame_pair_eo(const float *e, const float *o, fa::melpk::LanePk &v) {
    static_assert(kPkHop == 160, "offsets below are written for hop 160");
    const unsigned ea = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const float *)e));
    const unsigned oa = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const float *)o));
    if (EZ) {   // blocks n1 = 0 and n1 = 15 meet a zero window: literal zeros, 28 reads
        const fa::melpk::f2 zero = {0.0f, 0.0f};
        v.re[0] = zero; v.im[0] = zero; v.re[15] = zero; v.im[15] = zero;
        asm volatile("ds_read2_b32 %0, %28 offset0:16 offset1:176\n" "ds_read2_b32 %1, %31 offset0:16 offset1:176\n"
                     "ds_read2_b32 %2, %28 offset0:32 offset1:192\n" "ds_read2_b32 %3, %31 offset0:32 offset1:192\n"
                     "ds_read2_b32 %4, %28 offset0:48 offset1:208\n" "ds_read2_b32 %5, %31 offset0:48 offset1:208\n"
                     "ds_read2_b32 %6, %28 offset0:64 offset1:224\n" "ds_read2_b32 %7, %31 offset0:64 offset1:224\n"
                     "ds_read2_b32 %8, %28 offset0:80 offset1:240\n" "ds_read2_b32 %9, %31 offset0:80 offset1:240\n"
                     "ds_read2_b32 %10, %29 offset0:0 offset1:160\n" "ds_read2_b32 %11, %32 offset0:0 offset1:160\n"
                     "ds_read2_b32 %12, %29 offset0:16 offset1:176\n" "ds_read2_b32 %13, %32 offset0:16 offset1:176\n"
                     "ds_read2_b32 %14, %29 offset0:32 offset1:192\n" "ds_read2_b32 %15, %32 offset0:32 offset1:192\n"
                     "ds_read2_b32 %16, %29 offset0:48 offset1:208\n" "ds_read2_b32 %17, %32 offset0:48 offset1:208\n"
                     "ds_read2_b32 %18, %29 offset0:64 offset1:224\n" "ds_read2_b32 %19, %32 offset0:64 offset1:224\n"
                     "ds_read2_b32 %20, %29 offset0:80 offset1:240\n" "ds_read2_b32 %21, %32 offset0:80 offset1:240\n"
                     "ds_read2_b32 %22, %30 offset0:0 offset1:160\n" "ds_read2_b32 %23, %33 offset0:0 offset1:160\n"
                     "ds_read2_b32 %24, %30 offset0:16 offset1:176\n" "ds_read2_b32 %25, %33 offset0:16 offset1:176\n"
                     "ds_read2_b32 %26, %30 offset0:32 offset1:192\n" "ds_read2_b32 %27, %33 offset0:32 offset1:192\n"
                     "s_waitcnt lgkmcnt(0)\n"
                     : "=&v"(v.re[1]), "=&v"(v.im[1]), "=&v"(v.re[2]), "=&v"(v.im[2]), "=&v"(v.re[3]), "=&v"(v.im[3]), "=&v"(v.re[4]), "=&v"(v.im[4]),
                       "=&v"(v.re[5]), "=&v"(v.im[5]), "=&v"(v.re[6]), "=&v"(v.im[6]), "=&v"(v.re[7]), "=&v"(v.im[7]), "=&v"(v.re[8]), "=&v"(v.im[8]),
                       "=&v"(v.re[9]), "=&v"(v.im[9]), "=&v"(v.re[10]), "=&v"(v.im[10]), "=&v"(v.re[11]), "=&v"(v.im[11]), "=&v"(v.re[12]), "=&v"(v.im[12]),
                       "=&v"(v.re[13]), "=&v"(v.im[13]), "=&v"(v.re[14]), "=&v"(v.im[14])
                     : "v"(ea), "v"(ea + 384), "v"(ea + 768), "v"(oa), "v"(oa + 384), "v"(oa + 768)
                     : "memory");
    } else {
        asm volatile("ds_read2_b32 %0, %32 offset0:0 offset1:160\n" "ds_read2_b32 %1, %35 offset0:0 offset1:160\n"
                     "ds_read2_b32 %2, %32 offset0:16 offset1:176\n" "ds_read2_b32 %3, %35 offset0:16 offset1:176\n"
                     "ds_read2_b32 %4, %32 offset0:32 offset1:192\n" "ds_read2_b32 %5, %35 offset0:32 offset1:192\n"
                     "ds_read2_b32 %6, %32 offset0:48 offset1:208\n" "ds_read2_b32 %7, %35 offset0:48 offset1:208\n"
                     "ds_read2_b32 %8, %32 offset0:64 offset1:224\n" "ds_read2_b32 %9, %35 offset0:64 offset1:224\n"
                     "ds_read2_b32 %10, %32 offset0:80 offset1:240\n" "ds_read2_b32 %11, %35 offset0:80 offset1:240\n"
                     "ds_read2_b32 %12, %33 offset0:0 offset1:160\n" "ds_read2_b32 %13, %36 offset0:0 offset1:160\n"
                     "ds_read2_b32 %14, %33 offset0:16 offset1:176\n" "ds_read2_b32 %15, %36 offset0:16 offset1:176\n"
                     "ds_read2_b32 %16, %33 offset0:32 offset1:192\n" "ds_read2_b32 %17, %36 offset0:32 offset1:192\n"
                     "ds_read2_b32 %18, %33 offset0:48 offset1:208\n" "ds_read2_b32 %19, %36 offset0:48 offset1:208\n"
                     "ds_read2_b32 %20, %33 offset0:64 offset1:224\n" "ds_read2_b32 %21, %36 offset0:64 offset1:224\n"
                     "ds_read2_b32 %22, %33 offset0:80 offset1:240\n" "ds_read2_b32 %23, %36 offset0:80 offset1:240\n"
                     "ds_read2_b32 %24, %34 offset0:0 offset1:160\n" "ds_read2_b32 %25, %37 offset0:0 offset1:160\n"
                     "ds_read2_b32 %26, %34 offset0:16 offset1:176\n" "ds_read2_b32 %27, %37 offset0:16 offset1:176\n"
                     "ds_read2_b32 %28, %34 offset0:32 offset1:192\n" "ds_read2_b32 %29, %37 offset0:32 offset1:192\n"
                     "ds_read2_b32 %30, %34 offset0:48 offset1:208\n" "ds_read2_b32 %31, %37 offset0:48 offset1:208\n"
                     "s_waitcnt lgkmcnt(0)\n"
                     : "=&v"(v.re[0]), "=&v"(v.im[0]), "=&v"(v.re[1]), "=&v"(v.im[1]), "=&v"(v.re[2]), "=&v"(v.im[2]), "=&v"(v.re[3]), "=&v"(v.im[3]),
                       "=&v"(v.re[4]), "=&v"(v.im[4]), "=&v"(v.re[5]), "=&v"(v.im[5]), "=&v"(v.re[6]), "=&v"(v.im[6]), "=&v"(v.re[7]), "=&v"(v.im[7]),
                       "=&v"(v.re[8]), "=&v"(v.im[8]), "=&v"(v.re[9]), "=&v"(v.im[9]), "=&v"(v.re[10]), "=&v"(v.im[10]), "=&v"(v.re[11]), "=&v"(v.im[11]),
                       "=&v"(v.re[12]), "=&v"(v.im[12]), "=&v"(v.re[13]), "=&v"(v.im[13]), "=&v"(v.re[14]), "=&v"(v.im[14]), "=&v"(v.re[15]), "=&v"(v.im[15])
                     : "v"(ea), "v"(ea + 384), "v"(ea + 768), "v"(oa), "v"(oa + 384), "v"(oa + 768)
                     : "memory");
    }
}

// The tile queue runs two tiles ahead, so that the loads of the next tile are issued right behind B2 and travel during the
// whole second pass (30 more live registers there) instead of only during the store phase.
template <int LAYOUT, bool EZ, bool CLAMPED>
__global__ __launch_bounds__(kThreads, 3) void mel_kernel_v4(const MelArgs a) {
    constexpr bool AHEAD = true;   // the next tile's loads are issued before the store phase of the current one (measured equal to issuing them at the top of their own iteration)
    using namespace fa::melpk;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *area = smem;
    float *mw = area + kV4AreaFloats;
    float *wtab = mw + kV4WeightFloats;
    float *t1tab = wtab + kWindowTableFloats;
    float *t2tab = t1tab + kV4T1Floats;
    volatile int *qslot = reinterpret_cast<volatile int *>(t2tab + kV4T2Floats);   // tile indices handed from thread 0 to the workgroup

    const int tid = threadIdx.x;
    // Lane geometry is re-derived from an opaque copy of the thread id in every phase of the tile loop (FA_V4_LANE): as loop
    // invariants the per-lane LDS / global addresses of all phases stay live across the whole loop (~40 VGPRs) and spill.
#define FA_V4_LANE()                                                                                              \
    int tidp = tid;                                                                                               \
    asm volatile("" : "+v"(tidp));                                                                                \
    const int l = tidp & (kGroup - 1);            /* lane inside the 16-lane frame group */                        \
    const int grp = tidp >> 4;                    /* 0..15 = region */                                             \
    const int fbase = 8 * (grp >> 2) + 4 * ((grp >> 1) & 1) + (grp & 1); /* the group computes frames fbase, fbase + 2 */ \
    (void)fbase; (void)l

    for (int i = tid; i < kV4WeightFloats; i += kThreads) {   // power bins carry an exact factor 4
        const int slot = 2 * (i >> 5) + (i & 1), lane = (i >> 1) & 15, src = slot * kGroup + lane;
        mw[i] = src < a.n_weights ? 0.25f * a.mel_w[src] : 0.0f;
    }
    window_table_fill(tid, kThreads, a.windowz, wtab);
    for (int i = tid; i < kV4T1Floats / 2; i += kThreads) {   // row `lane`: exp(-2 pi i lane k1 / 256), k1 = 1..15, then padding
        const int lane = i / (kV4T1Stride / 2), k = i % (kV4T1Stride / 2);
        const float2 t = k < 15 ? a.tw256[(lane * (k + 1)) & 255] : make_float2(0.0f, 0.0f);
        t1tab[2 * i] = t.x; t1tab[2 * i + 1] = t.y;
    }
    for (int i = tid; i < kV4T2Floats / 2; i += kThreads) {   // row `lane`: exp(-2 pi i (lane + 16 j) / 512), j = 0..7, then padding
        const int lane = i / (kV4T2Stride / 2), j = i % (kV4T2Stride / 2);
        const float2 t = j < 8 ? a.tw512[lane + 16 * j] : make_float2(0.0f, 0.0f);
        t2tab[2 * i] = t.x; t2tab[2 * i + 1] = t.y;
    }
    int mlo[(kFastGroups + 2) / 3];
#pragma unroll
    for (int i = 0; i < (kFastGroups + 2) / 3; ++i) mlo[i] = 0;
#pragma unroll
    for (int i = 0; i < kFastGroups; ++i) mlo[i / 3] |= (a.mel_tab[(tid & 15) + 16 * i] & 1023) << (10 * (i % 3));
    __syncthreads();

    // Tiles are handed out dynamically: one atomic per tile on a counter that never resets.  Every workgroup draws one index
    // per tile it processes plus the two (>= total_tiles) it holds when it stops (the queue runs two tiles ahead), so a launch advances the counter
    // by exactly total_tiles + 2 gridDim.x and launch k owns the values from queue_base = k (total_tiles + 2 gridDim.x).  Static ranges lose a third of the machine here: the
    // workgroups of a CU are served by age (the oldest issues first), so the first-dispatched workgroup of every CU finishes
    // its range in 0.47 ms, the second in 0.58 ms, the third in 0.69 ms (profiles/r02_mel_v4_static_ranges.txt).  The next
    // index is requested right after B1 and consumed after B3: its latency hides behind the pass.
    const int total_tiles = static_cast<int>(a.total_tiles);
    auto grab = [&]() { return static_cast<int>(atomicAdd(a.queue, 1ull) - a.queue_base); };
    auto tile_info = [&](const int tl) {
        TileInfo ti;
        const int tli = __builtin_amdgcn_readfirstlane(tl);
        const int b = tli / a.tiles_per_utt;
        ti.t0 = (tli - b * a.tiles_per_utt) * kTileFrames;
        typedef const int32_t __attribute__((address_space(4))) *c_i32;   // constant address space: scalar loads (see mel_kernel)
        typedef const int64_t __attribute__((address_space(4))) *c_i64;
        typedef const float __attribute__((address_space(4))) *c_f32;
        ti.T = ((c_i32)a.frames)[b];
        const int64_t base = ((c_i64)a.offsets)[b];
        ti.len = ((c_i64)a.offsets)[b + 1] - base;
        ti.x = a.pcm + base;
        ti.ob = a.out + static_cast<int64_t>(b) * a.utt_stride;
        ti.lastv = a.last ? ((c_f32)a.last)[b] : 0.0f;
        ti.n0 = static_cast<int64_t>(ti.t0) * kPkHop - a.pad;
        ti.stage = ti.t0 < ti.T;
        ti.interior = ti.n0 >= 1 && ti.n0 + kStageVec * kThreads * 4 <= ti.len;
        if (ti.t0 == 0 && threadIdx.x == 0 && a.lengths) a.lengths[b] = ti.T;
        return ti;
    };
    // Raw samples of a tile: thread t owns the float4 groups t, t + 256, ... of the staged span plus the sample before each.
    // ONE code path for every tile: the group base is clamped into the utterance (32-bit utterance-relative indices: scalar
    // base + lane offset; the plan rejects utterances of 2^31 samples), so interior tiles load exactly their samples and edge
    // tiles load something valid that stage() replaces (groups outside the utterance are zeros, the one group straddling its
    // end is re-read element-wise there).  Utterances shorter than 4 samples load nothing here.
    float4 raw[kStageVec];
    float rprev[kStageVec];
    auto fetch = [&](const TileInfo &ti) {
        int tidf = threadIdx.x;
        asm volatile("" : "+v"(tidf));
        const int n0i = static_cast<int>(ti.n0), hi = static_cast<int>(ti.len) - 4;
        if (hi < 0) return;
#pragma unroll
        for (int r = 0; r < kStageVec; ++r) {
            int nb = n0i + 4 * (tidf + kThreads * r);
            nb = nb < 0 ? 0 : (nb > hi ? hi : nb);
            const float *src = ti.x + nb;
            raw[r] = *reinterpret_cast<const float4 *>(src);
            int before = nb > 0 ? -1 : 0;
            asm volatile("" : "+v"(before));   // keeps the two loads apart (see mel_kernel)
            rprev[r] = src[before];
        }
    };
    auto stage = [&](const TileInfo &ti) {   // pre-emphasis (:211,:219-225), zero outside [0, len); even samples -> E, odd -> O
        float *E = area, *O = area + kV4HalfSamples;
        int tids = threadIdx.x;
        asm volatile("" : "+v"(tids));
        const int n0i = static_cast<int>(ti.n0), len_i = static_cast<int>(ti.len);
#pragma unroll
        for (int r = 0; r < kStageVec; ++r) {
            const int e = 4 * (tids + kThreads * r);
            float4 xv = raw[r];
            float xp = rprev[r];
            if (!ti.interior) {   // workgroup-uniform
                const int n = n0i + e;
                if (n == 0 && len_i >= 4) xp = ti.lastv;                           // x[-1] = the carried last sample (:211)
                else if (n < 1 || n + 3 >= len_i) {                                // outside the utterance, or straddling its end
                    auto at = [&](const int m) { return m >= 0 && m < len_i ? ti.x[m] : (m == -1 ? ti.lastv : 0.0f); };
                    xp = at(n - 1); xv.x = at(n); xv.y = at(n + 1); xv.z = at(n + 2); xv.w = at(n + 3);
                }
            }
            float4 y;
            y.x = xv.x - a.preemph * xp;
            y.y = xv.y - a.preemph * xv.x;
            y.z = xv.z - a.preemph * xv.y;
            y.w = xv.w - a.preemph * xv.z;
            if (!ti.interior) {
                const int n = n0i + e;
                if (n < 0 || n >= len_i) y.x = 0.f;
                if (n + 1 < 0 || n + 1 >= len_i) y.y = 0.f;
                if (n + 2 < 0 || n + 2 >= len_i) y.z = 0.f;
                if (n + 3 < 0 || n + 3 >= len_i) y.w = 0.f;
            }
            *reinterpret_cast<float2 *>(E + (e >> 1)) = make_float2(y.x, y.z);
            *reinterpret_cast<float2 *>(O + (e >> 1)) = make_float2(y.y, y.w);
        }
    };

    __builtin_amdgcn_s_waitcnt(0x0F70);   // table loads complete: vmcnt(0) once, outside the tile loop
    if (tid == 0) { qslot[0] = grab(); qslot[1] = grab(); }
    __syncthreads();
    int tl = __builtin_amdgcn_readfirstlane(qslot[0]);
    int tl_n = __builtin_amdgcn_readfirstlane(qslot[1]);   // the tile after `tl`, known one iteration ahead
    __syncthreads();                                       // (both slots are reused below)
    int par = 1;
    TileInfo cur{};
    cur.stage = false;
    if (tl < total_tiles) { cur = tile_info(tl); if (AHEAD && cur.stage) fetch(cur); }
    long long n_done = 0;

    unsigned long long t_seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // cycle stamps, inert while a.prof is null (MelArgs::prof): stage | B1 | reads + first pass | B2 | rest of the pass | B3 | loads + stores | B4
    unsigned long long t_prev = a.prof ? clock64() : 0;
    const unsigned long long t_begin = t_prev, w_begin = a.prof ? wall_clock64() : 0;   // wall_clock64: constant 100 MHz
#define V4_FINE(i) do { } while (0)
#define V4_STAMP(i) V4_STAMP_(i)
#define V4_STAMP_(i) do { if (a.prof) { const unsigned long long t_now = clock64(); t_seg[i] += t_now - t_prev; t_prev = t_now; } } while (0)
    while (tl < total_tiles) {
        ++n_done;
        if (!cur.stage) {   // workgroup-uniform: a tile of padding frames only (t >= T): padValue (:39), nothing to compute
            const int n_out = LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR ? kFastGroups * kGroup * kTileFrames : kTileFrames * kFastGroups * kGroup;
            for (int idx = threadIdx.x; idx < n_out; idx += kThreads) {
                const int m = LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR ? idx >> 5 : idx & 127, t = cur.t0 + (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR ? idx & 31 : idx >> 7);
                if (t >= a.frame_stride) continue;
                if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR) cur.ob[static_cast<int64_t>(m) * a.frame_stride + t] = 0.0f;
                else cur.ob[static_cast<int64_t>(t) * (kFastGroups * kGroup) + m] = 0.0f;
            }
            if (tid == 0) qslot[par] = grab();
            __syncthreads();
            tl = tl_n;
            tl_n = __builtin_amdgcn_readfirstlane(qslot[par]);
            par ^= 1;
            if (tl < total_tiles) { cur = tile_info(tl); if (AHEAD && cur.stage) fetch(cur); }
            continue;
        }
        if (!AHEAD) fetch(cur);                            // (AHEAD: issued during the previous tile's store phase)
        stage(cur);
        V4_STAMP(0);
        __syncthreads();                                   // B1: the tile's samples are staged
        V4_STAMP(1);
        LanePk v;
        {
            FA_V4_LANE();
            float4 w4[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) w4[q] = reinterpret_cast<const float4 *>(wtab)[q * kGroup + l];
            load_frame_pair_eo<EZ>(area + (kPkHop / 2) * fbase + l, area + kV4HalfSamples + (kPkHop / 2) * fbase + l, v);
#pragma unroll
            for (int q = 0; q < 8; ++q) {   // window
                const f2 wa = f2{w4[q].x, w4[q].y}, wb = f2{w4[q].z, w4[q].w};
                if (!(EZ && q == 0)) { v.re[2 * q] = mul_lo(v.re[2 * q], wa); v.im[2 * q] = mul_hi(v.im[2 * q], wa); }
                if (!(EZ && q == 7)) { v.re[2 * q + 1] = mul_lo(v.re[2 * q + 1], wb); v.im[2 * q + 1] = mul_hi(v.im[2 * q + 1], wb); }
            }
            // inter-pass twiddles: all 15 reads issued here, behind the window products (whose 32 registers they take over) — left to
            // the scheduler they sit right in front of their uses, eight exposed LDS round trips per tile and wavefront
            f2 tw1[16];
#pragma unroll
            for (int q = 0; q < 8; ++q) { const v4f t = lds_ld16(t1tab + l * kV4T1Stride + 4 * q); tw1[2 * q] = f2{t.x, t.y}; tw1[2 * q + 1] = f2{t.z, t.w}; }
            __builtin_amdgcn_sched_barrier(0);
            fft16(v);
#pragma unroll
            for (int k1 = 1; k1 < 16; ++k1) cmul_w(v.re[k1], v.im[k1], tw1[k1 - 1]);
        }
        // The next tile: requested at the end of the first pass (one lane), first touched before B3.  Inline assembly, because atomicAdd() is lowered to a
        // wave-aggregated form whose result is broadcast with v_readfirstlane right away: an s_waitcnt vmcnt(0) behind the atomic,
        // i.e. its whole round trip (~2.5 k cycles) in front of the pass of wavefront 0, with the other wavefronts waiting at B2.
        unsigned long long got = 0;
        if (tid == 0) {
            const unsigned long long one = 1;
            asm volatile("global_atomic_add_x2 %0, %1, %2, off sc0" : "=&v"(got) : "v"(a.queue), "v"(one) : "memory");
        }
        V4_STAMP(2);
        __syncthreads();                                   // B2: every wavefront holds its frames; the area becomes the regions
        V4_STAMP(3);
        TileInfo nxt{};
        nxt.stage = false;
        if (tl_n < total_tiles) { nxt = tile_info(tl_n); if (nxt.stage) fetch(nxt); }   // in flight during the second pass
        V4_FINE(1);
        {
            FA_V4_LANE();
            f2 *P2 = reinterpret_cast<f2 *>(__builtin_assume_aligned(area + grp * kV4RegionFloats, 8));
            auto put = [&](const f2 (&c)[16]) {
#pragma unroll
                for (int k1 = 0; k1 < 16; ++k1) P2[k1 * kV4EStride + l] = c[k1];
            };
            auto get = [&](f2 (&c)[16]) {
#pragma unroll
                for (int q = 0; q < 8; ++q) { const v4f t = lds_ld16(reinterpret_cast<const float *>(P2 + l * kV4EStride) + 4 * q); c[2 * q] = f2{t.x, t.y}; c[2 * q + 1] = f2{t.z, t.w}; }
            };
            put(v.re);   // LDS operations of one wavefront complete in program order: write re, read re, write im (over re), read im
            get(v.re);
            put(v.im);
            get(v.im);
            V4_FINE(3);
            // recombination twiddles: read before the pass (the stores into the region below may alias the table as far as the
            // compiler knows, so it would read each one right in front of its use: eight more exposed round trips)
            f2 tw2[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const v4f t = lds_ld16(t2tab + l * kV4T2Stride + 4 * q); tw2[2 * q] = f2{t.x, t.y}; tw2[2 * q + 1] = f2{t.z, t.w}; }
            __builtin_amdgcn_sched_barrier(0);
            fft16(v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // Z[256 - (l + 16 j)]: lane (16 - l) & 15, register 15 - j (lane 0: own (16 - j) & 15)
                const f2 qr = partner_or(v.re[15 - j], v.re[(16 - j) & 15]), qi = partner_or(v.im[15 - j], v.im[(16 - j) & 15]);
                f2 plo, phi;
                pair_power4(v.re[j], v.im[j], qr, qi, tw2[j], plo, phi);
                P2[l + 16 * j] = plo;
                P2[kHalf - (l + 16 * j)] = phi;
            }
            V4_FINE(5);
            if (l == 0) P2[128] = 4.0f * (v.re[8] * v.re[8] + v.im[8] * v.im[8]);  // k = 128: X = conj(Z[128])
            f2 acc[kFastGroups];
            const f2 *P[kFastGroups];
            int mlo_now[(kFastGroups + 2) / 3];   // opaque copies: as loop invariants the 8 unpacked offsets are hoisted out of the tile loop and spilled
#pragma unroll
            for (int i = 0; i < (kFastGroups + 2) / 3; ++i) { mlo_now[i] = mlo[i]; asm volatile("" : "+v"(mlo_now[i])); }
#pragma unroll
            for (int i = 0; i < kFastGroups; ++i) {
                acc[i] = f2{0.0f, 0.0f};
                P[i] = P2 + ((mlo_now[i / 3] >> (10 * (i % 3))) & 1023);
            }
            constexpr int kSplit = fast_slot_base(6) & ~1;
            {
                f2 w[kSplit / 2], pb[kSplit];
#pragma unroll
                for (int sp = 0; sp < kSplit / 2; ++sp) w[sp] = lds_ld8(reinterpret_cast<const f2 *>(mw) + sp * kGroup + l);
#pragma unroll
                for (int s = 0; s < kSplit; ++s) constexpr_for_slot(s, [&](const int i, const int j) { pb[s] = lds_ld8(P[i] + j); });
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
                for (int sp = 0; sp < (kRest + 1) / 2; ++sp) w[sp] = lds_ld8(reinterpret_cast<const f2 *>(mw) + (kSplit / 2 + sp) * kGroup + l);
#pragma unroll
                for (int s = kSplit; s < kFastSlots; ++s) constexpr_for_slot(s, [&](const int i, const int j) { pb[s - kSplit] = lds_ld8(P[i] + j); });
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = kSplit; s < kFastSlots; ++s)
                    constexpr_for_slot(s, [&](const int i, const int) {
                        acc[i] = (s & 1) ? fma_hi(pb[s - kSplit], w[(s - kSplit) / 2], acc[i]) : fma_lo(pb[s - kSplit], w[(s - kSplit) / 2], acc[i]);
                    });
            }
            // log (:542-549) and the group's 128 x 2 values over its own region (all of its reads are issued; LDS operations of
            // a wavefront complete in order): mel m at slot (m + 4 c) & 127, c = frame quad of the group
            __builtin_amdgcn_sched_barrier(0);
            V4_FINE(7);
            const float add_floor = CLAMPED ? 0.0f : a.log_floor, clamp_floor = a.log_floor;
            f2 *outp = P2 + l + 4 * (grp >> 1);   // slot m + 4 c: at most 127 + 28 < 272, no wrap
#pragma unroll
            for (int i = 0; i < kFastGroups; ++i) {
                constexpr float kLn2 = 0.693147180559945309f;
                const f2 x = acc[i] + add_floor;
                f2 val;
                val.x = __builtin_amdgcn_logf(CLAMPED ? fmaxf(x.x, clamp_floor) : x.x);   // additive: acc + floor > 0 already
                val.y = __builtin_amdgcn_logf(CLAMPED ? fmaxf(x.y, clamp_floor) : x.y);
                outp[16 * i] = val * kLn2;
            }
        }
        if (tid == 0) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(got) : : "memory");   // the compiler does not track the assembly's load counter
            qslot[par] = static_cast<int>(got - a.queue_base);
        }
        V4_STAMP(4);
        __syncthreads();                                   // B3: the log-mel tile is complete
        V4_STAMP(5);
        const int tl_next = __builtin_amdgcn_readfirstlane(qslot[par]);
        par ^= 1;
        const f2 *R = reinterpret_cast<const f2 *>(area);
        constexpr int kRegF2 = kV4RegionFloats / 2;
        const bool full_tile = cur.t0 + kTileFrames <= cur.T && cur.t0 + kTileFrames <= a.frame_stride;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR && full_tile) {
#pragma unroll
            for (int it = 0; it < kFastGroups * kGroup * (kTileFrames / 4) / kThreads; ++it) {
                const int idx = tid + kThreads * it, m = idx >> 3, c = idx & 7, slot = m + 4 * c;
                const f2 A = R[(2 * c) * kRegF2 + slot], B = R[(2 * c + 1) * kRegF2 + slot];   // frames (4c, 4c + 2) and (4c + 1, 4c + 3)
                *reinterpret_cast<float4 *>(cur.ob + static_cast<int64_t>(m) * a.frame_stride + cur.t0 + 4 * c) = make_float4(A.x, B.x, A.y, B.y);
            }
        } else if (LAYOUT == FA_MEL_LAYOUT_MEL_MAJOR) {
            for (int idx = tid; idx < kFastGroups * kGroup * (kTileFrames / 4); idx += kThreads) {
                const int m = idx >> 3, c = idx & 7, slot = m + 4 * c, t = cur.t0 + 4 * c;
                if (t >= a.frame_stride) continue;
                const f2 A = R[(2 * c) * kRegF2 + slot], B = R[(2 * c + 1) * kRegF2 + slot];
                const float e[4] = {A.x, B.x, A.y, B.y};
                float *dst = cur.ob + static_cast<int64_t>(m) * a.frame_stride + t;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (t + q < a.frame_stride) dst[q] = t + q < cur.T ? e[q] : 0.0f;   // padValue (:39) for t >= T
            }
        } else {
            for (int idx = tid; idx < kTileFrames * kFastGroups * kGroup; idx += kThreads) {
                const int f = idx >> 7, m = idx & 127, t = cur.t0 + f;
                if (t >= a.frame_stride) continue;
                const int r = f & 7, g = 4 * (f >> 3) + 2 * (r >> 2) + (r & 1);   // group holding frame f, component (r >> 1) & 1
                float val = 0.0f;
                if (t < cur.T) { const f2 p = R[g * kRegF2 + m + 4 * (g >> 1)]; val = ((r >> 1) & 1) ? p.y : p.x; }
                cur.ob[static_cast<int64_t>(t) * (kFastGroups * kGroup) + m] = val;   // :451
            }
        }
        V4_STAMP(6);
        __syncthreads();                                   // B4: the regions are free for the next tile's samples
        V4_STAMP(7);
        cur = nxt;
        tl = tl_n;
        tl_n = tl_next;
    }
    if (a.prof && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) {
        for (int i = 0; i < 8; ++i) atomicAdd(&a.prof[8 + i], t_seg[i]);
        atomicAdd(&a.prof[7], static_cast<unsigned long long>(n_done));
        atomicAdd(&a.prof[0], clock64() - t_begin);          // shader-clock ticks and 100 MHz ticks of the same interval:
        atomicAdd(&a.prof[1], wall_clock64() - w_begin);     // their ratio is the clock the kernel actually ran at
    }
    if (a.prof && threadIdx.x == 0) {   // spread of workgroup start / end times (100 MHz ticks): late starters = workgroups that were not resident at launch
        atomicMin(&a.prof[2], w_begin); atomicMax(&a.prof[3], w_begin);
        const unsigned long long w_end = wall_clock64();
        atomicMin(&a.prof[4], w_end); atomicMax(&a.prof[5], w_end);
        if (blockIdx.x < 8192) reinterpret_cast<unsigned *>(a.prof + 16)[blockIdx.x] = static_cast<unsigned>(w_end - w_begin);   // per-workgroup duration
    }
#undef V4_STAMP
#undef V4_STAMP_
#undef V4_FINE
#undef FA_V4_LANE
}
