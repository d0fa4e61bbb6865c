// ahc_batch.hip — kernels that advance several linkage problems by the same round launch: the uniform-layout round, the block-map and the argument-table
// rounds, and their launchers (ahc_launch.h; the host side: ahc_batch_host.hip; ahc_ws.h: the map).
#include "ahc_round_body.h"
#include "ahc_launch.h"

using namespace fa_ahc;

namespace {
// ahc_round_uni: K problems in ONE launch without any look-up in front of the round (round 4).  The host lays the K workspaces out with the
// SAME layout (that of the largest problem; a smaller one simply has more dead padding slots) at a constant stride, so every array of
// problem k is the array of problem 0 + k * stride: the grid is (blocks, problems), the problem index is the workgroup id in y (an SGPR the
// hardware hands over), and the addresses of the round's first memory round trip are arithmetic on PRELOADED kernel arguments — the same
// zero scalar round trips as the single-problem kernel.  (ahc_round_args, the round-2 form: 154 scalar instructions and three dependent
// scalar-cache round trips — block -> problem search over 16 block ranges, then two batches of workspace fields out of a by-value array
// indexed by the problem — in front of its first request: 11 us per round of 16 problems against 5.3 us for one.)  Only N differs per
// problem: it comes from the hot part of the problem's state, with the first batch of loads.
// arg 0 = (blocks << 2) | (round & 3), stride in 4 KB pages: 14 preloaded dwords like ahc_round_t.
template <int CPT, int KC = 4 / CPT>
__device__ __forceinline__ void ahc_round_uni_body(const unsigned nblk_ph, const unsigned stride_pages, AhcState *const state_, RecA *const recA_, int4 *const recI_,
                                                   RecP *const recP_, const unsigned off_row, const unsigned off_node, const unsigned off_e2, const unsigned off_flags,
                                                   const Ws &w_one) {
    const size_t sh = (static_cast<size_t>(blockIdx.y) * stride_pages) << 12;
    auto at = [sh](auto *p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char *>(p) + sh); };
    Ws w_ = w_one;
    const int nblk_ = static_cast<int>(nblk_ph >> 2);
    w_.nblk = nblk_; w_.Np = nblk_ * kBlk * CPT; w_.state = at(state_); w_.recA = at(recA_); w_.recI = at(recI_); w_.recP = at(recP_);
    char *base = reinterpret_cast<char *>(w_.state);
    w_.row = reinterpret_cast<RowSt *>(base + off_row); w_.node = reinterpret_cast<int *>(base + off_node);
    w_.e2 = reinterpret_cast<double *>(base + off_e2); w_.flags = reinterpret_cast<int *>(base + off_flags);
    ahc_round_body<true, false, CPT, KC>(w_, blockIdx.x, static_cast<int>(nblk_ph & 3u), sh);   // the host sends problems of more than 65 536 points elsewhere
}
#define FA_AHC_UNI_KERNEL(NAME, ATTR, CPT, KC)                                                                                                              \
    __global__ __launch_bounds__(kBlk) ATTR void NAME(const unsigned nblk_ph, const unsigned stride_pages, AhcState *const state_, RecA *const recA_,  \
                                                      int4 *const recI_, RecP *const recP_, const unsigned off_row, const unsigned off_node,           \
                                                      const unsigned off_e2, const unsigned off_flags, const Ws w_one) {                              \
        ahc_round_uni_body<CPT, KC>(nblk_ph, stride_pages, state_, recA_, recI_, recP_, off_row, off_node, off_e2, off_flags, w_one);                      \
    }
// one slot per thread at three register budgets (more co-resident workgroups per CU against spills; round 4) and the round-5 forms with 2 / 4 slots per
// thread (which one serves a batch: route::uniform_kernel)
FA_AHC_UNI_KERNEL(ahc_round_uni, , 1, 4)
FA_AHC_UNI_KERNEL(ahc_round_uni_w3, __attribute__((amdgpu_waves_per_eu(6, 6))), 1, 4)   // "w3" / "w4": the second and third budget
FA_AHC_UNI_KERNEL(ahc_round_uni_w4, __attribute__((amdgpu_waves_per_eu(8, 8))), 1, 4)
FA_AHC_UNI_KERNEL(ahc_round_uni_c2, , 2, 2)
FA_AHC_UNI_KERNEL(ahc_round_uni_c4, , 4, 1)
// the same with the block records a lane of the first reduction actually owns held in registers (round 6: a request for a record the lane does not own is
// not free, ahc_round_body): problems of up to 16 384 / 32 768 / 49 152 slots at one slot per thread, up to 32 768 slots at two
FA_AHC_UNI_KERNEL(ahc_round_uni_k1, , 1, 1)
FA_AHC_UNI_KERNEL(ahc_round_uni_k2, , 1, 2)
FA_AHC_UNI_KERNEL(ahc_round_uni_k3, , 1, 3)
FA_AHC_UNI_KERNEL(ahc_round_uni_c2k1, , 2, 1)

struct BatchArgs : RoundArgs {};   // the kernel's own name for its argument (a type of this unit, like the kernel)

template <bool BIG>
__global__ __launch_bounds__(kBlk) void ahc_round_args(const BatchArgs a, const int ph) {
    const int b = blockIdx.x;
    int prob = 0;
#pragma unroll
    for (int k = 1; k < kArgProblems; ++k) prob += (k < a.count && b >= a.first_block[k]) ? 1 : 0;
    ahc_round_body<false, BIG>(a.w[prob], b - a.first_block[prob], ph);
}

}  // namespace

// ---- launchers: each family is a table indexed by what ahc_route.h answered
namespace {
using UniFn = void (*)(unsigned, unsigned, AhcState *, RecA *, int4 *, RecP *, unsigned, unsigned, unsigned, unsigned, Ws);
constexpr UniFn kRoundUni[route::kUniKernels] = {   // in the order of route::UniKernel
    ahc_round_uni, ahc_round_uni_w3, ahc_round_uni_w4, ahc_round_uni_c2, ahc_round_uni_c4, ahc_round_uni_k1, ahc_round_uni_k2, ahc_round_uni_k3, ahc_round_uni_c2k1};
using MapFn = void (*)(int, int, AhcState *, RecA *, int4 *, RecP *, unsigned, unsigned, unsigned, unsigned, Ws, const Ws *, const int2 *);
constexpr MapFn kRoundMap[2] = {ahc_round_t<true, false>, ahc_round_t<true, true>};   // by BIG
using ArgsFn = void (*)(BatchArgs, int);
constexpr ArgsFn kRoundArgs[2] = {ahc_round_args<false>, ahc_round_args<true>};
}  // namespace

namespace fa_ahc {
void launch_round_map(hipStream_t st, const bool big, const int ph, const int grid, const Ws *d_table, const int2 *d_map, const size_t lds) {
    hipLaunchKernelGGL(kRoundMap[big], dim3(grid), dim3(kBlk), lds, st, ph, 0, static_cast<AhcState *>(nullptr), static_cast<RecA *>(nullptr), static_cast<int4 *>(nullptr),
                       static_cast<RecP *>(nullptr), 0u, 0u, 0u, 0u, Ws{}, d_table, d_map);
}
void round_map_lds(const bool big, const size_t lds) { kernel_lds(reinterpret_cast<const void *>(kRoundMap[big]), lds); }
void launch_round_args(hipStream_t st, const bool big, const int ph, const int grid, const RoundArgs &a, const size_t lds) {
    hipLaunchKernelGGL(kRoundArgs[big], dim3(grid), dim3(kBlk), lds, st, BatchArgs{a}, ph);
}
void round_args_lds(const bool big, const size_t lds) { kernel_lds(reinterpret_cast<const void *>(kRoundArgs[big]), lds); }
void launch_round_uni(hipStream_t st, const route::UniKernel kernel, const int ph, const int grid_y, const Ws &w0, const RoundOffsets &o, const unsigned stride_pages,
                      const size_t lds) {
    const unsigned a0 = (static_cast<unsigned>(w0.nblk) << 2) | static_cast<unsigned>(ph & 3);
    hipLaunchKernelGGL(kRoundUni[kernel], dim3(static_cast<unsigned>(w0.nblk), static_cast<unsigned>(grid_y)), dim3(kBlk), lds, st, a0, stride_pages, w0.state, w0.recA,
                       w0.recI, w0.recP, o.row, o.node, o.e2, o.flags, w0);
}
void round_uni_lds(const route::UniKernel kernel, const size_t lds) { kernel_lds(reinterpret_cast<const void *>(kRoundUni[kernel]), lds); }
}  // namespace fa_ahc
