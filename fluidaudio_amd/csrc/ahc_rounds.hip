// ahc_rounds.hip — kernels of ONE linkage problem: the single-problem builds of the round, the one-block form, records, heights, adoption, and their
// launchers (ahc_launch.h; the host side: ahc_rounds_host.hip; ahc_ws.h: the map).
#include "ahc_round_body.h"
#include "ahc_launch.h"

using namespace fa_ahc;

namespace {
// Exact heights from the stored centroids, the reference's summation order, then sqrt
// (cluster_result::sqrt, FastClusterWrapper.cpp:128-130).
__global__ void ahc_heights(Ws w) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= w.N - 1) return;
    double *z = w.Z + static_cast<size_t>(s) * 4;
    const double *ca = w.C + static_cast<size_t>(z[0]) * w.d, *cb = w.C + static_cast<size_t>(z[1]) * w.d;
    double sum = 0.0;
    for (int k = 0; k < w.d; ++k) {
        const double diff = __dsub_rn(ca[k], cb[k]);
        sum = __dadd_rn(sum, __dmul_rn(diff, diff));
    }
    if (sum != sum) w.flags[0] = 1;
    z[2] = __dsqrt_rn(sum);
}

}  // namespace

// ---- adopting a clustering in progress (prob_adopt): what the start-up leaves for the rounds, from a matrix some of whose slots are dead already
namespace {
// Row minimum, lowest-slot argmin and second minimum of every live row over its LIVE columns (the start-up's ahc_row_minima reads a fresh matrix whose dead
// columns hold +inf; here merged-away slots hold whatever their last row was).  One workgroup per row.  Every entry is read as the rounds read it (pair_entry
// under the sym_limit ahc_adopt_state has just written): the column copies of the newest node may be stale (ahc_rom.hip, the hand-over).
__global__ __launch_bounds__(kBlk) void ahc_adopt_rows(Ws w) {
    __shared__ double s_val[kWaves], s_second[kWaves];
    __shared__ int s_idx[kWaves];
    __shared__ int s_win;
    const int i = blockIdx.x, ni = w.node[i], sym_limit = w.state[0].sym_limit;
    double v = dinf(), v2 = dinf();
    int ix = INT_MAX;
    if (ni != kDead) {
        for (int x = threadIdx.x; x < w.Np; x += kBlk) {
            const int nx = w.node[x];
            const double m = (x != i && nx != kDead) ? pair_entry(w.M, w.Np, i, ni, x, nx, sym_limit) : dinf();
            if (m < v) { v2 = v; v = m; ix = x; }   // x ascending per thread: the lowest index of equal values is kept
            else if (m < v2) v2 = m;
        }
    }
    const double mine = v;
    const int mine_ix = ix;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(ix, off);
        if (lt2(ov, oi, v, ix)) { v = ov; ix = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_val[threadIdx.x >> 6] = v; s_idx[threadIdx.x >> 6] = ix; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kWaves; ++wv) if (lt2(s_val[wv], s_idx[wv], v, ix)) { v = s_val[wv]; ix = s_idx[wv]; }
        RowSt r; r.d1 = v; r.nn = ix == INT_MAX ? -1 : ix; r.nnnode = ix == INT_MAX ? -1 : w.node[ix];
        w.row[i] = r;
        s_win = ix;
    }
    __syncthreads();
    double c2 = mine_ix == s_win ? v2 : mine;   // the smallest entry that is not the winner's
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(c2, off); if (o < c2) c2 = o; }
    if ((threadIdx.x & 63) == 0) s_second[threadIdx.x >> 6] = c2;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kWaves; ++wv) if (s_second[wv] < c2) c2 = s_second[wv];
        w.e2[i] = c2;
    }
}
// the state record after `merges` merges, the window counters, and the dendrogram rows of the merges done (heights are filled by ahc_heights at the end)
__global__ void ahc_adopt_state(Ws w, const int merges, const double eps, const double *__restrict__ pair_a, const double *__restrict__ pair_b) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < merges) {
        const double a = pair_a[r], b = pair_b[r];
        double *z = w.Z + static_cast<size_t>(r) * 4;
        z[0] = a < b ? a : b; z[1] = a < b ? b : a; z[2] = 0.0;
        z[3] = w.sizes[w.N + r];                      // the size of the node this merge created (LinkageOutput::append, FastClusterWrapper.cpp:150-160)
    }
    if (r != 0) return;
    AhcState s{};
    s.mode = FA_AHC_MODE_AUTO;
    s.step = merges;
    for (int k = 0; k < kPend; ++k) { s.pend_row[k] = -1; s.pend_node[k] = -1; }
    s.prev_op = OP_NONE;
    s.n_points = w.N; s.rounds32 = 0;
    s.sym_limit = w.N + merges - 1;                   // every node below the newest has both copies of its pairs; the newest is read through its row (pair_entry)
    s.eps = eps;
    s.dmax_bits = w.state[0].dmax_bits; s.nmax_bits = w.state[0].nmax_bits;
    w.state[0] = s; w.state[1] = s;
    for (int i = 0; i < 4; ++i) { w.cnt[i].stale_key = ~0ULL; w.cnt[i].ncand = 0; w.cnt[i].npairs = 0; }
    w.flags[1] = 0; w.flags[3] = 0;                   // [0]: a NaN distance seen so far stays; [2]: the Gram start-up's
    for (int i = 0; i < 16; ++i) w.prof[i] = 0;
}
}  // namespace

// ---- launchers: each family is a table indexed by what ahc_route.h answered
namespace {
using RoundFn = void (*)(int, int, AhcState *, RecA *, int4 *, RecP *, unsigned, unsigned, unsigned, unsigned, Ws, const Ws *, const int2 *);
constexpr RoundFn kRoundSingle[route::kSingleKernels] = {   // in the order of route::SingleKernel
    ahc_round_t<false, false, 1, 1, true>, ahc_round_t<false, false, 1, 2, true>, ahc_round_t<false, false, 1, 3, true>, ahc_round_t<false, false, 1, 4, true>,
    ahc_round_t<false, true, 4>, ahc_round_t<false, false, 4>, ahc_round_t<false, true, 2>, ahc_round_t<false, false, 2>, ahc_round_t<false, true, 1>,
    ahc_round_t<false, false, 1, 1>, ahc_round_t<false, false, 1, 2>, ahc_round_t<false, false, 1, 3>, ahc_round_t<false, false, 1, 4>};
using BlockFn = void (*)(Ws, int);
using RecordsFn = void (*)(Ws);
constexpr int by_cpt(const int cpt) { return cpt == 4 ? 2 : cpt == 2 ? 1 : 0; }
constexpr BlockFn kSingleBlock[3] = {ahc_rounds_single_block<1>, ahc_rounds_single_block<2>, ahc_rounds_single_block<4>};
constexpr RecordsFn kRecords[3] = {ahc_records<1>, ahc_records<2>, ahc_records<4>};
}  // namespace

namespace fa_ahc {
void launch_round_single(hipStream_t st, const route::SingleKernel kernel, const int ph, const Ws &w, const RoundOffsets &o, const size_t lds) {
    hipLaunchKernelGGL(kRoundSingle[kernel], dim3(w.nblk), dim3(kBlk), lds, st, ph, w.nblk, w.state, w.recA, w.recI, w.recP, o.row, o.node, o.e2, o.flags, w,
                       static_cast<const Ws *>(nullptr), static_cast<const int2 *>(nullptr));
}
void round_single_lds(const route::SingleKernel kernel, const size_t lds) { kernel_lds(reinterpret_cast<const void *>(kRoundSingle[kernel]), lds); }
void launch_single_block(hipStream_t st, const int cpt, const Ws &w, const int rounds, const size_t lds) {
    hipLaunchKernelGGL(kSingleBlock[by_cpt(cpt)], dim3(1), dim3(kBlk), lds, st, w, rounds);
}
void single_block_lds(const int cpt, const size_t lds) { kernel_lds(reinterpret_cast<const void *>(kSingleBlock[by_cpt(cpt)]), lds); }
void launch_records(hipStream_t st, const int cpt, const Ws &w) { hipLaunchKernelGGL(kRecords[by_cpt(cpt)], dim3(w.nblk, 2), dim3(kBlk), 0, st, w); }
void launch_heights(hipStream_t st, const Ws &w) { hipLaunchKernelGGL(ahc_heights, dim3((w.N + 255) / 256), dim3(256), 0, st, w); }
void launch_adopt(hipStream_t st, const Ws &w, const int merges, const double eps, const double *pair_a, const double *pair_b) {
    hipLaunchKernelGGL(ahc_adopt_state, dim3(static_cast<unsigned>((std::max(merges, 1) + 255) / 256)), dim3(256), 0, st, w, merges, eps, pair_a, pair_b);
    hipLaunchKernelGGL(ahc_adopt_rows, dim3(w.Np), dim3(kBlk), 0, st, w);
}
}  // namespace fa_ahc
