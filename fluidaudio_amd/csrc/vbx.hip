// vbx.hip — VBx variational-Bayes refinement of AHC labels (fp64) on gfx950.
//
// Replaces VBxClustering.refine / runVBx
// (reference: Sources/FluidAudio/Diarizer/Offline/Clustering/VBxClustering.swift:41-165,167-664).
// The reference's two DGEMMs per iteration (gamma^T rho: S x D <- T; rho alpha^T: T x S) and its
// row soft-max are small and skinny (T ~ 4e4, D = 128, S = #AHC clusters); they are evaluated
// here with deterministic reductions (fixed split of T, partials summed in a fixed order) so
// that repeated runs are bit-identical.  fp64 throughout, like the reference (cblas_d*, vvexp).
//
// Everything that crosses frames goes through ONE record per slice of the frame axis (kSplit = 64 slices): the slice's
// sum_t gamma[t][s] (rho[t][:], 1) and its sum of the per-frame log-likelihoods.  An iteration reads the 64 records in slice
// order (speaker statistics, pi, ELBO) and writes the 64 records of the new posteriors — so the same kernels run the whole
// problem on one device (vbx_host.hip: run) or a contiguous range of slices per device with one all-gather of the records per
// iteration in between (fa_vbx_shard_*: SURVEY §8(e) row 4, the iteration loop of VBxClustering.swift:301-661 sharded over
// T).  Both give the same bits: a shard computes exactly the records the single device computes for those slices.
#include "vbx_launch.h"

namespace fa {
namespace vbx {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}

// rho = X * sqrt(phi) (:242-265); G[t] = -0.5 (||x_t||^2 + D ln 2 pi) (:267-282).  One wave per frame.
__global__ void vbx_prepare(VbxWs w) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (t >= w.T) return;
    const int lane = threadIdx.x & 63;
    double ss = 0.0;
    for (int d = lane; d < w.D; d += 64) {
        const double x = w.X[t * w.D + d];
        w.rho[t * w.D + d] = x * sqrt(w.phi[d]);
        ss += x * x;
    }
    ss = wave_sum(ss);
    if (lane == 0) w.G[t] = -0.5 * (ss + static_cast<double>(w.D) * log(2.0 * M_PI));
}

// one-hot from labels -> softmax(7 * onehot) -> renormalise (:102-107, :190-237). One wave per frame.
__global__ void vbx_init_gamma(VbxWs w, const int32_t *labels, double smoothing) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (t >= w.T) return;
    const int lane = threadIdx.x & 63;
    int sp = labels[t];
    sp = sp > w.S - 1 ? w.S - 1 : sp;
    sp = sp < 0 ? 0 : sp;
    double *g = w.gamma + t * w.S;
    // row max of smoothing*onehot is `smoothing` (or 0 when smoothing < 0 is not used by the reference)
    const double mx = smoothing > 0.0 ? smoothing : 0.0;
    double sum = 0.0;
    for (int s = lane; s < w.S; s += 64) sum += exp((s == sp ? smoothing : 0.0) - mx);
    sum = wave_sum(sum);
    const double inv = 1.0 / sum;
    double sum2 = 0.0;
    for (int s = lane; s < w.S; s += 64) { const double v = exp((s == sp ? smoothing : 0.0) - mx) * inv; g[s] = v; sum2 += v; }
    sum2 = wave_sum(sum2);
    const double inv2 = 1.0 / sum2;
    for (int s = lane; s < w.S; s += 64) g[s] *= inv2;
}

__global__ void vbx_fill(double *p, int n, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// record[z][s][0..D] = sum over the z-th slice of frames of gamma[t][s] * (rho[t][:], 1)   (:312-325, :342-357)
// grid: (ceil((D+1)/64), ceil(S/4), slices owned), block 256 = 64 columns x 4 speakers.
__global__ __launch_bounds__(kThreads) void vbx_gt_rho(VbxWs w) {
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int s = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int z = w.z_lo + blockIdx.z;
    const FrameRange fr = slice_range(w.Tg, z);                     // global frames of the slice ...
    const int64_t t0 = fr.lo - w.t0g, t1 = fr.hi - w.t0g;           // ... as local rows
    if (s >= w.S || col > w.D) return;
    double acc = 0.0;
    // (unrolled: 16 independent loads in flight per thread; the additions keep their order — t ascending — so the sums keep their bits)
    if (col < w.D) {
#pragma unroll 8
        for (int64_t t = t0; t < t1; ++t) acc += w.gamma[t * w.S + s] * w.rho[t * w.D + col];
    } else {
#pragma unroll 8
        for (int64_t t = t0; t < t1; ++t) acc += w.gamma[t * w.S + s];
    }
    w.rec_out[blockIdx.z * w.stride + static_cast<int64_t>(s) * (w.D + 1) + col] = acc;
}

// last double of a slice record: the sum of the per-frame log-likelihoods of the slice (:623-630), fixed order.  One workgroup per slice.
__global__ __launch_bounds__(kThreads) void vbx_llpart(VbxWs w) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int z = w.z_lo + blockIdx.x;
    const FrameRange fr = slice_range(w.Tg, z);                     // global frames of the slice ...
    const int64_t t0 = fr.lo - w.t0g, t1 = fr.hi - w.t0g;           // ... as local rows
    double a = 0.0;
    for (int64_t t = t0 + tid; t < t1; t += kThreads) a += w.llrow[t];
    red[tid] = a;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) { if (tid < off) red[tid] += red[tid + off]; __syncthreads(); }
    if (tid == 0) w.rec_out[blockIdx.x * w.stride + w.stride - 1] = red[0];
}

// Per speaker: N_s, invL, alpha, phi term (:330-337, :370-387, :402-432).  One workgroup per speaker.
// mode 0: E-step quantities; mode 1: only pi[s] = sum_t gamma (used after the soft-max, :586-603).
__global__ __launch_bounds__(kThreads) void vbx_speaker(VbxWs w, int mode) {
    __shared__ double red[kThreads / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int D = w.D;
    if (mode == 1) {
        if (tid == 0) {
            double ns = 0.0;
            for (int z = 0; z < kSplit; ++z) ns += w.rec_in[z * w.stride + static_cast<int64_t>(s) * (D + 1) + D];
            w.pi[s] = ns;
        }
        return;
    }
    double ns = 0.0;
    for (int z = 0; z < kSplit; ++z) ns += w.rec_in[z * w.stride + static_cast<int64_t>(s) * (D + 1) + D];
    const double weight = (w.Fa / w.Fb) * ns;
    double acc = 0.0;
    for (int d = tid; d < D; d += kThreads) {
        double tmp = 0.0;
        for (int z = 0; z < kSplit; ++z) tmp += w.rec_in[z * w.stride + static_cast<int64_t>(s) * (D + 1) + d];
        const double den = 1.0 + weight * w.phi[d];
        const double il = 1.0 / (den > 1e-12 ? den : 1e-12);
        const double al = (tmp * il) * (w.Fa / w.Fb);
        w.invL[static_cast<int64_t>(s) * D + d] = il;
        w.alpha[static_cast<int64_t>(s) * D + d] = al;
        acc += (al * al + il) * w.phi[d];
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) { double v = 0.0; for (int i = 0; i < kThreads / 64; ++i) v += red[i]; w.phiT[s] = v; }
}

__global__ void vbx_logpi(VbxWs w) {  // log(max(pi, 1e-8)) (:498-514)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < w.S) { const double p = w.pi[s]; w.logpi[s] = log(p >= 1e-8 ? p : 1e-8); }
}

__device__ __forceinline__ void vbx_softmax_row(const VbxWs &w, int64_t t, double *g, double mx, int lane);

// E-step for one frame per wave: logP[s] = Fa (rho_t . alpha_s - phiT_s/2 + G_t) (:441-492),
// gamma = softmax(logP + log pi), llrow = logsumexp (:516-572).  S is processed in chunks of 64.
__global__ __launch_bounds__(kThreads) void vbx_estep(VbxWs w) {
    extern __shared__ double sm[];  // [4 waves][D] rho rows
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 4 + wave;
    if (t >= w.T) return;
    double *rt = sm + wave * w.D;
    for (int d = lane; d < w.D; d += 64) rt[d] = w.rho[t * w.D + d];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double *g = w.gamma + t * w.S;
    const double gt = w.G[t];
    double mx = -1.7976931348623157e308;
    for (int s = lane; s < w.S; s += 64) {
        const double *al = w.alpha + static_cast<int64_t>(s) * w.D;
        double dot = 0.0;
        for (int d = 0; d < w.D; ++d) dot += rt[d] * al[d];
        const double lp = ((dot + w.phiT[s] * -0.5) + gt) * w.Fa + w.logpi[s];
        g[s] = lp;  // staged in place; overwritten below
        mx = lp > mx ? lp : mx;
    }
    mx = wave_max(mx);
    vbx_softmax_row(w, t, g, mx, lane);
}

// gamma = softmax of the staged row, llrow = its logsumexp (:516-572); `mx` = the row maximum, known to every lane.
__device__ __forceinline__ void vbx_softmax_row(const VbxWs &w, const int64_t t, double *g, const double mx, const int lane) {
    double sum = 0.0;
    for (int s = lane; s < w.S; s += 64) { const double e = exp(g[s] - mx); g[s] = e; sum += e; }
    sum = wave_sum(sum);
    if (sum <= 0.0 || !isfinite(sum)) {
        for (int s = lane; s < w.S; s += 64) g[s] = 1.0 / static_cast<double>(w.S);
        if (lane == 0) w.llrow[t] = mx;
    } else {
        const double inv = 1.0 / sum;
        for (int s = lane; s < w.S; s += 64) g[s] *= inv;
        if (lane == 0) w.llrow[t] = mx + log(sum);
    }
}

// ---- many speakers (the hard sessions: AHC leaves hundreds of clusters, e.g. 597 at sigma = 0.041) ------------------------------------------
// Both contractions of an iteration are then real matrix products — gamma^T (rho, 1): [S x T_slice] x [T_slice x (D + 1)] per slice, and
// rho alpha^T: [T x D] x [D x S] — and the kernels above (one speaker per wavefront column / one frame per wavefront, every multiply-add fed by
// two global loads, the alpha rows of 64 lanes in 64 different lines) take 7.6 ms per iteration at S = 597, T = 43 200: 46 ms of the 300 ms
// of that recording.  Tiled form: 64 x 64 outputs per workgroup, 4 x 4 per thread, both operands k-major in LDS (16 k per stage), operands read
// as 16-byte pairs.  Every output is ONE accumulator fed in ascending k by fused multiply-adds with the same operands as the kernels above —
// the same bits, so single-device and sharded runs, and small-S and large-S code paths, agree on every record.  (fp64 vector FMA runs at the
// rate of the fp64 matrix core on this part; the MFMA form would have to keep this summation order to keep the records' bits and does not.)
constexpr int kVT = 64, kVK = 16, kVPad = 2;

// record[z][s][0..D] for the slices owned; grid (ceil((D + 1) / 64), ceil(S / 64), z_n)
__global__ __launch_bounds__(kThreads) void vbx_gt_rho_tiled(VbxWs w) {
    __shared__ __attribute__((aligned(16))) double sa[kVK][kVT + kVPad], sb[kVK][kVT + kVPad];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;   // tx: column quad, ty: speaker quad
    const int c0 = blockIdx.x * kVT, s0 = blockIdx.y * kVT;
    const int z = w.z_lo + blockIdx.z;
    const FrameRange fr = slice_range(w.Tg, z);                     // global frames of the slice ...
    const int64_t t0 = fr.lo - w.t0g, t1 = fr.hi - w.t0g;           // ... as local rows
    const int D = w.D, S = w.S;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int64_t k0 = t0; k0 < t1; k0 += kVK) {
        for (int e = tid; e < kVK * kVT; e += kThreads) {
            const int kk = e / kVT, i = e % kVT;
            const int64_t t = k0 + kk;
            const bool in = t < t1;
            sa[kk][i] = in && s0 + i < S ? w.gamma[t * S + s0 + i] : 0.0;
            const int col = c0 + i;
            sb[kk][i] = !in ? 0.0 : (col < D ? w.rho[t * D + col] : (col == D ? 1.0 : 0.0));
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kVK; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = sa[kk][4 * ty + r]; b[r] = sb[kk][4 * tx + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int sp = s0 + 4 * ty + r, col = c0 + 4 * tx + c;
            if (sp < S && col <= D) w.rec_out[blockIdx.z * w.stride + static_cast<int64_t>(sp) * (D + 1) + col] = acc[r][c];
        }
}

// logP staged in gamma: gamma[t][s] = Fa (rho_t . alpha_s - phiT_s / 2 + G_t) + log pi_s; grid (ceil(S / 64), ceil(T / 64))
__global__ __launch_bounds__(kThreads) void vbx_logits_tiled(VbxWs w) {
    __shared__ __attribute__((aligned(16))) double sa[kVK][kVT + kVPad], sb[kVK][kVT + kVPad];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;   // tx: speaker quad, ty: frame quad
    const int s0 = blockIdx.x * kVT;
    const int64_t f0 = static_cast<int64_t>(blockIdx.y) * kVT;
    const int D = w.D, S = w.S;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < D; k0 += kVK) {
        for (int e = tid; e < kVK * kVT; e += kThreads) {
            const int i = e / kVK, kk = e % kVK, d = k0 + kk;       // 16 consecutive d of one row: 128-byte segments
            sa[kk][i] = f0 + i < w.T && d < D ? w.rho[(f0 + i) * D + d] : 0.0;
            sb[kk][i] = s0 + i < S && d < D ? w.alpha[static_cast<int64_t>(s0 + i) * D + d] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kVK; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = sa[kk][4 * ty + r]; b[r] = sb[kk][4 * tx + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t t = f0 + 4 * ty + r;
        if (t >= w.T) continue;
        const double gt = w.G[t];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int sp = s0 + 4 * tx + c;
            if (sp < S) w.gamma[t * S + sp] = fma(fma(w.phiT[sp], -0.5, acc[r][c]) + gt, w.Fa, w.logpi[sp]);
        }
    }
}

// the row soft-max over the staged logits; one wavefront per frame
__global__ __launch_bounds__(kThreads) void vbx_softmax_rows(VbxWs w) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 4 + wave;
    if (t >= w.T) return;
    double *g = w.gamma + t * w.S;
    double mx = -1.7976931348623157e308;
    for (int s = lane; s < w.S; s += 64) { const double lp = g[s]; mx = lp > mx ? lp : mx; }
    mx = wave_max(mx);
    vbx_softmax_row(w, t, g, mx, lane);
}

// Scalars of one iteration: normalise pi (:605-621), log-likelihood (the slice sums in slice order) and
// ELBO = ll + Fb/2 * sum(log invL - invL - alpha^2 + 1) (:623-647).  One workgroup, fixed order.
__global__ __launch_bounds__(kThreads) void vbx_scalars(VbxWs w) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    double ll = 0.0;
    for (int z = 0; z < kSplit; ++z) ll += w.rec_in[z * w.stride + w.stride - 1];
    double b = 0.0;
    const int64_t n = static_cast<int64_t>(w.S) * w.D;
    for (int64_t i = tid; i < n; i += kThreads) { const double il = w.invL[i], al = w.alpha[i]; b += log(il) - il - al * al + 1.0; }
    red[tid] = b;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) { if (tid < off) red[tid] += red[tid + off]; __syncthreads(); }
    if (tid == 0) {
        w.scal[0] = ll + w.Fb * 0.5 * red[0];
        w.scal[1] = ll;
        double ps = 0.0;
        for (int s = 0; s < w.S; ++s) ps += w.pi[s];
        if (ps > 0.0 && isfinite(ps)) { const double inv = 1.0 / ps; for (int s = 0; s < w.S; ++s) w.pi[s] *= inv; }
        else for (int s = 0; s < w.S; ++s) w.pi[s] = 1.0 / static_cast<double>(w.S);
    }
}

__global__ void vbx_hard(VbxWs w, int32_t *hard) {  // first maximum (:144-146)
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= w.T) return;
    const double *g = w.gamma + t * w.S;
    int b = 0;
    for (int s = 1; s < w.S; ++s) if (g[b] < g[s]) b = s;
    hard[t] = b;
}

// VBxClustering.refine's catch block (VBxClustering.swift:136-141): when runVBx throws, the refinement does not fail — it returns
// gamma = initialGamma (the plain one-hot of the clamped initial labels, :100-104, NOT the smoothed start of runVBx), pi = 1/S, no ELBOs,
// and hardClusters = argmax of that gamma = the clamped labels (:144-146).  The stages behind it go on with those.
__global__ void vbx_degrade_kernel(const int32_t *__restrict__ labels, double *__restrict__ gamma, int32_t *__restrict__ hard, const int64_t T, const int32_t S) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= T * S) return;
    const int64_t t = i / S;
    const int32_t s = static_cast<int32_t>(i - t * S);
    int32_t l = labels[t];
    l = l < 0 ? 0 : (l > S - 1 ? S - 1 : l);   // max(0, min(cluster, speakerCount - 1)) (:102)
    gamma[i] = s == l ? 1.0 : 0.0;
    if (s == 0) hard[t] = l;
}

}  // namespace

void launch_prepare(hipStream_t st, const VbxWs &w, const int32_t *d_labels) {
    if (w.T > 0) {
        const unsigned wave_blocks = fa::grid_for(w.T, 4);
        hipLaunchKernelGGL(vbx_prepare, dim3(wave_blocks), dim3(kThreads), 0, st, w);
        hipLaunchKernelGGL(vbx_init_gamma, dim3(wave_blocks), dim3(kThreads), 0, st, w, d_labels, 7.0);
    }
    hipLaunchKernelGGL(vbx_fill, dim3(fa::grid_for(w.S, 256)), dim3(256), 0, st, w.pi, w.S, 1.0 / static_cast<double>(w.S));  // :239
}

void launch_records(hipStream_t st, const VbxWs &w) {
    if (w.z_n <= 0) return;
    if (w.tiled)
        hipLaunchKernelGGL(vbx_gt_rho_tiled, dim3(fa::grid_for(w.D + 1, kVT), fa::grid_for(w.S, kVT), w.z_n), dim3(kThreads), 0, st, w);
    else
        hipLaunchKernelGGL(vbx_gt_rho, dim3(fa::grid_for(w.D + 1, 64), fa::grid_for(w.S, 4), w.z_n), dim3(kThreads), 0, st, w);
    hipLaunchKernelGGL(vbx_llpart, dim3(w.z_n), dim3(kThreads), 0, st, w);
}

void launch_estep(hipStream_t st, const VbxWs &w) {
    hipLaunchKernelGGL(vbx_speaker, dim3(w.S), dim3(kThreads), 0, st, w, 0);
    hipLaunchKernelGGL(vbx_logpi, dim3(fa::grid_for(w.S, 256)), dim3(256), 0, st, w);
    if (w.T <= 0) return;
    if (w.tiled) {
        hipLaunchKernelGGL(vbx_logits_tiled, dim3(fa::grid_for(w.S, kVT), fa::grid_for(w.T, kVT)), dim3(kThreads), 0, st, w);
        hipLaunchKernelGGL(vbx_softmax_rows, dim3(fa::grid_for(w.T, kEstepWaves)), dim3(kThreads), 0, st, w);
    } else
        hipLaunchKernelGGL(vbx_estep, dim3(fa::grid_for(w.T, kEstepWaves)), dim3(kThreads), estep_lds_bytes(w.D), st, w);
}

void launch_finish(hipStream_t st, const VbxWs &w) {
    hipLaunchKernelGGL(vbx_speaker, dim3(w.S), dim3(kThreads), 0, st, w, 1);
    hipLaunchKernelGGL(vbx_scalars, dim3(1), dim3(kThreads), 0, st, w);
}

void launch_hard(hipStream_t st, const VbxWs &w, int32_t *d_hard) {
    if (w.T > 0) hipLaunchKernelGGL(vbx_hard, dim3(fa::grid_for(w.T, 256)), dim3(256), 0, st, w, d_hard);
}

void launch_degrade(hipStream_t st, const int32_t *d_labels, double *d_gamma, double *d_pi, int32_t *d_hard, const int64_t T, const int32_t S) {
    if (T > 0) hipLaunchKernelGGL(vbx_degrade_kernel, dim3(fa::grid_for(T * S, 256)), dim3(256), 0, st, d_labels, d_gamma, d_hard, T, S);
    hipLaunchKernelGGL(vbx_fill, dim3(fa::grid_for(S, 256)), dim3(256), 0, st, d_pi, S, 1.0 / static_cast<double>(S));   // :139
}

}  // namespace vbx
}  // namespace fa
