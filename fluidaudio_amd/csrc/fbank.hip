// fbank.hip — Kaldi fbank -> LFR -> CMVN for gfx950, batched over utterances: the front end FunASR's WavFrontend puts before
// Paraformer, SenseVoice, FSMN-VAD and CAM++ (the arithmetic is stated in include/fluidaudio_hip.h, section "Kaldi fbank").
//
// One workgroup (256 threads = 16 groups of 16 lanes) owns a tile of 32 consecutive frames of one utterance.
//   staging    the tile's (32 - 1) hop + win samples go from HBM to LDS once, 16 bytes per load, times the waveform scale;
//              neighbouring frames overlap by 1 - hop / win = 60 % and meet again only in LDS.
//   prologue   a group takes one frame per pass: lane l reads the positions 32 n1 + 2 l, + 1 (the radix-16 loader geometry of
//              mel_core.h, the window placed at position 0), the frame mean is the fixed-order reduction of fbank_core.h, the
//              pre-emphasis restarts inside the frame (left neighbour from LDS, less the same mean), the window is phase_a2's.
//   FFT        the radix-16 phases of mel_core.h: one LDS transpose, the Z[k] <-> Z[256 - k] exchange a DPP lane permutation.
//   bank       Kaldi's triangles are contiguous bin ranges: (first bin, bins, weights) per mel, held in LDS.
//   epilogue   every output element has exactly one source frame, so the group that computed frame t stores its n_mels
//              values into every (row, slot) of the stacked output that takes frame t (fbank_core.h: for_each_target), the
//              shift and scale applied in that store.  Rows >= R(b) are zero-filled by the utterance's workgroups, each a slice.
// After the staging barrier nothing synchronises across groups: all exchange is inside a 16-lane group of one wavefront.
#include "fbank_launch.h"

using namespace fa::fbank;
using namespace fa::melcore;

namespace {

// lane l <- lane (16 - l) & 15 inside every row of 16 lanes: row_mirror (l <- 15 - l), then row_ror:1 (l <- l - 1)
__device__ __forceinline__ float dpp_partner(const float x) {
    int v = __float_as_int(x);
    v = __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);
    v = __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, true);
    return __int_as_float(v);
}

__global__ __launch_bounds__(kThreads, 2) void fbank_kernel(const FbankArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *samples = smem;
    float *regions = samples + a.stage_alloc;
    int32_t *mtab = reinterpret_cast<int32_t *>(regions + kGroups * kRegionFloats);
    float *mw = reinterpret_cast<float *>(mtab + 2 * a.n_mels);

    const int tid = threadIdx.x;
    const int l = tid & (kGroup - 1);
    const int grp = tid >> 4;
    const int b = static_cast<int>(blockIdx.x / a.tiles_per_utt);
    const int q = static_cast<int>(blockIdx.x - static_cast<unsigned>(b) * a.tiles_per_utt);
    const int64_t base = a.offsets[b];
    const int64_t len = a.offsets[b + 1] - base;
    const int T = static_cast<int>(num_frames(len, a.win, a.hop));
    const int R = static_cast<int>(num_rows(T, a.lfr_m, a.lfr_n, a.tail));
    const float *x = a.pcm + base;
    float *ob = a.out + static_cast<int64_t>(b) * a.utt_stride;
    if (q == 0 && tid == 0 && a.rows) a.rows[b] = R;

    {   // rows R .. row_stride - 1 are one contiguous run of zeros: tile q of the utterance writes the q-th slice of it
        const int64_t zeros = static_cast<int64_t>(a.row_stride - R) * a.row_floats;
        const int64_t per = (zeros + a.tiles_per_utt - 1) / a.tiles_per_utt;
        const int64_t z0 = per * q, z1 = z0 + per < zeros ? z0 + per : zeros;
        float *zb = ob + static_cast<int64_t>(R) * a.row_floats;
        for (int64_t i = z0 + tid; i < z1; i += kThreads) zb[i] = 0.0f;
    }
    const int t0 = q * kTileFrames;
    if (t0 >= T) return;   // workgroup-uniform

    for (int i = tid; i < 2 * a.n_mels; i += kThreads) mtab[i] = a.mel_tab[i];
    for (int i = tid; i < a.n_weights; i += kThreads) mw[i] = a.mel_w[i];
    LaneConst kc;
    {
        Tables c;
        c.windowz = a.windowz;
        c.tw256 = reinterpret_cast<const float *>(a.tw256);
        c.tw512 = reinterpret_cast<const float *>(a.tw512);
        lane_const_init(l, c, kc);
    }
    // staging: the samples the tile's live frames cover, [n0, n0 + need), all inside the utterance by the definition of T
    const int live = T - t0 < kTileFrames ? T - t0 : kTileFrames;
    const int need = (live - 1) * a.hop + a.win;
    const int64_t n0 = static_cast<int64_t>(t0) * a.hop;
    for (int e = 4 * tid; e < need; e += 4 * kThreads) {
        float4 v;
        if (e + 3 < need) {
            v = *reinterpret_cast<const float4 *>(x + n0 + e);
        } else {
            v.x = x[n0 + e];
            v.y = e + 1 < need ? x[n0 + e + 1] : 0.0f;
            v.z = e + 2 < need ? x[n0 + e + 2] : 0.0f;
            v.w = 0.0f;
        }
        v.x *= a.wave_scale; v.y *= a.wave_scale; v.z *= a.wave_scale; v.w *= a.wave_scale;
        *reinterpret_cast<float4 *>(samples + e) = v;   // e + 3 < stage_alloc: stage_alloc is the largest `need` rounded up to 4
    }
    __syncthreads();

    float *Rg = static_cast<float *>(__builtin_assume_aligned(regions + grp * kRegionFloats, 8));
    const int n_mels = a.n_mels;
#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int f = pass * kGroups + grp;
        const int t = t0 + f;
        if (t >= T) continue;   // uniform inside the 16-lane group: everything below stays inside it
        const float *fs = samples + f * a.hop;
        Lane v;
        float left[16];   // the sample before re[n1]
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            const int j = 32 * n1 + 2 * l;
            v.re[n1] = j < a.win ? fs[j] : 0.0f;
            v.im[n1] = j + 1 < a.win ? fs[j + 1] : 0.0f;
            left[n1] = j < a.win ? fs[j > 0 ? j - 1 : 0] : 0.0f;   // Kaldi: y[0] = x[0] - c x[0]
        }
        float mean = 0.0f;
        if (a.remove_dc) {
            float s = lane_partial(v.re, v.im);
#pragma unroll
            for (int d = 1; d < kGroup; d <<= 1) s += __shfl_xor(s, d);
            mean = s / static_cast<float>(a.win);
        }
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            const int j = 32 * n1 + 2 * l;
            const float xr = v.re[n1] - mean, xi = v.im[n1] - mean, xl = left[n1] - mean;
            v.re[n1] = j < a.win ? xr - a.preemph * xl : 0.0f;
            v.im[n1] = j + 1 < a.win ? xi - a.preemph * xr : 0.0f;
        }
        phase_a2(l, v, kc, Rg);   // window, first radix-16 pass, transpose through the group's region
        phase_b1(l, Rg, v);
        float qr[8], qi[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // Z[256 - (l + 16 j)]: lane (16 - l) & 15, register 15 - j (lane 0: own (16 - j) & 15)
            const float pr = dpp_partner(v.re[15 - j]), pi = dpp_partner(v.im[15 - j]);
            qr[j] = l == 0 ? v.re[(16 - j) & 15] : pr;
            qi[j] = l == 0 ? v.im[(16 - j) & 15] : pi;
        }
        Power p;
        phase_c1v2(l, v, qr, qi, kc, p);
        // power bins at Rg + {0, 14, 28, 10}[frame of the wavefront]: regions are 578 = 2 (mod 32) floats apart, this puts the
        // two frames of a 32-lane LDS service group 16 banks apart
        float *PR = Rg + ((0x0a1c0e00u >> (8 * (grp & 3))) & 0xff);
        phase_c2(l, p, PR);
        float *O = Rg + kRegionOut;
        for (int m = l; m < n_mels; m += kGroup) {   // lane l owns the mels l, l + 16, ...
            const int packed = mtab[2 * m];
            const float *P = PR + (packed & 0xffff);
            const float *wgt = mw + mtab[2 * m + 1];
            const int cnt = packed >> 16;
            float acc = 0.0f;
            for (int j = 0; j < cnt; ++j) acc += wgt[j] * P[j];
            // log(max(e, floor)): the floor's own logarithm is the host's, so a silent frame gives the same bits everywhere
            O[m] = acc > a.log_floor ? logf(acc) : a.log_of_floor;
        }
        // the frame's values go straight to every (row, slot) that takes frame t; LDS operations of a wavefront complete in
        // program order, so the reads below see the writes above
        if (a.vec) {
            for (int c = 4 * l; c < n_mels; c += 4 * kGroup) {
                const float4 val = make_float4(O[c], O[c + 1], O[c + 2], O[c + 3]);
                for_each_target(t, T, R, a.lfr_m, a.lfr_n, [&](const int row, const int slot) {
                    const int j = slot * n_mels + c;
                    float4 y = val;
                    if (a.shift) { const float4 s = *reinterpret_cast<const float4 *>(a.shift + j); y.x += s.x; y.y += s.y; y.z += s.z; y.w += s.w; }
                    if (a.scale) { const float4 s = *reinterpret_cast<const float4 *>(a.scale + j); y.x *= s.x; y.y *= s.y; y.z *= s.z; y.w *= s.w; }
                    *reinterpret_cast<float4 *>(ob + static_cast<int64_t>(row) * a.row_floats + j) = y;
                });
            }
        } else {
            for (int c = l; c < n_mels; c += kGroup) {
                const float val = O[c];
                for_each_target(t, T, R, a.lfr_m, a.lfr_n, [&](const int row, const int slot) {
                    const int j = slot * n_mels + c;
                    float y = val;
                    if (a.shift) y += a.shift[j];
                    if (a.scale) y *= a.scale[j];
                    ob[static_cast<int64_t>(row) * a.row_floats + j] = y;
                });
            }
        }
    }
}

}  // namespace

namespace fa {
namespace fbank {

void launch(const FbankArgs &a, const int64_t grid, hipStream_t stream) {
    hipLaunchKernelGGL(fbank_kernel, dim3(static_cast<unsigned>(grid)), dim3(kThreads), lds_bytes(a), stream, a);
}

}  // namespace fbank
}  // namespace fa
