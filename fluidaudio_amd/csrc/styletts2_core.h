// styletts2_core.h — the integers and the fp32 operation orders of the StyleTTS2 session (kernels: styletts2.hip, host code:
// styletts2_host.hip), restated from TTS/StyleTTS2/Pipeline/Preprocess/StyleTTS2MelExtractor.swift:77-84,226-250,
// Synthesize/StyleTTS2Synthesizer.swift:41-53,127-132, StyleTTS2GlueOps.swift:23-46,147-161, Sampler/StyleTTS2DiffusionSchedule.swift:16-35
// and Assets/StyleTTS2ModelStore.swift:200-205.  Plain C++: no HIP type appears here.  Every count is decided on the host before a launch
// (plan_item); tests/test_styletts2_cpu.py checks it through fa_styletts2_plan against a line-by-line restatement.
//
// The blend (blend_of): oma = 1 - a in fp32; p = a * x and q = oma * y are two rounded products; the result is p + q.  No contraction.
//
// A token's duration (duration_of): the float32 sum over c ascending, from 0, of 1 / (1 + expf(-x[c])) with the accurate expf and the
// correctly rounded division, then round_duration: half away from zero, at least 1 (a NaN sum gives 1).
//
// The seeded Gaussian stack is LuxTTS's per-element function (luxtts_core.h: gaussian_at), the same StyleTTS2NoiseSource as a counter.
#pragma once
#include <math.h>
#include <stdint.h>

#include "luxtts_core.h"   // gaussian_at

#if defined(__HIPCC__)
#define FA_ST2_HD __host__ __device__ __forceinline__
#else
#define FA_ST2_HD inline
#endif

namespace fa {
namespace styletts2 {

using fa::luxtts::gaussian_at;

constexpr int kNfft = 2048;        // run as a 1024-point complex transform (16 x 16 x 4); every other n_fft is refused
constexpr int kHalf = kNfft / 2;
constexpr int kBins = kNfft / 2 + 1;
constexpr int kStyle = 256;        // s_pred / ref_s; the halves are kStyle / 2
constexpr int kMaxBuckets = 4;
constexpr int kMaxTokens = 256;    // the start table of an item lives in LDS
constexpr int kMaxChannels = 64;   // of the duration logits
constexpr int kMaxMels = 128;

// status of an item: 0, or what refuses it
enum Status : int32_t {
    kOk = 0,
    kNoTokens = 1,         // an empty token list (TextCleaner always emits the pad token)
    kTextTooLong = 2,      // Synthesizer :51, ModelStore :204: beyond the largest bucket
    kClipTooLong = 3,      // the reference clip has more frames than the session's mel rows hold
    kTooManyFrames = 4,    // known after the durations only: the item's total passes the session's frame capacity
};

struct Geometry {
    int n_fft, win, hop, n_mels, filter_rate, max_ref_frames, default_tokens, n_buckets, buckets[kMaxBuckets], style_dim, diffusion_steps;
    int d_channels, asr_channels, max_frames, tail_trim;
    float log_eps, log_mean, log_std;
};

struct ItemPlan {
    int64_t samples;
    int32_t ref_frames, tokens, bucket, status;
};

// MelExtractor :79-84 on the reflect-padded clip: (n + n_fft - n_fft) / hop + 1; an empty clip is n_fft zeros, one frame
inline int64_t ref_frames_of(const Geometry &g, const int64_t samples) { return samples / g.hop + 1; }

// Synthesizer :45-53 with ModelStore.resolveBucket; 0: no bucket holds the tokens
inline int bucket_of(const Geometry &g, const int tokens) {
    if (tokens <= g.default_tokens) return g.default_tokens;
    for (int i = 0; i < g.n_buckets; ++i)
        if (tokens <= g.buckets[i]) return g.buckets[i];
    return 0;
}

inline ItemPlan plan_item(const Geometry &g, const int64_t samples, const int32_t tokens) {
    ItemPlan p{};
    if (tokens < 1) { p.status = kNoTokens; return p; }
    if (!bucket_of(g, tokens)) { p.status = kTextTooLong; return p; }
    if (ref_frames_of(g, samples) > g.max_ref_frames) { p.status = kClipTooLong; return p; }
    p.samples = samples; p.ref_frames = static_cast<int32_t>(ref_frames_of(g, samples)); p.tokens = tokens; p.bucket = bucket_of(g, tokens);
    return p;
}

// DiffusionSchedule :16-35; out has steps + 1 entries, the last one the 0 of F.pad
inline void karras_sigmas(const int steps, const double sigma_min, const double sigma_max, const double rho, double *out) {
    const double rho_inv = 1.0 / rho, denom = static_cast<double>(steps - 1);
    const double base_max = pow(sigma_max, rho_inv), base_min = pow(sigma_min, rho_inv);
    for (int i = 0; i < steps; ++i) {
        const double frac = static_cast<double>(i) / denom;
        out[i] = pow(base_max + frac * (base_min - base_max), rho);
    }
    out[steps] = 0.0;
}

// GlueOps :154-159
FA_ST2_HD float blend_of(const float a, const float x, const float y) {
#pragma clang fp contract(off)
    const float oma = 1.0f - a;
    const float p = a * x, q = oma * y;
    return p + q;
}

// GlueOps :36-44
FA_ST2_HD float sigmoid_term(const float x) { return 1.0f / (1.0f + expf(-x)); }
FA_ST2_HD int32_t round_duration(const float sum) { return sum >= 1.5f ? static_cast<int32_t>(roundf(sum)) : 1; }

// Synthesizer :127-132
inline int64_t trimmed_length(const Geometry &g, const int64_t len) { return len - (len < g.tail_trim ? len : g.tail_trim); }

}  // namespace styletts2
}  // namespace fa
