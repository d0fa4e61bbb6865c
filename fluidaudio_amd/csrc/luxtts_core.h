// luxtts_core.h — the integers and the fp32 operation orders of the LuxTTS session (kernels: luxtts.hip, host code: luxtts_host.hip),
// restated from TTS/LuxTts/LuxTtsSynthesizer.swift:59-128,163-164,203-249,274-287, LuxTtsSolver.swift:11-50 and
// StyleTTS2/Pipeline/Sampler/StyleTTS2DiffusionSchedule.swift:49-73.  Plain C++: no HIP type appears here.  Every count is decided on
// the host before a launch (plan_item); tests/test_luxtts_cpu.py checks it through fa_luxtts_plan against a line-by-line restatement.
//
// The prompt's mean square.  vDSP_measqv leaves its summation order open, so the order is the library's definition: kRmsThreads
// accumulators; sample e of the (capped) prompt belongs to accumulator (e / 4) % kRmsThreads and every accumulator takes its samples in
// ascending order by acc = fmaf(x, x, acc) from 0; the 64 accumulators of a wavefront are folded by the butterfly acc += acc[lane ^ off],
// off = 32, 16, 8, 4, 2, 1 (commutative, so all lanes agree); the wavefronts are added in ascending order; the mean is that sum / float(n),
// rms = sqrtf(mean), gain = target / rms where rms < target (else 1).  mean_square() below runs exactly this on the host.
//
// The anchor-Euler update (anchor_euler): t, t_next are float(time step), omt = 1 - t and w0 = 1 - t_next in fp32;
// x1p = fmaf(v, omt, x); last step: x = x1p; else x0p = fmaf(v, -t, x); x = fmaf(x0p, w0, x1p * t_next).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FA_LUX_HD __host__ __device__ __forceinline__
#else
#define FA_LUX_HD inline
#endif

namespace fa {
namespace luxtts {

constexpr int kNfft = 1024;        // the radix-16 x radix-16 x radix-4 route; every other n_fft is refused
constexpr int kBins = kNfft / 2 + 1;
constexpr int kRmsThreads = 256;   // accumulators of the mean square: 4 wavefronts
constexpr int kMaxBuckets = 4;
constexpr int kMaxSteps = 16;
constexpr int kMaxMels = 128;

// status of an item: 0, or the first guard of the reference that refuses it, in the reference's order
enum Status : int32_t {
    kOk = 0,
    kNoSamples = 1,        // Synthesizer :59
    kBadSpeed = 2,         // :62
    kPromptTooShort = 3,   // :95  no mel frame
    kTooManyTokens = 4,    // :102 tokens + pad slot > max_tokens
    kTooManyFrames = 5,    // :112 features_length > max_frames
    kTextTooShort = 6,     // :118 gen_frames < 2
    kNoBucket = 7,         // :124
    kDegenerate = 8,       // Solver :37 avg < 1
    kSilentPrompt = 9,     // Synthesizer :78, known on the device only (the record of fa_luxtts_prompt_dev)
};

struct Geometry {
    int sample_rate, n_fft, hop, n_mels, max_tokens, max_frames, n_buckets, buckets[kMaxBuckets], out_hop, num_steps;
    int64_t max_prompt_samples;   // Int(max_prompt_seconds * Double(sample_rate))
    double t_shift;
    float log_floor, feat_scale, target_rms;
};

struct ItemPlan {
    int64_t samples;          // of the prompt, behind the cap
    int32_t prompt_frames, tokens, features_length, gen_frames, avg, bucket;
    int64_t sample_count;
    int32_t status;
};

// Synthesizer :59-128 and Solver :11-17,:33-40 for one item; prompt_tokens, text_tokens >= 1 (the entries refuse an empty token list)
inline ItemPlan plan_item(const Geometry &g, const int64_t prompt_samples, const int32_t prompt_tokens, const int32_t text_tokens, const float speed) {
    ItemPlan p{};
    auto refuse = [&p](const Status s) { p.status = s; return p; };
    if (prompt_samples < 1) return refuse(kNoSamples);
    if (!(speed > 0.0f)) return refuse(kBadSpeed);
    p.samples = prompt_samples < g.max_prompt_samples ? prompt_samples : g.max_prompt_samples;
    p.prompt_frames = static_cast<int32_t>((p.samples + g.hop / 2) / g.hop);
    if (p.prompt_frames < 1) return refuse(kPromptTooShort);
    p.tokens = prompt_tokens + text_tokens;
    if (static_cast<int64_t>(prompt_tokens) + text_tokens + 1 > g.max_tokens) return refuse(kTooManyTokens);
    const double generated = static_cast<double>(p.prompt_frames) / static_cast<double>(prompt_tokens) * static_cast<double>(text_tokens) / static_cast<double>(speed);
    const double up = ceil(generated);
    if (!(up <= 1e9)) return refuse(kTooManyFrames);   // beyond any frame budget (and Int() would trap on the reference)
    p.features_length = p.prompt_frames + static_cast<int32_t>(up);
    if (p.features_length > g.max_frames) return refuse(kTooManyFrames);
    p.gen_frames = p.features_length - p.prompt_frames;
    if (p.gen_frames < 2) return refuse(kTextTooShort);
    for (int i = 0; i < g.n_buckets && !p.bucket; ++i)
        if (g.buckets[i] >= p.gen_frames) p.bucket = g.buckets[i];
    if (!p.bucket) return refuse(kNoBucket);
    p.avg = p.features_length / p.tokens;
    if (p.avg < 1) return refuse(kDegenerate);
    const int64_t want = static_cast<int64_t>(p.gen_frames - 1) * g.out_hop, have = static_cast<int64_t>(p.bucket - 1) * g.out_hop;
    p.sample_count = want < have ? want : have;
    return p;
}

// what a refused item keeps: nothing runs for it and its slab rows are zeros
inline ItemPlan refused(ItemPlan p) {
    if (p.status != kOk) { const int32_t s = p.status; p = ItemPlan{}; p.status = s; }
    return p;
}

// Solver :21-26
inline double time_step(const Geometry &g, const int i) {
    const double u = static_cast<double>(i) / static_cast<double>(g.num_steps);
    return g.t_shift * u / (1.0 + (g.t_shift - 1.0) * u);
}

// Solver :32-50 as a function of the frame: the embedding row frame f copies
FA_LUX_HD int token_row(const int f, const int tokens, const int avg) { return f < tokens * avg ? f / avg : tokens; }

// ---- the mean square's order (see the head of this file)
inline float mean_square(const float *x, const int64_t n) {
    float acc[kRmsThreads];
    for (int t = 0; t < kRmsThreads; ++t) acc[t] = 0.0f;
    for (int64_t e = 0; e < n; ++e) { float &a = acc[(e / 4) % kRmsThreads]; a = fmaf(x[e], x[e], a); }
    float total = 0.0f;
    for (int w = 0; w < kRmsThreads / 64; ++w) {
        float lane[64], next[64];
        for (int l = 0; l < 64; ++l) lane[l] = acc[64 * w + l];
        for (int off = 32; off >= 1; off >>= 1) {
            for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off];
            for (int l = 0; l < 64; ++l) lane[l] = next[l];
        }
        total = w == 0 ? lane[0] : total + lane[0];
    }
    return total / static_cast<float>(n);
}

struct Loudness { float mean_square, rms, gain; int32_t status; };
FA_LUX_HD Loudness loudness_of(const float mean_sq, const float target) {
    Loudness r;
    r.mean_square = mean_sq;
    r.rms = sqrtf(mean_sq);
    r.status = r.rms > 0.0f ? kOk : kSilentPrompt;                         // Synthesizer :78
    r.gain = r.rms > 0.0f && r.rms < target ? target / r.rms : 1.0f;     // :81-82; target 0 switches the normalisation off
    return r;
}

// ---- the anchor-Euler update's order (Synthesizer :236-248)
struct StepTimes { float t, t_next, omt, w0; int32_t last; };
inline StepTimes step_times(const Geometry &g, const int step) {
    StepTimes s;
    s.t = static_cast<float>(time_step(g, step));
    s.t_next = static_cast<float>(time_step(g, step + 1));
    s.omt = 1.0f - s.t;
    s.w0 = 1.0f - s.t_next;
    s.last = step == g.num_steps - 1;
    return s;
}
FA_LUX_HD float anchor_euler(const float x, const float v, const StepTimes &s) {
    const float x1p = fmaf(v, s.omt, x);
    if (s.last) return x1p;
    const float x0p = fmaf(v, -s.t, x);
    return fmaf(x0p, s.w0, x1p * s.t_next);
}

// ---- the start noise as a counter (StyleTTS2DiffusionSchedule.swift:49-73): the k-th SplitMix64 output of a seed
FA_LUX_HD uint64_t splitmix_at(const uint64_t seed, const uint64_t k) {
    uint64_t z = (seed == 0 ? 0xdeadbeefcafebabeull : seed) + k * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
FA_LUX_HD double uniform_of(const uint64_t z) {
    const double u = static_cast<double>(z >> 11) / 9007199254740992.0;   // 2^53
    return u <= 0.0 ? 2.2250738585072014e-308 : u;                        // .leastNormalMagnitude
}
FA_LUX_HD float gaussian_at(const uint64_t seed, const uint64_t i) {
    const double u1 = uniform_of(splitmix_at(seed, 2 * i + 1)), u2 = uniform_of(splitmix_at(seed, 2 * i + 2));
    return static_cast<float>(sqrt(-2.0 * log(u1)) * cos(2.0 * 3.14159265358979323846 * u2));
}

}  // namespace luxtts
}  // namespace fa
