// fluidaudio.hpp — C++17 host-side mirror of the Swift types on FluidAudio's hot path, header-only, over the C ABI of
// include/fluidaudio_hip.h (libfluidaudio_hip.so).  Same names, argument meaning and error behaviour as the reference types
// (file:line cited per class), so that a C++ host — or a Swift shim generated from it — reads like the reference's callers.
// The reference's toolchain (Swift) is not in this image; its host language is compiled, hence this mirror is C++ (the
// Python package fluidaudio_amd/ is the ctypes twin used by the pytest suite).  No arithmetic lives here: guards that the
// reference performs before touching data are repeated so that the error behaviour is identical, everything else is a call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "fluidaudio_hip.h"

namespace fluidaudio {

struct Error : std::runtime_error {
    fa_status status;
    Error(fa_status st, const std::string &where, const char *detail = nullptr)
        : std::runtime_error(where + ": status " + std::to_string(static_cast<int>(st)) + (detail && *detail ? std::string(" (") + detail + ")" : "")), status(st) {}
};

// One device context (stream + scratch).  The reference's value types are "one instance per thread" (AudioMelSpectrogram.swift:48-57);
// the same holds for a Context.
class Context {
public:
    explicit Context(int device = 0) { const fa_status st = fa_ctx_create(device, nullptr, &h_); if (st != FA_SUCCESS) throw Error(st, "fa_ctx_create"); }
    ~Context() { fa_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    fa_ctx *handle() const { return h_; }
    void check(fa_status st, const char *where) const { if (st != FA_SUCCESS) throw Error(st, where, fa_ctx_last_error(h_)); }
    // Memory policy of the cached linkage workspace (N^2 * 8 bytes: 15 GB at 43 200 embeddings): keep at most `bytes` between calls /
    // refuse calls that need more than `bytes` (ALLOCATION_FAILURE = the reference's status 4: AHCClustering degrades to singletons) /
    // release everything cached now / what is cached (helper contexts of in-flight batches included).
    void setWorkspaceLimit(size_t bytes) { check(fa_ctx_set_workspace_limit(h_, bytes), "fa_ctx_set_workspace_limit"); }
    void setWorkspaceCap(size_t bytes) { check(fa_ctx_set_workspace_cap(h_, bytes), "fa_ctx_set_workspace_cap"); }
    void trim() { check(fa_ctx_trim(h_), "fa_ctx_trim"); }
    size_t workspaceBytes() const { return fa_ctx_workspace_bytes(h_); }
    // server start-up: the workspace of `recordings` linkage problems of up to nMax embeddings now, not inside the first request
    void reserve(size_t nMax, size_t d, int32_t recordings = 1) { check(fa_ctx_reserve(h_, nMax, d, recordings), "fa_ctx_reserve"); }
private:
    fa_ctx *h_ = nullptr;
};

// A set of devices for one host process (fa_pool): `lease()` hands the calling thread a context of a free device for the
// lifetime of the returned object — what a host with several OfflineDiarizerManager instances (one per worker thread, the
// reference's model: OfflineDiarizerManager.swift:270) needs to use every GPU; the *_sharded calls split one batch over all of them.
class DevicePool {
public:
    DevicePool() { const fa_status st = fa_pool_create(nullptr, 0, &h_); if (st != FA_SUCCESS) throw Error(st, "fa_pool_create"); }
    explicit DevicePool(const std::vector<int32_t> &devices) {
        const fa_status st = fa_pool_create(devices.data(), static_cast<int32_t>(devices.size()), &h_);
        if (st != FA_SUCCESS) throw Error(st, "fa_pool_create");
    }
    ~DevicePool() { fa_pool_destroy(h_); }
    DevicePool(const DevicePool &) = delete;
    DevicePool &operator=(const DevicePool &) = delete;
    int size() const { return fa_pool_size(h_); }
    fa_pool *handle() const { return h_; }
    struct Lease {
        fa_pool *pool; fa_ctx *ctx;
        Lease(fa_pool *p, fa_ctx *c) : pool(p), ctx(c) {}
        Lease(Lease &&o) noexcept : pool(o.pool), ctx(o.ctx) { o.ctx = nullptr; }
        Lease(const Lease &) = delete;
        Lease &operator=(const Lease &) = delete;
        ~Lease() { if (ctx) fa_pool_release(pool, ctx); }
        int device() const { return fa_ctx_device(ctx); }
    };
    Lease lease() { fa_ctx *c = nullptr; const fa_status st = fa_pool_acquire(h_, &c); if (st != FA_SUCCESS) throw Error(st, "fa_pool_acquire"); return Lease(h_, c); }
    // recordings across the devices (fa_ahc_linkage_many): row-major fp64 matrices in, scipy-layout dendrograms out, per-problem statuses
    std::vector<fa_status> linkageMany(const std::vector<std::vector<double>> &data, size_t d, std::vector<std::vector<double>> &dendrograms) {
        const size_t k = data.size();
        std::vector<const double *> dp(k);
        std::vector<double *> zp(k);
        std::vector<size_t> n(k);
        std::vector<int32_t> st(k, 0);
        dendrograms.assign(k, {});
        static double dummy[4];
        for (size_t i = 0; i < k; ++i) {
            n[i] = d ? data[i].size() / d : 0;
            dendrograms[i].assign(n[i] > 1 ? (n[i] - 1) * 4 : 0, 0.0);
            dp[i] = data[i].empty() ? dummy : data[i].data();
            zp[i] = dendrograms[i].empty() ? dummy : dendrograms[i].data();
        }
        (void)fa_ahc_linkage_many(h_, static_cast<int32_t>(k), dp.data(), n.data(), d, zp.data(), FA_AHC_MODE_AUTO, nullptr, st.data());
        std::vector<fa_status> out(k);
        for (size_t i = 0; i < k; ++i) out[i] = static_cast<fa_status>(st[i]);
        return out;
    }
private:
    fa_pool *h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------ mel
// AudioMelSpectrogram (Sources/FluidAudio/Shared/AudioMelSpectrogram.swift:59-70 ctor, :185-292 computeFlat, :325-456 computeFlatTransposed)
class AudioMelSpectrogram {
public:
    enum class LogFloorMode { additive, clamped };   // :24-27
    enum class PaddingMode { center, prePadded };    // :19-22
    struct Flat { std::vector<float> mel; int melLength; int numFrames; };

    AudioMelSpectrogram(Context &ctx, int sampleRate = 16000, int nMels = 128, int nFFT = 512, int hopLength = 160, int winLength = 400,
                        float preemph = 0.97f, int padTo = 0, float logFloor = std::ldexp(1.0f, -24), LogFloorMode logFloorMode = LogFloorMode::additive,
                        bool windowPeriodic = false)
        : ctx_(ctx) {
        fa_mel_default_config(&cfg_);
        cfg_.sample_rate = sampleRate; cfg_.n_mels = nMels; cfg_.n_fft = nFFT; cfg_.hop = hopLength; cfg_.win = winLength; cfg_.preemph = preemph;
        cfg_.pad_to = padTo; cfg_.log_floor = logFloor; cfg_.floor_mode = logFloorMode == LogFloorMode::clamped ? FA_MEL_FLOOR_CLAMPED : FA_MEL_FLOOR_ADDITIVE;
        cfg_.window_periodic = windowPeriodic ? 1 : 0;
    }
    // computeFlat(audio:lastAudioSample:) -> (mel [nMels, numFrames] flat, melLength, numFrames)
    Flat computeFlat(const std::vector<float> &audio, float lastAudioSample = 0.0f) const { return run(audio, lastAudioSample, FA_MEL_PAD_CENTER, FA_MEL_LAYOUT_MEL_MAJOR, std::nullopt); }
    // computeFlatTransposed(audio:lastAudioSample:paddingMode:expectedFrameCount:) -> (mel [numFrames, nMels] flat, melLength, numFrames)
    Flat computeFlatTransposed(const std::vector<float> &audio, float lastAudioSample = 0.0f, PaddingMode paddingMode = PaddingMode::center,
                               std::optional<int> expectedFrameCount = std::nullopt) const {
        return run(audio, lastAudioSample, paddingMode == PaddingMode::prePadded ? FA_MEL_PAD_PREPADDED : FA_MEL_PAD_CENTER, FA_MEL_LAYOUT_FRAME_MAJOR, expectedFrameCount);
    }
    std::vector<float> hannWindow() const { std::vector<float> w(cfg_.win); fa_mel_hann_window(&cfg_, w.data()); return w; }
    std::vector<float> melFilterbankFlat() const { std::vector<float> f(static_cast<size_t>(cfg_.n_mels) * (cfg_.n_fft / 2 + 1)); fa_mel_filterbank(&cfg_, f.data()); return f; }

private:
    Flat run(const std::vector<float> &audio, float last, int pad, int layout, std::optional<int> expected) const {
        fa_mel_config c = cfg_;
        c.padding_mode = pad; c.layout = layout;
        int T = expected ? *expected : fa_mel_num_frames(&c, static_cast<int64_t>(audio.size()));
        if (T <= 0 || audio.empty()) return Flat{std::vector<float>(static_cast<size_t>(c.n_mels), 0.0f), 0, 1};   // :199-201, :349-351
        const int Tpad = fa_mel_padded_frames(&c, T);
        Flat out{std::vector<float>(static_cast<size_t>(c.n_mels) * Tpad, 0.0f), 0, Tpad};
        const int64_t offs[2] = {0, static_cast<int64_t>(audio.size())};
        int32_t len = 0, exp = T;
        ctx_.check(fa_mel_batch(ctx_.handle(), &c, audio.data(), offs, 1, &last, expected ? &exp : nullptr, Tpad, out.mel.data(), &len), "fa_mel_batch");
        out.melLength = len;
        return out;
    }
    Context &ctx_;
    fa_mel_config cfg_{};
};

// ------------------------------------------------------------------------------------------------------------------ CTC
using Vocabulary = std::map<int, std::string>;   // [Int: String]

// decodeCtcTokenIds (…/CTC/CtcDecoder.swift:289-294): pieces joined, U+2581 -> space, spaces trimmed
inline std::string decodeCtcTokenIds(const std::vector<int> &ids, const Vocabulary &vocabulary) {
    std::string s;
    for (int id : ids) { auto it = vocabulary.find(id); if (it != vocabulary.end()) s += it->second; }
    std::string o;
    for (size_t i = 0; i < s.size();) {
        if (s.compare(i, 3, "\xe2\x96\x81") == 0) { o += ' '; i += 3; } else o += s[i++];
    }
    const size_t a = o.find_first_not_of(" \t"), b = o.find_last_not_of(" \t");
    return a == std::string::npos ? std::string() : o.substr(a, b - a + 1);
}

// LogitsArgmax.argmaxPerFrame (Sources/FluidAudio/ASR/Shared/LogitsArgmax.swift:16-55) on a [frames, vocab] matrix with row stride
inline std::vector<int> argmaxPerFrame(Context &ctx, const float *logits, int frames, int vocab, int64_t rowStride) {
    std::vector<int32_t> ids(frames > 0 ? frames : 0), toks(ids.size());
    int32_t n = 0;
    if (frames > 0) ctx.check(fa_ctc_greedy_batch(ctx.handle(), logits, FA_DTYPE_F32, 1, frames, vocab, rowStride, static_cast<int64_t>(frames) * rowStride, nullptr, -1,
                                                   ids.data(), toks.data(), &n), "fa_ctc_greedy_batch");
    return std::vector<int>(ids.begin(), ids.end());
}

// ctcGreedyDecode(logProbs:vocabulary:blankId:) (CtcDecoder.swift:15-36): the [[Float]] overload — each frame's scan is seeded with frame[0]
// (a NaN there => index 0, :25), frames keep their own lengths (:26), empty frames are skipped before `prev` is touched (:23)
inline std::string ctcGreedyDecode(Context &ctx, const std::vector<std::vector<float>> &logProbs, const Vocabulary &vocabulary, int blankId = 1024) {
    const size_t T = logProbs.size();
    if (T == 0) return "";
    std::vector<int64_t> offs(T + 1, 0);
    for (size_t t = 0; t < T; ++t) offs[t + 1] = offs[t] + static_cast<int64_t>(logProbs[t].size());
    std::vector<float> flat;
    flat.reserve(static_cast<size_t>(offs[T]));
    for (const auto &r : logProbs) flat.insert(flat.end(), r.begin(), r.end());
    std::vector<int32_t> toks(T);
    int32_t n = 0;
    ctx.check(fa_ctc_greedy_rows(ctx.handle(), flat.data(), offs.data(), static_cast<int64_t>(T), nullptr, 1, blankId, nullptr, toks.data(), &n), "fa_ctc_greedy_rows");
    return decodeCtcTokenIds(std::vector<int>(toks.begin(), toks.begin() + n), vocabulary);
}

// ctcGreedyDecode(logProbs: MLMultiArray [1, T, V], …) (CtcDecoder.swift:45-70): contiguous rows, -inf seed (a NaN never wins)
inline std::string ctcGreedyDecode(Context &ctx, const float *logProbs, int T, int V, const Vocabulary &vocabulary, int blankId = 1024) {
    if (T <= 0 || V <= 0) return "";
    std::vector<int32_t> toks(T);
    int32_t n = 0;
    ctx.check(fa_ctc_greedy_batch(ctx.handle(), logProbs, FA_DTYPE_F32, 1, T, V, static_cast<int64_t>(V), static_cast<int64_t>(T) * V, nullptr, blankId, nullptr,
                                  toks.data(), &n), "fa_ctc_greedy_batch");
    return decodeCtcTokenIds(std::vector<int>(toks.begin(), toks.begin() + n), vocabulary);
}

// ARPALanguageModel (…/CTC/ARPALanguageModel.swift:16-104)
class ARPALanguageModel {
public:
    static constexpr float unkLogProb = -23.026f;
    explicit ARPALanguageModel(const std::string &arpaText) { const fa_status st = fa_arpa_parse(nullptr, arpaText.data(), static_cast<int64_t>(arpaText.size()), &h_); if (st != FA_SUCCESS) throw Error(st, "fa_arpa_parse"); }
    ~ARPALanguageModel() { fa_arpa_destroy(h_); }
    ARPALanguageModel(const ARPALanguageModel &) = delete;
    ARPALanguageModel &operator=(const ARPALanguageModel &) = delete;
    int64_t unigramCount() const { return fa_arpa_unigram_count(h_); }
    int64_t bigramContextCount() const { return fa_arpa_bigram_context_count(h_); }
    float score(const std::string &word, const std::optional<std::string> &prev = std::nullopt) const {   // :98-103
        float out = 0.0f;
        fa_arpa_score(h_, word.c_str(), prev ? prev->c_str() : nullptr, &out);
        return out;
    }
    fa_arpa_lm *handle() const { return h_; }
private:
    fa_arpa_lm *h_ = nullptr;
};

// ctcBeamSearch(logProbs:vocabulary:lm:beamWidth:lmWeight:wordBonus:blankId:tokenCandidates:) (CtcDecoder.swift:118-241)
inline std::string ctcBeamSearch(Context &ctx, const std::vector<std::vector<float>> &logProbs, const Vocabulary &vocabulary, const ARPALanguageModel *lm = nullptr,
                                 int beamWidth = 100, float lmWeight = 0.3f, float wordBonus = 0.0f, int blankId = 1024, int tokenCandidates = 40) {
    if (logProbs.empty() || logProbs[0].empty()) return "";   // :129-131
    const int T = static_cast<int>(logProbs.size()), V = static_cast<int>(logProbs[0].size());
    std::vector<float> flat;
    flat.reserve(static_cast<size_t>(T) * V);
    for (const auto &r : logProbs) flat.insert(flat.end(), r.begin(), r.begin() + V);
    fa_ctc_vocab *voc = nullptr;
    if (lm) {
        std::vector<int32_t> ids;
        std::vector<const char *> pieces;
        for (const auto &kv : vocabulary) { ids.push_back(kv.first); pieces.push_back(kv.second.c_str()); }
        ctx.check(fa_ctc_vocab_create(ctx.handle(), ids.data(), pieces.data(), static_cast<int32_t>(ids.size()), V, &voc), "fa_ctc_vocab_create");
    }
    std::vector<int32_t> toks(T);
    int32_t n = 0;
    float score = 0.0f;
    const fa_status st = fa_ctc_beam_search_batch(ctx.handle(), flat.data(), 1, T, V, nullptr, voc, lm ? lm->handle() : nullptr, beamWidth, lmWeight, wordBonus, blankId,
                                                  tokenCandidates, toks.data(), &n, &score);
    fa_ctc_vocab_destroy(voc);
    ctx.check(st, "fa_ctc_beam_search_batch");
    return decodeCtcTokenIds(std::vector<int>(toks.begin(), toks.begin() + n), vocabulary);
}

// ------------------------------------------------------------------------------------------------------------------ clustering
using Matrix = std::vector<std::vector<double>>;   // [[Double]]

inline std::vector<double> flatten(const Matrix &m, size_t &n, size_t &d) {
    n = m.size(); d = n ? m[0].size() : 0;
    std::vector<double> f;
    f.reserve(n * d);
    for (const auto &r : m) f.insert(f.end(), r.begin(), r.begin() + d);
    return f;
}

// AHCClustering.cluster(embeddingFeatures:threshold:) (Sources/FluidAudio/Diarizer/Offline/Clustering/AHCClustering.swift:20-67)
struct AHCClustering {
    Context &ctx;
    std::vector<int> cluster(const Matrix &embeddingFeatures, double threshold) const {
        size_t n, d;
        const std::vector<double> x = flatten(embeddingFeatures, n, d);
        if (n == 0) return {};                                   // :24
        if (d == 0) return std::vector<int>(n, 0);               // :25-27
        if (n == 1) return {0};                                  // :28
        std::vector<int32_t> labels(n);
        (void)fa_ahc_cluster(ctx.handle(), x.data(), n, d, threshold, FA_AHC_MODE_AUTO, labels.data(), nullptr);   // failure -> 0..<n inside (:52-55)
        return std::vector<int>(labels.begin(), labels.end());
    }
};

// SpeakerCountConstraints (…/Clustering/SpeakerCountConstraints.swift:6-77)
struct SpeakerCountConstraints {
    std::optional<int> numSpeakers;
    int minSpeakers, maxSpeakers;
    static SpeakerCountConstraints resolve(int numEmbeddings, std::optional<int> numSpeakers, std::optional<int> minSpeakers, std::optional<int> maxSpeakers) {
        int64_t a = numSpeakers.value_or(0), b = minSpeakers.value_or(0), c = maxSpeakers.value_or(0), out[3];
        fa_speaker_constraints_resolve(numEmbeddings, numSpeakers ? &a : nullptr, minSpeakers ? &b : nullptr, maxSpeakers ? &c : nullptr, out);
        return SpeakerCountConstraints{out[0] < 0 ? std::nullopt : std::optional<int>(static_cast<int>(out[0])), static_cast<int>(out[1]), static_cast<int>(out[2])};
    }
    bool needsAdjustment(int detectedCount) const { return detectedCount < minSpeakers || detectedCount > maxSpeakers; }
    int targetCount(int detectedCount) const { return detectedCount < minSpeakers ? minSpeakers : (detectedCount > maxSpeakers ? maxSpeakers : detectedCount); }
};

// KMeansClustering (…/Clustering/KMeansClustering.swift:39-129)
struct KMeansClustering {
    static std::pair<std::vector<int>, Matrix> clusterWithCentroids(Context &ctx, const Matrix &embeddings, int numClusters, int maxIterations = 300,
                                                                    std::optional<uint64_t> seed = std::nullopt, int nInit = 1) {
        size_t n, d;
        const std::vector<double> x = flatten(embeddings, n, d);
        if (n == 0) return {};
        std::vector<int32_t> labels(n);
        std::vector<double> cen(static_cast<size_t>(std::max<int64_t>(1, std::min<int64_t>(numClusters, static_cast<int64_t>(n)))) * std::max<size_t>(d, 1));
        int32_t k = 0;
        ctx.check(nInit > 1 ? fa_kmeans_cluster_ninit(ctx.handle(), x.data(), static_cast<int64_t>(n), static_cast<int32_t>(d), numClusters, maxIterations, nInit, seed.value_or(0),
                                                      labels.data(), cen.data(), &k, nullptr, nullptr)
                            : fa_kmeans_cluster(ctx.handle(), x.data(), static_cast<int64_t>(n), static_cast<int32_t>(d), numClusters, maxIterations, seed.value_or(0), labels.data(),
                                                cen.data(), &k, nullptr),
                  "fa_kmeans_cluster");
        Matrix c(k, std::vector<double>(d));
        for (int i = 0; i < k; ++i) std::copy(cen.begin() + static_cast<size_t>(i) * d, cen.begin() + static_cast<size_t>(i + 1) * d, c[i].begin());
        return {std::vector<int>(labels.begin(), labels.end()), c};
    }
    static std::pair<std::vector<int>, Matrix> clusterWithCentroidsNInit(Context &ctx, const Matrix &embeddings, int numClusters, int maxIterations = 300, int nInit = 10,
                                                                         uint64_t baseSeed = 0) {
        return clusterWithCentroids(ctx, embeddings, numClusters, maxIterations, baseSeed, nInit);
    }
};

// VBxOutput / VBxClustering.refine / refineWithConstraints (…/Clustering/VBxClustering.swift:41-165, :685-733; OfflineDiarizerTypes.swift:675-702)
struct VBxOutput {
    Matrix gamma;
    std::vector<double> pi;
    std::vector<int> hardClusters;
    Matrix centroids;
    int numClusters = 0;
    std::vector<double> elbos;
    bool wasAdjusted = false;
    std::optional<int> originalClusterCount;
    int assignedClusterCount() const {
        if (gamma.empty()) { int c = 0; for (double p : pi) c += p > 1e-7; return pi.empty() ? numClusters : c; }
        std::vector<char> win(gamma[0].size(), 0);
        for (const auto &row : gamma) { size_t b = 0; for (size_t i = 1; i < row.size(); ++i) if (row[i] > row[b]) b = i; if (!row.empty()) win[b] = 1; }
        int c = 0; for (char w : win) c += w; return c;
    }
};

struct VBxClustering {
    Context &ctx;
    std::vector<double> phiParameters;
    int maxIterations = 20;
    double convergenceTolerance = 1e-4, warmStartFa = 0.07, warmStartFb = 0.8;   // OfflineDiarizerTypes.swift:155-163,189-192

    VBxOutput refine(const Matrix &rhoFeatures, const std::vector<int> &initialClusters) const {
        size_t T, D;
        const std::vector<double> rho = flatten(rhoFeatures, T, D);
        if (T == 0 || D == 0) return {};                         // :45-67
        std::vector<int32_t> init(initialClusters.begin(), initialClusters.end());
        std::vector<double> phi = phiParameters.size() == D ? phiParameters : std::vector<double>(D, 1.0);   // :72-76
        const int S = std::max(1, fa_vbx_speaker_count(init.data(), static_cast<int64_t>(T)));
        std::vector<double> gamma(T * S), pi(S), elbos(std::max(maxIterations, 1));
        std::vector<int32_t> hard(T);
        int32_t it = 0, ns = 0;
        ctx.check(fa_vbx_refine(ctx.handle(), rho.data(), static_cast<int64_t>(T), static_cast<int32_t>(D), init.data(), phi.data(), warmStartFa, warmStartFb, maxIterations,
                                convergenceTolerance, gamma.data(), pi.data(), hard.data(), elbos.data(), &it, &ns), "fa_vbx_refine");
        VBxOutput o;
        o.gamma.assign(T, std::vector<double>(S));
        for (size_t t = 0; t < T; ++t) std::copy(gamma.begin() + t * S, gamma.begin() + (t + 1) * S, o.gamma[t].begin());
        o.pi = pi; o.hardClusters.assign(hard.begin(), hard.end()); o.numClusters = S; o.elbos.assign(elbos.begin(), elbos.begin() + it);
        return o;
    }
    VBxOutput refineWithConstraints(const Matrix &rhoFeatures, const Matrix &trainingEmbeddings, const std::vector<int> &initialClusters,
                                    const std::optional<SpeakerCountConstraints> &constraints) const {
        VBxOutput out = refine(rhoFeatures, initialClusters);
        if (!constraints) return out;
        const int detected = out.assignedClusterCount();
        if (!constraints->needsAdjustment(detected)) return out;
        const int target = constraints->targetCount(detected);
        auto km = KMeansClustering::clusterWithCentroidsNInit(ctx, trainingEmbeddings, target, 100, 10, 0);   // :716-722
        out.hardClusters = km.first; out.centroids = km.second; out.numClusters = target; out.wasAdjusted = true; out.originalClusterCount = detected;
        return out;
    }
};

// HungarianAssignment.maxScoreAssignment / ConstrainedClusterAssignment.assign (Diarizer/HungarianAssignment.swift:67-97,
// …/Clustering/ConstrainedClusterAssignment.swift:20-42)
struct ConstrainedClusterAssignment {
    static std::vector<int> assign(Context &ctx, const Matrix &scores, const std::vector<int> &chunkIndices) {
        size_t n, K;
        const std::vector<double> s = flatten(scores, n, K);
        std::vector<int32_t> chunks(chunkIndices.begin(), chunkIndices.end()), out(chunkIndices.size());
        if (!chunks.empty()) ctx.check(fa_constrained_assign(ctx.handle(), s.data(), static_cast<int64_t>(chunks.size()), static_cast<int32_t>(K), chunks.data(), out.data()), "fa_constrained_assign");
        return std::vector<int>(out.begin(), out.end());
    }
};

// OfflineDiarizerManager.cluster (…/Offline/Core/OfflineDiarizerManager.swift:270-375) on precomputed embeddings: one device-resident call
struct OfflineClusteringConfig {   // OfflineDiarizerTypes.swift:155-163,189-192
    double clusteringThreshold = 0.6, warmStartFa = 0.07, warmStartFb = 0.8, convergenceTolerance = 1e-4;
    int maxVbxIterations = 20;
    bool constrainedAssignment = true;
    std::optional<int> numSpeakers, minSpeakers, maxSpeakers;
    // the clustering / VBx guards of OfflineDiarizerConfig.validate (OfflineDiarizerTypes.swift:357-408: invalidConfiguration)
    void validate() const {
        if (!(clusteringThreshold > 0 && clusteringThreshold <= 2.0)) throw Error(FA_INVALID_ARGUMENT, "invalidConfiguration: clustering.threshold must be within (0, 2]");
        if (!(warmStartFa > 0 && warmStartFb > 0)) throw Error(FA_INVALID_ARGUMENT, "invalidConfiguration: clustering warm-start Fa/Fb must be positive");
        if (!(maxVbxIterations > 0)) throw Error(FA_INVALID_ARGUMENT, "invalidConfiguration: maxVBxIterations must be > 0");
        if (!(convergenceTolerance > 0)) throw Error(FA_INVALID_ARGUMENT, "invalidConfiguration: convergenceTolerance must be positive");
    }
};
struct OfflineClusteringResult {
    std::vector<int> assignments;   // -2: slot dropped by the constrained assignment
    Matrix centroids;
    fa_offline_cluster_info info{};
};
inline OfflineClusteringResult clusterEmbeddings(Context &ctx, const std::vector<std::vector<float>> &embeddings, const Matrix &rhoFeatures, const std::vector<int> &chunkIndices,
                                                 const std::vector<double> &phi, const OfflineClusteringConfig &config = {}) {
    config.validate();
    if (embeddings.empty()) throw Error(FA_INVALID_ARGUMENT, "noSpeechDetected");   // :281-283
    const size_t n = embeddings.size(), d = embeddings[0].size();
    std::vector<float> e(n * d);
    for (size_t i = 0; i < n; ++i) std::copy(embeddings[i].begin(), embeddings[i].end(), e.begin() + i * d);
    size_t rn = 0, rd = 0;
    const std::vector<double> rho = flatten(rhoFeatures, rn, rd);
    std::vector<double> ph = phi.size() == rd ? phi : std::vector<double>(rd, 1.0);   // VBxClustering.swift:72-76
    std::vector<int32_t> chunks(chunkIndices.begin(), chunkIndices.end()), labels(n);
    fa_offline_cluster_config c;
    fa_offline_cluster_default_config(&c);
    c.clustering_threshold = config.clusteringThreshold; c.warm_start_fa = config.warmStartFa; c.warm_start_fb = config.warmStartFb;
    c.max_vbx_iterations = config.maxVbxIterations; c.convergence_tolerance = config.convergenceTolerance; c.constrained_assignment = config.constrainedAssignment ? 1 : 0;
    c.num_speakers = config.numSpeakers.value_or(-1); c.min_speakers = config.minSpeakers.value_or(-1); c.max_speakers = config.maxSpeakers.value_or(-1);
    OfflineClusteringResult out;
    std::vector<double> cen(256 * d);
    int32_t k = 0;
    ctx.check(fa_offline_cluster(ctx.handle(), e.data(), static_cast<int64_t>(n), static_cast<int32_t>(d), rd ? rho.data() : nullptr, static_cast<int32_t>(rd), chunks.data(),
                                 rd ? ph.data() : nullptr, &c, 0, labels.data(), cen.data(), 256, &k, &out.info), "fa_offline_cluster");
    out.assignments.assign(labels.begin(), labels.end());
    out.centroids.assign(k, std::vector<double>(d));
    for (int i = 0; i < k; ++i) std::copy(cen.begin() + static_cast<size_t>(i) * d, cen.begin() + static_cast<size_t>(i + 1) * d, out.centroids[i].begin());
    return out;
}

// Several recordings through the stage in one call (fa_offline_cluster_batch: their merge chains advance together).  One entry per
// recording; a recording that fails (e.g. no embeddings) yields an empty optional and does not stop the others.
struct OfflineRecording { std::vector<std::vector<float>> embeddings; Matrix rhoFeatures; std::vector<int> chunkIndices; };
inline std::vector<std::optional<OfflineClusteringResult>> clusterEmbeddingsBatch(Context &ctx, const std::vector<OfflineRecording> &recordings, const std::vector<double> &phi,
                                                                                   const OfflineClusteringConfig &config = {}) {
    config.validate();
    const size_t count = recordings.size();
    std::vector<std::optional<OfflineClusteringResult>> out(count);
    if (count == 0) return out;
    size_t d = 0, rd = 0;
    for (const auto &r : recordings) { if (!r.embeddings.empty()) d = r.embeddings[0].size(); if (!r.rhoFeatures.empty()) rd = r.rhoFeatures[0].size(); }
    if (d == 0) return out;
    std::vector<std::vector<float>> e(count);
    std::vector<std::vector<double>> rho(count), cen(count, std::vector<double>(256 * d));
    std::vector<std::vector<int32_t>> chunks(count), labels(count);
    std::vector<const float *> ep(count);
    std::vector<const double *> rp(count);
    std::vector<const int32_t *> cp(count);
    std::vector<int32_t *> lp(count);
    std::vector<double *> zp(count);
    std::vector<int64_t> n(count);
    static const float dummy_f[4] = {0, 0, 0, 0};
    static const double dummy_d[4] = {0, 0, 0, 0};
    static const int32_t dummy_i[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < count; ++i) {
        const auto &r = recordings[i];
        n[i] = static_cast<int64_t>(r.embeddings.size());
        e[i].resize(r.embeddings.size() * d);
        for (size_t t = 0; t < r.embeddings.size(); ++t) std::copy(r.embeddings[t].begin(), r.embeddings[t].end(), e[i].begin() + t * d);
        size_t rn = 0, rdi = 0;
        rho[i] = flatten(r.rhoFeatures, rn, rdi);
        chunks[i].assign(r.chunkIndices.begin(), r.chunkIndices.end());
        labels[i].assign(std::max<size_t>(r.embeddings.size(), 1), 0);
        ep[i] = e[i].empty() ? dummy_f : e[i].data();
        rp[i] = rho[i].empty() ? dummy_d : rho[i].data();
        cp[i] = chunks[i].empty() ? dummy_i : chunks[i].data();
        lp[i] = labels[i].data();
        zp[i] = cen[i].data();
    }
    std::vector<double> ph = phi.size() == rd ? phi : std::vector<double>(rd, 1.0);
    fa_offline_cluster_config c;
    fa_offline_cluster_default_config(&c);
    c.clustering_threshold = config.clusteringThreshold; c.warm_start_fa = config.warmStartFa; c.warm_start_fb = config.warmStartFb;
    c.max_vbx_iterations = config.maxVbxIterations; c.convergence_tolerance = config.convergenceTolerance; c.constrained_assignment = config.constrainedAssignment ? 1 : 0;
    c.num_speakers = config.numSpeakers.value_or(-1); c.min_speakers = config.minSpeakers.value_or(-1); c.max_speakers = config.maxSpeakers.value_or(-1);
    std::vector<int32_t> k(count, 0), st(count, 0);
    std::vector<fa_offline_cluster_info> infos(count);
    (void)fa_offline_cluster_batch(ctx.handle(), static_cast<int32_t>(count), ep.data(), n.data(), static_cast<int32_t>(d), rd ? rp.data() : nullptr, static_cast<int32_t>(rd), cp.data(),
                                   rd ? ph.data() : nullptr, &c, lp.data(), zp.data(), 256, k.data(), infos.data(), st.data());
    for (size_t i = 0; i < count; ++i) {
        if (st[i] != FA_SUCCESS) continue;
        OfflineClusteringResult r;
        r.assignments.assign(labels[i].begin(), labels[i].begin() + n[i]);
        r.centroids.assign(k[i], std::vector<double>(d));
        for (int q = 0; q < k[i]; ++q) std::copy(cen[i].begin() + static_cast<size_t>(q) * d, cen[i].begin() + static_cast<size_t>(q + 1) * d, r.centroids[q].begin());
        r.info = infos[i];
        out[i] = std::move(r);
    }
    return out;
}

// LuxTtsMelExtractor (Sources/FluidAudio/TTS/LuxTts/LuxTtsMelExtractor.swift:15-132): the torchaudio-flavoured front end, same C ABI
struct LuxTtsMelExtractor {
    Context &ctx;
    static constexpr int nFFT = 1024, hop = 256, nMels = 100, sampleRate = 24000;
    int frameCount(int sampleCount) const { return (sampleCount + hop / 2) / hop; }   // :45-47
    std::vector<std::vector<float>> extract(const std::vector<float> &audio) const {
        const int T = frameCount(static_cast<int>(audio.size()));
        if (audio.empty() || T <= 0) return {};
        fa_mel_config c;
        fa_mel_default_config(&c);
        c.sample_rate = sampleRate; c.n_mels = nMels; c.n_fft = nFFT; c.hop = hop; c.win = nFFT; c.preemph = 0.0f; c.log_floor = 1e-7f; c.floor_mode = FA_MEL_FLOOR_CLAMPED;
        c.window_periodic = 1; c.layout = FA_MEL_LAYOUT_FRAME_MAJOR; c.power = 1.0f; c.center_pad = FA_MEL_CENTER_REFLECT; c.mel_scale = FA_MEL_SCALE_HTK_NONORM;
        c.tail_mode = FA_MEL_TAIL_REPLICATE;
        std::vector<float> flat(static_cast<size_t>(T) * nMels);
        const int64_t offs[2] = {0, static_cast<int64_t>(audio.size())};
        int32_t len = 0, exp = T;
        ctx.check(fa_mel_batch(ctx.handle(), &c, audio.data(), offs, 1, nullptr, &exp, T, flat.data(), &len), "fa_mel_batch");
        std::vector<std::vector<float>> out(T, std::vector<float>(nMels));
        for (int t = 0; t < T; ++t) std::copy(flat.begin() + static_cast<size_t>(t) * nMels, flat.begin() + static_cast<size_t>(t + 1) * nMels, out[t].begin());
        return out;
    }
};

// ------------------------------------------------------------------------------------------------------------------ wire formats
// AudioWAV.data(from:sampleRate:normalize:) (Sources/FluidAudio/Shared/AudioConverter.swift:474-532)
struct AudioWAV {
    static std::vector<uint8_t> data(Context &ctx, const std::vector<float> &samples, double sampleRate, bool normalize = true) {
        std::vector<uint8_t> out(static_cast<size_t>(fa_wav_pcm16_size(static_cast<int64_t>(samples.size()))));
        int64_t len = 0;
        ctx.check(fa_wav_encode_pcm16(ctx.handle(), samples.data(), static_cast<int64_t>(samples.size()), sampleRate, normalize ? 1 : 0, out.data(), static_cast<int64_t>(out.size()), &len), "fa_wav_encode_pcm16");
        return out;
    }
};

// RTTMParser.loadSegments (Sources/FluidAudioCLI/Utils/RTTMParser.swift:22-63) on text
struct RTTMParserError : std::runtime_error { using std::runtime_error::runtime_error; };
struct RTTMParser {
    static std::vector<fa_rttm_segment> parse(const std::string &text) {
        int64_t count = 0;
        char bad[512] = {0};
        if (fa_rttm_parse(text.data(), static_cast<int64_t>(text.size()), 1, nullptr, 0, &count, bad, sizeof(bad)) != FA_SUCCESS) throw RTTMParserError(std::string("Invalid RTTM line: ") + bad);
        std::vector<fa_rttm_segment> segs(static_cast<size_t>(count));
        if (count) fa_rttm_parse(text.data(), static_cast<int64_t>(text.size()), 1, segs.data(), count, &count, bad, sizeof(bad));
        return segs;
    }
};


// ------------------------------------------------------------------------------------------------------------------ speaker segments
// OfflineReconstruction (Sources/FluidAudio/Diarizer/Offline/Utils/OfflineReconstruction.swift:24-357) over fa_offline_reconstruct:
// speakerWeights [chunks][frames][speakers] (powerset decode output), hardClusters [chunks][speakers] (chunk assignments, -2 = none),
// centroids [K][d].  buildSegments runs on the device; buildSpeakerDatabase is the host fp32 average of the segments' centroids.
// The zero-vote re-embed pass is the caller's (fa_reconstruct_info.zero_vote_runs + overrides, include/fluidaudio_hip.h).
class OfflineReconstruction {
public:
    struct Result { std::vector<fa_rttm_segment> segments; std::map<std::string, std::vector<float>> speakerDatabase; };
    explicit OfflineReconstruction(fa_reconstruct_config config = defaultConfig()) : cfg_(config) {}
    static fa_reconstruct_config defaultConfig() { fa_reconstruct_config c; fa_reconstruct_default_config(&c); return c; }
    std::vector<fa_rttm_segment> buildSegments(Context &ctx, const std::vector<std::vector<std::vector<float>>> &speakerWeights,
                                               const std::vector<double> &chunkOffsets, const std::vector<std::vector<int>> &hardClusters,
                                               int32_t clusterCount) const {
        const int64_t C = static_cast<int64_t>(speakerWeights.size());
        const int32_t F = C ? static_cast<int32_t>(speakerWeights[0].size()) : 0;
        const int32_t S = F ? static_cast<int32_t>(speakerWeights[0][0].size()) : 0;
        std::vector<float> w;
        w.reserve(static_cast<size_t>(C * F * S));
        for (const auto &chunk : speakerWeights) {
            if (static_cast<int32_t>(chunk.size()) != F) throw Error(FA_INVALID_ARGUMENT, "OfflineReconstruction: ragged frames");
            for (const auto &frame : chunk) {
                if (static_cast<int32_t>(frame.size()) != S) throw Error(FA_INVALID_ARGUMENT, "OfflineReconstruction: ragged speakers");
                w.insert(w.end(), frame.begin(), frame.end());
            }
        }
        std::vector<int32_t> hard(static_cast<size_t>(C * S), -2);   // chunks past hardClusters.count: -2 (:65-67)
        for (size_t c = 0; c < hardClusters.size() && static_cast<int64_t>(c) < C; ++c)
            for (size_t s = 0; s < hardClusters[c].size() && static_cast<int32_t>(s) < S; ++s) hard[c * S + s] = hardClusters[c][s];
        int64_t n = 0;
        fa_reconstruct_info info{};
        const auto call = [&](fa_rttm_segment *out, int64_t cap) {
            return fa_offline_reconstruct(ctx.handle(), &cfg_, w.data(), C, F, S, chunkOffsets.data(), static_cast<int64_t>(chunkOffsets.size()), hard.data(),
                                          clusterCount, nullptr, 0, out, cap, &n, &info);
        };
        std::vector<fa_rttm_segment> segs(4096);
        fa_status st = call(segs.data(), static_cast<int64_t>(segs.size()));
        if (st == FA_OUTPUT_TOO_SMALL) { segs.resize(static_cast<size_t>(n)); st = call(segs.data(), n); }
        ctx.check(st, "fa_offline_reconstruct");
        segs.resize(static_cast<size_t>(n));
        return segs;
    }
    // buildSpeakerDatabase (:300-357): per speaker the fp32 sum of Float(centroid) over its segments, in segment order, times 1 / Float(count)
    static std::map<std::string, std::vector<float>> buildSpeakerDatabase(const std::vector<fa_rttm_segment> &segments, const Matrix &centroids) {
        std::map<std::string, std::vector<float>> sums;
        std::map<std::string, int> counts;
        const size_t dim = centroids.empty() ? 0 : centroids[0].size();
        for (const auto &s : segments) {
            const std::string id(s.speaker_id);
            const long k = std::strtol(s.speaker_id + 1, nullptr, 10) - 1;
            std::vector<float> e(dim, 0.0f);
            if (k >= 0 && static_cast<size_t>(k) < centroids.size()) for (size_t i = 0; i < dim; ++i) e[i] = static_cast<float>(centroids[k][i]);
            auto it = sums.find(id);
            if (it == sums.end()) sums.emplace(id, e);
            else for (size_t i = 0; i < dim; ++i) it->second[i] += e[i];
            ++counts[id];
        }
        for (auto &kv : sums) { const float scale = 1.0f / static_cast<float>(counts[kv.first]); for (float &v : kv.second) v *= scale; }
        return sums;
    }
    Result build(Context &ctx, const std::vector<std::vector<std::vector<float>>> &speakerWeights, const std::vector<double> &chunkOffsets,
                 const std::vector<std::vector<int>> &hardClusters, const Matrix &centroids) const {
        Result r;
        r.segments = buildSegments(ctx, speakerWeights, chunkOffsets, hardClusters, static_cast<int32_t>(centroids.size()));
        r.speakerDatabase = buildSpeakerDatabase(r.segments, centroids);
        return r;
    }
private:
    fa_reconstruct_config cfg_;
};

// ------------------------------------------------------------------------------------------------------------------ embedding inputs
// OfflineEmbeddingExtractor.extractEmbeddings up to the networks (Sources/FluidAudio/Diarizer/Offline/Extraction/OfflineEmbeddingExtractor.swift:
// 177-711) over fa_embedding_plan: speakerWeights [chunks][frames][speakers] (powerset decode output) -> which (chunk, speaker) pairs get an
// embedding (records: the TimedEmbedding metadata), the model run each one carries (runOfJob), the fbank window of each run (windowOfRun,
// windowStart) and the resampled masks the embedding model takes (runWeights [runs][weightFrames]).  The networks are the caller's.
class OfflineEmbeddingPlanner {
public:
    struct Plan {
        std::vector<fa_export_embedding> records;
        std::vector<int32_t> runOfJob, windowOfRun, windowChunk;
        std::vector<int64_t> windowStart;
        std::vector<std::vector<float>> runWeights, frameWeights;   // frameWeights: the chosen masks before resampling (when asked for)
        fa_embedding_info info{};
    };
    explicit OfflineEmbeddingPlanner(fa_embedding_config config = defaultConfig()) : cfg_(config) {}
    static fa_embedding_config defaultConfig() { fa_embedding_config c; fa_embedding_default_config(&c); return c; }
    Plan plan(Context &ctx, const std::vector<std::vector<std::vector<float>>> &speakerWeights, const std::vector<double> &chunkOffsets,
              int64_t totalSamples, double frameDuration = 0.0, bool frameWeights = false) const {
        const int64_t C = static_cast<int64_t>(speakerWeights.size());
        const int32_t F = C ? static_cast<int32_t>(speakerWeights[0].size()) : 0;
        const int32_t S = F ? static_cast<int32_t>(speakerWeights[0][0].size()) : 0;
        std::vector<float> w;
        w.reserve(static_cast<size_t>(C * F * S));
        for (const auto &chunk : speakerWeights) {
            if (static_cast<int32_t>(chunk.size()) != F) throw Error(FA_INVALID_ARGUMENT, "OfflineEmbeddingPlanner: ragged frames");
            for (const auto &frame : chunk) {
                if (static_cast<int32_t>(frame.size()) != S) throw Error(FA_INVALID_ARGUMENT, "OfflineEmbeddingPlanner: ragged speakers");
                w.insert(w.end(), frame.begin(), frame.end());
            }
        }
        fa_embedding_config cfg = cfg_;
        cfg.frame_duration = frameDuration;
        const size_t cap = static_cast<size_t>(std::max<int64_t>(C * S, 1)), W = static_cast<size_t>(std::max(cfg.weight_frames, 1));
        Plan p;
        p.records.resize(cap);
        p.runOfJob.resize(cap);
        p.windowOfRun.resize(cap);
        p.windowStart.resize(static_cast<size_t>(std::max<int64_t>(C, 1)));
        p.windowChunk.resize(p.windowStart.size());
        std::vector<float> rows(cap * W), masks(frameWeights ? cap * static_cast<size_t>(std::max(F, 1)) : 0);
        ctx.check(fa_embedding_plan(ctx.handle(), &cfg, w.data(), C, F, S, chunkOffsets.data(), static_cast<int64_t>(chunkOffsets.size()), totalSamples,
                                    p.records.data(), p.runOfJob.data(), p.windowOfRun.data(), p.windowStart.data(), p.windowChunk.data(), rows.data(),
                                    frameWeights ? masks.data() : nullptr, &p.info),
                  "fa_embedding_plan");
        const size_t jobs = static_cast<size_t>(p.info.jobs), runs = static_cast<size_t>(p.info.runs), nw = static_cast<size_t>(p.info.planned_chunks);
        p.records.resize(jobs);
        p.runOfJob.resize(jobs);
        p.windowOfRun.resize(runs);
        p.windowStart.resize(nw);
        p.windowChunk.resize(nw);
        for (size_t r = 0; r < runs; ++r) p.runWeights.emplace_back(rows.begin() + r * W, rows.begin() + (r + 1) * W);
        if (frameWeights) for (size_t j = 0; j < jobs; ++j) p.frameWeights.emplace_back(masks.begin() + j * F, masks.begin() + (j + 1) * F);
        return p;
    }
private:
    fa_embedding_config cfg_;
};

// ------------------------------------------------------------------------------------------------------------------ offline Sortformer, timeline
// OfflineSortformerConfig (Sources/FluidAudio/Diarizer/Sortformer/Offline/OfflineSortformerDiarizer.swift:14-58) with the window geometry of
// processComplete (:303-363) over fa_sortformer_offline_windows.
struct OfflineSortformerConfig {
    int windowOutputFrames = 384, subsamplingFactor = 8, numSpeakers = 4, melFeatures = 128, sampleRate = 16000, melStride = 160, overlapOutputFrames = 100;
    int windowMelFrames() const { return windowOutputFrames * subsamplingFactor; }
    float frameDurationSeconds() const { return static_cast<float>(subsamplingFactor) * static_cast<float>(melStride) / static_cast<float>(sampleRate); }
    fa_sortformer_offline_config c() const { return fa_sortformer_offline_config{windowOutputFrames, subsamplingFactor, numSpeakers, melFeatures, overlapOutputFrames}; }
    struct Windows { std::vector<fa_sortformer_window> windows; std::vector<int64_t> totalOut, windowRange; };
    Windows windows(const std::vector<int64_t> &numMelFrames) const {
        const fa_sortformer_offline_config cfg = c();
        const int32_t B = static_cast<int32_t>(numMelFrames.size());
        Windows w;
        w.totalOut.resize(numMelFrames.size());
        w.windowRange.resize(numMelFrames.size() + 1);
        int64_t n = 0;
        fa_status st = fa_sortformer_offline_windows(&cfg, numMelFrames.data(), B, nullptr, 0, &n, w.totalOut.data(), w.windowRange.data());
        if (st != FA_SUCCESS) throw Error(st, "fa_sortformer_offline_windows");
        w.windows.resize(static_cast<size_t>(n));
        st = fa_sortformer_offline_windows(&cfg, numMelFrames.data(), B, w.windows.data(), n, &n, nullptr, nullptr);
        if (st != FA_SUCCESS) throw Error(st, "fa_sortformer_offline_windows");
        return w;
    }
};

// SortformerSpeakerStitcher.alignment (Sortformer/Offline/SortformerSpeakerStitcher.swift:27-77): mapping[windowSpeaker] == globalSpeaker
struct SortformerSpeakerStitcher {
    static std::vector<int> alignment(const std::vector<float> &global, const std::vector<float> &window, int frames, int numSpeakers) {
        std::vector<int> identity(static_cast<size_t>(std::max(numSpeakers, 0)));
        for (int i = 0; i < numSpeakers; ++i) identity[i] = i;
        const int64_t need = static_cast<int64_t>(frames) * numSpeakers;
        if (!(frames > 0 && numSpeakers > 0 && static_cast<int64_t>(global.size()) >= need && static_cast<int64_t>(window.size()) >= need)) return identity;
        std::vector<int32_t> m(static_cast<size_t>(numSpeakers));
        const fa_status st = fa_sortformer_stitcher_alignment(global.data(), window.data(), frames, numSpeakers, m.data());
        if (st != FA_SUCCESS) throw Error(st, "fa_sortformer_stitcher_alignment");
        return std::vector<int>(m.begin(), m.end());
    }
};

// DiarizerTimelineConfig (Sources/FluidAudio/Diarizer/DiarizerTimeline.swift:9-164); fromSeconds is the second initialiser's
// Int(round(x / frameDuration)) in fp32 (std::round: half away from zero)
struct DiarizerTimelineConfig {
    int numSpeakers = 1;
    float frameDurationSeconds = 0.08f, onsetThreshold = 0.5f, offsetThreshold = 0.5f;
    int onsetPadFrames = 0, offsetPadFrames = 0, minFramesOn = 0, minFramesOff = 0;
    static DiarizerTimelineConfig sortformerDefault() { DiarizerTimelineConfig c; c.numSpeakers = 4; return c; }
    static DiarizerTimelineConfig fromSeconds(int numSpeakers, float frameDurationSeconds, float onsetThreshold, float offsetThreshold, float onsetPadSeconds,
                                              float offsetPadSeconds, float minDurationOn, float minDurationOff) {
        DiarizerTimelineConfig c;
        c.numSpeakers = numSpeakers;
        c.frameDurationSeconds = frameDurationSeconds;
        c.onsetThreshold = onsetThreshold;
        c.offsetThreshold = offsetThreshold;
        c.onsetPadFrames = static_cast<int>(std::round(onsetPadSeconds / frameDurationSeconds));
        c.offsetPadFrames = static_cast<int>(std::round(offsetPadSeconds / frameDurationSeconds));
        c.minFramesOn = static_cast<int>(std::round(minDurationOn / frameDurationSeconds));
        c.minFramesOff = static_cast<int>(std::round(minDurationOff / frameDurationSeconds));
        return c;
    }
    fa_timeline_config c() const {
        fa_timeline_config t;
        fa_timeline_default_config(&t);
        t.onset_threshold = onsetThreshold;
        t.offset_threshold = offsetThreshold;
        t.onset_pad_frames = onsetPadFrames;
        t.offset_pad_frames = offsetPadFrames;
        t.min_frames_on = minFramesOn;
        t.min_frames_off = minFramesOff;
        t.frame_duration = frameDurationSeconds;
        t.speakers = numSpeakers;
        return t;
    }
};

struct DiarizerSegment {   // DiarizerSegment (:492-560)
    int speakerIndex = 0;
    int64_t startFrame = 0, endFrame = 0;
    bool isFinalized = true;
    float frameDurationSeconds = 0.08f, activity = 0.0f;
    int64_t length() const { return endFrame - startFrame; }
    float startTime() const { return static_cast<float>(startFrame) * frameDurationSeconds; }
    float endTime() const { return static_cast<float>(endFrame) * frameDurationSeconds; }
    float duration() const { return static_cast<float>(endFrame - startFrame) * frameDurationSeconds; }
};

// DiarizerTimeline.rebuild(finalizedPredictions:tentativePredictions:keepingSpeakers:false,isComplete:) (:945-1003) over fa_timeline_segments:
// flat [frames * numSpeakers] predictions of one recording -> its speakers' segments, by speaker, the finalized list before the tentative one.
class DiarizerTimeline {
public:
    explicit DiarizerTimeline(DiarizerTimelineConfig config = DiarizerTimelineConfig::sortformerDefault()) : cfg_(config) {}
    std::vector<DiarizerSegment> rebuild(Context &ctx, const std::vector<float> &finalizedPredictions, const std::vector<float> &tentativePredictions = {},
                                         bool isComplete = true) const {
        const size_t S = static_cast<size_t>(std::max(cfg_.numSpeakers, 1));
        if (finalizedPredictions.size() % S != 0 || tentativePredictions.size() % S != 0) throw Error(FA_INVALID_ARGUMENT, "DiarizerTimeline: misaligned predictions");
        const fa_timeline_config cfg = cfg_.c();
        const int64_t nf = static_cast<int64_t>(finalizedPredictions.size() / S), nt = static_cast<int64_t>(tentativePredictions.size() / S);
        int64_t n = 0;
        const auto call = [&](fa_diarizer_segment *out, int64_t cap) {
            return fa_timeline_segments(ctx.handle(), &cfg, finalizedPredictions.data(), &nf, tentativePredictions.data(), &nt, 1, isComplete ? 1 : 0, out, cap, &n,
                                        nullptr);
        };
        ctx.check(call(nullptr, 0), "fa_timeline_segments");
        std::vector<fa_diarizer_segment> recs(static_cast<size_t>(n));
        if (n > 0) ctx.check(call(recs.data(), n), "fa_timeline_segments");
        std::vector<DiarizerSegment> out;
        out.reserve(recs.size());
        for (const auto &r : recs) {
            DiarizerSegment s;
            s.speakerIndex = r.speaker;
            s.startFrame = r.start_frame;
            s.endFrame = r.end_frame;
            s.isFinalized = (r.finalized & 1) != 0;
            s.frameDurationSeconds = cfg_.frameDurationSeconds;
            s.activity = r.activity;
            out.push_back(s);
        }
        return out;
    }
private:
    DiarizerTimelineConfig cfg_;
};

// ------------------------------------------------------------------------------------------------------------------ diarization error rate
// DERSpeakerSegment, DERResult and DiarizationDER.compute (Sources/FluidAudio/Diarizer/DiarizationDER.swift:26-175) over fa_der_score_batch.
// The labels are numbered here by first appearance (:61-80) and the seconds and the rate are formed here with the reference's expressions
// (:160-164); the counts come from the device.  A side holds at most FA_DER_MAX_LABELS speakers (INVALID_ARGUMENT beyond, as for the
// arguments the reference traps on: frameStep <= 0, collar < 0, a non-finite time).
struct DERSpeakerSegment {
    std::string speaker;
    double start = 0.0, end = 0.0;
};

struct DERResult {
    double der = 0.0, confusion = 0.0, falseAlarm = 0.0, miss = 0.0, totalRefSpeech = 0.0;
    std::map<std::string, std::string> mapping;   // hyp label -> ref label; hyp labels without a partner are left out
    fa_der_counts counts{};                       // the integers behind the seconds
    std::vector<std::string> refLabels, hypLabels;
    std::vector<int32_t> indexMapping;            // hyp index -> ref index or -1
    std::vector<int64_t> overlap;                 // [hypLabels][refLabels] frames both are active in, before the collar
};

struct DiarizationDER {
    static DERResult compute(Context &ctx, const std::vector<DERSpeakerSegment> &ref, const std::vector<DERSpeakerSegment> &hyp, double frameStep = 0.01,
                             double collar = 0.0) {
        return compute(ctx.handle(), ref, hyp, frameStep, collar);
    }
    // on a raw handle: argument errors are answered before the handle is looked at
    static DERResult compute(fa_ctx *ctx, const std::vector<DERSpeakerSegment> &ref, const std::vector<DERSpeakerSegment> &hyp, double frameStep = 0.01,
                             double collar = 0.0) {
        DERResult out;
        const auto number = [](const std::vector<DERSpeakerSegment> &segs, std::vector<std::string> &labels) {
            std::map<std::string, int32_t> idx;
            std::vector<fa_der_segment> packed;
            packed.reserve(segs.size());
            for (const auto &s : segs) {
                const auto it = idx.emplace(s.speaker, static_cast<int32_t>(labels.size()));
                if (it.second) labels.push_back(s.speaker);
                packed.push_back(fa_der_segment{it.first->second, 0, s.start, s.end});
            }
            return packed;
        };
        const std::vector<fa_der_segment> r = number(ref, out.refLabels), h = number(hyp, out.hypLabels);
        if (out.refLabels.size() > FA_DER_MAX_LABELS || out.hypLabels.size() > FA_DER_MAX_LABELS) throw Error(FA_INVALID_ARGUMENT, "DiarizationDER: more than 64 labels on a side");
        const int64_t refRange[2] = {0, static_cast<int64_t>(r.size())}, hypRange[2] = {0, static_cast<int64_t>(h.size())};
        const int64_t mapRange[2] = {0, static_cast<int64_t>(out.hypLabels.size())};
        out.indexMapping.assign(out.hypLabels.size(), -1);
        out.overlap.assign(out.hypLabels.size() * out.refLabels.size(), 0);
        const fa_der_config cfg{frameStep, collar};
        const fa_status st = fa_der_score_batch(ctx, &cfg, r.data(), refRange, h.data(), hypRange, 1, &out.counts, out.indexMapping.data(), mapRange,
                                                out.overlap.data(), static_cast<int64_t>(out.overlap.size()));
        if (st != FA_SUCCESS) throw Error(st, "fa_der_score_batch", ctx ? fa_ctx_last_error(ctx) : nullptr);
        out.miss = static_cast<double>(out.counts.miss) * frameStep;
        out.falseAlarm = static_cast<double>(out.counts.false_alarm) * frameStep;
        out.confusion = static_cast<double>(out.counts.confusion) * frameStep;
        out.totalRefSpeech = static_cast<double>(out.counts.ref) * frameStep;
        out.der = out.totalRefSpeech > 0 ? (out.miss + out.falseAlarm + out.confusion) / out.totalRefSpeech : 0.0;
        for (size_t i = 0; i < out.indexMapping.size(); ++i)
            if (out.indexMapping[i] >= 0) out.mapping[out.hypLabels[i]] = out.refLabels[static_cast<size_t>(out.indexMapping[i])];
        return out;
    }
};

// ------------------------------------------------------------------------------------------------------------------ word / character error rate
// WERCalculator.editDistance and the metrics formed from it (Sources/FluidAudioCLI/Utils/WERCalculator.swift:7-56, 178-239) and
// StringUtils.levenshteinDistance (Sources/FluidAudio/Shared/StringUtils.swift:12-40) over fa_edit_distance_batch.  The tokens are numbered
// here by first appearance and compared as integers on the device; the rates are formed here with the reference's expressions (:19, :40,
// :45).  TextNormalizer, the split at whitespace and grapheme segmentation are the caller's: the tokens arrive normalised.
struct WERCalculator {
    using Tokens = std::vector<std::string>;
    struct EditDistanceResult {   // :171-176
        int total = 0, insertions = 0, deletions = 0, substitutions = 0;
    };
    struct WERMetrics {           // the tuple of calculateWERMetrics (:10)
        double wer = 0.0;
        int insertions = 0, deletions = 0, substitutions = 0, totalWords = 0;
    };
    // the batch form: every (hypothesis, reference) pair in one device call, answers in input order
    static std::vector<EditDistanceResult> editDistance(fa_ctx *ctx, const std::vector<std::pair<Tokens, Tokens>> &pairs) {
        std::map<std::string, int32_t> idx;
        std::vector<int32_t> hyp, ref;
        std::vector<int64_t> hypRange{0}, refRange{0};
        const auto number = [&idx](const Tokens &t, std::vector<int32_t> &ids, std::vector<int64_t> &range) {
            for (const std::string &s : t) ids.push_back(idx.emplace(s, static_cast<int32_t>(idx.size())).first->second);
            range.push_back(static_cast<int64_t>(ids.size()));
        };
        for (const auto &p : pairs) {
            number(p.first, hyp, hypRange);
            number(p.second, ref, refRange);
        }
        std::vector<EditDistanceResult> out;
        for (const fa_edit_counts &c : run(ctx, hyp, hypRange, ref, refRange)) out.push_back(EditDistanceResult{c.total, c.insertions, c.deletions, c.substitutions});
        return out;
    }
    static EditDistanceResult editDistance(fa_ctx *ctx, const Tokens &hyp, const Tokens &ref) { return editDistance(ctx, {{hyp, ref}})[0]; }
    static EditDistanceResult editDistance(Context &ctx, const Tokens &hyp, const Tokens &ref) { return editDistance(ctx.handle(), hyp, ref); }
    // calculateWERMetrics (:7-22) behind the normalizer and the split
    static WERMetrics calculateWERMetrics(fa_ctx *ctx, const Tokens &hypWords, const Tokens &refWords) {
        const EditDistanceResult d = editDistance(ctx, hypWords, refWords);
        const double wer = refWords.empty() ? 0.0 : static_cast<double>(d.total) / static_cast<double>(refWords.size());
        return WERMetrics{wer, d.insertions, d.deletions, d.substitutions, static_cast<int>(refWords.size())};
    }
    static std::vector<fa_edit_counts> run(fa_ctx *ctx, const std::vector<int32_t> &hyp, const std::vector<int64_t> &hypRange, const std::vector<int32_t> &ref,
                                           const std::vector<int64_t> &refRange) {
        const int64_t n = static_cast<int64_t>(hypRange.size()) - 1;
        std::vector<fa_edit_counts> out(static_cast<size_t>(n > 0 ? n : 0));
        if (n <= 0) return out;
        static const int32_t none = 0;   // a side without symbols still gets an array
        const fa_status st = fa_edit_distance_batch(ctx, hyp.empty() ? &none : hyp.data(), hypRange.data(), ref.empty() ? &none : ref.data(), refRange.data(), n, out.data());
        if (st != FA_SUCCESS) throw Error(st, "fa_edit_distance_batch", ctx ? fa_ctx_last_error(ctx) : nullptr);
        return out;
    }
};

struct StringUtils {
    // levenshteinDistance<T: Equatable>(_ a: [T], _ b: [T]) for T = Int (:12-36)
    static int levenshteinDistance(fa_ctx *ctx, const std::vector<int> &a, const std::vector<int> &b) {
        const std::vector<int32_t> x(a.begin(), a.end()), y(b.begin(), b.end());
        return WERCalculator::run(ctx, x, {0, static_cast<int64_t>(x.size())}, y, {0, static_cast<int64_t>(y.size())})[0].total;
    }
    static int levenshteinDistance(Context &ctx, const std::vector<int> &a, const std::vector<int> &b) { return levenshteinDistance(ctx.handle(), a, b); }
};

// ------------------------------------------------------------------------------------------------------------------ TDT language mode
// Language / Script / TokenLanguageFilter (Sources/FluidAudio/Shared/TokenLanguageFilter.swift:4-134) and the decoding entry of
// TdtDecoderV3.decodeWithTimings(..., language:) (TdtDecoderV3.swift:103-607, the filters :284-299, 371-387, 635-703) over
// fa_tdt_token_classes and fa_tdt_greedy_logits(_lang)_dev.  The joint logits and every per-chunk array live on the device.
enum class Script : int32_t { latin = FA_TDT_SCRIPT_LATIN, cyrillic = FA_TDT_SCRIPT_CYRILLIC, greek = FA_TDT_SCRIPT_GREEK };
enum class Language {
    english, spanish, french, german, italian, portuguese, romanian, dutch, danish, swedish, finnish, hungarian, estonian, latvian, lithuanian, maltese,
    polish, czech, slovak, slovenian, croatian, bosnian, russian, ukrainian, belarusian, bulgarian, serbian, greek
};
inline const char *rawValue(Language l) {
    static const char *const codes[] = {"en", "es", "fr", "de", "it", "pt", "ro", "nl", "da", "sv", "fi", "hu", "et", "lv", "lt", "mt",
                                        "pl", "cs", "sk", "sl", "hr", "bs", "ru", "uk", "be", "bg", "sr", "el"};
    return codes[static_cast<int>(l)];
}
inline Script script(Language l) {
    if (l == Language::greek) return Script::greek;
    return l >= Language::russian && l <= Language::serbian ? Script::cyrillic : Script::latin;
}

struct TokenLanguageFilter {
    // The class bytes of a vocabulary (FA_TDT_CLASS_*): vocabulary[i] empty optional = id i is not in the vocabulary
    static std::vector<uint8_t> tokenClasses(const std::vector<std::optional<std::string>> &vocabulary, const std::vector<int32_t> &blocklistIds = {}) {
        std::vector<const char *> texts(vocabulary.size());
        for (size_t i = 0; i < vocabulary.size(); ++i) {
            if (vocabulary[i] && vocabulary[i]->find('\0') != std::string::npos) throw Error(FA_INVALID_ARGUMENT, "fa_tdt_token_classes", "a token text holds a NUL");
            texts[i] = vocabulary[i] ? vocabulary[i]->c_str() : nullptr;
        }
        std::vector<uint8_t> classes(vocabulary.size());
        const fa_status st = fa_tdt_token_classes(texts.data(), nullptr, static_cast<int32_t>(vocabulary.size()), blocklistIds.data(),
                                                  static_cast<int32_t>(blocklistIds.size()), classes.data());
        if (st != FA_SUCCESS) throw Error(st, "fa_tdt_token_classes", "text that is not UTF-8, or a blocklist id outside the vocabulary");
        return classes;
    }
    // matches(_:script:) (:81-134).  U+2581 is stripped wherever it stands, also in front of a combining mark, where Foundation's
    // string search may leave it: the reference's tests pin no such token.
    static bool matches(const std::string &text, Script script) {
        return (tokenClasses({text})[0] & (FA_TDT_CLASS_LATIN_OK << static_cast<int32_t>(script))) != 0;
    }
};

struct TdtDecoderV3 {
    static bool englishBlocklistApplies(std::optional<Language> language) { return language && *language == Language::french; }   // :623-625
    struct Chunks {              // DEVICE pointers; the operands of fa_tdt_greedy_logits_dev
        const void *logits = nullptr;
        int32_t dtype = FA_DTYPE_F32, batch = 0, U = 0, T = 0, vocabWithBlank = 0;
        int64_t rowStride = 0;
        const int32_t *encLen = nullptr, *audioFrames = nullptr, *t0 = nullptr, *isLast = nullptr, *globalOffset = nullptr, *emitAfter = nullptr;
        int32_t maxOut = 0;
        int32_t *tokens = nullptr, *timestamps = nullptr, *durations = nullptr;
        float *confidences = nullptr;
        int32_t *counts = nullptr, *finalTime = nullptr, *finalU = nullptr, *status = nullptr;
    };
    struct LanguageMode {        // what transcribe(..., language:) adds: DEVICE class bytes of TokenLanguageFilter::tokenClasses, DEVICE outputs
        Language language = Language::english;
        const uint8_t *classes = nullptr;
        bool useBlocklist = false;      // the caller's decision: englishBlocklistApplies(language) and a blocklist in the class bytes
        int32_t topK = FA_TDT_MAX_TOP_K;
        int32_t *routes = nullptr;      // [batch][maxOut] FA_TDT_ROUTE_*
        int32_t *swapCounts = nullptr;  // [batch][2]
    };
    fa_tdt_config config{};
    TdtDecoderV3() { fa_tdt_default_config(&config); }
    // decodeWithTimings for a batch of chunks; language == nil is the plain walk
    void decodeWithTimings(Context &ctx, const Chunks &c, const std::optional<LanguageMode> &language = std::nullopt) const {
        if (!language) {
            ctx.check(fa_tdt_greedy_logits_dev(ctx.handle(), &config, c.logits, c.dtype, c.batch, c.U, c.T, c.vocabWithBlank, c.rowStride, c.encLen, c.audioFrames, c.t0,
                                               c.isLast, c.globalOffset, c.emitAfter, c.maxOut, c.tokens, c.timestamps, c.durations, c.confidences, c.counts,
                                               c.finalTime, c.finalU, c.status), "fa_tdt_greedy_logits_dev");
            return;
        }
        ctx.check(fa_tdt_greedy_logits_lang_dev(ctx.handle(), &config, c.logits, c.dtype, c.batch, c.U, c.T, c.vocabWithBlank, c.rowStride, c.encLen, c.audioFrames,
                                                c.t0, c.isLast, c.globalOffset, c.emitAfter, c.maxOut, c.tokens, c.timestamps, c.durations, c.confidences, c.counts,
                                                c.finalTime, c.finalU, c.status, language->classes, static_cast<int32_t>(script(language->language)),
                                                language->useBlocklist ? 1 : 0, language->topK, language->routes, language->swapCounts),
                  "fa_tdt_greedy_logits_lang_dev");
    }
};

// ------------------------------------------------------------------------------------------------------------------ streaming RNN-T
// RnntDecoder.decodeWithEOU (Sources/FluidAudio/ASR/Parakeet/Streaming/RnntDecoder.swift:73-127) and NemotronVocabularyBias
// (Streaming/Nemotron/NemotronVocabularyBias.swift:55-340) over fa_rnnt_greedy_logits_dev and fa_rnnt_bias_build / _candidates.
// Texts arrive FOLDED (lowercased().precomposedStringWithCanonicalMapping) and past the caller's letter-count guard (usableSurfaces,
// :203-212): both need Unicode tables this header does not carry.
struct RnntConfig {
    int32_t blankId = 1024, eouId = -1, maxSymbolsPerStep = 10;
    RnntConfig() { fa_rnnt_config c; fa_rnnt_default_config(&c); blankId = c.blank_id; eouId = c.eou_id; maxSymbolsPerStep = c.max_symbols_per_step; }
    fa_rnnt_config c() const { return fa_rnnt_config{blankId, eouId, maxSymbolsPerStep}; }
};
struct CustomVocabularyTerm {      // the fields the bias reads
    std::string text;
    std::optional<float> weight;
    std::vector<std::string> aliases;
};
class NemotronVocabularyBias {
public:
    static constexpr float defaultBoost = FA_RNNT_BIAS_DEFAULT_BOOST, maxBoost = FA_RNNT_BIAS_MAX_BOOST;
    struct Candidate {
        int tokenId;
        float boost;
    };
    static float effectiveBoost(const CustomVocabularyTerm &term, float fallback = defaultBoost) {   // :196-199
        return fa_rnnt_bias_effective_boost(term.weight ? 1 : 0, term.weight.value_or(0.0f), fallback);
    }
    // init?(terms:pieces:defaultBoost:) (:126-182): nullopt when no usable term remains.  pieces[id]: the folded piece, empty optional = no piece.
    static std::optional<NemotronVocabularyBias> make(const std::vector<CustomVocabularyTerm> &terms, const std::vector<std::optional<std::string>> &pieces,
                                                      float fallback = defaultBoost) {
        std::vector<const char *> surfaces, texts(pieces.size());
        std::vector<float> boosts;
        auto checked = [](const std::string &s) -> const char * {
            if (s.find('\0') != std::string::npos) throw Error(FA_INVALID_ARGUMENT, "fa_rnnt_bias_build", "a text holds a NUL");
            return s.c_str();
        };
        for (const CustomVocabularyTerm &t : terms) {
            const float boost = effectiveBoost(t, fallback);
            if (!(boost > 0.0f)) continue;                                                            // :206
            surfaces.push_back(checked(t.text)); boosts.push_back(boost);
            for (const std::string &a : t.aliases) { surfaces.push_back(checked(a)); boosts.push_back(boost); }
        }
        NemotronVocabularyBias b;
        b.advances_.resize(pieces.size());
        for (size_t i = 0; i < pieces.size(); ++i) {
            texts[i] = pieces[i] ? checked(*pieces[i]) : nullptr;
            b.advances_[i] = pieces[i] && !pieces[i]->empty() && !(pieces[i]->front() == '<' && pieces[i]->back() == '>');   // :152
        }
        int64_t words = 0;
        const int32_t n = static_cast<int32_t>(surfaces.size()), vocab = static_cast<int32_t>(pieces.size());
        fa_status st = fa_rnnt_bias_build(texts.data(), vocab, surfaces.data(), boosts.data(), n, nullptr, 0, &words, &b.tailCap_);
        if (st != FA_SUCCESS) throw Error(st, "fa_rnnt_bias_build", "text that is not UTF-8, or a term longer than FA_RNNT_BIAS_MAX_FORM scalars");
        if (words == 0) return std::nullopt;
        b.blob_.resize(static_cast<size_t>(words));
        st = fa_rnnt_bias_build(texts.data(), vocab, surfaces.data(), boosts.data(), n, b.blob_.data(), words, &words, &b.tailCap_);
        if (st != FA_SUCCESS) throw Error(st, "fa_rnnt_bias_build");
        return b;
    }
    // observe(_:) (:254-261).  The device entry carries the tail's scalars; this mirror keeps the ids that put them there: a token with
    // a piece adds at least one scalar, so the last tailCap of them hold the whole tail.
    void observe(int tokenId) {
        if (tokenId < 0 || static_cast<size_t>(tokenId) >= advances_.size() || !advances_[static_cast<size_t>(tokenId)]) return;
        observed_.push_back(tokenId);
        if (observed_.size() > static_cast<size_t>(tailCap_)) observed_.erase(observed_.begin());
    }
    void resetMatchState() { observed_.clear(); }                                                    // :265-268
    std::vector<Candidate> candidates() const {                                                       // :280-306; ascending token id
        int32_t count = 0;
        const int32_t n = static_cast<int32_t>(observed_.size());
        fa_status st = fa_rnnt_bias_candidates(blob_.data(), static_cast<int64_t>(blob_.size()), observed_.data(), n, nullptr, nullptr, 0, &count);
        if (st != FA_SUCCESS && st != FA_OUTPUT_TOO_SMALL) throw Error(st, "fa_rnnt_bias_candidates");
        std::vector<int32_t> ids(static_cast<size_t>(count));
        std::vector<float> boosts(static_cast<size_t>(count));
        if (count > 0) {
            st = fa_rnnt_bias_candidates(blob_.data(), static_cast<int64_t>(blob_.size()), observed_.data(), n, ids.data(), boosts.data(), count, &count);
            if (st != FA_SUCCESS) throw Error(st, "fa_rnnt_bias_candidates");
        }
        std::vector<Candidate> out(ids.size());
        for (size_t i = 0; i < ids.size(); ++i) out[i] = Candidate{ids[i], boosts[i]};
        return out;
    }
    const std::vector<int32_t> &blob() const { return blob_; }   // upload as it is: d_bias / bias_words of fa_rnnt_greedy_logits_dev
    int32_t tailCap() const { return tailCap_; }

private:
    std::vector<int32_t> blob_, observed_;
    std::vector<char> advances_;
    int32_t tailCap_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------ AED greedy decoding
// The host loops round the attention encoder-decoder models over the fa_aed_* entries: CoherePipeline (Sources/FluidAudio/ASR/Cohere/
// CoherePipeline.swift:525-959: transcribeLong's windows, mergeTokenStreams, encoderValidFrames, decodeCacheExternal's step, the two masks)
// and CanaryManager (Sources/FluidAudio/ASR/Canary/CanaryManager.swift:50-275: the same windows and merge, makeDecoderContext,
// greedyDecode).  The networks and every device buffer are the caller's; pointers named d... are DEVICE pointers.
struct AedConfig {
    int32_t mode = FA_AED_FEED_TOKEN, vocab = 16384, eosId = 3, maxSeq = 108, maxNew = 108, noRepeatNgram = 3;
    float repetitionPenalty = 1.1f;
    int32_t windowTokens = 32, minMatch = 4;
    int64_t chunkSamples = 560000, hopSamples = 480000;
    static AedConfig preset(int32_t model) {
        fa_aed_config c;
        fa_aed_default_config(&c, model);
        AedConfig a;
        a.mode = c.mode; a.vocab = c.vocab; a.eosId = c.eos_id; a.maxSeq = c.max_seq; a.maxNew = c.max_new; a.noRepeatNgram = c.no_repeat_ngram;
        a.repetitionPenalty = c.repetition_penalty; a.windowTokens = c.window_tokens; a.minMatch = c.min_match; a.chunkSamples = c.chunk_samples; a.hopSamples = c.hop_samples;
        return a;
    }
    static AedConfig cohere() { return preset(FA_AED_MODEL_COHERE); }   // CohereAsrConfig + transcribe's defaults
    static AedConfig canary() { return preset(FA_AED_MODEL_CANARY); }   // CanaryConfig
    fa_aed_config c() const { return fa_aed_config{mode, vocab, eosId, maxSeq, maxNew, noRepeatNgram, repetitionPenalty, windowTokens, minMatch, 0, chunkSamples, hopSamples}; }
    int32_t maxOut() const { const fa_aed_config k = c(); return fa_aed_max_out(&k); }
    int64_t stateBytes(int32_t batch) const { const fa_aed_config k = c(); return fa_aed_state_bytes(&k, batch); }
};
// The decode state of a batch: dState (stateBytes(batch) bytes) and the arrays of the feed in use are the caller's device buffers.
struct AedDecodeState {
    AedConfig config;
    int32_t batch = 0;
    void *dState = nullptr;
    int32_t *dInputId = nullptr, *dPositionId = nullptr;   // token feed [batch]
    void *dSelfMask = nullptr;                             // token feed, optional [batch][maxSeq]
    int32_t maskDtype = FA_DTYPE_F32;
    int32_t *dInputIds = nullptr;                          // sequence feed [batch][maxSeq]
    float *dDecoderMask = nullptr;
    struct Result {
        std::vector<std::vector<int32_t>> tokens;
        std::vector<int32_t> reasons, steps;               // FA_AED_RUNNING / FA_AED_END_EOS / FA_AED_END_CAP
    };
    void begin(Context &ctx, const int32_t *dPrompts, int32_t promptStride, const std::vector<int32_t> &promptLens) const {
        const fa_aed_config k = config.c();
        if (static_cast<size_t>(batch) != promptLens.size()) throw Error(FA_INVALID_ARGUMENT, "fa_aed_begin_dev", "one prompt length per utterance");
        ctx.check(fa_aed_begin_dev(ctx.handle(), &k, batch, dPrompts, promptStride, promptLens.data(), dState, dInputId, dPositionId, dSelfMask, maskDtype, dInputIds, dDecoderMask),
                  "fa_aed_begin_dev");
    }
    // one launch, nothing allocated, nothing waited for
    void step(Context &ctx, const void *dLogits, int32_t dtype, int64_t rowStride) const {
        const fa_aed_config k = config.c();
        ctx.check(fa_aed_step_dev(ctx.handle(), &k, batch, dState, dLogits, dtype, rowStride, dInputId, dPositionId, dSelfMask, maskDtype, dInputIds, dDecoderMask), "fa_aed_step_dev");
    }
    Result finish(Context &ctx) const {
        const fa_aed_config k = config.c();
        const int32_t m = config.maxOut();
        std::vector<int32_t> tok(static_cast<size_t>(std::max(batch, 0)) * static_cast<size_t>(std::max(m, 0)) + 1), cnt(static_cast<size_t>(std::max(batch, 0)) + 1);
        Result r;
        r.reasons.resize(cnt.size());
        r.steps.resize(cnt.size());
        ctx.check(fa_aed_finish(ctx.handle(), &k, batch, dState, m, tok.data(), cnt.data(), r.reasons.data(), r.steps.data()), "fa_aed_finish");
        r.reasons.resize(static_cast<size_t>(batch));
        r.steps.resize(static_cast<size_t>(batch));
        for (int32_t b = 0; b < batch; ++b) r.tokens.emplace_back(tok.begin() + static_cast<ptrdiff_t>(b) * m, tok.begin() + static_cast<ptrdiff_t>(b) * m + cnt[static_cast<size_t>(b)]);
        return r;
    }
    // CanaryManager.greedyDecode's hidden row pos - 1 of every running utterance -> dHidden float[batch][D]
    void gatherHidden(Context &ctx, const void *dDec, int32_t dtype, int32_t S, int32_t D, int64_t strideB, int64_t strideS, int64_t strideD, float *dHidden) const {
        const fa_aed_config k = config.c();
        ctx.check(fa_aed_gather_hidden_dev(ctx.handle(), &k, batch, dState, dDec, dtype, S, D, strideB, strideS, strideD, dHidden), "fa_aed_gather_hidden_dev");
    }
};
struct AedLongForm {   // what CoherePipeline and CanaryManager share: the window loop and mergeTokenStreams
    struct Window { int64_t start, length; };
    static std::vector<std::vector<Window>> planWindows(const AedConfig &config, const std::vector<int64_t> &samples) {
        const fa_aed_config k = config.c();
        std::vector<int64_t> range(samples.size() + 1);
        int64_t count = 0;
        fa_status st = fa_aed_plan_windows(&k, samples.data(), static_cast<int64_t>(samples.size()), range.data(), nullptr, nullptr, 0, &count);
        if (st != FA_SUCCESS) throw Error(st, "fa_aed_plan_windows");
        std::vector<int64_t> starts(static_cast<size_t>(count) + 1), lens(static_cast<size_t>(count) + 1);
        st = fa_aed_plan_windows(&k, samples.data(), static_cast<int64_t>(samples.size()), range.data(), starts.data(), lens.data(), count, &count);
        if (st != FA_SUCCESS) throw Error(st, "fa_aed_plan_windows");
        std::vector<std::vector<Window>> out(samples.size());
        for (size_t r = 0; r < samples.size(); ++r)
            for (int64_t w = range[r]; w < range[r + 1]; ++w) out[r].push_back(Window{starts[static_cast<size_t>(w)], lens[static_cast<size_t>(w)]});
        return out;
    }
    // the fold of mergeTokenStreams over every recording's windows in one device call; answers in input order
    static std::vector<std::vector<int32_t>> mergeRecordings(Context &ctx, const std::vector<std::vector<std::vector<int32_t>>> &recordings, int windowTokens = 32,
                                                             int minMatch = 4) {
        std::vector<int32_t> flat;
        std::vector<int64_t> offsets{0}, range{0}, outRange{0};
        for (const auto &r : recordings) {
            for (const auto &w : r) { flat.insert(flat.end(), w.begin(), w.end()); offsets.push_back(static_cast<int64_t>(flat.size())); }
            range.push_back(static_cast<int64_t>(offsets.size()) - 1);
            outRange.push_back(static_cast<int64_t>(flat.size()));
        }
        AedConfig config;
        config.windowTokens = windowTokens; config.minMatch = minMatch;
        const fa_aed_config k = config.c();
        std::vector<int32_t> out(flat.size() + 1), counts(recordings.size() + 1);
        flat.push_back(0);
        ctx.check(fa_aed_merge_windows(ctx.handle(), &k, flat.data(), offsets.data(), range.data(), static_cast<int64_t>(recordings.size()), out.data(), outRange.data(),
                                       counts.data(), nullptr, nullptr), "fa_aed_merge_windows");
        std::vector<std::vector<int32_t>> merged(recordings.size());
        for (size_t r = 0; r < recordings.size(); ++r) merged[r].assign(out.begin() + outRange[r], out.begin() + outRange[r] + counts[r]);
        return merged;
    }
    static std::vector<int32_t> mergeTokenStreams(Context &ctx, const std::vector<int32_t> &prefix, const std::vector<int32_t> &suffix, int windowTokens = 32, int minMatch = 4) {
        return mergeRecordings(ctx, {{prefix, suffix}}, windowTokens, minMatch)[0];
    }
};
struct CoherePipeline : AedLongForm {
    static int encoderValidFrames(int64_t featureLength, int encoderSeqLen, int melFrames = 3500, int encoderFrames = 438) {
        return fa_aed_encoder_valid_frames(featureLength, encoderSeqLen, melFrames, encoderFrames);
    }
    // buildCrossAttentionMask for a batch: dMask [batch][encoderSeqLen] of dtype (FA_DTYPE_F32 / FA_DTYPE_F16 bits), dValid int32[batch]
    static void buildCrossAttentionMask(Context &ctx, const int32_t *dValid, int32_t batch, int32_t encoderSeqLen, int32_t dtype, void *dMask) {
        ctx.check(fa_aed_cross_mask_dev(ctx.handle(), dValid, batch, encoderSeqLen, dtype, dMask), "fa_aed_cross_mask_dev");
    }
    // buildSelfAttentionMask: the static row of a step is AedDecodeState's dSelfMask; the dynamic variant is step + 1 zeros
    static std::vector<float> buildDynamicSelfAttentionMask(int step) { return std::vector<float>(static_cast<size_t>(std::max(step, 0)) + 1, 0.0f); }
    static std::vector<std::vector<Window>> planWindows(const std::vector<int64_t> &samples) { return AedLongForm::planWindows(AedConfig::cohere(), samples); }
};
struct CanaryManager : AedLongForm {
    // makeDecoderContext for a batch: dEnc [batch][D][T] at element strides -> dEmb float[batch][T][D], dMask float[batch][T]
    static void makeDecoderContext(Context &ctx, const void *dEnc, int32_t dtype, int32_t batch, int32_t D, int32_t T, int64_t strideB, int64_t strideD, int64_t strideT,
                                   const int32_t *dLen, float *dEmb, float *dMask) {
        ctx.check(fa_aed_encoder_context_dev(ctx.handle(), dEnc, dtype, batch, D, T, strideB, strideD, strideT, dLen, dEmb, dMask), "fa_aed_encoder_context_dev");
    }
    static std::vector<std::vector<Window>> planWindows(const std::vector<int64_t> &samples) { return AedLongForm::planWindows(AedConfig::canary(), samples); }
};

// ------------------------------------------------------------------------------------------------------------------ TDT long-form merging
// ChunkProcessor's fold of mergeChunks over a recording's windows and enforceMonotonicTimestamps (Sources/FluidAudio/ASR/Parakeet/
// SlidingWindow/TDT/ChunkProcessor.swift:843-855, 952-1219) over fa_tdt_merge_windows: the windows of one or more recordings in one
// device call.  The safe set and the case table (spliceSafeTokenIds, caseVariantCanonicalIds) are the caller's, as tables over the
// vocabulary; collapseSeamWordDuplicates, repairSeamGaps and the planning of chunk starts are out of scope.
struct ChunkProcessor {
    struct TokenWindow {          // ChunkProcessor.TokenWindow
        int token = 0, timestamp = 0, duration = 0;
        float confidence = 0.0f;
    };
    using Window = std::vector<TokenWindow>;
    struct Merged {
        std::vector<TokenWindow> tokens;
        fa_status status = FA_SUCCESS;          // FA_OUTPUT_TOO_SMALL cannot happen here: the slices get the safe bound
        std::vector<int32_t> seamRoutes;        // one per window, FA_TDT_MERGE_NO_SEAM for the first
    };
    double frameSeconds = 1280.0 / 16000.0, overlapSeconds = 2.0;
    std::vector<uint8_t> spliceSafe;            // with hasSpliceSafe: uint8[vocab]
    std::vector<int32_t> caseCanon;             // with hasCaseCanon: int32[vocab], -1 without an entry
    bool hasSpliceSafe = false, hasCaseCanon = false;

    // every recording's windows (global timestamps) in one call; answers in input order
    std::vector<Merged> mergeRecordings(fa_ctx *ctx, const std::vector<std::vector<Window>> &recordings) const {
        const int64_t n = static_cast<int64_t>(recordings.size());
        std::vector<Merged> out(recordings.size());
        if (n == 0) return out;
        size_t maxOut = 1, windows = 0;
        for (const auto &r : recordings)
            for (const Window &w : r) { maxOut = std::max(maxOut, w.size()); ++windows; }
        std::vector<int32_t> tok(windows * maxOut), time(windows * maxOut), dur(windows * maxOut), count(windows);
        std::vector<float> conf(windows * maxOut);
        std::vector<int64_t> windowRange{0}, outRange{0};
        size_t at = 0;
        for (const auto &r : recordings) {
            int64_t cap = 0;
            for (size_t k = 0; k < r.size(); ++k, ++at) {
                for (size_t i = 0; i < r[k].size(); ++i) {
                    tok[at * maxOut + i] = r[k][i].token; time[at * maxOut + i] = r[k][i].timestamp;
                    dur[at * maxOut + i] = r[k][i].duration; conf[at * maxOut + i] = r[k][i].confidence;
                }
                count[at] = static_cast<int32_t>(r[k].size());
                cap += static_cast<int64_t>(r[k].size()) * (k == 0 ? 1 : 2);   // a right token is emitted at most twice
            }
            windowRange.push_back(static_cast<int64_t>(at));
            outRange.push_back(outRange.back() + cap);
        }
        const size_t total = static_cast<size_t>(outRange.back());
        std::vector<int32_t> oTok(total + 1), oTime(total + 1), oDur(total + 1), counts(recordings.size()), statuses(recordings.size()), routes(windows + 1);
        std::vector<float> oConf(total + 1);
        const size_t vocab = hasSpliceSafe ? spliceSafe.size() : (hasCaseCanon ? caseCanon.size() : 0);
        if (hasSpliceSafe && hasCaseCanon && spliceSafe.size() != caseCanon.size()) throw Error(FA_INVALID_ARGUMENT, "fa_tdt_merge_windows", "the tables disagree about the vocabulary");
        static const uint8_t noSafe = 0;
        static const int32_t noCanon = -1;
        const fa_tdt_merge_config cfg{frameSeconds, overlapSeconds};
        const fa_status st = fa_tdt_merge_windows(ctx, &cfg, tok.data(), time.data(), dur.data(), conf.data(), count.data(), static_cast<int32_t>(maxOut), windowRange.data(), n,
                                                  hasSpliceSafe ? (spliceSafe.empty() ? &noSafe : spliceSafe.data()) : nullptr,
                                                  hasCaseCanon ? (caseCanon.empty() ? &noCanon : caseCanon.data()) : nullptr, static_cast<int32_t>(vocab), oTok.data(),
                                                  oTime.data(), oDur.data(), oConf.data(), outRange.data(), counts.data(), statuses.data(), routes.data());
        if (st != FA_SUCCESS) throw Error(st, "fa_tdt_merge_windows", ctx ? fa_ctx_last_error(ctx) : nullptr);
        for (size_t r = 0; r < recordings.size(); ++r) {
            out[r].status = static_cast<fa_status>(statuses[r]);
            for (int32_t i = 0; i < counts[r]; ++i) {
                const size_t q = static_cast<size_t>(outRange[r]) + static_cast<size_t>(i);
                out[r].tokens.push_back(TokenWindow{oTok[q], oTime[q], oDur[q], oConf[q]});
            }
            out[r].seamRoutes.assign(routes.begin() + windowRange[r], routes.begin() + windowRange[r + 1]);
        }
        return out;
    }
    // mergeChunks(left, right) alone, without the clamp's effect on later seams: a recording of two windows
    Merged mergeRecording(fa_ctx *ctx, const std::vector<Window> &windows) const { return mergeRecordings(ctx, {windows})[0]; }
    Merged mergeRecording(Context &ctx, const std::vector<Window> &windows) const { return mergeRecording(ctx.handle(), windows); }
};

// ------------------------------------------------------------------------------------------------------------------ CTC word spotting
// CtcKeywordSpotter.spotKeywordsFromLogProbs (…/WordSpotting/CtcKeywordSpotter.swift:191-254) and the two scans of CtcDPAlgorithm it and
// the rescorer call (CtcDPAlgorithm.swift:250-392), over fa_ctc_kws_spot_batch / fa_ctc_kws_score_windows.  A term carries its token ids
// (the tokenizer is not part of this library); the caller leaves out terms shorter than minTermLength.  The threshold rule (:217-222) and
// startTime = frame x frameDuration (:232-233) are applied here; the DP runs on the device.
struct CtcKeywordSpotter {
    static constexpr int32_t wildcardTokenId = FA_KWS_WILDCARD;   // ContextBiasingConstants
    static constexpr int32_t defaultBlankId = 1024;
    static constexpr float defaultMinSpotterScore = -15.0f;
    struct Term {
        std::string text;
        std::vector<int32_t> tokenIds;
    };
    struct KeywordDetection {
        size_t term = 0;   // index into the vocabulary's terms
        float score = 0.0f;
        int32_t totalFrames = 0, startFrame = 0, endFrame = 0;
        double startTime = 0.0, endTime = 0.0;
    };
    struct Spot {
        float score;
        int32_t startFrame, endFrame;
    };
    using LogProbs = std::vector<std::vector<float>>;   // [T][V], every frame of one length

    static std::vector<KeywordDetection> spotKeywordsFromLogProbs(fa_ctx *ctx, const LogProbs &logProbs, double frameDuration, const std::vector<Term> &terms,
                                                                  std::optional<float> minScore = std::nullopt, int32_t blankId = defaultBlankId) {
        std::vector<KeywordDetection> out;
        const int32_t T = static_cast<int32_t>(logProbs.size());
        if (T == 0) return out;   // :198-200
        std::vector<std::vector<int32_t>> ids;
        std::vector<float> thresholds;
        for (const Term &t : terms) {
            ids.push_back(t.tokenIds);
            thresholds.push_back(fa_kws_adjusted_threshold(minScore ? 1 : 0, minScore.value_or(0.0f), static_cast<int32_t>(t.tokenIds.size())));
        }
        for (const fa_kws_detection &d : spot(ctx, logProbs, ids, thresholds, true, blankId))
            out.push_back(KeywordDetection{static_cast<size_t>(d.keyword), d.score, T, d.start_frame, d.end_frame, static_cast<double>(d.start_frame) * frameDuration,
                                           static_cast<double>(d.end_frame) * frameDuration});
        return out;
    }
    static std::vector<Spot> ctcWordSpotMultiple(fa_ctx *ctx, const LogProbs &logProbs, const std::vector<int32_t> &keywordTokens,
                                                 float minScore = defaultMinSpotterScore, bool mergeOverlap = true, int32_t blankId = defaultBlankId) {
        std::vector<Spot> out;
        for (const fa_kws_detection &d : spot(ctx, logProbs, {keywordTokens}, {minScore}, mergeOverlap, blankId)) out.push_back(Spot{d.score, d.start_frame, d.end_frame});
        return out;
    }
    static Spot ctcWordSpotConstrained(fa_ctx *ctx, const LogProbs &logProbs, const std::vector<int32_t> &keywordTokens, int32_t searchStartFrame,
                                       int32_t searchEndFrame, int32_t blankId = defaultBlankId) {
        int32_t T = 0, V = 0;
        const std::vector<float> flat = flatten(logProbs, T, V);
        const int64_t off[2] = {0, static_cast<int64_t>(keywordTokens.size())};
        const fa_kws_window w{0, 0, searchStartFrame, searchEndFrame};
        fa_kws_detection d{};
        const fa_status st = fa_ctc_kws_score_windows(ctx, flat.data(), 1, T, V, V, static_cast<int64_t>(T) * V, nullptr, keywordTokens.data(), off, 1, &w, 1, blankId, &d);
        if (st != FA_SUCCESS) throw Error(st, "fa_ctc_kws_score_windows", ctx ? fa_ctx_last_error(ctx) : nullptr);
        return Spot{d.score, d.start_frame, d.end_frame};
    }
    static std::vector<KeywordDetection> spotKeywordsFromLogProbs(Context &ctx, const LogProbs &logProbs, double frameDuration, const std::vector<Term> &terms,
                                                                  std::optional<float> minScore = std::nullopt, int32_t blankId = defaultBlankId) {
        return spotKeywordsFromLogProbs(ctx.handle(), logProbs, frameDuration, terms, minScore, blankId);
    }

private:
    static std::vector<float> flatten(const LogProbs &lp, int32_t &T, int32_t &V) {
        T = static_cast<int32_t>(lp.size());
        V = T > 0 ? static_cast<int32_t>(lp[0].size()) : 1;
        std::vector<float> flat;
        flat.reserve(static_cast<size_t>(T) * static_cast<size_t>(V));
        for (const auto &row : lp) {
            if (static_cast<int32_t>(row.size()) != V) throw Error(FA_INVALID_ARGUMENT, "CtcKeywordSpotter: frames of different lengths");
            flat.insert(flat.end(), row.begin(), row.end());
        }
        if (V < 1) V = 1;
        return flat;
    }
    static std::vector<fa_kws_detection> spot(fa_ctx *ctx, const LogProbs &logProbs, const std::vector<std::vector<int32_t>> &keywords, const std::vector<float> &thresholds,
                                              bool mergeOverlap, int32_t blankId) {
        int32_t T = 0, V = 0;
        const std::vector<float> flat = flatten(logProbs, T, V);
        std::vector<int32_t> tokens;
        std::vector<int64_t> off{0};
        for (const auto &k : keywords) {
            tokens.insert(tokens.end(), k.begin(), k.end());
            off.push_back(static_cast<int64_t>(tokens.size()));
        }
        std::vector<fa_kws_detection> dets(64);
        int64_t count = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {   // the second call has room for the count the first one reported
            const fa_status st = fa_ctc_kws_spot_batch(ctx, flat.data(), 1, T, V, V, static_cast<int64_t>(T) * V, nullptr, tokens.data(), off.data(),
                                                       static_cast<int32_t>(keywords.size()), thresholds.data(), blankId, mergeOverlap ? 1 : 0, dets.data(),
                                                       static_cast<int64_t>(dets.size()), &count, nullptr);
            if (st == FA_OUTPUT_TOO_SMALL && attempt == 0) { dets.resize(static_cast<size_t>(count)); continue; }
            if (st != FA_SUCCESS) throw Error(st, "fa_ctc_kws_spot_batch", ctx ? fa_ctx_last_error(ctx) : nullptr);
            break;
        }
        dets.resize(static_cast<size_t>(count));
        return dets;
    }
};

// VocabularyRescorer's term-centric path (…/Rescorer/VocabularyRescorer+TokenRescoring.swift:693-1034, :272-307, +TokenEvaluation.swift:29-173)
// for one utterance, over fa_vocab_rescore_build / _candidates / _decide.  A word or a form is a row of symbols, one per Character of the
// normalized string (any injective numbering, `space` for the space): normalizeForSimilarity, both tokenizers, the word timings and the
// stopword lists are the caller's, as are preserveCapitalization and the rebuilt text.  The spotter-anchored rescue is not part of it.
struct VocabularyRescorer {
    static constexpr int32_t space = FA_VR_SPACE;
    static constexpr float minSimilarityFloor = 0.50f;   // ContextBiasingConstants
    using Symbols = std::vector<int32_t>;
    using LogProbs = CtcKeywordSpotter::LogProbs;
    struct Term {
        int32_t charCount = 0;                       // vocabTerm.count
        std::optional<float> minSimilarity;
        std::vector<Symbols> forms;                  // buildNormalizedForms' order, the canonical form first (it may be empty)
        std::vector<int32_t> ctcTokenIds, altTokenIds;   // encode(text); encodeWithoutBoundary(text), empty: none
    };
    struct Word {
        Symbols symbols;                             // normalizeForSimilarity(word), possibly empty
        bool stopword = false, multiWordStopword = false;
        double startTime = 0.0, endTime = 0.0;
    };
    struct Decision {
        std::vector<fa_vr_candidate> candidates;
        std::vector<fa_vr_verdict> verdicts;         // one per candidate
        std::vector<int32_t> applied;                // indices into candidates, in application order
    };

    std::vector<Term> terms;
    std::vector<int32_t> blob;
    fa_vr_decide_config config;

    explicit VocabularyRescorer(std::vector<Term> vocabulary, int32_t minTermLength = 3) : terms(std::move(vocabulary)) {
        fa_vocab_rescore_default_config(&config);
        std::vector<int32_t> counts, symbols;
        std::vector<float> mins;
        std::vector<int64_t> termRows{0}, rowOffsets{0};
        for (const Term &t : terms) {
            counts.push_back(t.charCount);
            mins.push_back(t.minSimilarity.value_or(-1.0f));
            for (const Symbols &f : t.forms) {
                symbols.insert(symbols.end(), f.begin(), f.end());
                rowOffsets.push_back(static_cast<int64_t>(symbols.size()));
            }
            termRows.push_back(static_cast<int64_t>(rowOffsets.size()) - 1);
        }
        symbols.push_back(0);   // never an empty array
        counts.push_back(0);
        mins.push_back(0.0f);
        char text[192] = "";
        int64_t need = 0;
        for (int pass = 0; pass < 2; ++pass) {   // the size, then the blob
            const fa_status st = fa_vocab_rescore_build(counts.data(), mins.data(), termRows.data(), rowOffsets.data(), symbols.data(), static_cast<int32_t>(terms.size()),
                                                        minTermLength, pass ? blob.data() : nullptr, pass ? need : 0, &need, text, static_cast<int64_t>(sizeof(text)));
            if (st != FA_SUCCESS) throw Error(st, "fa_vocab_rescore_build", text);
            if (need == 0) break;
            blob.resize(static_cast<size_t>(need));
        }
    }

    // the candidate records of one utterance in the reference's append order
    std::vector<fa_vr_candidate> candidates(fa_ctx *ctx, const std::vector<Word> &words, float minSimilarity = minSimilarityFloor) const {
        std::vector<int32_t> symbols;
        std::vector<int64_t> wordOffsets{0};
        std::vector<uint8_t> flags;
        for (const Word &w : words) {
            symbols.insert(symbols.end(), w.symbols.begin(), w.symbols.end());
            wordOffsets.push_back(static_cast<int64_t>(symbols.size()));
            flags.push_back(static_cast<uint8_t>((w.stopword ? FA_VR_WORD_STOPWORD : 0) | (w.multiWordStopword ? FA_VR_WORD_MULTI_WORD_STOPWORD : 0)));
        }
        symbols.push_back(0);
        flags.push_back(0);
        const int64_t utterance[2] = {0, static_cast<int64_t>(words.size())};
        std::vector<fa_vr_candidate> out(64);
        int64_t count = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {   // the second call has room for the count the first one reported
            const fa_status st = fa_vocab_rescore_candidates(ctx, blob.data(), static_cast<int64_t>(blob.size()), utterance, 1, wordOffsets.data(), symbols.data(), flags.data(),
                                                             minSimilarity, out.data(), static_cast<int64_t>(out.size()), &count, nullptr);
            if (st == FA_OUTPUT_TOO_SMALL && attempt == 0) { out.resize(static_cast<size_t>(count)); continue; }
            if (st != FA_SUCCESS) throw Error(st, "fa_vocab_rescore_candidates", ctx ? fa_ctx_last_error(ctx) : nullptr);
            break;
        }
        out.resize(static_cast<size_t>(count));
        return out;
    }

    // evaluateCTCMatch for each candidate and arbitratePendingReplacements; phraseTokens[c]: encode(originalPhrase) of candidate c
    Decision decide(fa_ctx *ctx, const LogProbs &logProbs, const std::vector<Word> &words, std::vector<fa_vr_candidate> found,
                    const std::vector<std::vector<int32_t>> &phraseTokens, const std::vector<uint8_t> &occupied = {}) const {
        if (phraseTokens.size() != found.size() || (!occupied.empty() && occupied.size() != words.size()))
            throw Error(FA_INVALID_ARGUMENT, "VocabularyRescorer: a token row per candidate and an occupied byte per word are required");
        const int32_t T = static_cast<int32_t>(logProbs.size());
        int32_t V = T > 0 ? static_cast<int32_t>(logProbs[0].size()) : 1;
        std::vector<float> flat;
        for (const auto &row : logProbs) {
            if (static_cast<int32_t>(row.size()) != V) throw Error(FA_INVALID_ARGUMENT, "VocabularyRescorer: frames of different lengths");
            flat.insert(flat.end(), row.begin(), row.end());
        }
        if (V < 1) V = 1;
        flat.push_back(0.0f);
        std::vector<double> starts, ends;
        for (const Word &w : words) { starts.push_back(w.startTime); ends.push_back(w.endTime); }
        starts.push_back(0.0);
        ends.push_back(0.0);
        const auto pack = [](const auto &rows, auto row_of, std::vector<int32_t> &tokens, std::vector<int64_t> &off) {
            off.assign(1, 0);
            for (const auto &r : rows) {
                const std::vector<int32_t> &t = row_of(r);
                tokens.insert(tokens.end(), t.begin(), t.end());
                off.push_back(static_cast<int64_t>(tokens.size()));
            }
            tokens.push_back(0);
        };
        std::vector<int32_t> termTokens, altTokens, phrases;
        std::vector<int64_t> termOff, altOff, phraseOff;
        pack(terms, [](const Term &t) -> const std::vector<int32_t> & { return t.ctcTokenIds; }, termTokens, termOff);
        pack(terms, [](const Term &t) -> const std::vector<int32_t> & { return t.altTokenIds; }, altTokens, altOff);
        pack(phraseTokens, [](const std::vector<int32_t> &t) -> const std::vector<int32_t> & { return t; }, phrases, phraseOff);
        const int64_t utterance[2] = {0, static_cast<int64_t>(words.size())};
        Decision d;
        d.candidates = std::move(found);
        d.verdicts.resize(d.candidates.size() + 1);
        d.applied.resize(d.candidates.size() + 1);
        int64_t applied = 0;
        const fa_status st = fa_vocab_rescore_decide(ctx, flat.data(), 1, T, V, V, static_cast<int64_t>(T) * V, nullptr, &config, d.candidates.data(),
                                                     static_cast<int64_t>(d.candidates.size()), utterance, starts.data(), ends.data(), static_cast<int32_t>(terms.size()),
                                                     termTokens.data(), termOff.data(), altTokens.data(), altOff.data(), phrases.data(), phraseOff.data(),
                                                     occupied.empty() ? nullptr : occupied.data(), d.verdicts.data(), d.applied.data(), &applied);
        if (st != FA_SUCCESS) throw Error(st, "fa_vocab_rescore_decide", ctx ? fa_ctx_last_error(ctx) : nullptr);
        d.verdicts.resize(d.candidates.size());
        d.applied.resize(static_cast<size_t>(applied));
        return d;
    }

    // The term-centric path of ctcTokenRescore round the caller's tokenizer: encode(first word, span length) gives the tokens of the
    // original phrase — the raw words of the span joined by a space — and is asked once per distinct span.
    template <class Encode>
    Decision ctcTokenRescore(fa_ctx *ctx, const LogProbs &logProbs, const std::vector<Word> &words, Encode &&encode, float minSimilarity = minSimilarityFloor) const {
        std::vector<fa_vr_candidate> found = candidates(ctx, words, minSimilarity);
        std::map<std::pair<int32_t, int32_t>, std::vector<int32_t>> cache;
        std::vector<std::vector<int32_t>> phraseTokens;
        for (const fa_vr_candidate &c : found) {
            const auto key = std::make_pair(c.first_word, c.span_len);
            auto at = cache.find(key);
            if (at == cache.end()) at = cache.emplace(key, encode(c.first_word, c.span_len)).first;
            phraseTokens.push_back(at->second);
        }
        return decide(ctx, logProbs, words, std::move(found), phraseTokens);
    }
};

// ------------------------------------------------------------------------------------------------------------------ Paraformer
// ParaformerConfig (Sources/FluidAudio/ASR/Paraformer/ParaformerConfig.swift:8-39)
struct ParaformerConfig {
    static constexpr int featureDim = 560, encoderDim = 512;
    static constexpr int decoderEncFrames = 512, decoderMaxTokens = 128;
    static constexpr int blankId = 0, sosId = 1, eosId = 2;
    static constexpr float cifThreshold = 1.0f, cifTailThreshold = 0.45f;
    static constexpr int sampleRate = 16000;
    static constexpr float waveformScale = 32768.0f;
    static int pickEncoderBucket(int frames) {
        for (const int b : {128, 256, 512, 1024, 1800})
            if (b >= frames) return b;
        return 1800;
    }
};

// ParaformerCif (Sources/FluidAudio/ASR/Paraformer/ParaformerCif.swift:19-55) over fa_paraformer_cif: one utterance, every token (the
// token budget of the call is the frame count + 1, so nothing is clamped), as the Swift routine returns them.
struct ParaformerCif {
    using Rows = std::vector<std::vector<float>>;
    struct Fired {
        Rows embeds;
        std::vector<int> fireFrames;
    };
    static Fired integrateAndFireWithFireFrames(fa_ctx *ctx, const Rows &encRows, const std::vector<float> &alphas) {
        const int32_t T = static_cast<int32_t>(encRows.size());
        const int32_t dim = T > 0 ? static_cast<int32_t>(encRows[0].size()) : ParaformerConfig::encoderDim;
        if (alphas.size() < encRows.size() || dim < 1) throw Error(FA_INVALID_ARGUMENT, "ParaformerCif: an alpha per row and rows of one length >= 1 are required");
        std::vector<float> flat;
        flat.reserve(static_cast<size_t>(T) * static_cast<size_t>(dim));
        for (const auto &row : encRows) {
            if (static_cast<int32_t>(row.size()) != dim) throw Error(FA_INVALID_ARGUMENT, "ParaformerCif: rows of different lengths");
            flat.insert(flat.end(), row.begin(), row.end());
        }
        fa_paraformer_cif_config cfg;
        fa_paraformer_cif_default_config(&cfg);
        cfg.max_tokens = T + 1;
        cfg.enc_frames = 0;
        std::vector<float> ac(static_cast<size_t>(T + 1) * static_cast<size_t>(dim));
        std::vector<int32_t> frames(static_cast<size_t>(T) + 1);
        int32_t tokens = 0, fires = 0;
        static const float none = 0.0f;   // an utterance without frames still gets arrays
        const fa_status st = fa_paraformer_cif(ctx, &cfg, T > 0 ? flat.data() : &none, FA_DTYPE_F32, 1, T, dim, dim, static_cast<int64_t>(T) * dim,
                                               T > 0 ? alphas.data() : &none, T, nullptr, ac.data(), nullptr, &tokens, &fires, frames.data());
        if (st != FA_SUCCESS) throw Error(st, "fa_paraformer_cif", ctx ? fa_ctx_last_error(ctx) : nullptr);
        Fired out;
        for (int32_t l = 0; l < fires; ++l) {
            out.embeds.emplace_back(ac.begin() + static_cast<int64_t>(l) * dim, ac.begin() + static_cast<int64_t>(l + 1) * dim);
            out.fireFrames.push_back(frames[static_cast<size_t>(l)]);
        }
        return out;
    }
    static Rows integrateAndFire(fa_ctx *ctx, const Rows &encRows, const std::vector<float> &alphas) { return integrateAndFireWithFireFrames(ctx, encRows, alphas).embeds; }
    static Fired integrateAndFireWithFireFrames(Context &ctx, const Rows &encRows, const std::vector<float> &alphas) { return integrateAndFireWithFireFrames(ctx.handle(), encRows, alphas); }
    static Rows integrateAndFire(Context &ctx, const Rows &encRows, const std::vector<float> &alphas) { return integrateAndFire(ctx.handle(), encRows, alphas); }
};

// TimestampedSegment (Sources/FluidAudio/ASR/Paraformer/ParaformerManager.swift:12-22)
struct TimestampedSegment {
    double startTime = 0.0, endTime = 0.0;
    std::string text;
};

// The host side of ParaformerManager behind the decoder's argmax (ParaformerManager.swift): decode (:450-463) and decodeWithTimestamps
// (:134-257) over fa_paraformer_timestamps — the fires, the envelope and the walk run on the device; the charList filter becomes the
// keep table, and the BPE merge of the emission (:228-256) runs here on the raw spans.  The vocabulary maps an id to its piece.
struct ParaformerManager {
    using Vocabulary = std::map<int, std::string>;
    static bool special(int id) { return id == ParaformerConfig::blankId || id == ParaformerConfig::sosId || id == ParaformerConfig::eosId; }
    // decode (:450-463): pieces joined, U+2581 -> blank, blanks and tabs trimmed
    static std::string decode(const std::vector<int> &ids, const Vocabulary &vocabulary) {
        std::string joined;
        for (const int id : ids) {
            if (special(id)) continue;
            const auto it = vocabulary.find(id);
            if (it != vocabulary.end()) joined += it->second;
        }
        const std::string boundary = "\xE2\x96\x81";
        std::string out;
        for (size_t i = 0; i < joined.size();) {
            if (joined.compare(i, boundary.size(), boundary) == 0) { out += ' '; i += boundary.size(); }
            else out += joined[i++];
        }
        const size_t a = out.find_first_not_of(" \t");
        return a == std::string::npos ? std::string() : out.substr(a, out.find_last_not_of(" \t") - a + 1);
    }
    // the charList filter (:146-156) as a table over the ids 0 ... size - 1
    static std::vector<uint8_t> keepTable(const Vocabulary &vocabulary, int size) {
        std::vector<uint8_t> keep(static_cast<size_t>(size > 0 ? size : 0), 0);
        for (const auto &kv : vocabulary)
            if (kv.first >= 0 && kv.first < size && !special(kv.first) && !kv.second.empty()) keep[static_cast<size_t>(kv.first)] = 1;
        return keep;
    }
    // the raw spans (:141-226) of one utterance: tokenIds is the argmax of the decoder's tokenCount positions
    static std::vector<fa_paraformer_span> rawSpans(fa_ctx *ctx, const std::vector<int> &tokenIds, const Vocabulary &vocabulary, const std::vector<float> &alphas,
                                                    const std::vector<float> &audio) {
        fa_paraformer_cif_config cfg;
        fa_paraformer_cif_default_config(&cfg);
        cfg.max_tokens = static_cast<int32_t>(tokenIds.size() > 0 ? tokenIds.size() : 1);
        int size = 0;
        for (const int id : tokenIds) size = id >= size ? id + 1 : size;
        const std::vector<uint8_t> keep = keepTable(vocabulary, size);
        std::vector<int32_t> ids(static_cast<size_t>(cfg.max_tokens), 0);
        for (size_t i = 0; i < tokenIds.size(); ++i) ids[i] = tokenIds[i];
        const int32_t n = static_cast<int32_t>(tokenIds.size());
        const int64_t off[2] = {0, static_cast<int64_t>(audio.size())};
        std::vector<fa_paraformer_span> spans(tokenIds.size());
        int64_t count = 0;
        static const float none = 0.0f;
        static const uint8_t no_keep = 0;
        const fa_status st = fa_paraformer_timestamps(ctx, &cfg, alphas.empty() ? &none : alphas.data(), static_cast<int64_t>(alphas.size()), 1,
                                                      static_cast<int32_t>(alphas.size()), nullptr, ids.data(), &n, keep.empty() ? &no_keep : keep.data(), size,
                                                      audio.empty() ? &none : audio.data(), off, spans.data(), static_cast<int64_t>(spans.size()), &count, nullptr);
        if (st != FA_SUCCESS) throw Error(st, "fa_paraformer_timestamps", ctx ? fa_ctx_last_error(ctx) : nullptr);
        spans.resize(static_cast<size_t>(count));
        return spans;
    }
    // the emission (:228-256): pieces[i] is the text of span i
    static std::vector<TimestampedSegment> segments(const std::vector<std::string> &pieces, const std::vector<fa_paraformer_span> &spans) {
        const std::string boundary = "\xE2\x96\x81", cont = "@@";
        const auto has_prefix = [](const std::string &s, const std::string &p) { return s.compare(0, p.size(), p) == 0; };
        const auto has_suffix = [](const std::string &s, const std::string &p) { return s.size() >= p.size() && s.compare(s.size() - p.size(), p.size(), p) == 0; };
        std::vector<TimestampedSegment> out;
        for (size_t i = 0; i < spans.size(); ++i) {
            std::string text = pieces[i];
            double end = spans[i].end;
            const double start = spans[i].start;
            while (has_suffix(text, cont)) {
                text.resize(text.size() - cont.size());
                ++i;
                if (i < spans.size()) {
                    text += has_prefix(pieces[i], boundary) ? pieces[i].substr(boundary.size()) : pieces[i];
                    end = spans[i].end;
                }
            }
            if (has_prefix(text, boundary)) text = text.substr(boundary.size());
            if (!text.empty()) out.push_back(TimestampedSegment{start >= 0 ? start : 0.0, end, text});
        }
        return out;
    }
    // decodeWithTimestamps (:134-257) behind the argmax
    static std::vector<TimestampedSegment> decodeWithTimestamps(fa_ctx *ctx, const std::vector<int> &tokenIds, const Vocabulary &vocabulary, const std::vector<float> &alphas,
                                                                const std::vector<float> &audio) {
        const std::vector<fa_paraformer_span> spans = rawSpans(ctx, tokenIds, vocabulary, alphas, audio);
        std::vector<std::string> pieces;
        for (const fa_paraformer_span &s : spans) pieces.push_back(vocabulary.at(tokenIds[static_cast<size_t>(s.token_index)]));
        return segments(pieces, spans);
    }
    static std::vector<TimestampedSegment> decodeWithTimestamps(Context &ctx, const std::vector<int> &tokenIds, const Vocabulary &vocabulary, const std::vector<float> &alphas,
                                                                const std::vector<float> &audio) {
        return decodeWithTimestamps(ctx.handle(), tokenIds, vocabulary, alphas, audio);
    }
};

// ------------------------------------------------------------------------------------------------------------------ VAD
// VadConfig (Sources/FluidAudio/VAD/VadTypes.swift:4-21) without the CoreML fields
struct VadConfig {
    float defaultThreshold = 0.85f;
};

// VadSegmentationConfig (VadTypes.swift:24-91).  The preconditions of its init are the refusals of the entries it is handed to.
struct VadSegmentationConfig {
    double minSpeechDuration = 0.15, minSilenceDuration = 0.75, maxSpeechDuration = 14.0, speechPadding = 0.1;
    float silenceThresholdForSplit = 0.3f;
    std::optional<float> negativeThreshold;
    float negativeThresholdOffset = 0.15f;
    double minSilenceAtMaxSpeech = 0.098;
    bool useMaxPossibleSilenceAtMaxSpeech = true;
    float effectiveNegativeThreshold(float baseThreshold) const {
        if (negativeThreshold) return *negativeThreshold;
        const float x = baseThreshold - negativeThresholdOffset;
        return 0.01f >= x ? 0.01f : x;
    }
    fa_vad_segmentation_config abi(const VadConfig &vad = VadConfig{}) const {
        fa_vad_segmentation_config c{};
        c.default_threshold = vad.defaultThreshold;
        c.min_speech_duration = minSpeechDuration; c.min_silence_duration = minSilenceDuration; c.max_speech_duration = maxSpeechDuration; c.speech_padding = speechPadding;
        c.silence_threshold_for_split = silenceThresholdForSplit;
        c.has_negative_threshold = negativeThreshold ? 1 : 0; c.negative_threshold = negativeThreshold.value_or(0.0f); c.negative_threshold_offset = negativeThresholdOffset;
        c.min_silence_at_max_speech = minSilenceAtMaxSpeech;
        c.use_max_possible_silence_at_max_speech = useMaxPossibleSilenceAtMaxSpeech ? 1 : 0;
        return c;
    }
};

// VadSegment (VadTypes.swift:137-164)
struct VadSegment {
    double startTime = 0.0, endTime = 0.0;
    double duration() const { return endTime - startTime; }
    int64_t startSample(int sampleRate) const { return static_cast<int64_t>(startTime * static_cast<double>(sampleRate)); }
    int64_t endSample(int sampleRate) const { return static_cast<int64_t>(endTime * static_cast<double>(sampleRate)); }
    int64_t sampleCount(int sampleRate) const { return endSample(sampleRate) - startSample(sampleRate); }
};

// VadStreamState (VadTypes.swift:166-187) without the model's state, which stays with whoever runs the network
struct VadStreamState {
    bool triggered = false;
    std::optional<int64_t> tempEndSample;
    int64_t processedSamples = 0;
    static VadStreamState initial() { return VadStreamState{}; }
    fa_vad_stream_state abi() const { return fa_vad_stream_state{triggered ? 1 : 0, tempEndSample ? 1 : 0, tempEndSample.value_or(0), processedSamples}; }
    static VadStreamState from(const fa_vad_stream_state &s) {
        VadStreamState r;
        r.triggered = s.triggered != 0;
        if (s.has_temp_end) r.tempEndSample = s.temp_end_sample;
        r.processedSamples = s.processed_samples;
        return r;
    }
};

// VadStreamEvent (VadTypes.swift:189-207)
struct VadStreamEvent {
    enum class Kind { speechStart = FA_VAD_SPEECH_START, speechEnd = FA_VAD_SPEECH_END };
    Kind kind = Kind::speechStart;
    int64_t sampleIndex = 0;
    std::optional<double> time;
    bool isStart() const { return kind == Kind::speechStart; }
    bool isEnd() const { return kind == Kind::speechEnd; }
};

// The host arithmetic of VadManager round the network (VadManager+SpeechSegmentation.swift, VadManager+Streaming.swift, VadManager.swift)
// for ONE recording or stream; the batched forms are the C entries.
struct VadManager {
    static constexpr int chunkSize = 4096, contextLength = 64, sampleRate = 16000, modelInputSize = 4160;
    VadConfig config;
    // segmentSpeech(from:totalSamples:config:) on the probabilities the network gave, one per chunk
    std::vector<VadSegment> segmentSpeech(Context &ctx, const std::vector<float> &probabilities, int64_t totalSamples, const VadSegmentationConfig &cfg = {}) const {
        const fa_vad_segmentation_config c = cfg.abi(config);
        const int64_t range[2] = {0, static_cast<int64_t>(probabilities.size())};
        std::vector<fa_vad_segment> segs(probabilities.size());                  // at most one segment per frame
        int64_t count = 0;
        ctx.check(fa_vad_segments(ctx.handle(), &c, probabilities.data(), range, &totalSamples, 1, segs.data(), static_cast<int64_t>(segs.size()), &count, nullptr), "fa_vad_segments");
        std::vector<VadSegment> out;
        for (int64_t i = 0; i < count; ++i) out.push_back(VadSegment{segs[static_cast<size_t>(i)].start_time, segs[static_cast<size_t>(i)].end_time});
        return out;
    }
    // the audio_input rows of processAudioSamples: [chunks][4160]
    static std::vector<float> modelInputs(Context &ctx, const std::vector<float> &samples) {
        const int64_t offsets[2] = {0, static_cast<int64_t>(samples.size())};
        int64_t range[2] = {0, 0};
        std::vector<float> rows(static_cast<size_t>(fa_vad_chunk_count(offsets[1])) * modelInputSize);
        ctx.check(fa_vad_pack_chunks(ctx.handle(), samples.data(), offsets, 1, rows.data(), fa_vad_chunk_count(offsets[1]), range), "fa_vad_pack_chunks");
        return rows;
    }
    // streamingStateMachine for one chunk
    std::optional<VadStreamEvent> streamingStateMachine(Context &ctx, float probability, int32_t chunkSampleCount, VadStreamState &state, const VadSegmentationConfig &cfg = {},
                                                        bool returnSeconds = false, int timeResolution = 1) const {
        const fa_vad_segmentation_config c = cfg.abi(config);
        fa_vad_stream_state st = state.abi();
        fa_vad_stream_event ev{};
        const int32_t one = 1;
        int64_t count = 0;
        ctx.check(fa_vad_stream_advance(ctx.handle(), &c, &probability, &one, &chunkSampleCount, 1, 1, &st, returnSeconds ? 1 : 0, timeResolution, &ev, 1, &count), "fa_vad_stream_advance");
        state = VadStreamState::from(st);
        if (count == 0) return std::nullopt;
        VadStreamEvent out;
        out.kind = static_cast<VadStreamEvent::Kind>(ev.kind);
        out.sampleIndex = ev.sample_index;
        if (returnSeconds) out.time = ev.time;
        return out;
    }
};

// ---- FSMN-VAD (Sources/FluidAudio/VAD/Fsmn/FsmnVadManager.swift) for ONE recording; the batched forms are the C entries
struct FsmnVadSegment {                      // :5-8
    int64_t startMs = 0, endMs = 0;
    bool operator==(const FsmnVadSegment &o) const { return startMs == o.startMs && endMs == o.endMs; }
};

// The decision constants the reference keeps private (:37-45); their bounds are the refusals of the entries they are handed to.
struct FsmnVadConfig {
    float silenceThreshold = 0.2f;
    int windowFrames = 20, silToSpeech = 15, speechToSil = 15, maxEndSilenceFrames = 80, lookbackFrames = 20, lookaheadFrames = 10, maxSegmentFrames = 6000, frameMs = 10;
    fa_fsmn_vad_config abi() const {
        return fa_fsmn_vad_config{silenceThreshold, windowFrames, silToSpeech, speechToSil, maxEndSilenceFrames, lookbackFrames, lookaheadFrames, maxSegmentFrames, frameMs};
    }
};

struct FsmnVadManager {
    static constexpr int hopSamples = 160, fbankWindowSamples = 400, lfrPadFrames = 2, featureDim = 400;
    FsmnVadConfig config;
    static int64_t lfrFrameCount(int64_t samples) { return fa_fsmn_vad_frame_count(samples); }
    // the chunks concatenateChunks scores, with the frame each one's first kept frame lands at
    static std::vector<fa_fsmn_vad_chunk> chunks(int64_t sampleCount, int64_t *frames = nullptr) {
        int64_t count = 0, chunkRange[2] = {0, 0}, frameRange[2] = {0, 0};
        fa_status st = fa_fsmn_vad_plan_chunks(&sampleCount, 1, nullptr, 0, &count, chunkRange, frameRange);
        std::vector<fa_fsmn_vad_chunk> out(static_cast<size_t>(count));
        if (st == FA_SUCCESS) st = fa_fsmn_vad_plan_chunks(&sampleCount, 1, out.data(), count, &count, chunkRange, frameRange);
        if (st != FA_SUCCESS) throw Error(st, "fa_fsmn_vad_plan_chunks");
        if (frames) *frames = frameRange[1];
        return out;
    }
    // decide on the silence probabilities the scorer gave, one per 10 ms frame
    std::vector<FsmnVadSegment> decide(Context &ctx, const std::vector<float> &silence) const {
        const fa_fsmn_vad_config c = config.abi();
        const int64_t range[2] = {0, static_cast<int64_t>(silence.size())};
        std::vector<fa_fsmn_vad_segment> segs(silence.size());                   // at most one segment per frame
        int64_t count = 0;
        ctx.check(fa_fsmn_vad_segments(ctx.handle(), &c, silence.data(), range, 1, segs.data(), static_cast<int64_t>(segs.size()), &count, nullptr), "fa_fsmn_vad_segments");
        std::vector<FsmnVadSegment> out;
        for (int64_t i = 0; i < count; ++i) out.push_back(FsmnVadSegment{segs[static_cast<size_t>(i)].start_ms, segs[static_cast<size_t>(i)].end_ms});
        return out;
    }
};

// ---- TDT long-form: planning the windows (ChunkProcessor.swift; the C entries are batched over recordings, this is ONE recording)
struct ChunkLayout {                         // chunkLayout's tuple (:140-161)
    int64_t chunkSamples = 0, strideSamples = 0, melContextSamples = 0, warmupPrefixSamples = 0;
};

struct ChunkStartDecision {                  // :20-23
    int64_t start = 0;
    bool useWarmupPrefix = false;
};

struct TdtWindowPlanner {
    bool melChunkContext = true;             // ASRConfig.melChunkContext
    bool silenceAligned = false;             // preferSilenceAlignment: !melChunkContext && modelVersion == .v3
    int warmupPrefixFrames = 0;              // path B of the arbitration: 7
    bool endAligned = true;                  // supportsSuppressedPrefix(modelVersion)
    double overlapSeconds = 2.0;

    fa_tdt_window_config abi() const {
        fa_tdt_window_config c;
        fa_tdt_window_default_config(&c);
        c.overlap_seconds = overlapSeconds;
        c.mel_chunk_context = melChunkContext ? 1 : 0; c.silence_aligned = silenceAligned ? 1 : 0;
        c.warmup_prefix_frames = warmupPrefixFrames; c.end_aligned = endAligned ? 1 : 0;
        return c;
    }
    ChunkLayout chunkLayout() const {
        const fa_tdt_window_config c = abi();
        ChunkLayout l;
        const fa_status st = fa_tdt_window_layout(&c, &l.chunkSamples, &l.strideSamples, &l.melContextSamples, &l.warmupPrefixSamples);
        if (st != FA_SUCCESS) throw Error(st, "fa_tdt_window_layout");
        return l;
    }
    // the windows process decodes, in order; speechEnd (nullable): speechEndSamples
    std::vector<fa_tdt_window> plan(Context &ctx, const std::vector<float> &samples, int64_t *speechEnd = nullptr) const {
        const fa_tdt_window_config c = abi();
        const int64_t offsets[2] = {0, static_cast<int64_t>(samples.size())};
        const int64_t bound = fa_tdt_window_count_bound(&c, offsets[1]);
        if (bound < 0) throw Error(FA_INVALID_ARGUMENT, "fa_tdt_window_count_bound");
        std::vector<fa_tdt_window> windows(static_cast<size_t>(bound));
        int64_t range[2] = {0, 0}, end = 0;
        int32_t status = FA_SUCCESS;
        ctx.check(fa_tdt_plan_windows(ctx.handle(), &c, samples.data(), offsets, 1, windows.data(), bound, range, nullptr, nullptr, nullptr, nullptr, nullptr, &end, &status),
                  "fa_tdt_plan_windows");
        if (status != FA_SUCCESS) throw Error(static_cast<fa_status>(status), "fa_tdt_plan_windows", "the recording holds a non-finite energy");
        windows.resize(static_cast<size_t>(range[1]));
        if (speechEnd) *speechEnd = end;
        return windows;
    }
    std::vector<ChunkStartDecision> chunkStartDecisions(Context &ctx, const std::vector<float> &samples) const {
        std::vector<ChunkStartDecision> out;
        for (const fa_tdt_window &w : plan(ctx, samples)) out.push_back(ChunkStartDecision{w.chunk_start, w.use_warmup_prefix != 0});
        return out;
    }
    int64_t speechEndSamples(Context &ctx, const std::vector<float> &samples) const {
        int64_t end = 0;
        (void)plan(ctx, samples, &end);
        return end;
    }
    // padAudioIfNeeded of every window: [windows][maxModelSamples]
    std::vector<float> packWindows(Context &ctx, const std::vector<float> &samples, const std::vector<fa_tdt_window> &windows) const {
        const fa_tdt_window_config c = abi();
        const int64_t offsets[2] = {0, static_cast<int64_t>(samples.size())};
        std::vector<float> rows(windows.size() * static_cast<size_t>(c.max_model_samples));
        ctx.check(fa_tdt_pack_windows(ctx.handle(), &c, samples.data(), offsets, 1, windows.data(), static_cast<int64_t>(windows.size()), rows.data(),
                                      static_cast<int64_t>(windows.size()), nullptr), "fa_tdt_pack_windows");
        return rows;
    }
    float adaptiveSpeechRmsThreshold(Context &ctx, const std::vector<float> &samples) const {
        const fa_tdt_window_config c = abi();
        const int64_t offsets[2] = {0, static_cast<int64_t>(samples.size())};
        float threshold = 0.0f;
        ctx.check(fa_tdt_speech_gate(ctx.handle(), &c, samples.data(), offsets, 1, nullptr, &threshold, nullptr, 0, nullptr, nullptr, nullptr), "fa_tdt_speech_gate");
        return threshold;
    }
    // threshold: the recording's adaptive one when not given
    double speechLikeSeconds(Context &ctx, const std::vector<float> &samples, int64_t startSample, int64_t endSample, std::optional<float> threshold = std::nullopt) const {
        const fa_tdt_window_config c = abi();
        const int64_t offsets[2] = {0, static_cast<int64_t>(samples.size())};
        const fa_tdt_span span{0, 0, startSample, endSample};
        const float over = threshold.value_or(0.0f);
        double seconds = 0.0;
        ctx.check(fa_tdt_speech_gate(ctx.handle(), &c, samples.data(), offsets, 1, threshold ? &over : nullptr, nullptr, &span, 1, nullptr, &seconds, nullptr), "fa_tdt_speech_gate");
        return seconds;
    }
};

// ---- online diarizer: the speaker database (Diarizer/Clustering/SpeakerManager.swift, SpeakerTypes.swift; the C entries are batched over
// streams, this is ONE stream).  Ids are ints from 1, dates are caller-supplied ticks, names stay with the caller (fluidaudio_hip.h).
struct SpeakerUtilities {
    static std::vector<float> l2Normalize(const std::vector<float> &e) {             // VDSPOperations.l2Normalize with the library's sums
        if (e.size() != 256) throw Error(FA_INVALID_ARGUMENT, "fa_speaker_l2_normalize", "an embedding has 256 elements");
        std::vector<float> out(256);
        (void)fa_speaker_l2_normalize(e.data(), out.data());
        return out;
    }
    static float cosineDistance(const std::vector<float> &a, const std::vector<float> &b) {   // infinity for sizes other than 256, as for a mismatch
        if (a.size() != 256 || b.size() != 256) return std::numeric_limits<float>::infinity();
        return fa_speaker_cosine_distance(a.data(), b.data());
    }
    static bool validateEmbedding(const std::vector<float> &e, float minMagnitude = 0.1f) {
        return e.size() == 256 && fa_speaker_validate_embedding(e.data(), minMagnitude) != 0;
    }
};

struct RawEmbedding {               // SpeakerTypes.swift:208-218 without the UUID: normalised when it is made
    std::vector<float> embedding;
    int64_t timestamp = 0;
    RawEmbedding() = default;
    explicit RawEmbedding(const std::vector<float> &e, int64_t timestamp = 0) : embedding(SpeakerUtilities::l2Normalize(e)), timestamp(timestamp) {}
};

struct Speaker {                    // the fields of Speaker the database keeps; currentEmbedding is normalised by the constructor (Speaker.init)
    int id = 0;
    std::vector<float> currentEmbedding;
    float duration = 0.0f;
    int64_t createdAt = 0, updatedAt = 0;
    int updateCount = 1;
    std::vector<RawEmbedding> rawEmbeddings;   // oldest first
    bool isPermanent = false;
    Speaker() = default;
    Speaker(int id, const std::vector<float> &currentEmbedding, float duration = 0.0f, int64_t createdAt = 0, int64_t updatedAt = 0, bool isPermanent = false)
        : id(id), currentEmbedding(SpeakerUtilities::l2Normalize(currentEmbedding)), duration(duration), createdAt(createdAt), updatedAt(updatedAt), isPermanent(isPermanent) {}
};

struct TimedSpeakerSegment {        // SpeakerTypes / DiarizerTypes: a record of fa_online_chunk_finish_dev with the caller's embedding beside it
    int speakerId = 0;              // the database's id (the reference: a string)
    std::vector<float> embedding;
    float startTimeSeconds = 0.0f, endTimeSeconds = 0.0f, qualityScore = 0.0f;
    float durationSeconds() const { return endTimeSeconds - startTimeSeconds; }
    static TimedSpeakerSegment from(const fa_online_segment &r, const float *embedding256 = nullptr) {
        TimedSpeakerSegment t;
        t.speakerId = r.id; t.startTimeSeconds = r.start; t.endTimeSeconds = r.end; t.qualityScore = r.quality;
        if (embedding256) t.embedding.assign(embedding256, embedding256 + 256);
        return t;
    }
};

class SpeakerManager {
  public:
    static constexpr int embeddingSize = 256;
    struct Pair { int speakerToMerge, destination; };
    SpeakerManager(Context &ctx, float speakerThreshold = 0.65f, float embeddingThreshold = 0.45f, float minSpeechDuration = 1.0f, int maxSpeakers = 16, int rawCapacity = 50)
        : ctx_(ctx) {
        fa_speaker_db_default_config(&cfg_);
        cfg_.speaker_threshold = speakerThreshold; cfg_.embedding_threshold = embeddingThreshold; cfg_.min_speech_duration = minSpeechDuration;
        cfg_.max_speakers = maxSpeakers; cfg_.raw_capacity = rawCapacity;
        ctx_.check(fa_speaker_db_create(ctx_.handle(), &cfg_, 1, &db_), "fa_speaker_db_create");
    }
    ~SpeakerManager() { fa_speaker_db_destroy(db_); }
    SpeakerManager(const SpeakerManager &) = delete;
    SpeakerManager &operator=(const SpeakerManager &) = delete;

    fa_speaker_assignment lastAssignment{0, -1, FA_SPEAKER_SKIPPED, 0.0f};   // the path the last assignSpeaker took
    // assignSpeaker (:135-177): nil for an embedding of another size, too short a duration, a non-finite embedding or a full table
    std::optional<Speaker> assignSpeaker(const std::vector<float> &embedding, float speechDuration, int64_t tick = 0) {
        if (embedding.size() != static_cast<size_t>(embeddingSize)) return std::nullopt;
        ctx_.check(fa_speaker_db_assign(ctx_.handle(), db_, embedding.data(), &speechDuration, nullptr, 1, tick, &lastAssignment), "fa_speaker_db_assign");
        return lastAssignment.id ? getSpeaker(lastAssignment.id) : std::nullopt;
    }
    std::pair<std::optional<int>, float> findSpeaker(const std::vector<float> &embedding, std::optional<float> speakerThreshold = std::nullopt) {   // :184-191
        const std::vector<float> d = distances(embedding);
        const std::vector<int> ids = slotIds();
        int best = -1;
        for (size_t s = 0; s < d.size(); ++s)
            if (d[s] < (best < 0 ? std::numeric_limits<float>::infinity() : d[best])) best = static_cast<int>(s);
        if (best >= 0 && d[best] <= speakerThreshold.value_or(cfg_.speaker_threshold)) return {ids[best], d[best]};
        return {std::nullopt, std::numeric_limits<float>::infinity()};
    }
    std::vector<std::pair<int, float>> findMatchingSpeakers(const std::vector<float> &embedding, std::optional<float> speakerThreshold = std::nullopt) {   // :198-212
        const std::vector<float> d = distances(embedding);
        const std::vector<int> ids = slotIds();
        std::vector<std::pair<int, float>> out;
        for (size_t s = 0; s < d.size(); ++s)
            if (ids[s] && d[s] <= speakerThreshold.value_or(cfg_.speaker_threshold)) out.emplace_back(ids[s], d[s]);
        std::stable_sort(out.begin(), out.end(), [](const auto &a, const auto &b) { return a.second < b.second; });
        return out;
    }
    std::vector<Pair> findMergeablePairs(std::optional<float> speakerThreshold = std::nullopt, bool excludeIfBothPermanent = true) {   // :282-328
        const int cap = std::max(1, cfg_.max_speakers * (cfg_.max_speakers - 1) / 2);
        std::vector<fa_speaker_pair> rec(static_cast<size_t>(cap));
        int32_t n = 0;
        ctx_.check(fa_speaker_db_mergeable_pairs(ctx_.handle(), db_, speakerThreshold.value_or(cfg_.speaker_threshold), excludeIfBothPermanent ? 1 : 0, rec.data(), cap, &n),
                   "fa_speaker_db_mergeable_pairs");
        std::vector<Pair> out;
        for (int i = 0; i < n; ++i) out.push_back(Pair{rec[static_cast<size_t>(i)].source_id, rec[static_cast<size_t>(i)].destination_id});
        return out;
    }
    void upsertSpeaker(const Speaker &s) {   // :552-606; pass a Speaker's fields as they are: an existing id is overwritten without normalising
        std::vector<float> raws;
        for (const RawEmbedding &r : s.rawEmbeddings) raws.insert(raws.end(), r.embedding.begin(), r.embedding.end());
        if (s.currentEmbedding.size() != static_cast<size_t>(embeddingSize) || raws.size() != s.rawEmbeddings.size() * embeddingSize)
            throw Error(FA_INVALID_ARGUMENT, "fa_speaker_db_upsert", "an embedding has 256 elements");
        const fa_speaker_info info{s.id, -1, static_cast<int32_t>(s.rawEmbeddings.size()), s.updateCount, s.isPermanent ? 1 : 0, s.duration, s.createdAt, s.updatedAt};
        ctx_.check(fa_speaker_db_upsert(ctx_.handle(), db_, 0, &info, s.currentEmbedding.data(), raws.empty() ? nullptr : raws.data()), "fa_speaker_db_upsert");
    }
    std::optional<Speaker> getSpeaker(int id) {
        fa_speaker_info info{};
        std::vector<float> cur(embeddingSize), raws(static_cast<size_t>(cfg_.raw_capacity) * embeddingSize);
        ctx_.check(fa_speaker_db_get(ctx_.handle(), db_, 0, id, &info, cur.data(), raws.data(), cfg_.raw_capacity), "fa_speaker_db_get");
        if (info.id == 0) return std::nullopt;
        Speaker s;
        s.id = info.id; s.currentEmbedding = cur; s.duration = info.duration; s.createdAt = info.created_tick; s.updatedAt = info.updated_tick;
        s.updateCount = info.update_count; s.isPermanent = info.is_permanent != 0;
        for (int k = 0; k < info.raw_count; ++k) {
            RawEmbedding r;
            r.embedding.assign(raws.begin() + static_cast<ptrdiff_t>(k) * embeddingSize, raws.begin() + static_cast<ptrdiff_t>(k + 1) * embeddingSize);
            s.rawEmbeddings.push_back(std::move(r));
        }
        return s;
    }
    bool hasSpeaker(int id) { return getSpeaker(id).has_value(); }
    void makeSpeakerPermanent(int id) { ctx_.check(fa_speaker_db_set_permanent(ctx_.handle(), db_, 0, id, 1), "fa_speaker_db_set_permanent"); }
    void revokePermanence(int id) { ctx_.check(fa_speaker_db_set_permanent(ctx_.handle(), db_, 0, id, 0), "fa_speaker_db_set_permanent"); }
    void removeSpeaker(int id, bool keepIfPermanent = true) { ctx_.check(fa_speaker_db_remove(ctx_.handle(), db_, 0, id, keepIfPermanent ? 1 : 0), "fa_speaker_db_remove"); }
    void removeSpeakersInactive(int64_t sinceTick, bool keepIfPermanent = true) {
        ctx_.check(fa_speaker_db_remove_inactive(ctx_.handle(), db_, 0, sinceTick, keepIfPermanent ? 1 : 0), "fa_speaker_db_remove_inactive");
    }
    void reset(bool keepIfPermanent = false) { ctx_.check(fa_speaker_db_reset(ctx_.handle(), db_, 0, keepIfPermanent ? 1 : 0), "fa_speaker_db_reset"); }
    int speakerCount() {
        int32_t n = 0;
        ctx_.check(fa_speaker_db_count(ctx_.handle(), db_, &n), "fa_speaker_db_count");
        return n;
    }
    std::vector<int> speakerIds() {   // ascending, as the reference sorts them
        std::vector<int32_t> ids(static_cast<size_t>(cfg_.max_speakers));
        int32_t n = 0;
        ctx_.check(fa_speaker_db_ids(ctx_.handle(), db_, 0, ids.data(), &n), "fa_speaker_db_ids");
        std::vector<int> out(ids.begin(), ids.begin() + n);
        std::sort(out.begin(), out.end());
        return out;
    }

  private:
    std::vector<float> distances(const std::vector<float> &embedding) {
        if (embedding.size() != static_cast<size_t>(embeddingSize)) throw Error(FA_INVALID_ARGUMENT, "fa_speaker_db_distances", "an embedding has 256 elements");
        std::vector<float> d(static_cast<size_t>(cfg_.max_speakers));
        ctx_.check(fa_speaker_db_distances(ctx_.handle(), db_, embedding.data(), 1, d.data(), nullptr), "fa_speaker_db_distances");
        return d;
    }
    std::vector<int> slotIds() {      // the id in every slot, 0 for a free one
        std::vector<int> out(static_cast<size_t>(cfg_.max_speakers), 0);
        for (const int id : speakerIds()) {
            fa_speaker_info info{};
            ctx_.check(fa_speaker_db_get(ctx_.handle(), db_, 0, id, &info, nullptr, nullptr, 0), "fa_speaker_db_get");
            if (info.slot >= 0) out[static_cast<size_t>(info.slot)] = id;
        }
        return out;
    }
    Context &ctx_;
    fa_speaker_db_config cfg_{};
    fa_speaker_db *db_ = nullptr;
};

// ---- streaming Sortformer: the state between chunks (Diarizer/Sortformer/SortformerTypes.swift, SortformerStateUpdater.swift; the C
// entries are batched over streams, this is ONE stream on host arrays).
struct SortformerConfig {           // SortformerConfig with its presets; the clamps are the library's (fa_sortformer_stream_geometry)
    fa_sortformer_stream_config c{};
    SortformerConfig() { fa_sortformer_stream_default_config(&c); }
    explicit SortformerConfig(int preset) {
        if (fa_sortformer_stream_preset_config(preset, &c) != FA_SUCCESS) throw Error(FA_INVALID_ARGUMENT, "fa_sortformer_stream_preset_config", "no such preset");
    }
    static SortformerConfig balanced() { return SortformerConfig(FA_SORTFORMER_STREAM_PRESET_BALANCED); }
    static SortformerConfig highContext() { return SortformerConfig(FA_SORTFORMER_STREAM_PRESET_HIGH_CONTEXT); }
    static SortformerConfig efficient() { return SortformerConfig(FA_SORTFORMER_STREAM_PRESET_EFFICIENT); }
    fa_sortformer_stream_geometry_info geometry() const {
        fa_sortformer_stream_geometry_info g{};
        if (fa_sortformer_stream_geometry(&c, &g) != FA_SUCCESS) throw Error(FA_INVALID_ARGUMENT, "fa_sortformer_stream_geometry", "the config is refused");
        return g;
    }
    int chunkMelFrames() const { return geometry().chunk_mel_frames; }
    // getNextChunkFeaturesLocked on a buffer of featLength frames
    fa_sortformer_chunk nextChunk(int64_t featLength, int64_t startFeat) const {
        fa_sortformer_chunk k{};
        if (fa_sortformer_stream_chunk_plan(&c, &featLength, &startFeat, 1, &k) != FA_SUCCESS) throw Error(FA_INVALID_ARGUMENT, "fa_sortformer_stream_chunk_plan", "refused");
        return k;
    }
    // SortformerFeatureLoader: every chunk of a file; numChunks (nullable) as the loader computes it
    std::vector<fa_sortformer_chunk> fileChunks(int64_t featLength, int64_t featSeqLength, int64_t *numChunks = nullptr) const {
        int64_t n = 0;
        const fa_status st = fa_sortformer_stream_file_chunks(&c, featLength, featSeqLength, nullptr, 0, &n, numChunks);
        if (st != FA_SUCCESS && st != FA_OUTPUT_TOO_SMALL) throw Error(st, "fa_sortformer_stream_file_chunks", "refused");
        std::vector<fa_sortformer_chunk> out(static_cast<size_t>(n));
        if (n > 0 && fa_sortformer_stream_file_chunks(&c, featLength, featSeqLength, out.data(), n, &n, numChunks) != FA_SUCCESS)
            throw Error(FA_RUNTIME_ERROR, "fa_sortformer_stream_file_chunks", "the count changed");
        return out;
    }
};

struct StreamingUpdateResult {      // SortformerTypes.swift:398-420
    std::vector<float> confirmed, tentative;
    int numSpeakers = 0;
    int status = FA_SORTFORMER_STREAM_OK;   // the reference throws; here the update's per-stream status
    int confirmedFrameCount() const { return numSpeakers ? static_cast<int>(confirmed.size()) / numSpeakers : 0; }
    int tentativeFrameCount() const { return numSpeakers ? static_cast<int>(tentative.size()) / numSpeakers : 0; }
};

class SortformerStreamingState {    // SortformerStreamingState + SortformerStateUpdater.streamingUpdate for one stream
  public:
    SortformerStreamingState(Context &ctx, const SortformerConfig &config = SortformerConfig()) : ctx_(ctx), cfg_(config), geo_(config.geometry()) {
        ctx_.check(fa_sortformer_stream_create(ctx_.handle(), &cfg_.c, 1, &st_), "fa_sortformer_stream_create");
    }
    ~SortformerStreamingState() { fa_sortformer_stream_destroy(st_); }
    SortformerStreamingState(const SortformerStreamingState &) = delete;
    SortformerStreamingState &operator=(const SortformerStreamingState &) = delete;

    // chunk: [rows][d_model] flattened, preds: [rows][speakers] flattened, as the reference takes them
    StreamingUpdateResult streamingUpdate(const std::vector<float> &chunk, const std::vector<float> &preds, int leftContext, int rightContext) {
        const size_t D = static_cast<size_t>(cfg_.c.d_model), S = static_cast<size_t>(cfg_.c.speakers), M = static_cast<size_t>(geo_.out_rows);
        if (chunk.size() % D != 0 || chunk.size() / D > M) throw Error(FA_INVALID_ARGUMENT, "fa_sortformer_stream_update", "a chunk of at most max_chunk_frames rows of d_model");
        std::vector<float> embs(M * D, 0.0f), conf(M * S), tent(M * S);
        std::copy(chunk.begin(), chunk.end(), embs.begin());
        const int32_t embLen = static_cast<int32_t>(chunk.size() / D), predRows = static_cast<int32_t>(preds.size() / S), lc = leftContext, rc = rightContext;
        int32_t counts[2] = {0, 0}, status = 0;
        const float none = 0.0f;
        ctx_.check(fa_sortformer_stream_update(ctx_.handle(), st_, embs.data(), FA_DTYPE_F32, &embLen, preds.empty() ? &none : preds.data(), predRows > 0 ? predRows : 1, &predRows,
                                               &lc, &rc, nullptr, conf.data(), tent.data(), counts, &status, nullptr), "fa_sortformer_stream_update");
        StreamingUpdateResult r;
        r.numSpeakers = cfg_.c.speakers; r.status = status;
        r.confirmed.assign(conf.begin(), conf.begin() + static_cast<ptrdiff_t>(counts[0] * S));
        r.tentative.assign(tent.begin(), tent.begin() + static_cast<ptrdiff_t>(counts[1] * S));
        return r;
    }
    fa_sortformer_stream_info info() {
        fa_sortformer_stream_info i{};
        ctx_.check(fa_sortformer_stream_get(ctx_.handle(), st_, 0, &i, nullptr, nullptr, nullptr, nullptr, nullptr), "fa_sortformer_stream_get");
        return i;
    }
    int spkcacheLength() { return info().spkcache_length; }
    int fifoLength() { return info().fifo_length; }
    int silenceFrameCount() { return info().silence_frame_count; }
    std::vector<float> spkcache() { return rows(0, geo_.spkcache_len, cfg_.c.d_model, info().spkcache_length); }
    std::vector<float> fifo() { return rows(2, cfg_.c.fifo_len, cfg_.c.d_model, info().fifo_length); }
    std::vector<float> meanSilenceEmbedding() { return rows(4, 1, cfg_.c.d_model, 1); }
    void cleanup() { ctx_.check(fa_sortformer_stream_reset(ctx_.handle(), st_, 0), "fa_sortformer_stream_reset"); }

  private:
    std::vector<float> rows(int which, int capacity, int width, int length) {   // the first `length` rows of one of get's arrays
        std::vector<float> all(static_cast<size_t>(capacity) * width);
        float *p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        p[which] = all.data();
        fa_sortformer_stream_info i{};
        ctx_.check(fa_sortformer_stream_get(ctx_.handle(), st_, 0, &i, p[0], p[1], p[2], p[3], p[4]), "fa_sortformer_stream_get");
        all.resize(static_cast<size_t>(length) * width);
        return all;
    }
    Context &ctx_;
    SortformerConfig cfg_;
    fa_sortformer_stream_geometry_info geo_{};
    fa_sortformer_stream *st_ = nullptr;
};

// ---- the Nemotron streaming session around its networks (ASR/Parakeet/Streaming/Nemotron/StreamingNemotronMultilingualAsrManager+Pipeline.swift,
// +Buffers.swift, +BlankRescue.swift; the C entries are batched over streams, this is ONE stream on host arrays).
struct NemotronStreamConfig {       // the knobs of the gate, the mel cache and the blank-span rescue; totalMelFrames is the caller's
    fa_rnnt_stream_config c{};
    explicit NemotronStreamConfig(int totalMelFrames) { fa_rnnt_stream_default_config(&c); c.total_mel_frames = totalMelFrames; }
    fa_rnnt_stream_geometry_info geometry() const {
        fa_rnnt_stream_geometry_info g{};
        if (fa_rnnt_stream_geometry(&c, &g) != FA_SUCCESS) throw Error(FA_INVALID_ARGUMENT, "fa_rnnt_stream_geometry", "the config is refused");
        return g;
    }
};

struct RescueRequest {              // what closeSpanAndMaybeRescue hands to rescueDecode, the audio padded as :243-251
    fa_rnnt_stream_request record{};
    std::vector<float> audio;       // decode_chunks * rescueChunkSamples
};

struct NemotronTokenTiming {        // the fields of TokenTiming this path reads; startTime = frame * 0.08
    int tokenId = 0;
    int frame = 0;
    double startTime() const { return static_cast<double>(frame) * 0.08; }
};

class NemotronStreamSession {       // the gate, the span tracker and mergeRescuedTokens of one stream
  public:
    NemotronStreamSession(Context &ctx, const NemotronStreamConfig &config, std::vector<uint8_t> tokenClasses)
        : ctx_(ctx), cfg_(config), classes_(std::move(tokenClasses)) {
        ctx_.check(fa_rnnt_stream_create(ctx_.handle(), &cfg_.c, 1, &st_), "fa_rnnt_stream_create");
    }
    ~NemotronStreamSession() { fa_rnnt_stream_destroy(st_); }
    NemotronStreamSession(const NemotronStreamSession &) = delete;
    NemotronStreamSession &operator=(const NemotronStreamSession &) = delete;

    static float rms(const std::vector<float> &x, bool gate = false) {
        float r = 0.0f;
        if (fa_rnnt_stream_rms(x.empty() ? nullptr : x.data(), static_cast<int64_t>(x.size()), gate ? 1 : 0, &r) != FA_SUCCESS) throw Error(FA_INVALID_ARGUMENT, "fa_rnnt_stream_rms");
        return r;
    }
    // Pipeline.swift:86-104: true when the chunk skips the encoder
    bool gate(const std::vector<float> &samples, float *rmsOut = nullptr) {
        float r = 0.0f;
        int32_t skip = 0, run = 0, count = 0, status = 0;
        ctx_.check(fa_rnnt_stream_gate(ctx_.handle(), st_, samples.empty() ? nullptr : samples.data(), static_cast<int32_t>(samples.size()), nullptr, &r, &skip, &run, &count, &status),
                   "fa_rnnt_stream_gate");
        if (rmsOut) *rmsOut = r;
        return skip != 0;
    }
    // updateRescueSpans over one chunk against the live timings: the spans that ask for a rescue decode
    std::vector<RescueRequest> track(const std::vector<float> &samples, const std::vector<NemotronTokenTiming> &timings, int rescueChunkSamples) {
        const int32_t windows = static_cast<int32_t>(samples.size()) / cfg_.c.window_samples, capacity = windows / (cfg_.c.close_silent_windows + 1) + 1;
        const fa_rnnt_stream_geometry_info g = cfg_.geometry();
        const int64_t room = static_cast<int64_t>(capacity) * (static_cast<int64_t>(g.span_capacity) + 2 * static_cast<int64_t>(rescueChunkSamples));
        std::vector<int32_t> frames(timings.size() + 1), ids(timings.size() + 1);
        for (size_t i = 0; i < timings.size(); ++i) { frames[i] = timings[i].frame; ids[i] = timings[i].tokenId; }
        const int32_t count = static_cast<int32_t>(timings.size());
        std::vector<fa_rnnt_stream_request> records(static_cast<size_t>(capacity));
        std::vector<float> arena(static_cast<size_t>(room));
        int32_t found = 0, status = 0;
        ctx_.check(fa_rnnt_stream_track(ctx_.handle(), st_, samples.empty() ? nullptr : samples.data(), static_cast<int32_t>(samples.size()), nullptr, frames.data(), ids.data(), &count,
                                        count, classes_.empty() ? nullptr : classes_.data(), static_cast<int32_t>(classes_.size()), rescueChunkSamples, records.data(), capacity,
                                        arena.data(), room, &found, &status), "fa_rnnt_stream_track");
        if (status != FA_RNNT_STREAM_OK || found > capacity) throw Error(FA_RUNTIME_ERROR, "fa_rnnt_stream_track", "a request did not fit");
        std::vector<RescueRequest> out(static_cast<size_t>(found));
        for (int32_t i = 0; i < found; ++i) {
            out[static_cast<size_t>(i)].record = records[static_cast<size_t>(i)];
            const float *p = arena.data() + records[static_cast<size_t>(i)].audio_offset;
            out[static_cast<size_t>(i)].audio.assign(p, p + static_cast<int64_t>(records[static_cast<size_t>(i)].decode_chunks) * rescueChunkSamples);
        }
        return out;
    }
    // rescueDecode's staging and mergeRescuedTokens: true when the rescue was committed.  stagedIds with language tags, one frame per id that is none.
    bool mergeRescued(const RescueRequest &request, const std::vector<int> &stagedIds, const std::vector<int> &stagedFrames, std::vector<int> &liveIds,
                      std::vector<NemotronTokenTiming> &liveTimings) {
        const int32_t scap = static_cast<int32_t>(stagedIds.size()) + 1, lcap = static_cast<int32_t>(liveIds.size() + stagedIds.size()) + 1;
        std::vector<int32_t> sid(static_cast<size_t>(scap)), sfr(static_cast<size_t>(scap)), ids(static_cast<size_t>(lcap)), frames(static_cast<size_t>(lcap)), timed(static_cast<size_t>(lcap));
        std::copy(stagedIds.begin(), stagedIds.end(), sid.begin());
        std::copy(stagedFrames.begin(), stagedFrames.end(), sfr.begin());
        std::copy(liveIds.begin(), liveIds.end(), ids.begin());
        for (size_t i = 0; i < liveTimings.size(); ++i) { frames[i] = liveTimings[i].frame; timed[i] = liveTimings[i].tokenId; }
        int32_t nid = static_cast<int32_t>(stagedIds.size()), nfr = static_cast<int32_t>(stagedFrames.size()), idc = static_cast<int32_t>(liveIds.size()),
                tc = static_cast<int32_t>(liveTimings.size()), status = 0;
        fa_rnnt_stream_request r = request.record;
        r.stream = 0;
        ctx_.check(fa_rnnt_stream_merge_rescued(ctx_.handle(), st_, &r, 1, sid.data(), sfr.data(), &nid, &nfr, scap, ids.data(), frames.data(), timed.data(), &idc, &tc, lcap,
                                                classes_.empty() ? nullptr : classes_.data(), static_cast<int32_t>(classes_.size()), &status), "fa_rnnt_stream_merge_rescued");
        if (status != FA_RNNT_STREAM_OK && status != FA_RNNT_STREAM_NO_LEXICAL) throw Error(FA_INVALID_ARGUMENT, "fa_rnnt_stream_merge_rescued", "the staged tokens are refused");
        liveIds.assign(ids.begin(), ids.begin() + idc);
        liveTimings.resize(static_cast<size_t>(tc));
        for (int32_t i = 0; i < tc; ++i) liveTimings[static_cast<size_t>(i)] = NemotronTokenTiming{timed[static_cast<size_t>(i)], frames[static_cast<size_t>(i)]};
        return status == FA_RNNT_STREAM_OK;
    }
    fa_rnnt_stream_info info() {
        fa_rnnt_stream_info i{};
        ctx_.check(fa_rnnt_stream_get(ctx_.handle(), st_, 0, &i, nullptr, nullptr, nullptr), "fa_rnnt_stream_get");
        return i;
    }
    int detectedBlankSpanCount() { return info().detected_blank_spans; }
    int blankRescueCount() { return info().blank_rescues; }
    void reset() { ctx_.check(fa_rnnt_stream_reset(ctx_.handle(), st_, 0), "fa_rnnt_stream_reset"); }

  private:
    Context &ctx_;
    NemotronStreamConfig cfg_;
    std::vector<uint8_t> classes_;
    fa_rnnt_stream *st_ = nullptr;
};

}  // namespace fluidaudio
