// Single-core C++ baseline of the two Paraformer host loops for scripts/paraformer_probe.py: integrate-and-fire with the decoder's ac
// (ParaformerCif.swift:19-50, ParaformerManager.swift:428-431) and the raw spans of decodeWithTimestamps (ParaformerManager.swift:134-226,
// 262-358), written as the reference writes them — a row at a time, arrays grown as it grows them, a sort for each percentile.
// Build: g++ -O2 -ffp-contract=off -std=c++17.  Input: one binary file (layout in main).  Output: "cif_ms stamps_ms" and the checksums
// the probe compares with the device's: sum of the ac bit patterns, sum of the fire frames, sum of the token counts, sum of the fire
// counts, number of spans, sums of the start and end bit patterns (all modulo 2^64).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using Clock = std::chrono::steady_clock;

static std::vector<int> fire_indices(const std::vector<float> &a, float threshold) {
    float integrate = 0;
    std::vector<int> fires;
    for (size_t t = 0; t < a.size(); ++t) {
        integrate += a[t];
        if (integrate >= threshold) {
            fires.push_back(static_cast<int>(t));
            integrate -= 1.0f;
        }
    }
    return fires;
}

static float percentile(std::vector<float> v, float q) {
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    const long n = static_cast<long>(v.size());
    return v[static_cast<size_t>(std::max(0l, std::min(n - 1, static_cast<long>(static_cast<float>(n - 1) * q))))];
}

struct Span { int token; double start, end; };

static std::vector<Span> raw_spans(const int32_t *ids, int n_ids, const uint8_t *keep, int vocab, const float *alphas, int T, const float *audio, long n_audio) {
    const double time_rate = 10.0 * 6.0 / 1000.0 / 3.0, hop_sec = 0.01;
    const float threshold = 1.0f - 1e-4f;
    std::vector<int> kept;
    for (int i = 0; i < n_ids; ++i)
        if (ids[i] >= 0 && ids[i] < vocab && keep[ids[i]]) kept.push_back(i);
    if (kept.empty()) return {};
    std::vector<float> us;
    for (int t = 0; t < T; ++t)
        for (int k = 0; k < 3; ++k) us.push_back(alphas[t]);
    us.push_back(0.45f);
    std::vector<int> fires = fire_indices(us, threshold);
    if (fires.size() != kept.size() + 1) {
        float sum = 0;
        for (const float a : us) sum += a;
        const float scale = static_cast<float>(kept.size() + 1) / (1e-6f >= sum ? 1e-6f : sum);
        for (float &a : us) a *= scale;
        fires = fire_indices(us, threshold);
    }
    if (fires.size() < 2) return {};
    const double audio_end = static_cast<double>(n_audio) / 16000.0;
    std::vector<float> raw_env;
    if (n_audio > 160)
        for (long i = 0; i + 160 <= n_audio; i += 160) {
            float sum = 0;
            for (int j = 0; j < 160; ++j) sum += audio[i + j] * audio[i + j];
            raw_env.push_back(std::sqrt(sum / 160.0f));
        }
    std::vector<float> env = raw_env;
    const long ne = static_cast<long>(env.size());
    if (ne > 3)
        for (long i = 0; i < ne; ++i) {
            const long lo = std::max(0l, i - 1), hi = std::min(ne - 1, i + 1);
            float sum = 0;
            for (long k = lo; k <= hi; ++k) sum += raw_env[k];
            env[i] = sum / static_cast<float>(hi - lo + 1);
        }
    const float floor = env.empty() ? 0.0f : percentile(env, 0.1f), scaled = floor * 2.5f, energy = 1e-4f >= scaled ? 1e-4f : scaled;
    const int n = static_cast<int>(std::min(kept.size(), fires.size() - 1));
    std::vector<float> spacings;
    for (int i = 1; i < n; ++i) spacings.push_back(static_cast<float>(fires[i] * time_rate - fires[i - 1] * time_rate));
    const double typical = spacings.empty() ? static_cast<double>(0.3f) : static_cast<double>(percentile(spacings, 0.5f));
    std::vector<Span> out;
    double cursor = 0;
    for (int i = 0; i < n; ++i) {
        const double c = fires[i] * time_rate;
        const double dur = i < n - 1 ? fires[i + 1] * time_rate - c : std::min(audio_end - c, std::max(typical * 2, 0.4));
        const double to = std::min(audio_end, c + dur * 1.5 + 0.15);
        bool found = false;
        long best_lo = 0, best_hi = 0, best_d = 0;
        if (ne > 0 && to > cursor) {
            const long i0 = std::max(0l, static_cast<long>(cursor / hop_sec)), i1 = std::min(ne - 1, std::max(i0, static_cast<long>(to / hop_sec)));
            const long ci = static_cast<long>(c / hop_sec);
            for (long j = i0; j <= i1;) {
                if (env[j] > energy) {
                    long k = j;
                    while (k <= i1 && env[k] > energy) ++k;
                    if (k - j >= 3) {
                        const long d = std::labs(j + k - 1 - 2 * ci);
                        if (!found || d < best_d) { found = true; best_d = d; best_lo = j; best_hi = k - 1; }
                    }
                    j = k;
                } else {
                    ++j;
                }
            }
        }
        const double s = found ? best_lo * hop_sec : cursor, e = found ? best_hi * hop_sec : std::min(audio_end, cursor + std::max(dur, 0.1));
        cursor = e;
        out.push_back(Span{kept[i], s, e});
    }
    return out;
}

template <class T> static std::vector<T> read(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(1); }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    // int64 B, T, D, max_tokens, vocab; float enc[B][T][D], alphas[B][T]; int32 valid[B], token_ids[B][max_tokens], token_counts[B];
    // uint8 keep[vocab]; int64 audio_off[B + 1]; float audio[audio_off[B]]
    const std::vector<int64_t> h = read<int64_t>(f, 5);
    const size_t B = h[0], T = h[1], D = h[2], M = h[3], V = h[4];
    const std::vector<float> enc = read<float>(f, B * T * D), alphas = read<float>(f, B * T);
    const std::vector<int32_t> valid = read<int32_t>(f, B), ids = read<int32_t>(f, B * M), counts = read<int32_t>(f, B);
    const std::vector<uint8_t> keep = read<uint8_t>(f, V);
    const std::vector<int64_t> off = read<int64_t>(f, B + 1);
    const std::vector<float> audio = read<float>(f, static_cast<size_t>(off[B]));
    std::fclose(f);

    uint64_t ac_sum = 0, fires_sum = 0, tokens_sum = 0, count_sum = 0;
    std::vector<float> ac(B * M * D, 0.0f);
    const auto t0 = Clock::now();
    for (size_t b = 0; b < B; ++b) {
        const size_t Tb = static_cast<size_t>(valid[b]);
        std::vector<std::vector<float>> embeds;
        std::vector<float> frame(D, 0.0f), zero(D, 0.0f);
        float integrate = 0;
        for (size_t t = 0; t <= Tb; ++t) {
            const float alpha = t < Tb ? alphas[b * T + t] : 0.45f;
            const float *hidden = t < Tb ? &enc[(b * T + t) * D] : zero.data();
            integrate += alpha;
            if (integrate < 1.0f) {
                for (size_t d = 0; d < D; ++d) frame[d] += alpha * hidden[d];
            } else {
                const float used = alpha - (integrate - 1.0f);
                for (size_t d = 0; d < D; ++d) frame[d] += used * hidden[d];
                embeds.push_back(frame);
                fires_sum += t;
                integrate -= 1.0f;
                const float leftover = alpha - used;
                for (size_t d = 0; d < D; ++d) frame[d] = hidden[d] * leftover;
            }
        }
        const size_t L = std::min(embeds.size(), M);
        for (size_t l = 0; l < L; ++l) std::memcpy(&ac[(b * M + l) * D], embeds[l].data(), D * sizeof(float));
        tokens_sum += L;
        count_sum += embeds.size();
    }
    const auto t1 = Clock::now();
    for (const float v : ac) { uint32_t u; std::memcpy(&u, &v, 4); ac_sum += u; }

    uint64_t spans = 0, start_sum = 0, end_sum = 0;
    const auto t2 = Clock::now();
    for (size_t b = 0; b < B; ++b)
        for (const Span &s : raw_spans(&ids[b * M], counts[b], keep.data(), static_cast<int>(V), &alphas[b * T], valid[b], audio.data() + off[b], off[b + 1] - off[b])) {
            uint64_t u;
            std::memcpy(&u, &s.start, 8); start_sum += u;
            std::memcpy(&u, &s.end, 8); end_sum += u;
            ++spans;
        }
    const auto t3 = Clock::now();
    const auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::printf("%.3f %.3f %llu %llu %llu %llu %llu %llu %llu\n", ms(t0, t1), ms(t2, t3), (unsigned long long)ac_sum, (unsigned long long)fires_sum,
                (unsigned long long)tokens_sum, (unsigned long long)count_sum, (unsigned long long)spans, (unsigned long long)start_sum, (unsigned long long)end_sum);
    return 0;
}
