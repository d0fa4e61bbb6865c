// The single-thread host baseline of scripts/tdt_plan_timing.py: the reference's loops as ChunkProcessor writes them
// (speechEndSamples, silenceAlignedChunkStarts with bestBoundaryCandidate / shouldUseWarmupPrefix / wouldCompressSpeechTail and a fresh
// boundaryEnergyScore per candidate, the window loop, padAudioIfNeeded) over one recording, in C++ with -ffp-contract=off.  A CPU
// restatement, not the Swift reference; the window loop's integers are csrc/tdt_plan_core.h.  Written for the timing script only.
//   tdt_plan_baseline <file of float32 samples> <mel_chunk_context> <silence_aligned> <warmup_prefix_frames> <pack>
//   prints   milliseconds of the plan, milliseconds of the pack, windows, sum of chunk_start, sum of length, speech_end
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../fluidaudio_amd/csrc/tdt_plan_launch.h"

namespace tp = fa::tdt_plan;

static const float *x;
static int64_t total;

static float sum_squares(int64_t start, int64_t count) {
    float sum = 0;
    for (int64_t i = 0; i < count; ++i) sum += x[start + i] * x[start + i];
    return sum;
}

static float boundary_energy_score(int64_t center, int64_t half) {
    const int64_t start = std::max<int64_t>(0, center - half), end = std::min(total, center + half), count = end - start;
    return count > 0 ? sum_squares(start, count) / static_cast<float>(count) : 0.0f;
}

struct Candidate { int64_t start; float score, median; };

static Candidate best_boundary(const tp::Geometry &g, int64_t target_frame, int64_t radius, int64_t previous_start, int64_t latest) {
    const int64_t F = g.frame, lower = std::max<int64_t>(1, target_frame - radius), upper = std::min((total - 1) / F, target_frame + radius);
    const int64_t target_start = std::min(std::max(target_frame * F, previous_start + F), latest);
    Candidate c{target_start, 3.402823466e+38f, 0.0f};
    std::vector<float> scores;
    for (int64_t frame = lower; frame <= upper; ++frame) {
        const int64_t candidate = frame * F;
        if (candidate <= previous_start || candidate > latest) continue;
        const float score = boundary_energy_score(candidate, F);
        scores.push_back(score);
        if (score < c.score) { c.score = score; c.start = candidate; }
    }
    if (scores.empty()) return c;
    std::sort(scores.begin(), scores.end());
    c.median = scores[scores.size() / 2];
    return c;
}

static bool should_use_warmup(const tp::Geometry &g, int64_t center) {
    int64_t offset = 0, quiet = 0;
    while (offset < g.lookahead) {
        const int64_t start = center + offset;
        if (!(start < total)) break;
        const int64_t count = std::min(std::min(g.probe_window, total - start), g.lookahead - offset);
        if (!(count > 0)) break;
        if (!(std::sqrt(sum_squares(start, count) / static_cast<float>(count)) < 0.003f)) break;
        quiet += count;
        if (quiet >= g.stable_quiet) return false;
        offset += count;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    total = std::ftell(f) / 4;
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> samples(static_cast<size_t>(total));
    if (std::fread(samples.data(), 4, samples.size(), f) != samples.size()) return 2;
    std::fclose(f);
    x = samples.data();
    fa_tdt_window_config cfg = tp::config_or_default(nullptr);
    cfg.mel_chunk_context = std::atoi(argv[2]); cfg.silence_aligned = std::atoi(argv[3]); cfg.warmup_prefix_frames = std::atoi(argv[4]);
    tp::Geometry g{};
    if (tp::derive(cfg, &g).status != FA_SUCCESS) return 2;
    const int64_t F = g.frame;

    const auto t0 = std::chrono::steady_clock::now();
    int64_t speech_end = total;                                                  // speechEndSamples
    for (int64_t end = total; end > 0;) {
        const int64_t frame_start = std::max<int64_t>(0, end - F);
        if (std::sqrt(sum_squares(frame_start, end - frame_start) / static_cast<float>(end - frame_start)) >= 0.0005f) { speech_end = end; break; }
        end = frame_start;
    }
    std::vector<std::pair<int64_t, bool>> starts{{0, false}};
    if (g.aligned) {                                                             // silenceAlignedChunkStarts
        int64_t previous_start = 0;
        for (int64_t target = g.stride; target < total; target += g.stride) {
            const int64_t target_frame = target / F, latest = previous_start + g.chunk - 6 * F;
            const int64_t target_start = std::min(std::max(target_frame * F, previous_start + F), latest);
            const Candidate s = best_boundary(g, target_frame, g.silence_radius, previous_start, latest);
            int64_t best_start;
            bool use_warmup = false;
            if (s.score <= (s.median > 0 ? s.median * 0.05f : 0.0f)) {
                const bool should = g.can_warmup ? should_use_warmup(g, s.start) : false;
                bool compresses = false;
                if (should && s.start < target_start && s.median > 0) {
                    const int64_t forced = s.start + g.chunk - 6 * F;
                    if (forced < total) compresses = boundary_energy_score(target_start, F) > s.median * 0.8f && boundary_energy_score(forced, F) > s.median * 0.8f;
                }
                if (compresses) best_start = target_start; else { best_start = s.start; use_warmup = should; }
            } else {
                const Candidate v = best_boundary(g, target_frame, g.valley_radius, previous_start, latest);
                best_start = v.score <= (v.median > 0 ? v.median * 0.35f : 0.0f) ? v.start : target_start;
            }
            if (best_start <= previous_start) best_start = std::min(previous_start + g.stride, total);
            starts.push_back({best_start, use_warmup});
            previous_start = best_start;
        }
    } else {
        for (int64_t start = g.stride; start < total; start += g.stride) starts.push_back({start, false});
    }
    std::vector<fa_tdt_window> windows;
    int64_t chunk_start = 0;
    bool use_warmup = false;
    for (int64_t index = 0;; ++index) {                                          // the window loop of process
        const tp::Turn t = tp::turn(g, 0, total, g.end_aligned ? speech_end : total, chunk_start, use_warmup, index);
        if (t.record) windows.push_back(t.w);
        if (t.ends) break;
        if (index + 1 < static_cast<int64_t>(starts.size())) { chunk_start = starts[index + 1].first; use_warmup = starts[index + 1].second; }
        else { chunk_start += g.stride; use_warmup = false; }
    }
    const auto t1 = std::chrono::steady_clock::now();
    int64_t sum_start = 0, sum_length = 0;
    for (const fa_tdt_window &w : windows) { sum_start += w.chunk_start; sum_length += w.length; }
    double pack_ms = 0;
    if (std::atoi(argv[5])) {                                                    // padAudioIfNeeded of every window
        std::vector<float> rows(windows.size() * static_cast<size_t>(g.max_model));
        const auto p0 = std::chrono::steady_clock::now();
        for (size_t i = 0; i < windows.size(); ++i) {
            float *row = rows.data() + i * static_cast<size_t>(g.max_model);
            std::memcpy(row, x + windows[i].context_start, sizeof(float) * static_cast<size_t>(windows[i].length));
            std::memset(row + windows[i].length, 0, sizeof(float) * static_cast<size_t>(g.max_model - windows[i].length));
        }
        pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
        if (rows.empty() || rows[0] != rows[0]) sum_length += 0;                 // keep the rows alive
    }
    std::printf("%.3f %.3f %zu %lld %lld %lld\n", std::chrono::duration<double, std::milli>(t1 - t0).count(), pack_ms, windows.size(), (long long)sum_start, (long long)sum_length,
                (long long)speech_end);
    return 0;
}
