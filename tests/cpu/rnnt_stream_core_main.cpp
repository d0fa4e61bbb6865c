// A stand-alone program over fluidaudio_amd/csrc/rnnt_stream_core.h, built with -fsanitize=address,undefined by tests/test_rnnt_stream_cpu.py.
//   exhaustive          the window machine (slab offsets, the pre-roll ring, the closures) against a naive machine that keeps its audio in
//                       vectors as the reference does, on every loud / silent sequence of up to 16 windows under a grid of configs and
//                       chunk cuts; the two insert indices of mergeRescuedTokens as word steps against naive loops on every tag mask
//   rms <waves> <hex..> the RMS of the fp32 bit patterns in the kernels' order
//   gate <thr> <hang> <W> <n> <bits>   the gate's counters over a sequence of silent (1) / loud (0) chunks of n samples
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fluidaudio_amd/csrc/rnnt_stream_core.h"

using namespace fa::rns;

namespace {

constexpr int kMost = 48;   // windows a span or a slab can hold here: 16 windows and a pre-roll, or the largest room + 1
struct Naive {   // BlankRescue.swift:70-136 with arrays; a window's audio is its absolute frame number
    bool open = false, overflowed = false;
    int start = 0, last = 0, speech = 0, pre_frames = 0, run = 0;
    int audio[kMost], na = 0, tail[kMost], nt = 0;
};

struct Closed { int start, last, speech, pre_frames, overflowed, na; int audio[kMost]; };

bool naive_step(const Config &c, Naive &s, const bool silent, const int frame, Closed *out) {
    const int W = c.window_samples;
    if (s.open) {
        if (silent) s.run += 1; else { s.run = 0; s.last = frame; s.speech += 1; }
    } else if (!silent) {
        s.open = true; s.start = frame; s.last = frame; s.speech = 1; s.run = 0;
        std::memcpy(s.audio, s.tail, sizeof(int) * static_cast<size_t>(s.nt)); s.na = s.nt; s.pre_frames = s.nt; s.overflowed = false;
    }
    if (s.open && !s.overflowed) {
        if (s.na >= kMost) std::abort();
        s.audio[s.na++] = frame;
        if (static_cast<long long>(s.na) * W > c.max_span_samples) { s.overflowed = true; s.na = 0; }
    } else if (!s.open) {
        s.tail[s.nt++] = frame;
        if (s.nt > c.pre_roll_windows) { const int drop = s.nt - c.pre_roll_windows; std::memmove(s.tail, s.tail + drop, sizeof(int) * static_cast<size_t>(c.pre_roll_windows)); s.nt = c.pre_roll_windows; }
    }
    if (s.open && s.run >= c.close_silent_windows) {
        *out = Closed{s.start, s.last, s.speech, s.pre_frames, s.overflowed, s.na, {}};
        std::memcpy(out->audio, s.audio, sizeof(int) * static_cast<size_t>(s.na));
        s.open = false; s.na = 0; s.speech = 0; s.run = 0; s.overflowed = false; s.nt = 0;
        return true;
    }
    return false;
}

// the core's machine with the copies a kernel would do
struct Device {
    Span s{};
    int slab[kMost], ring[8];
    int slab_windows = 0, ring_windows = 0;
    int &slab_at(const int i) { if (i < 0 || i >= slab_windows) std::abort(); return slab[i]; }
    int &ring_at(const int i) { if (i < 0 || i >= ring_windows) std::abort(); return ring[i]; }
};

long long run_machines(const Config &c, const unsigned bits, const int n, long long *closures, long long *overflows, long long *reopen) {
    Naive naive;
    Device dev;
    dev.slab_windows = span_capacity(c) / c.window_samples;
    dev.ring_windows = c.pre_roll_windows > 0 ? c.pre_roll_windows : 1;
    if (dev.slab_windows > kMost) std::abort();
    long long bad = 0;
    bool closed_before = false;
    for (int f = 0; f < n; ++f) {
        const bool silent = !((bits >> f) & 1u);
        Closed want{};
        const bool closed = naive_step(c, naive, silent, f, &want);
        const Step r = window_step(c, dev.s, silent, f);
        for (int i = 0; i < r.ring_windows; ++i) dev.slab_at(i) = dev.ring_at((r.ring_head + i) % c.pre_roll_windows);
        if (r.dest == kToSpan) dev.slab_at(r.offset / c.window_samples) = f;
        else if (r.dest == kToRing) dev.ring_at(r.offset) = f;
        if (closed != (r.closed != 0)) { ++bad; continue; }
        if (closed) {
            ++*closures;
            *overflows += want.overflowed;
            const Closure &k = r.closure;
            bad += k.start != want.start || k.last != want.last || k.speech != want.speech || k.pre_frames != want.pre_frames || (k.overflowed != 0) != (want.overflowed != 0) ||
                   k.len != want.na * c.window_samples;
            for (int i = 0; i < want.na; ++i) bad += dev.slab_at(i) != want.audio[i];
        }
        if (!silent && closed_before && dev.s.open && dev.s.pre_frames == 0) ++*reopen;
        closed_before = closed;
        // the state every window leaves
        bad += (dev.s.open != 0) != naive.open || dev.s.run != naive.run || dev.s.speech != naive.speech || (dev.s.overflowed != 0) != naive.overflowed ||
               dev.s.len != naive.na * c.window_samples || dev.s.pre_count != naive.nt;
        for (int i = 0; i < naive.nt; ++i) bad += dev.ring_at((dev.s.pre_head + i) % c.pre_roll_windows) != naive.tail[i];
        for (int i = 0; i < naive.na; ++i) bad += dev.slab_at(i) != naive.audio[i];
    }
    return bad;
}

int exhaustive() {
    long long runs = 0, bad = 0, closures = 0, overflows = 0, reopen = 0;
    for (int close = 1; close <= 3; ++close)
        for (int pre = 0; pre <= 3; ++pre)
            for (int cap : {1, 3, 8, 40}) {
                Config c{};
                c.window_samples = 4; c.close_silent_windows = close; c.pre_roll_windows = pre; c.min_speech_windows = 2; c.max_span_samples = cap * 4 + (cap == 3 ? 2 : 0);
                for (int n = 0; n <= 16; ++n)
                    for (unsigned bits = 0; bits < (1u << n); ++bits) { ++runs; bad += run_machines(c, bits, n, &closures, &overflows, &reopen); }
            }
    // the insert indices: every plain / tag mask of up to 16 ids across a word boundary (ids 56 ... 71), every need
    long long index_runs = 0, index_bad = 0;
    for (int n = 0; n <= 16; ++n)
        for (unsigned mask = 0; mask < (1u << n); ++mask)
            for (int t_at = 0; t_at <= n; ++t_at) {
                ++index_runs;
                const int lead = 56, total = lead + n;                 // 56 plain ids in front, then the mask
                int want = total, seen = 0;                            // BlankRescue.swift:337-347
                for (int i = 0; i < total; ++i) {
                    const bool plain = i < lead || ((mask >> (i - lead)) & 1u);
                    if (seen == t_at + lead && plain) { want = i; break; }
                    if (plain) ++seen;
                }
                int got = total, need = t_at + lead;
                for (int base = 0; base < total; base += 64) {
                    uint64_t word = 0;
                    for (int j = 0; j < 64 && base + j < total; ++j)
                        if (base + j < lead || ((mask >> (base + j - lead)) & 1u)) word |= uint64_t{1} << j;
                    const int p = ids_word(word, base, need);
                    if (p >= 0) { got = p; break; }
                }
                index_bad += got != want;
                // the timing index: the first set bit of `above`
                uint64_t above = static_cast<uint64_t>(mask) << 3;
                const int tw = timing_word(above, 64);
                int tn = -1;
                for (int j = 0; j < 64; ++j) if ((above >> j) & 1u) { tn = 64 + j; break; }
                index_bad += tw != tn;
            }
    std::printf("exhaustive %lld %lld %lld %lld %lld %lld %lld\n", runs, bad, closures, overflows, reopen, index_runs, index_bad);
    return 0;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "exhaustive") {
            exhaustive();
        } else if (cmd == "rms") {
            int waves = 1;
            in >> waves;
            std::vector<float> x;
            std::string h;
            while (in >> h) { const uint32_t u = static_cast<uint32_t>(std::strtoul(h.c_str(), nullptr, 16)); float f; std::memcpy(&f, &u, 4); x.push_back(f); }
            const float r = rms(x.data(), static_cast<int64_t>(x.size()), waves);
            uint32_t u;
            std::memcpy(&u, &r, 4);
            std::printf("rms %08x\n", u);
        } else if (cmd == "gate") {
            Config c{};
            std::string seq;
            int n = 0;
            in >> c.vad_rms_threshold >> c.vad_hangover_chunks >> c.window_samples >> n >> seq;
            int32_t low = 0, skips = 0, base = 0;
            std::printf("gate");
            for (const char ch : seq) std::printf(" %d", gate_step(c, ch == '1', n, low, skips, base));
            std::printf(" | %d %d %d\n", low, skips, base);
        } else if (!cmd.empty()) {
            std::printf("unknown %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
