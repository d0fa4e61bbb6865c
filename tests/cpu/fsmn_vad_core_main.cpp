// fsmn_vad_core_main.cpp — fluidaudio_amd/csrc/fsmn_vad_core.h (the word step host and kernel share) and fsmn_vad_launch.h (the
// argument pass, the chunk schedule, the plan) as a stand-alone program for the sanitizers.  Test infrastructure: built by
// tests/test_fsmn_vad_cpu.py with g++ and the address / undefined-behaviour sanitizers, no GPU, nothing loaded into Python.
//
// The word-stepped machine here is the kernel's loop with the ballots spelled as loops over the lanes.  A step may be narrower than 64
// frames (`step`): `prev` is then the 64 frames in front of the step's lane 0, which is what it is on the device too, so sequences of 16
// frames cross step boundaries.
//   exhaustive                   every speech-bit sequence of 0 ... 16 frames, every config with window <= 4, every threshold pair,
//                                max_end_silence, max_segment and look-back in 1 ... 3, against the naive per-frame loop
//                                -> "exhaustive runs mismatches opens end_silence max_length end_of_audio toggles holds"
//   frames S                     -> "frames n"
//   chunks capacity B total[B]   -> "chunks status count | chunk_range | frame_range | records written"
//   seg cfg device have_probs have_segs capacity have_count B range[B + 1]
//                                -> "seg status | frames arena out_slots | B x (frame0 slot0 frames slots)"
//   decide cfg step bits         -> "decide n | n x (start end reason)"; bits a string of 0 / 1, '-' for none
// cfg is 9 words: the threshold as fp32 hex bits, then the eight integers in the struct's order.
#include <atomic>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "../../fluidaudio_amd/csrc/fsmn_vad_launch.h"

namespace fv = fa::fsmnvad;

struct Seg {
    int64_t start, end;
    int32_t reason;
    bool operator==(const Seg &o) const { return start == o.start && end == o.end && reason == o.reason; }
};

struct Tally {
    int64_t opens = 0, closes[3] = {0, 0, 0}, toggles = 0, holds = 0;
};

// decide (FsmnVadManager.swift:159-201), frame by frame
static void naive(const uint8_t *speech, const int64_t T, const fv::Params &o, std::vector<Seg> *out, Tally *tally) {
    int win[fv::kWave] = {0};
    int pos = 0, sum = 0;
    bool pre = false, in_seg = false;
    int64_t seg_start = 0, cont = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int cur = speech[t] ? 1 : 0;
        sum -= win[pos];
        sum += cur;
        win[pos] = cur;
        pos = pos + 1 == o.window ? 0 : pos + 1;                        // (pos + 1) % windowFrames
        tally->toggles += sum >= o.on && sum <= o.off;
        tally->holds += sum < o.on && sum > o.off;
        if (!pre && sum >= o.on) {
            pre = true;
            if (!in_seg) {
                in_seg = true;
                seg_start = t - o.on - o.lookback > 0 ? t - o.on - o.lookback : 0;
                cont = 0;
                ++tally->opens;
            }
        } else if (pre && sum <= o.off) {
            pre = false;
        }
        if (in_seg && !pre) ++cont; else cont = 0;
        if (in_seg && cont >= o.max_end_silence) {
            out->push_back(Seg{seg_start, t - o.max_end_silence + o.lookahead, fv::kEndSilence});
            in_seg = false;
        } else if (in_seg && t - seg_start >= o.max_segment) {
            out->push_back(Seg{seg_start, t, fv::kMaxLength});
            in_seg = false;
            pre = false;
        }
    }
    if (in_seg) out->push_back(Seg{seg_start, T, fv::kEndOfAudio});
    for (const Seg &s : *out) ++tally->closes[s.reason];
}

// the kernel's loop, `step` frames at a time
static void stepped(const uint8_t *speech, const int64_t T, const fv::Params &o, const int step, std::vector<Seg> *out) {
    fv::Machine m = fv::machine_start();
    const auto emit = [&](const int64_t start, const int64_t end, const int32_t reason) { out->push_back(Seg{start, end, reason}); ++m.count; };
    for (int64_t b0 = 0; b0 < T; b0 += step) {
        const int v = T - b0 < step ? static_cast<int>(T - b0) : step;
        uint64_t cur = 0;
        for (int l = 0; l < v; ++l) cur |= static_cast<uint64_t>(speech[b0 + l] ? 1 : 0) << l;
        uint64_t at_on = 0, above_off = 0;
        for (int l = 0; l < v; ++l) {                                   // the lanes beyond v are masked by the walk
            const int w = fv::window_count(m.prev, cur, o.window, l);
            at_on |= static_cast<uint64_t>(w >= o.on) << l;
            above_off |= static_cast<uint64_t>(w > o.off) << l;
        }
        const fv::Classes c = fv::classes(at_on, above_off);
        const auto word = [&](const int from, const bool carry) {
            uint64_t P = 0;
            for (int l = from; l < v; ++l) P |= static_cast<uint64_t>(fv::state_at(c, from, carry, l)) << l;
            return P;
        };
        fv::walk_step(m, o, b0, v, word(0, m.pre_speech), [&](const int from) { return word(from, false); }, emit);
        m.prev = v == fv::kWave ? cur : (m.prev >> v) | (cur << (fv::kWave - v));   // the 64 frames in front of the next step
    }
    if (m.in_seg) emit(m.seg_start, T, fv::kEndOfAudio);
}

// What a sequence's steps hold that window, on and off alone decide: the words of state_at for either carry-in and for every `from`.
// The 27 configs that share the three walk the same tables, so the lanes are evaluated once for all of them.
struct StepTable {
    int v;
    uint64_t carried[2];                     // the word with carry-in false / true in front of lane 0
    uint64_t from[17];                       // the word with carry-in false in front of lane `from`, 0 ... v
};

static int tabulate(const uint8_t *speech, const int T, const int window, const int on, const int off, const int step, StepTable *steps) {
    uint64_t prev = 0;
    int n = 0;
    for (int b0 = 0; b0 < T; b0 += step, ++n) {
        StepTable &s = steps[n];
        s.v = T - b0 < step ? T - b0 : step;
        uint64_t cur = 0, at_on = 0, above_off = 0;
        for (int l = 0; l < s.v; ++l) cur |= static_cast<uint64_t>(speech[b0 + l] ? 1 : 0) << l;
        for (int l = 0; l < s.v; ++l) {
            const int w = fv::window_count(prev, cur, window, l);
            at_on |= static_cast<uint64_t>(w >= on) << l;
            above_off |= static_cast<uint64_t>(w > off) << l;
        }
        const fv::Classes c = fv::classes(at_on, above_off);
        const auto word = [&](const int from, const bool carry) {
            uint64_t P = 0;
            for (int l = from; l < s.v; ++l) P |= static_cast<uint64_t>(fv::state_at(c, from, carry, l)) << l;
            return P;
        };
        s.carried[0] = word(0, false); s.carried[1] = word(0, true);
        for (int from = 0; from <= s.v; ++from) s.from[from] = word(from, false);
        prev = s.v == fv::kWave ? cur : (prev >> s.v) | (cur << (fv::kWave - s.v));
    }
    return n;
}

static void walk_tables(const StepTable *steps, const int n, const int64_t T, const fv::Params &o, std::vector<Seg> *out) {
    fv::Machine m = fv::machine_start();
    const auto emit = [&](const int64_t start, const int64_t end, const int32_t reason) { out->push_back(Seg{start, end, reason}); ++m.count; };
    int64_t b0 = 0;
    for (int k = 0; k < n; ++k) {
        const StepTable &s = steps[k];
        fv::walk_step(m, o, b0, s.v, s.carried[m.pre_speech ? 1 : 0], [&](const int from) { return s.from[from]; }, emit);
        b0 += s.v;
    }
    if (m.in_seg) emit(m.seg_start, T, fv::kEndOfAudio);
}

static int exhaustive() {
    constexpr int kFrames = 16;
    const int widths[8] = {1, 2, 3, 5, 7, 11, 16, 64};
    struct Item { int window, on, off, T; };
    std::vector<Item> items;
    for (int T = kFrames; T >= 0; --T)                                  // the long ones first: they are the most work
        for (int window = 1; window <= 4; ++window)
            for (int on = 0; on <= window; ++on)
                for (int off = 0; off <= window; ++off) items.push_back(Item{window, on, off, T});
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t workers = hw == 0 ? 1 : hw > 16 ? 16 : hw;
    std::atomic<size_t> next{0};
    std::atomic<int64_t> runs{0}, mismatches{0};
    std::vector<Tally> tallies(workers);
    std::vector<std::thread> pool;
    for (size_t w = 0; w < workers; ++w)
        pool.emplace_back([&, w] {
            std::vector<Seg> want, got;
            want.reserve(kFrames + 1); got.reserve(kFrames + 1);
            Tally tally;                                                // the thread's own: no line shared with another
            uint8_t speech[kFrames];
            StepTable steps[kFrames];
            int64_t mine = 0, bad = 0;
            for (size_t i = next++; i < items.size(); i = next++) {
                const Item it = items[i];
                for (uint32_t bits = 0; bits < (uint32_t{1} << it.T); ++bits) {
                    for (int t = 0; t < it.T; ++t) speech[t] = (bits >> t) & 1;
                    const int width = widths[(bits * 2654435761u + static_cast<uint32_t>(i) * 40503u) >> 13 & 7];
                    const int n = tabulate(speech, it.T, it.window, it.on, it.off, width, steps);
                    for (int end_silence = 1; end_silence <= 3; ++end_silence)
                        for (int max_segment = 1; max_segment <= 3; ++max_segment)
                            for (int lookback = 1; lookback <= 3; ++lookback) {
                                const fv::Params o{0.2f, it.window, it.on, it.off, end_silence, lookback, (it.window + lookback) % 3, max_segment, 10};
                                want.clear(); got.clear();
                                naive(speech, it.T, o, &want, &tally);
                                walk_tables(steps, n, it.T, o, &got);
                                ++mine;
                                if (!(want == got) && bad++ == 0)
                                    fprintf(stderr, "mismatch: window %d on %d off %d end_silence %d lookback %d lookahead %d max_segment %d, T %d bits %x width %d\n", o.window,
                                            o.on, o.off, o.max_end_silence, o.lookback, o.lookahead, o.max_segment, it.T, bits, width);
                            }
                }
            }
            tallies[w] = tally;
            runs += mine;
            mismatches += bad;
        });
    for (std::thread &t : pool) t.join();
    Tally sum;
    for (const Tally &t : tallies) {
        sum.opens += t.opens; sum.toggles += t.toggles; sum.holds += t.holds;
        for (int r = 0; r < 3; ++r) sum.closes[r] += t.closes[r];
    }
    printf("exhaustive %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", runs.load(), mismatches.load(), sum.opens, sum.closes[0],
           sum.closes[1], sum.closes[2], sum.toggles, sum.holds);
    return mismatches.load() == 0 ? 0 : 1;
}

static int64_t i64() { int64_t v; if (!(std::cin >> v)) exit(2); return v; }

static fa_fsmn_vad_config config() {
    std::string hex;
    if (!(std::cin >> hex)) exit(2);
    const uint32_t b = static_cast<uint32_t>(strtoul(hex.c_str(), nullptr, 16));
    fa_fsmn_vad_config c;
    memcpy(&c.silence_threshold, &b, 4);
    c.window_frames = static_cast<int32_t>(i64()); c.sil_to_speech_frames = static_cast<int32_t>(i64()); c.speech_to_sil_frames = static_cast<int32_t>(i64());
    c.max_end_silence_frames = static_cast<int32_t>(i64()); c.lookback_frames = static_cast<int32_t>(i64()); c.lookahead_frames = static_cast<int32_t>(i64());
    c.max_segment_frames = static_cast<int32_t>(i64()); c.frame_ms = static_cast<int32_t>(i64());
    return c;
}

// exactly n entries: the sanitizers watch the plan's reads
static std::vector<int64_t> list(const int64_t n) {
    std::vector<int64_t> v(static_cast<size_t>(n > 0 ? n : 0));
    for (int64_t &x : v) x = i64();
    return v;
}

int main() {
    std::string cmd;
    int dummy = 0;
    while (std::cin >> cmd) {
        if (cmd == "exhaustive") {
            if (exhaustive() != 0) return 1;
        } else if (cmd == "frames") {
            printf("frames %" PRId64 "\n", fv::frame_count(i64()));
        } else if (cmd == "chunks") {
            const int64_t capacity = i64();
            const int32_t B = static_cast<int32_t>(i64());
            const std::vector<int64_t> total = list(B);
            std::vector<fa_fsmn_vad_chunk> chunks(static_cast<size_t>(capacity > 0 ? capacity : 0));
            std::vector<int64_t> chunk_range(static_cast<size_t>(B > 0 ? B : 0) + 1, -1), frame_range(chunk_range);
            int64_t count = -1;
            const fa::Verdict v = fv::plan_chunks(total.data(), B, chunks.data(), capacity, &count, chunk_range.data(), frame_range.data());
            printf("chunks %d %" PRId64 " |", static_cast<int>(v.status), count);
            for (const int64_t x : chunk_range) printf(" %" PRId64, x);
            printf(" |");
            for (const int64_t x : frame_range) printf(" %" PRId64, x);
            printf(" |");
            for (int64_t i = 0; i < count && i < capacity; ++i) {
                const fa_fsmn_vad_chunk &c = chunks[static_cast<size_t>(i)];
                printf(" %d %d %" PRId64 " %" PRId64 " %d %d %" PRId64, c.recording, c.bucket, c.start_sample, c.end_sample, c.frames, c.keep_from, c.first_frame);
            }
            printf("\n");
        } else if (cmd == "seg") {
            const fa_fsmn_vad_config c = config();
            const bool device = i64(), have_probs = i64(), have_segs = i64();
            const int64_t capacity = i64();
            const bool have_count = i64();
            const int32_t B = static_cast<int32_t>(i64());
            const std::vector<int64_t> range = list(static_cast<int64_t>(B) + 1);
            fv::Params o{};
            fv::SegPlan p;
            const fa::Verdict v = fv::plan_segments(c, have_probs ? &dummy : nullptr, range.data(), B, have_segs ? &dummy : nullptr, capacity, have_count ? &dummy : nullptr, device, &o, &p);
            printf("seg %d |", static_cast<int>(v.status));
            if (v.status == FA_SUCCESS) {
                printf(" %" PRId64 " %" PRId64 " %" PRId64 " |", p.frames, p.arena, p.out_slots);
                for (const fv::SegRecording &r : p.rec) printf(" %" PRId64 " %" PRId64 " %d %d", r.frame0, r.slot0, r.frames, r.slots);
            }
            printf("\n");
        } else if (cmd == "decide") {
            const fa_fsmn_vad_config c = config();
            const int step = static_cast<int>(i64());
            std::string bits;
            if (!(std::cin >> bits)) return 2;
            fv::Params o{};
            if (fv::derive(c, &o).status != FA_SUCCESS || step < 1 || step > fv::kWave) return 2;
            std::vector<uint8_t> speech;
            if (bits != "-") for (const char ch : bits) speech.push_back(ch == '1');
            std::vector<Seg> got;
            stepped(speech.data(), static_cast<int64_t>(speech.size()), o, step, &got);
            printf("decide %zu |", got.size());
            for (const Seg &s : got) printf(" %" PRId64 " %" PRId64 " %d", s.start, s.end, s.reason);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
