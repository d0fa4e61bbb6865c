// rnnt_bias_core_main.cpp — fluidaudio_amd/csrc/rnnt_bias_core.h (the text host and kernel share) as a stand-alone program for the
// address and undefined-behaviour sanitizers: it builds bias tables into heap buffers of exactly their size, walks them — through
// candidates() and through a ring of suffix starts, the way the kernel's lanes do —, and then walks truncated and bit-flipped copies,
// which must be refused or walked without one read outside the buffer.  Prints the candidates of a few match states for
// tests/test_rnnt_bias_core_asan.py to compare with the restatement, and a count of the malformed walks.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../fluidaudio_amd/csrc/rnnt_bias_core.h"

namespace rb = fa::rnnt_bias;

namespace {

const char *kPieces[] = {"\xe2\x96\x81", "\xe2\x96\x81to", "r", "vane", "\xe2\x96\x81tor", "\xe2\x96\x81torvane", "\xe2\x96\x81the", "\xe2\x96\x81the", "\xe2\x96\x81ran",
                         "\xe2\x96\x81t", "\xe2\x96\x81""cr", "an", nullptr, "\xe4\xb8\x9c", "\xe4\xba\xac", "<unk>", "\xe2\x96\x81""ab", "\xe2\x96\x81""c", "v", "qqqqqqqqqqqq"};
constexpr int kVocab = sizeof(kPieces) / sizeof(kPieces[0]);
const char *kSurfaces[] = {"torvane", "ab ab c", "\xe4\xb8\x9c\xe4\xba\xac", "the", "torment"};
const float kBoosts[] = {2.0f, 4.5f, 4.5f, 5.5f, 5.0f};
constexpr int kSurfaceCount = 5;

// an exact-size heap copy of the first `words` words: a read at blob[words] is a heap overflow the sanitizer reports
std::unique_ptr<int32_t[]> exact(const std::vector<int32_t> &blob, const size_t words) {
    std::unique_ptr<int32_t[]> p(new int32_t[words ? words : 1]);
    if (words) std::memcpy(p.get(), blob.data(), words * sizeof(int32_t));
    return p;
}

// the kernel's matcher on the host: a ring of tail_cap suffix starts, every appended scalar advances the live ones by one child look-up
struct Ring {
    const int32_t *blob;
    rb::Header h;
    std::vector<int32_t> node;
    int head = 0, len = 0;
    bool append(const uint32_t scalar) {
        const int cap = h.tail_cap;
        int slot;
        if (len == cap) { slot = head; head = head + 1 == cap ? 0 : head + 1; }
        else { slot = (head + len) % cap; ++len; }
        for (int i = 0; i < cap; ++i) {
            int n = i == slot ? 0 : node[i];
            if (n >= 0) { int32_t child; if (!rb::node_child(blob, h, n, scalar, child)) return false; n = child; }
            node[i] = n;
        }
        return true;
    }
    bool observe(const int32_t id) {
        int32_t first, count;
        if (!rb::piece_span(blob, h, id, first, count)) return false;
        for (int32_t i = 0; i < count; ++i)
            if (!append(rb::piece_scalar(blob, h, first + i))) return false;
        return true;
    }
    // the strongest boost per id over the root's list and the live nodes' lists
    bool candidates(std::map<int32_t, float> &best) const {
        auto add = [&](const int32_t n) {
            int32_t first, count;
            if (!rb::node_candidates(blob, h, n, first, count)) return false;
            for (int32_t i = 0; i < count; ++i) {
                int32_t id;
                float boost;
                rb::candidate(blob, h, first + i, id, boost);
                if (!best.count(id) || boost > best[id]) best[id] = boost;
            }
            return true;
        };
        if (!add(0)) return false;
        for (const int32_t n : node)
            if (n >= 0 && !add(n)) return false;
        return true;
    }
};

// both walks of blob[words] after `observed`; -1: refused, otherwise the number of candidates (the two walks must agree)
int walk(const int32_t *blob, const int64_t words, const std::vector<int32_t> &observed, const bool print) {
    std::vector<int32_t> ids(kVocab + 8);
    std::vector<float> boosts(kVocab + 8);
    int32_t count = -1;
    const int st = rb::candidates(blob, words, observed.data(), static_cast<int32_t>(observed.size()), ids.data(), boosts.data(), static_cast<int32_t>(ids.size()), &count);
    Ring r;
    r.blob = blob;
    bool ok = rb::read_header(blob, words, -1, -1, r.h) == rb::kHeaderOk;
    std::map<int32_t, float> best;
    if (ok) {
        r.node.assign(static_cast<size_t>(r.h.tail_cap), -1);
        for (const int32_t id : observed) ok = ok && r.observe(id);
        ok = ok && r.candidates(best);
    }
    if (st == rb::kBuildInvalid) return ok ? -2 : -1;         // (-2: the walks disagree)
    if (st == rb::kBuildTooSmall) return ok ? count : -2;     // a bit-flipped blob may list more ids than the vocabulary has
    if (!ok || static_cast<size_t>(count) != best.size()) return -2;
    int k = 0;
    for (const auto &kv : best) { if (ids[k] != kv.first || std::memcmp(&boosts[k], &kv.second, sizeof(float)) != 0) return -2; ++k; }   // (bit patterns: a flipped boost may be NaN)
    if (print) {
        std::printf("CAND");
        for (const int32_t id : observed) std::printf(" %d", id);
        std::printf(" :");
        for (int i = 0; i < count; ++i) std::printf(" %d=%g", ids[i], static_cast<double>(boosts[i]));
        std::printf("\n");
    }
    return count;
}

}  // namespace

int main() {
    int64_t need = 0;
    int32_t cap = 0;
    if (rb::build(kPieces, kVocab, kSurfaces, kBoosts, kSurfaceCount, nullptr, 0, &need, &cap) != rb::kBuildOk || need <= rb::kHeaderWords) return 1;
    std::vector<int32_t> blob(static_cast<size_t>(need));
    if (rb::build(kPieces, kVocab, kSurfaces, kBoosts, kSurfaceCount, blob.data(), need - 1, &need, &cap) != rb::kBuildTooSmall) return 2;
    if (rb::build(kPieces, kVocab, kSurfaces, kBoosts, kSurfaceCount, blob.data(), need, &need, &cap) != rb::kBuildOk) return 3;
    std::printf("BUILT %lld %d\n", static_cast<long long>(need), cap);
    const std::vector<std::vector<int32_t>> states = {{}, {4}, {4, 15, 12, 99, -3}, {4, 6}, {16, 16}, {16, 16, 16}, {13}, {19, 19, 4, 18}, {1, 2}, {16, 16, 17, 4, 3}};
    {
        const auto p = exact(blob, blob.size());
        for (const auto &s : states)
            if (walk(p.get(), need, s, true) < 0) return 4;
    }
    long refused = 0, walked = 0;
    auto tally = [&](const int r) { if (r == -2) return false; ++(r == -1 ? refused : walked); return true; };
    for (size_t words = 0; words < blob.size(); ++words) {               // truncated
        const auto p = exact(blob, words);
        if (walk(p.get(), static_cast<int64_t>(words), states[words % states.size()], false) != -1) return 5;
        ++refused;
    }
    for (size_t w = 0; w < blob.size(); ++w) {                             // one bit flipped: every bit of the header and of the node table, four per other word
        const bool dense = w < static_cast<size_t>(rb::kHeaderWords) + 4u * static_cast<size_t>(blob[4]);
        for (int bit = 0; bit < 32; bit += dense ? 1 : 9) {
            const auto p = exact(blob, blob.size());
            p[w] ^= static_cast<int32_t>(1u << bit);
            for (size_t s = 0; s < states.size(); s += dense ? 1 : 3)
                if (!tally(walk(p.get(), need, states[s], false))) return 6;
        }
    }
    uint32_t lcg = 12345;                                                 // eight words overwritten at once
    for (int round = 0; round < 4000; ++round) {
        const auto p = exact(blob, blob.size());
        for (int k = 0; k < 8; ++k) {
            lcg = lcg * 1664525u + 1013904223u;
            const size_t w = (lcg >> 8) % blob.size();
            lcg = lcg * 1664525u + 1013904223u;
            p[w] = (k & 1) ? static_cast<int32_t>(lcg) : static_cast<int32_t>(lcg >> 24);
        }
        if (!tally(walk(p.get(), need, states[round % states.size()], false))) return 7;
    }
    std::printf("MALFORMED refused %ld walked %ld\n", refused, walked);
    return 0;
}
