// rnnt_bias_core.h — the hotword-bias tables of the streaming RNN-T walk (kernels: rnnt.hip, host entries: rnnt_host.hip, operands:
// rnnt_launch.h): the blob's layout, the bounds-checked accessors host and kernel both walk it through, and — host only — the builder.
// Plain C++ (tests/cpu/rnnt_bias_core_main.cpp builds and walks tables under a sanitizer); the accessors are __host__ __device__ under hipcc.
//
// Restated from FluidAudio/ASR/Parakeet/Streaming/Nemotron/NemotronVocabularyBias.swift: init :126-182 (special pieces :147-156, the trie
// :160-175), effectiveBoost :196-199, isCJK :219-228, pieceForm :233-250, observe :254-261, candidates :280-306, accumulate :310-339.
// Case folding, NFC and the letter-count guard of usableSurfaces (:203-212) are the caller's.
//
// THE BLOB: int32 words, position independent (every reference is an index into one of its sections).
//   [0] magic  [1] version  [2] vocab  [3] tail_cap  [4] n_nodes  [5] off_nodes  [6] n_edges  [7] off_edge_keys  [8] off_edge_children
//   [9] n_cands  [10] off_cands  [11] off_piece_index  [12] n_piece_scalars  [13] off_piece_scalars  [14] total words  [15] 0
//   nodes        [n_nodes][4]   first edge, edge count, first candidate, candidate count; node 0 is the root (its list: freshStartCandidates)
//   edge keys    [n_edges]      the scalars of a node's children, ascending within the node: the child is found by a binary search
//   edge children[n_edges]      node index per edge
//   candidates   [n_cands][2]   token id, boost as its bit pattern; within a node one entry per id (the strongest boost), ascending id
//   piece index  [vocab + 1]    token id -> first scalar of its folded piece; an id without a piece (or a special one) has an empty span
//   piece scalars[n_piece_scalars]
// Nothing read from a blob forms an address before it is compared with the blob's length in words; a reader gets `false` instead.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FA_RB_HD __host__ __device__
#else
#define FA_RB_HD
#endif

#ifndef FA_RNNT_BIAS_MAX_FORM
#define FA_RNNT_BIAS_MAX_FORM 256
#endif

namespace fa {
namespace rnnt_bias {

constexpr int32_t kMagic = 0x42524146;   // "FARB"
constexpr int32_t kVersion = 1;
constexpr int32_t kHeaderWords = 16;
constexpr int32_t kMaxForm = FA_RNNT_BIAS_MAX_FORM;
constexpr uint32_t kMarker = 0x2581;     // SentencePiece's word-boundary marker (:215)

struct Header {
    int32_t vocab, tail_cap, n_nodes, off_nodes, n_edges, off_edge_keys, off_edge_children, n_cands, off_cands, off_piece_index, n_piece_scalars,
        off_piece_scalars;
};

enum HeaderVerdict { kHeaderOk = 0, kHeaderMismatch = 1, kHeaderMalformed = 2 };

// a section of `count` records of `per` words at `off` lies behind the header and inside the blob
FA_RB_HD inline bool section_ok(const int64_t off, const int64_t count, const int64_t per, const int64_t words) {
    return off >= kHeaderWords && count >= 0 && count <= words && off <= words && off + count * per <= words;
}

// The header of blob[words], checked: kHeaderMismatch — no header, another magic / version, or a table for another vocab / tail_cap
// (vocab < 0 / tail_cap < 0: whatever the blob says) —, kHeaderMalformed — a section that leaves the blob.
FA_RB_HD inline HeaderVerdict read_header(const int32_t *blob, const int64_t words, const int32_t vocab, const int32_t tail_cap, Header &h) {
    if (!blob || words < kHeaderWords) return kHeaderMismatch;
    if (blob[0] != kMagic || blob[1] != kVersion) return kHeaderMismatch;
    h.vocab = blob[2]; h.tail_cap = blob[3]; h.n_nodes = blob[4]; h.off_nodes = blob[5]; h.n_edges = blob[6]; h.off_edge_keys = blob[7];
    h.off_edge_children = blob[8]; h.n_cands = blob[9]; h.off_cands = blob[10]; h.off_piece_index = blob[11]; h.n_piece_scalars = blob[12];
    h.off_piece_scalars = blob[13];
    if (h.vocab < 1 || h.tail_cap < 1 || h.tail_cap > kMaxForm) return kHeaderMismatch;
    if ((vocab >= 0 && h.vocab != vocab) || (tail_cap >= 0 && h.tail_cap != tail_cap)) return kHeaderMismatch;
    if (blob[14] > words || blob[14] < kHeaderWords) return kHeaderMalformed;
    if (h.n_nodes < 1 || !section_ok(h.off_nodes, h.n_nodes, 4, words) || !section_ok(h.off_edge_keys, h.n_edges, 1, words) ||
        !section_ok(h.off_edge_children, h.n_edges, 1, words) || !section_ok(h.off_cands, h.n_cands, 2, words) ||
        !section_ok(h.off_piece_index, static_cast<int64_t>(h.vocab) + 1, 1, words) || !section_ok(h.off_piece_scalars, h.n_piece_scalars, 1, words))
        return kHeaderMalformed;
    return kHeaderOk;
}

// Everything below takes a header that read_header accepted for the same blob.

// node's candidate list: records [first, first + count) of the candidate section
FA_RB_HD inline bool node_candidates(const int32_t *blob, const Header &h, const int32_t node, int32_t &first, int32_t &count) {
    if (node < 0 || node >= h.n_nodes) return false;
    const int32_t *n = blob + h.off_nodes + 4 * static_cast<int64_t>(node);
    first = n[2]; count = n[3];
    return first >= 0 && count >= 0 && static_cast<int64_t>(first) + count <= h.n_cands;
}

FA_RB_HD inline void candidate(const int32_t *blob, const Header &h, const int32_t index, int32_t &id, float &boost) {   // index: inside a checked list
    const int32_t *c = blob + h.off_cands + 2 * static_cast<int64_t>(index);
    id = c[0];
    union { int32_t i; float f; } u;
    u.i = c[1];
    boost = u.f;
}

// The child of `node` along `scalar`: child >= 1, or -1 where the trie has none.  At most 32 halvings, whatever the blob holds.
FA_RB_HD inline bool node_child(const int32_t *blob, const Header &h, const int32_t node, const uint32_t scalar, int32_t &child) {
    child = -1;
    if (node < 0 || node >= h.n_nodes) return false;
    const int32_t *n = blob + h.off_nodes + 4 * static_cast<int64_t>(node);
    const int32_t first = n[0], count = n[1];
    if (first < 0 || count < 0 || static_cast<int64_t>(first) + count > h.n_edges) return false;
    const int32_t *keys = blob + h.off_edge_keys;
    int32_t lo = first, hi = first + count;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int32_t mid = lo + (hi - lo) / 2;
        const uint32_t k = static_cast<uint32_t>(keys[mid]);
        if (k == scalar) {
            const int32_t c = blob[h.off_edge_children + static_cast<int64_t>(mid)];
            if (c < 1 || c >= h.n_nodes) return false;
            child = c;
            return true;
        }
        if (k < scalar) lo = mid + 1; else hi = mid;
    }
    return true;
}

// the scalars of token id's folded piece: [first, first + count) of the piece-scalar section; empty for an id outside the vocabulary
FA_RB_HD inline bool piece_span(const int32_t *blob, const Header &h, const int32_t id, int32_t &first, int32_t &count) {
    first = 0; count = 0;
    if (id < 0 || id >= h.vocab) return true;
    const int32_t *p = blob + h.off_piece_index + static_cast<int64_t>(id);
    const int32_t a = p[0], b = p[1];
    if (a < 0 || b < a || b > h.n_piece_scalars) return false;
    first = a; count = b - a;
    return true;
}

FA_RB_HD inline uint32_t piece_scalar(const int32_t *blob, const Header &h, const int32_t index) {   // index: inside a checked span
    return static_cast<uint32_t>(blob[h.off_piece_scalars + static_cast<int64_t>(index)]);
}

inline float effective_boost(const int has_weight, const float weight, const float default_boost) {   // :196-199
    return (has_weight && weight <= 6.0f) ? weight : default_boost;
}

}  // namespace rnnt_bias
}  // namespace fa

// ---- host only: the builder and the reference's candidates() on a blob
#include <algorithm>
#include <map>
#include <vector>

namespace fa {
namespace rnnt_bias {

enum BuildStatus { kBuildOk = 0, kBuildInvalid = 1, kBuildTooSmall = 3 };   // the values of fa_status

typedef std::vector<uint32_t> Scalars;

// text -> scalars; false: not well-formed UTF-8 (a stray or missing continuation byte, an overlong form, a surrogate, above U+10FFFF)
inline bool decode_utf8(const char *text, Scalars &out) {
    const unsigned char *s = reinterpret_cast<const unsigned char *>(text);
    out.clear();
    while (*s) {
        const unsigned c = *s++;
        if (c < 0x80) { out.push_back(c); continue; }
        int more;
        uint32_t v, least;
        if (c >= 0xC2 && c <= 0xDF) { more = 1; v = c & 0x1F; least = 0x80; }
        else if (c >= 0xE0 && c <= 0xEF) { more = 2; v = c & 0x0F; least = 0x800; }
        else if (c >= 0xF0 && c <= 0xF4) { more = 3; v = c & 0x07; least = 0x10000; }
        else return false;
        for (int i = 0; i < more; ++i) {
            const unsigned d = *s;                      // a NUL is no continuation byte: the scan never passes the terminator
            if ((d & 0xC0) != 0x80) return false;
            ++s;
            v = (v << 6) | (d & 0x3F);
        }
        if (v < least || v > 0x10FFFF || (v >= 0xD800 && v <= 0xDFFF)) return false;
        out.push_back(v);
    }
    return true;
}

inline bool is_cjk(const uint32_t v) {          // :219-228
    return (v >= 0x3040 && v <= 0x30FF) || (v >= 0x3400 && v <= 0x4DBF) || (v >= 0x4E00 && v <= 0x9FFF) || (v >= 0xAC00 && v <= 0xD7AF) ||
           (v >= 0xF900 && v <= 0xFAFF);
}

inline bool is_white_space(const uint32_t v) {  // the Unicode White_Space property
    return (v >= 0x09 && v <= 0x0D) || v == 0x20 || v == 0x85 || v == 0xA0 || v == 0x1680 || (v >= 0x2000 && v <= 0x200A) || v == 0x2028 ||
           v == 0x2029 || v == 0x202F || v == 0x205F || v == 0x3000;
}

inline Scalars piece_form(const Scalars &folded) {   // :233-250
    const bool anchored = !(folded.size() && is_cjk(folded[0]));
    Scalars form;
    bool at_boundary = true;
    for (const uint32_t v : folded) {
        if (is_white_space(v)) { at_boundary = true; continue; }
        if (at_boundary) { if (anchored) form.push_back(kMarker); at_boundary = false; }
        form.push_back(v);
    }
    return form;
}

inline bool is_special(const Scalars &piece) { return piece.size() && piece.front() == '<' && piece.back() == '>'; }   // :152

struct Entry { Scalars form; float boost; };
struct Node {
    std::map<uint32_t, int32_t> children;
    std::vector<int32_t> entries;
    int32_t depth = 0;
};

// accumulate (:310-339): the vocabulary pieces equal to a prefix of form[offset...] -> best[id] = the strongest boost
inline void accumulate(const Entry &e, const size_t offset, const std::map<Scalars, std::vector<int32_t>> &ids_by_piece, std::map<int32_t, float> &best) {
    if (offset >= e.form.size()) return;
    Scalars piece;
    int letters = 0;
    for (size_t i = offset; i < e.form.size(); ++i) {
        piece.push_back(e.form[i]);
        if (e.form[i] != kMarker) ++letters;
        if (piece.size() == 1 && piece[0] == kMarker) continue;            // the bare marker narrows nothing
        const auto hit = ids_by_piece.find(piece);
        if (hit == ids_by_piece.end()) continue;
        if (offset == 0 && e.form[0] == kMarker && letters < 2) continue;  // opening a fresh word needs two letters
        for (const int32_t id : hit->second) {
            const auto at = best.find(id);
            if (at == best.end()) best[id] = e.boost;
            else if (e.boost > at->second) at->second = e.boost;
        }
    }
}

// fa_rnnt_bias_build (include/fluidaudio_hip.h) without the C types
inline int build(const char *const *folded_pieces, const int32_t vocab, const char *const *folded_surfaces, const float *boosts, const int32_t n_surfaces,
                 int32_t *blob, const int64_t capacity_words, int64_t *words_needed, int32_t *tail_cap) {
    if (!words_needed || !tail_cap || vocab < 0 || n_surfaces < 0 || capacity_words < 0 || (capacity_words > 0 && !blob)) return kBuildInvalid;
    if ((vocab > 0 && !folded_pieces) || (n_surfaces > 0 && (!folded_surfaces || !boosts))) return kBuildInvalid;
    std::vector<Entry> entries;
    int32_t cap = 0;
    Scalars s;
    for (int32_t i = 0; i < n_surfaces; ++i) {
        if (!folded_surfaces[i] || !(boosts[i] > 0.0f) || !decode_utf8(folded_surfaces[i], s)) return kBuildInvalid;   // (a NaN boost is not > 0)
        Scalars form = piece_form(s);
        if (form.size() > static_cast<size_t>(kMaxForm)) return kBuildInvalid;
        if (form.empty()) continue;                                        // nothing to match: no trie node, no candidate
        cap = std::max(cap, static_cast<int32_t>(form.size()));
        entries.push_back(Entry{std::move(form), boosts[i]});
    }
    std::map<Scalars, std::vector<int32_t>> ids_by_piece;
    std::vector<int32_t> piece_index(static_cast<size_t>(vocab) + 1, 0);
    std::vector<int32_t> piece_scalars;
    for (int32_t id = 0; id < vocab; ++id) {
        piece_index[id] = static_cast<int32_t>(piece_scalars.size());
        if (!folded_pieces[id]) continue;
        if (!decode_utf8(folded_pieces[id], s)) return kBuildInvalid;
        if (is_special(s)) continue;
        ids_by_piece[s].push_back(id);
        if (piece_scalars.size() + s.size() > static_cast<size_t>(INT32_MAX / 2)) return kBuildInvalid;
        piece_scalars.insert(piece_scalars.end(), s.begin(), s.end());
    }
    if (vocab >= 0) piece_index[vocab] = static_cast<int32_t>(piece_scalars.size());
    *words_needed = 0;
    *tail_cap = 0;
    if (entries.empty() || vocab == 0) return kBuildOk;                    // "no bias"

    std::vector<Node> nodes(1);
    for (size_t e = 0; e < entries.size(); ++e) {
        nodes[0].entries.push_back(static_cast<int32_t>(e));               // every entry continues from offset 0: freshStartCandidates
        int32_t at = 0;
        for (const uint32_t v : entries[e].form) {
            int32_t next;
            const auto hit = nodes[at].children.find(v);
            if (hit == nodes[at].children.end()) {
                next = static_cast<int32_t>(nodes.size());
                nodes[at].children[v] = next;
                const int32_t depth = nodes[at].depth + 1;
                nodes.emplace_back();
                nodes.back().depth = depth;
            } else next = hit->second;
            nodes[next].entries.push_back(static_cast<int32_t>(e));
            at = next;
        }
    }
    std::vector<int32_t> node_words, edge_keys, edge_children, cands;
    for (const Node &n : nodes) {
        node_words.push_back(static_cast<int32_t>(edge_keys.size()));
        node_words.push_back(static_cast<int32_t>(n.children.size()));
        for (const auto &kv : n.children) { edge_keys.push_back(static_cast<int32_t>(kv.first)); edge_children.push_back(kv.second); }   // (a map: ascending keys)
        std::map<int32_t, float> best;
        for (const int32_t e : n.entries) accumulate(entries[e], static_cast<size_t>(n.depth), ids_by_piece, best);
        node_words.push_back(static_cast<int32_t>(cands.size() / 2));
        node_words.push_back(static_cast<int32_t>(best.size()));
        for (const auto &kv : best) {
            union { float f; int32_t i; } u;
            u.f = kv.second;
            cands.push_back(kv.first);
            cands.push_back(u.i);
        }
    }
    const int64_t total = static_cast<int64_t>(kHeaderWords) + static_cast<int64_t>(node_words.size()) + 2 * static_cast<int64_t>(edge_keys.size()) +
                          static_cast<int64_t>(cands.size()) + static_cast<int64_t>(piece_index.size()) + static_cast<int64_t>(piece_scalars.size());
    if (total > INT32_MAX) return kBuildInvalid;
    *words_needed = total;
    *tail_cap = cap;
    if (capacity_words == 0) return kBuildOk;
    if (capacity_words < total) return kBuildTooSmall;
    int32_t at = kHeaderWords;
    auto put = [&](const std::vector<int32_t> &v) { const int32_t off = at; std::copy(v.begin(), v.end(), blob + at); at += static_cast<int32_t>(v.size()); return off; };
    blob[0] = kMagic; blob[1] = kVersion; blob[2] = vocab; blob[3] = cap;
    blob[4] = static_cast<int32_t>(nodes.size()); blob[5] = put(node_words);
    blob[6] = static_cast<int32_t>(edge_keys.size()); blob[7] = put(edge_keys); blob[8] = put(edge_children);
    blob[9] = static_cast<int32_t>(cands.size() / 2); blob[10] = put(cands);
    blob[11] = put(piece_index);
    blob[12] = static_cast<int32_t>(piece_scalars.size()); blob[13] = put(piece_scalars);
    blob[14] = static_cast<int32_t>(total); blob[15] = 0;
    return kBuildOk;
}

// The match state, host form: the trie node of every suffix of the tail that is still a prefix of some form, by suffix start.  One
// appended scalar advances every live suffix by one child look-up; a suffix as long as the longest form has no child, so dropping the
// oldest start at tail_cap never drops a live match.
struct Matcher {
    const int32_t *blob;
    Header h;
    std::vector<uint32_t> tail;
    std::vector<int32_t> node;   // per tail position: the node of tail[position ...], or -1
    bool append(const uint32_t scalar) {
        if (tail.size() == static_cast<size_t>(h.tail_cap)) { tail.erase(tail.begin()); node.erase(node.begin()); }   // the oldest start makes room
        tail.push_back(scalar);
        node.push_back(0);
        for (int32_t &n : node) {
            if (n < 0) continue;
            int32_t c;
            if (!node_child(blob, h, n, scalar, c)) return false;
            n = c;
        }
        return true;
    }
    bool observe(const int32_t id) {   // :254-261
        int32_t first, count;
        if (!piece_span(blob, h, id, first, count)) return false;
        for (int32_t i = 0; i < count; ++i)
            if (!append(piece_scalar(blob, h, first + i))) return false;
        return true;
    }
    bool candidates(std::map<int32_t, float> &best) const {   // :280-306
        auto add = [&](const int32_t n) {
            int32_t first, count;
            if (!node_candidates(blob, h, n, first, count)) return false;
            for (int32_t i = 0; i < count; ++i) {
                int32_t id;
                float boost;
                candidate(blob, h, first + i, id, boost);
                const auto at = best.find(id);
                if (at == best.end()) best[id] = boost;
                else if (boost > at->second) at->second = boost;
            }
            return true;
        };
        if (!add(0)) return false;
        for (const int32_t n : node)
            if (n >= 0 && !add(n)) return false;
        return true;
    }
};

// fa_rnnt_bias_candidates without the C types
inline int candidates(const int32_t *blob, const int64_t words, const int32_t *observed, const int32_t n_observed, int32_t *ids, float *boosts,
                      const int32_t capacity, int32_t *count) {
    if (!count || n_observed < 0 || capacity < 0 || (n_observed > 0 && !observed) || (capacity > 0 && (!ids || !boosts))) return kBuildInvalid;
    Matcher m;
    m.blob = blob;
    if (read_header(blob, words, -1, -1, m.h) != kHeaderOk) return kBuildInvalid;
    for (int32_t i = 0; i < n_observed; ++i)
        if (!m.observe(observed[i])) return kBuildInvalid;
    std::map<int32_t, float> best;
    if (!m.candidates(best)) return kBuildInvalid;
    *count = static_cast<int32_t>(best.size());
    if (static_cast<int64_t>(best.size()) > capacity) return kBuildTooSmall;
    int32_t k = 0;
    for (const auto &kv : best) { ids[k] = kv.first; boosts[k] = kv.second; ++k; }
    return kBuildOk;
}

}  // namespace rnnt_bias
}  // namespace fa
