// tdt_lang_host.hip — the class bytes the language mode of the TDT walk reads (tdt_lang.h): TokenLanguageFilter.matches
// (Shared/TokenLanguageFilter.swift:81-134) for the three scripts, vocabulary membership and the caller's blocklist, one byte per token.
// Host only: no context, no device.  The text is decoded here, scalar by scalar; nothing but well-formed UTF-8 is accepted.
#include <cstdint>

#include "../../include/fluidaudio_hip.h"

namespace {

constexpr uint32_t kBoundary = 0x2581;   // SentencePiece's word-boundary marker: stripped, it carries no script (:73, :82)

// the next scalar of s; false: not well-formed UTF-8 (a stray or missing continuation byte, an overlong form, a surrogate, above U+10FFFF)
bool next_scalar(const unsigned char *&s, uint32_t &out) {
    const unsigned c = *s++;
    if (c < 0x80) { out = c; return true; }
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
    out = v;
    return true;
}

bool ascii_letter(const uint32_t v) { return (v >= 0x41 && v <= 0x5A) || (v >= 0x61 && v <= 0x7A); }
bool in(const uint32_t v, const uint32_t lo, const uint32_t hi) { return v >= lo && v <= hi; }

bool latin_scalar(const uint32_t v) {      // :91-98
    return in(v, 0x0020, 0x007F) || in(v, 0x00A0, 0x00FF) || in(v, 0x0100, 0x017F) || in(v, 0x0180, 0x024F) || in(v, 0x0300, 0x036F) || in(v, 0x1E00, 0x1EFF);
}
bool cyrillic_scalar(const uint32_t v) {   // :100-112: ASCII is neutral except for its letters
    return in(v, 0x0400, 0x04FF) || (in(v, 0x0020, 0x007F) && !ascii_letter(v));
}
bool greek_scalar(const uint32_t v) {      // :114-131
    return in(v, 0x0370, 0x03FF) || in(v, 0x1F00, 0x1FFF) || in(v, 0x0300, 0x036F) || (in(v, 0x0020, 0x007F) && !ascii_letter(v));
}

// the *_OK bits of a text; false: not UTF-8.  No scalar besides the marker: every script matches (:86).
bool script_bits(const char *text, uint8_t &bits) {
    bool latin = true, cyrillic = true, greek = true;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(text);
    while (*s) {
        uint32_t v;
        if (!next_scalar(s, v)) return false;
        if (v == kBoundary) continue;
        latin = latin && latin_scalar(v);
        cyrillic = cyrillic && cyrillic_scalar(v);
        greek = greek && greek_scalar(v);
    }
    bits = static_cast<uint8_t>((latin ? FA_TDT_CLASS_LATIN_OK : 0) | (cyrillic ? FA_TDT_CLASS_CYRILLIC_OK : 0) | (greek ? FA_TDT_CLASS_GREEK_OK : 0));
    return true;
}

}  // namespace

extern "C" fa_status fa_tdt_token_classes(const char *const *utf8_tokens, const int32_t *present, int32_t vocab_with_blank, const int32_t *blocklist_ids,
                                          int32_t n_block, uint8_t *classes) {
    if (vocab_with_blank < 0 || n_block < 0 || (vocab_with_blank > 0 && (!utf8_tokens || !classes)) || (n_block > 0 && !blocklist_ids)) return FA_INVALID_ARGUMENT;
    for (int32_t i = 0; i < n_block; ++i)
        if (blocklist_ids[i] < 0 || blocklist_ids[i] >= vocab_with_blank) return FA_INVALID_ARGUMENT;
    for (int32_t i = 0; i < vocab_with_blank; ++i) {        // every text is checked before a byte is written
        uint8_t bits;
        if (utf8_tokens[i] && !script_bits(utf8_tokens[i], bits)) return FA_INVALID_ARGUMENT;
    }
    for (int32_t i = 0; i < vocab_with_blank; ++i) {
        const bool there = utf8_tokens[i] && (!present || present[i]);
        uint8_t bits = 0;
        script_bits(there ? utf8_tokens[i] : "", bits);
        classes[i] = static_cast<uint8_t>(bits | (there ? FA_TDT_CLASS_IN_VOCAB : 0));
    }
    for (int32_t i = 0; i < n_block; ++i) classes[blocklist_ids[i]] |= FA_TDT_CLASS_BLOCKLISTED;
    return FA_SUCCESS;
}
