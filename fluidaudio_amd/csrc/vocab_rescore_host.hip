// vocab_rescore_host.hip — the host unit of the vocabulary rescorer (kernels: vocab_rescore.hip, operands: vocab_rescore_launch.h, the
// plain C++ of the blob, the arithmetic and the arbitration: vocab_rescore_core.h): the candidate call and the verdict call as their
// steps — argument pass, stage, launch, fetch, sort / arbitrate, deliver — and the C ABI.  The verdict call scores nothing itself: the
// three keywords of a candidate go through fa_ctc_kws_score_windows(_dev) in one batched call.
#include <cmath>
#include <cstdlib>

#include "vocab_rescore_launch.h"

namespace {

using fa::vr::Block;
using fa::vr::Header;
using fa::vr::WalkArgs;
using fa::vr::Words;

fa_status accepted(fa_ctx *ctx, const char *what, const fa::Verdict &v) {
    return v.status == FA_SUCCESS ? FA_SUCCESS : fa::set_error(ctx, v.status, "%s: %s", what, v.text);
}

const fa_vr_boost_config kDefaultBoost{1, 3, 1, 2.0f};   // ContextBiasingConstants: defaultUseAdaptiveThresholds, defaultReferenceTokenCount, the taper off

fa_status candidates(fa_ctx *ctx, const int32_t *blob, int64_t blob_words, const int64_t *utterance_offsets, int32_t batch, const int64_t *word_offsets,
                     const int32_t *word_symbols, const uint8_t *word_flags, float min_similarity, fa_vr_candidate *out, int64_t capacity, int64_t *count,
                     int64_t *utt_counts) {
    const char *what = "vocab_rescore_candidates";
    if (count) *count = 0;
    if (!ctx || !count) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: ctx and count are required", what);
    if (capacity < 0 || (capacity > 0 && !out)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: negative capacity, or a capacity without an output", what);
    return fa::no_throw(ctx, what, [&]() -> fa_status {
        // the argument pass: the blob whole, then the words as dense ids
        Header h;
        FA_TRY(accepted(ctx, what, fa::vr::validate(blob, blob_words, h)));
        Words w;
        FA_TRY(accepted(ctx, what, fa::vr::check_words(blob, h, utterance_offsets, batch, word_offsets, word_symbols, word_flags, min_similarity, w)));
        if (utt_counts) std::fill(utt_counts, utt_counts + batch, int64_t{0});
        const int64_t n_words = w.n_words();
        if (n_words == 0 || h.n_terms == 0) return FA_SUCCESS;
        std::vector<Block> blocks;
        for (int32_t u = 0; u < batch; ++u) {
            const int64_t W = w.utt_words[u + 1] - w.utt_words[u];
            for (int64_t i = 0; i < W; i += fa::vr::kStarts) blocks.push_back(Block{u, static_cast<int32_t>(i)});
        }
        if (static_cast<int64_t>(blocks.size()) * h.n_terms >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "%s: 2^31 (word block, term) pairs or more", what);
        const char *forced = fa::sw(fa::Sw::VR_ARENA);   // tests ask for a smaller arena
        int64_t arena_cap = forced ? std::max<int64_t>(0, std::atoll(forced)) : std::max<int64_t>(fa::vr::kDefaultArena, capacity);

        // stage
        fa::DeviceGuard guard(ctx->device);
        hipStream_t st = ctx->stream;
        fa::DevBuf b_blob, b_syms, b_woff, b_uoff, b_flags, b_sid, b_blocks, b_arena, b_cursor;
        FA_TRY(fa::take(ctx, what, {{&b_blob, sizeof(int32_t) * static_cast<size_t>(h.total), true, blob},
                                    {&b_syms, sizeof(uint16_t) * w.syms.size(), true, w.syms.data()},
                                    {&b_woff, sizeof(int64_t) * w.word_off.size(), true, w.word_off.data()},
                                    {&b_uoff, sizeof(int64_t) * w.utt_words.size(), true, w.utt_words.data()},
                                    {&b_flags, w.flags.size(), true, w.flags.data()},
                                    {&b_sid, sizeof(int32_t) * fa::vr::kMaxSpan * static_cast<size_t>(n_words)},
                                    {&b_blocks, sizeof(Block) * blocks.size(), true, blocks.data()},
                                    {&b_arena, sizeof(fa_vr_candidate) * static_cast<size_t>(arena_cap)},
                                    {&b_cursor, sizeof(unsigned long long)}}));
        WalkArgs a{};
        a.blob = b_blob.as<int32_t>(); a.h = h; a.syms = b_syms.as<uint16_t>(); a.word_off = b_woff.as<int64_t>(); a.utt_words = b_uoff.as<int64_t>();
        a.flags = b_flags.as<uint8_t>(); a.sid = b_sid.as<int32_t>(); a.n_words = n_words; a.batch = batch; a.blocks = b_blocks.as<Block>();
        a.n_blocks = static_cast<int32_t>(blocks.size()); a.min_similarity = min_similarity; a.arena = b_arena.as<fa_vr_candidate>(); a.arena_cap = arena_cap;
        a.cursor = b_cursor.as<unsigned long long>();

        // the pre-pass and the walk, then the cursor and the arena's first records behind ONE synchronisation
        std::vector<fa_vr_candidate> recs;
        unsigned long long cursor = 0;
        double device_ms = 0.0;
        const auto walk = [&](const bool with_sids) -> fa_status {
            FA_HIP_TRY(ctx, hipMemsetAsync(a.cursor, 0, sizeof(unsigned long long), st));
            FA_TRY(fa::DeviceTiming{ctx}.begin());
            if (with_sids) fa::vr::launch_sids(st, a);
            fa::vr::launch_walk(st, a);
            FA_HIP_TRY(ctx, hipGetLastError());
            FA_TRY(fa::DeviceTiming{ctx}.end());
            const int64_t first = std::min(a.arena_cap, fa::vr::kDefaultArena);
            recs.resize(static_cast<size_t>(first));
            FA_HIP_TRY(ctx, hipMemcpyAsync(&cursor, a.cursor, sizeof(cursor), hipMemcpyDeviceToHost, st));
            if (first > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(recs.data(), a.arena, sizeof(fa_vr_candidate) * static_cast<size_t>(first), hipMemcpyDeviceToHost, st));
            FA_HIP_TRY(ctx, hipStreamSynchronize(st));
            FA_TRY(fa::DeviceTiming{ctx}.read(&device_ms));
            return FA_SUCCESS;
        };
        FA_TRY(walk(true));
        if (cursor > static_cast<unsigned long long>(a.arena_cap)) {   // the count is known now: once more with room for it
            if (cursor >= static_cast<unsigned long long>(INT32_MAX)) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "%s: 2^31 candidates or more", what);
            arena_cap = static_cast<int64_t>(cursor);
            b_arena.reset();
            FA_TRY(fa::take(ctx, what, {{&b_arena, sizeof(fa_vr_candidate) * static_cast<size_t>(arena_cap)}}));
            a.arena = b_arena.as<fa_vr_candidate>(); a.arena_cap = arena_cap;
            const unsigned long long before = cursor;
            FA_TRY(walk(false));
            if (cursor != before) return fa::set_error(ctx, FA_RUNTIME_ERROR, "%s: the second walk found %llu candidates, the first %llu", what, cursor, before);
        }
        const size_t total = static_cast<size_t>(cursor);
        if (total > recs.size()) {   // more than the first fetch held
            const size_t have = recs.size();
            recs.resize(total);
            FA_HIP_TRY(ctx, hipMemcpyAsync(recs.data() + have, a.arena + have, sizeof(fa_vr_candidate) * (total - have), hipMemcpyDeviceToHost, st));
            FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        recs.resize(total);
        for (const fa_vr_candidate &r : recs)   // what the device wrote is checked before it orders or indexes anything
            if (r.utterance < 0 || r.utterance >= batch || r.term < 0 || r.term >= h.input_terms || r.first_word < 0 || r.span_len < 1 || r.span_len > fa::vr::kMaxSpan ||
                (r.origin != FA_VR_ORIGIN_MULTI_WORD && r.origin != FA_VR_ORIGIN_SINGLE_WORD))
                return fa::set_error(ctx, FA_RUNTIME_ERROR, "%s: a record names utterance %d, term %d, word %d, span %d", what, r.utterance, r.term, r.first_word, r.span_len);
        std::sort(recs.begin(), recs.end(), fa::vr::candidate_before);   // the keys are distinct: the reference's append order
        return accepted(ctx, what, fa::vr::deliver(recs, batch, out, capacity, count, utt_counts));
    });
}

bool ascends(const int64_t *off, const int64_t n) {
    if (off[0] < 0) return false;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

fa_status decide(fa_ctx *ctx, const float *lp, bool device, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                 const int32_t *valid_frames, const fa_vr_decide_config *cfg_in, const fa_vr_candidate *cands, int64_t n, const int64_t *utt_off,
                 const double *word_starts, const double *word_ends, int32_t terms, const int32_t *term_tokens, const int64_t *term_off, const int32_t *alt_tokens,
                 const int64_t *alt_off, const int32_t *phrase_tokens, const int64_t *phrase_off, const uint8_t *occupied, fa_vr_verdict *verdicts, int32_t *applied,
                 int64_t *applied_counts) {
    const char *what = "vocab_rescore_decide";
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n < 0 || n >= INT32_MAX / 4 || batch < 0 || terms < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: bad shape", what);
    if (n > 0 && (!cands || !verdicts || !utt_off || !word_starts || !word_ends || !term_off || !phrase_off))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: candidates, verdicts, utterance_offsets, word times, term_token_offsets and phrase_token_offsets are required", what);
    return fa::no_throw(ctx, what, [&]() -> fa_status {
        fa_vr_decide_config cfg;
        if (cfg_in) cfg = *cfg_in; else fa_vocab_rescore_default_config(&cfg);
        if (!(cfg.frame_duration > 0.0) || !std::isfinite(cfg.frame_duration) || !std::isfinite(cfg.margin_seconds))
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: frame_duration has to be positive and finite, margin_seconds finite", what);
        if (applied_counts) std::fill(applied_counts, applied_counts + batch, int64_t{0});
        if (n == 0) return FA_SUCCESS;
        if (!ascends(utt_off, batch)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: utterance_offsets does not ascend from 0 or more", what);
        if (!ascends(term_off, terms) || (alt_off && !ascends(alt_off, terms)) || !ascends(phrase_off, n))
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: token offsets do not ascend from 0 or more", what);
        if ((term_off[terms] > term_off[0] && !term_tokens) || (alt_off && alt_off[terms] > alt_off[0] && !alt_tokens) || (phrase_off[n] > phrase_off[0] && !phrase_tokens))
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: tokens are required where the offsets name some", what);
        for (int32_t t = 0; t < terms; ++t) {
            const int64_t a = term_off[t + 1] - term_off[t], b = alt_off ? alt_off[t + 1] - alt_off[t] : 0;
            if (a > FA_KWS_MAX_TOKENS || b > FA_KWS_MAX_TOKENS)
                return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: term %d has %lld tokens, at most %d are supported", what, t, (long long)std::max(a, b), (int)FA_KWS_MAX_TOKENS);
        }
        std::vector<int32_t> valid(static_cast<size_t>(batch), frames);
        if (valid_frames)
            for (int32_t u = 0; u < batch; ++u) valid[u] = std::min(frames, std::max(0, valid_frames[u]));

        // the keywords of the one window call: the terms, their alternatives, the phrases; per candidate up to three windows
        std::vector<int32_t> tokens;
        std::vector<int64_t> off{0};
        const auto add = [&](const int32_t *src, const int64_t a, const int64_t b) {
            if (b > a) tokens.insert(tokens.end(), src + a, src + b);
            off.push_back(static_cast<int64_t>(tokens.size()));
        };
        for (int32_t t = 0; t < terms; ++t) add(term_tokens, term_off[t], term_off[t + 1]);
        for (int32_t t = 0; t < terms; ++t) add(alt_tokens, alt_off ? alt_off[t] : 0, alt_off ? alt_off[t + 1] : 0);
        for (int64_t c = 0; c < n; ++c) {
            if (phrase_off[c + 1] - phrase_off[c] > FA_KWS_MAX_TOKENS)
                return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: candidate %lld's phrase has %lld tokens, at most %d are supported", what, (long long)c,
                                     (long long)(phrase_off[c + 1] - phrase_off[c]), (int)FA_KWS_MAX_TOKENS);
            add(phrase_tokens, phrase_off[c], phrase_off[c + 1]);
        }
        const int64_t keywords = static_cast<int64_t>(off.size()) - 1;
        if (keywords >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "%s: 2^31 keywords or more", what);
        struct Slots { int64_t term = -1, alt = -1, phrase = -1; };
        std::vector<Slots> slots(static_cast<size_t>(n));
        std::vector<fa_kws_window> windows;
        for (int64_t c = 0; c < n; ++c) {
            const fa_vr_candidate &r = cands[c];
            if (r.utterance < 0 || r.utterance >= batch || r.term < 0 || r.term >= terms)
                return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: candidate %lld names utterance %d, term %d", what, (long long)c, r.utterance, r.term);
            const int64_t W = utt_off[r.utterance + 1] - utt_off[r.utterance];
            if (r.first_word < 0 || r.span_len < 1 || static_cast<int64_t>(r.first_word) + r.span_len > W)
                return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: candidate %lld spans the words %d + %d of %lld", what, (long long)c, r.first_word, r.span_len, (long long)W);
            if (!fa::vr::bucket_ok(r.similarity)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: candidate %lld's similarity is not a usable number", what, (long long)c);
            const int64_t g = utt_off[r.utterance] + r.first_word;
            fa_vr_verdict &v = verdicts[c];
            v = fa_vr_verdict{-HUGE_VALF, -HUGE_VALF, 0.0f, -HUGE_VALF, 0, 0, 0, FA_VR_UNAVAILABLE, 0, 0};
            if (!fa::vr::frame_window(word_starts[g], word_ends[g + r.span_len - 1], cfg.frame_duration, cfg.margin_seconds, valid[r.utterance], v.start_frame, v.end_frame))
                return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: candidate %lld's times give no frame window", what, (long long)c);
            const int64_t nt = off[r.term + 1] - off[r.term], na = off[terms + r.term + 1] - off[terms + r.term];
            const auto window = [&](const int64_t keyword) {
                windows.push_back(fa_kws_window{r.utterance, static_cast<int32_t>(keyword), v.start_frame, v.end_frame});
                return static_cast<int64_t>(windows.size()) - 1;
            };
            if (nt == 0) continue;   // the reference leaves a term without tokens before it looks for candidates (:738-742)
            slots[c].term = window(r.term);
            const bool same = na == nt && std::equal(tokens.begin() + off[r.term], tokens.begin() + off[r.term + 1], tokens.begin() + off[terms + r.term]);
            if (na > 0 && !same) slots[c].alt = window(terms + r.term);                                  // :61-75
            if (off[2 * terms + c + 1] > off[2 * terms + c]) slots[c].phrase = window(2 * static_cast<int64_t>(terms) + c);   // :93-107
        }
        std::vector<fa_kws_detection> scores(windows.size());
        if (!windows.empty()) {
            const int32_t dummy = 0;
            const int32_t *tok = tokens.empty() ? &dummy : tokens.data();
            FA_TRY((device ? fa_ctc_kws_score_windows_dev : fa_ctc_kws_score_windows)(ctx, lp, batch, frames, vocab, row_stride, matrix_stride, valid_frames, tok, off.data(),
                                                                                      static_cast<int32_t>(keywords), windows.data(), static_cast<int64_t>(windows.size()),
                                                                                      cfg.blank_id, scores.data()));
        }

        // the verdicts (:50-122), then the arbitration per utterance (:272-307)
        std::vector<std::vector<int32_t>> pending(static_cast<size_t>(batch));
        for (int64_t c = 0; c < n; ++c) {
            fa_vr_verdict &v = verdicts[c];
            const Slots &s = slots[c];
            if (s.term < 0) continue;
            v.term_score = scores[s.term].score;
            int64_t used = off[cands[c].term + 1] - off[cands[c].term];
            if (s.alt >= 0 && scores[s.alt].score > v.term_score) {
                v.term_score = scores[s.alt].score;
                v.alt_won = 1;
                used = off[terms + cands[c].term + 1] - off[terms + cands[c].term];
            }
            v.boosted_score = v.term_score;
            if (s.phrase < 0) continue;
            v.compared = 1;
            v.original_score = scores[s.phrase].score;
            v.boost = fa::vr::boost(cfg.cbw, static_cast<int32_t>(used), cfg.boost);
            v.boosted_score = v.term_score + v.boost;
            v.should_replace = v.boosted_score > v.original_score ? 1 : 0;
            v.outcome = v.should_replace ? FA_VR_SUPERSEDED : FA_VR_REJECTED;
            if (v.should_replace) pending[cands[c].utterance].push_back(static_cast<int32_t>(c));
        }
        int64_t at = 0;
        std::vector<float> sims;
        std::vector<int32_t> firsts, spans, order;
        std::vector<uint8_t> taken, superseded;
        for (int32_t u = 0; u < batch; ++u) {
            const std::vector<int32_t> &p = pending[u];
            const int64_t W = utt_off[u + 1] - utt_off[u];
            taken.assign(static_cast<size_t>(W), 0);
            if (occupied)
                for (int64_t i = 0; i < W; ++i) taken[i] = occupied[utt_off[u] + i] ? 1 : 0;
            sims.clear(); firsts.clear(); spans.clear();
            for (const int32_t c : p) { sims.push_back(cands[c].similarity); firsts.push_back(cands[c].first_word); spans.push_back(cands[c].span_len); }
            fa::vr::arbitrate(static_cast<int32_t>(p.size()), sims.data(), firsts.data(), spans.data(), taken.data(), order, superseded);
            for (const int32_t i : order) {
                verdicts[p[i]].outcome = FA_VR_APPLIED;
                if (applied) applied[at] = p[i];
                ++at;
            }
            if (applied_counts) applied_counts[u] = static_cast<int64_t>(order.size());
        }
        return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_vocab_rescore_default_config(fa_vr_decide_config *cfg) {
    if (!cfg) return;
    cfg->frame_duration = 0.08;
    cfg->margin_seconds = 0.10;   // defaultMarginSeconds
    cfg->cbw = 3.0f;              // defaultCbw
    cfg->blank_id = 1024;         // defaultBlankId
    cfg->boost = kDefaultBoost;
}

float fa_vocab_rescore_boost(float cbw, int32_t token_count, const fa_vr_boost_config *cfg) { return fa::vr::boost(cbw, token_count, cfg ? *cfg : kDefaultBoost); }

fa_status fa_vocab_rescore_build(const int32_t *char_counts, const float *min_similarities, const int64_t *term_rows, const int64_t *row_offsets, const int32_t *symbols,
                                 int32_t terms, int32_t min_term_length, int32_t *blob, int64_t capacity_words, int64_t *words_needed, char *text, int64_t text_capacity) {
    if (text && text_capacity > 0) text[0] = 0;
    return fa::no_throw(nullptr, "fa_vocab_rescore_build", [&]() {
        const fa::Verdict v = fa::vr::build(char_counts, min_similarities, term_rows, row_offsets, symbols, terms, min_term_length, blob, capacity_words, words_needed);
        if (v.status != FA_SUCCESS && text && text_capacity > 0) snprintf(text, static_cast<size_t>(text_capacity), "%s", v.text);
        return v.status;
    });
}

fa_status fa_vocab_rescore_candidates(fa_ctx *ctx, const int32_t *blob, int64_t blob_words, const int64_t *utterance_offsets, int32_t batch, const int64_t *word_offsets,
                                      const int32_t *word_symbols, const uint8_t *word_flags, float min_similarity, fa_vr_candidate *out, int64_t capacity,
                                      int64_t *count, int64_t *utterance_counts) {
    return candidates(ctx, blob, blob_words, utterance_offsets, batch, word_offsets, word_symbols, word_flags, min_similarity, out, capacity, count, utterance_counts);
}

fa_status fa_vocab_rescore_decide_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                                      const int32_t *valid_frames, const fa_vr_decide_config *cfg, const fa_vr_candidate *cands, int64_t n_candidates,
                                      const int64_t *utterance_offsets, const double *word_starts, const double *word_ends, int32_t terms, const int32_t *term_tokens,
                                      const int64_t *term_token_offsets, const int32_t *alt_tokens, const int64_t *alt_token_offsets, const int32_t *phrase_tokens,
                                      const int64_t *phrase_token_offsets, const uint8_t *occupied, fa_vr_verdict *verdicts, int32_t *applied, int64_t *applied_counts) {
    return decide(ctx, d_log_probs, true, batch, frames, vocab, row_stride, matrix_stride, valid_frames, cfg, cands, n_candidates, utterance_offsets, word_starts, word_ends,
                  terms, term_tokens, term_token_offsets, alt_tokens, alt_token_offsets, phrase_tokens, phrase_token_offsets, occupied, verdicts, applied, applied_counts);
}

fa_status fa_vocab_rescore_decide(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                                  const int32_t *valid_frames, const fa_vr_decide_config *cfg, const fa_vr_candidate *cands, int64_t n_candidates,
                                  const int64_t *utterance_offsets, const double *word_starts, const double *word_ends, int32_t terms, const int32_t *term_tokens,
                                  const int64_t *term_token_offsets, const int32_t *alt_tokens, const int64_t *alt_token_offsets, const int32_t *phrase_tokens,
                                  const int64_t *phrase_token_offsets, const uint8_t *occupied, fa_vr_verdict *verdicts, int32_t *applied, int64_t *applied_counts) {
    return decide(ctx, log_probs, false, batch, frames, vocab, row_stride, matrix_stride, valid_frames, cfg, cands, n_candidates, utterance_offsets, word_starts, word_ends,
                  terms, term_tokens, term_token_offsets, alt_tokens, alt_token_offsets, phrase_tokens, phrase_token_offsets, occupied, verdicts, applied, applied_counts);
}

}  // extern "C"
