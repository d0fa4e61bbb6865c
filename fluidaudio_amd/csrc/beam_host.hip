// beam_host.hip — host side of CTC prefix beam search (kernels and their launchers: beam.hip; shared: beam_launch.h): the ARPA reader
// (ARPALanguageModel, reference: Sources/FluidAudio/ASR/Parakeet/SlidingWindow/CTC/ARPALanguageModel.swift:16-147), the builder of the model's
// hash tables and their upload, the vocabulary's word-hash steps, the launch plan of a search, and the C ABI.  No kernel lives here.
// Built with -ffp-contract=off like beam.hip: fa_arpa_score is the float arithmetic of the walk and of the restatement, bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "beam_launch.h"
#include "text_util.h"

using namespace fa::beam;

struct fa_arpa_lm {
    fa_ctx *ctx = nullptr;
    std::vector<UniEntry> uni;
    std::vector<BiEntry> bi;
    int64_t n_uni = 0, n_bi_ctx = 0, n_bi = 0;
    void *d_uni = nullptr, *d_bi = nullptr;
    int dev_id = -1;   // device holding d_uni / d_bi
    LmView host_view() const { return LmView{uni.empty() ? nullptr : uni.data(), bi.empty() ? nullptr : bi.data(), static_cast<uint32_t>(uni.size() - 1), static_cast<uint32_t>(bi.size() - 1)}; }
    LmView dev_view() const { return LmView{static_cast<const UniEntry *>(d_uni), static_cast<const BiEntry *>(d_bi), static_cast<uint32_t>(uni.size() - 1), static_cast<uint32_t>(bi.size() - 1)}; }
};

struct fa_ctc_vocab {
    fa_ctx *ctx = nullptr;
    int32_t vocab_size = 0;
    void *d_tok = nullptr;
};

namespace {

inline uint32_t pow2_at_least(size_t n) { uint32_t c = 16; while (c < n) c <<= 1; return c; }

// ---- the ARPA text: what the reference's reader keeps of it, in the order of first appearance (a repeated entry overwrites)
struct ArpaText {
    struct Uni { std::string w; float p, b; };
    struct Bi { std::string c, w; float p; };
    std::vector<Uni> us;
    std::vector<Bi> bs;
    size_t contexts = 0;   // distinct first words of the bigrams
};

ArpaText read_arpa(const char *text, const int64_t len) {
    const float log10_to_nat = static_cast<float>(std::log(10.0));           // ARPALanguageModel.log10ToNat (:30)
    ArpaText a;
    std::unordered_map<std::string, size_t> uidx, bidx;
    std::unordered_map<std::string, int> contexts;
    std::string section;
    for (int64_t pos = 0; pos <= len;) {
        int64_t e = pos;
        while (e < len && text[e] != '\n') ++e;                                              // the reader cuts at the byte \n only (:126)
        const char *la = text + pos, *lb = text + e;
        pos = e + 1;
        fa_text::trim(la, lb, fa_text::ws_or_nl_len);                                        // trimmingCharacters(in: .whitespacesAndNewlines) (:131)
        const std::string line(la, lb);
        if (line.empty() || line.rfind("\\data\\", 0) == 0) continue;                       // :54
        if (line == "\\end\\") break;                                                       // :55
        if (line[0] == '\\') { section = line; continue; }                                  // :56-59
        if (line.rfind("ngram ", 0) == 0) continue;                                         // :61
        std::vector<std::string> parts;
        for (size_t i = 0;;) { const size_t j = line.find('\t', i); parts.emplace_back(line.substr(i, j == std::string::npos ? j : j - i)); if (j == std::string::npos) break; i = j + 1; }
        float l10;
        if (!fa_text::parse_float(parts[0], l10)) continue;                                 // Swift's Float(String); malformed line skipped (:64-67)
        const float prob = l10 * log10_to_nat;
        auto backoff = [&](size_t i) { float v; return parts.size() > i ? (fa_text::parse_float(parts[i], v) ? v : 0.0f) * log10_to_nat : 0.0f; };
        if (section == "\\1-grams:" && parts.size() >= 2) {
            const float bo = backoff(2);
            auto it = uidx.find(parts[1]);
            if (it == uidx.end()) { uidx[parts[1]] = a.us.size(); a.us.push_back({parts[1], prob, bo}); } else { a.us[it->second].p = prob; a.us[it->second].b = bo; }
        } else if (section == "\\2-grams:" && parts.size() >= 3) {
            const std::string key = parts[1] + '\t' + parts[2];
            auto it = bidx.find(key);
            if (it == bidx.end()) { bidx[key] = a.bs.size(); a.bs.push_back({parts[1], parts[2], prob}); } else a.bs[it->second].p = prob;
            contexts[parts[1]] = 1;
        }
    }
    a.contexts = contexts.size();
    return a;
}

// open addressing, linear probing, at most half full: the first slots are uni_slot / bi_slot, which the probers (uni_find, bi_find) start from too
void build_tables(const ArpaText &a, fa_arpa_lm &lm) {
    lm.n_uni = static_cast<int64_t>(a.us.size()); lm.n_bi = static_cast<int64_t>(a.bs.size()); lm.n_bi_ctx = static_cast<int64_t>(a.contexts);
    lm.uni.assign(pow2_at_least(2 * a.us.size() + 1), UniEntry{0, 0, 0.f, 0.f, 0});
    lm.bi.assign(pow2_at_least(2 * a.bs.size() + 1), BiEntry{0, 0, 0, 0, 0.f, 0});
    const uint32_t um = static_cast<uint32_t>(lm.uni.size() - 1), bm = static_cast<uint32_t>(lm.bi.size() - 1);
    for (const ArpaText::Uni &x : a.us) {
        uint64_t h, m; hash_bytes(x.w.data(), x.w.size(), h, m);
        const int32_t l = static_cast<int32_t>(x.w.size());
        uint32_t s = uni_slot(h, l, um);
        while (lm.uni[s].used) s = (s + 1) & um;
        lm.uni[s] = UniEntry{h, l, x.p, x.b, 1};
    }
    for (const ArpaText::Bi &x : a.bs) {
        uint64_t hp, hw, m; hash_bytes(x.c.data(), x.c.size(), hp, m); hash_bytes(x.w.data(), x.w.size(), hw, m);
        const int32_t lp = static_cast<int32_t>(x.c.size()), lw = static_cast<int32_t>(x.w.size());
        uint32_t s = bi_slot(hp, lp, hw, lw, bm);
        while (lm.bi[s].used) s = (s + 1) & bm;
        lm.bi[s] = BiEntry{hp, hw, lp, lw, x.p, 1};
    }
}

// The model's tables on the context's device (the caller holds that device's guard): uploaded at the first search there, all or nothing; tables
// the model holds on another device are released there first.
fa_status lm_tables_on(fa_ctx *ctx, fa_arpa_lm *lm) {
    if (lm->d_uni && lm->dev_id == ctx->device) return FA_SUCCESS;
    if (lm->d_uni || lm->d_bi) {
        fa::DeviceGuard other(lm->dev_id);
        (void)hipDeviceSynchronize();
        (void)hipFree(lm->d_uni); (void)hipFree(lm->d_bi);
        lm->d_uni = nullptr; lm->d_bi = nullptr;
    }
    void *du = nullptr, *db = nullptr;
    hipError_t e = hipMalloc(&du, sizeof(UniEntry) * lm->uni.size());
    if (e == hipSuccess) e = hipMalloc(&db, sizeof(BiEntry) * lm->bi.size());
    if (e == hipSuccess) e = hipMemcpy(du, lm->uni.data(), sizeof(UniEntry) * lm->uni.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db, lm->bi.data(), sizeof(BiEntry) * lm->bi.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(du); (void)hipFree(db); return fa::hip_status(ctx, e, "arpa table upload"); }
    lm->d_uni = du; lm->d_bi = db;
    lm->ctx = ctx; lm->dev_id = ctx->device;
    return FA_SUCCESS;
}

struct VocabDelete { void operator()(fa_ctc_vocab *v) const { fa_ctc_vocab_destroy(v); } };   // the half-built vocabulary may own device memory

// ---- what a search of these shapes launches.  One prefix trie per utterance in flight — a hash table of `stride` slots, twice the
// frames x beam_width nodes a walk can create — and at most ~2 GiB of them at a time: longer batches are walked in pieces.
struct BeamPlan {
    int64_t stride, per;   // trie slots of an utterance, their bytes
    int chunk;             // utterances per launch
    int64_t launches;
    int ntop;              // top tokens a frame offers: min(token_candidates, tokens of the vocabulary other than the blank)
};

// false: beam width or token candidates outside the supported range.  batch, frames >= 0 and vocab >= 1 are the caller's to check.
bool beam_plan(const int32_t batch, const int32_t frames, const int32_t vocab, const int32_t beam_width, const int32_t blank_id, const int32_t token_candidates,
               BeamPlan &p) {
    if (beam_width < 1 || beam_width > kMaxBeam || token_candidates < 0 || token_candidates > kMaxTop) return false;
    p.stride = pow2_at_least(static_cast<size_t>(2) * frames * beam_width + 2);
    p.per = p.stride * static_cast<int64_t>(sizeof(unsigned long long));
    p.chunk = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(batch, (int64_t(2) << 30) / std::max<int64_t>(p.per, 1))));
    p.launches = batch > 0 ? (static_cast<int64_t>(batch) + p.chunk - 1) / p.chunk : 0;
    p.ntop = std::min(token_candidates, vocab - (blank_id >= 0 && blank_id < vocab ? 1 : 0));
    return true;
}

}  // namespace

extern "C" {

fa_status fa_arpa_parse(fa_ctx *ctx, const char *text, int64_t len, fa_arpa_lm **out) {
    if (!out || (!text && len > 0) || len < 0) return FA_INVALID_ARGUMENT;   // ctx may be NULL: parsing and scoring are host code
    *out = nullptr;
    return fa::no_throw(ctx, "arpa", [&]() -> fa_status {
        std::unique_ptr<fa_arpa_lm> lm(new fa_arpa_lm());   // no device memory before the first search
        lm->ctx = ctx;
        build_tables(read_arpa(text, len), *lm);
        *out = lm.release();
        return FA_SUCCESS;
    });
}

void fa_arpa_destroy(fa_arpa_lm *lm) {
    if (!lm) return;
    if (lm->d_uni || lm->d_bi) { fa::DeviceGuard guard(lm->dev_id); (void)hipFree(lm->d_uni); (void)hipFree(lm->d_bi); }
    delete lm;
}

int64_t fa_arpa_unigram_count(const fa_arpa_lm *lm) { return lm ? lm->n_uni : 0; }
int64_t fa_arpa_bigram_context_count(const fa_arpa_lm *lm) { return lm ? lm->n_bi_ctx : 0; }

fa_status fa_arpa_score(const fa_arpa_lm *lm, const char *word, const char *prev, float *out) {
    if (!lm || !word || !out) return FA_INVALID_ARGUMENT;
    uint64_t hw, hp = 0, m;
    hash_bytes(word, strlen(word), hw, m);
    if (prev) hash_bytes(prev, strlen(prev), hp, m);
    *out = lm_score(lm->host_view(), hw, static_cast<int32_t>(strlen(word)), hp, prev ? static_cast<int32_t>(strlen(prev)) : -1);
    return FA_SUCCESS;
}

fa_status fa_ctc_vocab_create(fa_ctx *ctx, const int32_t *ids, const char *const *pieces, int32_t n, int32_t vocab_size, fa_ctc_vocab **out) {
    if (!ctx || !out || n < 0 || vocab_size < 1 || (n > 0 && (!ids || !pieces))) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    return fa::no_throw(ctx, "ctc vocab", [&]() -> fa_status {
        std::vector<TokInfo> tok(vocab_size, TokInfo{1, 0, 0, 0});                        // missing id: vocabulary[v] ?? "" (:181)
        static const char kBoundary[] = "\xe2\x96\x81";                                   // U+2581, ASRConstants.sentencePieceWordBoundary
        for (int32_t i = 0; i < n; ++i) {
            if (ids[i] < 0 || ids[i] >= vocab_size || !pieces[i]) continue;
            const char *p = pieces[i];
            size_t len = strlen(p);
            TokInfo t{1, 0, 0, 0};
            if (len >= 3 && memcmp(p, kBoundary, 3) == 0) { t.boundary = 1; p += 3; len -= 3; }   // hasPrefix + dropFirst (:184,:192)
            hash_bytes(p, len, t.add, t.mult);
            t.len = static_cast<int32_t>(len);
            tok[ids[i]] = t;
        }
        fa::DeviceGuard guard(ctx->device);
        std::unique_ptr<fa_ctc_vocab, VocabDelete> v(new (std::nothrow) fa_ctc_vocab());
        if (!v) return FA_ALLOCATION_FAILURE;
        v->ctx = ctx; v->vocab_size = vocab_size;
        hipError_t e = hipMalloc(&v->d_tok, sizeof(TokInfo) * vocab_size);
        if (e == hipSuccess) e = hipMemcpy(v->d_tok, tok.data(), sizeof(TokInfo) * vocab_size, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fa::hip_status(ctx, e, "ctc vocab upload");
        *out = v.release();
        return FA_SUCCESS;
    });
}

void fa_ctc_vocab_destroy(fa_ctc_vocab *v) {
    if (!v) return;
    if (v->d_tok) { fa::DeviceGuard guard(v->ctx->device); (void)hipFree(v->d_tok); }
    delete v;
}

fa_status fa_ctc_beam_search_batch_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride,
                                       int64_t matrix_stride, const int32_t *d_valid_frames, const fa_ctc_vocab *vocabulary, fa_arpa_lm *lm,
                                       int32_t beam_width, float lm_weight, float word_bonus, int32_t blank_id, int32_t token_candidates,
                                       int32_t *d_tokens, int32_t *d_lens, float *d_scores) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0) return FA_SUCCESS;
    if (batch < 0 || frames < 0 || vocab < 1 || !d_tokens || !d_lens || (frames > 0 && !d_log_probs))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "beam search: bad arguments");
    BeamPlan plan;
    if (!beam_plan(batch, frames, vocab, beam_width, blank_id, token_candidates, plan))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "beam search: beam width 1..%d, token candidates 0..%d", kMaxBeam, kMaxTop);
    if (lm && (!vocabulary || vocabulary->vocab_size < vocab)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "beam search: the language model needs a vocabulary covering all tokens");
    if (row_stride < vocab) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "beam search: row stride < vocab");
    fa::DeviceGuard guard(ctx->device);
    if (lm) FA_TRY(lm_tables_on(ctx, lm));
    BeamArgs a{};
    a.logp = d_log_probs; a.valid = d_valid_frames; a.tok = vocabulary ? static_cast<const TokInfo *>(vocabulary->d_tok) : nullptr;
    if (lm) a.lm = lm->dev_view();
    a.tokens = d_tokens; a.lens = d_lens; a.scores = d_scores;
    a.row_stride = row_stride; a.matrix_stride = matrix_stride; a.arena_stride = plan.stride;
    a.frames = frames; a.vocab = vocab; a.blank = blank_id; a.beam_width = beam_width; a.top_k = token_candidates;
    a.use_lm = lm != nullptr; a.lm_weight = lm_weight; a.word_bonus = word_bonus;
    // d_arena: the tries of one launch; d_top: the pre-pass' table of one launch, K (token, log-prob) pairs + the blank's log-prob per frame.
    // From the context's buffer cache: a second call pays no hipMalloc
    fa::DevBuf d_arena, d_top;
    const size_t rows_max = static_cast<size_t>(plan.chunk) * std::max(frames, 1);
    FA_TRY(fa::take(ctx, "beam search", {{&d_arena, static_cast<size_t>(plan.per) * plan.chunk}, {&d_top, sizeof(TopEntry) * rows_max * (token_candidates + 1)}}));
    a.arena = d_arena.as<unsigned long long>();
    a.top = d_top.as<TopEntry>();
    TopArgs ta{};
    ta.logp = d_log_probs; ta.valid = d_valid_frames; ta.tok = a.tok; ta.top = d_top.as<TopEntry>();
    ta.row_stride = row_stride; ta.matrix_stride = matrix_stride; ta.frames = frames; ta.vocab = vocab; ta.blank = blank_id;
    ta.top_k = token_candidates; ta.use_lm = a.use_lm;
    fa::DeviceTiming tim{ctx};   // device work of the call: behind the allocations
    FA_TRY(tim.begin());
    for (int first = 0; first < batch; first += plan.chunk) {
        const int now = std::min(plan.chunk, batch - first);
        a.first = first;
        FA_HIP_TRY(ctx, hipMemsetAsync(d_arena.p, 0xff, static_cast<size_t>(plan.per) * now, ctx->stream));
        if (frames > 0) {
            ta.first = first; ta.rows = static_cast<int64_t>(now) * frames;
            launch_top(ctx->stream, ta);
            FA_HIP_TRY(ctx, hipGetLastError());
        }
        launch_walk(ctx->stream, a, now, plan.ntop);
        FA_HIP_TRY(ctx, hipGetLastError());
    }
    FA_TRY(tim.end());
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the arena and the tables go back to the context's cache on return
    FA_TRY(tim.read());
    return FA_SUCCESS;
}

// What a call of these shapes launches (bench.py prints it next to its timing): out = { trie slots per utterance (arena_stride), utterances
// per launch (the ~2 GiB arena cap), launches, extension keys per thread of the ctc_beam_kernel instance the walk launcher picks }.
fa_status fa_ctc_beam_plan(int32_t batch, int32_t frames, int32_t vocab, int32_t beam_width, int32_t blank_id, int32_t token_candidates, int64_t out[4]) {
    BeamPlan plan;
    if (!out || batch < 0 || frames < 0 || vocab < 1 || !beam_plan(batch, frames, vocab, beam_width, blank_id, token_candidates, plan)) return FA_INVALID_ARGUMENT;
    out[0] = plan.stride; out[1] = plan.chunk; out[2] = plan.launches; out[3] = walk_keys(plan.ntop);
    return FA_SUCCESS;
}

fa_status fa_ctc_beam_search_batch(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab, const int32_t *valid_frames,
                                   const fa_ctc_vocab *vocabulary, fa_arpa_lm *lm, int32_t beam_width, float lm_weight, float word_bonus,
                                   int32_t blank_id, int32_t token_candidates, int32_t *tokens, int32_t *lens, float *scores) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (batch == 0) return FA_SUCCESS;
    if (batch < 0 || frames < 0 || vocab < 1 || !tokens || !lens || (frames > 0 && !log_probs)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "beam search: bad arguments");
    fa::DeviceGuard guard(ctx->device);
    const size_t n = static_cast<size_t>(batch) * frames * vocab;
    fa::DevBuf d_lp, d_valid, d_tok, d_len, d_sc;
    FA_TRY(fa::take_once(ctx, "beam search", {{&d_lp, sizeof(float) * n, true, log_probs}, {&d_tok, sizeof(int32_t) * static_cast<size_t>(batch) * std::max(frames, 1)},
                                              {&d_len, sizeof(int32_t) * batch}, {&d_sc, sizeof(float) * batch},
                                              {&d_valid, sizeof(int32_t) * batch, valid_frames != nullptr, valid_frames}}));
    FA_TRY(fa_ctc_beam_search_batch_dev(ctx, d_lp.as<float>(), batch, frames, vocab, vocab, static_cast<int64_t>(frames) * vocab,
                                        valid_frames ? d_valid.as<int32_t>() : nullptr, vocabulary, lm, beam_width, lm_weight, word_bonus, blank_id,
                                        token_candidates, d_tok.as<int32_t>(), d_len.as<int32_t>(), d_sc.as<float>()));
    if (frames > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(tokens, d_tok.p, sizeof(int32_t) * static_cast<size_t>(batch) * frames, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(lens, d_len.p, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, ctx->stream));
    if (scores) FA_HIP_TRY(ctx, hipMemcpyAsync(scores, d_sc.p, sizeof(float) * batch, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

}  // extern "C"
