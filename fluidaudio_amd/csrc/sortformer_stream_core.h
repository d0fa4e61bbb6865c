// sortformer_stream_core.h — the integers of streaming Sortformer that the host entries, the kernels and the tests share
// (reference: Sources/FluidAudio/Diarizer/Sortformer/SortformerStateUpdater.swift:43-164, 220-232, SortformerDiarizer.swift:933-979,
// SortformerTypes.swift:239-254, 347-383): the config's clamps, the pop-out length, the per-speaker quotas with the reference's
// Int(Float(x) * rate) truncation, the slab sizes, one update's validation and plan, and the two chunk plans.  Plain C++: it compiles on
// the host alone (tests/cpu/sortformer_stream_core_main.cpp runs it under the sanitizers) and inside the kernels.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FA_SFS_HD __host__ __device__
#else
#define FA_SFS_HD
#endif

namespace fa {
namespace sfs {

constexpr int kMaxSpeakers = 4;            // as the stitch entry
constexpr uint32_t kLn2Bits = 0x3F317218u; // logf(2) as the reference's fp32 literal; -logf(0.5) is the same bits

// fa_sortformer_stream_config, field for field (sortformer_stream_host.hip asserts the sizes).
struct Config {
    int32_t speakers, d_model, chunk_len, chunk_left_context, chunk_right_context, fifo_len, spkcache_len, spkcache_update_period;
    int32_t sil_frames_per_spk, max_index, max_chunk_frames, subsampling, n_mels, reserved;
    float silence_threshold, pred_score_threshold, scores_boost_latest, strong_boost_rate, weak_boost_rate, min_pos_scores_rate;
};

// per-stream status of one update
enum Status : int32_t {
    kOk = 0, kInactive = 1, kShortPredsFifo = 2, kShortChunk = 3, kShortPredsChunk = 4, kShortPredsTentative = 5, kNegativeCore = 6, kBadPred = 7,
    kBadOperand = 8
};
// what an accepted update does to the rows
enum Mode : int32_t { kSkip = 0, kAppend = 1, kPop = 2, kCompress = 3 };

FA_SFS_HD inline int32_t imin(const int32_t a, const int32_t b) { return a < b ? a : b; }
FA_SFS_HD inline int32_t imax(const int32_t a, const int32_t b) { return a > b ? a : b; }

// SortformerConfig.init's clamps (:239, :253-254)
FA_SFS_HD inline void clamp(Config &c) {
    c.chunk_len = imax(1, c.chunk_len);
    const int64_t least = (1 + static_cast<int64_t>(c.sil_frames_per_spk)) * c.speakers;
    if (c.spkcache_len < least && least <= INT32_MAX) c.spkcache_len = static_cast<int32_t>(least);
    const int64_t room = static_cast<int64_t>(c.fifo_len) + c.chunk_len;
    const int64_t period = c.spkcache_update_period < room ? c.spkcache_update_period : room;
    c.spkcache_update_period = static_cast<int32_t>(period > c.chunk_len ? period : c.chunk_len);
}

// :119-121
FA_SFS_HD inline int32_t pop_out_length(const int32_t period, const int32_t context, const int32_t fifo_len) {
    return imin(imax(period, context - fifo_len), context);
}

// Int(Float(x) * rate): the product in fp32, truncated towards zero (rates are validated to be finite, >= 0 and small)
FA_SFS_HD inline int32_t quota(const int32_t x, const float rate) { return static_cast<int32_t>(static_cast<float>(x) * rate); }

struct Quotas {
    int32_t len_per_spk, strong, weak, min_pos;
};
FA_SFS_HD inline Quotas quotas(const Config &c) {   // :229-232
    Quotas q;
    q.len_per_spk = c.spkcache_len / c.speakers - c.sil_frames_per_spk;
    q.strong = quota(q.len_per_spk, c.strong_boost_rate);
    q.weak = quota(q.len_per_spk, c.weak_boost_rate);
    q.min_pos = quota(q.len_per_spk, c.min_pos_scores_rate);
    return q;
}

// The slab sizes.  A pop takes at most max_pop rows: pop <= max(period, context - fifo_len) and context - fifo_len <= the core rows.
struct Slabs {
    int32_t max_pop;        // rows one pop can take
    int32_t score_rows;     // spkcache_len + max_pop: the rows a compression scores, the row stride of d_log_scores and of the cache's preds
    int32_t fifo_pred_rows; // fifo_len + max_chunk_frames: the FIFO's preds before the pop
    int32_t keys;           // (score_rows + sil) * speakers: the keys of the global selection
    int64_t lds_bytes;      // what the control kernel keeps in LDS
};
FA_SFS_HD inline Slabs slabs(const Config &c) {
    Slabs s;
    s.max_pop = imin(imax(c.spkcache_update_period, c.max_chunk_frames), c.fifo_len + c.max_chunk_frames);
    s.score_rows = c.spkcache_len + s.max_pop;
    s.fifo_pred_rows = c.fifo_len + c.max_chunk_frames;
    s.keys = (s.score_rows + c.sil_frames_per_spk) * c.speakers;
    // preds and scores of the scored rows, the FIFO's preds, the keys, the flags of the selection, 256 partial counts
    s.lds_bytes = 8ll * s.score_rows * c.speakers + 4ll * s.fifo_pred_rows * c.speakers + 8ll * s.keys + 4ll * s.keys + 4ll * 256;
    return s;
}

// Why a config is refused (0: it is sound).  After clamp().
FA_SFS_HD inline int32_t config_fault(const Config &c) {
    const auto rate_ok = [](const float r) { return r >= 0.0f && r <= 1024.0f; };   // NaN fails both
    if (c.speakers < 1 || c.speakers > kMaxSpeakers) return 1;
    if (c.d_model < 4 || c.d_model % 4 != 0 || c.d_model > 8192) return 2;
    if (c.chunk_left_context < 0 || c.chunk_right_context < 0 || c.fifo_len < 0 || c.sil_frames_per_spk < 0 || c.max_chunk_frames < 1 || c.subsampling < 1 ||
        c.n_mels < 1)
        return 3;
    if (c.spkcache_len > (1 << 20) || c.fifo_len > (1 << 20) || c.max_chunk_frames > (1 << 20) || c.chunk_len > (1 << 20) || c.sil_frames_per_spk > (1 << 20) ||
        c.chunk_left_context > (1 << 20) || c.chunk_right_context > (1 << 20))
        return 4;
    if (!rate_ok(c.strong_boost_rate) || !rate_ok(c.weak_boost_rate) || !rate_ok(c.min_pos_scores_rate)) return 5;
    if (!(c.pred_score_threshold > 0.0f && c.pred_score_threshold < 1.0f) || !(c.silence_threshold == c.silence_threshold) ||
        !(c.scores_boost_latest > -3.0e38f && c.scores_boost_latest < 3.0e38f))
        return 6;
    if (c.max_index < 1) return 7;
    // a live permuted index must stay below the sentinel: the reference would mistake it for a disabled slot
    const Slabs s = slabs(c);
    if (static_cast<int64_t>(c.speakers) * (static_cast<int64_t>(c.spkcache_len) + s.max_pop + c.sil_frames_per_spk) >= c.max_index) return 8;
    if (s.lds_bytes > 60 * 1024) return 9;
    return 0;
}

// One update's integers (:43-161): validated in the reference's order, then planned.  pred_rows = preds.count / speakers.
struct Plan {
    int32_t status, mode;
    int32_t core, lc, rc;
    int32_t old_fifo, old_spk;     // the lengths the update found
    int32_t pop, new_fifo, new_spk;
    int32_t first_overflow;        // the cache's preds are initialised from this call's preds
    int32_t chunk_start;           // the first confirmed row of preds
    int32_t sil_before;            // silenceFrameCount before the pop (the control kernel fills it in)
};
FA_SFS_HD inline Plan plan_update(const Config &c, const int32_t spk_len, const int32_t fifo_length, const int32_t preds_present, const int32_t emb_len,
                                  const int32_t pred_rows, const int32_t pred_stride, const int32_t lc, const int32_t rc) {
    Plan p{};
    p.old_fifo = fifo_length; p.old_spk = spk_len; p.new_fifo = fifo_length; p.new_spk = spk_len; p.lc = lc; p.rc = rc;
    p.status = kOk; p.mode = kSkip;
    if (emb_len < 0 || emb_len > c.max_chunk_frames || pred_rows < 0 || pred_rows > pred_stride || lc < 0) { p.status = kBadOperand; return p; }
    if (fifo_length > 0 && spk_len + fifo_length > pred_rows) { p.status = kShortPredsFifo; return p; }   // :47-53
    if (rc < 0) { p.status = kShortChunk; return p; }                                                   // :62-70: embsEndIdx <= chunk.count is rc >= 0
    p.core = emb_len - lc - rc;
    if (p.core < 0) { p.status = kNegativeCore; return p; }
    p.chunk_start = spk_len + fifo_length + lc;
    const int64_t chunk_end = static_cast<int64_t>(p.chunk_start) + p.core;
    if (chunk_end + rc > pred_rows) { p.status = chunk_end > pred_rows ? kShortPredsChunk : kShortPredsTentative; return p; }   // :84-92
    const int32_t context = p.core + fifo_length;
    p.new_fifo = context;
    p.mode = kAppend;
    if (context > c.fifo_len) {
        p.pop = pop_out_length(c.spkcache_update_period, context, c.fifo_len);
        p.new_fifo = context - p.pop;
        p.new_spk = spk_len + p.pop;
        p.mode = kPop;
        if (p.new_spk > c.spkcache_len) {
            p.first_overflow = preds_present ? 0 : 1;
            p.new_spk = c.spkcache_len;
            p.mode = kCompress;
        }
    }
    return p;
}

// getNextChunkFeaturesLocked (SortformerDiarizer.swift:933-979) and SortformerFeatureLoader.next (SortformerTypes.swift:362-384); fa_sortformer_chunk
struct Chunk {
    int32_t ready, chunk_length, left_offset, right_offset;
    int64_t start_frame, rows, new_start_feat, frames_to_drop;
};
FA_SFS_HD inline int64_t lmin(const int64_t a, const int64_t b) { return a < b ? a : b; }
FA_SFS_HD inline int64_t lmax(const int64_t a, const int64_t b) { return a > b ? a : b; }

// feat_length: frames in the stream's buffer; start_feat: where the next core begins in it
FA_SFS_HD inline Chunk stream_chunk(const Config &c, const int64_t feat_length, const int64_t start_feat) {
    Chunk k{};
    k.new_start_feat = start_feat;
    const int64_t core = static_cast<int64_t>(c.chunk_len) * c.subsampling, lcf = static_cast<int64_t>(c.chunk_left_context) * c.subsampling,
                  rcf = static_cast<int64_t>(c.chunk_right_context) * c.subsampling;
    const int64_t end_feat = lmin(start_feat + core, feat_length);
    if (!(end_feat > start_feat) || !(end_feat + rcf <= feat_length)) return k;
    const int64_t left = lmin(lcf, start_feat);
    k.ready = 1;
    k.left_offset = static_cast<int32_t>(left);
    k.right_offset = static_cast<int32_t>(rcf);
    k.start_frame = start_feat - left;
    k.rows = end_feat + rcf - k.start_frame;
    k.chunk_length = static_cast<int32_t>(k.rows);
    k.frames_to_drop = lmax(0, end_feat - lcf);
    k.new_start_feat = end_feat - k.frames_to_drop;
    return k;
}

// the loader's next(): feat_length frames in the file, feat_seq_length the mel's valid length; start_feat advances to new_start_feat
FA_SFS_HD inline Chunk file_chunk(const Config &c, const int64_t feat_length, const int64_t feat_seq_length, const int64_t start_feat) {
    Chunk k = stream_chunk(c, feat_length, start_feat);
    if (!k.ready) return k;
    k.chunk_length = static_cast<int32_t>(lmax(lmin(feat_seq_length - start_feat + k.left_offset, k.rows), 0));
    k.new_start_feat = start_feat + (k.rows - k.left_offset - k.right_offset);   // endFeat: the loader drops nothing
    k.frames_to_drop = 0;
    return k;
}
FA_SFS_HD inline int64_t file_num_chunks(const Config &c, const int64_t feat_length) {   // :359
    const int64_t core = static_cast<int64_t>(c.chunk_len) * c.subsampling, rcf = static_cast<int64_t>(c.chunk_right_context) * c.subsampling;
    return lmax(0, (feat_length - rcf) / core);
}

}  // namespace sfs
}  // namespace fa
