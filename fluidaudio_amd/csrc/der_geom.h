// der_geom.h — the argument pass and the plan of the DER scorer (kernels: der.hip, entries: der_host.hip): what a call's arguments
// decide before any device work — label counts, maxEnd, numFrames (DiarizationDER.swift:61-86), the word offsets of every recording's
// bit planes and overlap table, the raster's item and block counts.  Plain C++ without a HIP call and without a context, shared by the
// two units and by tests/cpu/der_geom.cpp, which walks it on the host.  A refusal comes back as a verdict: the status and the text
// der_host.hip hands to the context.  Internal; not part of the C ABI.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fa_verdict.h"

namespace fa {
namespace der {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxLabels = FA_DER_MAX_LABELS;
constexpr int kRasterLanes = 8;          // lanes that share one range in der_raster
constexpr int kOverlapTileWords = 256;   // words per workgroup of der_overlap: one 64-word chunk per wavefront
constexpr int kAccWordsPerWave = 8;      // consecutive words a wavefront of der_accumulate sums before it reduces
constexpr int kAccTileWords = kAccWordsPerWave * (kThreads / kWave);

static_assert(kMaxLabels == kWave, "der_assign gives every column a lane and der_accumulate keeps a label set in one 64-bit word");

struct DerRec {
    int64_t ref_begin, ref_end, hyp_begin, hyp_end;   // the recording's segments in the uploaded lists, which start at the first segment used
    int64_t plane_off;                                // first word of its planes: R ref planes, H hyp planes, the excluded plane
    int64_t ov_off;                                   // first entry of its [H][R] overlap table
    int32_t words, num_frames, R, H;
};

struct Plan {
    std::vector<DerRec> rec;        // [B]
    int64_t r0 = 0, h0 = 0;         // the first reference / hypothesis segment used: the uploads start there
    int64_t n_ref = 0, n_hyp = 0;   // segments uploaded
    int64_t plane_words = 0;        // 0: no recording has a label, every output is zero
    int64_t ov_entries = 0;
    int32_t max_words = 0;
    int64_t items = 0;              // of der_raster: the reference segments, the hypothesis segments, (collar > 0) two boundaries per reference segment
    int64_t raster_blocks = 0;
};

// The labels and times of recording b, and with them its geometry (:61-86).
inline Verdict recording_geometry(const fa_der_config &cfg, const fa_der_segment *ref, const int64_t *ref_range, const fa_der_segment *hyp,
                                  const int64_t *hyp_range, const int32_t b, Plan &plan) {
    DerRec &r = plan.rec[b];
    r = DerRec{ref_range[b], ref_range[b + 1], hyp_range[b], hyp_range[b + 1], plan.plane_words, plan.ov_entries, 0, 0, 0, 0};
    if (r.ref_begin < 0 || r.ref_end < r.ref_begin || r.hyp_begin < 0 || r.hyp_end < r.hyp_begin)
        return refuse(FA_INVALID_ARGUMENT, "der: the segment ranges of recording %d do not ascend", b);
    if ((r.ref_end > r.ref_begin && !ref) || (r.hyp_end > r.hyp_begin && !hyp)) return refuse(FA_INVALID_ARGUMENT, "der: segments are required");
    double max_end = 0.0;
    int32_t labels[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        const fa_der_segment *s = side ? hyp : ref;
        for (int64_t i = side ? r.hyp_begin : r.ref_begin, e = side ? r.hyp_end : r.ref_end; i < e; ++i) {
            if (!std::isfinite(s[i].start) || !std::isfinite(s[i].end))
                return refuse(FA_INVALID_ARGUMENT, "der: recording %d has a segment with a non-finite time", b);
            if (s[i].label < 0 || s[i].label >= kMaxLabels)
                return refuse(FA_INVALID_ARGUMENT, "der: recording %d has label %d; a side holds at most %d labels, numbered from 0", b, s[i].label, kMaxLabels);
            labels[side] = std::max(labels[side], s[i].label + 1);
            max_end = std::max(max_end, s[i].end);   // degenerate segments count too (:72, :79)
        }
    }
    r.R = labels[0];
    r.H = labels[1];
    if (r.R == 0 && r.H == 0) return Verdict{};   // :82-86: every output is zero
    const double frames = std::ceil(max_end / cfg.frame_step) + 1.0;
    if (!(frames < 2147483584.0)) return refuse(FA_INDEX_OVERFLOW, "der: recording %d has 2^31 frames or more", b);
    r.num_frames = static_cast<int32_t>(frames);
    r.words = (r.num_frames + 63) / 64;
    plan.plane_words += static_cast<int64_t>(r.words) * (r.R + r.H + 1);
    plan.ov_entries += static_cast<int64_t>(r.R) * r.H;
    return Verdict{};
}

// The argument pass of a call and its plan.  Nothing is written but `plan`; no device is touched.  The refusals come in this order: the
// config, the sizes and required pointers, then recording by recording its ranges, its missing segment arrays, segment by segment
// (reference side first) a non-finite time before a label out of range, and its frame count; then recording by recording its mapping
// range, the room in it and the missing mapping array; last the overlap capacity.  B == 0 leaves the plan empty.
inline Verdict make_plan(const fa_der_config &cfg, const fa_der_segment *ref, const int64_t *ref_range, const fa_der_segment *hyp, const int64_t *hyp_range,
                         const int32_t B, const void *counts, const void *mapping, const int64_t *mapping_range, const void *overlap,
                         const int64_t overlap_capacity, Plan &plan) {
    plan = Plan{};
    if (!(cfg.frame_step > 0.0) || !std::isfinite(cfg.frame_step) || !(cfg.collar >= 0.0) || !std::isfinite(cfg.collar))
        return refuse(FA_INVALID_ARGUMENT, "der: frame_step must be positive and finite, collar non-negative and finite");
    if (B < 0 || overlap_capacity < 0 || (B > 0 && (!ref_range || !hyp_range || !counts || !mapping_range))) return refuse(FA_INVALID_ARGUMENT, "der: bad arguments");
    if (B == 0) return Verdict{};
    plan.rec.resize(static_cast<size_t>(B));
    for (int32_t b = 0; b < B; ++b) {
        const Verdict v = recording_geometry(cfg, ref, ref_range, hyp, hyp_range, b, plan);
        if (v.status != FA_SUCCESS) return v;
    }
    for (int32_t b = 0; b < B; ++b) {
        const int64_t room = mapping_range[b + 1] - mapping_range[b];
        if (mapping_range[b] < 0 || room < 0) return refuse(FA_INVALID_ARGUMENT, "der: the mapping range of recording %d does not ascend", b);
        if (room < plan.rec[b].H)
            return refuse(FA_OUTPUT_TOO_SMALL, "der: recording %d has %d hypothesis labels, its mapping range holds %lld", b, plan.rec[b].H, (long long)room);
        if (room > 0 && !mapping) return refuse(FA_INVALID_ARGUMENT, "der: mapping is required");
        plan.max_words = std::max(plan.max_words, plan.rec[b].words);
    }
    if (overlap && overlap_capacity < plan.ov_entries)
        return refuse(FA_OUTPUT_TOO_SMALL, "der: the overlap tables take %lld entries, the output holds %lld", (long long)plan.ov_entries, (long long)overlap_capacity);
    plan.r0 = ref_range[0];
    plan.h0 = hyp_range[0];
    plan.n_ref = ref_range[B] - plan.r0;
    plan.n_hyp = hyp_range[B] - plan.h0;
    for (DerRec &r : plan.rec) { r.ref_begin -= plan.r0; r.ref_end -= plan.r0; r.hyp_begin -= plan.h0; r.hyp_end -= plan.h0; }
    plan.items = plan.n_ref + plan.n_hyp + (cfg.collar > 0.0 ? 2 * plan.n_ref : 0);
    plan.raster_blocks = (plan.items * kRasterLanes + kThreads - 1) / kThreads;
    return Verdict{};
}

// der_raster's grid is one dimension of workgroups.  Asked once the outputs are initialised and only of a call that has planes, as the
// entry always has.
inline Verdict check_raster(const Plan &plan) {
    if (plan.raster_blocks >= INT32_MAX) return refuse(FA_INDEX_OVERFLOW, "der: %lld segments", (long long)plan.items);
    return Verdict{};
}

}  // namespace der
}  // namespace fa
