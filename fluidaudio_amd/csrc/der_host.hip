// der_host.hip — the host side of the DER scorer (kernels: der.hip, argument pass and plan: der_geom.h, operands: der_launch.h): the
// staging of the segments and records, the launches, the call's one synchronisation, the copy-back and the C ABI.  Built with
// -ffp-contract=off like der.hip: the plan does the reference's fp64 arithmetic.
#include "der_launch.h"

namespace {

using namespace fa::der;

fa_status der_score(fa_ctx *ctx, const fa_der_config *cfg, const fa_der_segment *ref, const int64_t *ref_range, const fa_der_segment *hyp,
                    const int64_t *hyp_range, int32_t B, fa_der_counts *counts, int32_t *mapping, const int64_t *mapping_range, int64_t *overlap,
                    int64_t overlap_capacity) {
    if (!ctx || !cfg) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "der: ctx and config are required");
    return fa::no_throw(ctx, "der", [&]() -> fa_status {
    Plan plan;
    fa::Verdict v = make_plan(*cfg, ref, ref_range, hyp, hyp_range, B, counts, mapping, mapping_range, overlap, overlap_capacity, plan);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    if (B == 0) return FA_SUCCESS;
    const std::vector<DerRec> &rec = plan.rec;
    for (int32_t b = 0; b < B; ++b) {
        counts[b] = fa_der_counts{rec[b].num_frames, 0, 0, 0, 0, rec[b].R, rec[b].H};
        for (int64_t i = mapping_range[b]; i < mapping_range[b + 1]; ++i) mapping[i] = -1;
    }
    if (plan.plane_words == 0) return FA_SUCCESS;   // no recording has a label
    v = check_raster(plan);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "%s", v.text);
    const int64_t plane_words = plan.plane_words, ov_entries = plan.ov_entries, n_ref = plan.n_ref, n_hyp = plan.n_hyp;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_ref, b_hyp, b_rec, b_planes, b_work;
    // b_work: the overlap tables, the accumulators, then the mappings — what comes back to the host, in one buffer
    const size_t ov_bytes = sizeof(int64_t) * ov_entries, acc_bytes = sizeof(int64_t) * 4 * B, map_bytes = sizeof(int32_t) * kMaxLabels * static_cast<size_t>(B);
    FA_TRY(fa::take(ctx, "der", {{&b_ref, sizeof(fa_der_segment) * n_ref, true, ref + plan.r0}, {&b_hyp, sizeof(fa_der_segment) * n_hyp, true, hyp + plan.h0},
                                 {&b_rec, sizeof(DerRec) * B, true, rec.data()}, {&b_planes, sizeof(uint64_t) * plane_words},
                                 {&b_work, ov_bytes + acc_bytes + map_bytes}}));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_planes.p, 0, sizeof(uint64_t) * plane_words, st));
    FA_HIP_TRY(ctx, hipMemsetAsync(b_work.p, 0, ov_bytes + acc_bytes, st));   // der_assign writes every mapping entry it owns
    char *work = b_work.as<char>();
    DerArgs a{b_ref.as<fa_der_segment>(), b_hyp.as<fa_der_segment>(), b_rec.as<DerRec>(), b_planes.as<unsigned long long>(),
              reinterpret_cast<unsigned long long *>(work), reinterpret_cast<unsigned long long *>(work + ov_bytes),
              reinterpret_cast<int32_t *>(work + ov_bytes + acc_bytes), n_ref, n_hyp, B, cfg->frame_step, cfg->collar};
    launch_raster(st, a, plan);
    launch_overlap(st, a, plan);
    launch_assign(st, a);
    launch_accumulate(st, a, plan);
    FA_HIP_TRY(ctx, hipGetLastError());
    std::vector<int64_t> h_acc(static_cast<size_t>(4) * B);
    std::vector<int32_t> h_map(static_cast<size_t>(kMaxLabels) * B);
    if (overlap && ov_entries > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(overlap, work, ov_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(h_acc.data(), work + ov_bytes, acc_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipMemcpyAsync(h_map.data(), work + ov_bytes + acc_bytes, map_bytes, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    for (int32_t b = 0; b < B; ++b) {
        counts[b].miss = h_acc[4 * b + 0];
        counts[b].false_alarm = h_acc[4 * b + 1];
        counts[b].confusion = h_acc[4 * b + 2];
        counts[b].ref = h_acc[4 * b + 3];
        for (int32_t h = 0; h < rec[b].H; ++h) mapping[mapping_range[b] + h] = h_map[static_cast<size_t>(kMaxLabels) * b + h];
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_der_default_config(fa_der_config *cfg) {
    if (!cfg) return;
    cfg->frame_step = 0.01;   // DiarizationDER.compute's defaults (:55-56)
    cfg->collar = 0.0;
}

fa_status fa_der_score_batch(fa_ctx *ctx, const fa_der_config *cfg, const fa_der_segment *ref_segs, const int64_t *ref_range, const fa_der_segment *hyp_segs,
                             const int64_t *hyp_range, int32_t batch, fa_der_counts *counts, int32_t *mapping, const int64_t *mapping_range, int64_t *overlap,
                             int64_t overlap_capacity) {
    return der_score(ctx, cfg, ref_segs, ref_range, hyp_segs, hyp_range, batch, counts, mapping, mapping_range, overlap, overlap_capacity);
}

}  // extern "C"
