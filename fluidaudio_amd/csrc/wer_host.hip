// wer_host.hip — the host side of the batched edit distance (kernel: wer.hip, plan: wer_launch.h): the argument pass, the uploads of the
// host-pointer entry, the launches by class, the one synchronisation of a call and the C ABI.
#include "fa_common.h"
#include "wer_launch.h"

namespace {

using fa::wer::Job;
using fa::wer::WalkArgs;

fa_status edit_distance(fa_ctx *ctx, const int32_t *hyp, const int64_t *hyp_range, const int32_t *ref, const int64_t *ref_range, const int64_t n_pairs,
                        fa_edit_counts *out, const bool device) {
    if (n_pairs < 0 || (n_pairs > 0 && (!hyp_range || !ref_range || !out))) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "edit_distance: bad arguments");
    if (n_pairs >= INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "edit_distance: 2^31 - 1 pairs or more");
    if (n_pairs > 0) {
        const fa::wer::Verdict v = fa::wer::check_ranges(hyp, hyp_range, ref, ref_range, n_pairs);
        if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "edit_distance: %s (pair %lld)", v.what, (long long)v.pair);
    }
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n_pairs == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "edit_distance", [&]() -> fa_status {
    // the host-pointer entry uploads from the first symbol used on
    const int64_t h0 = device ? 0 : hyp_range[0], r0 = device ? 0 : ref_range[0];
    fa::wer::Plan plan;
    fa::wer::make_plan(hyp_range, ref_range, n_pairs, h0, r0, out, plan);
    const size_t J = plan.jobs.size();
    if (J == 0) return FA_SUCCESS;   // every pair has an empty side

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_hyp, b_ref, b_jobs, b_out, b_ws;
    const size_t hyp_bytes = device ? 0 : sizeof(int32_t) * static_cast<size_t>(hyp_range[n_pairs] - h0);
    const size_t ref_bytes = device ? 0 : sizeof(int32_t) * static_cast<size_t>(ref_range[n_pairs] - r0);
    // hyp_bytes and ref_bytes are 0 for the device entry: nothing is uploaded then
    FA_TRY(fa::take(ctx, "edit_distance", {{&b_hyp, hyp_bytes, true, hyp + h0}, {&b_ref, ref_bytes, true, ref + r0}, {&b_jobs, sizeof(Job) * J, true, plan.jobs.data()},
                                           {&b_out, sizeof(int32_t) * 4 * J}, {&b_ws, sizeof(int32_t) * static_cast<size_t>(plan.ws_ints)}}));
    WalkArgs a{device ? hyp : b_hyp.as<int32_t>(), device ? ref : b_ref.as<int32_t>(), nullptr, 0, b_ws.as<int32_t>(), nullptr};
    fa::DeviceTiming tim{ctx};
    FA_TRY(tim.begin());
    size_t base = 0;
    for (int c = 0; c < fa::wer::kClasses; ++c) {   // one launch per class that has pairs
        a.jobs = b_jobs.as<Job>() + base;
        a.n_jobs = plan.n_class[c];
        a.out = b_out.as<int32_t>() + 4 * base;
        fa::wer::launch_walk(st, a, c);
        base += static_cast<size_t>(plan.n_class[c]);
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_TRY(tim.end());
    std::vector<int32_t> got(4 * J);
    FA_HIP_TRY(ctx, hipMemcpyAsync(got.data(), b_out.p, sizeof(int32_t) * 4 * J, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    FA_TRY(tim.read());
    for (size_t i = 0; i < J; ++i) {
        fa_edit_counts &o = out[plan.jobs[i].pair];
        o.total = got[4 * i + 0];
        o.insertions = got[4 * i + 1];
        o.deletions = got[4 * i + 2];
        o.substitutions = got[4 * i + 3];
    }
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

fa_status fa_edit_distance_batch(fa_ctx *ctx, const int32_t *hyp, const int64_t *hyp_range, const int32_t *ref, const int64_t *ref_range, int64_t n_pairs,
                                 fa_edit_counts *out) {
    return edit_distance(ctx, hyp, hyp_range, ref, ref_range, n_pairs, out, false);
}

fa_status fa_edit_distance_batch_dev(fa_ctx *ctx, const int32_t *d_hyp, const int64_t *hyp_range, const int32_t *d_ref, const int64_t *ref_range,
                                     int64_t n_pairs, fa_edit_counts *out) {
    return edit_distance(ctx, d_hyp, hyp_range, d_ref, ref_range, n_pairs, out, true);
}

}  // extern "C"
