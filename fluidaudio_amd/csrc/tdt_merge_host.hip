// tdt_merge_host.hip — the host side of the TDT seam merge (kernel: tdt_merge.hip, plan: tdt_merge_launch.h): the argument pass, the
// uploads of the host-pointer entry, the workspace, the one synchronisation of a call and the C ABI.  Nothing of the reference's merge
// is decided here: what is decided here is decided from the arguments alone, before any device work.
#include <algorithm>

#include "fa_common.h"
#include "tdt_merge_launch.h"

namespace fa {
namespace tdtmerge {
void launch(hipStream_t stream, const Args &a, int32_t slots);
}
}  // namespace fa

namespace {

namespace mg = fa::tdtmerge;

fa_status merge(fa_ctx *ctx, const fa_tdt_merge_config *cfg, const int32_t *tok, const int32_t *time, const int32_t *dur, const float *conf, const int32_t *count,
                const int32_t max_out, const int64_t *window_range, const int64_t n, const uint8_t *safe, const int32_t *canon, const int32_t vocab,
                int32_t *out_tok, int32_t *out_time, int32_t *out_dur, float *out_conf, const int64_t *out_range, int32_t *out_counts, int32_t *statuses,
                int32_t *seam_routes, const bool device) {
    const fa_tdt_merge_config c = mg::config_or_default(cfg);
    const fa::Verdict v = mg::check(c, tok, time, dur, conf, count, max_out, window_range, n, vocab, out_tok, out_time, out_dur, out_conf, out_range, out_counts, statuses);
    if (v.status != FA_SUCCESS) return fa::set_error(ctx, v.status, "tdt_merge_windows: %s", v.text);
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n == 0) return FA_SUCCESS;
    return fa::no_throw(ctx, "tdt_merge_windows", [&]() -> fa_status {
    mg::Plan plan;
    mg::make_plan(window_range, out_range, n, max_out, plan);
    const size_t N = static_cast<size_t>(n), W = static_cast<size_t>(plan.windows), T = static_cast<size_t>(plan.out_tokens);
    const size_t cells = W * static_cast<size_t>(max_out), w0 = static_cast<size_t>(window_range[0]), o0 = static_cast<size_t>(out_range[0]);
    const bool tables = vocab > 0;

    fa::DeviceGuard guard(ctx->device);
    hipStream_t st = ctx->stream;
    fa::DevBuf b_recs, b_safe, b_canon, b_runmax, b_ws, b_routes, b_res, b_win, b_cnt, b_out;
    // the window arrays go up below, four to a buffer; a null table has 0 bytes and no upload
    const fa_status taken = fa::take(ctx, "tdt_merge_windows", {{&b_recs, sizeof(mg::Rec) * N, true, plan.recs.data()},
                                                                {&b_safe, safe && tables ? static_cast<size_t>(vocab) : 0, true, safe},
                                                                {&b_canon, canon && tables ? sizeof(int32_t) * static_cast<size_t>(vocab) : 0, true, canon},
                                                                {&b_runmax, sizeof(int32_t) * T}, {&b_ws, static_cast<size_t>(plan.slot_bytes) * static_cast<size_t>(plan.slots)},
                                                                {&b_routes, sizeof(int32_t) * W}, {&b_res, sizeof(int32_t) * 2 * N}, {&b_win, 16 * cells, !device},
                                                                {&b_cnt, sizeof(int32_t) * W, !device, count + w0}, {&b_out, 16 * T, !device}});
    if (taken == FA_ALLOCATION_FAILURE)   // the workspace is what grows with the input
        return fa::set_error(ctx, taken, "tdt_merge_windows: device allocation failed (%lld wave slots of %lld bytes)", (long long)plan.slots, (long long)plan.slot_bytes);
    FA_TRY(taken);

    mg::Args a{};
    if (device) {
        const size_t at = w0 * static_cast<size_t>(max_out);
        a.win = mg::Stream{const_cast<int32_t *>(tok) + at, const_cast<int32_t *>(time) + at, const_cast<int32_t *>(dur) + at, const_cast<float *>(conf) + at};
        a.counts = count + w0;
        a.out = mg::Stream{out_tok + o0, out_time + o0, out_dur + o0, out_conf + o0};
    } else {   // the windows of the call, array after array in one buffer; the same for the output
        int32_t *win = b_win.as<int32_t>(), *out = b_out.as<int32_t>();
        a.win = mg::Stream{win, win + cells, win + 2 * cells, reinterpret_cast<float *>(win + 3 * cells)};
        a.counts = b_cnt.as<int32_t>();
        a.out = mg::Stream{out, out + T, out + 2 * T, reinterpret_cast<float *>(out + 3 * T)};
        const size_t at = w0 * static_cast<size_t>(max_out);
        if (cells) {
            FA_HIP_TRY(ctx, hipMemcpyAsync(a.win.tok, tok + at, 4 * cells, hipMemcpyHostToDevice, st));
            FA_HIP_TRY(ctx, hipMemcpyAsync(a.win.time, time + at, 4 * cells, hipMemcpyHostToDevice, st));
            FA_HIP_TRY(ctx, hipMemcpyAsync(a.win.dur, dur + at, 4 * cells, hipMemcpyHostToDevice, st));
            FA_HIP_TRY(ctx, hipMemcpyAsync(a.win.conf, conf + at, 4 * cells, hipMemcpyHostToDevice, st));
        }
    }
    a.max_out = max_out;
    a.recs = b_recs.as<mg::Rec>();
    a.n_recs = static_cast<int32_t>(n);
    // without a vocabulary a table has no entry: every id is unsafe and has no twin, which is what an all-zero table says
    a.tb = mg::Tables{safe ? b_safe.as<uint8_t>() : nullptr, canon ? b_canon.as<int32_t>() : nullptr, vocab};
    a.tm = mg::Times{c.frame_seconds, c.overlap_seconds};
    a.runmax = b_runmax.as<int32_t>();
    a.ws = b_ws.as<unsigned char>();
    a.slot_bytes = plan.slot_bytes; a.big_l = plan.big_l; a.big_r = plan.big_r;
    a.small_side = mg::small_side_of(fa::sw(fa::Sw::TDT_MERGE_LDS_SIDE));
    a.routes = b_routes.as<int32_t>();
    a.out_counts = b_res.as<int32_t>();
    a.statuses = a.out_counts + N;

    fa::DeviceTiming tim{ctx};
    FA_TRY(tim.begin());
    mg::launch(st, a, plan.slots);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_TRY(tim.end());
    std::vector<int32_t> res(2 * N);
    FA_HIP_TRY(ctx, hipMemcpyAsync(res.data(), b_res.p, sizeof(int32_t) * 2 * N, hipMemcpyDeviceToHost, st));
    if (seam_routes && W) FA_HIP_TRY(ctx, hipMemcpyAsync(seam_routes + w0, b_routes.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
    if (!device && T) {
        FA_HIP_TRY(ctx, hipMemcpyAsync(out_tok + o0, a.out.tok, 4 * T, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(out_time + o0, a.out.time, 4 * T, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(out_dur + o0, a.out.dur, 4 * T, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(out_conf + o0, a.out.conf, 4 * T, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    FA_TRY(tim.read());
    std::copy(res.begin(), res.begin() + n, out_counts);
    std::copy(res.begin() + n, res.end(), statuses);
    return FA_SUCCESS;
    });
}

}  // namespace

extern "C" {

void fa_tdt_merge_default_config(fa_tdt_merge_config *cfg) {
    if (cfg) *cfg = mg::config_or_default(nullptr);
}

fa_status fa_tdt_merge_windows_dev(fa_ctx *ctx, const fa_tdt_merge_config *cfg, const int32_t *d_tok, const int32_t *d_time, const int32_t *d_dur, const float *d_conf,
                                   const int32_t *d_count, int32_t max_out, const int64_t *window_range, int64_t n_recordings, const uint8_t *splice_safe,
                                   const int32_t *case_canon, int32_t vocab, int32_t *d_out_tok, int32_t *d_out_time, int32_t *d_out_dur, float *d_out_conf,
                                   const int64_t *out_range, int32_t *out_counts, int32_t *statuses, int32_t *seam_routes) {
    return merge(ctx, cfg, d_tok, d_time, d_dur, d_conf, d_count, max_out, window_range, n_recordings, splice_safe, case_canon, vocab, d_out_tok, d_out_time, d_out_dur,
                 d_out_conf, out_range, out_counts, statuses, seam_routes, true);
}

fa_status fa_tdt_merge_windows(fa_ctx *ctx, const fa_tdt_merge_config *cfg, const int32_t *tok, const int32_t *time, const int32_t *dur, const float *conf,
                               const int32_t *count, int32_t max_out, const int64_t *window_range, int64_t n_recordings, const uint8_t *splice_safe,
                               const int32_t *case_canon, int32_t vocab, int32_t *out_tok, int32_t *out_time, int32_t *out_dur, float *out_conf, const int64_t *out_range,
                               int32_t *out_counts, int32_t *statuses, int32_t *seam_routes) {
    return merge(ctx, cfg, tok, time, dur, conf, count, max_out, window_range, n_recordings, splice_safe, case_canon, vocab, out_tok, out_time, out_dur, out_conf, out_range,
                 out_counts, statuses, seam_routes, false);
}

}  // extern "C"
