// sortformer_host.hip — the host side of the offline Sortformer diarizer around its network: window geometry (reference:
// Sources/FluidAudio/Diarizer/Sortformer/Offline/OfflineSortformerDiarizer.swift:303-363), the window plan that the pack and stitch
// entries share, the enumeration of the bijections and the host twin of the alignment (SortformerSpeakerStitcher.swift:27-90), and the
// C ABI.  The kernels and their launchers are sortformer.hip; what both share is sortformer_launch.h.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "sortformer_launch.h"

namespace {

using namespace fa::sortformer;

// ---------------------------------------------------------------- window geometry (:303-363)

struct Geometry {
    std::vector<fa_sortformer_window> win;
    std::vector<int64_t> total_out, range;   // per recording; range[B + 1]
    int32_t overlap_out = 0, hop_out = 0;
};

bool config_ok(const fa_sortformer_offline_config *c) {
    return c && c->window_output_frames >= 1 && c->subsampling >= 1 && c->speakers >= 1 && c->n_mels >= 1 &&
           static_cast<int64_t>(c->window_output_frames) * c->subsampling <= INT32_MAX / 2;
}

// false: a recording's length is negative or its windows overflow 32-bit frame indices
bool geometry(const fa_sortformer_offline_config &c, const int64_t *n_mel, int32_t B, Geometry &g) {
    const int64_t window = c.window_output_frames, sub = c.subsampling, window_mel = window * sub;
    const int64_t overlap = std::max<int64_t>(0, std::min<int64_t>(c.overlap_output_frames, window - 1));
    const int64_t hop_out = window - overlap, hop_mel = hop_out * sub;
    g.overlap_out = static_cast<int32_t>(overlap);
    g.hop_out = static_cast<int32_t>(hop_out);
    g.total_out.assign(static_cast<size_t>(B), 0);
    g.range.assign(static_cast<size_t>(B) + 1, 0);
    for (int32_t b = 0; b < B; ++b) {
        const int64_t n = n_mel[b];
        if (n < 0 || n > INT32_MAX - window_mel) return false;
        g.total_out[b] = (n + sub - 1) / sub;
        int64_t mel_start = 0;
        bool first = true;
        while (mel_start < n) {
            const int64_t valid_mel = std::min(window_mel, n - mel_start);
            fa_sortformer_window w;
            w.recording = b;
            w.valid_mel = static_cast<int32_t>(valid_mel);
            w.valid_out = static_cast<int32_t>(std::min(window, (valid_mel + sub - 1) / sub));
            w.first = first ? 1 : 0;
            w.mel_start = mel_start;
            w.g_start = mel_start / sub;
            g.win.push_back(w);
            first = false;
            if (valid_mel < window_mel) break;
            mel_start += hop_mel;
        }
        g.range[b + 1] = static_cast<int64_t>(g.win.size());
    }
    return true;
}

// ---------------------------------------------------------------- the window plan of a device call

struct WindowPlan {
    const char *what = "";            // "sortformer pack" / "sortformer stitch": the prefix of every message
    Geometry geo;
    std::vector<int64_t> gofs;        // stitch: [B + 1] first global frame of each recording, the prefix sums of geo.total_out
    int64_t W = 0, items = 0;         // windows; stitch: global frames * speakers
    int32_t speakers = 0;
};

// The one place that derives the windows of a device call and refuses what the 32-bit grids of the launchers cannot hold.
fa_status plan_windows(fa_ctx *ctx, const char *what, const fa_sortformer_offline_config &cfg, const int64_t *n_mel_frames, int32_t batch, int64_t windows,
                       bool need_gofs, WindowPlan &p) {
    p.what = what;
    p.speakers = cfg.speakers;
    if (!geometry(cfg, n_mel_frames, batch, p.geo)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: bad recording lengths", what);
    p.W = static_cast<int64_t>(p.geo.win.size());
    if (p.W != windows) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: %lld windows given, the geometry has %lld", what, (long long)windows, (long long)p.W);
    bool fits;
    if (need_gofs) {   // launch_stitch: a workgroup per window, kMergeItems items per workgroup
        p.gofs.assign(static_cast<size_t>(batch) + 1, 0);
        for (int32_t b = 0; b < batch; ++b) p.gofs[b + 1] = p.gofs[b] + p.geo.total_out[b];
        p.items = p.gofs[batch] * cfg.speakers;
        fits = p.W < INT32_MAX && p.items / kMergeItems < INT32_MAX;
    } else {           // launch_pack: a workgroup per (window, mel row) or per tile
        const int64_t window_mel = static_cast<int64_t>(cfg.window_output_frames) * cfg.subsampling;
        const int64_t tiles = ((window_mel + kPackTile - 1) / kPackTile) * ((cfg.n_mels + kPackTile - 1) / kPackTile);
        fits = p.W * cfg.n_mels < INT32_MAX && p.W * tiles < INT32_MAX;
    }
    if (!fits) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "%s: %lld windows", what, (long long)p.W);
    return FA_SUCCESS;
}

struct WindowTables { fa::DevBuf win, range, gofs, corr, ov; };   // pack takes win only

// The plan's tables on the device, on the context's stream; they are released with the call, after its synchronisation.
fa_status stage_windows(fa_ctx *ctx, const WindowPlan &p, WindowTables &t) {
    const bool stitch = !p.gofs.empty();
    const size_t win_bytes = sizeof(fa_sortformer_window) * p.W, rec_bytes = sizeof(int64_t) * p.geo.range.size();
    return fa::take(ctx, p.what, {{&t.win, win_bytes, true, p.geo.win.data()}, {&t.range, rec_bytes, stitch, p.geo.range.data()}, {&t.gofs, rec_bytes, stitch, p.gofs.data()},
                                  {&t.corr, sizeof(float) * p.W * p.speakers * p.speakers, stitch}, {&t.ov, sizeof(int32_t) * p.W, stitch}});
}

// ---------------------------------------------------------------- the stitcher's host side

// the reference's enumeration (SortformerSpeakerStitcher.swift:80-90): swap recursion, not lexicographic
void enumerate(int *arr, int k, int S, Perms &out) {
    if (k == S) {
        for (int i = 0; i < S; ++i) out.p[out.n][i] = static_cast<uint8_t>(arr[i]);
        ++out.n;
        return;
    }
    for (int i = k; i < S; ++i) {
        std::swap(arr[k], arr[i]);
        enumerate(arr, k + 1, S, out);
        std::swap(arr[k], arr[i]);
    }
}

Perms make_perms(int S) {
    Perms p;
    memset(&p, 0, sizeof(p));
    int arr[kMaxSpeakers] = {0, 1, 2, 3};
    enumerate(arr, 0, S, p);
    return p;
}

// the host twin of the alignment (SortformerSpeakerStitcher.alignment :27-77).  The correlation step is written out here, in stitch_corr and
// in stitch_serial: a helper that takes the two values makes both kernels load the window's value before the guard
void alignment_host(const float *global, const float *window, int64_t frames, int S, int32_t *mapping) {
    float corr[kMaxSpeakers][kMaxSpeakers] = {};
    for (int64_t f = 0; f < frames; ++f) {
        for (int g = 0; g < S; ++g) {
            const float gv = global[f * S + g];
            if (!(gv != 0.0f)) continue;
            for (int w = 0; w < S; ++w) corr[g][w] += gv * window[f * S + w];
        }
    }
    const Perms perms = make_perms(S);
    int best = -1;
    float best_score = -3.40282347e38f;
    for (int p = 0; p < perms.n; ++p) {
        float score = 0.0f;
        for (int g = 0; g < S; ++g) score += corr[g][perms.p[p][g]];
        if (score > best_score) { best_score = score; best = p; }
    }
    for (int g = 0; g < S; ++g) mapping[best >= 0 ? perms.p[best][g] : g] = g;
}

}  // namespace

extern "C" {

void fa_sortformer_offline_default_config(fa_sortformer_offline_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->window_output_frames = 384;    // OfflineSortformerDiarizer.swift:17-43
    cfg->subsampling = 8;
    cfg->speakers = 4;
    cfg->n_mels = 128;
    cfg->overlap_output_frames = 100;
}

fa_status fa_sortformer_offline_windows(const fa_sortformer_offline_config *cfg, const int64_t *n_mel_frames, int32_t batch, fa_sortformer_window *windows,
                                        int64_t capacity, int64_t *count, int64_t *total_out, int64_t *window_range) {
    if (!config_ok(cfg) || !count || batch < 0 || capacity < 0 || (batch > 0 && !n_mel_frames)) return FA_INVALID_ARGUMENT;
    *count = 0;
    return fa::no_throw(nullptr, "sortformer windows", [&]() -> fa_status {
        Geometry g;
        if (!geometry(*cfg, n_mel_frames, batch, g)) return FA_INVALID_ARGUMENT;
        *count = static_cast<int64_t>(g.win.size());
        if (total_out) std::copy(g.total_out.begin(), g.total_out.end(), total_out);
        if (window_range) std::copy(g.range.begin(), g.range.end(), window_range);
        if (!windows) return FA_SUCCESS;
        if (capacity < *count) return FA_OUTPUT_TOO_SMALL;
        std::copy(g.win.begin(), g.win.end(), windows);
        return FA_SUCCESS;
    });
}

fa_status fa_sortformer_pack_windows_dev(fa_ctx *ctx, const fa_sortformer_offline_config *cfg, const float *d_mel, int32_t layout, int64_t rec_stride,
                                         int64_t frame_stride, const int64_t *n_mel_frames, int32_t batch, int64_t windows, float *d_out,
                                         int32_t *d_mel_length) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!config_ok(cfg) || batch < 0 || windows < 0 || (batch > 0 && !n_mel_frames) || rec_stride < 0 || frame_stride < 0 ||
        (layout != FA_MEL_LAYOUT_MEL_MAJOR && layout != FA_MEL_LAYOUT_FRAME_MAJOR))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: bad arguments");
    return fa::no_throw(ctx, "sortformer pack", [&]() -> fa_status {
    WindowPlan plan;
    FA_TRY(plan_windows(ctx, "sortformer pack", *cfg, n_mel_frames, batch, windows, false, plan));
    if (plan.W == 0) return FA_SUCCESS;
    if (!d_mel || !d_out || !d_mel_length) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: mel, output and mel_length are required");
    const int32_t n_mels = cfg->n_mels, window_mel = cfg->window_output_frames * cfg->subsampling;
    for (int32_t b = 0; b < batch; ++b) {   // every recording's frames lie inside its slot of the mel buffer
        const int64_t n = n_mel_frames[b];
        const bool fits = layout == FA_MEL_LAYOUT_MEL_MAJOR ? (n <= frame_stride && (batch == 1 || static_cast<int64_t>(n_mels) * frame_stride <= rec_stride))
                                                            : (batch == 1 || n * n_mels <= rec_stride);
        if (!fits) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer pack: recording %d does not fit its strides", b);
    }
    fa::DeviceGuard guard(ctx->device);
    WindowTables t;
    FA_TRY(stage_windows(ctx, plan, t));
    launch_pack(ctx->stream, PackArgs{d_mel, t.win.as<fa_sortformer_window>(), d_out, d_mel_length, rec_stride, frame_stride, n_mels, window_mel}, layout, plan.W);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the staged window table is released with this call
    return FA_SUCCESS;
    });
}

fa_status fa_sortformer_stitch_dev(fa_ctx *ctx, const fa_sortformer_offline_config *cfg, const float *d_preds, const int64_t *n_mel_frames, int32_t batch,
                                   int64_t windows, float *d_global, int32_t *d_mapping) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (!config_ok(cfg) || batch < 0 || windows < 0 || (batch > 0 && !n_mel_frames) || cfg->speakers > kMaxSpeakers)
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer stitch: bad arguments (1 to %d speakers)", kMaxSpeakers);
    return fa::no_throw(ctx, "sortformer stitch", [&]() -> fa_status {
    WindowPlan plan;
    FA_TRY(plan_windows(ctx, "sortformer stitch", *cfg, n_mel_frames, batch, windows, true, plan));
    if (plan.W == 0) return FA_SUCCESS;
    if (!d_preds || !d_global || !d_mapping) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "sortformer stitch: predictions, timeline and mapping are required");
    fa::DeviceGuard guard(ctx->device);
    WindowTables t;
    FA_TRY(stage_windows(ctx, plan, t));
    const StitchArgs sa{d_preds, t.win.as<fa_sortformer_window>(), t.range.as<int64_t>(), t.gofs.as<int64_t>(), t.corr.as<float>(), t.ov.as<int32_t>(),
                        d_global, d_mapping, batch, cfg->speakers, cfg->window_output_frames, plan.geo.overlap_out, plan.geo.hop_out};
    FA_HIP_TRY(ctx, launch_stitch(ctx->stream, sa, make_perms(cfg->speakers), plan.W, plan.items));
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the staged geometry is released with this call
    return FA_SUCCESS;
    });
}

fa_status fa_sortformer_stitcher_alignment(const float *global, const float *window, int64_t frames, int32_t speakers, int32_t *mapping) {
    if (speakers < 1 || speakers > kMaxSpeakers || !mapping) return FA_INVALID_ARGUMENT;
    for (int32_t s = 0; s < speakers; ++s) mapping[s] = s;
    if (frames <= 0) return FA_SUCCESS;           // nothing to align on: identity (:34-39)
    if (!global || !window) return FA_INVALID_ARGUMENT;
    alignment_host(global, window, frames, speakers, mapping);
    return FA_SUCCESS;
}

}  // extern "C"
