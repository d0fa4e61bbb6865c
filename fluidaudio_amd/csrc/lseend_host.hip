// lseend_host.hip — host side of the LS-EEND front end (kernels: lseend.hip): the tables (the mel featurizer's own periodic Hann and
// Slaney bank, through its C entries), the plans of lseend_core.h as C records, the offline entry, the stream state with its carried
// tails in HBM, the gather of the network's output, and the host-pointer forms.  Nothing here waits for the device except get / set
// and the host-pointer forms, and every count is computed before the launches.
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "lseend_launch.h"

using namespace fa::lseend;

namespace {

constexpr int64_t kMaxItemSamples = (int64_t{1} << 31) - (int64_t{1} << 22);   // an item's sequence, tail and flush included, stays an int32

bool geometry_of(const fa_lseend_config *c, Geometry &g) {
    if (!c || c->sample_rate < 1 || !(c->log_floor > 0.0f) || c->n_mels > kMaxMels) return false;
    return make_geometry(c->n_fft, c->hop, c->win, c->n_mels, c->context_size, c->subsampling, c->conv_delay, c->chunk_size, g);
}

struct Tables {
    fa::DevBuf dev;
    Args base{};      // geometry, constants and the pointers into `dev`
    size_t lds = 0;
};

// the window and the bank are the mel featurizer's (fa_mel_hann_window / fa_mel_filterbank in the LS-EEND flavour of LSEENDPreprocessor.swift:70-82)
fa_status make_tables(fa_ctx *ctx, const fa_lseend_config *cfg, Tables &t, const bool cached) {
    Geometry g;
    if (!geometry_of(cfg, g)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend: unsupported configuration");
    if (g.n_fft != kNfft) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend: n_fft %d (this kernel generation serves 256)", g.n_fft);
    fa_mel_config mc;
    fa_mel_default_config(&mc);
    mc.sample_rate = cfg->sample_rate; mc.n_mels = g.n_mels; mc.n_fft = g.n_fft; mc.hop = g.hop; mc.win = g.win;
    mc.preemph = 0.0f; mc.log_floor = cfg->log_floor; mc.floor_mode = FA_MEL_FLOOR_CLAMPED; mc.window_periodic = 1; mc.padding_mode = FA_MEL_PAD_PREPADDED;
    const int bins = kBins;
    std::vector<float> hann(g.win), fb(static_cast<size_t>(g.n_mels) * bins), windowz(kNfft, 0.0f), weights;
    FA_TRY(fa_mel_hann_window(&mc, hann.data()));
    FA_TRY(fa_mel_filterbank(&mc, fb.data()));
    for (int i = 0; i < g.win; ++i) windowz[(g.n_fft - g.win) / 2 + i] = hann[i];   // centred in n_fft
    std::vector<int32_t> tab(2 * static_cast<size_t>(g.n_mels), 0);
    for (int m = 0; m < g.n_mels; ++m) {   // a row's support: first to last non-zero bin, interior zeros kept
        int l0 = -1, h0 = -1;
        for (int k = 0; k < bins; ++k) if (fb[static_cast<size_t>(m) * bins + k] != 0.0f) { if (l0 < 0) l0 = k; h0 = k; }
        const int cnt = l0 < 0 ? 0 : h0 - l0 + 1;
        tab[2 * m] = (l0 < 0 ? 0 : l0) | (cnt << 16);
        tab[2 * m + 1] = static_cast<int32_t>(weights.size());
        for (int j = 0; j < cnt; ++j) weights.push_back(fb[static_cast<size_t>(m) * bins + l0 + j]);
    }
    if (weights.empty()) weights.push_back(0.0f);
    std::vector<float2> tw(256);
    for (int k = 0; k < 256; ++k) { const double a = -2.0 * M_PI * k / 256; tw[k] = make_float2(static_cast<float>(cos(a)), static_cast<float>(sin(a))); }

    Args &a = t.base;
    a.g = g;
    a.n_weights = static_cast<int32_t>(weights.size());
    a.stage_alloc = ((kTileFrames - 1) * g.hop + g.n_fft + 3) & ~3;
    a.log_floor = cfg->log_floor;
    a.log10_scale = static_cast<float>(1.0 / log(10.0));   // :36
    t.lds = lds_bytes(a);
    if (t.lds > 64 * 1024) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend: tile does not fit LDS");
    std::vector<char> img;
    auto add = [&img](const void *src, size_t bytes) { const size_t at = img.size(); img.resize((at + bytes + 255) & ~static_cast<size_t>(255), 0); memcpy(img.data() + at, src, bytes); return at; };
    const size_t o_win = add(windowz.data(), sizeof(float) * windowz.size()), o_tw = add(tw.data(), sizeof(float2) * tw.size());
    const size_t o_tab = add(tab.data(), sizeof(int32_t) * tab.size()), o_w = add(weights.data(), sizeof(float) * weights.size());
    if ((cached ? t.dev.alloc(ctx, img.size()) : t.dev.alloc(img.size())) != hipSuccess) { (void)hipGetLastError(); return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "lseend: device allocation failed"); }
    FA_HIP_TRY(ctx, hipMemcpyAsync(t.dev.p, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream));
    // (here and in launch_job the source is pageable host memory: the copy has left it when the call returns, so a local may go)
    if (!cached) FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    char *d = t.dev.as<char>();
    a.windowz = reinterpret_cast<const float *>(d + o_win); a.tw256 = reinterpret_cast<const float2 *>(d + o_tw);
    a.mel_tab = reinterpret_cast<const int32_t *>(d + o_tab); a.mel_w = reinterpret_cast<const float *>(d + o_w);
    return FA_SUCCESS;
}

// the items of one call with their tiles, and the call's totals
struct Job {
    std::vector<Item> items;
    std::vector<int32_t> tile_item;
    int64_t frames = 0, windows = 0, out_rows = 0;
};

void add_item(Job &j, const Step &s, Item it, const int64_t pcm_off, const int64_t n_new) {
    it.pcm_off = pcm_off; it.n_new = static_cast<int32_t>(n_new);
    it.frames0 = s.frames0; it.windows0 = s.windows0; it.windows1 = s.windows0 + s.windows;
    it.row0 = j.frames; it.win0 = j.windows; it.out_row0 = j.out_rows;
    it.tail_in = s.tail_in; it.tail_out = s.tail_out; it.mel_in = s.mel_in;
    it.frames = static_cast<int32_t>(s.frames);
    it.tile0 = static_cast<int32_t>(j.tile_item.size());
    it.tiles = static_cast<int32_t>((s.frames + kTileFrames - 1) / kTileFrames);
    j.tile_item.insert(j.tile_item.end(), it.tiles, static_cast<int32_t>(j.items.size()));
    j.items.push_back(it);
    j.frames += s.frames; j.windows += s.windows; j.out_rows += s.out_rows;
}

void fill_plan(fa_lseend_item_plan *p, const Geometry &g, const Step &s, const Counters &after, const Job &before) {
    p->frames = s.frames; p->frame0 = before.frames; p->windows = s.windows; p->window0 = before.windows;
    p->out_rows = s.out_rows; p->out_row0 = before.out_rows; p->flush_samples = s.zeros; p->stream_window0 = s.windows0;
    p->unread_audio = s.tail_out; p->unread_mel_rows = s.mel_out; p->decoder_mask_end = mask_end_of(g, after.windows); p->reserved = 0;
}

// warm-up counts and mask slices of the windows [w0, w0 + n) of a stream, behind `at` windows already described
void describe_windows(const Geometry &g, const int64_t w0, const int64_t n, const int64_t at, int32_t *warmups, float *masks) {
    for (int64_t k = 0; k < n; ++k) {
        if (warmups) warmups[at + k] = warmup_of(g, w0 + k);
        if (masks)
            for (int j = 0; j < g.chunk; ++j) masks[(at + k) * g.chunk + j] = mask_end_of(g, w0 + k + 1) - g.chunk + j >= g.conv_delay ? 1.0f : 0.0f;
    }
}

// upload the job's two tables and launch; the device copies of items / tiles and the three work arrays are the caller's
fa_status launch_job(fa_ctx *ctx, const Tables &t, const Job &j, void *d_items, void *d_tiles, double *d_sums, double *d_prefix, float *d_rows, const float *d_pcm,
                     const int64_t pcm_total, float *d_windows, float *d_masks, int32_t *d_warmups, int64_t *d_out_rows) {
    Args a = t.base;
    FA_HIP_TRY(ctx, hipMemcpyAsync(d_items, j.items.data(), sizeof(Item) * j.items.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!j.tile_item.empty()) FA_HIP_TRY(ctx, hipMemcpyAsync(d_tiles, j.tile_item.data(), sizeof(int32_t) * j.tile_item.size(), hipMemcpyHostToDevice, ctx->stream));
    a.items = static_cast<const Item *>(d_items); a.tile_item = static_cast<const int32_t *>(d_tiles);
    a.pcm = d_pcm; a.pcm_total = pcm_total; a.vec = reinterpret_cast<uintptr_t>(d_pcm) % 16 == 0;
    a.rows = d_rows; a.tile_sums = d_sums; a.tile_prefix = d_prefix;
    a.windows = d_windows; a.masks = d_masks; a.warmups = d_warmups; a.out_rows = d_out_rows;
    a.n_items = static_cast<int32_t>(j.items.size()); a.n_tiles = static_cast<int32_t>(j.tile_item.size());
    run(a, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // namespace

struct fa_lseend_stream {
    fa_ctx *ctx = nullptr;
    Geometry g{};
    Tables tab;
    int32_t streams = 0;
    int64_t max_push = 0, max_frames = 0, max_tiles = 0;   // per call, all streams together
    int64_t tail_stride = 0, mel_stride = 0;               // floats per stream and buffer
    std::vector<Counters> cnt;
    std::vector<uint8_t> parity, is_fresh;                 // which of the two buffers holds the state; fresh: nothing on the device yet, all zeros
    fa::DevBuf tails, mels, sums, items, tiles, tsums, tprefix, rows;
    float *tail(int s, int par) const { return tails.as<float>() + (static_cast<int64_t>(par) * streams + s) * tail_stride; }
    float *mel(int s, int par) const { return mels.as<float>() + (static_cast<int64_t>(par) * streams + s) * mel_stride; }
    double *sum(int s, int par) const { return sums.as<double>() + (static_cast<int64_t>(par) * streams + s) * g.n_mels; }
};

extern "C" {

void fa_lseend_default_config(fa_lseend_config *c) {
    if (!c) return;
    c->sample_rate = 8000; c->n_mels = 23; c->n_fft = 256; c->hop = 80; c->win = 200;
    c->context_size = 7; c->subsampling = 10; c->conv_delay = 9; c->chunk_size = 5;
    c->log_floor = 1e-10f;
}

int32_t fa_lseend_mel_frames(const fa_lseend_config *cfg) {
    Geometry g;
    return geometry_of(cfg, g) ? g.mel_frames : 0;
}

fa_status fa_lseend_plan_push(const fa_lseend_config *cfg, fa_lseend_stream_info *state, int64_t samples, int32_t flush, fa_lseend_item_plan *plan, int32_t *warmups,
                              float *masks, int64_t window_capacity) {
    Geometry g;
    if (!geometry_of(cfg, g) || !state || samples < 0 || state->audio_samples < 0) return FA_INVALID_ARGUMENT;
    Counters c{g.n_fft / 2 + state->audio_samples, state->frames, state->windows};
    if (c.frames != frames_of(g, c.audio) || c.windows != windows_of(g, c.frames)) return FA_INVALID_ARGUMENT;   // not a state the queues reach
    const Step s = advance(g, c, samples, flush != 0);
    if ((warmups || masks) && s.windows > window_capacity) return FA_OUTPUT_TOO_SMALL;
    describe_windows(g, s.windows0, s.windows, 0, warmups, masks);
    if (plan) fill_plan(plan, g, s, c, Job());
    state->audio_samples = c.audio - g.n_fft / 2; state->frames = c.frames; state->windows = c.windows;
    state->unread_audio = s.tail_out; state->unread_mel_rows = s.mel_out; state->decoder_mask_end = mask_end_of(g, c.windows); state->reserved = 0;
    return FA_SUCCESS;
}

fa_status fa_lseend_plan_file(const fa_lseend_config *cfg, const int64_t *offsets, int32_t batch, fa_lseend_item_plan *items, int32_t *warmups, float *masks,
                              int64_t window_capacity) {
    Geometry g;
    if (!geometry_of(cfg, g) || !offsets || batch < 1 || !items) return FA_INVALID_ARGUMENT;
    Job j;   // totals only
    for (int b = 0; b < batch; ++b) {
        const int64_t len = offsets[b + 1] - offsets[b];
        if (len < 0) return FA_INVALID_ARGUMENT;
        if (len > kMaxItemSamples) return FA_INDEX_OVERFLOW;
        Counters c = fresh(g);
        const Step s = advance(g, c, len, true);
        if ((warmups || masks) && j.windows + s.windows > window_capacity) return FA_OUTPUT_TOO_SMALL;
        describe_windows(g, 0, s.windows, j.windows, warmups, masks);
        fill_plan(&items[b], g, s, c, j);
        j.frames += s.frames; j.windows += s.windows; j.out_rows += s.out_rows;
    }
    return FA_SUCCESS;
}

fa_status fa_lseend_features_dev(fa_ctx *ctx, const fa_lseend_config *cfg, const float *d_pcm, const int64_t *offsets, int32_t batch, float *d_windows,
                                 float *d_masks, int32_t *d_warmups, int64_t *d_out_rows, float *d_raw) {
    if (!ctx || !cfg || !offsets || batch < 1 || !d_windows) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_lseend_features_dev", [&]() -> fa_status {
        Tables t;
        FA_TRY(make_tables(ctx, cfg, t, true));
        Job j;
        for (int b = 0; b < batch; ++b) {
            const int64_t len = offsets[b + 1] - offsets[b];
            if (len < 0 || offsets[b] < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend: offsets not monotone");
            if (len > kMaxItemSamples) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "lseend: recording too long");
            Counters c = fresh(t.base.g);
            add_item(j, advance(t.base.g, c, len, true), Item{}, offsets[b], len);   // no carried state in, none out
        }
        if (offsets[batch] > 0 && !d_pcm) return FA_INVALID_ARGUMENT;
        if (j.tile_item.size() > static_cast<size_t>(INT32_MAX / 2)) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "lseend: too many tiles in one call");
        const size_t n = static_cast<size_t>(t.base.g.n_mels), tiles = j.tile_item.size();
        fa::DevBuf d_items, d_tiles, d_sums, d_prefix, d_rows;
        FA_TRY(fa::take(ctx, "fa_lseend_features_dev", {{&d_items, sizeof(Item) * j.items.size()}, {&d_tiles, sizeof(int32_t) * tiles}, {&d_sums, sizeof(double) * tiles * n},
                                                        {&d_prefix, sizeof(double) * tiles * n}, {&d_rows, sizeof(float) * static_cast<size_t>(j.frames) * n, d_raw == nullptr}}));
        return launch_job(ctx, t, j, d_items.p, d_tiles.p, d_sums.as<double>(), d_prefix.as<double>(), d_raw ? d_raw : d_rows.as<float>(), d_pcm, offsets[batch], d_windows,
                          d_masks, d_warmups, d_out_rows);
    });
}

fa_status fa_lseend_features(fa_ctx *ctx, const fa_lseend_config *cfg, const float *pcm, const int64_t *offsets, int32_t batch, float *windows, float *masks,
                             int32_t *warmups, int64_t *out_rows, float *raw) {
    if (!ctx || !cfg || !offsets || batch < 1) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_lseend_features", [&]() -> fa_status {
        Geometry g;
        if (!geometry_of(cfg, g)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend: unsupported configuration");
        std::vector<fa_lseend_item_plan> plan(batch);
        FA_TRY(fa_lseend_plan_file(cfg, offsets, batch, plan.data(), nullptr, nullptr, 0));
        const size_t W = static_cast<size_t>(plan.back().window0 + plan.back().windows), F = static_cast<size_t>(plan.back().frame0 + plan.back().frames);
        const size_t ns = static_cast<size_t>(offsets[batch]), wf = W * g.mel_frames * g.n_mels;
        if ((ns > 0 && !pcm) || (W > 0 && !windows)) return FA_INVALID_ARGUMENT;
        fa::DevBuf d_pcm, d_win, d_masks, d_warm, d_or, d_raw;
        FA_TRY(fa::take(ctx, "fa_lseend_features", {{&d_pcm, sizeof(float) * ns, true, pcm}, {&d_win, sizeof(float) * wf}, {&d_masks, sizeof(float) * W * g.chunk, masks != nullptr},
                                                    {&d_warm, sizeof(int32_t) * W, warmups != nullptr}, {&d_or, sizeof(int64_t) * W, out_rows != nullptr},
                                                    {&d_raw, sizeof(float) * F * g.n_mels, raw != nullptr}}));
        FA_TRY(fa_lseend_features_dev(ctx, cfg, d_pcm.as<float>(), offsets, batch, d_win.as<float>(), d_masks.as<float>(), d_warm.as<int32_t>(), d_or.as<int64_t>(), d_raw.as<float>()));
        if (wf) FA_HIP_TRY(ctx, hipMemcpyAsync(windows, d_win.p, sizeof(float) * wf, hipMemcpyDeviceToHost, ctx->stream));
        if (masks && W) FA_HIP_TRY(ctx, hipMemcpyAsync(masks, d_masks.p, sizeof(float) * W * g.chunk, hipMemcpyDeviceToHost, ctx->stream));
        if (warmups && W) FA_HIP_TRY(ctx, hipMemcpyAsync(warmups, d_warm.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, ctx->stream));
        if (out_rows && W) FA_HIP_TRY(ctx, hipMemcpyAsync(out_rows, d_or.p, sizeof(int64_t) * W, hipMemcpyDeviceToHost, ctx->stream));
        if (raw && F) FA_HIP_TRY(ctx, hipMemcpyAsync(raw, d_raw.p, sizeof(float) * F * g.n_mels, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_lseend_stream_create(fa_ctx *ctx, const fa_lseend_config *cfg, int32_t streams, int64_t max_push_samples, fa_lseend_stream **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    if (!cfg || streams < 1 || streams > 65536 || max_push_samples < 1 || max_push_samples > kMaxItemSamples) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend stream: bad arguments");
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_lseend_stream_create", [&]() -> fa_status {
        std::unique_ptr<fa_lseend_stream> st(new fa_lseend_stream());
        st->ctx = ctx;
        FA_TRY(make_tables(ctx, cfg, st->tab, false));
        const Geometry &g = st->g = st->tab.base.g;
        st->streams = streams; st->max_push = max_push_samples;
        // a call's sequence of one stream: the carried tail, the push, the flush and its rounding
        const int64_t per_stream = (g.audio_tail_cap + max_push_samples + g.flush_samples + g.chunk_samples) / g.hop + 1;
        st->max_frames = per_stream * streams;
        st->max_tiles = (per_stream / kTileFrames + 1) * streams;
        st->tail_stride = (g.audio_tail_cap + 3) & ~3;
        st->mel_stride = static_cast<int64_t>(g.mel_tail_cap > 0 ? g.mel_tail_cap : 1) * g.n_mels;
        st->cnt.assign(streams, fresh(g)); st->parity.assign(streams, 0); st->is_fresh.assign(streams, 1);
        const size_t n = static_cast<size_t>(g.n_mels), S = static_cast<size_t>(streams);
        FA_TRY(fa::take_once(ctx, "fa_lseend_stream_create", {{&st->tails, sizeof(float) * 2 * S * st->tail_stride}, {&st->mels, sizeof(float) * 2 * S * st->mel_stride},
                                                             {&st->sums, sizeof(double) * 2 * S * n}, {&st->items, sizeof(Item) * S}, {&st->tiles, sizeof(int32_t) * st->max_tiles},
                                                             {&st->tsums, sizeof(double) * st->max_tiles * n}, {&st->tprefix, sizeof(double) * st->max_tiles * n},
                                                             {&st->rows, sizeof(float) * st->max_frames * n}}));
        *out = st.release();
        return FA_SUCCESS;
    });
}

void fa_lseend_stream_destroy(fa_lseend_stream *st) {
    if (!st) return;
    if (st->tails.p) { (void)hipSetDevice(st->ctx->device); (void)hipStreamSynchronize(st->ctx->stream); }
    delete st;
}

fa_status fa_lseend_stream_reset(fa_ctx *ctx, fa_lseend_stream *st, int32_t stream) {
    if (!ctx || !st || ctx != st->ctx || stream < -1 || stream >= st->streams) return FA_INVALID_ARGUMENT;
    for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? st->streams : stream + 1); ++s) { st->cnt[s] = fresh(st->g); st->is_fresh[s] = 1; }
    return FA_SUCCESS;
}

fa_status fa_lseend_stream_push_dev(fa_ctx *ctx, fa_lseend_stream *st, const float *d_pcm, const int64_t *offsets, const int32_t *flush, int64_t window_capacity,
                                    float *d_windows, float *d_masks, int32_t *d_warmups, int64_t *d_out_rows, float *d_raw, fa_lseend_item_plan *plans) {
    if (!ctx || !st || ctx != st->ctx || !offsets || window_capacity < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_lseend_stream_push_dev", [&]() -> fa_status {
        const Geometry &g = st->g;
        Job j;
        std::vector<Counters> next = st->cnt;
        for (int s = 0; s < st->streams; ++s) {
            const int64_t len = offsets[s + 1] - offsets[s];
            if (len < 0 || offsets[s] < 0 || len > st->max_push) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend stream: a push of %lld samples (limit %lld)", (long long)len, (long long)st->max_push);
            const Job before = j;   // totals only are read
            const Step step = advance(g, next[s], len, flush && flush[s]);
            const int par = st->parity[s];
            Item it{};
            if (!st->is_fresh[s]) { it.tail_src = st->tail(s, par); it.mel_src = st->mel(s, par); it.sum_src = st->sum(s, par); }
            it.tail_dst = st->tail(s, par ^ 1); it.mel_dst = st->mel(s, par ^ 1); it.sum_dst = st->sum(s, par ^ 1);
            if (plans) { Job totals; totals.frames = before.frames; totals.windows = before.windows; totals.out_rows = before.out_rows; fill_plan(&plans[s], g, step, next[s], totals); }
            add_item(j, step, it, offsets[s], len);
        }
        if (offsets[st->streams] > 0 && !d_pcm) return FA_INVALID_ARGUMENT;
        if (j.windows > window_capacity || (j.windows > 0 && !d_windows)) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "lseend stream: %lld windows ready, room for %lld", (long long)j.windows, (long long)window_capacity);
        if (j.frames > st->max_frames || static_cast<int64_t>(j.tile_item.size()) > st->max_tiles) return fa::set_error(ctx, FA_RUNTIME_ERROR, "lseend stream: workspace bound exceeded");
        FA_TRY(launch_job(ctx, st->tab, j, st->items.p, st->tiles.p, st->tsums.as<double>(), st->tprefix.as<double>(), d_raw ? d_raw : st->rows.as<float>(), d_pcm, offsets[st->streams],
                          d_windows, d_masks, d_warmups, d_out_rows));
        st->cnt = next;   // the launches are queued: the other buffers hold the state from here on
        for (int s = 0; s < st->streams; ++s) { st->parity[s] ^= 1; st->is_fresh[s] = 0; }
        return FA_SUCCESS;
    });
}

fa_status fa_lseend_stream_push(fa_ctx *ctx, fa_lseend_stream *st, const float *pcm, const int64_t *offsets, const int32_t *flush, int64_t window_capacity, float *windows,
                                float *masks, int32_t *warmups, int64_t *out_rows, float *raw, int64_t raw_capacity, fa_lseend_item_plan *plans) {
    if (!ctx || !st || ctx != st->ctx || !offsets || !plans || window_capacity < 0 || raw_capacity < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_lseend_stream_push", [&]() -> fa_status {
        const Geometry &g = st->g;
        const size_t ns = static_cast<size_t>(offsets[st->streams] > 0 ? offsets[st->streams] : 0), cap = static_cast<size_t>(window_capacity);
        if (ns > 0 && !pcm) return FA_INVALID_ARGUMENT;
        if (raw && raw_capacity < st->max_frames) {   // the rows of this call have to fit: count them first
            int64_t frames = 0;
            for (int s = 0; s < st->streams; ++s) { Counters c = st->cnt[s]; frames += advance(g, c, offsets[s + 1] - offsets[s], flush && flush[s]).frames; }
            if (frames > raw_capacity) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "lseend stream: %lld raw rows, room for %lld", (long long)frames, (long long)raw_capacity);
        }
        fa::DevBuf d_pcm, d_win, d_masks, d_warm, d_or, d_raw;
        FA_TRY(fa::take(ctx, "fa_lseend_stream_push", {{&d_pcm, sizeof(float) * ns, true, pcm}, {&d_win, sizeof(float) * cap * g.mel_frames * g.n_mels}, {&d_masks, sizeof(float) * cap * g.chunk, masks != nullptr},
                                                       {&d_warm, sizeof(int32_t) * cap, warmups != nullptr}, {&d_or, sizeof(int64_t) * cap, out_rows != nullptr},
                                                       {&d_raw, sizeof(float) * static_cast<size_t>(st->max_frames) * g.n_mels, raw != nullptr}}));
        FA_TRY(fa_lseend_stream_push_dev(ctx, st, d_pcm.as<float>(), offsets, flush, window_capacity, d_win.as<float>(), d_masks.as<float>(), d_warm.as<int32_t>(), d_or.as<int64_t>(),
                                         d_raw.as<float>(), plans));
        const fa_lseend_item_plan &last = plans[st->streams - 1];
        const size_t W = static_cast<size_t>(last.window0 + last.windows), F = static_cast<size_t>(last.frame0 + last.frames);
        if (W && !windows) return FA_INVALID_ARGUMENT;
        if (W) FA_HIP_TRY(ctx, hipMemcpyAsync(windows, d_win.p, sizeof(float) * W * g.mel_frames * g.n_mels, hipMemcpyDeviceToHost, ctx->stream));
        if (masks && W) FA_HIP_TRY(ctx, hipMemcpyAsync(masks, d_masks.p, sizeof(float) * W * g.chunk, hipMemcpyDeviceToHost, ctx->stream));
        if (warmups && W) FA_HIP_TRY(ctx, hipMemcpyAsync(warmups, d_warm.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, ctx->stream));
        if (out_rows && W) FA_HIP_TRY(ctx, hipMemcpyAsync(out_rows, d_or.p, sizeof(int64_t) * W, hipMemcpyDeviceToHost, ctx->stream));
        if (raw && F) FA_HIP_TRY(ctx, hipMemcpyAsync(raw, d_raw.p, sizeof(float) * F * g.n_mels, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_lseend_stream_get(fa_ctx *ctx, fa_lseend_stream *st, int32_t stream, fa_lseend_stream_info *info, float *audio_tail, float *mel_tail, double *sums) {
    if (!ctx || !st || ctx != st->ctx || stream < 0 || stream >= st->streams || !info) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    const Geometry &g = st->g;
    const Counters &c = st->cnt[stream];
    info->audio_samples = c.audio - g.n_fft / 2; info->frames = c.frames; info->windows = c.windows;
    info->unread_audio = static_cast<int32_t>(unread_audio(g, c)); info->unread_mel_rows = static_cast<int32_t>(unread_mel(g, c));
    info->decoder_mask_end = mask_end_of(g, c.windows); info->reserved = 0;
    const int par = st->parity[stream];
    const size_t ab = sizeof(float) * info->unread_audio, mb = sizeof(float) * info->unread_mel_rows * g.n_mels, sb = sizeof(double) * g.n_mels;
    if (st->is_fresh[stream]) {   // the seeds: zeros
        if (audio_tail) memset(audio_tail, 0, ab);
        if (mel_tail) memset(mel_tail, 0, mb);
        if (sums) memset(sums, 0, sb);
        return FA_SUCCESS;
    }
    if (audio_tail && ab) FA_HIP_TRY(ctx, hipMemcpyAsync(audio_tail, st->tail(stream, par), ab, hipMemcpyDeviceToHost, ctx->stream));
    if (mel_tail && mb) FA_HIP_TRY(ctx, hipMemcpyAsync(mel_tail, st->mel(stream, par), mb, hipMemcpyDeviceToHost, ctx->stream));
    if (sums) FA_HIP_TRY(ctx, hipMemcpyAsync(sums, st->sum(stream, par), sb, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_lseend_stream_set(fa_ctx *ctx, fa_lseend_stream *st, int32_t stream, const fa_lseend_stream_info *info, const float *audio_tail, const float *mel_tail,
                               const double *sums) {
    if (!ctx || !st || ctx != st->ctx || stream < 0 || stream >= st->streams || !info || !sums || info->audio_samples < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    const Geometry &g = st->g;
    const Counters c{g.n_fft / 2 + info->audio_samples, info->frames, info->windows};
    if (c.frames != frames_of(g, c.audio) || c.windows != windows_of(g, c.frames)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "lseend stream: not a state the queues reach");
    const int par = st->parity[stream];
    const size_t ab = sizeof(float) * unread_audio(g, c), mb = sizeof(float) * unread_mel(g, c) * g.n_mels;
    if ((ab && !audio_tail) || (mb && !mel_tail)) return FA_INVALID_ARGUMENT;
    if (ab) FA_HIP_TRY(ctx, hipMemcpyAsync(st->tail(stream, par), audio_tail, ab, hipMemcpyHostToDevice, ctx->stream));
    if (mb) FA_HIP_TRY(ctx, hipMemcpyAsync(st->mel(stream, par), mel_tail, mb, hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(st->sum(stream, par), sums, sizeof(double) * g.n_mels, hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the caller's arrays are free again
    st->cnt[stream] = c; st->is_fresh[stream] = 0;
    return FA_SUCCESS;
}

fa_status fa_lseend_gather_probs_dev(fa_ctx *ctx, const float *d_probs, int32_t windows, int32_t chunk_size, int32_t speakers, int64_t window_stride, int64_t row_stride,
                                     const int32_t *d_warmups, const int64_t *d_out_rows, float *d_out, int64_t out_capacity) {
    if (!ctx || windows < 0 || chunk_size < 1 || speakers < 1 || row_stride < speakers || window_stride < 0 || out_capacity < 0) return FA_INVALID_ARGUMENT;
    if (windows == 0) return FA_SUCCESS;
    if (!d_probs || !d_warmups || !d_out_rows || !d_out) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    GatherArgs a{d_probs, d_warmups, d_out_rows, d_out, window_stride, row_stride, out_capacity, windows, chunk_size, speakers};
    gather(a, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_lseend_gather_probs(fa_ctx *ctx, const float *probs, int32_t windows, int32_t chunk_size, int32_t speakers, int64_t window_stride, int64_t row_stride,
                                 const int32_t *warmups, const int64_t *out_rows, float *out, int64_t out_capacity) {
    if (!ctx || windows < 0 || chunk_size < 1 || speakers < 1 || row_stride < speakers || out_capacity < 0) return FA_INVALID_ARGUMENT;
    if (windows == 0) return FA_SUCCESS;
    if (!probs || !warmups || !out_rows || !out || window_stride < static_cast<int64_t>(chunk_size - 1) * row_stride + speakers) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_lseend_gather_probs", [&]() -> fa_status {
        const size_t W = static_cast<size_t>(windows), pf = (W - 1) * window_stride + static_cast<size_t>(chunk_size - 1) * row_stride + speakers, of = static_cast<size_t>(out_capacity) * speakers;
        fa::DevBuf d_probs, d_warm, d_or, d_out;
        FA_TRY(fa::take(ctx, "fa_lseend_gather_probs", {{&d_probs, sizeof(float) * pf, true, probs}, {&d_warm, sizeof(int32_t) * W, true, warmups}, {&d_or, sizeof(int64_t) * W, true, out_rows},
                                                        {&d_out, sizeof(float) * of, true, out}}));   // rows no window writes keep the caller's values
        FA_TRY(fa_lseend_gather_probs_dev(ctx, d_probs.as<float>(), windows, chunk_size, speakers, window_stride, row_stride, d_warm.as<int32_t>(), d_or.as<int64_t>(), d_out.as<float>(), out_capacity));
        if (of) FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, sizeof(float) * of, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

}  // extern "C"
