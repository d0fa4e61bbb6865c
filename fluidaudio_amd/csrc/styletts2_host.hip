// styletts2_host.hip — host side of the StyleTTS2 session (kernels: styletts2.hip): the tables (the centred periodic Hann and the HTK
// bank of StyleTTS2MelExtractor.swift:148-221, built in float32 as the reference builds them), the plan of styletts2_core.h as C records,
// the session with its slabs in HBM, the device entries and their host-pointer forms.  Nothing here waits for the device except
// fa_styletts2_durations_dev (the caller sizes the decoder's batch from the totals), fa_styletts2_session_get and the host-pointer forms;
// after fa_styletts2_session_create nothing is allocated by a device entry.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "styletts2_launch.h"

using namespace fa::styletts2;

namespace {

bool geometry_of(const fa_styletts2_config *c, Geometry &g) {
    if (!c || c->n_fft < 2 || c->win < 2 || c->win > c->n_fft || c->win % 2 || (c->n_fft - c->win) % 8 || c->hop < 4 || c->hop % 4 || c->n_mels < 1 || c->n_mels > kMaxMels ||
        c->filter_rate < 1 || c->max_ref_frames < 4 || c->max_ref_frames % 4 || c->max_ref_frames > (1 << 20) || c->default_tokens < 1 || c->n_buckets < 1 || c->n_buckets > kMaxBuckets ||
        c->style_dim < 2 || c->diffusion_steps < 2 || c->diffusion_steps > 64 || c->d_channels < 4 || c->d_channels % 4 || c->asr_channels < 4 || c->asr_channels % 4 ||
        c->d_channels > 65536 || c->asr_channels > 65536 || c->max_frames < 1 || c->max_frames > (1 << 24) || c->tail_trim < 0 || !(c->log_eps > 0.0f) || !std::isfinite(c->log_mean) || !(c->log_std > 0.0f) ||
        !(c->sigma_min > 0.0) || !(c->sigma_max > c->sigma_min) || !(c->rho > 0.0))
        return false;
    g = Geometry{};
    g.n_fft = c->n_fft; g.win = c->win; g.hop = c->hop; g.n_mels = c->n_mels; g.filter_rate = c->filter_rate; g.max_ref_frames = c->max_ref_frames;
    g.default_tokens = c->default_tokens; g.n_buckets = c->n_buckets; g.style_dim = c->style_dim; g.diffusion_steps = c->diffusion_steps;
    g.d_channels = c->d_channels; g.asr_channels = c->asr_channels; g.max_frames = c->max_frames; g.tail_trim = c->tail_trim;
    g.log_eps = c->log_eps; g.log_mean = c->log_mean; g.log_std = c->log_std;
    for (int i = 0; i < c->n_buckets; ++i) {
        if (c->buckets[i] < 1 || c->buckets[i] > kMaxTokens || (i && c->buckets[i] <= c->buckets[i - 1])) return false;
        g.buckets[i] = c->buckets[i];
    }
    return g.default_tokens <= g.buckets[g.n_buckets - 1];
}

int token_stride_of(const Geometry &g) { return g.buckets[g.n_buckets - 1]; }

// MelExtractor :148-158: the periodic Hann of `win` samples (the zeros round it are not stored)
void window_of(const Geometry &g, float *w) {
    const float two_pi = 3.14159265358979323846f * 2.0f, denom = static_cast<float>(g.win);
    for (int n = 0; n < g.win; ++n) w[n] = 0.5f * (1.0f - cosf(two_pi * static_cast<float>(n) / denom));
}

// MelExtractor :160-221 in float32: HTK scale, triangles, no normalisation, bin frequencies of the filter rate (16 kHz on 24 kHz audio, :10-16)
void bank_of(const Geometry &g, float *fb) {
    const int bins = g.n_fft / 2 + 1;
    auto hz_to_mel = [](const float hz) { return 2595.0f * log10f(1.0f + hz / 700.0f); };
    auto mel_to_hz = [](const float mel) { return 700.0f * (powf(10.0f, mel / 2595.0f) - 1.0f); };
    const float bin_step = static_cast<float>(g.filter_rate) / static_cast<float>(g.n_fft);
    const float mel_min = hz_to_mel(0.0f), mel_max = hz_to_mel(static_cast<float>(g.filter_rate) / 2.0f);
    std::vector<float> hz(static_cast<size_t>(g.n_mels) + 2);
    for (int i = 0; i < g.n_mels + 2; ++i) hz[i] = mel_to_hz(mel_min + (mel_max - mel_min) * (static_cast<float>(i) / static_cast<float>(g.n_mels + 1)));
    memset(fb, 0, sizeof(float) * static_cast<size_t>(g.n_mels) * bins);
    for (int m = 0; m < g.n_mels; ++m) {
        const float left = hz[m], center = hz[m + 1], right = hz[m + 2], up = center - left, down = right - center;
        for (int k = 0; k < bins; ++k) {
            const float f = static_cast<float>(k) * bin_step;
            if (f < left || f > right) continue;
            const float val = f <= center ? (up > 0.0f ? (f - left) / up : 0.0f) : (down > 0.0f ? (right - f) / down : 0.0f);
            fb[static_cast<size_t>(m) * bins + k] = val > 0.0f ? val : 0.0f;
        }
    }
}

fa_status plan_batch(const Geometry &g, const int32_t batch, const int64_t *samples, const int32_t *tokens, fa_styletts2_item_plan *items) {
    if (batch < 1 || !samples || !tokens || !items) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < batch; ++b) {
        if (samples[b] < 0 || tokens[b] < 0) return FA_INVALID_ARGUMENT;
        const ItemPlan p = plan_item(g, samples[b], tokens[b]);
        items[b] = fa_styletts2_item_plan{p.samples, p.ref_frames, p.tokens, p.bucket, p.status};
    }
    return FA_SUCCESS;
}

constexpr int kSlabs = 11;

}  // namespace

struct fa_styletts2_session {
    fa_ctx *ctx = nullptr;
    Geometry g{};
    int32_t batch = 0;
    bool planned = false, timed = false;   // timed: the durations of this plan are known
    std::vector<fa_styletts2_item_plan> items;
    std::vector<int32_t> totals, statuses;
    fa::DevBuf tables, slabs, work;
    fa_styletts2_slabs s{};
    MelArgs mel{};                 // geometry, constants and the pointers into `tables`
    // device copies of the calls' host arrays, inside `work`
    fa_styletts2_item_plan *d_items = nullptr;
    int64_t *d_offsets = nullptr, *d_token_offsets = nullptr, *d_ranges = nullptr;
    uint64_t *d_seeds = nullptr;
    float *d_alphas = nullptr, *d_betas = nullptr;
    size_t slab_bytes(const int which) const {
        const size_t B = static_cast<size_t>(batch), T = static_cast<size_t>(token_stride_of(g));
        switch (which) {
        case FA_STYLETTS2_SLAB_MEL: return B * g.n_mels * g.max_ref_frames * 4;
        case FA_STYLETTS2_SLAB_TOKENS: case FA_STYLETTS2_SLAB_ATTENTION_MASK: case FA_STYLETTS2_SLAB_DURATIONS: case FA_STYLETTS2_SLAB_STARTS: return B * T * 4;
        case FA_STYLETTS2_SLAB_NOISE_INIT: return B * kStyle * 4;
        case FA_STYLETTS2_SLAB_NOISES_AUX: return static_cast<size_t>(g.diffusion_steps - 1) * B * kStyle * 4;
        case FA_STYLETTS2_SLAB_REF: case FA_STYLETTS2_SLAB_S: return B * (kStyle / 2) * 4;
        case FA_STYLETTS2_SLAB_TOTAL_FRAMES: case FA_STYLETTS2_SLAB_STATUS: return B * 4;
        }
        return 0;
    }
    void *slab(const int which) const {
        void *const p[kSlabs] = {s.mel, s.tokens, s.attention_mask, s.noise_init, s.noises_aux, s.ref, s.s, s.durations, s.starts, s.total_frames, s.status};
        return which >= 0 && which < kSlabs ? p[which] : nullptr;
    }
};

namespace {

fa_status make_tables(fa_ctx *ctx, fa_styletts2_session &st) {
    const Geometry &g = st.g;
    std::vector<float> hann(g.win), fb(static_cast<size_t>(g.n_mels) * kBins), weights;
    window_of(g, hann.data());
    bank_of(g, fb.data());
    std::vector<int32_t> tab(2 * static_cast<size_t>(g.n_mels), 0);
    for (int m = 0; m < g.n_mels; ++m) {   // a row's support: first to last non-zero bin, interior zeros kept
        int l0 = -1, h0 = -1;
        for (int k = 0; k < kBins; ++k) if (fb[static_cast<size_t>(m) * kBins + k] != 0.0f) { if (l0 < 0) l0 = k; h0 = k; }
        const int cnt = l0 < 0 ? 0 : h0 - l0 + 1;
        tab[2 * m] = (l0 < 0 ? 0 : l0) | (cnt << 16);
        tab[2 * m + 1] = static_cast<int32_t>(weights.size());
        for (int j = 0; j < cnt; ++j) weights.push_back(fb[static_cast<size_t>(m) * kBins + l0 + j]);
    }
    if (weights.empty()) weights.push_back(0.0f);
    std::vector<float2> tw(kNfft + 1);
    for (int k = 0; k <= kNfft; ++k) { const double a = -2.0 * M_PI * k / kNfft; tw[k] = make_float2(static_cast<float>(cos(a)), static_cast<float>(sin(a))); }

    MelArgs &a = st.mel;
    a.n_mels = g.n_mels; a.hop = g.hop; a.win = g.win; a.lead = (g.n_fft - g.win) / 2; a.stride = g.max_ref_frames;
    a.log_eps = g.log_eps; a.log_mean = g.log_mean; a.log_std = g.log_std;
    if (mel_lds_bytes(a) > 64 * 1024) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2: tile does not fit LDS (hop %d, win %d)", g.hop, g.win);
    std::vector<char> img;
    auto add = [&img](const void *src, size_t bytes) { const size_t at = img.size(); img.resize((at + bytes + 255) & ~static_cast<size_t>(255), 0); memcpy(img.data() + at, src, bytes); return at; };
    const size_t o_win = add(hann.data(), sizeof(float) * hann.size()), o_tw = add(tw.data(), sizeof(float2) * tw.size());
    const size_t o_tab = add(tab.data(), sizeof(int32_t) * tab.size()), o_w = add(weights.data(), sizeof(float) * weights.size());
    FA_TRY(fa::take_once(ctx, "fa_styletts2_session_create", {{&st.tables, img.size()}}));
    FA_HIP_TRY(ctx, hipMemcpyAsync(st.tables.p, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    char *d = st.tables.as<char>();
    a.window = reinterpret_cast<const float *>(d + o_win); a.tw2048 = reinterpret_cast<const float2 *>(d + o_tw);
    a.mel_tab = reinterpret_cast<const int32_t *>(d + o_tab); a.mel_w = reinterpret_cast<const float *>(d + o_w);
    return FA_SUCCESS;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

fa_status ready(fa_ctx *ctx, const fa_styletts2_session *s) {
    if (!ctx || !s || ctx != s->ctx) return FA_INVALID_ARGUMENT;
    if (!s->planned) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2: fa_styletts2_session_begin has not planned a batch");
    return FA_SUCCESS;
}

int max_tokens_of(const fa_styletts2_session *s) {
    int n = 1;
    for (const fa_styletts2_item_plan &p : s->items) n = p.tokens > n ? p.tokens : n;
    return n;
}

}  // namespace

extern "C" {

void fa_styletts2_default_config(fa_styletts2_config *c) {   // StyleTTS2Constants.swift
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->sigma_min = 0.0001; c->sigma_max = 3.0; c->rho = 9.0;
    c->n_fft = 2048; c->win = 1200; c->hop = 300; c->n_mels = 80; c->filter_rate = 16000; c->max_ref_frames = 2400;
    c->default_tokens = 57; c->n_buckets = 3; c->buckets[0] = 64; c->buckets[1] = 128; c->buckets[2] = 256;
    c->style_dim = 256; c->diffusion_steps = 5; c->d_channels = 640; c->asr_channels = 512; c->max_frames = 4096; c->tail_trim = 50;
    c->log_eps = 1e-5f; c->log_mean = -4.0f; c->log_std = 4.0f;
}

fa_status fa_styletts2_plan(const fa_styletts2_config *cfg, int32_t batch, const int64_t *samples, const int32_t *tokens, fa_styletts2_item_plan *items) {
    Geometry g;
    if (!geometry_of(cfg, g)) return FA_INVALID_ARGUMENT;
    return plan_batch(g, batch, samples, tokens, items);
}

fa_status fa_styletts2_karras_sigmas(const fa_styletts2_config *cfg, int32_t steps, double *out) {
    Geometry g;
    if (!geometry_of(cfg, g) || steps < 2 || !out) return FA_INVALID_ARGUMENT;
    karras_sigmas(steps, cfg->sigma_min, cfg->sigma_max, cfg->rho, out);
    return FA_SUCCESS;
}

fa_status fa_styletts2_window(const fa_styletts2_config *cfg, float *out) {
    Geometry g;
    if (!geometry_of(cfg, g) || !out) return FA_INVALID_ARGUMENT;
    window_of(g, out);
    return FA_SUCCESS;
}

fa_status fa_styletts2_filterbank(const fa_styletts2_config *cfg, float *out) {
    Geometry g;
    if (!geometry_of(cfg, g) || !out) return FA_INVALID_ARGUMENT;
    bank_of(g, out);
    return FA_SUCCESS;
}

fa_status fa_styletts2_session_create(fa_ctx *ctx, const fa_styletts2_config *cfg, int32_t batch, fa_styletts2_session **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    Geometry g;
    if (!geometry_of(cfg, g) || batch < 1 || batch > 65535) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 session: unsupported configuration or batch");
    if (g.n_fft != kNfft || g.style_dim != kStyle) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2: n_fft %d, style width %d (this kernel generation serves 2048 and 256)", g.n_fft, g.style_dim);
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_session_create", [&]() -> fa_status {
        std::unique_ptr<fa_styletts2_session> st(new fa_styletts2_session());
        st->ctx = ctx; st->g = g; st->batch = batch;
        st->items.resize(batch); st->totals.assign(batch, 0); st->statuses.assign(batch, 0);
        FA_TRY(make_tables(ctx, *st));
        size_t at[kSlabs], total = 0;
        for (int w = 0; w < kSlabs; ++w) { at[w] = total; total += (st->slab_bytes(w) + 255) & ~static_cast<size_t>(255); }
        const size_t B = static_cast<size_t>(batch);
        auto up = [](const size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); };
        const size_t o_items = 0, o_off = o_items + up(B * sizeof(fa_styletts2_item_plan)), o_tok = o_off + up((B + 1) * 8), o_rng = o_tok + up((B + 1) * 8);
        const size_t o_seed = o_rng + up((B + 1) * 8), o_alpha = o_seed + up(B * 8), o_beta = o_alpha + up(B * 4);
        FA_TRY(fa::take_once(ctx, "fa_styletts2_session_create", {{&st->slabs, total}, {&st->work, o_beta + up(B * 4)}}));
        char *d = st->slabs.as<char>(), *wk = st->work.as<char>();
        fa_styletts2_slabs &s = st->s;
        s.mel = reinterpret_cast<float *>(d + at[0]); s.tokens = reinterpret_cast<int32_t *>(d + at[1]); s.attention_mask = reinterpret_cast<int32_t *>(d + at[2]);
        s.noise_init = reinterpret_cast<float *>(d + at[3]); s.noises_aux = reinterpret_cast<float *>(d + at[4]); s.ref = reinterpret_cast<float *>(d + at[5]);
        s.s = reinterpret_cast<float *>(d + at[6]); s.durations = reinterpret_cast<int32_t *>(d + at[7]); s.starts = reinterpret_cast<int32_t *>(d + at[8]);
        s.total_frames = reinterpret_cast<int32_t *>(d + at[9]); s.status = reinterpret_cast<int32_t *>(d + at[10]);
        st->d_items = reinterpret_cast<fa_styletts2_item_plan *>(wk + o_items); st->d_offsets = reinterpret_cast<int64_t *>(wk + o_off);
        st->d_token_offsets = reinterpret_cast<int64_t *>(wk + o_tok); st->d_ranges = reinterpret_cast<int64_t *>(wk + o_rng);
        st->d_seeds = reinterpret_cast<uint64_t *>(wk + o_seed); st->d_alphas = reinterpret_cast<float *>(wk + o_alpha); st->d_betas = reinterpret_cast<float *>(wk + o_beta);
        st->mel.mel = s.mel; st->mel.items = st->d_items; st->mel.offsets = st->d_offsets;
        *out = st.release();
        return FA_SUCCESS;
    });
}

void fa_styletts2_session_destroy(fa_styletts2_session *s) {
    if (!s) return;
    if (s->slabs.p) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    delete s;
}

fa_status fa_styletts2_session_slabs(fa_styletts2_session *s, fa_styletts2_slabs *out) {
    if (!s || !out) return FA_INVALID_ARGUMENT;
    *out = s->s;
    return FA_SUCCESS;
}

fa_status fa_styletts2_session_begin(fa_ctx *ctx, fa_styletts2_session *s, const int64_t *samples, const int32_t *tokens, fa_styletts2_item_plan *items) {
    if (!ctx || !s || ctx != s->ctx) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    s->planned = s->timed = false;
    FA_TRY(plan_batch(s->g, s->batch, samples, tokens, s->items.data()));
    // (here and below the source is pageable host memory: the copy has left it when the call returns)
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_items, s->items.data(), sizeof(fa_styletts2_item_plan) * s->items.size(), hipMemcpyHostToDevice, ctx->stream));
    if (items) memcpy(items, s->items.data(), sizeof(fa_styletts2_item_plan) * s->items.size());
    s->planned = true;
    return FA_SUCCESS;
}

fa_status fa_styletts2_session_get(fa_ctx *ctx, fa_styletts2_session *s, int32_t slab, void *out) {
    if (!ctx || !s || ctx != s->ctx || !out || !s->slab(slab)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(out, s->slab(slab), s->slab_bytes(slab), hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_styletts2_reference_mel_dev(fa_ctx *ctx, fa_styletts2_session *s, const float *d_pcm, const int64_t *offsets) {
    FA_TRY(ready(ctx, s));
    if (!offsets) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < s->batch; ++b)
        if (offsets[b] < 0 || offsets[b + 1] - offsets[b] < s->items[b].samples) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 reference mel: item %d has fewer samples than planned", b);
    if (offsets[s->batch] > 0 && !d_pcm) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_offsets, offsets, sizeof(int64_t) * (s->batch + 1), hipMemcpyHostToDevice, ctx->stream));
    MelArgs a = s->mel;
    a.pcm = d_pcm; a.vec = aligned16(d_pcm);
    run_reference_mel(a, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_styletts2_inputs_dev(fa_ctx *ctx, fa_styletts2_session *s, const int32_t *d_token_ids, const int64_t *token_offsets, const uint64_t *seeds) {
    FA_TRY(ready(ctx, s));
    if (!token_offsets || !seeds) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < s->batch; ++b)
        if (token_offsets[b] < 0 || token_offsets[b + 1] - token_offsets[b] < s->items[b].tokens) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 inputs: item %d has fewer token ids than planned", b);
    if (token_offsets[s->batch] > 0 && !d_token_ids) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_token_offsets, token_offsets, sizeof(int64_t) * (s->batch + 1), hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_seeds, seeds, sizeof(uint64_t) * s->batch, hipMemcpyHostToDevice, ctx->stream));
    run_inputs(InputArgs{s->d_items, d_token_ids, s->d_token_offsets, s->d_seeds, s->s, s->batch, token_stride_of(s->g), s->g.diffusion_steps - 1}, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_styletts2_blend_dev(fa_ctx *ctx, fa_styletts2_session *s, const float *d_s_pred, int64_t s_pred_stride, const float *d_ref_s, int64_t ref_s_stride,
                                 const float *alphas, const float *betas) {
    FA_TRY(ready(ctx, s));
    if (!d_s_pred || !d_ref_s || !alphas || !betas || s_pred_stride < 0 || ref_s_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_alphas, alphas, sizeof(float) * s->batch, hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_betas, betas, sizeof(float) * s->batch, hipMemcpyHostToDevice, ctx->stream));
    run_blend(BlendArgs{d_s_pred, d_ref_s, s->d_alphas, s->d_betas, s_pred_stride, ref_s_stride, s->s}, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_styletts2_durations_dev(fa_ctx *ctx, fa_styletts2_session *s, const float *d_logits, int32_t channels, int64_t item_stride, int64_t token_stride, int64_t channel_stride,
                                     int32_t *total_frames, int32_t *statuses) {
    FA_TRY(ready(ctx, s));
    if (!d_logits || channels < 1 || channels > kMaxChannels || item_stride < 0 || token_stride < 0 || channel_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    s->timed = false;
    run_durations(DurationArgs{s->d_items, d_logits, item_stride, token_stride, channel_stride, s->s, channels, token_stride_of(s->g), s->g.max_frames}, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->totals.data(), s->s.total_frames, sizeof(int32_t) * s->batch, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->statuses.data(), s->s.status, sizeof(int32_t) * s->batch, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the session's one wait: the totals size the decoder's batch
    if (total_frames) memcpy(total_frames, s->totals.data(), sizeof(int32_t) * s->batch);
    if (statuses) memcpy(statuses, s->statuses.data(), sizeof(int32_t) * s->batch);
    s->timed = true;
    return FA_SUCCESS;
}

fa_status fa_styletts2_align_dev(fa_ctx *ctx, fa_styletts2_session *s, const float *d_d, int64_t d_row_stride, int64_t d_item_stride, const float *d_t_en, int64_t t_row_stride,
                                 int64_t t_item_stride, int32_t shift, float *d_en, float *d_asr, int32_t frame_stride) {
    FA_TRY(ready(ctx, s));
    if (!s->timed) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 align: fa_styletts2_durations has not run on this plan");
    if (!d_d || !d_t_en || !d_en || !d_asr || d_row_stride < s->g.d_channels || t_row_stride < max_tokens_of(s) || d_item_stride < 0 || t_item_stride < 0 || frame_stride < 1) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < s->batch; ++b)
        if (s->statuses[b] == kOk && s->totals[b] > frame_stride) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 align: item %d has %d frames, the stride is %d", b, s->totals[b], frame_stride);
    fa::DeviceGuard guard(ctx->device);
    AlignArgs a{};
    a.items = s->d_items; a.d = d_d; a.t_en = d_t_en; a.d_row_stride = d_row_stride; a.d_item_stride = d_item_stride; a.t_row_stride = t_row_stride; a.t_item_stride = t_item_stride;
    a.en = d_en; a.asr = d_asr; a.s = s->s; a.d_channels = s->g.d_channels; a.asr_channels = s->g.asr_channels; a.d_slabs = (s->g.d_channels + kAlignChannels - 1) / kAlignChannels;
    a.frame_stride = frame_stride; a.token_stride = token_stride_of(s->g); a.shift = shift != 0;
    a.vec_d = aligned16(d_d) && d_row_stride % 4 == 0 && d_item_stride % 4 == 0;
    a.vec_out = aligned16(d_en) && aligned16(d_asr) && frame_stride % 4 == 0;
    run_align(a, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_styletts2_finish_dev(fa_ctx *ctx, fa_styletts2_session *s, const float *d_audio, int64_t row_stride, const int64_t *lengths, float *d_out, int64_t *out_offsets) {
    FA_TRY(ready(ctx, s));
    if (!lengths || !out_offsets || row_stride < 0) return FA_INVALID_ARGUMENT;
    int64_t longest = 0;
    out_offsets[0] = 0;
    for (int b = 0; b < s->batch; ++b) {   // Synthesizer :127-132; the items land back to back in their order
        if (lengths[b] < 0 || lengths[b] > row_stride) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 finish: item %d has %lld samples in a row of %lld", b, (long long)lengths[b], (long long)row_stride);
        const int64_t keep = trimmed_length(s->g, lengths[b]);
        out_offsets[b + 1] = out_offsets[b] + keep;
        longest = keep > longest ? keep : longest;
    }
    if (longest == 0) return FA_SUCCESS;
    if (!d_audio || !d_out) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_ranges, out_offsets, sizeof(int64_t) * (s->batch + 1), hipMemcpyHostToDevice, ctx->stream));
    run_finish(FinishArgs{d_audio, s->d_ranges, d_out, row_stride, aligned16(d_audio) && aligned16(d_out)}, s->batch, longest, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

// ---- host-pointer forms: upload, run, fetch, one synchronisation
fa_status fa_styletts2_reference_mel(fa_ctx *ctx, fa_styletts2_session *s, const float *pcm, const int64_t *offsets) {
    FA_TRY(ready(ctx, s));
    if (!offsets || offsets[s->batch] < 0 || (offsets[s->batch] > 0 && !pcm)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_reference_mel", [&]() -> fa_status {
        fa::DevBuf d_pcm;
        FA_TRY(fa::take(ctx, "fa_styletts2_reference_mel", {{&d_pcm, sizeof(float) * static_cast<size_t>(offsets[s->batch]), true, pcm}}));
        FA_TRY(fa_styletts2_reference_mel_dev(ctx, s, d_pcm.as<float>(), offsets));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_styletts2_inputs(fa_ctx *ctx, fa_styletts2_session *s, const int32_t *token_ids, const int64_t *token_offsets, const uint64_t *seeds) {
    FA_TRY(ready(ctx, s));
    if (!token_offsets || token_offsets[s->batch] < 0 || (token_offsets[s->batch] > 0 && !token_ids)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_inputs", [&]() -> fa_status {
        fa::DevBuf d_ids;
        FA_TRY(fa::take(ctx, "fa_styletts2_inputs", {{&d_ids, sizeof(int32_t) * static_cast<size_t>(token_offsets[s->batch]), true, token_ids}}));
        FA_TRY(fa_styletts2_inputs_dev(ctx, s, d_ids.as<int32_t>(), token_offsets, seeds));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_styletts2_blend(fa_ctx *ctx, fa_styletts2_session *s, const float *s_pred, int64_t s_pred_stride, const float *ref_s, int64_t ref_s_stride, const float *alphas,
                             const float *betas) {
    FA_TRY(ready(ctx, s));
    if (!s_pred || !ref_s || s_pred_stride < 0 || ref_s_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_blend", [&]() -> fa_status {
        const size_t B1 = static_cast<size_t>(s->batch - 1);
        fa::DevBuf d_p, d_r;
        FA_TRY(fa::take(ctx, "fa_styletts2_blend", {{&d_p, sizeof(float) * (B1 * s_pred_stride + kStyle), true, s_pred}, {&d_r, sizeof(float) * (B1 * ref_s_stride + kStyle), true, ref_s}}));
        FA_TRY(fa_styletts2_blend_dev(ctx, s, d_p.as<float>(), s_pred_stride, d_r.as<float>(), ref_s_stride, alphas, betas));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_styletts2_durations(fa_ctx *ctx, fa_styletts2_session *s, const float *logits, int32_t channels, int64_t item_stride, int64_t token_stride, int64_t channel_stride,
                                 int32_t *total_frames, int32_t *statuses) {
    FA_TRY(ready(ctx, s));
    if (!logits || channels < 1 || item_stride < 0 || token_stride < 0 || channel_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_durations", [&]() -> fa_status {
        const size_t floats = static_cast<size_t>(s->batch - 1) * item_stride + static_cast<size_t>(max_tokens_of(s) - 1) * token_stride + static_cast<size_t>(channels - 1) * channel_stride + 1;
        fa::DevBuf d;
        FA_TRY(fa::take(ctx, "fa_styletts2_durations", {{&d, sizeof(float) * floats, true, logits}}));
        return fa_styletts2_durations_dev(ctx, s, d.as<float>(), channels, item_stride, token_stride, channel_stride, total_frames, statuses);
    });
}

fa_status fa_styletts2_align(fa_ctx *ctx, fa_styletts2_session *s, const float *d, int64_t d_row_stride, int64_t d_item_stride, const float *t_en, int64_t t_row_stride,
                             int64_t t_item_stride, int32_t shift, float *en, float *asr, int32_t frame_stride) {
    FA_TRY(ready(ctx, s));
    if (!d || !t_en || !en || !asr || d_row_stride < s->g.d_channels || t_row_stride < 1 || d_item_stride < 0 || t_item_stride < 0 || frame_stride < 1) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_align", [&]() -> fa_status {
        const size_t B = static_cast<size_t>(s->batch), n = static_cast<size_t>(max_tokens_of(s));
        const size_t d_floats = (B - 1) * d_item_stride + (n - 1) * d_row_stride + s->g.d_channels, t_floats = (B - 1) * t_item_stride + static_cast<size_t>(s->g.asr_channels - 1) * t_row_stride + n;
        const size_t en_bytes = sizeof(float) * B * s->g.d_channels * frame_stride, asr_bytes = sizeof(float) * B * s->g.asr_channels * frame_stride;
        fa::DevBuf d_d, d_t, d_en, d_asr;
        FA_TRY(fa::take(ctx, "fa_styletts2_align", {{&d_d, sizeof(float) * d_floats, true, d}, {&d_t, sizeof(float) * t_floats, true, t_en}, {&d_en, en_bytes}, {&d_asr, asr_bytes}}));
        FA_TRY(fa_styletts2_align_dev(ctx, s, d_d.as<float>(), d_row_stride, d_item_stride, d_t.as<float>(), t_row_stride, t_item_stride, shift, d_en.as<float>(), d_asr.as<float>(), frame_stride));
        FA_HIP_TRY(ctx, hipMemcpyAsync(en, d_en.p, en_bytes, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipMemcpyAsync(asr, d_asr.p, asr_bytes, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_styletts2_finish(fa_ctx *ctx, fa_styletts2_session *s, const float *audio, int64_t row_stride, const int64_t *lengths, float *out, int64_t out_capacity,
                              int64_t *out_offsets) {
    FA_TRY(ready(ctx, s));
    if (!lengths || !out_offsets || row_stride < 0 || out_capacity < 0) return FA_INVALID_ARGUMENT;
    int64_t total = 0;
    for (int b = 0; b < s->batch; ++b) total += lengths[b] > 0 ? trimmed_length(s->g, lengths[b]) : 0;
    if (total > out_capacity) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "styletts2 finish: %lld samples for a capacity of %lld", (long long)total, (long long)out_capacity);
    if (total > 0 && (!audio || !out)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_styletts2_finish", [&]() -> fa_status {
        fa::DevBuf d_audio, d_out;
        FA_TRY(fa::take(ctx, "fa_styletts2_finish", {{&d_audio, sizeof(float) * static_cast<size_t>(s->batch) * row_stride, total > 0, audio}, {&d_out, sizeof(float) * static_cast<size_t>(total), total > 0}}));
        FA_TRY(fa_styletts2_finish_dev(ctx, s, d_audio.as<float>(), row_stride, lengths, d_out.as<float>(), out_offsets));
        if (total > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, sizeof(float) * static_cast<size_t>(total), hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

}  // extern "C"
