// luxtts_host.hip — host side of the LuxTTS session (kernels: luxtts.hip): the tables (the mel featurizer's own periodic Hann and HTK
// bank, through its C entries), the plan of luxtts_core.h as C records, the session with its slabs in HBM, the device entries and their
// host-pointer forms.  Nothing here waits for the device except fa_luxtts_session_get and the host-pointer forms; after
// fa_luxtts_session_create nothing is allocated by a device entry.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "luxtts_launch.h"

using namespace fa::luxtts;

namespace {

bool geometry_of(const fa_luxtts_config *c, Geometry &g) {
    if (!c || c->sample_rate < 1 || c->hop < 1 || c->n_mels < 4 || c->n_mels > kMaxMels || c->n_mels % 4 || c->max_tokens < 2 || c->max_frames < kTileFrames || c->max_frames % kTileFrames || c->max_frames > 65536 ||
        c->max_tokens > 65536 || c->n_buckets < 1 || c->n_buckets > kMaxBuckets || c->out_hop < 1 || c->num_steps < 1 || c->num_steps > kMaxSteps ||
        !(c->log_floor > 0.0f) || !(c->feat_scale > 0.0f) || !(c->target_rms >= 0.0f) || !(c->max_prompt_seconds > 0.0) || !(c->max_prompt_seconds <= 3600.0) || !std::isfinite(c->t_shift))
        return false;
    g = Geometry{};
    g.sample_rate = c->sample_rate; g.n_fft = c->n_fft; g.hop = c->hop; g.n_mels = c->n_mels; g.max_tokens = c->max_tokens; g.max_frames = c->max_frames;
    g.n_buckets = c->n_buckets; g.out_hop = c->out_hop; g.num_steps = c->num_steps;
    for (int i = 0; i < c->n_buckets; ++i) {
        if (c->buckets[i] < 1 || c->buckets[i] > c->max_frames || (i && c->buckets[i] <= c->buckets[i - 1])) return false;
        g.buckets[i] = c->buckets[i];
    }
    g.max_prompt_samples = static_cast<int64_t>(c->max_prompt_seconds * static_cast<double>(c->sample_rate));   // Synthesizer :71-72
    g.t_shift = c->t_shift; g.log_floor = c->log_floor; g.feat_scale = c->feat_scale; g.target_rms = c->target_rms;
    return g.max_prompt_samples >= 1;
}

fa_luxtts_item_plan record_of(const ItemPlan &p) {
    return fa_luxtts_item_plan{p.samples, p.sample_count, p.prompt_frames, p.tokens, p.features_length, p.gen_frames, p.avg, p.bucket, p.status, 0};
}

fa_status plan_batch(const Geometry &g, const int32_t batch, const int64_t *prompt_samples, const int32_t *prompt_tokens, const int32_t *text_tokens, const float *speeds,
                     fa_luxtts_item_plan *items) {
    if (batch < 1 || !prompt_samples || !prompt_tokens || !text_tokens || !speeds || !items) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < batch; ++b) {
        if (prompt_tokens[b] < 1 || text_tokens[b] < 1 || prompt_samples[b] < 0) return FA_INVALID_ARGUMENT;
        items[b] = record_of(refused(plan_item(g, prompt_samples[b], prompt_tokens[b], text_tokens[b], speeds[b])));
    }
    return FA_SUCCESS;
}

}  // namespace

struct fa_luxtts_session {
    fa_ctx *ctx = nullptr;
    Geometry g{};
    int32_t batch = 0;
    bool planned = false;
    std::vector<fa_luxtts_item_plan> items;
    fa::DevBuf tables, slabs, work;
    fa_luxtts_slabs s{};
    MelArgs mel{};                 // geometry, constants and the pointers into `tables`
    // device copies of the calls' host arrays, inside `work`
    fa_luxtts_item_plan *d_items = nullptr;
    int64_t *d_offsets = nullptr, *d_token_offsets = nullptr, *d_sample_offsets = nullptr;
    uint64_t *d_seeds = nullptr;
    int32_t *d_list = nullptr;     // [n_buckets][batch]
    size_t slab_bytes(const int which) const {
        const size_t B = static_cast<size_t>(batch), rows = B * g.max_frames * g.n_mels * sizeof(float);
        switch (which) {
        case FA_LUXTTS_SLAB_TOKENS: case FA_LUXTTS_SLAB_TOKEN_MASK: return B * g.max_tokens * 4;
        case FA_LUXTTS_SLAB_TEXT_CONDITION: case FA_LUXTTS_SLAB_SPEECH_CONDITION: case FA_LUXTTS_SLAB_X: return rows;
        case FA_LUXTTS_SLAB_FRAME_MASK: return B * g.max_frames * 4;
        case FA_LUXTTS_SLAB_RECORDS: return B * sizeof(fa_luxtts_record);
        }
        return 0;
    }
    void *slab(const int which) const {
        void *const p[] = {s.tokens, s.token_mask, s.text_condition, s.speech_condition, s.x, s.frame_mask, s.records};
        return which >= 0 && which < 7 ? p[which] : nullptr;
    }
};

namespace {

// the window and the bank are the mel featurizer's (fa_mel_hann_window / fa_mel_filterbank in the LuxTTS flavour of LuxTtsMelExtractor.swift:143-187)
fa_status make_tables(fa_ctx *ctx, const fa_luxtts_config *cfg, fa_luxtts_session &st) {
    const Geometry &g = st.g;
    fa_mel_config mc;
    fa_mel_default_config(&mc);
    mc.sample_rate = g.sample_rate; mc.n_mels = g.n_mels; mc.n_fft = g.n_fft; mc.hop = g.hop; mc.win = g.n_fft;
    mc.preemph = 0.0f; mc.pad_to = 0; mc.log_floor = g.log_floor; mc.floor_mode = FA_MEL_FLOOR_CLAMPED; mc.window_periodic = 1; mc.padding_mode = FA_MEL_PAD_CENTER;
    mc.power = 1.0f; mc.center_pad = FA_MEL_CENTER_REFLECT; mc.mel_scale = FA_MEL_SCALE_HTK_NONORM; mc.tail_mode = FA_MEL_TAIL_REPLICATE;
    std::vector<float> hann(kNfft), fb(static_cast<size_t>(g.n_mels) * kBins), weights;
    FA_TRY(fa_mel_hann_window(&mc, hann.data()));
    FA_TRY(fa_mel_filterbank(&mc, fb.data()));
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
    std::vector<float2> tw(kNfft);
    for (int k = 0; k < kNfft; ++k) { const double a = -2.0 * M_PI * k / kNfft; tw[k] = make_float2(static_cast<float>(cos(a)), static_cast<float>(sin(a))); }

    std::vector<float> undo(kBins, 0.0f);
    for (int k = 1; k < kBins; ++k) undo[k] = static_cast<float>(1.0 / (2.0 * sin(M_PI * k / kNfft)));

    MelArgs &a = st.mel;
    a.n_weights = static_cast<int32_t>(weights.size()); a.n_mels = g.n_mels; a.hop = g.hop; a.max_frames = g.max_frames;
    a.log_floor = g.log_floor; a.feat_scale = g.feat_scale; a.target_rms = g.target_rms;
    if (mel_lds_bytes(a) > 64 * 1024) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts: tile does not fit LDS (hop %d)", g.hop);
    std::vector<char> img;
    auto add = [&img](const void *src, size_t bytes) { const size_t at = img.size(); img.resize((at + bytes + 255) & ~static_cast<size_t>(255), 0); memcpy(img.data() + at, src, bytes); return at; };
    const size_t o_win = add(hann.data(), sizeof(float) * hann.size()), o_tw = add(tw.data(), sizeof(float2) * tw.size());
    const size_t o_tab = add(tab.data(), sizeof(int32_t) * tab.size()), o_w = add(weights.data(), sizeof(float) * weights.size()), o_undo = add(undo.data(), sizeof(float) * undo.size());
    FA_TRY(fa::take_once(ctx, "fa_luxtts_session_create", {{&st.tables, img.size()}}));
    FA_HIP_TRY(ctx, hipMemcpyAsync(st.tables.p, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    char *d = st.tables.as<char>();
    a.window = reinterpret_cast<const float *>(d + o_win); a.tw1024 = reinterpret_cast<const float2 *>(d + o_tw);
    a.mel_tab = reinterpret_cast<const int32_t *>(d + o_tab); a.mel_w = reinterpret_cast<const float *>(d + o_w);
    a.undo = reinterpret_cast<const float *>(d + o_undo);
    return FA_SUCCESS;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

fa_status ready(fa_ctx *ctx, const fa_luxtts_session *s) {
    if (!ctx || !s || ctx != s->ctx) return FA_INVALID_ARGUMENT;
    if (!s->planned) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts: fa_luxtts_session_begin has not planned a batch");
    return FA_SUCCESS;
}

RowArgs row_args(const fa_luxtts_session *s, const float *src, const int64_t row_stride, const int64_t item_stride) {
    RowArgs a{};
    a.items = s->d_items; a.src = src; a.row_stride = row_stride; a.item_stride = item_stride; a.s = s->s;
    a.n_mels = s->g.n_mels; a.max_frames = s->g.max_frames;
    a.vec = aligned16(src) && row_stride % 4 == 0 && item_stride % 4 == 0;
    return a;
}

// floats behind a strided [batch][rows][row_stride] host operand
size_t strided_floats(const fa_luxtts_session *s, const int64_t row_stride, const int64_t item_stride, const int64_t rows) {
    return static_cast<size_t>(s->batch - 1) * item_stride + static_cast<size_t>(rows - 1) * row_stride + s->g.n_mels;
}

}  // namespace

extern "C" {

void fa_luxtts_default_config(fa_luxtts_config *c) {   // LuxTtsConstants.swift
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->t_shift = 0.5; c->max_prompt_seconds = 5.0;
    c->sample_rate = 24000; c->n_fft = 1024; c->hop = 256; c->n_mels = 100; c->max_tokens = 256; c->max_frames = 1024;
    c->n_buckets = 2; c->buckets[0] = 282; c->buckets[1] = 555; c->out_hop = 512; c->num_steps = 4;
    c->log_floor = 1e-7f; c->feat_scale = 0.1f; c->target_rms = 0.1f;
}

fa_status fa_luxtts_plan(const fa_luxtts_config *cfg, int32_t batch, const int64_t *prompt_samples, const int32_t *prompt_tokens, const int32_t *text_tokens,
                         const float *speeds, fa_luxtts_item_plan *items, int32_t *bucket_counts, int32_t *bucket_items) {
    Geometry g;
    if (!geometry_of(cfg, g)) return FA_INVALID_ARGUMENT;
    FA_TRY(plan_batch(g, batch, prompt_samples, prompt_tokens, text_tokens, speeds, items));
    for (int k = 0; k < g.n_buckets; ++k) {
        int32_t n = 0;
        for (int b = 0; b < batch; ++b)
            if (items[b].status == kOk && items[b].bucket == g.buckets[k]) { if (bucket_items) bucket_items[static_cast<int64_t>(k) * batch + n] = b; ++n; }
        if (bucket_counts) bucket_counts[k] = n;
    }
    return FA_SUCCESS;
}

fa_status fa_luxtts_time_steps(const fa_luxtts_config *cfg, double *out) {
    Geometry g;
    if (!geometry_of(cfg, g) || !out) return FA_INVALID_ARGUMENT;
    for (int i = 0; i <= g.num_steps; ++i) out[i] = time_step(g, i);
    return FA_SUCCESS;
}

fa_status fa_luxtts_prompt_loudness(const fa_luxtts_config *cfg, const float *pcm, int64_t n, fa_luxtts_record *out) {
    Geometry g;
    if (!geometry_of(cfg, g) || !pcm || n < 1 || !out) return FA_INVALID_ARGUMENT;
    const Loudness r = loudness_of(mean_square(pcm, n < g.max_prompt_samples ? n : g.max_prompt_samples), g.target_rms);
    *out = fa_luxtts_record{r.mean_square, r.rms, r.gain, r.status};
    return FA_SUCCESS;
}

fa_status fa_luxtts_anchor_euler(const fa_luxtts_config *cfg, int32_t step, float *x, const float *v, int64_t n) {
    Geometry g;
    if (!geometry_of(cfg, g) || step < 0 || step >= g.num_steps || n < 0 || (n && (!x || !v))) return FA_INVALID_ARGUMENT;
    const StepTimes t = step_times(g, step);
    for (int64_t i = 0; i < n; ++i) x[i] = anchor_euler(x[i], v[i], t);
    return FA_SUCCESS;
}

fa_status fa_luxtts_session_create(fa_ctx *ctx, const fa_luxtts_config *cfg, int32_t batch, fa_luxtts_session **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    Geometry g;
    if (!geometry_of(cfg, g) || batch < 1 || batch > 65535) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts session: unsupported configuration or batch");
    if (g.n_fft != kNfft) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts: n_fft %d (this kernel generation serves 1024)", g.n_fft);
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_session_create", [&]() -> fa_status {
        std::unique_ptr<fa_luxtts_session> st(new fa_luxtts_session());
        st->ctx = ctx; st->g = g; st->batch = batch;
        st->items.resize(batch);
        FA_TRY(make_tables(ctx, cfg, *st));
        size_t at[8], total = 0;
        for (int w = 0; w < 7; ++w) { at[w] = total; total += (st->slab_bytes(w) + 255) & ~static_cast<size_t>(255); }
        const size_t B = static_cast<size_t>(batch), pad = 256;
        const size_t o_items = 0, o_off = o_items + ((B * sizeof(fa_luxtts_item_plan) + pad - 1) & ~(pad - 1)), o_tok = o_off + (((B + 1) * 8 + pad - 1) & ~(pad - 1));
        const size_t o_smp = o_tok + (((B + 1) * 8 + pad - 1) & ~(pad - 1)), o_seed = o_smp + (((B + 1) * 8 + pad - 1) & ~(pad - 1)), o_list = o_seed + ((B * 8 + pad - 1) & ~(pad - 1));
        FA_TRY(fa::take_once(ctx, "fa_luxtts_session_create", {{&st->slabs, total}, {&st->work, o_list + B * 4 * kMaxBuckets}}));
        char *d = st->slabs.as<char>(), *wk = st->work.as<char>();
        st->s.tokens = reinterpret_cast<int32_t *>(d + at[0]); st->s.token_mask = reinterpret_cast<float *>(d + at[1]);
        st->s.text_condition = reinterpret_cast<float *>(d + at[2]); st->s.speech_condition = reinterpret_cast<float *>(d + at[3]);
        st->s.x = reinterpret_cast<float *>(d + at[4]); st->s.frame_mask = reinterpret_cast<float *>(d + at[5]);
        st->s.records = reinterpret_cast<fa_luxtts_record *>(d + at[6]);
        st->d_items = reinterpret_cast<fa_luxtts_item_plan *>(wk + o_items); st->d_offsets = reinterpret_cast<int64_t *>(wk + o_off);
        st->d_token_offsets = reinterpret_cast<int64_t *>(wk + o_tok); st->d_sample_offsets = reinterpret_cast<int64_t *>(wk + o_smp);
        st->d_seeds = reinterpret_cast<uint64_t *>(wk + o_seed); st->d_list = reinterpret_cast<int32_t *>(wk + o_list);
        st->mel.s = st->s; st->mel.items = st->d_items; st->mel.offsets = st->d_offsets;
        *out = st.release();
        return FA_SUCCESS;
    });
}

void fa_luxtts_session_destroy(fa_luxtts_session *s) {
    if (!s) return;
    if (s->slabs.p) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    delete s;
}

fa_status fa_luxtts_session_slabs(fa_luxtts_session *s, fa_luxtts_slabs *out) {
    if (!s || !out) return FA_INVALID_ARGUMENT;
    *out = s->s;
    return FA_SUCCESS;
}

fa_status fa_luxtts_session_begin(fa_ctx *ctx, fa_luxtts_session *s, const int64_t *prompt_samples, const int32_t *prompt_tokens, const int32_t *text_tokens,
                                  const float *speeds, fa_luxtts_item_plan *items) {
    if (!ctx || !s || ctx != s->ctx) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    std::vector<fa_luxtts_item_plan> &plan = s->items;
    s->planned = false;
    FA_TRY(plan_batch(s->g, s->batch, prompt_samples, prompt_tokens, text_tokens, speeds, plan.data()));
    // (here and below the source is pageable host memory: the copy has left it when the call returns)
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_items, plan.data(), sizeof(fa_luxtts_item_plan) * plan.size(), hipMemcpyHostToDevice, ctx->stream));
    if (items) memcpy(items, plan.data(), sizeof(fa_luxtts_item_plan) * plan.size());
    s->planned = true;
    return FA_SUCCESS;
}

fa_status fa_luxtts_session_get(fa_ctx *ctx, fa_luxtts_session *s, int32_t slab, void *out) {
    if (!ctx || !s || ctx != s->ctx || !out || !s->slab(slab)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(out, s->slab(slab), s->slab_bytes(slab), hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_luxtts_prompt_dev(fa_ctx *ctx, fa_luxtts_session *s, const float *d_pcm, const int64_t *offsets) {
    FA_TRY(ready(ctx, s));
    if (!offsets) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < s->batch; ++b)
        if (offsets[b] < 0 || offsets[b + 1] - offsets[b] < s->items[b].samples) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts prompt: item %d has fewer samples than planned", b);
    if (offsets[s->batch] > 0 && !d_pcm) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_offsets, offsets, sizeof(int64_t) * (s->batch + 1), hipMemcpyHostToDevice, ctx->stream));
    MelArgs a = s->mel;
    a.pcm = d_pcm; a.vec = aligned16(d_pcm);
    run_prompt(a, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_luxtts_inputs_dev(fa_ctx *ctx, fa_luxtts_session *s, const int32_t *d_token_ids, const int64_t *token_offsets, const uint64_t *seeds) {
    FA_TRY(ready(ctx, s));
    if (!token_offsets || !seeds) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < s->batch; ++b)
        if (token_offsets[b] < 0 || token_offsets[b + 1] - token_offsets[b] < s->items[b].tokens) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts inputs: item %d has fewer token ids than planned", b);
    if (token_offsets[s->batch] > 0 && !d_token_ids) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_token_offsets, token_offsets, sizeof(int64_t) * (s->batch + 1), hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_seeds, seeds, sizeof(uint64_t) * s->batch, hipMemcpyHostToDevice, ctx->stream));
    InputArgs a{s->d_items, d_token_ids, s->d_token_offsets, s->d_seeds, s->s, s->g.n_mels, s->g.max_tokens, s->g.max_frames};
    run_inputs(a, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_luxtts_text_condition_dev(fa_ctx *ctx, fa_luxtts_session *s, const float *d_embeds, int64_t row_stride, int64_t item_stride) {
    FA_TRY(ready(ctx, s));
    if (!d_embeds || row_stride < s->g.n_mels || item_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    run_text_condition(row_args(s, d_embeds, row_stride, item_stride), s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_luxtts_step_dev(fa_ctx *ctx, fa_luxtts_session *s, int32_t step, const float *d_v, int64_t row_stride, int64_t item_stride) {
    FA_TRY(ready(ctx, s));
    if (!d_v || step < 0 || step >= s->g.num_steps || row_stride < s->g.n_mels || item_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    RowArgs a = row_args(s, d_v, row_stride, item_stride);
    a.times = step_times(s->g, step);
    run_step(a, s->batch, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_luxtts_vocoder_input_dev(fa_ctx *ctx, fa_luxtts_session *s, int32_t bucket, const int32_t *items, int32_t n, float *d_mel) {
    FA_TRY(ready(ctx, s));
    if (n < 0 || n > s->batch) return FA_INVALID_ARGUMENT;
    if (n == 0) return FA_SUCCESS;
    if (!items || !d_mel) return FA_INVALID_ARGUMENT;
    int slot = -1;
    for (int k = 0; k < s->g.n_buckets; ++k) if (s->g.buckets[k] == bucket) slot = k;
    if (slot < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts vocoder input: %d is no bucket of the configuration", bucket);
    for (int k = 0; k < n; ++k)
        if (items[k] < 0 || items[k] >= s->batch || s->items[items[k]].status != kOk || s->items[items[k]].bucket != bucket)
            return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts vocoder input: entry %d is no accepted item of bucket %d", k, bucket);
    fa::DeviceGuard guard(ctx->device);
    int32_t *d_list = s->d_list + static_cast<int64_t>(slot) * s->batch;
    FA_HIP_TRY(ctx, hipMemcpyAsync(d_list, items, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    // Synthesizer :253-254: the floor value and the scale are formed once, in fp32
    VocoderArgs a{s->d_items, d_list, s->s, d_mel, bucket, s->g.n_mels, s->g.max_frames, aligned16(d_mel), logf(s->g.log_floor), 1.0f / s->g.feat_scale};
    run_vocoder_input(a, n, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_luxtts_finish_dev(fa_ctx *ctx, fa_luxtts_session *s, const float *d_audio, int64_t row_stride, const int64_t *sample_offsets, float *d_out) {
    FA_TRY(ready(ctx, s));
    if (!sample_offsets || row_stride < 0) return FA_INVALID_ARGUMENT;
    int64_t longest = 0;
    for (int b = 0; b < s->batch; ++b) {
        const int64_t n = s->items[b].sample_count;
        if (sample_offsets[b] < 0 || sample_offsets[b + 1] - sample_offsets[b] < n || n > row_stride) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "luxtts finish: item %d needs %lld samples", b, (long long)n);
        longest = n > longest ? n : longest;
    }
    if (longest == 0) return FA_SUCCESS;
    if (!d_audio || !d_out) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_sample_offsets, sample_offsets, sizeof(int64_t) * (s->batch + 1), hipMemcpyHostToDevice, ctx->stream));
    FinishArgs a{s->d_items, d_audio, s->d_sample_offsets, d_out, s->s, row_stride, aligned16(d_audio) && aligned16(d_out), s->g.target_rms};
    run_finish(a, s->batch, longest, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

// ---- host-pointer forms: upload, run, fetch, one synchronisation
fa_status fa_luxtts_prompt(fa_ctx *ctx, fa_luxtts_session *s, const float *pcm, const int64_t *offsets) {
    FA_TRY(ready(ctx, s));
    if (!offsets || offsets[s->batch] < 0 || (offsets[s->batch] > 0 && !pcm)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_prompt", [&]() -> fa_status {
        fa::DevBuf d_pcm;
        FA_TRY(fa::take(ctx, "fa_luxtts_prompt", {{&d_pcm, sizeof(float) * static_cast<size_t>(offsets[s->batch]), true, pcm}}));
        FA_TRY(fa_luxtts_prompt_dev(ctx, s, d_pcm.as<float>(), offsets));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_luxtts_inputs(fa_ctx *ctx, fa_luxtts_session *s, const int32_t *token_ids, const int64_t *token_offsets, const uint64_t *seeds) {
    FA_TRY(ready(ctx, s));
    if (!token_offsets || token_offsets[s->batch] < 0 || (token_offsets[s->batch] > 0 && !token_ids)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_inputs", [&]() -> fa_status {
        fa::DevBuf d_ids;
        FA_TRY(fa::take(ctx, "fa_luxtts_inputs", {{&d_ids, sizeof(int32_t) * static_cast<size_t>(token_offsets[s->batch]), true, token_ids}}));
        FA_TRY(fa_luxtts_inputs_dev(ctx, s, d_ids.as<int32_t>(), token_offsets, seeds));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_luxtts_text_condition(fa_ctx *ctx, fa_luxtts_session *s, const float *embeds, int64_t row_stride, int64_t item_stride) {
    FA_TRY(ready(ctx, s));
    if (!embeds || row_stride < s->g.n_mels || item_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_text_condition", [&]() -> fa_status {
        int64_t rows = 1;
        for (const fa_luxtts_item_plan &p : s->items) rows = p.tokens + 1 > rows ? p.tokens + 1 : rows;
        fa::DevBuf d;
        FA_TRY(fa::take(ctx, "fa_luxtts_text_condition", {{&d, sizeof(float) * strided_floats(s, row_stride, item_stride, rows), true, embeds}}));
        FA_TRY(fa_luxtts_text_condition_dev(ctx, s, d.as<float>(), row_stride, item_stride));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_luxtts_step(fa_ctx *ctx, fa_luxtts_session *s, int32_t step, const float *v, int64_t row_stride, int64_t item_stride) {
    FA_TRY(ready(ctx, s));
    if (!v || row_stride < s->g.n_mels || item_stride < 0) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_step", [&]() -> fa_status {
        int64_t rows = 1;
        for (const fa_luxtts_item_plan &p : s->items) rows = p.features_length > rows ? p.features_length : rows;
        fa::DevBuf d;
        FA_TRY(fa::take(ctx, "fa_luxtts_step", {{&d, sizeof(float) * strided_floats(s, row_stride, item_stride, rows), true, v}}));
        FA_TRY(fa_luxtts_step_dev(ctx, s, step, d.as<float>(), row_stride, item_stride));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_luxtts_vocoder_input(fa_ctx *ctx, fa_luxtts_session *s, int32_t bucket, const int32_t *items, int32_t n, float *mel) {
    FA_TRY(ready(ctx, s));
    if (n < 0 || n > s->batch || bucket < 1 || (n > 0 && !mel)) return FA_INVALID_ARGUMENT;
    if (n == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_vocoder_input", [&]() -> fa_status {
        const size_t bytes = sizeof(float) * static_cast<size_t>(n) * s->g.n_mels * bucket;
        fa::DevBuf d;
        FA_TRY(fa::take(ctx, "fa_luxtts_vocoder_input", {{&d, bytes}}));
        FA_TRY(fa_luxtts_vocoder_input_dev(ctx, s, bucket, items, n, d.as<float>()));
        FA_HIP_TRY(ctx, hipMemcpyAsync(mel, d.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_luxtts_finish(fa_ctx *ctx, fa_luxtts_session *s, const float *audio, int64_t row_stride, const int64_t *sample_offsets, float *out) {
    FA_TRY(ready(ctx, s));
    if (!sample_offsets || row_stride < 0 || sample_offsets[s->batch] < 0) return FA_INVALID_ARGUMENT;
    const size_t total = static_cast<size_t>(sample_offsets[s->batch]);
    if (total == 0) return FA_SUCCESS;
    if (!audio || !out) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_luxtts_finish", [&]() -> fa_status {
        fa::DevBuf d_audio, d_out;
        FA_TRY(fa::take(ctx, "fa_luxtts_finish", {{&d_audio, sizeof(float) * static_cast<size_t>(s->batch) * row_stride, true, audio}, {&d_out, sizeof(float) * total, true, out}}));
        FA_TRY(fa_luxtts_finish_dev(ctx, s, d_audio.as<float>(), row_stride, sample_offsets, d_out.as<float>()));   // samples no item writes keep the caller's values
        FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, sizeof(float) * total, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

}  // extern "C"
