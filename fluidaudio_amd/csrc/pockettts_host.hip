// pockettts_host.hip — host side of the PocketTTS session (kernels: pockettts.hip): the configuration, the voice and projection tables,
// the plans of pockettts_core.h as C records, the session with its slabs in HBM, the entries and their host-pointer forms.  Nothing
// here waits for the device except fa_pockettts_session_get and the host-pointer forms; after fa_pockettts_session_create nothing is
// allocated by an entry that takes no host data array.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "pockettts_launch.h"

using namespace fa::pockettts;

namespace {

constexpr int kSlabs = 13;

bool config_ok(const fa_pockettts_config *c) {
    return c && c->layers >= 1 && c->layers <= kMaxLayers && c->kv_format >= kKvCombined && c->kv_format <= kKvHalf && c->streams >= 1 && c->streams <= 4096 && c->voices >= 1 &&
           c->voices <= 4096 && c->voice_seq >= 1 && c->voice_seq <= kKvSeq && c->projections >= 0 && c->projections <= 1024 && c->vocab >= 1 && c->vocab <= (1 << 20) &&
           c->windows >= 1 && c->windows <= 65535 && c->clones >= 1 && c->clones <= 65535 && c->max_frames >= 1 && c->max_frames <= 65536 && (c->bos_sequence == 0 || c->bos_sequence == 1);
}

struct Voice {
    bool present = false, has_snapshot = false;
    int32_t src_seq = 0, prompt_length = 0;
};

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

struct fa_pockettts_session {
    fa_ctx *ctx = nullptr;
    fa_pockettts_config c{};
    int32_t P = 0, vocab = 0, n_windows = 0;
    bool have_bos = false;
    std::vector<Voice> voices;
    std::vector<Window> windows;            // the plan
    std::vector<AdvanceItem> advance;       // its accepted streams and their rows
    std::vector<int64_t> ids_from;          // per accepted stream: where its ids start in the caller's array
    std::vector<int32_t> ids_count, ids;
    int64_t ids_total = 0;                  // ids of all listed streams in the caller's array
    fa::DevBuf slabs, tables, work;
    fa_pockettts_slabs s{};
    float *d_projections = nullptr, *d_bos_before_voice = nullptr, *d_bos_embedding = nullptr, *d_table = nullptr, *d_voice_offsets = nullptr;
    char *d_work = nullptr;                 // the records of one call
    int32_t *d_ids = nullptr;
    size_t slab_bytes(const int which) const {
        const size_t S = c.streams, L = c.layers;
        switch (which) {
        case FA_POCKETTTS_SLAB_KV: return S * L * 2 * kPlane * (c.kv_format == kKvHalf ? 2 : 4);
        case FA_POCKETTTS_SLAB_POSITIONS: return S * P * 4;
        case FA_POCKETTTS_SLAB_VOICE_ROWS: return static_cast<size_t>(c.voices) * kMaxVoiceFrames * kDim * 4;
        case FA_POCKETTTS_SLAB_VOICE_KV: return static_cast<size_t>(c.voices) * L * 2 * c.voice_seq * kKvRow * 4;
        case FA_POCKETTTS_SLAB_ENCODER_INPUT: return static_cast<size_t>(c.clones) * kEncoderSamples * 4;
        case FA_POCKETTTS_SLAB_WINDOWS: return static_cast<size_t>(c.windows) * kWindow * kDim * 4;
        case FA_POCKETTTS_SLAB_VALID_LEN: case FA_POCKETTTS_SLAB_WINDOW_POSITION: return static_cast<size_t>(c.windows) * 4;
        case FA_POCKETTTS_SLAB_SEQUENCE: return S * kLatent * 4;
        case FA_POCKETTTS_SLAB_STATE: return S * sizeof(StreamState);
        case FA_POCKETTTS_SLAB_RUNNING: return S * 4;
        case FA_POCKETTTS_SLAB_N_RUNNING: return 4;
        case FA_POCKETTTS_SLAB_AUDIO: return S * c.max_frames * kFrameSamples * 4;
        }
        return 0;
    }
    void *slab(const int which) const {
        void *const p[kSlabs] = {s.kv, s.positions, s.voice_rows, s.voice_kv, s.encoder_input, s.windows, s.valid_len, s.window_position, s.sequence, s.state, s.running, s.n_running, s.audio};
        return which >= 0 && which < kSlabs ? p[which] : nullptr;
    }
    size_t work_bytes() const {
        const size_t most = static_cast<size_t>(c.streams > c.clones ? c.streams : c.clones);
        return (most > static_cast<size_t>(c.windows) ? most : static_cast<size_t>(c.windows)) * sizeof(Window) + static_cast<size_t>(c.streams) * sizeof(AdvanceItem);
    }
    KvArgs kv_args(const KvItem *items) const {
        return KvArgs{items, s.kv, s.positions, s.voice_kv, d_voice_offsets, static_cast<int64_t>(c.voice_seq) * kKvRow, c.kv_format, c.streams, c.layers, P};
    }
    // the records of a call are pageable host memory: the copy has left them when hipMemcpyAsync returns
    template <class T> fa_status upload(void *dst, const std::vector<T> &v) {
        if (v.empty()) return FA_SUCCESS;
        FA_HIP_TRY(ctx, hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, ctx->stream));
        return FA_SUCCESS;
    }
};

static_assert(sizeof(StreamState) == sizeof(fa_pockettts_stream_state) && sizeof(Window) == sizeof(fa_pockettts_window), "the C records are the core's");

namespace {

fa_status ready(fa_ctx *ctx, const fa_pockettts_session *s) { return !ctx || !s || ctx != s->ctx ? FA_INVALID_ARGUMENT : FA_SUCCESS; }

bool in_range(const int32_t v, const int32_t n) { return v >= 0 && v < n; }

fa_status clone_plan(const int32_t n, const int64_t *samples, const int32_t *available, int32_t *usable, int32_t *statuses) {
    if (n < 1 || !samples || !usable || !statuses) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < n; ++b) {
        if (samples[b] < 0 || (available && available[b] < 0)) return FA_INVALID_ARGUMENT;
        statuses[b] = clip_status(samples[b]);
        usable[b] = statuses[b] == kOk ? usable_frames(samples[b], available ? available[b] : kMaxVoiceFrames) : 0;
    }
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

void fa_pockettts_default_config(fa_pockettts_config *c) {   // PocketTtsConstants.swift
    if (!c) return;
    *c = fa_pockettts_config{6, FA_POCKETTTS_KV_COMBINED, 4, 4, kKvSeq, 2, 4001, 16, 4, 256, 0};
}

fa_status fa_pockettts_clone_plan(int32_t n, const int64_t *samples, const int32_t *available, int32_t *usable, int32_t *statuses) {
    return clone_plan(n, samples, available, usable, statuses);
}

fa_status fa_pockettts_session_create(fa_ctx *ctx, const fa_pockettts_config *cfg, fa_pockettts_session **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    if (!config_ok(cfg)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "pockettts session: unsupported configuration");
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_session_create", [&]() -> fa_status {
        std::unique_ptr<fa_pockettts_session> st(new fa_pockettts_session());
        st->ctx = ctx; st->c = *cfg; st->P = positions_of(cfg->kv_format, cfg->layers);
        st->voices.resize(cfg->voices);
        auto up = [](const size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); };
        size_t at[kSlabs], total = 0;
        for (int w = 0; w < kSlabs; ++w) { at[w] = total; total += up(st->slab_bytes(w)); }
        const size_t o_proj = 0, o_bbv = o_proj + up(static_cast<size_t>(cfg->projections) * 2 * kDim * kLatent * 4), o_bos = o_bbv + up(kDim * 4), o_tab = o_bos + up(kLatent * 4);
        const size_t o_off = o_tab + up(static_cast<size_t>(cfg->vocab) * kDim * 4), tables = o_off + up(static_cast<size_t>(cfg->voices) * kMaxLayers * 4);
        const size_t o_ids = up(st->work_bytes());
        FA_TRY(fa::take_once(ctx, "fa_pockettts_session_create", {{&st->slabs, total}, {&st->tables, tables}, {&st->work, o_ids + up(static_cast<size_t>(cfg->windows) * kWindow * 4)}}));
        char *d = st->slabs.as<char>(), *t = st->tables.as<char>();
        fa_pockettts_slabs &s = st->s;
        s.kv = d + at[0]; s.positions = reinterpret_cast<float *>(d + at[1]); s.voice_rows = reinterpret_cast<float *>(d + at[2]); s.voice_kv = reinterpret_cast<float *>(d + at[3]);
        s.encoder_input = reinterpret_cast<float *>(d + at[4]); s.windows = reinterpret_cast<float *>(d + at[5]); s.valid_len = reinterpret_cast<float *>(d + at[6]);
        s.window_position = reinterpret_cast<float *>(d + at[7]); s.sequence = reinterpret_cast<float *>(d + at[8]); s.state = reinterpret_cast<fa_pockettts_stream_state *>(d + at[9]);
        s.running = reinterpret_cast<int32_t *>(d + at[10]); s.n_running = reinterpret_cast<int32_t *>(d + at[11]); s.audio = reinterpret_cast<float *>(d + at[12]);
        st->d_projections = reinterpret_cast<float *>(t + o_proj); st->d_bos_before_voice = reinterpret_cast<float *>(t + o_bbv); st->d_bos_embedding = reinterpret_cast<float *>(t + o_bos);
        st->d_table = reinterpret_cast<float *>(t + o_tab); st->d_voice_offsets = reinterpret_cast<float *>(t + o_off);
        st->d_work = st->work.as<char>(); st->d_ids = reinterpret_cast<int32_t *>(st->d_work + o_ids);
        // every stream idle, position 0, no stream running; the BOS latent zeros until the constants arrive
        for (const int w : {FA_POCKETTTS_SLAB_POSITIONS, FA_POCKETTTS_SLAB_STATE, FA_POCKETTTS_SLAB_N_RUNNING, FA_POCKETTTS_SLAB_SEQUENCE})
            FA_HIP_TRY(ctx, hipMemsetAsync(st->slab(w), 0, st->slab_bytes(w), ctx->stream));
        FA_HIP_TRY(ctx, hipMemsetAsync(st->d_bos_embedding, 0, kLatent * 4, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *out = st.release();
        return FA_SUCCESS;
    });
}

void fa_pockettts_session_destroy(fa_pockettts_session *s) {
    if (!s) return;
    if (s->slabs.p) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    delete s;
}

fa_status fa_pockettts_session_slabs(fa_pockettts_session *s, fa_pockettts_slabs *out) {
    if (!s || !out) return FA_INVALID_ARGUMENT;
    *out = s->s;
    return FA_SUCCESS;
}

fa_status fa_pockettts_session_get(fa_ctx *ctx, fa_pockettts_session *s, int32_t slab, int64_t offset, int64_t bytes, void *out) {
    FA_TRY(ready(ctx, s));
    if (!out || !s->slab(slab) || offset < 0 || bytes < 0 || static_cast<size_t>(offset) + static_cast<size_t>(bytes) > s->slab_bytes(slab)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    if (bytes) FA_HIP_TRY(ctx, hipMemcpyAsync(out, static_cast<char *>(s->slab(slab)) + offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_pockettts_session_put(fa_ctx *ctx, fa_pockettts_session *s, int32_t slab, int64_t offset, int64_t bytes, const void *src) {
    FA_TRY(ready(ctx, s));
    if (!src || !s->slab(slab) || offset < 0 || bytes < 0 || static_cast<size_t>(offset) + static_cast<size_t>(bytes) > s->slab_bytes(slab)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    if (bytes) FA_HIP_TRY(ctx, hipMemcpyAsync(static_cast<char *>(s->slab(slab)) + offset, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_pockettts_projection_set(fa_ctx *ctx, fa_pockettts_session *s, int32_t index, const float *pinv, const float *w) {
    FA_TRY(ready(ctx, s));
    if (!in_range(index, s->c.projections) || !pinv || !w) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    float *d = s->d_projections + static_cast<size_t>(index) * 2 * kDim * kLatent;
    FA_HIP_TRY(ctx, hipMemcpyAsync(d, pinv, sizeof(float) * kDim * kLatent, hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(d + kDim * kLatent, w, sizeof(float) * kDim * kLatent, hipMemcpyHostToDevice, ctx->stream));
    return FA_SUCCESS;
}

fa_status fa_pockettts_constants_set(fa_ctx *ctx, fa_pockettts_session *s, const float *bos_before_voice, const float *bos_embedding, const float *table, int32_t vocab) {
    FA_TRY(ready(ctx, s));
    if (!table || vocab < 1 || vocab > s->c.vocab) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    if (bos_before_voice) FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_bos_before_voice, bos_before_voice, sizeof(float) * kDim, hipMemcpyHostToDevice, ctx->stream));
    if (bos_embedding) FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_bos_embedding, bos_embedding, sizeof(float) * kLatent, hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipMemcpyAsync(s->d_table, table, sizeof(float) * static_cast<size_t>(vocab) * kDim, hipMemcpyHostToDevice, ctx->stream));
    s->have_bos = bos_before_voice != nullptr;
    s->vocab = vocab;
    return FA_SUCCESS;
}

fa_status fa_pockettts_voice_add(fa_ctx *ctx, fa_pockettts_session *s, int32_t voice, int32_t layers, int32_t src_seq, const float *caches, const int64_t *float_counts,
                                 const int64_t *offsets, int32_t *status) {
    FA_TRY(ready(ctx, s));
    if (!in_range(voice, s->c.voices) || layers < 0 || layers > kMaxLayers || src_seq < 0 || !float_counts || !offsets || !status) return FA_INVALID_ARGUMENT;
    s->voices[voice] = Voice{};
    *status = snapshot_status(layers, s->c.layers, src_seq, s->c.voice_seq, float_counts);
    if (*status != kOk) return FA_SUCCESS;
    if (src_seq > 0 && !caches) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_voice_add", [&]() -> fa_status {
        const size_t per = static_cast<size_t>(src_seq) * kKvRow, plane = static_cast<size_t>(s->c.voice_seq) * kKvRow;
        for (int l = 0; l < layers && per; ++l)
            for (int kv = 0; kv < 2; ++kv)
                FA_HIP_TRY(ctx, hipMemcpyAsync(s->s.voice_kv + ((static_cast<size_t>(voice) * layers + l) * 2 + kv) * plane, caches + (static_cast<size_t>(l) * 2 + kv) * per, per * 4,
                                               hipMemcpyHostToDevice, ctx->stream));
        std::vector<float> off(kMaxLayers, 0.0f);
        for (int l = 0; l < layers; ++l) off[l] = static_cast<float>(offsets[l]);   // KVCache :449
        FA_TRY(s->upload(s->d_voice_offsets + static_cast<size_t>(voice) * kMaxLayers, off));
        s->voices[voice] = Voice{true, true, src_seq, 0};
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_encoder_input_dev(fa_ctx *ctx, fa_pockettts_session *s, int32_t n, const float *d_pcm, const int64_t *offsets, int32_t *usable, int32_t *statuses) {
    FA_TRY(ready(ctx, s));
    if (n < 1 || n > s->c.clones || !offsets || !usable || !statuses) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < n; ++b)
        if (offsets[b] < 0 || offsets[b + 1] < offsets[b]) return FA_INVALID_ARGUMENT;
    if (offsets[n] > 0 && !d_pcm) return FA_INVALID_ARGUMENT;
    for (int b = 0; b < n; ++b) {
        const int64_t len = offsets[b + 1] - offsets[b];
        FA_TRY(clone_plan(1, &len, nullptr, usable + b, statuses + b));
    }
    fa::DeviceGuard guard(ctx->device);
    const auto fill = [&](fa::rows::Group &g, const int64_t i, const int32_t k) {
        const int64_t len = offsets[i + 1] - offsets[i];
        g.src[k] = offsets[i];
        g.len[k] = static_cast<int32_t>(len < kEncoderSamples ? len : kEncoderSamples);
    };
    fa::rows::for_each_group(n, fill, [&](const fa::rows::Group &g, const int64_t g0) { run_encoder_rows(d_pcm, g, s->s.encoder_input + g0 * kEncoderSamples, true, ctx->stream); });
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_pockettts_clone_dev(fa_ctx *ctx, fa_pockettts_session *s, int32_t n, const int32_t *voices, const int32_t *projections, const int32_t *usable, const void *d_cond,
                                 int32_t dtype, int64_t item_stride, int64_t frame_stride, int64_t dim_stride) {
    FA_TRY(ready(ctx, s));
    if (n < 1 || n > s->c.clones || !voices || !projections || !usable || !d_cond || (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) || item_stride < 0 || frame_stride < 0 ||
        dim_stride < 1)
        return FA_INVALID_ARGUMENT;
    for (int b = 0; b < n; ++b) {
        if (!in_range(voices[b], s->c.voices) || projections[b] < -1 || projections[b] >= s->c.projections || usable[b] < 0 || usable[b] > kMaxVoiceFrames) return FA_INVALID_ARGUMENT;
        for (int o = 0; o < b; ++o)
            if (voices[o] == voices[b]) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "pockettts clone: items %d and %d name voice %d", o, b, voices[b]);
    }
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_clone_dev", [&]() -> fa_status {
        std::vector<CloneItem> items(n);
        for (int b = 0; b < n; ++b) items[b] = CloneItem{voices[b], projections[b], usable[b], 0};
        FA_TRY(s->upload(s->d_work, items));
        const int64_t esz = dtype == FA_DTYPE_F16 ? 2 : 4;
        const bool vec = dim_stride == 1 && aligned16(d_cond) && item_stride * esz % 16 == 0 && frame_stride * esz % 16 == 0;
        run_clone(CloneArgs{reinterpret_cast<const CloneItem *>(s->d_work), d_cond, item_stride, frame_stride, dim_stride, s->d_projections, s->s.voice_rows, vec}, dtype, n, ctx->stream);
        FA_HIP_TRY(ctx, hipGetLastError());
        for (int b = 0; b < n; ++b) s->voices[voices[b]] = Voice{true, false, 0, usable[b]};   // VoiceCloner :196
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_kv_reset(fa_ctx *ctx, fa_pockettts_session *s, int32_t n, const int32_t *streams, const int32_t *voices) {
    FA_TRY(ready(ctx, s));
    if (n < 1 || n > s->c.streams || !streams || !voices) return FA_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if (!in_range(streams[i], s->c.streams) || !in_range(voices[i], s->c.voices) || !s->voices[voices[i]].present) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_kv_reset", [&]() -> fa_status {
        std::vector<KvItem> items(n);
        for (int i = 0; i < n; ++i) {   // KVCache :482-487: a voice without a snapshot starts from the empty state
            const Voice &v = s->voices[voices[i]];
            items[i] = KvItem{streams[i], v.has_snapshot ? voices[i] : -1, v.has_snapshot ? v.src_seq : 0, 0};
        }
        FA_TRY(s->upload(s->d_work, items));
        run_kv_reset(s->kv_args(reinterpret_cast<const KvItem *>(s->d_work)), n, ctx->stream);
        FA_HIP_TRY(ctx, hipGetLastError());
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_kv_capture(fa_ctx *ctx, fa_pockettts_session *s, int32_t stream, int32_t voice, int32_t seq) {
    FA_TRY(ready(ctx, s));
    if (!in_range(stream, s->c.streams) || !in_range(voice, s->c.voices) || seq < 0 || seq > s->c.voice_seq) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_kv_capture", [&]() -> fa_status {
        const std::vector<KvItem> items(1, KvItem{stream, voice, seq, 0});
        FA_TRY(s->upload(s->d_work, items));
        run_kv_capture(s->kv_args(reinterpret_cast<const KvItem *>(s->d_work)), ctx->stream);
        FA_HIP_TRY(ctx, hipGetLastError());
        Voice &v = s->voices[voice];
        v.present = v.has_snapshot = true;
        v.src_seq = seq;
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_plan(fa_pockettts_session *s, int32_t n, const int32_t *streams, const int32_t *voices, const int32_t *token_counts, int32_t *n_windows,
                            fa_pockettts_window *windows, int32_t *statuses) {
    if (!s || n < 1 || n > s->c.streams || !streams || !voices || !token_counts || !n_windows || !statuses) return FA_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) {
        if (!in_range(streams[i], s->c.streams) || !in_range(voices[i], s->c.voices) || token_counts[i] < 0) return FA_INVALID_ARGUMENT;
        for (int o = 0; o < i; ++o)
            if (streams[o] == streams[i]) return FA_INVALID_ARGUMENT;
    }
    return fa::no_throw(s->ctx, "fa_pockettts_plan", [&]() -> fa_status {
        s->windows.assign(s->c.windows, Window{});
        s->advance.clear(); s->ids_from.clear(); s->ids_count.clear();
        int32_t count = 0, ids_at = 0;
        int64_t from = 0;
        for (int i = 0; i < n; ++i) {
            const Voice &v = s->voices[voices[i]];
            const int32_t first = count;
            statuses[i] = plan_stream(streams[i], voices[i], VoiceFacts{v.present, v.has_snapshot, v.prompt_length}, s->have_bos, token_counts[i], ids_at, s->windows.data(),
                                      s->c.windows, &count);
            if (statuses[i] == kOk) {
                int32_t rows = 0;
                for (int w = first; w < count; ++w) rows += s->windows[w].n;
                s->advance.push_back(AdvanceItem{streams[i], rows});
                s->ids_from.push_back(from); s->ids_count.push_back(token_counts[i]);
                ids_at += token_counts[i];
            }
            from += token_counts[i];
        }
        s->n_windows = count; s->ids_total = from;
        s->windows.resize(count);
        *n_windows = count;
        if (windows && count) memcpy(windows, s->windows.data(), sizeof(Window) * count);
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_prefill_inputs(fa_ctx *ctx, fa_pockettts_session *s, const int32_t *token_ids) {
    FA_TRY(ready(ctx, s));
    if (s->ids_total > 0 && !token_ids) return FA_INVALID_ARGUMENT;
    if (s->n_windows > 0 && s->vocab < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "pockettts prefill: fa_pockettts_constants_set has not run");
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_prefill_inputs", [&]() -> fa_status {
        s->ids.clear();   // the accepted streams' ids back to back: a window's rows never outnumber the arena's
        for (size_t i = 0; i < s->ids_from.size(); ++i) s->ids.insert(s->ids.end(), token_ids + s->ids_from[i], token_ids + s->ids_from[i] + s->ids_count[i]);
        AdvanceItem *d_adv = reinterpret_cast<AdvanceItem *>(s->d_work + sizeof(Window) * s->c.windows);
        FA_TRY(s->upload(s->d_work, s->windows));
        FA_TRY(s->upload(d_adv, s->advance));
        FA_TRY(s->upload(s->d_ids, s->ids));
        const PrefillArgs a{reinterpret_cast<const Window *>(s->d_work), s->d_ids, s->d_table, s->d_bos_before_voice, s->s.voice_rows, s->s.positions,
                            s->s.windows, s->s.valid_len, s->s.window_position, s->vocab, s->P};
        run_prefill(a, s->n_windows, d_adv, s->s.positions, static_cast<int>(s->advance.size()), ctx->stream);
        FA_HIP_TRY(ctx, hipGetLastError());
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_position_set(fa_ctx *ctx, fa_pockettts_session *s, int32_t stream, float position) {
    FA_TRY(ready(ctx, s));
    if (!in_range(stream, s->c.streams)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    run_position_set(s->s.positions + static_cast<size_t>(stream) * s->P, s->P, position, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_pockettts_step_begin(fa_ctx *ctx, fa_pockettts_session *s, int32_t n, const int32_t *streams, const int32_t *max_gen_len, const int32_t *frames_after_eos,
                                  int32_t *statuses) {
    FA_TRY(ready(ctx, s));
    if (n < 1 || n > s->c.streams || !streams || !max_gen_len || !frames_after_eos) return FA_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) {
        if (!in_range(streams[i], s->c.streams) || max_gen_len[i] < 0 || frames_after_eos[i] < 0 || frames_after_eos[i] > (1 << 20)) return FA_INVALID_ARGUMENT;
        for (int o = 0; o < i; ++o)
            if (streams[o] == streams[i]) return FA_INVALID_ARGUMENT;
    }
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_step_begin", [&]() -> fa_status {
        std::vector<BeginItem> items;
        for (int i = 0; i < n; ++i) {
            const int32_t st = max_gen_len[i] > s->c.max_frames ? kTooManyFrames : kOk;
            if (statuses) statuses[i] = st;
            if (st == kOk) items.push_back(BeginItem{streams[i], max_gen_len[i], frames_after_eos[i], 0});
        }
        FA_TRY(s->upload(s->d_work, items));
        StreamState *state = reinterpret_cast<StreamState *>(s->s.state);
        run_step_begin(reinterpret_cast<const BeginItem *>(s->d_work), static_cast<int>(items.size()), state, s->s.sequence, s->d_bos_embedding, s->c.bos_sequence, ctx->stream);
        run_step(StepArgs{state, nullptr, nullptr, s->s.sequence, s->s.positions, s->s.running, s->s.n_running, s->c.streams, s->P}, ctx->stream);
        FA_HIP_TRY(ctx, hipGetLastError());
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_step_dev(fa_ctx *ctx, fa_pockettts_session *s, const float *d_eos_logit, const float *d_latent) {
    FA_TRY(ready(ctx, s));
    if (!d_eos_logit || !d_latent) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    run_step(StepArgs{reinterpret_cast<StreamState *>(s->s.state), d_eos_logit, d_latent, s->s.sequence, s->s.positions, s->s.running, s->s.n_running, s->c.streams, s->P}, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_pockettts_append_audio_dev(fa_ctx *ctx, fa_pockettts_session *s, const float *d_samples) {
    FA_TRY(ready(ctx, s));
    if (!d_samples) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    run_append_audio(reinterpret_cast<const StreamState *>(s->s.state), d_samples, s->s.audio, s->c.streams, s->c.max_frames, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

// ---- host-pointer forms: upload, run, one synchronisation
fa_status fa_pockettts_encoder_input(fa_ctx *ctx, fa_pockettts_session *s, int32_t n, const float *pcm, const int64_t *offsets, int32_t *usable, int32_t *statuses) {
    FA_TRY(ready(ctx, s));
    if (n < 1 || n > s->c.clones || !offsets || offsets[n] < 0 || (offsets[n] > 0 && !pcm)) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_encoder_input", [&]() -> fa_status {
        fa::DevBuf d_pcm;
        FA_TRY(fa::take(ctx, "fa_pockettts_encoder_input", {{&d_pcm, sizeof(float) * static_cast<size_t>(offsets[n]), true, pcm}}));
        FA_TRY(fa_pockettts_encoder_input_dev(ctx, s, n, d_pcm.as<float>(), offsets, usable, statuses));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_clone(fa_ctx *ctx, fa_pockettts_session *s, int32_t n, const int32_t *voices, const int32_t *projections, const int32_t *usable, const void *cond,
                             int32_t dtype, int64_t item_stride, int64_t frame_stride, int64_t dim_stride) {
    FA_TRY(ready(ctx, s));
    if (n < 1 || !cond || !usable || (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16) || item_stride < 0 || frame_stride < 0 || dim_stride < 1) return FA_INVALID_ARGUMENT;
    int32_t frames = 1;   // the host array ends with the last usable frame of its longest item
    for (int b = 0; b < n; ++b) frames = usable[b] > frames ? usable[b] : frames;
    if (frames > kMaxVoiceFrames) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_clone", [&]() -> fa_status {
        const size_t elems = static_cast<size_t>(n - 1) * item_stride + static_cast<size_t>(frames - 1) * frame_stride + static_cast<size_t>(kDim - 1) * dim_stride + 1;
        fa::DevBuf d_cond;
        FA_TRY(fa::take(ctx, "fa_pockettts_clone", {{&d_cond, elems * (dtype == FA_DTYPE_F16 ? 2 : 4), true, cond}}));
        FA_TRY(fa_pockettts_clone_dev(ctx, s, n, voices, projections, usable, d_cond.p, dtype, item_stride, frame_stride, dim_stride));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_step(fa_ctx *ctx, fa_pockettts_session *s, const float *eos_logit, const float *latent) {
    FA_TRY(ready(ctx, s));
    if (!eos_logit || !latent) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_step", [&]() -> fa_status {
        const size_t S = s->c.streams;
        fa::DevBuf d_e, d_l;
        FA_TRY(fa::take(ctx, "fa_pockettts_step", {{&d_e, sizeof(float) * S, true, eos_logit}, {&d_l, sizeof(float) * S * kLatent, true, latent}}));
        FA_TRY(fa_pockettts_step_dev(ctx, s, d_e.as<float>(), d_l.as<float>()));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

fa_status fa_pockettts_append_audio(fa_ctx *ctx, fa_pockettts_session *s, const float *samples) {
    FA_TRY(ready(ctx, s));
    if (!samples) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_pockettts_append_audio", [&]() -> fa_status {
        fa::DevBuf d;
        FA_TRY(fa::take(ctx, "fa_pockettts_append_audio", {{&d, sizeof(float) * static_cast<size_t>(s->c.streams) * kFrameSamples, true, samples}}));
        FA_TRY(fa_pockettts_append_audio_dev(ctx, s, d.as<float>()));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return FA_SUCCESS;
    });
}

}  // extern "C"
