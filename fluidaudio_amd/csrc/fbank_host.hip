// fbank_host.hip — host side of the Kaldi fbank + LFR + CMVN front end (kernel: fbank.hip): the window and the HTK mel bank built
// in double and rounded to fp32, configuration checks, plans (fa_fbank_plan_*), the device entry and the host-pointer entry.
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "fbank_launch.h"

using namespace fa::fbank;

namespace {

void make_window(const fa_fbank_config *c, std::vector<float> &w) {
    w.resize(c->win);
    if (c->window) { w.assign(c->window, c->window + c->win); return; }
    for (int i = 0; i < c->win; ++i) {
        const double a = 2.0 * M_PI * i / (c->win - 1);
        const double v = c->window_type == FA_FBANK_WINDOW_POVEY ? pow(0.5 - 0.5 * cos(a), 0.85) : 0.54 - 0.46 * cos(a);
        w[i] = static_cast<float>(v);
    }
}

// Kaldi's mel bank, dense [n_mels][n_fft / 2 + 1]: triangles on the mel axis, mel(f) = 1127 ln(1 + f / 700); the Nyquist column is 0
void make_filterbank(const fa_fbank_config *c, std::vector<float> &fb) {
    const int bins = c->n_fft / 2 + 1;
    if (c->filterbank) { fb.assign(c->filterbank, c->filterbank + static_cast<size_t>(c->n_mels) * bins); return; }
    fb.assign(static_cast<size_t>(c->n_mels) * bins, 0.0f);
    auto mel = [](double f) { return 1127.0 * log(1.0 + f / 700.0); };
    const double nyquist = 0.5 * c->sample_rate;
    const double lo = mel(c->low_freq), hi = mel(c->high_freq > 0.0f ? c->high_freq : nyquist + c->high_freq);
    const double delta = (hi - lo) / (c->n_mels + 1);
    for (int b = 0; b < c->n_mels; ++b) {
        const double left = lo + b * delta, centre = left + delta, right = centre + delta;
        for (int k = 0; k < c->n_fft / 2; ++k) {
            const double m = mel(static_cast<double>(k) * c->sample_rate / c->n_fft);
            const double up = (m - left) / (centre - left), down = (right - m) / (right - centre);
            const double v = up < down ? up : down;
            fb[static_cast<size_t>(b) * bins + k] = static_cast<float>(v > 0.0 ? v : 0.0);
        }
    }
}

fa_status validate(const fa_fbank_config *c) {
    if (!c) return FA_INVALID_ARGUMENT;
    if (c->n_fft != fa::melcore::kNfft) return FA_INVALID_ARGUMENT;   // this kernel generation: win <= 512 samples
    if (c->win < 2 || c->win > c->n_fft || c->hop < 1 || c->hop > 4096) return FA_INVALID_ARGUMENT;
    if (c->n_mels < 1 || c->n_mels > kMaxMels || c->sample_rate < 1) return FA_INVALID_ARGUMENT;
    if (c->lfr_m < 1 || c->lfr_m > kMaxLfr || c->lfr_n < 1 || c->lfr_n > kMaxLfr) return FA_INVALID_ARGUMENT;
    if (c->tail_mode != FA_FBANK_TAIL_REPLICATE && c->tail_mode != FA_FBANK_TAIL_VALID) return FA_INVALID_ARGUMENT;
    if (c->window_type != FA_FBANK_WINDOW_HAMMING && c->window_type != FA_FBANK_WINDOW_POVEY) return FA_INVALID_ARGUMENT;
    if (!(c->log_floor > 0.0f) || !(c->low_freq >= 0.0f)) return FA_INVALID_ARGUMENT;
    const float high = c->high_freq > 0.0f ? c->high_freq : 0.5f * c->sample_rate + c->high_freq;
    if (!c->filterbank && !(high > c->low_freq && high <= 0.5f * c->sample_rate)) return FA_INVALID_ARGUMENT;
    return FA_SUCCESS;
}

std::vector<float2> twiddles(int count, int n) {
    std::vector<float2> tw(count);
    for (int k = 0; k < count; ++k) { const double a = -2.0 * M_PI * k / n; tw[k] = make_float2((float)cos(a), (float)sin(a)); }
    return tw;
}

// the plan's tables, back to back in one host image at 256-byte aligned offsets; place() points an operand into the uploaded copy
struct Image {
    std::vector<char> bytes;
    template <class T> size_t add(const T *src, size_t n) {
        const size_t at = bytes.size();
        bytes.resize((at + sizeof(T) * n + 255) & ~static_cast<size_t>(255), 0);
        memcpy(bytes.data() + at, src, sizeof(T) * n);
        return at;
    }
};
template <class T> void place(const T *&dst, const fa::DevBuf &buf, size_t at) { dst = reinterpret_cast<const T *>(buf.as<char>() + at); }

}  // namespace

struct fa_fbank_plan {
    fa_ctx *ctx = nullptr;
    int32_t batch = 0;
    int64_t total_samples = 0;
    int64_t grid = 0;
    size_t lds = 0;
    fa::DevBuf dev;   // every device-side table of the plan
    FbankArgs args{};
};

extern "C" {

void fa_fbank_default_config(fa_fbank_config *c) {
    if (!c) return;
    c->sample_rate = 16000; c->n_mels = 80; c->n_fft = 512; c->hop = 160; c->win = 400;
    c->waveform_scale = 32768.0f; c->preemph = 0.97f; c->low_freq = 20.0f; c->high_freq = 0.0f; c->log_floor = 1.1920929e-07f;
    c->window_type = FA_FBANK_WINDOW_HAMMING; c->remove_dc = 1;
    c->lfr_m = 7; c->lfr_n = 6; c->tail_mode = FA_FBANK_TAIL_REPLICATE;
    c->window = nullptr; c->filterbank = nullptr;
}

int32_t fa_fbank_num_frames(const fa_fbank_config *c, int64_t n) {
    if (!c || n <= 0 || c->hop < 1 || c->win < 1) return 0;
    const int64_t T = num_frames(n, c->win, c->hop);
    return T > INT32_MAX ? 0 : static_cast<int32_t>(T);
}

int32_t fa_fbank_num_rows(const fa_fbank_config *c, int32_t frames) {
    if (!c || frames <= 0 || c->lfr_m < 1 || c->lfr_n < 1) return 0;
    return static_cast<int32_t>(num_rows(frames, c->lfr_m, c->lfr_n, c->tail_mode));
}

fa_status fa_fbank_window(const fa_fbank_config *c, float *out) {
    if (!c || !out || c->win < 2) return FA_INVALID_ARGUMENT;
    return fa::no_throw(nullptr, "fa_fbank_window", [&]() -> fa_status {
        std::vector<float> w;
        make_window(c, w);
        memcpy(out, w.data(), sizeof(float) * w.size());
        return FA_SUCCESS;
    });
}

fa_status fa_fbank_filterbank(const fa_fbank_config *c, float *out) {
    if (!c || !out || c->n_fft < 2 || c->n_mels < 1 || c->sample_rate < 1) return FA_INVALID_ARGUMENT;
    return fa::no_throw(nullptr, "fa_fbank_filterbank", [&]() -> fa_status {
        std::vector<float> fb;
        make_filterbank(c, fb);
        memcpy(out, fb.data(), sizeof(float) * fb.size());
        return FA_SUCCESS;
    });
}

fa_status fa_fbank_plan_create(fa_ctx *ctx, const fa_fbank_config *cfg, const int64_t *offsets, int32_t batch, const float *shift,
                               const float *scale, int32_t row_stride, fa_fbank_plan **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    if (validate(cfg) != FA_SUCCESS) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "fbank: unsupported configuration");
    if (!offsets || batch < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "fbank: empty batch");
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fbank plan", [&]() -> fa_status {
        std::unique_ptr<fa_fbank_plan> p(new fa_fbank_plan());
        p->ctx = ctx;
        p->batch = batch;
        int64_t max_frames = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t len = offsets[b + 1] - offsets[b];
            if (len < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "fbank: offsets not monotone");
            const int64_t T = num_frames(len, cfg->win, cfg->hop);
            if (T > max_frames) max_frames = T;
        }
        if (max_frames > INT32_MAX / 2) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "fbank: utterance too long");
        const int64_t max_rows = num_rows(max_frames, cfg->lfr_m, cfg->lfr_n, cfg->tail_mode);
        if (row_stride <= 0) row_stride = static_cast<int32_t>(max_rows > 0 ? max_rows : 1);
        if (row_stride < max_rows) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "fbank: row_stride too small");
        p->total_samples = offsets[batch];

        const int bins = cfg->n_fft / 2 + 1;
        std::vector<float> window, fb, weights, windowz(fa::melcore::kNfft, 0.0f);
        make_window(cfg, window);
        make_filterbank(cfg, fb);
        for (int i = 0; i < cfg->win; ++i) windowz[i] = window[i];   // the frame sits at position 0 of the 512 buffer, as in Kaldi
        std::vector<int32_t> tab(2 * static_cast<size_t>(cfg->n_mels), 0);
        for (int m = 0; m < cfg->n_mels; ++m) {   // a row's support: first to last non-zero bin, interior zeros kept
            int l0 = -1, h0 = -1;
            for (int k = 0; k < bins; ++k) if (fb[static_cast<size_t>(m) * bins + k] != 0.0f) { if (l0 < 0) l0 = k; h0 = k; }
            const int cnt = l0 < 0 ? 0 : h0 - l0 + 1;
            tab[2 * m] = (l0 < 0 ? 0 : l0) | (cnt << 16);
            tab[2 * m + 1] = static_cast<int32_t>(weights.size());
            for (int j = 0; j < cnt; ++j) weights.push_back(fb[static_cast<size_t>(m) * bins + l0 + j]);
        }
        if (weights.empty()) weights.push_back(0.0f);

        FbankArgs &a = p->args;
        a.row_floats = cfg->lfr_m * cfg->n_mels;
        a.row_stride = row_stride;
        a.utt_stride = static_cast<int64_t>(row_stride) * a.row_floats;
        a.tiles_per_utt = static_cast<int32_t>(max_frames > 0 ? (max_frames + kTileFrames - 1) / kTileFrames : 1);
        p->grid = static_cast<int64_t>(a.tiles_per_utt) * batch;
        if (p->grid > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "fbank: too many tiles in one plan");
        a.n_mels = cfg->n_mels; a.n_weights = static_cast<int32_t>(weights.size());
        a.win = cfg->win; a.hop = cfg->hop;
        a.stage_alloc = ((kTileFrames - 1) * cfg->hop + cfg->win + 3) & ~3;
        a.lfr_m = cfg->lfr_m; a.lfr_n = cfg->lfr_n; a.tail = cfg->tail_mode; a.remove_dc = cfg->remove_dc != 0;
        a.wave_scale = cfg->waveform_scale; a.preemph = cfg->preemph; a.log_floor = cfg->log_floor;
        a.log_of_floor = static_cast<float>(log(static_cast<double>(cfg->log_floor)));
        p->lds = lds_bytes(a);
        if (p->lds > 64 * 1024) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "fbank: hop too large for LDS staging");

        Image img;
        const size_t o_off = img.add(offsets, static_cast<size_t>(batch) + 1), o_win = img.add(windowz.data(), windowz.size());
        const std::vector<float2> t256 = twiddles(256, 256), t512 = twiddles(129, 512);
        const size_t o_t256 = img.add(t256.data(), t256.size()), o_t512 = img.add(t512.data(), t512.size());
        const size_t o_tab = img.add(tab.data(), tab.size()), o_w = img.add(weights.data(), weights.size());
        const size_t o_shift = shift ? img.add(shift, static_cast<size_t>(a.row_floats)) : 0, o_scale = scale ? img.add(scale, static_cast<size_t>(a.row_floats)) : 0;
        if (p->dev.alloc(img.bytes.size()) != hipSuccess) { (void)hipGetLastError(); return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "fbank plan: device allocation failed"); }
        FA_HIP_TRY(ctx, hipMemcpy(p->dev.p, img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice));
        place(a.offsets, p->dev, o_off); place(a.windowz, p->dev, o_win); place(a.tw256, p->dev, o_t256); place(a.tw512, p->dev, o_t512);
        place(a.mel_tab, p->dev, o_tab); place(a.mel_w, p->dev, o_w);
        if (shift) place(a.shift, p->dev, o_shift);
        if (scale) place(a.scale, p->dev, o_scale);
        *out = p.release();
        return FA_SUCCESS;
    });
}

void fa_fbank_plan_destroy(fa_fbank_plan *p) {
    if (!p) return;
    if (p->dev.p) { (void)hipSetDevice(p->ctx->device); (void)hipStreamSynchronize(p->ctx->stream); }
    delete p;
}

int32_t fa_fbank_plan_row_stride(const fa_fbank_plan *p) { return p ? p->args.row_stride : 0; }
int64_t fa_fbank_plan_utt_stride(const fa_fbank_plan *p) { return p ? p->args.utt_stride : 0; }

fa_status fa_fbank_execute_dev(fa_fbank_plan *p, const float *d_pcm, float *d_out, int32_t *d_rows) {
    if (!p || !d_out || (!d_pcm && p->total_samples > 0)) return FA_INVALID_ARGUMENT;
    fa_ctx *ctx = p->ctx;
    fa::DeviceGuard guard(ctx->device);
    FbankArgs a = p->args;
    a.pcm = d_pcm; a.out = d_out; a.rows = d_rows;
    a.vec = a.n_mels % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
    launch(a, p->grid, ctx->stream);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

fa_status fa_fbank_batch(fa_ctx *ctx, const fa_fbank_config *cfg, const float *pcm, const int64_t *offsets, int32_t batch, const float *shift,
                         const float *scale, int32_t row_stride, float *out, int32_t *rows) {
    if (!ctx || !out || !offsets || batch < 1) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_fbank_batch", [&]() -> fa_status {
        fa_fbank_plan *plan = nullptr;
        FA_TRY(fa_fbank_plan_create(ctx, cfg, offsets, batch, shift, scale, row_stride, &plan));
        std::unique_ptr<fa_fbank_plan, void (*)(fa_fbank_plan *)> owner(plan, fa_fbank_plan_destroy);
        const int64_t ns = offsets[batch];
        if (ns > 0 && !pcm) return FA_INVALID_ARGUMENT;
        const size_t out_floats = static_cast<size_t>(plan->args.utt_stride) * batch;
        fa::DevBuf d_pcm, d_out, d_rows;
        FA_TRY(fa::take(ctx, "fa_fbank_batch", {{&d_pcm, sizeof(float) * static_cast<size_t>(ns), true, pcm}, {&d_out, sizeof(float) * out_floats},
                                               {&d_rows, sizeof(int32_t) * static_cast<size_t>(batch)}}));
        FA_TRY(fa_fbank_execute_dev(plan, d_pcm.as<float>(), d_out.as<float>(), d_rows.as<int32_t>()));
        FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, sizeof(float) * out_floats, hipMemcpyDeviceToHost, ctx->stream));
        if (rows) FA_HIP_TRY(ctx, hipMemcpyAsync(rows, d_rows.p, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, ctx->stream));
        FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the one synchronisation; the buffers go back to the cache behind it
        return FA_SUCCESS;
    });
}

}  // extern "C"
