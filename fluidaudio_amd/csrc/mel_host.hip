// mel_host.hip — host side of the mel featurizer (kernels: mel.hip): Hann / filterbank tables, configuration checks, plans
// (fa_mel_plan_*), the per-context plan cache of small host-pointer calls, the host-pointer entry fa_mel_batch with its PCIe
// slicing, and the per-feature normalisation (kernel and entry: it shares nothing with the featurizer kernels).
// Built with the default flags (no -ffp-contract=off): the tables below are bit-identical to what the kernels were tuned and tested with.
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "mel_launch.h"

using namespace fa::mel;

namespace {

// ----------------------------------------------------------------------------- host tables
// createHannWindow (:553-562)
void make_hann(int win, bool periodic, std::vector<float> &w) {
    w.resize(win);
    const float divisor = periodic ? static_cast<float>(win) : static_cast<float>(win - 1);
    const float pi_f = static_cast<float>(M_PI);
    for (int i = 0; i < win; ++i) {
        const float phase = 2.0f * pi_f * static_cast<float>(i) / divisor;
        w[i] = 0.5f * (1.0f - cosf(phase));
    }
}

float hz_to_mel(float hz) {  // :575-586
    const float f_sp = 200.0f / 3.0f, min_log_hz = 1000.0f;
    const float min_log_mel = min_log_hz / f_sp, log_step = logf(6.4f) / 27.0f;
    return hz >= min_log_hz ? min_log_mel + logf(hz / min_log_hz) / log_step : hz / f_sp;
}
float mel_to_hz(float mel) {  // :588-599
    const float f_sp = 200.0f / 3.0f, min_log_hz = 1000.0f;
    const float min_log_mel = min_log_hz / f_sp, log_step = logf(6.4f) / 27.0f;
    return mel >= min_log_mel ? min_log_hz * expf(log_step * (mel - min_log_mel)) : f_sp * mel;
}

// createMelFilterbank (:564-642), dense [n_mels][bins]
void make_filterbank(int n_fft, int n_mels, int sr, std::vector<float> &fb) {
    const int bins = n_fft / 2 + 1;
    fb.assign(static_cast<size_t>(n_mels) * bins, 0.0f);
    const float mel_min = hz_to_mel(0.0f), mel_max = hz_to_mel(static_cast<float>(sr) / 2.0f);
    std::vector<float> pts(n_mels + 2), freqs(bins);
    for (int i = 0; i < n_mels + 2; ++i)
        pts[i] = mel_to_hz(mel_min + static_cast<float>(i) * (mel_max - mel_min) / static_cast<float>(n_mels + 1));
    for (int i = 0; i < bins; ++i) freqs[i] = static_cast<float>(i) * static_cast<float>(sr) / static_cast<float>(n_fft);
    for (int m = 0; m < n_mels; ++m) {
        const float fl = pts[m], fc = pts[m + 1], fr = pts[m + 2];
        const float norm = 2.0f / (fr - fl);
        for (int k = 0; k < bins; ++k) {
            const float f = freqs[k];
            if (f >= fl && f < fc) fb[static_cast<size_t>(m) * bins + k] = norm * (f - fl) / (fc - fl);
            else if (f >= fc && f <= fr) fb[static_cast<size_t>(m) * bins + k] = norm * (fr - f) / (fr - fc);
        }
    }
}

// torchaudio melscale_fbanks(norm: nil, mel_scale: "htk") as built by LuxTtsMelExtractor.htkMelFilterbank
// (Sources/FluidAudio/TTS/LuxTts/LuxTtsMelExtractor.swift:160-189): double arithmetic, rounded to float at the end
void make_filterbank_htk(int n_fft, int n_mels, int sr, std::vector<float> &fb) {
    const int bins = n_fft / 2 + 1;
    fb.assign(static_cast<size_t>(n_mels) * bins, 0.0f);
    const double f_max = static_cast<double>(sr) / 2.0;
    auto hz_to_mel_htk = [](double hz) { return 2595.0 * log10(1.0 + hz / 700.0); };
    auto mel_to_hz_htk = [](double mel) { return 700.0 * (pow(10.0, mel / 2595.0) - 1.0); };
    const double mel_min = hz_to_mel_htk(0.0), mel_max = hz_to_mel_htk(f_max);
    std::vector<double> pts(n_mels + 2), freqs(bins);
    for (int i = 0; i < n_mels + 2; ++i) pts[i] = mel_to_hz_htk(mel_min + static_cast<double>(i) * (mel_max - mel_min) / static_cast<double>(n_mels + 1));
    for (int b = 0; b < bins; ++b) freqs[b] = static_cast<double>(b) * f_max / static_cast<double>(bins - 1);
    for (int m = 0; m < n_mels; ++m)
        for (int b = 0; b < bins; ++b) {
            const double up = (freqs[b] - pts[m]) / (pts[m + 1] - pts[m]), down = (pts[m + 2] - freqs[b]) / (pts[m + 2] - pts[m + 1]);
            const double v = up < down ? up : down;
            fb[static_cast<size_t>(m) * bins + b] = static_cast<float>(v > 0.0 ? v : 0.0);
        }
}

// the bank a configuration asks for: caller's table, HTK/no-norm, or the reference's Slaney bank
void config_filterbank(const fa_mel_config *c, std::vector<float> &fb) {
    const size_t n = static_cast<size_t>(c->n_mels) * (c->n_fft / 2 + 1);
    if (c->filterbank) fb.assign(c->filterbank, c->filterbank + n);
    else if (c->mel_scale == FA_MEL_SCALE_HTK_NONORM) make_filterbank_htk(c->n_fft, c->n_mels, c->sample_rate, fb);
    else make_filterbank(c->n_fft, c->n_mels, c->sample_rate, fb);
}

fa_status validate(const fa_mel_config *c) {
    if (!c) return FA_INVALID_ARGUMENT;
    if (c->n_fft < 64 || c->n_fft > 2048 || (c->n_fft & (c->n_fft - 1)) != 0) return FA_INVALID_ARGUMENT;  // power of two
    if (c->win < 2 || c->win > c->n_fft || c->hop < 1 || c->hop > 4096) return FA_INVALID_ARGUMENT;
    if (c->n_mels < 1 || c->n_mels > kMaxMels || c->sample_rate < 1) return FA_INVALID_ARGUMENT;
    if (c->padding_mode < 0 || c->padding_mode > 2 || c->layout < 0 || c->layout > 1) return FA_INVALID_ARGUMENT;
    if (c->floor_mode < 0 || c->floor_mode > 1) return FA_INVALID_ARGUMENT;
    if (c->power != 0.0f && c->power != 1.0f && c->power != 2.0f) return FA_INVALID_ARGUMENT;
    if (c->center_pad < 0 || c->center_pad > 1 || c->mel_scale < 0 || c->mel_scale > 1 || c->tail_mode < 0 || c->tail_mode > 1) return FA_INVALID_ARGUMENT;
    return FA_SUCCESS;
}

// configurations the tuned n_fft = 512 kernels do not cover take mel_generic_kernel
bool needs_generic(const fa_mel_config *c) {
    return c->n_fft != kNfft || c->power == 1.0f || (c->center_pad == FA_MEL_CENTER_REFLECT && c->padding_mode == FA_MEL_PAD_CENTER) ||
           c->tail_mode == FA_MEL_TAIL_REPLICATE || fa::sw_on(fa::Sw::MEL_GENERIC);
}

// support of every filterbank row: its first non-zero bin and the bins up to its last one (interior zeros kept); an empty row is (0, 0)
void sparse_rows(const std::vector<float> &fb, int n_mels, int bins, std::vector<int32_t> &lo, std::vector<int32_t> &cnt) {
    lo.assign(n_mels, 0);
    cnt.assign(n_mels, 0);
    for (int m = 0; m < n_mels; ++m) {
        int l0 = -1, h0 = -1;
        for (int k = 0; k < bins; ++k) if (fb[static_cast<size_t>(m) * bins + k] != 0.0f) { if (l0 < 0) l0 = k; h0 = k; }
        if (l0 >= 0) { lo[m] = l0; cnt[m] = h0 - l0 + 1; }
    }
}

// exp(-2 pi i k / n), k = 0 .. count - 1
std::vector<float2> twiddles(int count, int n) {
    std::vector<float2> tw(count);
    for (int k = 0; k < count; ++k) { const double a = -2.0 * M_PI * k / n; tw[k] = make_float2((float)cos(a), (float)sin(a)); }
    return tw;
}

// The device-side tables of a plan: arrays appended to one host image at 256-byte aligned offsets, each bound to the pointer of the
// kernel's argument struct that is to address it; upload() copies the image into one allocation and sets those pointers.
struct TableBlob {
    std::vector<char> image;
    std::vector<std::pair<void *, size_t>> bound;   // (where the device pointer goes, the array's offset)
    template <class P, class T> void add(P *&dst, const T *src, size_t n) {   // src == nullptr: zeros
        static_assert(std::is_same<typename std::remove_const<P>::type, T>::value, "table and pointer types differ");
        bound.emplace_back(&dst, image.size());
        image.resize((image.size() + sizeof(T) * n + 255) & ~static_cast<size_t>(255), 0);
        if (src) memcpy(image.data() + bound.back().second, src, sizeof(T) * n);
    }
    template <class P, class T> void add(P *&dst, const std::vector<T> &v) { add(dst, v.data(), v.size()); }
    fa_status upload(fa_ctx *ctx, fa::DevBuf &buf) {
        hipError_t e = buf.alloc(image.size());
        if (e != hipSuccess) return fa::hip_status(ctx, e, "mel plan hipMalloc");
        e = hipMemcpy(buf.p, image.data(), image.size(), hipMemcpyHostToDevice);
        for (auto &b : bound) { char *d = buf.as<char>() + b.second; memcpy(b.first, &d, sizeof(d)); }
        return fa::hip_status(ctx, e, "mel plan upload");
    }
};

}  // namespace

struct fa_mel_plan {
    fa_ctx *ctx = nullptr;
    fa_mel_config cfg{};
    int32_t batch = 0;
    int32_t frame_stride = 0;
    int64_t utt_stride = 0;
    int64_t total_frames = 0;
    int64_t total_samples = 0;
    fa::DevBuf dev;       // one allocation holding every device-side table of the plan
    Variant kernel;       // the kernel the plan runs; generic: `gargs` are its arguments, otherwise `args`
    MelArgs args{};
    fa::melgen::GenArgs gargs{};
    size_t lds_bytes = 0;
    int grid = 0;
    unsigned long long launches = 0;   // v4 launches made so far (spaces the tile-queue ranges)
};

extern "C" {

void fa_mel_default_config(fa_mel_config *c) {
    if (!c) return;
    c->sample_rate = 16000; c->n_mels = 128; c->n_fft = 512; c->hop = 160; c->win = 400;
    c->preemph = 0.97f; c->pad_to = 0; c->log_floor = ldexpf(1.0f, -24);
    c->floor_mode = FA_MEL_FLOOR_ADDITIVE; c->window_periodic = 0;
    c->padding_mode = FA_MEL_PAD_CENTER; c->layout = FA_MEL_LAYOUT_MEL_MAJOR;
    c->power = 2.0f; c->center_pad = FA_MEL_CENTER_ZERO; c->mel_scale = FA_MEL_SCALE_SLANEY; c->tail_mode = FA_MEL_TAIL_ZERO;
    c->filterbank = nullptr;
}

int32_t fa_mel_num_frames(const fa_mel_config *c, int64_t n) {
    if (!c || n <= 0 || c->hop < 1) return 0;
    int64_t frames;
    switch (c->padding_mode) {
        case FA_MEL_PAD_CENTER: frames = 1 + (n + 2 * static_cast<int64_t>(c->n_fft / 2) - c->win) / c->hop; break;  // :195-197
        case FA_MEL_PAD_PREPADDED: frames = (n - c->n_fft) / c->hop + 1; if (frames < 0) frames = 0; break;          // :345
        default: frames = 1 + (n - c->win) / c->hop; break;                                                          // :133
    }
    if (frames <= 0) return 0;
    return frames > INT32_MAX ? 0 : static_cast<int32_t>(frames);
}

int32_t fa_mel_padded_frames(const fa_mel_config *c, int32_t frames) {
    if (!c) return 0;
    const int32_t p = c->pad_to > 1 ? c->pad_to : 1;  // :72
    return ((frames + p - 1) / p) * p;                // :204,:354
}

fa_status fa_mel_hann_window(const fa_mel_config *c, float *out) {
    if (!c || !out || c->win < 1) return FA_INVALID_ARGUMENT;
    std::vector<float> w;
    make_hann(c->win, c->window_periodic != 0, w);
    memcpy(out, w.data(), sizeof(float) * w.size());
    return FA_SUCCESS;
}

fa_status fa_mel_filterbank(const fa_mel_config *c, float *out) {
    if (!c || !out || c->n_fft < 2 || c->n_mels < 1) return FA_INVALID_ARGUMENT;
    std::vector<float> fb;
    config_filterbank(c, fb);
    memcpy(out, fb.data(), sizeof(float) * fb.size());
    return FA_SUCCESS;
}

fa_status fa_mel_plan_create(fa_ctx *ctx, const fa_mel_config *cfg, const int64_t *offsets, int32_t batch,
                             const int32_t *expected_frames, int32_t frame_stride, fa_mel_plan **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    if (validate(cfg) != FA_SUCCESS) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "mel: unsupported configuration");
    if (!offsets || batch < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "mel: empty batch");
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "mel plan", [&]() -> fa_status {
        std::unique_ptr<fa_mel_plan> p(new fa_mel_plan());
        p->ctx = ctx;
        const int bins = cfg->n_fft / 2 + 1;
        std::vector<int32_t> frames(batch), natural(batch);
        int32_t max_padded = 1;
        for (int b = 0; b < batch; ++b) {
            const int64_t len = offsets[b + 1] - offsets[b];
            if (len < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "mel: offsets not monotone");
            int32_t T = fa_mel_num_frames(cfg, len);
            natural[b] = T;
            if (expected_frames && len > 0) T = expected_frames[b] > 0 ? expected_frames[b] : 0;  // :347
            frames[b] = T;
            p->total_frames += T;
            const int32_t tp = T > 0 ? fa_mel_padded_frames(cfg, T) : 1;
            if (tp > max_padded) max_padded = tp;
        }
        p->total_samples = offsets[batch];
        if (frame_stride <= 0) frame_stride = max_padded;
        if (frame_stride < max_padded) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "mel: frame_stride too small");
        p->frame_stride = frame_stride;
        p->utt_stride = static_cast<int64_t>(frame_stride) * cfg->n_mels;

        // tables: window, filterbank rows as (first bin, count), and the rows' weights back to back (not for the fast bank)
        std::vector<float> hann, fb, weights;
        make_hann(cfg->win, cfg->window_periodic != 0, hann);
        config_filterbank(cfg, fb);
        const int off = cfg->padding_mode == FA_MEL_PAD_LEGACY ? 0 : (cfg->n_fft - cfg->win) / 2;  // :234 / :148-153
        std::vector<int32_t> lo, cnt, start(cfg->n_mels, 0);
        sparse_rows(fb, cfg->n_mels, bins, lo, cnt);
        auto pack_rows = [&] {
            for (int m = 0; m < cfg->n_mels; ++m) {
                start[m] = static_cast<int32_t>(weights.size());
                for (int j = 0; j < cnt[m]; ++j) weights.push_back(fb[static_cast<size_t>(m) * bins + lo[m] + j]);
            }
        };
        Variant &kn = p->kernel;
        kn.layout = cfg->layout;
        kn.clamped = cfg->floor_mode == FA_MEL_FLOOR_CLAMPED;
        TableBlob blob;
        if (needs_generic(cfg)) {
            // sparse rows, window, twiddles exp(-2 pi i k / n_fft)
            const int N = cfg->n_fft;
            pack_rows();
            if (weights.empty()) weights.push_back(0.0f);
            fa::melgen::GenArgs &g = p->gargs;
            blob.add(g.offsets, offsets, static_cast<size_t>(batch) + 1);
            blob.add(g.frames, frames);
            blob.add(g.stft_frames, natural);
            blob.add(g.window, hann.data(), cfg->win);
            blob.add(g.tw, twiddles(N / 2 + 1, N));
            blob.add(g.mel_lo, lo);
            blob.add(g.mel_cnt, cnt);
            blob.add(g.mel_start, start);
            blob.add(g.mel_w, weights);
            FA_TRY(blob.upload(ctx, p->dev));
            g.utt_stride = p->utt_stride; g.batch = batch; g.frame_stride = frame_stride; g.n_mels = cfg->n_mels; g.n_fft = N;
            g.log2_m = 0; while ((2 << g.log2_m) < N) ++g.log2_m;           // log2(N / 2)
            g.win = cfg->win; g.off = off; g.hop = cfg->hop;
            g.pad = cfg->padding_mode == FA_MEL_PAD_CENTER ? N / 2 : 0;
            g.preemph = cfg->padding_mode == FA_MEL_PAD_LEGACY ? 0.0f : cfg->preemph;
            g.log_floor = cfg->log_floor; g.floor_clamped = kn.clamped;
            g.reflect = cfg->center_pad == FA_MEL_CENTER_REFLECT && cfg->padding_mode == FA_MEL_PAD_CENTER;
            g.magnitude = cfg->power == 1.0f; g.tail_replicate = cfg->tail_mode == FA_MEL_TAIL_REPLICATE;
            g.frame_major = cfg->layout == FA_MEL_LAYOUT_FRAME_MAJOR;
            kn.generic = true;
            p->lds_bytes = sizeof(float) * fa::melgen::kWaves * (2 * static_cast<size_t>(N) + 8);
            if (p->lds_bytes > 64 * 1024) raise_lds_limit(kn, p->lds_bytes);
            const int64_t items = (static_cast<int64_t>(batch) * frame_stride + fa::melgen::kWaves - 1) / fa::melgen::kWaves;
            p->grid = static_cast<int>(items < 256 * 16 ? (items < 1 ? 1 : items) : 256 * 16);
            *out = p.release();
            return FA_SUCCESS;
        }
        std::vector<float> windowz(kNfft, 0.0f);
        for (int i = 0; i < cfg->win; ++i) windowz[off + i] = hann[i];
        kn.edge_zero = true;
        for (int i = 0; i < 32; ++i) if (windowz[i] != 0.0f || windowz[kNfft - 32 + i] != 0.0f) kn.edge_zero = false;
        std::vector<int32_t> tab(cfg->n_mels);
        kn.fast = cfg->n_mels <= kFastGroups * kGroup;
        for (int m = 0; m < cfg->n_mels; ++m)
            if (cnt[m] > fast_slots(m / kGroup < kFastGroups ? m / kGroup : kFastGroups - 1)) kn.fast = false;
        if (kn.fast) {  // [slot][lane] zero-padded weights; mel_tab keeps (lo, cnt) and a dummy start
            weights.assign(static_cast<size_t>(kFastSlots) * kGroup, 0.0f);
            for (int m = 0; m < cfg->n_mels; ++m) {
                const int i = m / kGroup, l = m % kGroup;
                for (int j = 0; j < cnt[m]; ++j)
                    weights[static_cast<size_t>(fast_slot_base(i) + j) * kGroup + l] = fb[static_cast<size_t>(m) * bins + lo[m] + j];
            }
        } else {
            pack_rows();
        }
        for (int m = 0; m < cfg->n_mels; ++m) tab[m] = lo[m] | (cnt[m] << 10) | (start[m] << 20);
        if (weights.empty()) weights.push_back(0.0f);
        MelArgs &a = p->args;
        blob.add(a.offsets, offsets, static_cast<size_t>(batch) + 1);
        blob.add(a.frames, frames);
        blob.add(a.windowz, windowz);
        blob.add(a.tw256, twiddles(256, 256));
        blob.add(a.tw512, twiddles(129, 512));
        blob.add(a.mel_tab, tab);
        blob.add(a.mel_w, weights);
        blob.add(a.queue, static_cast<const unsigned long long *>(nullptr), 1);   // mel_kernel_v4's tile counter starts at zero
        FA_TRY(blob.upload(ctx, p->dev));
        a.utt_stride = p->utt_stride;
        a.tiles_per_utt = (frame_stride + kTileFrames - 1) / kTileFrames;
        a.total_tiles = static_cast<int64_t>(a.tiles_per_utt) * batch;
        if (a.total_tiles > INT32_MAX) return fa::set_error(ctx, FA_INDEX_OVERFLOW, "mel: too many tiles in one plan");
        a.frame_stride = frame_stride;
        a.n_mels = cfg->n_mels;
        a.n_weights = static_cast<int32_t>(weights.size());
        a.hop = cfg->hop;
        a.pad = cfg->padding_mode == FA_MEL_PAD_CENTER ? cfg->n_fft / 2 : 0;
        a.stage_count = (kTileFrames - 1) * cfg->hop + kNfft;
        a.stage_alloc = (a.stage_count + 3) & ~3;
        {
            const int mm = cfg->n_mels * kMelPad, fm = kTileFrames * (cfg->n_mels + kFramePad);
            a.out_alloc = ((mm > fm ? mm : fm) + 3) & ~3;
        }
        a.preemph = cfg->padding_mode == FA_MEL_PAD_LEGACY ? 0.0f : cfg->preemph;  // compute() has no pre-emphasis (:146-153)
        a.log_floor = cfg->log_floor;
        a.floor_clamped = kn.clamped;
        a.prio_lo = 0; a.prio_hi = 3; a.prio_pw = 1; a.prio_rd = 2;   // measured best of the sweep in DESIGN.md §3.1
        kn.pk = kn.fast && cfg->hop == kPkHop;
        kn.v4 = kn.pk && cfg->n_mels == kFastGroups * kGroup;
        p->lds_bytes = sizeof(float) * (a.stage_alloc + kRegions * (kn.pk ? kRegionFloatsPk : kRegionFloats) + a.out_alloc) + sizeof(int32_t) * kMaxMels +
                       sizeof(float) * (static_cast<size_t>(a.n_weights) + 24 + 4 + (kn.pk ? fa::melpk::kWindowTableFloats : 0));   // the paired weight reads of the packed kernel touch one slot row past the table
        if (kn.v4) p->lds_bytes = kV4LdsBytes;
        if (p->lds_bytes > 160 * 1024) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "mel: hop too large for LDS staging");
        if (p->lds_bytes > 64 * 1024) raise_lds_limit(kn, p->lds_bytes);
        hipDeviceProp_t prop;
        const int cus = hipGetDeviceProperties(&prop, ctx->device) == hipSuccess ? prop.multiProcessorCount : 256;
        // Equal-length batches: one persistent round (the per-workgroup prologue — tables, lane constants — is paid once:
        // 0.663 vs 0.685 ms with four rounds on the bench workload).  Ragged batches keep four rounds, so that the hardware
        // scheduler evens out ranges that hold many empty tiles of short utterances.
        bool uniform = true;
        for (int b = 1; b < batch; ++b) if (frames[b] != frames[0]) { uniform = false; break; }
        const int rounds = uniform ? 1 : 4;
        const int64_t want = static_cast<int64_t>(cus) * (kn.v4 ? 3 : 2) * rounds;  // resident workgroups per CU (mel_kernel_v4: three), `rounds` rounds of them
        p->grid = static_cast<int>(a.total_tiles < want ? a.total_tiles : want);
        if (p->grid < 1) p->grid = 1;
        *out = p.release();
        return FA_SUCCESS;
    });
}

void fa_mel_plan_destroy(fa_mel_plan *p) {
    if (!p) return;
    if (p->dev.p) { (void)hipSetDevice(p->ctx->device); (void)hipStreamSynchronize(p->ctx->stream); }
    delete p;   // releases the tables
}

int64_t fa_mel_plan_utt_stride(const fa_mel_plan *p) { return p ? p->utt_stride : 0; }
int32_t fa_mel_plan_frame_stride(const fa_mel_plan *p) { return p ? p->frame_stride : 0; }
int64_t fa_mel_plan_total_frames(const fa_mel_plan *p) { return p ? p->total_frames : 0; }

fa_status fa_mel_execute_dev(fa_mel_plan *p, const float *d_pcm, const float *d_last, float *d_mel, int32_t *d_lengths) {
    if (!p || !d_mel || (!d_pcm && p->total_samples > 0)) return FA_INVALID_ARGUMENT;
    fa_ctx *ctx = p->ctx;
    fa::DeviceGuard guard(ctx->device);
    if (p->kernel.generic) {
        fa::melgen::GenArgs g = p->gargs;
        g.pcm = d_pcm; g.last = d_last; g.out = d_mel; g.lengths = d_lengths;
        launch(p->kernel, p->grid, p->lds_bytes, ctx->stream, &g);
    } else {
        MelArgs a = p->args;
        a.pcm = d_pcm; a.last = d_last; a.out = d_mel; a.lengths = d_lengths;
        // mel_kernel_v4: every workgroup draws one index per tile it processes plus the two it holds when it stops (the queue runs two
        // tiles ahead): a launch advances the counter by exactly total_tiles + 2 grid
        if (p->kernel.v4) a.queue_base = p->launches++ * (static_cast<unsigned long long>(a.total_tiles) + 2ull * static_cast<unsigned long long>(p->grid));
        launch(p->kernel, p->grid, p->lds_bytes, ctx->stream, &a);
    }
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

// Plans of small host-pointer calls, kept per context (see fa_mel_batch).  Key = everything fa_mel_plan_create looks at.
}  // extern "C"
namespace {
constexpr int32_t kMelCacheMaxBatch = 8;
constexpr size_t kMelCacheEntries = 8;
constexpr size_t kMelCfgKeyBytes = offsetof(fa_mel_config, tail_mode) + sizeof(int32_t);   // every field in front of the filterbank pointer, no padding
struct MelPlanCache {
    struct Entry {
        fa_mel_config cfg;
        int32_t batch, frame_stride;
        bool has_expected;
        std::vector<int64_t> offsets;
        std::vector<int32_t> expected;
        fa_mel_plan *plan;
    };
    std::vector<Entry> entries;
};
void mel_cache_free(void *p) {
    MelPlanCache *c = static_cast<MelPlanCache *>(p);
    if (!c) return;
    for (auto &en : c->entries) fa_mel_plan_destroy(en.plan);
    delete c;
}
fa_status mel_cached_plan(fa_ctx *ctx, const fa_mel_config *cfg, const int64_t *offsets, int32_t batch, const int32_t *expected_frames,
                          int32_t frame_stride, fa_mel_plan **out) {
    return fa::no_throw(ctx, "mel plan cache", [&]() -> fa_status {
        if (!ctx->mel_cache) { ctx->mel_cache = new MelPlanCache; ctx->mel_cache_free = mel_cache_free; }
        MelPlanCache *c = static_cast<MelPlanCache *>(ctx->mel_cache);
        for (auto &en : c->entries) {
            if (en.batch != batch || en.frame_stride != frame_stride || en.has_expected != (expected_frames != nullptr)) continue;
            if (memcmp(&en.cfg, cfg, kMelCfgKeyBytes) != 0) continue;
            if (memcmp(en.offsets.data(), offsets, sizeof(int64_t) * (batch + 1)) != 0) continue;
            if (expected_frames && memcmp(en.expected.data(), expected_frames, sizeof(int32_t) * batch) != 0) continue;
            *out = en.plan;
            return FA_SUCCESS;
        }
        // everything that allocates on the host comes before the plan exists: nothing below can lose it
        MelPlanCache::Entry en{*cfg, batch, frame_stride, expected_frames != nullptr, std::vector<int64_t>(offsets, offsets + batch + 1), {}, nullptr};
        if (expected_frames) en.expected.assign(expected_frames, expected_frames + batch);
        c->entries.reserve(kMelCacheEntries + 1);
        FA_TRY(fa_mel_plan_create(ctx, cfg, offsets, batch, expected_frames, frame_stride, &en.plan));
        if (c->entries.size() >= kMelCacheEntries) { fa_mel_plan_destroy(c->entries.front().plan); c->entries.erase(c->entries.begin()); }
        c->entries.push_back(std::move(en));
        *out = c->entries.back().plan;
        return FA_SUCCESS;
    });
}

// second stream, per-slice events and per-slice plans of fa_mel_batch's sliced route
struct SliceSet {
    hipStream_t down = nullptr;
    std::vector<hipEvent_t> done;
    std::vector<fa_mel_plan *> plans;
    ~SliceSet() {
        for (auto *pl : plans) if (pl) fa_mel_plan_destroy(pl);
        for (auto ev : done) if (ev) (void)hipEventDestroy(ev);
        if (down) (void)hipStreamDestroy(down);
    }
};
}  // namespace
extern "C" {

// Host-pointer entry.  Pageable host buffers: copy in, kernel, copy out on the context's stream (each copy is a staged copy inside
// the runtime at ~55 GB/s; measured: slicing + a second host thread does not overlap the two directions, the staging serialises).
// PINNED host buffers (fa_host_alloc, or memory the caller registered with the HIP runtime): the batch is cut into slices of
// utterances (~64 MB of samples each), slice k + 1 is uploaded and launched on the context's stream while the log-mel of slice k
// is downloaded on a second stream — true DMA in both directions of the PCIe link at once.  One slice = one plan.
fa_status fa_mel_batch(fa_ctx *ctx, const fa_mel_config *cfg, const float *pcm, const int64_t *offsets, int32_t batch,
                       const float *last_samples, const int32_t *expected_frames, int32_t frame_stride, float *mel,
                       int32_t *mel_lengths) {
    if (!ctx || !mel || !offsets || batch < 1) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "fa_mel_batch", [&]() -> fa_status {
        fa_mel_plan *whole = nullptr;   // geometry of the whole batch (frame stride, utterance stride) + validation
        // Small calls (the reference's streaming callers: one chunk of a fixed length per call, StreamingEouAsrManager.swift:558) keep their
        // plan in the context: building the tables on the host, one hipMalloc / upload / hipFree for them and three more for the I/O buffers
        // were 110 of the 194 us such a call took (scripts/mel_latency_probe.py).
        const bool cached = batch <= kMelCacheMaxBatch && cfg && cfg->filterbank == nullptr;
        if (cached) FA_TRY(mel_cached_plan(ctx, cfg, offsets, batch, expected_frames, frame_stride, &whole));
        else FA_TRY(fa_mel_plan_create(ctx, cfg, offsets, batch, expected_frames, frame_stride, &whole));
        struct PlanOwner { fa_mel_plan *&p; bool own; ~PlanOwner() { if (own && p) fa_mel_plan_destroy(p); } } owner{whole, !cached};
        const int64_t ns = offsets[batch];
        if (ns > 0 && !pcm) return FA_INVALID_ARGUMENT;
        const int32_t fstride = whole->frame_stride;
        const int64_t ustride = whole->utt_stride;
        auto pinned = [](const void *p) {
            hipPointerAttribute_t at{};
            if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
            return at.type == hipMemoryTypeHost;
        };
        int64_t slice_bytes = pinned(pcm) && pinned(mel) ? (64ll << 20) : (1ll << 62);
        if (const char *se = fa::sw(fa::Sw::MEL_SLICE_MB)) { const long v = atol(se); slice_bytes = v > 0 ? v * (1ll << 20) : (1ll << 62); }   // diagnostics / tests; 0 = one slice
        // slices: consecutive utterances up to slice_bytes of samples or of output, whichever is reached first
        std::vector<int32_t> first{0};
        for (int32_t b = 0; b < batch; ++b) {
            const int32_t f = first.back();
            const int64_t in_bytes = 4 * (offsets[b + 1] - offsets[f]), out_bytes = 4 * ustride * (b + 1 - f);
            if (b + 1 < batch && (in_bytes >= slice_bytes || out_bytes >= slice_bytes)) first.push_back(b + 1);
        }
        first.push_back(batch);
        const int n_slices = static_cast<int>(first.size()) - 1;
        const size_t out_floats = static_cast<size_t>(ustride) * batch;
        hipError_t e = hipSuccess;
        if (n_slices <= 1) {   // one slice: samples, output and lengths in the context's scratch buffer (grow-only, kept between calls)
            auto al = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
            const size_t o_pcm = 0, o_out = al(sizeof(float) * static_cast<size_t>(ns)), o_len = o_out + al(sizeof(float) * out_floats),
                         o_last = o_len + al(sizeof(int32_t) * batch), total = o_last + al(sizeof(float) * batch);
            if (fa::ensure_scratch(ctx, total) != FA_SUCCESS) { (void)hipGetLastError(); return fa::set_error(ctx, FA_ALLOCATION_FAILURE, "fa_mel_batch: device allocation failed"); }
            char *base = static_cast<char *>(ctx->scratch);
            float *d_pcm = reinterpret_cast<float *>(base + o_pcm), *d_out = reinterpret_cast<float *>(base + o_out), *d_last = reinterpret_cast<float *>(base + o_last);
            int32_t *d_len = reinterpret_cast<int32_t *>(base + o_len);
            fa_status st = FA_SUCCESS;
            do {
                if (ns > 0 && (e = hipMemcpyAsync(d_pcm, pcm, sizeof(float) * ns, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) break;
                if (last_samples && (e = hipMemcpyAsync(d_last, last_samples, sizeof(float) * batch, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) break;
                st = fa_mel_execute_dev(whole, d_pcm, last_samples ? d_last : nullptr, d_out, d_len);
                if (st != FA_SUCCESS) break;
                if ((e = hipMemcpyAsync(mel, d_out, sizeof(float) * out_floats, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) break;
                if (mel_lengths && (e = hipMemcpyAsync(mel_lengths, d_len, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) break;
                e = hipStreamSynchronize(ctx->stream);
            } while (0);
            if (st != FA_SUCCESS) return st;
            return fa::hip_status(ctx, e, "fa_mel_batch");
        }
        fa::DevBuf d_pcm, d_last, d_out, d_len;
        // the samples go up slice by slice below
        FA_TRY(fa::take_once(ctx, "fa_mel_batch", {{&d_pcm, sizeof(float) * static_cast<size_t>(ns)}, {&d_out, sizeof(float) * out_floats}, {&d_len, sizeof(int32_t) * batch},
                                                   {&d_last, sizeof(float) * batch, last_samples != nullptr}}));
        if (owner.own) { fa_mel_plan_destroy(whole); whole = nullptr; }   // only its geometry was needed: every slice gets its own plan
        hipStream_t down = nullptr;
        FA_HIP_TRY(ctx, hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
        SliceSet s;
        s.down = down;
        s.done.assign(n_slices, nullptr);
        s.plans.assign(n_slices, nullptr);
        fa_status st = FA_SUCCESS;
        if (last_samples && (e = hipMemcpyAsync(d_last.p, last_samples, sizeof(float) * batch, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) st = fa::hip_status(ctx, e, "fa_mel_batch upload");
        for (int k = 0; k < n_slices && st == FA_SUCCESS; ++k) {
            const int32_t f = first[k], cnt = first[k + 1] - f;
            std::vector<int64_t> offs(cnt + 1);
            for (int32_t i = 0; i <= cnt; ++i) offs[i] = offsets[f + i] - offsets[f];
            st = fa_mel_plan_create(ctx, cfg, offs.data(), cnt, expected_frames ? expected_frames + f : nullptr, fstride, &s.plans[k]);
            if (st != FA_SUCCESS) break;
            hipError_t ue = hipSuccess;
            if (offs[cnt] > 0) ue = hipMemcpyAsync(d_pcm.as<float>() + offsets[f], pcm + offsets[f], sizeof(float) * offs[cnt], hipMemcpyHostToDevice, ctx->stream);
            if (ue == hipSuccess) st = fa_mel_execute_dev(s.plans[k], d_pcm.as<float>() + offsets[f], last_samples ? d_last.as<float>() + f : nullptr,
                                                          d_out.as<float>() + static_cast<size_t>(ustride) * f, d_len.as<int32_t>() + f);
            if (ue == hipSuccess && st == FA_SUCCESS) ue = hipEventCreateWithFlags(&s.done[k], hipEventDisableTiming);
            if (ue == hipSuccess && st == FA_SUCCESS) ue = hipEventRecord(s.done[k], ctx->stream);
            if (ue == hipSuccess && st == FA_SUCCESS) ue = hipStreamWaitEvent(down, s.done[k], 0);
            if (ue == hipSuccess && st == FA_SUCCESS)
                ue = hipMemcpyAsync(mel + static_cast<size_t>(ustride) * f, d_out.as<float>() + static_cast<size_t>(ustride) * f,
                                    sizeof(float) * static_cast<size_t>(ustride) * cnt, hipMemcpyDeviceToHost, down);
            if (ue != hipSuccess) st = fa::hip_status(ctx, ue, "fa_mel_batch slice");
        }
        if (st == FA_SUCCESS && mel_lengths && (e = hipMemcpyAsync(mel_lengths, d_len.p, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)
            st = fa::hip_status(ctx, e, "fa_mel_batch lengths");
        const hipError_t s1 = hipStreamSynchronize(ctx->stream), s2 = hipStreamSynchronize(down);   // before `s` releases the plans, the events and the stream
        if (st != FA_SUCCESS) return st;
        return fa::hip_status(ctx, s1 != hipSuccess ? s1 : s2, "fa_mel_batch");
    });
}

}  // extern "C"

// ----------------------------------------------------------------------------- per-feature normalisation
namespace {

// NeMo per_feature normalisation as done by UnifiedMelExtractor.normalizePerFeature
// (reference: Sources/FluidAudio/ASR/Parakeet/Unified/UnifiedMelExtractor.swift:91-113): for every mel bin subtract the
// mean and divide by the unbiased std (+1e-5) over the valid frames; frames >= valid become 0; valid == 0 zeroes the row.
// One wavefront per (utterance, mel) row of a [B][n_mels][frame_stride] tensor; rows of up to 2048 frames are held in
// registers between the three passes (sum, centred squares, write): one HBM read and one write per element.
constexpr int kNormRegs = 32;   // frames per lane held in registers: rows up to 2048 frames are read from HBM once

__global__ __launch_bounds__(256) void mel_norm_kernel(float *__restrict__ mel, const int32_t *__restrict__ valid_frames, int64_t rows,
                                                         int32_t n_mels, int32_t frame_stride, int32_t frames) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int b = static_cast<int>(row / n_mels);
    int valid = valid_frames[b];
    valid = valid < 0 ? 0 : (valid > frames ? frames : valid);
    float *x = mel + row * frame_stride;
    const bool in_regs = frames <= 64 * kNormRegs;
    float v[kNormRegs];
    float mean = 0.0f, inv_std = 0.0f;
    if (valid > 0) {
        float sum = 0.0f;
        if (in_regs) {
#pragma unroll
            for (int j = 0; j < kNormRegs; ++j) { const int t = lane + 64 * j; v[j] = t < valid ? x[t] : 0.0f; sum += v[j]; }
        } else {
            for (int t = lane; t < valid; t += 64) sum += x[t];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        mean = sum / static_cast<float>(valid);
        float var = 0.0f;
        if (in_regs) {
#pragma unroll
            for (int j = 0; j < kNormRegs; ++j) if (lane + 64 * j < valid) { const float dlt = v[j] - mean; var += dlt * dlt; }
        } else {
            for (int t = lane; t < valid; t += 64) { const float dlt = x[t] - mean; var += dlt * dlt; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) var += __shfl_xor(var, off);
        const float denom = static_cast<float>(valid > 1 ? valid - 1 : 1);
        inv_std = 1.0f / (sqrtf(var / denom) + 1e-5f);
    }
    if (in_regs && valid > 0) {
#pragma unroll
        for (int j = 0; j < kNormRegs; ++j) { const int t = lane + 64 * j; if (t < frames) x[t] = t < valid ? (v[j] - mean) * inv_std : 0.0f; }
    } else {
        for (int t = lane; t < frames; t += 64) x[t] = t < valid ? (x[t] - mean) * inv_std : 0.0f;
    }
}

}  // namespace

extern "C" {

fa_status fa_mel_normalize_per_feature_dev(fa_ctx *ctx, float *d_mel, int32_t batch, int32_t n_mels, int32_t frame_stride,
                                           int32_t frames, const int32_t *d_valid_frames) {
    if (!ctx || !d_mel || !d_valid_frames) return FA_INVALID_ARGUMENT;
    if (batch < 0 || n_mels < 1 || frames < 0 || frame_stride < frames) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "mel normalise: bad shape");
    if (batch == 0 || frames == 0) return FA_SUCCESS;
    fa::DeviceGuard guard(ctx->device);
    const int64_t rows = static_cast<int64_t>(batch) * n_mels;
    hipLaunchKernelGGL(mel_norm_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, ctx->stream, d_mel, d_valid_frames, rows,
                       n_mels, frame_stride, frames);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // extern "C"
