// resample_host.hip — host side of the sample-rate converter (polyphase kernels and their launchers: resample.hip; shared: resample_launch.h,
// resample_geom.h): the Kaiser taps, the plan a context keeps for its last rate pair, the route a call takes through the kernels (chosen by
// pick_route of resample_route.h, plain C++ that the CPU tests walk), and the C ABI.
//
// (1) fa_resample_linear replaces AudioConverter.linearResample
//     (reference: Sources/FluidAudio/Shared/AudioConverter.swift:388-442): mix N planar channels down to mono with
//     weight 1/N (:399-408), then linear interpolation at sourceIndex = i * (inRate / outRate) in double precision
//     (:419-434).  This is the only resampling arithmetic that exists in the reference tree; it is pinned by
//     AudioConverterTests.swift:546-761 and reproduced bit-for-bit (fp32 mix and blend with one rounding per operation).
// (2) fa_resample_poly is an EXTENSION with its own specification (PARITY UNPINNED): see resample.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "resample_launch.h"
#include "resample_route.h"

namespace {

using namespace fa::resample;
constexpr int kThreads = 256;

__global__ void mixdown_kernel(const float *__restrict__ planar, float *__restrict__ mono, int channels, int64_t frames) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (f >= frames) return;
    float sum = 0.0f;
    for (int c = 0; c < channels; ++c) sum = __fadd_rn(sum, planar[static_cast<int64_t>(c) * frames + f]);  // :403-407
    mono[f] = __fmul_rn(sum, 1.0f / static_cast<float>(channels));
}

__global__ void linear_kernel(const float *__restrict__ mono, float *__restrict__ out, int64_t frames, int64_t out_frames, double ratio) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= out_frames) return;
    const double src = static_cast<double>(i) * ratio;       // :424
    const int64_t idx = static_cast<int64_t>(src);            // Int(sourceIndex): truncation
    const float frac = static_cast<float>(src - static_cast<double>(idx));
    float v = 0.0f;
    if (idx < frames - 1) v = __fadd_rn(__fmul_rn(mono[idx], __fsub_rn(1.0f, frac)), __fmul_rn(mono[idx + 1], frac));  // :428-430
    else if (idx < frames) v = mono[idx];                     // :431-432
    out[i] = v;
}

double bessel_i0(double x) {  // power series, converges fast for the beta used here
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; ++k) { term *= q / (static_cast<double>(k) * k); sum += term; if (term < 1e-18 * sum) break; }
    return sum;
}

int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// ------------------------------------------------------------------------------ the plan of a rate pair
// What a context keeps for its last (up, down): everything a call needs that does not depend on the call.  Built by the first call of a pair
// (plan_get), with the taps; a repeated call with the same pair finds it and enqueues its kernels without host work, allocation or synchronisation.
struct ResamplePlan : PlanFacts {               // (resample_route.h: the pair, its filter, the families with an instance for it — what the route reads)
    float *d_taps = nullptr;
    RowsTables rows;                            // rows.d_tables set (has_rows): the row kernels serve the pair (rows.wide: a wide one)
    ~ResamplePlan() { (void)hipFree(d_taps); (void)hipFree(rows.d_tables); }
};
void plan_free(void *p) { delete static_cast<ResamplePlan *>(p); }

// Geometry + tables of the row kernels (resample_geom.h) and the kernel form that takes them; false when the pair does not suit them.
bool rows_build(RowsTables &R, const std::vector<float> &h, int up, int down, int64_t pre_remove, std::vector<int> &gtab, std::vector<float> &tt) {
    // the persistent kernels with two buffers (FA_RESAMPLE_NO_WIDE=1: the one-tile-per-workgroup kernel): tables built for one of the forms below that
    // resample.hip has an instance for (wide_instance: row length, phase groups, window, sharing, units per wavefront)
    if (!fa::sw_on(fa::Sw::RESAMPLE_NO_WIDE)) {
        // candidates, in order: {rows, wavefronts, LDS budget of rows_geometry (per 64 rows: it decides the phase groups; unbounded: one group)}.
        // FA_RESAMPLE_WIDE = "rows:waves" picks one.  Measured per audio hour (profiles/r05_resample_wide_steps.json): 16-row tiles, 8 wavefronts, two workgroups
        // per CU — 44.1 kHz 233 - 250 us, 22.05 kHz 128, 11.025 kHz 116; 32-row tiles with one workgroup per CU 243 - 262 / 152 / (no instance); 32-row tiles of one
        // phase GROUP (80 k phases: rows of <= 288 floats, two workgroups of ten wavefronts, no LDS bank conflicts, every wavefront the same number of units)
        // 245 - 257 / 152 / 159.  The 16-row form wins or ties in spite of its 2-way LDS bank conflicts (two phase quads with different window offsets share a
        // ds_read_b128 lane group).  (Round 6: windows of 32 reads — 88.2 kHz, 80 phases — first try 32-row tiles with ten wavefronts: 10 units of 8 phases, one per
        // wavefront; with 16-row tiles the 5 units of 16 phases leave three of eight wavefronts without work, and those still issue their share of the LDS reads)
        struct Cand { int rows, waves; size_t budget; };
        const size_t one_group = size_t{1} << 30, group_budget = size_t{64} * 288 * 4;      // (rows_geometry budgets 64 rows)
        std::vector<Cand> cands = {{32, 10, one_group}, {16, 8, one_group}, {32, 10, group_budget}, {32, 8, one_group}};
        if (const char *e = fa::sw(fa::Sw::RESAMPLE_WIDE)) {
            int r_ = 0, w_ = 0;
            // only the forms that exist: any other pair would reach the geometry arithmetic below (rows 0: a division by zero)
            if (sscanf(e, "%d:%d", &r_, &w_) == 2 && (r_ == 16 || r_ == 32) && (w_ == 8 || w_ == 10))
                cands = r_ == 32 && w_ == 10 ? std::vector<Cand>{{32, 10, one_group}, {32, 10, group_budget}} : std::vector<Cand>{{r_, w_, one_group}};
        }
        for (const Cand &c : cands) {
            RowsTables W;
            std::vector<int> gtab2;
            std::vector<float> tt2;
            if (!fa::rows_geometry(W.g, W.nv, h, up, down, pre_remove, gtab2, tt2, c.budget)) continue;
            if (c.rows == 32 && c.waves == 10 && c.budget > group_budget && W.nv != 32) continue;   // the ungrouped ten-wavefront form is for the long windows only
            const int pu = 4 * 64 / c.rows, units = (W.g.ppg + pu - 1) / pu;
            if (c.waves == 10 && units % 10 != 0) continue;              // (ten wavefronts only where they divide the units)
            W.wide = true; W.wide_rows = c.rows; W.wide_waves = c.waves; W.ch = (units + c.waves - 1) / c.waves;
            if (!wide_instance(c.rows, c.waves, W.nv, W.g.share, W.ch, W.g.sld, W.g.groups)) continue;
            R = W; gtab.swap(gtab2); tt.swap(tt2);
            return true;
        }
    }
    if (!fa::rows_geometry(R.g, R.nv, h, up, down, pre_remove, gtab, tt)) return false;   // the automatic LDS budget (resample_geom.h)
    if (R.g.sld > 64 * 5 && R.g.share != 1 && !fa::rows_geometry(R.g, R.nv, h, up, down, pre_remove, gtab, tt, 0, 1)) return false;   // the long-row build is instantiated for share = 1 only
    return rows_instance(R.nv);
}

// The context's plan for (up, down), both reduced; built, with the taps and the tables on the device, when the pair differs from the last call's.
fa_status plan_get(fa_ctx *ctx, const int up, const int down, const ResamplePlan *&out) {
    ResamplePlan *const have = static_cast<ResamplePlan *>(ctx->resample_plan);
    if (have && have->up == up && have->down == down) { out = have; return FA_SUCCESS; }
    std::unique_ptr<ResamplePlan> P(new ResamplePlan());
    P->up = up; P->down = down;
    FA_TRY(fa_resample_poly_taps(up, down, nullptr, 0, &P->n_taps, &P->pre_remove));
    std::vector<float> taps(P->n_taps);
    FA_TRY(fa_resample_poly_taps(up, down, taps.data(), P->n_taps, &P->n_taps, &P->pre_remove));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call may still read the previous pair's taps and tables
    if (have) { plan_free(have); ctx->resample_plan = nullptr; }
    FA_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&P->d_taps), sizeof(float) * P->n_taps));
    FA_HIP_TRY(ctx, hipMemcpyAsync(P->d_taps, taps.data(), sizeof(float) * P->n_taps, hipMemcpyHostToDevice, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // taps is a host temporary (first call of a rate pair only)
    // per-phase tables for the row kernels (non-integer ratios); a pair that does not suit them, or a failed upload, leaves the pair to the LDS-staged kernel
    std::vector<int> gtab;
    std::vector<float> tt;
    RowsTables &R = P->rows;
    if (rows_build(R, taps, up, down, P->pre_remove, gtab, tt)) {
        const size_t b0 = (sizeof(int) * gtab.size() + 255) & ~static_cast<size_t>(255), b1 = sizeof(float) * tt.size();
        R.tt_offset = b0;
        if (hipMalloc(&R.d_tables, b0 + b1) != hipSuccess ||
            hipMemcpyAsync(R.d_tables, gtab.data(), sizeof(int) * gtab.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(static_cast<char *>(R.d_tables) + b0, tt.data(), b1, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(R.d_tables);
            R.d_tables = nullptr;
        }
    }
    P->has_rows = R.d_tables != nullptr; P->rows_geom = R.g; P->tile_rows = R.tile_rows();
    const bool decim_pair = up == 1 && P->n_taps == 21 * down + 1 && P->pre_remove == 11;   // the geometry the decimation kernels are written for
    P->decim_tiles = decim_pair && decim_tiles_instance(down);
    P->decim_regs = decim_pair && decim_instance(down);
    P->interp = interp_instance(up, down, P->n_taps);
    P->lds_bytes = lds_need(up, down, P->n_taps);
    out = P.get();
    ctx->resample_plan = P.release();
    ctx->resample_plan_free = plan_free;
    return FA_SUCCESS;
}

// ------------------------------------------------------------------------------ the route of a call
// The context's plan for the pair and the family that serves this call (pick_route of resample_route.h), with the switches as they stand now.
fa_status route_get(fa_ctx *ctx, const float *d_x, const int64_t frames, const int32_t up, const int32_t down, const float *d_y, const int64_t n_out, const ResamplePlan *&P, Route &r) {
    const int64_t g = gcd64(up, down);
    FA_TRY(plan_get(ctx, static_cast<int>(up / g), static_cast<int>(down / g), P));
    const Switches sw = {fa::sw_on(fa::Sw::RESAMPLE_SIMPLE), fa::sw_on(fa::Sw::RESAMPLE_NO_DECIM), fa::sw_on(fa::Sw::RESAMPLE_NO_DECIM_TILES), fa::sw_on(fa::Sw::RESAMPLE_NO_ROWS)};
    r = pick_route(*P, sw, reinterpret_cast<uintptr_t>(d_x), reinterpret_cast<uintptr_t>(d_y), frames, n_out);
    return FA_SUCCESS;
}

}  // namespace

extern "C" {

int64_t fa_resample_linear_frames(int64_t frames, double in_rate, double out_rate) {
    if (frames < 0 || !(in_rate > 0) || !(out_rate > 0)) return 0;
    if (in_rate == out_rate) return frames;  // :414-416
    return static_cast<int64_t>(static_cast<double>(frames) / (in_rate / out_rate));  // :420
}

fa_status fa_resample_linear(fa_ctx *ctx, const float *planar, int32_t channels, int64_t frames, double in_rate, double out_rate,
                             float *out, int64_t out_capacity, int64_t *out_frames) {
    if (!ctx || !out_frames) return FA_INVALID_ARGUMENT;
    *out_frames = 0;
    if (channels < 1 || frames < 0 || !(in_rate > 0) || !(out_rate > 0)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "resample: bad arguments");
    const int64_t n_out = fa_resample_linear_frames(frames, in_rate, out_rate);
    if (n_out > out_capacity) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "resample: output buffer too small");
    *out_frames = n_out;
    if (frames == 0 || n_out == 0) return FA_SUCCESS;
    if (!planar || !out) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    fa::DevBuf d_in, d_mono, d_out;
    FA_TRY(fa::take_once(ctx, "fa_resample_linear", {{&d_in, sizeof(float) * frames * channels, true, planar}, {&d_mono, sizeof(float) * frames}, {&d_out, sizeof(float) * n_out}}));
    hipError_t e;
    do {
        hipLaunchKernelGGL(mixdown_kernel, dim3(static_cast<unsigned>((frames + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, d_in.as<float>(), d_mono.as<float>(), channels, frames);
        const float *src = d_mono.as<float>();
        if (in_rate != out_rate) {
            hipLaunchKernelGGL(linear_kernel, dim3(static_cast<unsigned>((n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, d_mono.as<float>(), d_out.as<float>(), frames, n_out, in_rate / out_rate);
            src = d_out.as<float>();
        }
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipMemcpyAsync(out, src, sizeof(float) * n_out, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) break;
        e = hipStreamSynchronize(ctx->stream);
    } while (0);
    return fa::hip_status(ctx, e, "fa_resample_linear");
}

int64_t fa_resample_poly_frames(int64_t frames, int32_t up, int32_t down) {
    if (frames < 0 || up < 1 || down < 1) return 0;
    const int64_t g = gcd64(up, down);
    const int64_t u = up / g, dn = down / g;
    return (frames * u + dn - 1) / dn;  // ceil(n * up / down)
}

fa_status fa_resample_poly_taps(int32_t up, int32_t down, float *taps, int64_t capacity, int64_t *n_taps, int64_t *pre_remove) {
    if (up < 1 || down < 1 || !n_taps || !pre_remove) return FA_INVALID_ARGUMENT;
    const int64_t g = gcd64(up, down);
    const int64_t u = up / g, dn = down / g, mx = u > dn ? u : dn;
    const int64_t half = 10 * mx, len = 2 * half + 1;
    const int64_t pre_pad = dn - half % dn;
    *n_taps = len + pre_pad;
    *pre_remove = (half + pre_pad) / dn;
    if (!taps) return FA_SUCCESS;
    if (capacity < *n_taps) return FA_OUTPUT_TOO_SMALL;
    try {
        // firwin(len, 1/mx, window=('kaiser', 5.0)) * up : windowed sinc, cut-off 1/mx of Nyquist, unit DC gain
        std::vector<double> h(len);
        const double fc = 1.0 / static_cast<double>(mx), alpha = 0.5 * (len - 1), beta = 5.0, i0b = bessel_i0(beta);
        double sum = 0.0;
        for (int64_t n = 0; n < len; ++n) {
            const double m = static_cast<double>(n) - alpha;
            const double a = M_PI * fc * m;
            const double sinc = m == 0.0 ? 1.0 : sin(a) / a;
            const double r = 2.0 * n / static_cast<double>(len - 1) - 1.0;
            const double w = bessel_i0(beta * sqrt(1.0 - r * r > 0 ? 1.0 - r * r : 0.0)) / i0b;
            h[n] = fc * sinc * w;
            sum += h[n];
        }
        for (int64_t n = 0; n < pre_pad; ++n) taps[n] = 0.0f;
        for (int64_t n = 0; n < len; ++n) taps[pre_pad + n] = static_cast<float>(h[n] / sum * static_cast<double>(u));
        return FA_SUCCESS;
    } catch (const std::bad_alloc &) {
        return FA_ALLOCATION_FAILURE;
    }
}

// Device-resident form: d_x (frames samples) -> d_y (fa_resample_poly_frames samples), enqueued on the context's stream.
fa_status fa_resample_poly_dev(fa_ctx *ctx, const float *d_x, int64_t frames, int32_t up, int32_t down, float *d_y, int64_t out_capacity, int64_t *out_frames) {
    if (!ctx || !out_frames) return FA_INVALID_ARGUMENT;
    *out_frames = 0;
    if (frames < 0 || up < 1 || down < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "resample_poly: bad arguments");
    const int64_t n_out = fa_resample_poly_frames(frames, up, down);
    if (n_out > out_capacity) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "resample_poly: output buffer too small");
    *out_frames = n_out;
    if (frames == 0) return FA_SUCCESS;
    if (!d_x || !d_y) return FA_INVALID_ARGUMENT;
    try {
        fa::DeviceGuard guard(ctx->device);
        const ResamplePlan *P = nullptr;
        Route r{};
        FA_TRY(route_get(ctx, d_x, frames, up, down, d_y, n_out, P, r));
        const Job job = {ctx->stream, d_x, P->d_taps, d_y, frames, n_out, P->n_taps, P->pre_remove, P->up, P->down};
        switch (r.kind) {
            case Kind::DECIM: launch_decim_tiles(P->down, job, r.lo, r.split); launch_decim(P->down, job, r.split, r.hi); break;
            case Kind::INTERP: launch_interp(job, r.lo, r.split, r.count); break;
            case Kind::ROWS: (P->rows.wide ? launch_rows_wide : launch_rows)(job, P->rows, r.count, r.hi); break;
            case Kind::LDS: launch_lds(job, P->lds_bytes); break;
            case Kind::SIMPLE: break;
        }
        launch_edges(job, 0, r.lo);
        launch_edges(job, r.hi, n_out);
        FA_HIP_TRY(ctx, hipGetLastError());
        return FA_SUCCESS;
    } catch (const std::bad_alloc &) {
        return FA_ALLOCATION_FAILURE;
    } catch (...) {
        return FA_UNKNOWN_ERROR;
    }
}

fa_status fa_debug_resample_route(fa_ctx *ctx, const float *d_x, int64_t frames, int32_t up, int32_t down, const float *d_y, fa_resample_route *out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    if (!fa_debug_hooks_enabled()) return FA_RUNTIME_ERROR;
    *out = fa_resample_route{};
    out->kind = FA_RESAMPLE_ROUTE_SIMPLE;
    if (frames < 0 || up < 1 || down < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "resample_route: bad arguments");
    if (frames == 0) return FA_SUCCESS;       // (such a call launches nothing and builds no plan)
    try {
        fa::DeviceGuard guard(ctx->device);
        const ResamplePlan *P = nullptr;
        Route r{};
        FA_TRY(route_get(ctx, d_x, frames, up, down, d_y, fa_resample_poly_frames(frames, up, down), P, r));
        static_assert(static_cast<int>(Kind::DECIM) == FA_RESAMPLE_ROUTE_DECIM && static_cast<int>(Kind::INTERP) == FA_RESAMPLE_ROUTE_INTERP &&
                      static_cast<int>(Kind::ROWS) == FA_RESAMPLE_ROUTE_ROWS && static_cast<int>(Kind::LDS) == FA_RESAMPLE_ROUTE_LDS &&
                      static_cast<int>(Kind::SIMPLE) == FA_RESAMPLE_ROUTE_SIMPLE, "the header's numbering");
        out->kind = static_cast<int32_t>(r.kind);
        out->lo = r.lo; out->hi = r.hi; out->split = r.split; out->count = r.count;
        if (r.kind == Kind::ROWS) {
            const RowsTables &R = P->rows;
            out->wide = R.wide ? 1 : 0; out->tile_rows = R.tile_rows(); out->wide_waves = R.wide_waves; out->nv = R.nv; out->share = R.g.share; out->groups = R.g.groups;
        }
        return FA_SUCCESS;
    } catch (const std::bad_alloc &) {
        return FA_ALLOCATION_FAILURE;
    } catch (...) {
        return FA_UNKNOWN_ERROR;
    }
}

fa_status fa_resample_poly(fa_ctx *ctx, const float *x, int64_t frames, int32_t up, int32_t down, float *out, int64_t out_capacity,
                           int64_t *out_frames) {
    if (!ctx || !out_frames) return FA_INVALID_ARGUMENT;
    *out_frames = 0;
    if (frames < 0 || up < 1 || down < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "resample_poly: bad arguments");
    const int64_t n_out = fa_resample_poly_frames(frames, up, down);
    if (n_out > out_capacity) return fa::set_error(ctx, FA_OUTPUT_TOO_SMALL, "resample_poly: output buffer too small");
    *out_frames = n_out;
    if (frames == 0) return FA_SUCCESS;
    if (!x || !out) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(ctx->device);
    fa::DevBuf d_x, d_y;
    FA_TRY(fa::take_once(ctx, "resample_poly", {{&d_x, sizeof(float) * frames, true, x}, {&d_y, sizeof(float) * n_out}}));
    int64_t got = 0;
    FA_TRY(fa_resample_poly_dev(ctx, d_x.as<float>(), frames, up, down, d_y.as<float>(), n_out, &got));
    FA_HIP_TRY(ctx, hipMemcpyAsync(out, d_y.p, sizeof(float) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

}  // extern "C"
