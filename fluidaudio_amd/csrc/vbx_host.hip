// vbx_host.hip — the host side of the VBx refinement (kernels and launchers: vbx.hip; index arithmetic: vbx_geom.h): the workspace of a
// run, the EM loop with the reference's convergence test, VBxClustering.refine's degrade rule — ONE function, fa::vbx_refine_dev, which
// fa_vbx_refine and the clustering stage (offline_host.hip) both call —, the shard handle of the runs sharded over frames, and the C ABI.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "vbx_launch.h"

namespace {

using fa::vbx::kSplit;
using fa::vbx::VbxWs;

// buffers + kernel arguments for the frames [t0g, t0g + T) of a problem of Tg frames; the device owns the slices z_lo .. z_lo + z_n - 1
fa_status vbx_setup(fa_ctx *ctx, const double *d_X, int64_t T, int64_t Tg, int64_t t0g, int32_t D, const int32_t *d_labels, int32_t S, const double *phi_host,
                    double Fa, double Fb, int32_t z_lo, int32_t z_n, fa::VbxDevice &o, VbxWs &w) {
    std::vector<double> phic(D);
    for (int d = 0; d < D; ++d) phic[d] = phi_host[d] > 1e-12 ? phi_host[d] : 1e-12;  // :241
    const size_t Tn = static_cast<size_t>(T > 0 ? T : 1);
    const size_t TD = Tn * D, TS = Tn * S, SD = static_cast<size_t>(S) * D;
    const int64_t stride = fa::vbx::record_stride(S, D);
    const size_t sD = static_cast<size_t>(D), sS = static_cast<size_t>(S);
    // from the context's buffer cache: 13 buffers per refinement
    FA_TRY(fa::take(ctx, "vbx", {{&o.phi, 8 * sD, true, phic.data()}, {&o.rho, 8 * TD}, {&o.G, 8 * Tn}, {&o.gamma, 8 * TS}, {&o.pi, 8 * sS}, {&o.logpi, 8 * sS},
                                 {&o.part, 8 * static_cast<size_t>(kSplit) * stride}, {&o.alpha, 8 * SD}, {&o.invL, 8 * SD}, {&o.phiT, 8 * sS}, {&o.ll, 8 * Tn}, {&o.scal, 64},
                                 {&o.hard, 4 * Tn}}));
    o.T = T; o.D = D; o.S = S;
    hipStream_t st = ctx->stream;
    FA_HIP_TRY(ctx, hipMemsetAsync(o.ll.p, 0, 8 * Tn, st));   // the records written before the first E-step carry a zero log-likelihood
    w = VbxWs{};
    w.X = d_X; w.phi = o.phi.as<double>(); w.rho = o.rho.as<double>(); w.G = o.G.as<double>();
    w.gamma = o.gamma.as<double>(); w.pi = o.pi.as<double>(); w.logpi = o.logpi.as<double>();
    w.rec_in = o.part.as<double>(); w.rec_out = o.part.as<double>() + static_cast<int64_t>(z_lo) * stride;
    w.alpha = o.alpha.as<double>(); w.invL = o.invL.as<double>(); w.phiT = o.phiT.as<double>(); w.llrow = o.ll.as<double>();
    w.scal = o.scal.as<double>(); w.T = T; w.Tg = Tg; w.t0g = t0g; w.stride = stride; w.D = D; w.S = S; w.z_lo = z_lo; w.z_n = z_n; w.Fa = Fa; w.Fb = Fb;
    w.tiled = fa::vbx::tiled_route(S, !fa::sw_on(fa::Sw::VBX_NO_TILED)) ? 1 : 0;   // once per refinement: not inside the iteration (several host threads run refinements at once)
    if (!fa::vbx::dim_fits(D)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "vbx: feature dimension too large");
    fa::vbx::launch_prepare(st, w, d_labels);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipStreamSynchronize(st));   // phic (a host temporary) has been consumed
    return FA_SUCCESS;
}

// the phases of an iteration: the launcher, then what the launches left behind
fa_status vbx_records(fa_ctx *ctx, const VbxWs &w) {
    fa::vbx::launch_records(ctx->stream, w);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}
fa_status vbx_estep_phase(fa_ctx *ctx, const VbxWs &w) {
    fa::vbx::launch_estep(ctx->stream, w);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}
// ... and the ELBO crosses to the host (8 bytes) for the convergence test
fa_status vbx_finish_phase(fa_ctx *ctx, const VbxWs &w, double *elbo) {
    fa::vbx::launch_finish(ctx->stream, w);
    FA_HIP_TRY(ctx, hipGetLastError());
    FA_HIP_TRY(ctx, hipMemcpyAsync(elbo, w.scal, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}
fa_status vbx_hard_phase(fa_ctx *ctx, const VbxWs &w, int32_t *d_hard) {
    fa::vbx::launch_hard(ctx->stream, w, d_hard);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

// The EM loop on device-resident inputs (d_X: [T][D] rho features, d_labels: [T] AHC labels with S distinct values); gamma, pi and
// the hard assignment stay on the device in `o`.  The ELBO of every iteration crosses to the host (8 bytes) for the
// convergence test of the reference (:653-659).
fa_status vbx_run_dev(fa_ctx *ctx, const double *d_X, int64_t T, int32_t D, const int32_t *d_labels, int32_t S, const double *phi_host,
                  double Fa, double Fb, int32_t max_iter, double epsilon, double *elbos, int32_t *n_iters, fa::VbxDevice &o) {
    *n_iters = 0;
    VbxWs w;
    FA_TRY(vbx_setup(ctx, d_X, T, T, 0, D, d_labels, S, phi_host, Fa, Fb, 0, kSplit, o, w));
    if (fa::fault_hit(FA_FAULT_VBX)) return fa::set_error(ctx, FA_RUNTIME_ERROR, "vbx: injected failure");
    FA_TRY(vbx_records(ctx, w));
    double prev = -1.7976931348623157e308;
    int iters = 0;
    for (int it = 0; it < max_iter; ++it) {
        iters = it + 1;
        FA_TRY(vbx_estep_phase(ctx, w));
        FA_TRY(vbx_records(ctx, w));      // of the NEW posteriors: pi and the log-likelihood of this iteration, the statistics of the next
        double elbo = 0.0;
        FA_TRY(vbx_finish_phase(ctx, w, &elbo));
        if (elbos) elbos[it] = elbo;
        if (it > 0 && std::fabs(elbo - prev) < epsilon) { prev = elbo; break; }  // :653-659
        prev = elbo;
    }
    FA_TRY(vbx_hard_phase(ctx, w, o.hard.as<int32_t>()));
    *n_iters = iters;
    return FA_SUCCESS;
}

// VBxClustering.refine's catch block (VBxClustering.swift:136-141): when runVBx throws, the refinement does not fail — it returns
// gamma = initialGamma (the plain one-hot of the clamped initial labels, :100-104, NOT the smoothed start of runVBx), pi = 1/S, no ELBOs,
// and hardClusters = the clamped labels.  Buffers of `o` that a failed run left allocated are reused; the three outputs are
// (re)allocated if the failure was the allocation itself.
fa_status vbx_degrade(fa_ctx *ctx, int64_t T, int32_t S, const int32_t *d_labels, fa::VbxDevice &o) {
    (void)hipGetLastError();
    if (T < 0 || S < 1) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "vbx degrade: bad shape");
    const size_t Tn = static_cast<size_t>(T > 0 ? T : 1);
    // a buffer the failed run left large enough is kept; any other is released and wanted again
    const auto need = [](fa::DevBuf &b, size_t bytes) { if (b.p && b.cap >= bytes) return false; b.reset(); return true; };
    const size_t gamma_bytes = 8 * Tn * S, pi_bytes = 8 * static_cast<size_t>(S), hard_bytes = 4 * Tn;
    FA_TRY(fa::take(ctx, "vbx degrade", {{&o.gamma, gamma_bytes, need(o.gamma, gamma_bytes)}, {&o.pi, pi_bytes, need(o.pi, pi_bytes)}, {&o.hard, hard_bytes, need(o.hard, hard_bytes)}}));
    o.T = T; o.S = S;
    fa::vbx::launch_degrade(ctx->stream, d_labels, o.gamma.as<double>(), o.pi.as<double>(), o.hard.as<int32_t>(), T, S);
    FA_HIP_TRY(ctx, hipGetLastError());
    return FA_SUCCESS;
}

}  // namespace

// VBx with the degrade rule.  The catch block covers what runVBx THROWS — an argument its BLAS calls refuse: the refinement degrades to
// its start, it does not fail.  That is the RUNTIME_ERROR class here (a failing launch, the injected fault).  An allocation failure (a
// retry may succeed; Swift would not have caught it either) and a refused argument are the caller's to see.  A degraded run returns
// SUCCESS with no iterations, *degraded set, and "<degraded_text> (<what failed>)" as the context's text: a SUCCESS return does not leave a
// failure text behind.
fa_status fa::vbx_refine_dev(fa_ctx *ctx, const double *d_X, int64_t T, int32_t D, const int32_t *d_labels, int32_t S, const double *phi_host,
                             double Fa, double Fb, int32_t max_iter, double epsilon, double *elbos, int32_t *n_iters, fa::VbxDevice &o,
                             const char *degraded_text, bool *degraded) {
    *degraded = false;
    const fa_status run = vbx_run_dev(ctx, d_X, T, D, d_labels, S, phi_host, Fa, Fb, max_iter, epsilon, elbos, n_iters, o);
    if (run == FA_SUCCESS || run == FA_ALLOCATION_FAILURE || run == FA_INVALID_ARGUMENT) return run;
    const std::string why = ctx->last_error;
    *n_iters = 0;          // elboHistory = []
    *degraded = true;
    FA_TRY(vbx_degrade(ctx, T, S, d_labels, o));
    fa::set_error(ctx, FA_SUCCESS, "%s (%s)", degraded_text, why.c_str());
    return FA_SUCCESS;
}

// ---- sharded over the frame axis -------------------------------------------------------------------------------
// One fa_vbx_shard per device holds a contiguous range of the 64 slices (world sizes that divide 64).  The caller moves the records:
//   begin(chunk) -> all-gather chunks -> repeat { iterate(full, chunk) -> all-gather -> finish_iteration(full, &elbo) } -> result.
// Every device evaluates the speaker statistics, pi and the ELBO from the same complete records, so all of them take the same
// convergence decision without a broadcast; the only collective is the all-gather of 64 (S (D + 1) + 1) doubles per iteration.
struct fa_vbx_shard {
    fa_ctx *ctx = nullptr;
    fa::VbxDevice dev;
    fa::DevBuf X, labels;
    VbxWs w{};
    int32_t rank = 0, world = 1;
    int64_t t_lo = 0, t_hi = 0;
};

namespace {

// the frames of this rank go up, then the workspace of its slices
fa_status shard_fill(fa_vbx_shard *h, const double *rho_local, int64_t T_total, int32_t D, const int32_t *labels_local, int32_t S, const double *phi,
                     double Fa, double Fb) {
    fa_ctx *ctx = h->ctx;
    const int64_t T = h->t_hi - h->t_lo;
    if (T > 0 && (!rho_local || !labels_local)) return FA_INVALID_ARGUMENT;
    const size_t Tn = static_cast<size_t>(T > 0 ? T : 1);
    // a rank without frames keeps one placeholder frame and uploads nothing
    FA_TRY(fa::take_once(ctx, "vbx shard", {{&h->X, 8 * Tn * D, true, T > 0 ? rho_local : nullptr}, {&h->labels, 4 * Tn, true, T > 0 ? labels_local : nullptr}}));
    const int32_t zn = kSplit / h->world;
    return vbx_setup(ctx, h->X.as<double>(), T, T_total, h->t_lo, D, h->labels.as<int32_t>(), S, phi, Fa, Fb, h->rank * zn, zn, h->dev, h->w);
}

}  // namespace

extern "C" {

int32_t fa_vbx_speaker_count(const int32_t *initial, int64_t T) {
    if (!initial || T <= 0) return 0;
    try {
        std::vector<int32_t> tmp(initial, initial + T);
        std::sort(tmp.begin(), tmp.end());
        const int64_t n = std::unique(tmp.begin(), tmp.end()) - tmp.begin();
        return static_cast<int32_t>(n < 1 ? 1 : n);  // max(1, Set(initialClusters).count) (:78)
    } catch (...) {
        return 0;
    }
}

fa_status fa_vbx_refine(fa_ctx *ctx, const double *rho, int64_t T, int32_t D, const int32_t *initial, const double *phi,
                        double Fa, double Fb, int32_t max_iter, double epsilon, double *gamma, double *pi, int32_t *hard,
                        double *elbos, int32_t *n_iters, int32_t *n_speakers) {
    if (!ctx || !n_iters || !n_speakers) return FA_INVALID_ARGUMENT;
    *n_iters = 0;
    *n_speakers = 0;
    if (T <= 0 || D <= 0) return FA_SUCCESS;  // empty VBxOutput (:45-67)
    if (!rho || !initial || !phi || !gamma || !pi || !hard || (max_iter > 0 && !elbos)) return FA_INVALID_ARGUMENT;
    const int32_t S = fa_vbx_speaker_count(initial, T);
    if (S < 1) return FA_ALLOCATION_FAILURE;
    *n_speakers = S;
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "vbx", [&]() -> fa_status {
        const size_t TD = static_cast<size_t>(T) * D, TS = static_cast<size_t>(T) * S;
        fa::DevBuf bX, blab;
        FA_TRY(fa::take_once(ctx, "vbx", {{&bX, 8 * TD, true, rho}, {&blab, 4 * static_cast<size_t>(T), true, initial}}));
        hipStream_t st = ctx->stream;
        fa::VbxDevice dev;
        bool degraded = false;
        FA_TRY(fa::vbx_refine_dev(ctx, bX.as<double>(), T, D, blab.as<int32_t>(), S, phi, Fa, Fb, max_iter, epsilon, elbos, n_iters, dev,
                                  "vbx: degraded to the initial clusters", &degraded));
        FA_HIP_TRY(ctx, hipMemcpyAsync(gamma, dev.gamma.p, 8 * TS, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(pi, dev.pi.p, 8 * S, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipMemcpyAsync(hard, dev.hard.p, 4 * T, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(ctx, hipStreamSynchronize(st));
        return FA_SUCCESS;
    });
}

int32_t fa_vbx_shard_slices(void) { return kSplit; }

void fa_vbx_shard_range(int64_t T_total, int32_t rank, int32_t world, int64_t *t_lo, int64_t *t_hi) {
    const fa::vbx::FrameRange r = fa::vbx::shard_range(T_total, rank, world);
    if (t_lo) *t_lo = r.lo;
    if (t_hi) *t_hi = r.hi;
}

int64_t fa_vbx_shard_chunk_doubles(int32_t S, int32_t D, int32_t world) { return fa::vbx::chunk_doubles(S, D, world); }

fa_status fa_vbx_shard_create(fa_ctx *ctx, const double *rho_local, int64_t T_total, int32_t D, const int32_t *labels_local, int32_t S,
                              const double *phi, double Fa, double Fb, int32_t rank, int32_t world, fa_vbx_shard **out) {
    if (!ctx || !out) return FA_INVALID_ARGUMENT;
    *out = nullptr;
    if (T_total <= 0 || D <= 0 || S < 1 || !phi || !fa::vbx::shard_ok(rank, world))
        return fa::set_error(ctx, FA_INVALID_ARGUMENT, "vbx shard: bad shape (the world size must divide 64)");
    fa::DeviceGuard guard(ctx->device);
    return fa::no_throw(ctx, "vbx shard", [&]() -> fa_status {
        std::unique_ptr<fa_vbx_shard> h(new fa_vbx_shard);
        h->ctx = ctx; h->rank = rank; h->world = world;
        fa_vbx_shard_range(T_total, rank, world, &h->t_lo, &h->t_hi);
        FA_TRY(shard_fill(h.get(), rho_local, T_total, D, labels_local, S, phi, Fa, Fb));
        *out = h.release();
        return FA_SUCCESS;
    });
}

void fa_vbx_shard_destroy(fa_vbx_shard *h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
}

void fa_vbx_shard_frames(const fa_vbx_shard *h, int64_t *t_lo, int64_t *t_hi) {
    if (t_lo) *t_lo = h ? h->t_lo : 0;
    if (t_hi) *t_hi = h ? h->t_hi : 0;
}

// d_chunk: DEVICE double[fa_vbx_shard_chunk_doubles]: the records of the slices held here, from the initial posteriors.  Complete on return.
fa_status fa_vbx_shard_begin(fa_vbx_shard *h, double *d_chunk) {
    if (!h || !d_chunk) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(h->ctx->device);
    VbxWs w = h->w;
    w.rec_out = d_chunk;
    FA_TRY(vbx_records(h->ctx, w));
    FA_HIP_TRY(h->ctx, hipStreamSynchronize(h->ctx->stream));
    return FA_SUCCESS;
}

// d_full: DEVICE double[64 x record]: the gathered records of the present posteriors; d_chunk: the records of the new ones.  Complete on return.
fa_status fa_vbx_shard_iterate(fa_vbx_shard *h, const double *d_full, double *d_chunk) {
    if (!h || !d_full || !d_chunk) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(h->ctx->device);
    VbxWs w = h->w;
    w.rec_in = d_full; w.rec_out = d_chunk;
    FA_TRY(vbx_estep_phase(h->ctx, w));
    FA_TRY(vbx_records(h->ctx, w));
    FA_HIP_TRY(h->ctx, hipStreamSynchronize(h->ctx->stream));
    return FA_SUCCESS;
}

// d_full: the gathered records of the posteriors fa_vbx_shard_iterate just wrote; *elbo: the ELBO of the iteration (:623-647)
fa_status fa_vbx_shard_finish_iteration(fa_vbx_shard *h, const double *d_full, double *elbo) {
    if (!h || !d_full || !elbo) return FA_INVALID_ARGUMENT;
    fa::DeviceGuard guard(h->ctx->device);
    VbxWs w = h->w;
    w.rec_in = d_full;
    return vbx_finish_phase(h->ctx, w, elbo);
}

// HOST outputs: gamma_local [frames held][S], pi [S], hard_local [frames held] (each may be NULL)
fa_status fa_vbx_shard_result(fa_vbx_shard *h, double *gamma_local, double *pi, int32_t *hard_local) {
    if (!h) return FA_INVALID_ARGUMENT;
    fa_ctx *ctx = h->ctx;
    fa::DeviceGuard guard(ctx->device);
    const int64_t T = h->t_hi - h->t_lo;
    FA_TRY(vbx_hard_phase(ctx, h->w, h->dev.hard.as<int32_t>()));
    if (gamma_local && T > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(gamma_local, h->dev.gamma.p, 8 * static_cast<size_t>(T) * h->w.S, hipMemcpyDeviceToHost, ctx->stream));
    if (pi) FA_HIP_TRY(ctx, hipMemcpyAsync(pi, h->dev.pi.p, 8 * static_cast<size_t>(h->w.S), hipMemcpyDeviceToHost, ctx->stream));
    if (hard_local && T > 0) FA_HIP_TRY(ctx, hipMemcpyAsync(hard_local, h->dev.hard.p, 4 * static_cast<size_t>(T), hipMemcpyDeviceToHost, ctx->stream));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FA_SUCCESS;
}

}  // extern "C"
