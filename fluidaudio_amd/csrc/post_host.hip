// post_host.hip — the host-pointer entries of the C ABI behind the VBx posteriors (kernels and launchers: post.hip): every entry is the
// same passage — room on the device, the inputs up, the device core, the result down, synchronise — over ONE staging helper, and the host
// part of the constrained assignment: the rows grouped by chunk (post_geom.h) and the tables the Hungarian kernel reads.
#include <climits>
#include <initializer_list>
#include <vector>

#include "post_launch.h"

namespace {

// a device buffer of one call, and what goes up into it (nothing when `host` is null or `up_bytes` is 0)
struct Room {
    fa::DevBuf *buf;
    size_t bytes;
    const void *host;
    size_t up_bytes;
};

// One host-pointer call: every buffer is allocated, then every input goes up, core() enqueues the device work, `down_bytes` of `result`
// come down to `out`, and the stream is synchronised.  The first HIP call that fails ends the passage and names the entry (`what`);
// a failing core keeps its own status and text.
template <class Core>
fa_status staged(fa_ctx *ctx, const char *what, std::initializer_list<Room> rooms, Core &&core, void *out, const fa::DevBuf &result, const size_t down_bytes) {
    hipError_t e = hipSuccess;
    for (const Room &r : rooms) if (e == hipSuccess) e = r.buf->alloc(r.bytes);
    for (const Room &r : rooms)
        if (e == hipSuccess && r.host && r.up_bytes) e = hipMemcpyAsync(r.buf->p, r.host, r.up_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        FA_TRY(core());
        e = hipMemcpyAsync(out, result.p, down_bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return fa::hip_status(ctx, e, what);
}

}  // namespace

fa_status fa::constrained_assign_dev(fa_ctx *ctx, const double *d_scores, int64_t n, int32_t K, const int32_t *chunk_indices, int32_t *d_out) {
    if (n <= 0) return FA_SUCCESS;
    const fa::post::ChunkGroups g = fa::post::group_by_chunk(chunk_indices, n);
    const int side = fa::post::hung_side(g.max_rows, K);
    fa::DevBuf d_start, d_rows, d_slabs;
    FA_TRY(fa::take(ctx, "constrained assign", {{&d_slabs, fa::post::hung_slab_bytes(side) * static_cast<size_t>(g.n_chunks()), fa::post::hung_in_slabs(side)},
                                                {&d_start, sizeof(int32_t) * g.starts.size(), true, g.starts.data()}, {&d_rows, sizeof(int32_t) * n, true, g.order.data()}}));
    FA_HIP_TRY(ctx, hipMemsetAsync(d_out, 0xfe, sizeof(int32_t) * n, ctx->stream));  // placeholder, every row is written
    FA_TRY(fa::hungarian_dev(ctx, d_scores, d_start.as<int32_t>(), d_rows.as<int32_t>(), d_out, g.n_chunks(), K, d_slabs.as<unsigned char>(), side));
    FA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the tables above are released on return
    return FA_SUCCESS;
}

extern "C" {

fa_status fa_vbx_weighted_centroids(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, const double *gamma, const double *pi,
                                    int32_t S, double *centroids, int32_t *map, int32_t *n_centroids) {
    if (!ctx || !n_centroids || !map || (S > 0 && !pi)) return FA_INVALID_ARGUMENT;
    *n_centroids = 0;
    if (n < 0 || d < 1 || S < 0) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "centroids: bad shape");
    return fa::no_throw(ctx, "centroids", [&]() -> fa_status {
        std::vector<int32_t> spk;
        for (int s = 0; s < S; ++s) {  // speakers kept: pi > 1e-7 (:630-640)
            map[s] = -1;
            if (pi[s] > 1e-7) { map[s] = static_cast<int32_t>(spk.size()); spk.push_back(s); }
        }
        const int K = static_cast<int>(spk.size());
        *n_centroids = K;
        if (K == 0) return FA_SUCCESS;
        if (!centroids || (n > 0 && (!emb || !gamma))) return FA_INVALID_ARGUMENT;
        fa::DeviceGuard guard(ctx->device);
        fa::DevBuf d_emb, d_gamma, d_spk, d_cent;
        return staged(ctx, "fa_vbx_weighted_centroids",
                      {{&d_emb, sizeof(double) * n * d, emb, sizeof(double) * n * d}, {&d_gamma, sizeof(double) * n * S, gamma, sizeof(double) * n * S},
                       {&d_spk, sizeof(int32_t) * K, spk.data(), sizeof(int32_t) * K}, {&d_cent, sizeof(double) * K * d, nullptr, 0}},
                      [&] { return fa::centroids_dev(ctx, d_emb.as<double>(), n, d, d_gamma.as<double>(), S, d_spk.as<int32_t>(), K, d_cent.as<double>()); },
                      centroids, d_cent, sizeof(double) * K * d);
    });
}

fa_status fa_assign_cosine(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, const double *centroids, int32_t K, int32_t *out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n == 0) return FA_SUCCESS;
    if (n < 0 || d < 1 || K < 0 || !out || !emb) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "assign: bad arguments");
    if (K == 0) { for (int64_t i = 0; i < n; ++i) out[i] = 0; return FA_SUCCESS; }  // guard (:795-797)
    if (!centroids) return FA_INVALID_ARGUMENT;
    return fa::no_throw(ctx, "assign", [&]() -> fa_status {
        fa::DeviceGuard guard(ctx->device);
        fa::DevBuf d_emb, d_c, d_cn, d_out;
        return staged(ctx, "fa_assign_cosine",
                      {{&d_emb, sizeof(double) * n * d, emb, sizeof(double) * n * d}, {&d_c, sizeof(double) * K * d, centroids, sizeof(double) * K * d},
                       {&d_cn, sizeof(double) * K * d, nullptr, 0}, {&d_out, sizeof(int32_t) * n, nullptr, 0}},
                      [&] { return fa::assign_dev(ctx, d_emb.as<double>(), n, d, d_c.as<double>(), K, d_cn.as<double>(), d_out.as<int32_t>()); },
                      out, d_out, sizeof(int32_t) * n);
    });
}

fa_status fa_centroid_scores(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, const double *centroids, int32_t K, double *scores) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n == 0 || K == 0) return FA_SUCCESS;
    if (n < 0 || d < 1 || K < 0 || !emb || !centroids || !scores) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "scores: bad arguments");
    return fa::no_throw(ctx, "scores", [&]() -> fa_status {
        fa::DeviceGuard guard(ctx->device);
        fa::DevBuf d_emb, d_c, d_cn, d_s;
        return staged(ctx, "fa_centroid_scores",
                      {{&d_emb, sizeof(double) * n * d, emb, sizeof(double) * n * d}, {&d_c, sizeof(double) * K * d, centroids, sizeof(double) * K * d},
                       {&d_cn, sizeof(double) * K * d, nullptr, 0}, {&d_s, sizeof(double) * n * K, nullptr, 0}},
                      [&] { return fa::scores_dev(ctx, d_emb.as<double>(), n, d, d_c.as<double>(), K, d_cn.as<double>(), d_s.as<double>()); },
                      scores, d_s, sizeof(double) * n * K);
    });
}

fa_status fa_constrained_assign(fa_ctx *ctx, const double *scores, int64_t n, int32_t K, const int32_t *chunk_indices, int32_t *out) {
    if (!ctx) return FA_INVALID_ARGUMENT;
    if (n == 0) return FA_SUCCESS;
    if (n < 0 || n > INT32_MAX || K < 0 || !chunk_indices || !out || (K > 0 && !scores)) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "constrained assign: bad arguments");
    return fa::no_throw(ctx, "constrained assign", [&]() -> fa_status {
        fa::DeviceGuard guard(ctx->device);
        fa::DevBuf d_s, d_out;
        return staged(ctx, "fa_constrained_assign",
                      {{&d_s, sizeof(double) * n * (K > 0 ? K : 1), scores, sizeof(double) * n * K}, {&d_out, sizeof(int32_t) * n, nullptr, 0}},
                      [&] { return fa::constrained_assign_dev(ctx, d_s.as<double>(), n, K, chunk_indices, d_out.as<int32_t>()); },
                      out, d_out, sizeof(int32_t) * n);
    });
}

}  // extern "C"
