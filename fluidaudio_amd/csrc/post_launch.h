// post_launch.h — what the host code behind the VBx posteriors (post_host.hip: the host-pointer entries; offline_host.hip: the clustering
// stage) and the kernel translation unit (post.hip) share: the Hungarian limits (post_geom.h) and one launcher per stage.  All pointers
// prefixed d_ are DEVICE pointers; everything is enqueued on ctx->stream; results stay on the device.  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"
#include "post_geom.h"

namespace fa {

constexpr long long kHungInf = 0x7fffffffffffffffLL / 4;  // Int.max / 4 (HungarianAssignment.swift:14)

// gamma-weighted means of the K speaker slots d_spk (computeCentroids :613-691); rows_finite: no row of d_emb holds NaN / Inf
fa_status centroids_dev(fa_ctx *ctx, const double *d_emb, int64_t n, int32_t d, const double *d_gamma, int32_t S, const int32_t *d_spk, int32_t K,
                        double *d_cent, bool rows_finite = false);
// d_cn = unit centroids; d_scores[i][k] = <unit e_i, unit c_k> (:789-798)
fa_status scores_dev(fa_ctx *ctx, const double *d_emb, int64_t n, int32_t d, const double *d_cent, int32_t K, double *d_cn, double *d_scores);
// d_cn = unit centroids; d_out[i] = first cosine maximum (:806-816); all 0 without centroids (:795-797)
fa_status assign_dev(fa_ctx *ctx, const double *d_emb, int64_t n, int32_t d, const double *d_cent, int32_t K, double *d_cn, int32_t *d_out);
// one Hungarian problem per chunk: d_rows = rows grouped by chunk, d_start = n_chunks + 1 offsets into it; d_slabs: n_chunks slabs of
// hung_slab_bytes(side) when hung_in_slabs(side), else unused
fa_status hungarian_dev(fa_ctx *ctx, const double *d_scores, const int32_t *d_start, const int32_t *d_rows, int32_t *d_out, int n_chunks, int32_t K,
                        unsigned char *d_slabs, int side);

// post_host.hip — chunk_indices is a HOST array (it is the caller's bookkeeping, not a device product): the grouping of rows by chunk is host
// work, the tables go up (8 n bytes) and stay alive until the kernel has run (the call synchronises the stream before it returns).
fa_status constrained_assign_dev(fa_ctx *ctx, const double *d_scores, int64_t n, int32_t K, const int32_t *chunk_indices_host, int32_t *d_out);

}  // namespace fa
