// offline_launch.h — the row kernels of the clustering stage (offline.hip) as the stage's host code (offline_host.hip) sees them: one
// launcher per kernel.  Device pointers; launch errors surface through hipGetLastError().  Internal; not part of the C ABI.
#pragma once
#include "fa_common.h"

namespace fa {
namespace offline {

// d_ok[r] = 1 when every element of row r is finite (selectTrainingEmbeddings keeps rows without NaN / Inf)
void launch_finite_rows(hipStream_t stream, const float *d_x, uint8_t *d_ok, int64_t n, int d);
// d_out[r][:] = double(d_x[d_rows ? d_rows[r] : r][:]) for n_out rows (Float -> Double, OfflineDiarizerManager.swift:286)
void launch_widen_rows(hipStream_t stream, const float *d_x, const int32_t *d_rows, double *d_out, int64_t n_out, int d);
// d_out[r][:] = d_x[d_rows[r]][:] for n_out rows
void launch_gather_rows(hipStream_t stream, const double *d_x, const int32_t *d_rows, double *d_out, int64_t n_out, int d);

}  // namespace offline
}  // namespace fa
