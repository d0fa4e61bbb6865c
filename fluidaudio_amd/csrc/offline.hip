// offline.hip — the row kernels of the clustering stage (offline_host.hip): training-row selection, widening and gathering of the
// embeddings on the device, with a launcher each (offline_launch.h).
#include "offline_launch.h"

namespace {

__global__ void widen_rows(const float *__restrict__ x, const int32_t *__restrict__ rows, double *__restrict__ out, int64_t n_out, int d) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_out * d) return;
    const int64_t r = i / d, k = i - r * d;
    const int64_t src = rows ? rows[r] : r;
    out[i] = static_cast<double>(x[src * d + k]);
}

__global__ void gather_rows_f64(const double *__restrict__ x, const int32_t *__restrict__ rows, double *__restrict__ out, int64_t n_out, int d) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_out * d) return;
    const int64_t r = i / d, k = i - r * d;
    out[i] = x[static_cast<int64_t>(rows[r]) * d + k];
}

// one flag per row: every element finite (selectTrainingEmbeddings keeps rows without NaN / Inf)
__global__ void finite_rows(const float *__restrict__ x, uint8_t *__restrict__ ok, int64_t n, int d) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & 63;
    int good = 1;
    for (int k = lane; k < d; k += 64) good &= isfinite(x[r * d + k]) ? 1 : 0;
    const unsigned long long all = __ballot(good != 0);
    if (lane == 0) ok[r] = all == ~0ull ? 1 : 0;
}

}  // namespace

namespace fa {
namespace offline {

void launch_finite_rows(hipStream_t stream, const float *d_x, uint8_t *d_ok, const int64_t n, const int d) {
    hipLaunchKernelGGL(finite_rows, dim3(fa::grid_for(n, 4)), dim3(256), 0, stream, d_x, d_ok, n, d);
}
void launch_widen_rows(hipStream_t stream, const float *d_x, const int32_t *d_rows, double *d_out, const int64_t n_out, const int d) {
    hipLaunchKernelGGL(widen_rows, dim3(fa::grid_for(n_out * d, 256)), dim3(256), 0, stream, d_x, d_rows, d_out, n_out, d);
}
void launch_gather_rows(hipStream_t stream, const double *d_x, const int32_t *d_rows, double *d_out, const int64_t n_out, const int d) {
    hipLaunchKernelGGL(gather_rows_f64, dim3(fa::grid_for(n_out * d, 256)), dim3(256), 0, stream, d_x, d_rows, d_out, n_out, d);
}

}  // namespace offline
}  // namespace fa
