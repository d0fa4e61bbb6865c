// row_pack.h — the row pack's kernel and launcher (operands and the host loop: row_pack_launch.h).  Row w of a group is
// audio[src[w] ... src[w] + len[w]) followed by zeros up to row_samples.  Without kScale the elements are copied as 32-bit words (NaN
// payloads included); with it an element is src[e] * scale, one fp32 multiply.  A template in a header: each kernel unit that packs rows
// instantiates it through launch_pack — tdt_plan.hip (the preprocessor's rows), sortformer_stream.hip (the chunk rows), fsmn_vad.hip (the
// scaled waveforms).
#pragma once
#include <hip/hip_runtime.h>

#include "fa_common.h"
#include "row_pack_launch.h"

namespace fa {
namespace rows {

// One workgroup per slice of kPackSlice elements of a row: grid (slices, rows of the group).
template <bool kWide, bool kScale>
__global__ __launch_bounds__(256) void pack(const uint32_t *__restrict__ audio, const Group g, const int64_t row_samples, const float scale, uint32_t *__restrict__ rows,
                                            int32_t *__restrict__ lengths) {
    const int w = blockIdx.y;
    const int64_t s0 = static_cast<int64_t>(blockIdx.x) * kPackSlice, s1 = row_samples < s0 + kPackSlice ? row_samples : s0 + kPackSlice;
    const int64_t length = g.len[w];
    const uint32_t *__restrict__ src = audio + g.src[w];
    uint32_t *__restrict__ out = rows + static_cast<int64_t>(w) * row_samples;
    if (blockIdx.x == 0 && threadIdx.x == 0 && lengths) lengths[w] = g.len[w];
    const auto element = [&](const int64_t s) -> uint32_t {
        if (!(s < length)) return 0u;
        return kScale ? __float_as_uint(__uint_as_float(src[s]) * scale) : src[s];
    };
    if (kWide) {
        for (int64_t s = s0 + 4 * threadIdx.x; s < s1; s += 4 * 256)                             // row_samples and kPackSlice are multiples of 4
            *reinterpret_cast<uint4 *>(out + s) = make_uint4(element(s), element(s + 1), element(s + 2), element(s + 3));
    } else {
        for (int64_t s = s0 + threadIdx.x; s < s1; s += 256) out[s] = element(s);
    }
}
static_assert(kPackSlice % 4 == 0, "a slice is whole groups of four");

// rows / lengths (nullable): the group's first row.  wide: 16-byte stores (rows is 16-byte aligned and row_samples a multiple of 4)
template <bool kScale>
inline void launch_pack(hipStream_t stream, const float *audio, const Group &g, const int64_t row_samples, float *rows, int32_t *lengths, const bool wide,
                        const float scale = 1.0f) {
    if (g.count == 0 || row_samples == 0) return;
    const dim3 grid(grid_for(row_samples, kPackSlice), static_cast<unsigned>(g.count));
    if (wide) pack<true, kScale><<<grid, 256, 0, stream>>>(reinterpret_cast<const uint32_t *>(audio), g, row_samples, scale, reinterpret_cast<uint32_t *>(rows), lengths);
    else pack<false, kScale><<<grid, 256, 0, stream>>>(reinterpret_cast<const uint32_t *>(audio), g, row_samples, scale, reinterpret_cast<uint32_t *>(rows), lengths);
}

}  // namespace rows
}  // namespace fa
