// der_launch.h — what the DER scorer's host code (der_host.hip: staging, the one synchronisation, the copy-back, the C ABI) and its
// kernel unit (der.hip) share beside the plan (der_geom.h): the kernels' operands and one launcher per kernel.  Internal; not part of
// the C ABI.
#pragma once
#include "der_geom.h"
#include "fa_common.h"

namespace fa {
namespace der {

struct DerArgs {
    const fa_der_segment *ref, *hyp;
    const DerRec *rec;
    unsigned long long *planes;
    unsigned long long *overlap;   // int64 counts, added as unsigned
    unsigned long long *acc;       // [B][4]: miss, false alarm, confusion, ref
    int32_t *mapping;              // [B][kMaxLabels]
    int64_t n_ref, n_hyp;
    int32_t B;
    double step, collar;
};

// In the order a call launches them; the grids come from the plan.  Launch errors surface through hipGetLastError().
void launch_raster(hipStream_t stream, const DerArgs &a, const Plan &plan);       // nothing to launch without items
void launch_overlap(hipStream_t stream, const DerArgs &a, const Plan &plan);      // nothing to launch without overlap entries
void launch_assign(hipStream_t stream, const DerArgs &a);
void launch_accumulate(hipStream_t stream, const DerArgs &a, const Plan &plan);

}  // namespace der
}  // namespace fa
