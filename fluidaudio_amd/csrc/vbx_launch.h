// vbx_launch.h — what the VBx host code (vbx_host.hip: set-up, the EM loop, the shard handle, the C ABI) and the kernel translation
// unit (vbx.hip) share: the kernels' operands and one launcher per phase of the refinement.  The launchers own the grids, the E-step's
// LDS size and the choice between the tiled and the plain kernels (w.tiled, decided ONCE per refinement by vbx_geom.h's tiled_route when
// the workspace is set up — never inside the iteration).  Internal; not part of the C ABI.  Launch errors surface through hipGetLastError().
#pragma once
#include "fa_common.h"
#include "vbx_geom.h"

namespace fa {
namespace vbx {

struct VbxWs {
    const double *X;   // [T][D] input features (rho of the reference)
    const double *phi; // [D] (already clamped to >= 1e-12)
    double *rho;       // [T][D] = X * sqrt(phi)
    double *G;         // [T]
    double *gamma;     // [T][S]
    double *pi;        // [S]
    double *logpi;     // [S]
    const double *rec_in;  // [kSplit][stride] complete slice records: [S][D+1] (column D carries sum_t gamma), then the slice's sum of llrow
    double *rec_out;       // [z_n][stride] records of the slices z_lo .. z_lo + z_n - 1 that this device owns
    double *alpha;     // [S][D]
    double *invL;      // [S][D]
    double *phiT;      // [S]
    double *llrow;     // [T]
    double *scal;      // [8]: 0 elbo, 1 ll
    int64_t T;         // frames held here: the global frames t0g .. t0g + T - 1
    int64_t Tg, t0g;   // frames of the whole problem; global index of local frame 0
    int64_t stride;    // doubles per slice record (record_stride)
    int32_t D, S;
    int32_t z_lo, z_n; // slices owned
    double Fa, Fb;
    int32_t tiled;     // tiled_route(S, switch), taken when the workspace is set up (several host threads run refinements at once)
};

// rho, G and the smoothed start of gamma from the labels (frames held here), pi = 1 / S
void launch_prepare(hipStream_t stream, const VbxWs &w, const int32_t *d_labels);
// the records of the owned slices from the present posteriors (and the present per-frame log-likelihoods); nothing when no slice is owned
void launch_records(hipStream_t stream, const VbxWs &w);
// speaker statistics from the complete records, then the E-step of the frames held here (:330-572)
void launch_estep(hipStream_t stream, const VbxWs &w);
// pi of the new posteriors (column D of the complete records, :586-621) and the ELBO (:623-647) into w.scal
void launch_finish(hipStream_t stream, const VbxWs &w);
// first maximum of every posterior row (:144-146)
void launch_hard(hipStream_t stream, const VbxWs &w, int32_t *d_hard);
// VBxClustering.refine's catch block (:136-141): gamma = one-hot of the clamped labels, hard = the clamped labels, pi = 1 / S
void launch_degrade(hipStream_t stream, const int32_t *d_labels, double *d_gamma, double *d_pi, int32_t *d_hard, int64_t T, int32_t S);

}  // namespace vbx
}  // namespace fa
