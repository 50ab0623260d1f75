// The result block of the small dense step (small_eig.hip) and the host's verdict on it.  Plain C++ (no HIP type), like plan_math.h:
// kernels.h includes it for the engine, tests/cpp/eig_result_audit.cpp includes it under a host compiler and walks every combination
// of the block's two flags.
#pragma once
#include <stdio.h>
#include "plan_math.h"

namespace gpca {

// layout of the result block `res` of launch_small_eigh (doubles): what the host reads back ONCE, at the end of the call
constexpr int kEigResSv = 0;                         // [128] singular values sqrt(max(w, 0)), descending
constexpr int kEigResEig = kMaxSketchCols;           // [128] w_c / denom for c < k
constexpr int kEigResW = 2 * kMaxSketchCols;         // [128] eigenvalues w, descending
constexpr int kEigResFlag = 3 * kMaxSketchCols;      // [0] the CholeskyQR pivot flag, [1] the eigen step's sweep / iteration cap was hit
constexpr int kEigResCount = 3 * kMaxSketchCols + 8;

// What the host makes of the two flags of a result block at the end of a call (gpca_rsvd, gpca_rsvd_condensed, gpca_refine and the
// test hook gpca_device_tail: finish_small_eigh).  status: 0, or kEigNotConverged (= GPCA_ERR_NOT_CONVERGED, include/gpca.h) with the
// message of the failure.  The pivot flag is older than the eigen step (a sketch that is not finite leaves nothing to converge on),
// so it is reported first when both are set.
constexpr int kEigNotConverged = -6;
struct EigVerdict { int status; char msg[160]; };
inline EigVerdict eig_result_verdict(const double* res, int l) {
    EigVerdict v;
    v.status = 0; v.msg[0] = 0;
    const int flag = (int)res[kEigResFlag];
    if (flag) {   // (computed redundantly on the replicated Y: the same on every rank)
        v.status = kEigNotConverged;
        snprintf(v.msg, sizeof v.msg, "CholeskyQR: pivot %d of the %d-column sketch is not finite (overflow or NaN in the sketch)", flag - 1, l);
    } else if (res[kEigResFlag + 1] != 0.0) {
        v.status = kEigNotConverged;
        snprintf(v.msg, sizeof v.msg, "the eigen step hit its sweep cap");
    }
    return v;
}

}  // namespace gpca
