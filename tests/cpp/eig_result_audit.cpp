// The host's verdict on the result block of the small dense step (genomic_pca_amd/csrc/eig_result.h): hand-made blocks with every
// combination of the CholeskyQR pivot flag and the eigen step's cap flag, on top of every payload the kernels can leave around them
// (zeros, finite values, NaN, Inf).  Includes the header the engine itself uses in finish_small_eigh; the status codes are checked
// against include/gpca.h.
#include "eig_result.h"
#include "gpca.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace gpca;

static long long g_checks = 0, g_fail = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { if (++g_fail <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } \
    } while (0)

int main() {
    static_assert(kEigNotConverged == GPCA_ERR_NOT_CONVERGED, "the header restates include/gpca.h");
    static_assert(kEigResFlag + 2 <= kEigResCount && kEigResW + kMaxSketchCols <= kEigResFlag, "the flags sit behind the three arrays");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double payloads[] = {0.0, 1.0, -3.5, 1e300, nan, inf};
    const int pivots[] = {0, 1, 2, 32, 33, 64, 65, 127, 128};            // the flag holds j + 1 for pivot j of a sketch of up to 128 columns
    const double caps[] = {0.0, 1.0, 2.0};                              // the kernels write (double)capped: 0 or 1; anything non-zero counts
    const int widths[] = {1, 20, 32, 64, 100, 128};
    for (double fill : payloads)
        for (int piv : pivots)
            for (double cap : caps)
                for (int l : widths) {
                    std::vector<double> res((size_t)kEigResCount, fill);
                    res[kEigResFlag] = (double)piv; res[kEigResFlag + 1] = cap;
                    const EigVerdict v = eig_result_verdict(res.data(), l);
                    char want[160];
                    if (piv) {
                        snprintf(want, sizeof want, "CholeskyQR: pivot %d of the %d-column sketch is not finite (overflow or NaN in the sketch)", piv - 1, l);
                        EXPECT(v.status == GPCA_ERR_NOT_CONVERGED && strcmp(v.msg, want) == 0, "pivot %d cap %g l %d: status %d \"%s\"", piv, cap, l, v.status, v.msg);
                    } else if (cap != 0.0) {
                        EXPECT(v.status == GPCA_ERR_NOT_CONVERGED && strcmp(v.msg, "the eigen step hit its sweep cap") == 0,
                               "pivot 0 cap %g l %d: status %d \"%s\"", cap, l, v.status, v.msg);
                    } else {
                        EXPECT(v.status == GPCA_OK && v.msg[0] == 0, "clean block l %d fill %g: status %d \"%s\"", l, fill, v.status, v.msg);
                    }
                    EXPECT(strlen(v.msg) < sizeof v.msg, "message not terminated");
                }
    printf("eig_result_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
