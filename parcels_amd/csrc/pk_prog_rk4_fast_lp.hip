// AdvectionRK4 on a rectilinear A-grid with float64 coordinates in the level-pair modes of the dedicated kernel (pk_fast_agrid.h:
// FAST_LP_REGS, FAST_LP_CACHE), field dtype x particle dtype.  The library's lean build only: modules that carry user kernels keep the
// arithmetic order of the general program and never ask for these.
#ifndef PK_MIN_WAVES
#define PK_MIN_WAVES 4
#endif
#include "pk_kernels.h"
#include <algorithm>
namespace pk {
static_assert(PK_FAST_LEAN != 0, "the level-pair modes belong to the lean build");
hipError_t launch_fast_lp(int lp, int field_f32, int particles_f32, const KArgs& a, size_t lds_bytes, int compute_units, int grid_cap, hipStream_t stream) {
    if (lp == FAST_LP_CACHE) {
        PK_LAUNCH_FAST_LP_KEYS(FAST_LP_CACHE)
    } else {
        PK_LAUNCH_FAST_LP_KEYS(FAST_LP_REGS)
    }
    return hipGetLastError();
}
}  // namespace pk
