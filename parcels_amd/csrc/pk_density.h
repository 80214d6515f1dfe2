// ParticleSet.density on the device-resident particle columns: particles (or the sum of a particle quantity) per cell of one grid of the
// fieldset.  Parcels had this through v3 (ParticleSet.density); v4 and the reference dropped it, so the cell rule is taken from what the
// reference does have -- grid.search(z, y, x) with no guess (ParticleSet.populate_indices, particleset.py:252-262), the rule pk_search
// reproduces -- and the sums from np.bincount.  Semantics and measurements: DESIGN.md section 14.
//
// density_run works on the caller's stream and returns 0, or a negative code with *err set.  No particle column crosses PCIe: the map,
// two counters and three event times come back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pk_device.h"

namespace pk {

// The device columns of the bound particles as they are (pk_device.h: DParticles), as far as this file reads them.
struct DensityColumns {
    int64_t n = 0;
    int32_t f32 = 0;  // storage dtype of x, y, z: 1 float32, 0 float64
    const void *x = nullptr, *y = nullptr, *z = nullptr;
    const int64_t* perm = nullptr;  // device row -> host row of the cell sort, NULL: the rows are in host order
};

// Weights of the rows (pk_particles_density: weight_kind / weight_dtype): none, a device column in DEVICE row order of dtype
// PK_DENSITY_F32 / _F64 / _I32 / _I64, or n float64 values on the HOST in host row order.
struct DensityWeights {
    int32_t kind = 0;
    int32_t dtype = 0;
    const void* dev = nullptr;
    const double* host = nullptr;
};

// ncells = max(zdim, 1) (levels only) * max(ydim, 1) * max(xdim, 1) of the grid; out: ncells int64 counts (no weights) or float64 sums on
// the host.  Counts: one lane per device row, equal keys of adjacent lanes are added once per run (integer adds commute: exact).  Sums:
// (cell, host row) keys are sorted and every cell's weights are added in ascending host row order in float64 from 0.0 -- np.bincount's
// order, so its bits.
int density_run(hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const DensityWeights& w, int64_t ncells, void* out,
                int64_t* n_outside, pk_density_info_t* info, std::string* err);

}  // namespace pk
