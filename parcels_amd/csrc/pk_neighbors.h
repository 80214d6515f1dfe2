// Fixed-radius neighbour search over the particles themselves: the hot path of particle-particle interaction kernels
// (reference: docs/user_guide/examples/tutorial_interaction.ipynb, whose kernels build dense N x N distance matrices in NumPy).
//
// Semantics.  Points are float64 (x, y[, z]), flat Euclidean.  For an ordered pair (i, j):
//   dx = x[j] - x[i], dy = y[j] - y[i], dz = z[j] - z[i];  dist = sqrt(dx*dx + dy*dy [+ dz*dz])
// summed left to right, every operation rounded on its own, correctly rounded square root -- NumPy's np.sqrt(dx**2 + dy**2).
// j is a neighbour of i iff i != j, dist < radius (strict), sources[j] (when given) and dist > 0 (PK_NEIGHBORS_NO_COINCIDENT).
// A particle with a non-finite coordinate has no neighbours and is nobody's neighbour.  Rows are ordered by i, j ascends
// within a row; the nearest neighbour is the smallest dist, ties to the smallest j.
//
// Spherical meshes (neighbors_build_spherical): x = longitude and y = latitude in degrees, any representation of the longitude
// (values are equivalent modulo 360), z and radius in metres, R = the sphere's radius, radius < (pi / 2) R.  With rad = pi / 180
// and every operation rounded on its own:
//   dx   = d - 360*rint(d/360),  d = x[j] - x[i]          degrees, in [-180, 180]
//   dy   = y[j] - y[i]                                    degrees
//   dz   = z[j] - z[i]                                    metres
//   a    = sin(0.5*rad*dy)**2 + cos(rad*y[i])*cos(rad*y[j])*sin(0.5*rad*dx)**2
//   dh   = 2*R*arcsin(min(1, sqrt(a)))                    metres
//   dist = dh without z, sqrt(dh*dh + dz*dz) with z
// The neighbour rule, the row order and the nearest neighbour are those above.  A particle with a non-finite coordinate or with
// |y| > 90 has no neighbours and is nobody's neighbour.  dx, dy, dz are the NumPy values bit for bit; dist goes through sin, cos
// and asin, whose device versions differ from NumPy's by ulps.  Points that coincide modulo 360 give a == 0 and dist == 0 exactly;
// two points mirrored east and west of a third on one latitude give the same dist bit for bit (sin is odd).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace pk {

struct Neighbors;  // cell list + scratch of one context: grown on demand, reused across calls, freed with the context

struct NeighborsInfo {
    int64_t n = 0, nvalid = 0;  // points, points with finite coordinates
    int64_t ncx = 0, ncy = 0;   // cells of the uniform (x, y) grid
    double h = 0;               // cell size
    int32_t doublings = 0;      // times the cell size was doubled to get under the cell cap
    int64_t total = -1;         // pairs of the last count pass, -1 before it
};

struct NeighborsSphInfo {
    int64_t n = 0, nvalid = 0;    // points, valid points
    int64_t bands = 0, cells = 0;  // latitude bands, longitude cells summed over them
    double band_height = 0;       // degrees
    int32_t periodic = 0;         // the bands wrap over 360 degrees (else: the cells span the arc of the valid points)
    int32_t doublings = 0;        // times the band height was doubled to get under the band and cell caps
    int64_t total = -1;           // pairs of the last count pass, -1 before it
};

Neighbors* neighbors_create();
void neighbors_free(Neighbors* nb);     // everything, the object included
void neighbors_release(Neighbors* nb);  // the device scratch only; the next build allocates again

// Every function returns 0, or a negative code with *err set.  x, y, z (may be NULL), sources (may be NULL; one byte per
// point, non-zero = source) are HOST arrays of length n; the outputs are host arrays too.
int neighbors_build(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources,
                    double radius, int32_t flags, std::string* err);
// The cell list of a spherical mesh; counts, nearest and pairs then serve it.
int neighbors_build_spherical(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z,
                              const uint8_t* sources, double radius, double sphere_radius, int32_t flags, std::string* err);
int neighbors_counts(Neighbors* nb, hipStream_t stream, int64_t* counts, int64_t* total, std::string* err);
int neighbors_nearest(Neighbors* nb, hipStream_t stream, int64_t* j, double* dist, std::string* err);
// after neighbors_counts; total = what it announced.  starts: n + 1; j, dx, dy, dz (NULL without z), dist: total
int neighbors_pairs(Neighbors* nb, hipStream_t stream, int64_t total, int64_t* starts, int64_t* j, double* dx, double* dy, double* dz,
                    double* dist, std::string* err);
void neighbors_info(const Neighbors* nb, NeighborsInfo* out);                    // zeros after a spherical build
void neighbors_info_spherical(const Neighbors* nb, NeighborsSphInfo* out);      // zeros after a flat build

// ---- device-resident input and output (pk_interact.hip: built-in interaction kernels on the particle columns) ----------------
// The points are DEVICE columns of n rows, float32 (widened, which is exact) or float64; nothing crosses PCIe but the bounding
// box partials the build finishes on the host.  mask (may be NULL): row i takes part iff mask[i] != 0 -- a row that does not is
// given a NaN x, so it is a point with a non-finite coordinate: it has no neighbours and is nobody's neighbour, and every index
// stays a row number.  (Row numbers order the rows that take part as their positions among themselves do, so row order, ties
// and sums are those of a search over the selected rows alone.)  use_sources: the flags of neighbors_set_sources.
struct NeighborsDeviceInput {
    const void *x = nullptr, *y = nullptr, *z = nullptr;  // z: NULL for a 2-D search
    int32_t f32 = 0;                                      // 1: the columns are float32
    const int32_t* mask = nullptr;
    int32_t use_sources = 0;
};
// One byte per row (non-zero = source), copied from the HOST array into a device buffer the cell list keeps until the next call,
// neighbors_release or neighbors_free.
int neighbors_set_sources(Neighbors* nb, hipStream_t stream, int64_t n, const uint8_t* sources, std::string* err);
// sphere_radius == 0: flat, else the spherical build
int neighbors_build_device(Neighbors* nb, hipStream_t stream, int64_t n, const NeighborsDeviceInput& in, double radius, double sphere_radius,
                           int32_t flags, std::string* err);
// The nearest pass and the pair passes (fill, row sort, finish) of neighbors_nearest / neighbors_pairs without the copies to the
// host: the results stay in the scratch that neighbors_device_view describes.
int neighbors_nearest_device(Neighbors* nb, hipStream_t stream, std::string* err);
int neighbors_pairs_device(Neighbors* nb, hipStream_t stream, int64_t total, std::string* err);
struct NeighborsDeviceView {
    int64_t n = 0, total = 0;
    const int64_t* starts = nullptr;  // n + 1 CSR row starts (after neighbors_counts)
    const double *dx = nullptr, *dy = nullptr, *dz = nullptr, *dist = nullptr;  // per pair, rows ordered by j (after neighbors_pairs_device)
    const int64_t* near_j = nullptr;  // per row (after neighbors_nearest_device)
    int32_t* flag = nullptr;          // the library-error flag of the fill pass, for a pass that walks the rows
};
void neighbors_device_view(const Neighbors* nb, NeighborsDeviceView* out);

}  // namespace pk
