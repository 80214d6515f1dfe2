// Fixed-radius neighbour search on the device: uniform cell list in (x, y) + one lane per particle scanning 3 x 3 cells.
// Serves particle-particle interaction kernels (reference: docs/user_guide/examples/tutorial_interaction.ipynb, which forms
// dense N x N distance matrices in NumPy and says of itself that it "scales as N^2").  Semantics: pk_neighbors.h.
//
// Passes (all on the caller's stream, no workgroup waits on another, every loop bounded by a number computed beforehand):
//   build    bbox of the finite points (block reduction, finished on the host) -> cell size -> key = cy * ncx + cx per point
//            (non-finite points: the sentinel key `ncells`, which sorts last) -> stable rocPRIM radix sort of (key, index), so
//            indices ascend within a cell -> coordinates gathered into sorted order + first / one-past-last sorted slot per cell
//   counts   one lane per sorted slot, result at the ORIGINAL index; rocPRIM exclusive scan -> CSR row starts
//   nearest  same scan, keeps (smallest dist, then smallest j)
//   pairs    fill (checks its write index against the end of its row: a mismatch raises a flag and never writes), rocPRIM
//            segmented radix sort of j within rows, then one lane per pair recomputes dx, dy, dz, dist from the ORIGINAL arrays
//
// Spherical meshes (neighbors_build_spherical; semantics: pk_neighbors.h) keep the sort, scan, fill and row-sort passes and
// replace the cell list, the query scan and the finish pass: latitude bands of equal height over the latitude extent of the
// valid points, each cut into equal longitude cells whose width grows towards the poles (see NB_SPH_MARGIN); the per-band table
// (first cell, cell count, cell width) is built on the host and lives in device memory.  A query scans bands b - 1, b, b + 1 and
// in each the cell of its own longitude +- 1, evaluates the great-circle distance of the header for every candidate that two
// cheap bounds do not rule out, and the finish pass recomputes it from the original arrays.
//
// The distance arithmetic must not be contracted into fused multiply-adds (NumPy rounds every operation): the Makefile builds
// with -ffp-contract=off and this file repeats it.
#pragma clang fp contract(off)
#include "pk_neighbors.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

namespace pk {
namespace {

constexpr int NB_BLOCK = 256;
constexpr int NB_BBOX_BLOCKS = 1024;
constexpr int64_t NB_MAX_POINTS = 2147483646ll;   // indices and the sentinel fit uint32 / int32
constexpr int64_t NB_MAX_PAIRS = 2147483647ll;    // rocPRIM's segmented sort counts its items in 32 bits
constexpr int64_t NB_CELL_CAP_MIN = 1ll << 20;
constexpr int64_t NB_CELL_CAP_MAX = 1ll << 30;    // keys fit 31 bits; a cell coordinate stays below 2^30 (see cell size)

// ---- cell size -------------------------------------------------------------------------------------------------------------
// Claim: with h >= radius * (1 + 2^-16) and h >= 2^-500, two points a, b with computed dist < radius have cell coordinates
// that differ by at most 1 in x and in y.
//   1. The computed dist bounds the true offset.  dx = fl(xb - xa) = (xb - xa)(1 + e), |e| <= u = 2^-53.  dist =
//      fl(sqrt(fl(fl(dx*dx) + fl(dy*dy) [+ ...]))) >= |dx| (1 - u)^3 up to an absolute 2^-537 where dx*dx is subnormal (absolute
//      error 2^-1075 under the root).  So |xb - xa| <= dist (1 + 5u) + 2^-536 < radius (1 + 5u) + 2^-536 <= h (1 - 2^-17):
//      the 2^-16 margin pays for 5u, and 2^-536 <= h 2^-36.  Overflow makes dist infinite, which is no neighbour.
//   2. The computed cell coordinate is t~ = fl(fl(x - xmin) / h) = t (1 + e'), |e'| <= 2u + u^2, t = (x - xmin) / h < 2^30
//      (cell cap).  Hence t~b - t~a <= (tb - ta) + 2 * 2^30 * 3u <= 1 - 2^-17 + 2^-20 < 1, and floor(t~b) - floor(t~a) <= 1;
//      by symmetry the difference never reaches 2.  Doubling h (exact) only shrinks tb - ta.
// The host sizes the grid with the same subtraction and division (xmax - xmin) / h the device applies to every point, and
// rounding is monotonic, so no point's coordinate exceeds the last cell; the clamp in cell_of is a guard, not a correction.
constexpr double NB_CELL_MARGIN = 1.0 + 0x1p-16;
constexpr double NB_CELL_MIN = 0x1p-500;

struct NbGrid {
    double xmin, ymin, h;
    int32_t ncx, ncy;
    uint32_t ncells;  // = ncx * ncy, also the sentinel key of a non-finite point
};

__device__ __forceinline__ bool nb_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN

__device__ __forceinline__ int32_t cell_of(double v, double vmin, double h, int32_t nc) {
    const double t = (v - vmin) / h;
    int32_t c = t >= (double)nc ? nc - 1 : (int32_t)t;
    if (!(t >= 0.0)) c = 0;  // NaN of inf / inf in the one-cell grid of an overflowing extent
    return c;
}

// partial[b * 5 + {0..4}] = xmin, xmax, ymin, ymax, number of finite points of block b
__global__ void __launch_bounds__(NB_BLOCK) nb_bbox_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                           int64_t n, double* __restrict__ partial) {
    __shared__ double red[NB_BLOCK];
    double v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * NB_BLOCK) {
        const double xi = x[i], yi = y[i];
        if (nb_finite(xi) && nb_finite(yi) && (!z || nb_finite(z[i]))) {
            v[0] = xi < v[0] ? xi : v[0];
            v[1] = xi > v[1] ? xi : v[1];
            v[2] = yi < v[2] ? yi : v[2];
            v[3] = yi > v[3] ? yi : v[3];
            v[4] += 1.0;  // exact: n < 2^53
        }
    }
    for (int k = 0; k < 5; k++) {
        red[threadIdx.x] = v[k];
        __syncthreads();
        for (int s = NB_BLOCK / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                const double a = red[threadIdx.x], b = red[threadIdx.x + s];
                red[threadIdx.x] = k == 4 ? a + b : ((k & 1) ? (b > a ? b : a) : (b < a ? b : a));
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * 5 + k] = red[0];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(NB_BLOCK) nb_key_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                          int64_t n, NbGrid g, uint32_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double xi = x[i], yi = y[i];
    uint32_t k = g.ncells;
    if (nb_finite(xi) && nb_finite(yi) && (!z || nb_finite(z[i])))
        k = (uint32_t)cell_of(yi, g.ymin, g.h, g.ncy) * (uint32_t)g.ncx + (uint32_t)cell_of(xi, g.xmin, g.h, g.ncx);
    key[i] = k;
    idx[i] = (uint32_t)i;
}

// sorted slot k: coordinates of its point, and the slot range [cell_begin[c], cell_end[c]) of every occupied cell c (the two
// arrays were zeroed: an empty cell has the empty range [0, 0)); both arrays have ncells + 1 entries, the last is the sentinel's
__global__ void __launch_bounds__(NB_BLOCK) nb_gather_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                             const uint8_t* __restrict__ src, int64_t n, const uint32_t* __restrict__ key_s,
                                                             const uint32_t* __restrict__ idx_s, double* __restrict__ xs, double* __restrict__ ys,
                                                             double* __restrict__ zs, uint8_t* __restrict__ srcs, uint32_t* __restrict__ cell_begin,
                                                             uint32_t* __restrict__ cell_end) {
    const int64_t k = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = idx_s[k];
    xs[k] = x[i];
    ys[k] = y[i];
    if (z) zs[k] = z[i];
    srcs[k] = src ? (uint8_t)(src[i] != 0) : (uint8_t)1;
    const uint32_t c = key_s[k];
    if (k == 0 || key_s[k - 1] != c) cell_begin[c] = (uint32_t)k;
    if (k == n - 1 || key_s[k + 1] != c) cell_end[c] = (uint32_t)(k + 1);
}

struct NbQuery {
    int64_t n;
    NbGrid g;
    double radius;
    int32_t no_coincident;
    const uint32_t *key_s, *idx_s, *cell_begin, *cell_end;
    const double *xs, *ys, *zs;
    const uint8_t* srcs;
    // outputs, by original index
    int64_t* count;           // COUNT
    int64_t* near_j;          // NEAREST
    double* near_d;
    const int64_t* starts;    // FILL: n + 1 row starts
    uint32_t *pair_i, *pair_j;
    int32_t* flag;
};

enum { NB_COUNT = 0, NB_NEAREST = 1, NB_FILL = 2 };

template <int MODE, bool HASZ>
__global__ void __launch_bounds__(NB_BLOCK) nb_query_kernel(NbQuery q) {
    const int64_t k = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (k >= q.n) return;
    const uint32_t i = q.idx_s[k];
    const uint32_t key = q.key_s[k];
    int64_t cnt = 0;
    int64_t best_j = -1;
    double best_d = INFINITY;
    int64_t w = 0, w_end = 0;
    if (MODE == NB_FILL) {
        w = q.starts[i];
        w_end = q.starts[i + 1];
    }
    if (key != q.g.ncells) {  // a finite point
        const int32_t cy = (int32_t)(key / (uint32_t)q.g.ncx), cx = (int32_t)(key - (uint32_t)cy * (uint32_t)q.g.ncx);
        const double xi = q.xs[k], yi = q.ys[k], zi = HASZ ? q.zs[k] : 0.0;
        for (int32_t oy = -1; oy <= 1; oy++) {
            const int32_t yy = cy + oy;
            if (yy < 0 || yy >= q.g.ncy) continue;
            for (int32_t ox = -1; ox <= 1; ox++) {
                const int32_t xx = cx + ox;
                if (xx < 0 || xx >= q.g.ncx) continue;
                const uint32_t c = (uint32_t)yy * (uint32_t)q.g.ncx + (uint32_t)xx;
                const int64_t pb = q.cell_begin[c], pe = q.cell_end[c];  // pe <= n: written by nb_gather_kernel from slot numbers
                for (int64_t p = pb; p < pe; p++) {
                    if (p == k || !q.srcs[p]) continue;
                    const double dx = q.xs[p] - xi, dy = q.ys[p] - yi;
                    double s = dx * dx + dy * dy;
                    if (HASZ) {
                        const double dz = q.zs[p] - zi;
                        s = s + dz * dz;
                    }
                    const double d = sqrt(s);
                    if (!(d < q.radius)) continue;
                    if (q.no_coincident && !(d > 0.0)) continue;
                    if (MODE == NB_COUNT) cnt++;
                    if (MODE == NB_NEAREST) {
                        const int64_t j = q.idx_s[p];
                        if (d < best_d || (d == best_d && j < best_j)) {
                            best_d = d;
                            best_j = j;
                        }
                    }
                    if (MODE == NB_FILL) {
                        if (w < w_end) {
                            q.pair_i[w] = i;
                            q.pair_j[w] = q.idx_s[p];
                        } else {
                            *q.flag = 1;  // more neighbours than the count pass announced: never write past the row
                        }
                        w++;
                    }
                }
            }
        }
    }
    if (MODE == NB_COUNT) q.count[i] = cnt;
    if (MODE == NB_NEAREST) {
        q.near_j[i] = best_j;
        q.near_d[i] = best_d;
    }
    if (MODE == NB_FILL && w != w_end) *q.flag = 1;
}

// one lane per pair, rows already ordered by j: the values NumPy computes from the original arrays
template <bool HASZ>
__global__ void __launch_bounds__(NB_BLOCK) nb_finish_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                             int64_t n, int64_t total, const uint32_t* __restrict__ pair_i,
                                                             const uint32_t* __restrict__ pair_j, int64_t* __restrict__ out_j, double* __restrict__ out_dx,
                                                             double* __restrict__ out_dy, double* __restrict__ out_dz, double* __restrict__ out_dist,
                                                             int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (p >= total) return;
    const uint32_t i = pair_i[p], j = pair_j[p];
    if ((int64_t)i >= n || (int64_t)j >= n) {  // cannot happen after a clean fill; never read out of bounds
        *flag = 1;
        return;
    }
    const double dx = x[j] - x[i], dy = y[j] - y[i];
    double s = dx * dx + dy * dy;
    if (HASZ) {
        const double dz = z[j] - z[i];
        s = s + dz * dz;
        out_dz[p] = dz;
    }
    out_j[p] = (int64_t)j;
    out_dx[p] = dx;
    out_dy[p] = dy;
    out_dist[p] = sqrt(s);
}

// ---- spherical meshes: bands and longitude cells -----------------------------------------------------------------------------
// x = longitude, y = latitude in degrees, distances in metres on a sphere of radius R; delta = radius / R < pi / 2 is the angular
// radius, S = sin(delta / 2) < 0.71.  A point is valid iff its coordinates are finite and |y| <= 90.
// Claim: two valid points i, j with computed dist < radius lie in bands that differ by at most 1, and in the band of j their
// longitude cells (both taken in that band's geometry) differ by at most 1, modulo the cell count where the bands are periodic.
//   0. What the computed distance bounds.  dist >= dh (1 - 2u) and dh = 2R asin(min(1, sqrt(a))), so sqrt(a) < S (1 + 8u), with
//      asin and sin within 2 ulp and condition numbers <= 1.3 below pi / 4.  a sums two non-negative terms, so each term is below
//      S^2 (1 + 24u): (i) sin(rad |dy| / 2) < S (1 + 16u), hence |dy| < delta_deg (1 + 2^-45); (ii) cos(rad y_i) cos(rad y_j)
//      sin^2(rad |dx| / 2) < S^2 (1 + 24u) in the COMPUTED cosines.  The 2^-500 floor of the band height keeps the squares normal.
//   1. Bands.  hb >= delta_deg (1 + 2^-16), and the band coordinate fl(fl(y - ymin) / hb) is below 2^30, so the argument at
//      NB_CELL_MARGIN applies word for word with (i) in place of its step 1.
//   2. Longitude cells of band b.  The host takes the band widened by (1 + 2^-10) bands and 2^-40 degrees on each side -- it holds
//      every point that the rounded band coordinate puts into bands b - 1 .. b + 1 -- and from its smallest colatitude e (radians)
//      c_b = sin(e) <= cos(rad y) for all of them.  Bands with e < 2^-20 get one cell.  Elsewhere fl(rad y) is off by at most
//      2^-51, so a computed cosine is the true one within a factor 1 +- 2^-31, and (ii) gives sin(rad |dx| / 2) <= q (1 + 2^-28),
//      q = S / c_b.  Bands with q > 0.99 get one cell; elsewhere asin has condition <= 5 and |dx| <= wq (1 + 2^-25), wq =
//      2 asin(q) in degrees.  The computed dx differs from the true circular difference by at most u |x_j - x_i| (the other two
//      operations of the wrap are exact), and a normalised longitude (sph_lon) from the true one by a few ulp of max |x|: both
//      stay below E / 8, E = 2^-47 max(360, max |x|).  Cells are W = L / nc >= w = wq (1 + 2^-16) + E wide, so the true offset
//      is below W (1 - 2^-17) and the cell coordinate fl(fl(xn - x0) / W) < 2^30 moves it by at most 2^-20 cells, as in step 2
//      at NB_CELL_MARGIN.  A point at the far end of the span (xn = x0 + L) is clamped into the last cell, which in a periodic
//      band is next to the first.  max |x| >= 2^47 * 360 makes every w exceed 360: one cell per band, longitudes unused.
//   3. Where the valid points span L < 179 degrees in one of the two normalisations, the cells cover that span and do not wrap:
//      normalised longitudes then differ by the circular difference itself.  Otherwise x0 = -180, L = 360, periodic.
// The same bounds let the query skip a candidate with |dy| > hb, or with |dx| > W in a band of more than one cell, before it
// takes any sine.  Doubling hb (exact) widens every band, lowers c_b and keeps all of the above; the host doubles the delta it
// sizes the longitude cells with alongside (up to pi), which only widens them, so that both directions coarsen together.
constexpr double NB_SPH_MARGIN = 1.0 + 0x1p-16;
constexpr double NB_SPH_LON_ABS = 0x1p-47;    // E / max(360, max |x|)
constexpr double NB_SPH_MIN_COLAT = 0x1p-20;  // radians
constexpr double NB_SPH_MAX_Q = 0.99;
constexpr double NB_SPH_ARC = 179.0;          // degrees: wider sets get periodic bands
constexpr int64_t NB_BAND_CAP = 1ll << 17;    // the host visits every band at every doubling
constexpr double NB_RAD = M_PI / 180.0;       // np.pi / 180
constexpr double NB_HALF_RAD = 0.5 * NB_RAD;  // exact

struct NbBand {
    uint32_t first;  // key of the band's first cell
    int32_t nc;      // cells of the band
    double w;        // their width in degrees, L / nc
};

struct NbSph {
    double ymin, hb;  // southern edge of band 0, band height (degrees)
    double x0;        // western edge of the longitude cells
    double R2;        // 2 * sphere radius
    int32_t nbands, periodic, lon01;  // lon01: longitudes normalised to [0, 360] instead of [-180, 180]
    uint32_t ncells;                  // sum of the bands' cell counts, also the sentinel key of an invalid point
    const NbBand* band;
    const double* cs;  // cos(rad * ys[k]) by sorted slot
};

__device__ __forceinline__ bool sph_valid(double x, double y) { return nb_finite(x) && fabs(y) <= 90.0; }  // false for NaN

__device__ __forceinline__ double sph_wrap(double d) { return d - 360.0 * rint(d / 360.0); }

__device__ __forceinline__ double sph_lon(double x, int32_t lon01) {
    const double xn = sph_wrap(x);
    return (lon01 && xn < 0.0) ? xn + 360.0 : xn;
}

// dh of the header from the wrapped dx, dy and the two cosines
__device__ __forceinline__ double sph_dh(double dx, double dy, double ci, double cj, double R2) {
    const double s1 = sin(NB_HALF_RAD * dy), s2 = sin(NB_HALF_RAD * dx);
    const double a = s1 * s1 + ci * cj * (s2 * s2);
    const double sa = sqrt(a);
    return R2 * asin(sa < 1.0 ? sa : 1.0);
}

// partial[b * 8 + {0..7}] = ymin, ymax, min and max longitude in [-180, 180], the same in [0, 360], max |x|, number of valid points
__global__ void __launch_bounds__(NB_BLOCK) nb_sph_bbox_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                               int64_t n, double* __restrict__ partial) {
    __shared__ double red[NB_BLOCK];
    double v[8] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * NB_BLOCK) {
        const double xi = x[i], yi = y[i];
        if (sph_valid(xi, yi) && (!z || nb_finite(z[i]))) {
            const double w[3] = {yi, sph_lon(xi, 0), sph_lon(xi, 1)};
            for (int k = 0; k < 3; k++) {
                v[2 * k] = w[k] < v[2 * k] ? w[k] : v[2 * k];
                v[2 * k + 1] = w[k] > v[2 * k + 1] ? w[k] : v[2 * k + 1];
            }
            v[6] = fabs(xi) > v[6] ? fabs(xi) : v[6];
            v[7] += 1.0;  // exact: n < 2^53
        }
    }
    for (int k = 0; k < 8; k++) {
        red[threadIdx.x] = v[k];
        __syncthreads();
        for (int s = NB_BLOCK / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                const double a = red[threadIdx.x], b = red[threadIdx.x + s];
                red[threadIdx.x] = k == 7 ? a + b : ((k & 1) || k == 6 ? (b > a ? b : a) : (b < a ? b : a));
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * 8 + k] = red[0];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(NB_BLOCK) nb_sph_key_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                              int64_t n, NbSph g, uint32_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double xi = x[i], yi = y[i];
    uint32_t k = g.ncells;
    if (sph_valid(xi, yi) && (!z || nb_finite(z[i]))) {
        const NbBand b = g.band[cell_of(yi, g.ymin, g.hb, g.nbands)];  // cell_of clamps into [0, nbands)
        k = b.first + (uint32_t)cell_of(sph_lon(xi, g.lon01), g.x0, b.w, b.nc);
    }
    key[i] = k;
    idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(NB_BLOCK) nb_sph_cos_kernel(const double* __restrict__ ys, int64_t n, double* __restrict__ cs) {
    const int64_t k = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (k < n) cs[k] = cos(NB_RAD * ys[k]);  // of an invalid point too: never read
}

template <int MODE, bool HASZ>
__global__ void __launch_bounds__(NB_BLOCK) nb_sph_query_kernel(NbQuery q, NbSph g) {
    const int64_t k = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (k >= q.n) return;
    const uint32_t i = q.idx_s[k];
    int64_t cnt = 0;
    int64_t best_j = -1;
    double best_d = INFINITY;
    int64_t w = 0, w_end = 0;
    if (MODE == NB_FILL) {
        w = q.starts[i];
        w_end = q.starts[i + 1];
    }
    if (q.key_s[k] != g.ncells) {  // a valid point
        const double xi = q.xs[k], yi = q.ys[k], zi = HASZ ? q.zs[k] : 0.0, ci = g.cs[k];
        const double xn = sph_lon(xi, g.lon01);
        const int32_t by = cell_of(yi, g.ymin, g.hb, g.nbands);  // the band nb_sph_key_kernel computed
        for (int32_t ob = -1; ob <= 1; ob++) {
            const int32_t bb = by + ob;
            if (bb < 0 || bb >= g.nbands) continue;
            const NbBand band = g.band[bb];
            const int32_t cx = cell_of(xn, g.x0, band.w, band.nc);
            // cells cx - 1 .. cx + 1 of this band, each once: all of them where a periodic band has fewer than three
            int32_t lo = cx - 1, m = 3;
            if (g.periodic) {
                if (band.nc < 3) {
                    lo = 0;
                    m = band.nc;
                }
            } else {
                lo = lo < 0 ? 0 : lo;
                m = (cx + 1 < band.nc ? cx + 1 : band.nc - 1) - lo + 1;
            }
            for (int32_t t = 0; t < m; t++) {
                int32_t xx = lo + t;
                xx = xx < 0 ? xx + band.nc : (xx >= band.nc ? xx - band.nc : xx);
                const uint32_t c = band.first + (uint32_t)xx;  // < ncells: xx < nc, and first + nc <= ncells by construction
                const int64_t pb = q.cell_begin[c], pe = q.cell_end[c];  // pe <= n: written by nb_gather_kernel from slot numbers
                for (int64_t p = pb; p < pe; p++) {
                    if (p == k || !q.srcs[p]) continue;
                    const double dy = q.ys[p] - yi;
                    if (fabs(dy) > g.hb) continue;  // step 1 of the claim: no neighbour
                    const double dx = sph_wrap(q.xs[p] - xi);
                    if (band.nc > 1 && fabs(dx) > band.w) continue;  // step 2
                    double d = sph_dh(dx, dy, ci, g.cs[p], g.R2);
                    if (HASZ) {
                        const double dz = q.zs[p] - zi;
                        d = sqrt(d * d + dz * dz);
                    }
                    if (!(d < q.radius)) continue;
                    if (q.no_coincident && !(d > 0.0)) continue;
                    if (MODE == NB_COUNT) cnt++;
                    if (MODE == NB_NEAREST) {
                        const int64_t j = q.idx_s[p];
                        if (d < best_d || (d == best_d && j < best_j)) {
                            best_d = d;
                            best_j = j;
                        }
                    }
                    if (MODE == NB_FILL) {
                        if (w < w_end) {
                            q.pair_i[w] = i;
                            q.pair_j[w] = q.idx_s[p];
                        } else {
                            *q.flag = 1;  // more neighbours than the count pass announced: never write past the row
                        }
                        w++;
                    }
                }
            }
        }
    }
    if (MODE == NB_COUNT) q.count[i] = cnt;
    if (MODE == NB_NEAREST) {
        q.near_j[i] = best_j;
        q.near_d[i] = best_d;
    }
    if (MODE == NB_FILL && w != w_end) *q.flag = 1;
}

// one lane per pair, rows already ordered by j: the header's formula from the ORIGINAL arrays
template <bool HASZ>
__global__ void __launch_bounds__(NB_BLOCK) nb_sph_finish_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                 const double* __restrict__ z, int64_t n, int64_t total, double R2,
                                                                 const uint32_t* __restrict__ pair_i, const uint32_t* __restrict__ pair_j,
                                                                 int64_t* __restrict__ out_j, double* __restrict__ out_dx, double* __restrict__ out_dy,
                                                                 double* __restrict__ out_dz, double* __restrict__ out_dist, int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (p >= total) return;
    const uint32_t i = pair_i[p], j = pair_j[p];
    if ((int64_t)i >= n || (int64_t)j >= n) {  // cannot happen after a clean fill; never read out of bounds
        *flag = 1;
        return;
    }
    const double yi = y[i], yj = y[j];
    const double dx = sph_wrap(x[j] - x[i]), dy = yj - yi;
    double d = sph_dh(dx, dy, cos(NB_RAD * yi), cos(NB_RAD * yj), R2);
    if (HASZ) {
        const double dz = z[j] - z[i];
        d = sqrt(d * d + dz * dz);
        out_dz[p] = dz;
    }
    out_j[p] = (int64_t)j;
    out_dx[p] = dx;
    out_dy[p] = dy;
    out_dist[p] = d;
}

// device-resident input (NeighborsDeviceInput): the columns widened into the build's own float64 arrays; a row outside the mask gets a
// NaN x, which every later pass treats as a non-finite point
template <class T>
__global__ void __launch_bounds__(NB_BLOCK) nb_load_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                           const int32_t* __restrict__ mask, const uint8_t* __restrict__ src_in, int64_t n,
                                                           double* __restrict__ ox, double* __restrict__ oy, double* __restrict__ oz,
                                                           uint8_t* __restrict__ osrc) {
    const int64_t i = (int64_t)blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= n) return;
    ox[i] = (!mask || mask[i] != 0) ? (double)x[i] : (double)NAN;
    oy[i] = (double)y[i];
    if (z) oz[i] = (double)z[i];
    if (src_in) osrc[i] = src_in[i];
}

struct Buf {  // grow-only device buffer
    void* p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void drop() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};

inline unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + NB_BLOCK - 1) / NB_BLOCK); }

inline unsigned bits_for(uint64_t max_value) {  // radix bits that cover 0 .. max_value
    unsigned b = 1;
    while (b < 32 && (max_value >> b) != 0) b++;
    return b;
}

#define NB_TRY(call)                                                                   \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            if (err) *err = std::string("neighbors: " #call ": ") + hipGetErrorString(e_); \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

}  // namespace

struct Neighbors {
    // per point
    Buf x, y, z, src, key, key_s, idx, idx_s, xs, ys, zs, srcs, count, starts, near_j, near_d;
    // per cell, per call
    Buf cell_begin, cell_end, partial, tmp, flag;
    // spherical builds: per band, per point
    Buf band, cs;
    // one byte per row, kept between builds (neighbors_set_sources)
    Buf src_in;
    int64_t src_in_n = -1;
    // per pair
    Buf pair_i, pair_j, pair_js, out_j, out_dx, out_dy, out_dz, out_dist;
    bool built = false, has_z = false, has_src = false, spherical = false;
    int64_t n = 0, nvalid = 0, total = -1;
    double radius = 0;
    int32_t flags = 0, doublings = 0;
    NbGrid g{};   // flat builds
    NbSph sg{};   // spherical builds

    Buf* all[32] = {&x, &y, &z, &src, &key, &key_s, &idx, &idx_s, &xs, &ys, &zs, &srcs, &count, &starts, &near_j, &near_d,
                    &cell_begin, &cell_end, &partial, &tmp, &flag, &band, &cs, &pair_i, &pair_j, &pair_js, &out_j, &out_dx, &out_dy, &out_dz,
                    &out_dist, &src_in};

    NbQuery query() const {
        NbQuery q{};
        q.n = n;
        q.g = g;
        q.radius = radius;
        q.no_coincident = (flags & 1) != 0;
        q.key_s = key_s.as<uint32_t>();
        q.idx_s = idx_s.as<uint32_t>();
        q.cell_begin = cell_begin.as<uint32_t>();
        q.cell_end = cell_end.as<uint32_t>();
        q.xs = xs.as<double>();
        q.ys = ys.as<double>();
        q.zs = has_z ? zs.as<double>() : nullptr;
        q.srcs = srcs.as<uint8_t>();
        q.flag = flag.as<int32_t>();
        return q;
    }
};

Neighbors* neighbors_create() { return new Neighbors(); }

void neighbors_release(Neighbors* nb) {
    if (!nb) return;
    for (Buf* b : nb->all) b->drop();
    nb->src_in_n = -1;
    nb->built = false;
    nb->n = 0;
    nb->total = -1;
}

void neighbors_free(Neighbors* nb) {
    if (!nb) return;
    neighbors_release(nb);
    delete nb;
}

void neighbors_info(const Neighbors* nb, NeighborsInfo* out) {
    *out = NeighborsInfo();
    if (!nb || !nb->built || nb->spherical) return;
    out->n = nb->n;
    out->nvalid = nb->nvalid;
    out->ncx = nb->g.ncx;
    out->ncy = nb->g.ncy;
    out->h = nb->g.h;
    out->doublings = nb->doublings;
    out->total = nb->total;
}

namespace {
// What both builds begin with: argument checks, the per-point buffers and the upload.  Returns 1 for n == 0 (an empty list is
// built, nothing else to do), 0 to go on, a negative code with *err set.
// din: the points are device columns (NeighborsDeviceInput) instead of the host arrays x, y, z, sources.
int build_begin(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources,
                const NeighborsDeviceInput* din, double radius, int32_t flags, bool spherical, std::string* err) {
    nb->built = false;
    nb->total = -1;
    if (n < 0 || n > NB_MAX_POINTS) {
        if (err) *err = "neighbors: n must be between 0 and 2147483646";
        return -2;
    }
    if (!(radius > 0.0) || !(radius <= DBL_MAX)) {
        if (err) *err = "neighbors: radius must be a finite positive number";
        return -2;
    }
    if (n > 0 && (din ? (!din->x || !din->y) : (!x || !y))) {
        if (err) *err = "neighbors: x and y must not be NULL";
        return -2;
    }
    if (din && din->use_sources && nb->src_in_n != n) {
        if (err) *err = "neighbors: the source flags were set for another number of rows (neighbors_set_sources)";
        return -2;
    }
    const bool has_z = din ? din->z != nullptr : z != nullptr;
    const bool has_src = din ? din->use_sources != 0 : sources != nullptr;
    nb->n = n;
    nb->radius = radius;
    nb->flags = flags;
    nb->has_z = has_z;
    nb->has_src = has_src;
    nb->spherical = spherical;
    nb->nvalid = 0;
    nb->doublings = 0;
    nb->g = NbGrid{0.0, 0.0, radius, 1, 1, 1u};
    nb->sg = NbSph{};
    NB_TRY(nb->flag.need(sizeof(int32_t)));
    if (n == 0) {
        nb->built = true;
        return 1;
    }
    const size_t nd = (size_t)n * sizeof(double), nu = (size_t)n * sizeof(uint32_t);
    NB_TRY(nb->x.need(nd));
    NB_TRY(nb->y.need(nd));
    NB_TRY(nb->xs.need(nd));
    NB_TRY(nb->ys.need(nd));
    if (has_z) {
        NB_TRY(nb->z.need(nd));
        NB_TRY(nb->zs.need(nd));
    }
    if (spherical) NB_TRY(nb->cs.need(nd));
    if (has_src) NB_TRY(nb->src.need((size_t)n));
    NB_TRY(nb->srcs.need((size_t)n));
    NB_TRY(nb->key.need(nu));
    NB_TRY(nb->key_s.need(nu));
    NB_TRY(nb->idx.need(nu));
    NB_TRY(nb->idx_s.need(nu));
    NB_TRY(nb->partial.need((size_t)NB_BBOX_BLOCKS * 8 * sizeof(double)));
    if (din) {
        double* oz = has_z ? nb->z.as<double>() : nullptr;
        const uint8_t* si = has_src ? nb->src_in.as<uint8_t>() : nullptr;
        if (din->f32)
            hipLaunchKernelGGL((nb_load_kernel<float>), dim3(blocks_for(n)), dim3(NB_BLOCK), 0, stream, (const float*)din->x, (const float*)din->y,
                               (const float*)din->z, din->mask, si, n, nb->x.as<double>(), nb->y.as<double>(), oz, nb->src.as<uint8_t>());
        else
            hipLaunchKernelGGL((nb_load_kernel<double>), dim3(blocks_for(n)), dim3(NB_BLOCK), 0, stream, (const double*)din->x, (const double*)din->y,
                               (const double*)din->z, din->mask, si, n, nb->x.as<double>(), nb->y.as<double>(), oz, nb->src.as<uint8_t>());
        NB_TRY(hipGetLastError());
        return 0;
    }
    NB_TRY(hipMemcpyAsync(nb->x.p, x, nd, hipMemcpyHostToDevice, stream));
    NB_TRY(hipMemcpyAsync(nb->y.p, y, nd, hipMemcpyHostToDevice, stream));
    if (z) NB_TRY(hipMemcpyAsync(nb->z.p, z, nd, hipMemcpyHostToDevice, stream));
    if (sources) NB_TRY(hipMemcpyAsync(nb->src.p, sources, (size_t)n, hipMemcpyHostToDevice, stream));
    return 0;
}

// zeroed slot ranges for ncells cells + the sentinel's (before the key kernel: both builds call this, launch their key kernel,
// then build_sort_gather)
int build_cells(Neighbors* nb, hipStream_t stream, uint32_t ncells, std::string* err) {
    const size_t cell_bytes = ((size_t)ncells + 1) * sizeof(uint32_t);
    NB_TRY(nb->cell_begin.need(cell_bytes));
    NB_TRY(nb->cell_end.need(cell_bytes));
    NB_TRY(hipMemsetAsync(nb->cell_begin.p, 0, cell_bytes, stream));
    NB_TRY(hipMemsetAsync(nb->cell_end.p, 0, cell_bytes, stream));
    return 0;
}

// stable sort of (key, index), coordinates into sorted order, slot range of every occupied cell
int build_sort_gather(Neighbors* nb, hipStream_t stream, uint32_t ncells, std::string* err) {
    const int64_t n = nb->n;
    const unsigned bits = bits_for(ncells);
    size_t tb = 0;
    NB_TRY(rocprim::radix_sort_pairs(nullptr, tb, nb->key.as<uint32_t>(), nb->key_s.as<uint32_t>(), nb->idx.as<uint32_t>(), nb->idx_s.as<uint32_t>(),
                                     (size_t)n, 0u, bits, stream));
    NB_TRY(nb->tmp.need(std::max<size_t>(tb, 16)));
    NB_TRY(rocprim::radix_sort_pairs(nb->tmp.p, tb, nb->key.as<uint32_t>(), nb->key_s.as<uint32_t>(), nb->idx.as<uint32_t>(), nb->idx_s.as<uint32_t>(),
                                     (size_t)n, 0u, bits, stream));
    hipLaunchKernelGGL(nb_gather_kernel, dim3(blocks_for(n)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(),
                       nb->has_z ? nb->z.as<double>() : nullptr, nb->has_src ? nb->src.as<uint8_t>() : nullptr, n, nb->key_s.as<uint32_t>(),
                       nb->idx_s.as<uint32_t>(), nb->xs.as<double>(), nb->ys.as<double>(), nb->has_z ? nb->zs.as<double>() : nullptr,
                       nb->srcs.as<uint8_t>(), nb->cell_begin.as<uint32_t>(), nb->cell_end.as<uint32_t>());
    return 0;
}
}  // namespace

namespace {
int build_flat(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources,
               const NeighborsDeviceInput* din, double radius, int32_t flags, std::string* err) {
    if (int rc = build_begin(nb, stream, n, x, y, z, sources, din, radius, flags, false, err)) return rc < 0 ? rc : 0;
    const double* dz = nb->has_z ? nb->z.as<double>() : nullptr;

    // 1. bounding box of the finite points
    const unsigned nbb = std::min<unsigned>(blocks_for(n), NB_BBOX_BLOCKS);
    hipLaunchKernelGGL(nb_bbox_kernel, dim3(nbb), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), dz, n, nb->partial.as<double>());
    std::vector<double> partial((size_t)nbb * 5);
    NB_TRY(hipMemcpyAsync(partial.data(), nb->partial.p, partial.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    NB_TRY(hipStreamSynchronize(stream));
    double bb[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY}, nvalid = 0;
    for (unsigned b = 0; b < nbb; b++) {
        const double* r = &partial[(size_t)b * 5];
        bb[0] = std::min(bb[0], r[0]);
        bb[1] = std::max(bb[1], r[1]);
        bb[2] = std::min(bb[2], r[2]);
        bb[3] = std::max(bb[3], r[3]);
        nvalid += r[4];
    }
    nb->nvalid = (int64_t)nvalid;

    // 2. cell size (see the argument at NB_CELL_MARGIN): a hair above the radius, doubled until the grid is under the cap
    NbGrid g{0.0, 0.0, radius, 1, 1, 1u};
    if (nb->nvalid > 0) {
        const int64_t cap = std::min(std::max(NB_CELL_CAP_MIN, 4 * n), NB_CELL_CAP_MAX);
        const double ex = bb[1] - bb[0], ey = bb[3] - bb[2];
        double h = std::max(radius * NB_CELL_MARGIN, NB_CELL_MIN);
        bool fits = false;
        int d = 0;
        for (; d < 2200 && h <= DBL_MAX; d++) {  // 2200 doublings span every float64 exponent
            const double fx = std::floor(ex / h) + 1.0, fy = std::floor(ey / h) + 1.0;
            if (fx * fy <= (double)cap) {  // false for the NaN / inf of an overflowing extent
                g.ncx = (int32_t)fx;
                g.ncy = (int32_t)fy;
                fits = true;
                break;
            }
            h *= 2.0;
        }
        g.xmin = bb[0];
        g.ymin = bb[2];
        if (fits) {
            g.h = h;
            nb->doublings = d;
        } else {  // xmax - xmin overflows: one cell, every pair is examined
            g.h = DBL_MAX;
            g.ncx = g.ncy = 1;
        }
        g.ncells = (uint32_t)((int64_t)g.ncx * g.ncy);
    }
    nb->g = g;

    // 3. keys, stable sort, gather
    if (int rc = build_cells(nb, stream, g.ncells, err)) return rc;
    hipLaunchKernelGGL(nb_key_kernel, dim3(blocks_for(n)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), dz, n, g,
                       nb->key.as<uint32_t>(), nb->idx.as<uint32_t>());
    if (int rc = build_sort_gather(nb, stream, g.ncells, err)) return rc;
    NB_TRY(hipGetLastError());
    NB_TRY(hipStreamSynchronize(stream));
    nb->built = true;
    return 0;
}
}  // namespace

int neighbors_build(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources,
                    double radius, int32_t flags, std::string* err) {
    return build_flat(nb, stream, n, x, y, z, sources, nullptr, radius, flags, err);
}

namespace {
// The band table of one band height (NB_SPH_MARGIN, step 2).  Returns the total number of cells, or -1 as soon as it passes cap.
int64_t sph_bands(std::vector<NbBand>& table, int64_t nbands, double ymin, double hb, double L, double sin_half_delta, double lon_abs,
                  int64_t cap) {
    table.resize((size_t)nbands);
    int64_t cells = 0;
    for (int64_t b = 0; b < nbands; b++) {
        const double lo = ymin + ((double)b - 1.0 - 0x1p-10) * hb - 0x1p-40, hi = ymin + ((double)b + 2.0 + 0x1p-10) * hb + 0x1p-40;
        const double colat = (90.0 - std::min(90.0, std::max(std::fabs(lo), std::fabs(hi)))) * NB_RAD;
        double nc = 1.0;
        if (colat >= NB_SPH_MIN_COLAT) {
            const double q = sin_half_delta / std::sin(colat);
            if (q <= NB_SPH_MAX_Q) nc = std::max(1.0, std::floor(L / (2.0 * std::asin(q) / NB_RAD * NB_SPH_MARGIN + lon_abs)));
        }
        if (!(nc <= (double)(cap - cells))) return -1;
        table[(size_t)b] = NbBand{(uint32_t)cells, (int32_t)nc, L / nc};
        cells += (int64_t)nc;
    }
    return cells;
}

int build_spherical(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources,
                    const NeighborsDeviceInput* din, double radius, double sphere_radius, int32_t flags, std::string* err) {
    if (!(sphere_radius > 0.0) || !(sphere_radius <= DBL_MAX) || !(radius < M_PI_2 * sphere_radius)) {
        nb->built = false;
        if (err) *err = "neighbors: the sphere radius must be finite and positive, and radius below a quarter of its circumference";
        return -2;
    }
    if (int rc = build_begin(nb, stream, n, x, y, z, sources, din, radius, flags, true, err)) return rc < 0 ? rc : 0;
    const double* dz = nb->has_z ? nb->z.as<double>() : nullptr;

    // 1. extent of the valid points: latitude, longitude in both normalisations, max |x|
    const unsigned nbb = std::min<unsigned>(blocks_for(n), NB_BBOX_BLOCKS);
    hipLaunchKernelGGL(nb_sph_bbox_kernel, dim3(nbb), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), dz, n,
                       nb->partial.as<double>());
    std::vector<double> partial((size_t)nbb * 8);
    NB_TRY(hipMemcpyAsync(partial.data(), nb->partial.p, partial.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    NB_TRY(hipStreamSynchronize(stream));
    double bb[8] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    for (unsigned b = 0; b < nbb; b++) {
        const double* r = &partial[(size_t)b * 8];
        for (int k = 0; k < 6; k++) bb[k] = (k & 1) ? std::max(bb[k], r[k]) : std::min(bb[k], r[k]);
        bb[6] = std::max(bb[6], r[6]);
        bb[7] += r[7];
    }
    nb->nvalid = (int64_t)bb[7];

    // 2. bands and their longitude cells (see the argument at NB_SPH_MARGIN); the band height is doubled until both are under
    //    their caps.  One band of one cell without a valid point.
    NbSph g{};
    g.R2 = 2.0 * sphere_radius;
    g.hb = 180.0;
    g.nbands = 1;
    g.periodic = 1;
    g.x0 = -180.0;
    g.ncells = 1;
    std::vector<NbBand> table(1, NbBand{0u, 1, 360.0});
    if (nb->nvalid > 0) {
        const double delta = radius / sphere_radius, lon_abs = NB_SPH_LON_ABS * std::max(360.0, bb[6]);
        const int lon01 = (bb[5] - bb[4]) < (bb[3] - bb[2]);
        double L = lon01 ? bb[5] - bb[4] : bb[3] - bb[2];
        if (L < NB_SPH_ARC && lon_abs < 1.0) {
            g.periodic = 0;
            g.lon01 = lon01;
            g.x0 = lon01 ? bb[4] : bb[2];
        } else {
            L = 360.0;
        }
        g.ymin = bb[0];
        const int64_t cap = std::min(std::max(NB_CELL_CAP_MIN, 4 * n), NB_CELL_CAP_MAX);
        const double ey = bb[1] - bb[0];  // <= 180
        double hb = std::max(delta / NB_RAD * NB_SPH_MARGIN, NB_CELL_MIN);
        int64_t cells = -1;
        int d = 0;
        double dl = delta;  // doubled with hb, so that the longitude cells coarsen with the bands; a larger delta only widens them
        for (; d < 2200; d++, hb *= 2.0, dl = std::min(2.0 * dl, M_PI)) {  // ends at hb > 180 at the latest: one band, one cell
            const double fb = std::floor(ey / hb) + 1.0;
            if (fb <= (double)NB_BAND_CAP) cells = sph_bands(table, (int64_t)fb, g.ymin, hb, L, std::sin(0.5 * dl), lon_abs, cap);
            if (cells >= 0) break;
        }
        if (cells < 0) {
            if (err) *err = "neighbors: no band height fits the cell caps";
            return -3;
        }
        g.hb = hb;
        g.nbands = (int32_t)table.size();
        g.ncells = (uint32_t)cells;
        nb->doublings = d;
    }
    NB_TRY(nb->band.need(table.size() * sizeof(NbBand)));
    NB_TRY(hipMemcpyAsync(nb->band.p, table.data(), table.size() * sizeof(NbBand), hipMemcpyHostToDevice, stream));
    g.band = nb->band.as<NbBand>();
    g.cs = nb->cs.as<double>();
    nb->sg = g;

    // 3. keys, stable sort, gather, cosines
    if (int rc = build_cells(nb, stream, g.ncells, err)) return rc;
    hipLaunchKernelGGL(nb_sph_key_kernel, dim3(blocks_for(n)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), dz, n, g,
                       nb->key.as<uint32_t>(), nb->idx.as<uint32_t>());
    if (int rc = build_sort_gather(nb, stream, g.ncells, err)) return rc;
    hipLaunchKernelGGL(nb_sph_cos_kernel, dim3(blocks_for(n)), dim3(NB_BLOCK), 0, stream, nb->ys.as<double>(), n, nb->cs.as<double>());
    NB_TRY(hipGetLastError());
    NB_TRY(hipStreamSynchronize(stream));  // also: `table` is read by the copy until here
    nb->built = true;
    return 0;
}
}  // namespace

int neighbors_build_spherical(Neighbors* nb, hipStream_t stream, int64_t n, const double* x, const double* y, const double* z,
                              const uint8_t* sources, double radius, double sphere_radius, int32_t flags, std::string* err) {
    return build_spherical(nb, stream, n, x, y, z, sources, nullptr, radius, sphere_radius, flags, err);
}

int neighbors_set_sources(Neighbors* nb, hipStream_t stream, int64_t n, const uint8_t* sources, std::string* err) {
    nb->src_in_n = -1;
    if (n < 0 || n > NB_MAX_POINTS || (n > 0 && !sources)) {
        if (err) *err = "neighbors: source flags need one byte per row";
        return -2;
    }
    if (n > 0) {
        NB_TRY(nb->src_in.need((size_t)n));
        NB_TRY(hipMemcpyAsync(nb->src_in.p, sources, (size_t)n, hipMemcpyHostToDevice, stream));
        NB_TRY(hipStreamSynchronize(stream));  // the host array is the caller's
    }
    nb->src_in_n = n;
    return 0;
}

int neighbors_build_device(Neighbors* nb, hipStream_t stream, int64_t n, const NeighborsDeviceInput& in, double radius, double sphere_radius,
                           int32_t flags, std::string* err) {
    if (sphere_radius != 0.0) return build_spherical(nb, stream, n, nullptr, nullptr, nullptr, nullptr, &in, radius, sphere_radius, flags, err);
    return build_flat(nb, stream, n, nullptr, nullptr, nullptr, nullptr, &in, radius, flags, err);
}

void neighbors_device_view(const Neighbors* nb, NeighborsDeviceView* out) {
    *out = NeighborsDeviceView();
    if (!nb || !nb->built) return;
    out->n = nb->n;
    out->total = nb->total < 0 ? 0 : nb->total;
    out->starts = nb->starts.as<int64_t>();
    out->dx = nb->out_dx.as<double>();
    out->dy = nb->out_dy.as<double>();
    out->dz = nb->has_z ? nb->out_dz.as<double>() : nullptr;
    out->dist = nb->out_dist.as<double>();
    out->near_j = nb->near_j.as<int64_t>();
    out->flag = nb->flag.as<int32_t>();
}

void neighbors_info_spherical(const Neighbors* nb, NeighborsSphInfo* out) {
    *out = NeighborsSphInfo();
    if (!nb || !nb->built || !nb->spherical) return;
    out->n = nb->n;
    out->nvalid = nb->nvalid;
    out->bands = nb->sg.nbands;
    out->cells = nb->sg.ncells;
    out->band_height = nb->sg.hb;
    out->periodic = nb->sg.periodic;
    out->doublings = nb->doublings;
    out->total = nb->total;
}

namespace {
int need_built(const Neighbors* nb, std::string* err) {
    if (nb && nb->built) return 0;
    if (err) *err = "neighbors: no cell list (build one first)";
    return -2;
}

template <int MODE>
void launch_query(const Neighbors* nb, hipStream_t stream, const NbQuery& q) {
    const dim3 grid(blocks_for(q.n)), block(NB_BLOCK);
    if (nb->spherical) {
        if (nb->has_z) hipLaunchKernelGGL((nb_sph_query_kernel<MODE, true>), grid, block, 0, stream, q, nb->sg);
        else hipLaunchKernelGGL((nb_sph_query_kernel<MODE, false>), grid, block, 0, stream, q, nb->sg);
    } else if (nb->has_z) {
        hipLaunchKernelGGL((nb_query_kernel<MODE, true>), grid, block, 0, stream, q);
    } else {
        hipLaunchKernelGGL((nb_query_kernel<MODE, false>), grid, block, 0, stream, q);
    }
}
}  // namespace

int neighbors_counts(Neighbors* nb, hipStream_t stream, int64_t* counts, int64_t* total, std::string* err) {
    if (int rc = need_built(nb, err)) return rc;
    const int64_t n = nb->n;
    nb->total = -1;
    if (n == 0) {
        nb->total = 0;
        if (total) *total = 0;
        return 0;
    }
    // count[n] = 0, so that the exclusive scan over n + 1 entries ends with the total
    const size_t bytes = (size_t)(n + 1) * sizeof(int64_t);
    NB_TRY(nb->count.need(bytes));
    NB_TRY(nb->starts.need(bytes));
    NB_TRY(hipMemsetAsync(nb->count.as<int64_t>() + n, 0, sizeof(int64_t), stream));
    NbQuery q = nb->query();
    q.count = nb->count.as<int64_t>();
    launch_query<NB_COUNT>(nb, stream, q);
    size_t tb = 0;
    NB_TRY(rocprim::exclusive_scan(nullptr, tb, nb->count.as<int64_t>(), nb->starts.as<int64_t>(), (int64_t)0, (size_t)(n + 1),
                                   rocprim::plus<int64_t>(), stream));
    NB_TRY(nb->tmp.need(std::max<size_t>(tb, 16)));
    NB_TRY(rocprim::exclusive_scan(nb->tmp.p, tb, nb->count.as<int64_t>(), nb->starts.as<int64_t>(), (int64_t)0, (size_t)(n + 1),
                                   rocprim::plus<int64_t>(), stream));
    int64_t t = 0;
    NB_TRY(hipMemcpyAsync(&t, nb->starts.as<int64_t>() + n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    if (counts) NB_TRY(hipMemcpyAsync(counts, nb->count.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    NB_TRY(hipGetLastError());
    NB_TRY(hipStreamSynchronize(stream));
    nb->total = t;
    if (total) *total = t;
    return 0;
}

int neighbors_nearest_device(Neighbors* nb, hipStream_t stream, std::string* err) {
    if (int rc = need_built(nb, err)) return rc;
    const int64_t n = nb->n;
    if (n == 0) return 0;
    NB_TRY(nb->near_j.need((size_t)n * sizeof(int64_t)));
    NB_TRY(nb->near_d.need((size_t)n * sizeof(double)));
    NbQuery q = nb->query();
    q.near_j = nb->near_j.as<int64_t>();
    q.near_d = nb->near_d.as<double>();
    launch_query<NB_NEAREST>(nb, stream, q);
    NB_TRY(hipGetLastError());
    return 0;
}

int neighbors_nearest(Neighbors* nb, hipStream_t stream, int64_t* j, double* dist, std::string* err) {
    if (int rc = need_built(nb, err)) return rc;
    const int64_t n = nb->n;
    if (n == 0) return 0;
    if (!j || !dist) {
        if (err) *err = "neighbors: nearest needs both output arrays";
        return -2;
    }
    if (int rc = neighbors_nearest_device(nb, stream, err)) return rc;
    NB_TRY(hipMemcpyAsync(j, nb->near_j.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    NB_TRY(hipMemcpyAsync(dist, nb->near_d.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    NB_TRY(hipGetLastError());
    NB_TRY(hipStreamSynchronize(stream));
    return 0;
}

namespace {
int pairs_check(const Neighbors* nb, int64_t total, std::string* err) {
    if (int rc = need_built(nb, err)) return rc;
    if (nb->total < 0) {
        if (err) *err = "neighbors: pairs need the count pass first";
        return -2;
    }
    if (total != nb->total) {
        if (err) *err = "neighbors: pairs asked for " + std::to_string(total) + " pairs, the count pass announced " + std::to_string(nb->total);
        return -2;
    }
    if (total > NB_MAX_PAIRS) {
        if (err) *err = "neighbors: " + std::to_string(total) + " pairs exceed the 2147483647 one call can list";
        return -2;
    }
    return 0;
}
}  // namespace

int neighbors_pairs(Neighbors* nb, hipStream_t stream, int64_t total, int64_t* starts, int64_t* j, double* dx, double* dy, double* dz,
                    double* dist, std::string* err) {
    if (int rc = pairs_check(nb, total, err)) return rc;
    const int64_t n = nb->n;
    if (!starts || (total > 0 && (!j || !dx || !dy || !dist || (nb->has_z && !dz)))) {
        if (err) *err = "neighbors: pairs need every output array";
        return -2;
    }
    if (n == 0) {
        starts[0] = 0;
        return 0;
    }
    NB_TRY(hipMemcpyAsync(starts, nb->starts.p, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    if (total == 0) {
        NB_TRY(hipStreamSynchronize(stream));
        return 0;
    }
    if (int rc = neighbors_pairs_device(nb, stream, total, err)) return rc;
    const size_t pd = (size_t)total * sizeof(double);
    NB_TRY(hipMemcpyAsync(j, nb->out_j.p, pd, hipMemcpyDeviceToHost, stream));
    NB_TRY(hipMemcpyAsync(dx, nb->out_dx.p, pd, hipMemcpyDeviceToHost, stream));
    NB_TRY(hipMemcpyAsync(dy, nb->out_dy.p, pd, hipMemcpyDeviceToHost, stream));
    if (nb->has_z) NB_TRY(hipMemcpyAsync(dz, nb->out_dz.p, pd, hipMemcpyDeviceToHost, stream));
    NB_TRY(hipMemcpyAsync(dist, nb->out_dist.p, pd, hipMemcpyDeviceToHost, stream));
    NB_TRY(hipStreamSynchronize(stream));
    return 0;
}

int neighbors_pairs_device(Neighbors* nb, hipStream_t stream, int64_t total, std::string* err) {
    if (int rc = pairs_check(nb, total, err)) return rc;
    const int64_t n = nb->n;
    if (n == 0 || total == 0) return 0;
    const size_t pu = (size_t)total * sizeof(uint32_t), pd = (size_t)total * sizeof(double);
    NB_TRY(nb->pair_i.need(pu));
    NB_TRY(nb->pair_j.need(pu));
    NB_TRY(nb->pair_js.need(pu));
    NB_TRY(nb->out_j.need(pd));
    NB_TRY(nb->out_dx.need(pd));
    NB_TRY(nb->out_dy.need(pd));
    NB_TRY(nb->out_dist.need(pd));
    if (nb->has_z) NB_TRY(nb->out_dz.need(pd));
    NB_TRY(hipMemsetAsync(nb->flag.p, 0, sizeof(int32_t), stream));
    // fill: unordered within a row
    NbQuery q = nb->query();
    q.starts = nb->starts.as<int64_t>();
    q.pair_i = nb->pair_i.as<uint32_t>();
    q.pair_j = nb->pair_j.as<uint32_t>();
    launch_query<NB_FILL>(nb, stream, q);
    // rows ordered by j
    const int64_t* offs = nb->starts.as<int64_t>();
    const unsigned bits = bits_for((uint64_t)n);
    size_t tb = 0;
    NB_TRY(rocprim::segmented_radix_sort_keys(nullptr, tb, nb->pair_j.as<uint32_t>(), nb->pair_js.as<uint32_t>(), (unsigned)total, (unsigned)n, offs,
                                              offs + 1, 0u, bits, stream));
    NB_TRY(nb->tmp.need(std::max<size_t>(tb, 16)));
    NB_TRY(rocprim::segmented_radix_sort_keys(nb->tmp.p, tb, nb->pair_j.as<uint32_t>(), nb->pair_js.as<uint32_t>(), (unsigned)total, (unsigned)n, offs,
                                              offs + 1, 0u, bits, stream));
    const double* zz = nb->has_z ? nb->z.as<double>() : nullptr;
    if (nb->spherical && nb->has_z)
        hipLaunchKernelGGL((nb_sph_finish_kernel<true>), dim3(blocks_for(total)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), zz,
                           n, total, nb->sg.R2, nb->pair_i.as<uint32_t>(), nb->pair_js.as<uint32_t>(), nb->out_j.as<int64_t>(),
                           nb->out_dx.as<double>(), nb->out_dy.as<double>(), nb->out_dz.as<double>(), nb->out_dist.as<double>(), nb->flag.as<int32_t>());
    else if (nb->spherical)
        hipLaunchKernelGGL((nb_sph_finish_kernel<false>), dim3(blocks_for(total)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), zz,
                           n, total, nb->sg.R2, nb->pair_i.as<uint32_t>(), nb->pair_js.as<uint32_t>(), nb->out_j.as<int64_t>(),
                           nb->out_dx.as<double>(), nb->out_dy.as<double>(), (double*)nullptr, nb->out_dist.as<double>(), nb->flag.as<int32_t>());
    else if (nb->has_z)
        hipLaunchKernelGGL((nb_finish_kernel<true>), dim3(blocks_for(total)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), zz, n,
                           total, nb->pair_i.as<uint32_t>(), nb->pair_js.as<uint32_t>(), nb->out_j.as<int64_t>(), nb->out_dx.as<double>(),
                           nb->out_dy.as<double>(), nb->out_dz.as<double>(), nb->out_dist.as<double>(), nb->flag.as<int32_t>());
    else
        hipLaunchKernelGGL((nb_finish_kernel<false>), dim3(blocks_for(total)), dim3(NB_BLOCK), 0, stream, nb->x.as<double>(), nb->y.as<double>(), zz, n,
                           total, nb->pair_i.as<uint32_t>(), nb->pair_js.as<uint32_t>(), nb->out_j.as<int64_t>(), nb->out_dx.as<double>(),
                           nb->out_dy.as<double>(), (double*)nullptr, nb->out_dist.as<double>(), nb->flag.as<int32_t>());
    int32_t flag = 0;
    NB_TRY(hipMemcpyAsync(&flag, nb->flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    NB_TRY(hipGetLastError());
    NB_TRY(hipStreamSynchronize(stream));
    if (flag) {
        if (err) *err = "neighbors: the fill pass disagreed with the count pass (no pair was written out of its row)";
        return -3;
    }
    return 0;
}

}  // namespace pk
