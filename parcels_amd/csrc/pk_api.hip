// pk_api.hip -- host side of libparcels_hip.so: the C ABI of include/parcels_hip.h.
//
// Owns device memory (grids, field-level rings, particle columns), two HIP streams (compute + copy, so that
// the upload of the next time level overlaps the RK sub-steps of the current one) and the launch logic.
// gfx950 only; no CUDA/other-backend paths.
#include "pk_api_ctx.h"

#include <rocprim/rocprim.hpp>

using namespace pkapi;

namespace pkapi {
std::string g_init_error;
}

// ---- small device kernels owned by this TU ------------------------------------------------------------
namespace pk {

PK_DEV unsigned long long order_double(double v) {  // order-preserving map double -> u64
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// histogram of `state` + min/max of t over particles still in Evaluate
// Clock probe, running NEXT TO the advection kernel (its own stream): 16 single-wavefront workgroups (dealt round-robin over the 8 XCDs) each
// spin for `ticks` of the constant 100 MHz counter (s_memrealtime) and count the shader-clock cycles (s_memtime) that passed meanwhile --
// both read by the SAME wavefront, so no pairing of counters across XCDs or launches is involved (the first version of this round paired
// two probes around the kernel by XCC id and produced 2.0 ... 6.0 GHz for one and the same launch; a probe BEHIND the kernel reads the idle
// boost clock, 2.41-2.44 GHz, not the clock under the fp64 load).  One wavefront on 16 of the 1024 SIMDs: below the noise of the timed kernel.
__global__ void __launch_bounds__(64) clock_probe_kernel(unsigned long long* out, unsigned long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c0 = __builtin_readcyclecounter();
    unsigned long long r = r0;
    while (r - r0 < ticks) {
        __builtin_amdgcn_s_sleep(8);
        r = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    out[blockIdx.x * 2] = c1 - c0;
    out[blockIdx.x * 2 + 1] = r - r0;
}

__global__ void __launch_bounds__(256) summarize_kernel(const int32_t* state, const double* t, int64_t n,
                                                        unsigned long long* out) {
    __shared__ unsigned int hist[PK_NUM_STATE_CODES];
    __shared__ unsigned long long smin, smax;
    for (int k = threadIdx.x; k < PK_NUM_STATE_CODES; k += 256) hist[k] = 0;
    if (threadIdx.x == 0) { smin = ~0ull; smax = 0ull; }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int s = state[i];
        if (s >= 0 && s < PK_NUM_STATE_CODES) atomicAdd(&hist[s], 1u);
        if (s == PK_EVALUATE) {
            unsigned long long o = order_double(t[i]);
            atomicMin(&smin, o);
            atomicMax(&smax, o);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PK_NUM_STATE_CODES; k += 256)
        if (hist[k]) atomicAdd(&out[k], (unsigned long long)hist[k]);
    if (threadIdx.x == 0) {
        atomicMin(&out[PK_NUM_STATE_CODES], smin);
        atomicMax(&out[PK_NUM_STATE_CODES + 1], smax);
    }
}

// ---- cell sort ----------------------------------------------------------------------------------------
// (its key kernel, sort_key_kernel, is compiled in pk_api_sample.hip, behind sort_keys: see there)
template <class T>
__global__ void __launch_bounds__(256) gather_rows_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                          const uint32_t* __restrict__ perm, int64_t n, int width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t src = perm[i];
    for (int k = 0; k < width; k++) out[i * width + k] = in[src * width + k];
}
// out[i] = in[perm[i]] with the int64 device-row -> host-row map of the cell sort (pk_particles_h2d_columns)
template <class T>
__global__ void __launch_bounds__(256) gather_rows64_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                            const int64_t* __restrict__ perm, int64_t n, int width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t src = perm[i];
    for (int k = 0; k < width; k++) out[i * width + k] = in[src * width + k];
}
__global__ void __launch_bounds__(256) fill_f64_kernel(double* __restrict__ out, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}
// smallest / largest finite-or-infinite (non-NaN) t as order-preserving integers, and the NaN count: out[0] = min, out[1] = max, out[2] = NaNs
__global__ void __launch_bounds__(256) t_stats_kernel(const double* __restrict__ t, int64_t n, unsigned long long* __restrict__ out) {
    unsigned long long lo = ~0ull, hi = 0ull, nn = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = t[i];
        if (v != v) { nn++; continue; }
        unsigned long long b;
        memcpy(&b, &v, 8);
        b = (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);  // order-preserving map of the doubles
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o), n2 = __shfl_xor(nn, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        nn += n2;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
        if (nn) atomicAdd(&out[2], nn);
    }
}
template <class T>
__global__ void __launch_bounds__(256) scatter_rows_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                           const int64_t* __restrict__ perm, int64_t n, int width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t dst = perm[i];
    for (int k = 0; k < width; k++) out[dst * width + k] = in[i * width + k];
}
__global__ void __launch_bounds__(256) compose_perm_kernel(const int64_t* __restrict__ old_perm, const uint32_t* __restrict__ perm,
                                                           int64_t* __restrict__ new_perm, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    new_perm[i] = old_perm ? old_perm[perm[i]] : (int64_t)perm[i];
}

// ---- device-side removal of deleted particles (Kernel.remove_deleted, kernel.py:98-106) ----------------------------------
__global__ void __launch_bounds__(256) keep_flags_kernel(const int32_t* __restrict__ state, const int64_t* __restrict__ perm, int64_t n,
                                                         unsigned long long* __restrict__ keep_dev, uint32_t* __restrict__ keep_host) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned k = state[i] != PK_DELETE;
    keep_dev[i] = k;
    keep_host[perm ? perm[i] : i] = k;
}
template <class T>
__global__ void __launch_bounds__(256) compact_rows_kernel(const T* __restrict__ in, T* __restrict__ out, const unsigned long long* __restrict__ keep,
                                                           const unsigned long long* __restrict__ pos, int64_t n, int width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int64_t dst = (int64_t)pos[i];
    for (int k = 0; k < width; k++) out[dst * width + k] = in[i * width + k];
}
// new_perm[new device row] = new host row of the old host row this device row mapped to
__global__ void __launch_bounds__(256) compact_perm_kernel(const int64_t* __restrict__ perm, const unsigned long long* __restrict__ keep,
                                                           const unsigned long long* __restrict__ pos, const uint32_t* __restrict__ host_pos,
                                                           int64_t n, int64_t* __restrict__ new_perm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    new_perm[pos[i]] = (int64_t)host_pos[perm[i]];
}

// scatter one contiguous field level into its component slot of a packed (array-of-structs) group buffer
// Cell-packed pair copy of the staggered velocity (FastC::vp): for every element e = (zi, yi, xi) of a level the four values the 2-D
// C-grid kernels read for cell e -- U at e + dU0 / dU1, V at e + dV0 / dV1 (byte offsets into the level rings, pk_fast_cgrid.h) -- of
// level slot `o0`, then of level slot `o1`.  Elements in the last row / column are no cells (their offsets leave the level): zeros.
template <class T>
__global__ void __launch_bounds__(256) cg_pack_pairs_kernel(const char* __restrict__ U, const char* __restrict__ V, int64_t dU0, int64_t dU1,
                                                            int64_t dV0, int64_t dV1, int64_t cb, int64_t o0, int64_t o1, int64_t n, int32_t ny,
                                                            int32_t nx, T* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int xi = (int)(e % nx), yi = (int)((e / nx) % ny);
        T v[8];
        if (xi < nx - 1 && yi < ny - 1) {
            const int64_t b0 = e * cb + o0, b1 = e * cb + o1;
            v[0] = *reinterpret_cast<const T*>(U + dU0 + b0);
            v[1] = *reinterpret_cast<const T*>(U + dU1 + b0);
            v[2] = *reinterpret_cast<const T*>(V + dV0 + b0);
            v[3] = *reinterpret_cast<const T*>(V + dV1 + b0);
            v[4] = *reinterpret_cast<const T*>(U + dU0 + b1);
            v[5] = *reinterpret_cast<const T*>(U + dU1 + b1);
            v[6] = *reinterpret_cast<const T*>(V + dV0 + b1);
            v[7] = *reinterpret_cast<const T*>(V + dV1 + b1);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = (T)0;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) out[e * 8 + k] = v[k];
    }
}

template <class T>
__global__ void __launch_bounds__(256) interleave_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t n, int ncomp) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i * ncomp] = src[i];
}

// device-to-device float4 copy used as the measured HBM ceiling: 4 independent 16-byte loads in flight per lane, one block
// per 4 KiB-per-wave tile (no grid-stride tail), which is what reaches the ~6.3 TB/s of MI355X_MICROARCH.md
__global__ void __launch_bounds__(256) copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    if (base + 768 < n) {
        const float4 a = src[base], b = src[base + 256], c = src[base + 512], d = src[base + 768];
        dst[base] = a; dst[base + 256] = b; dst[base + 512] = c; dst[base + 768] = d;
    } else {
        for (int k = 0; k < 4; k++)
            if (base + 256 * k < n) dst[base + 256 * k] = src[base + 256 * k];
    }
}

}  // namespace pk

// pageable -> pinned staging: a ring of PK_STAGE_BUFFERS fixed-size pinned chunks (allocated once; pinning a whole 4 GB level costs
// ~1 s).  The host fills chunk k+1 (pk_host_stage.cpp: persistent thread pool, AVX2 interleave, non-temporal stores) while chunk k
// is on the wire; a third chunk keeps the DMA queue from draining while the fill of the next one is being handed to the pool.
using pkhost::parallel_interleave;
using pkhost::parallel_memcpy;
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
namespace pkapi {
// the next staging chunk, free of its previous DMA (blocks on that DMA's event; the wait is accounted in stage_wait_s)
int32_t stage_acquire(pk_ctx* ctx, int* out) {
    const int k = ctx->stage_next;
    ctx->stage_next = (k + 1) % PK_STAGE_BUFFERS;
    if (!ctx->stage[k]) {
        if (!ctx->stage_chunk) ctx->stage_chunk = PK_STAGE_CHUNK_BYTES;
        PK_HIP(ctx, hipHostMalloc(&ctx->stage[k], ctx->stage_chunk, hipHostMallocDefault));
        ctx->stage_bytes[k] = ctx->stage_chunk;
    } else {
        const double t0 = now_s();
        PK_HIP(ctx, hipEventSynchronize(ctx->stage_ev[k]));
        ctx->stage_wait_s += now_s() - t0;
    }
    *out = k;
    return 0;
}
int32_t stage_submit(pk_ctx* ctx, int k, void* dst, size_t bytes) {
    PK_HIP(ctx, hipMemcpyAsync(dst, ctx->stage[k], bytes, hipMemcpyHostToDevice, ctx->copy));
    PK_HIP(ctx, hipEventRecord(ctx->stage_ev[k], ctx->copy));
    ctx->stage_bytes_total += (double)bytes;
    return 0;
}
}  // namespace pkapi

// DGrid::cell_tab: one record per cell, written by the device functions the search would otherwise run on every cache miss
// (identical instruction sequences, so the values are the ones the per-miss computation produces)
__global__ void cell_table_kernel(const pk::DGrid g, double* tab) {
    using namespace pk;
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (int64_t)(g.ny - 1) * g.nx) return;
    const int xi = (int)(cell % g.nx);
    double* out = tab + cell * CT_STRIDE;
    if (xi >= g.nx - 1) {  // not a cell (last node of a row): never read
        for (int k = 0; k < CT_STRIDE; k++) out[k] = 0.0;
        return;
    }
    const double* r0 = g.node_tab + cell * 5;
    const double* r1 = r0 + (int64_t)g.nx * 5;
    // corner order c0=(yi,xi) c1=(yi,xi+1) c2=(yi+1,xi+1) c3=(yi+1,xi)
    const double* nodes[4] = {r0, r0 + 5, r1 + 5, r1};
    double lon[4], lat[4], cX[4], cY[4], cZ[4];
    for (int k = 0; k < 4; k++) { lon[k] = nodes[k][0]; lat[k] = nodes[k][1]; cX[k] = nodes[k][2]; cY[k] = nodes[k][3]; cZ[k] = nodes[k][4]; }
    double eu[3] = {0, 0, 0}, ev[3] = {0, 0, 0}, pu[4] = {0, 0, 0, 0}, pv[4] = {0, 0, 0, 0};
    unsigned long long box;
    if (g.spherical) {
        spherical_project_cell(cX, cY, cZ, eu, ev, pu, pv);
        box = pack_quantised_box(g, cX, cY, cZ, true);
    } else {
        box = pack_quantised_box(g, lon, lat, lat, false);
    }
    for (int k = 0; k < 4; k++) { out[2 * k] = lon[k]; out[2 * k + 1] = lat[k]; }
    for (int k = 0; k < 3; k++) { out[8 + k] = eu[k]; out[11 + k] = ev[k]; }
    for (int k = 0; k < 4; k++) { out[14 + k] = pu[k]; out[18 + k] = pv[k]; }
    out[22] = __longlong_as_double((long long)box);
    out[23] = 0.0;
}

// FastC::ct2 (pk_fast_cgrid.h): per cell, the record of cell_table_kernel re-expressed for the dedicated C-grid kernels -- the
// query-independent sub-expressions of bilinear_inverse in ITS evaluation order (so that finishing them with the query point gives
// the bits bilinear_inverse gives) and the corner longitudes after CGrid_Velocity's antimeridian unwrapping (cgrid_velocity).
__global__ void cell_table2_kernel(const pk::DGrid g, double* tab, int* wide) {
    using namespace pk;
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (int64_t)(g.ny - 1) * g.nx) return;
    const int xi = (int)(cell % g.nx);
    double* out = tab + cell * CT2_STRIDE;
    for (int k = 0; k < CT2_STRIDE; k++) out[k] = 0.0;
    if (xi >= g.nx - 1) return;  // not a cell (last node of a row): never read
    const double* ct = g.cell_tab + cell * CT_STRIDE;
    double px[4], py[4];
    for (int k = 0; k < 4; k++) { px[k] = ct[14 + k]; py[k] = ct[18 + k]; }
    const double a0 = px[0];
    const double a1 = -px[0] + px[1];
    const double a2 = -px[0] + px[3];
    const double a3 = ((px[0] + -px[1]) + px[2]) + -px[3];
    const double b0 = py[0];
    const double b1 = -py[0] + py[1];
    const double b2 = -py[0] + py[3];
    const double b3 = ((py[0] + -py[1]) + py[2]) + -py[3];
    const double aa = a3 * b2 - a2 * b3;
    const double bb0 = a3 * b0 - a0 * b3 + a1 * b2 - a2 * b1;  // bb = bb0 + xq * b3 - yq * a3
    const double cc0 = a1 * b0 - a0 * b1;                      // cc = cc0 + xq * b1 - yq * a1
    for (int k = 0; k < 6; k++) out[k] = ct[8 + k];  // eu, ev
    out[6] = a0; out[7] = a1; out[8] = a2; out[9] = a3; out[10] = b1; out[11] = b3;
    out[12] = 4 * aa;
    out[13] = bb0;
    out[14] = cc0;
    out[15] = ct[22];  // quantised hash box
    double lon[4];
    for (int k = 0; k < 4; k++) lon[k] = pymod360(ct[2 * k] + 180.0) - 180.0;  // _xinterpolators.py:230-233
    for (int k = 1; k < 4; k++)
        if (lon[k] - lon[0] > 180) lon[k] = lon[k] - 360;
    for (int k = 1; k < 4; k++)
        if (-lon[k] + lon[0] > 180) lon[k] = lon[k] + 360;
    for (int k = 0; k < 4; k++) { out[16 + k] = lon[k]; out[20 + k] = ct[2 * k + 1]; out[24 + k] = py[k]; }
    // FastC::near_edges (pk_fast_cgrid.h, cos_near): every cell spans less than 2^-8 rad of latitude, so the edge points of CGrid_Velocity's
    // geodetic distances lie within 2^-7 rad of any sample point found in the cell
    const double la_lo = fmin(fmin(ct[1], ct[3]), fmin(ct[5], ct[7])), la_hi = fmax(fmax(ct[1], ct[3]), fmax(ct[5], ct[7]));
    if (!((la_hi - la_lo) * DEG2RAD <= 0.00390625)) atomicOr(wide, 1);
}

// Cells on which the reference's bilinear inverse (index_search.py:122-177, restated in bilinear_inverse) is numerically unreliable:
// the quadratic branch is taken (|aa| >= 1e-12) although the cell is a parallelogram to rounding, so (-bb + sqrt(bb^2 - 4 aa cc)) /
// (2 aa) cancels completely and the point-in-cell test of such a cell accepts points that lie elsewhere.  (A flat mesh in metres has
// aa ~ 1e-9 of pure rounding noise on an exact parallelogram; in degrees or on the unit sphere the same noise is below the 1e-12
// switch to the linear branch.)  The reference then returns whichever listed face comes first in table order; neighbour-first
// probing assumes at most one face contains the point, so it must be off on such a mesh.  Found by seed 2985 of the fuzz generator.
__global__ void illconditioned_cell_kernel(const pk::DGrid g, int* flag) {
    using namespace pk;
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (int64_t)(g.ny - 1) * g.nx || (int)(cell % g.nx) >= g.nx - 1) return;
    const double* r0 = g.node_tab + cell * 5;
    const double* r1 = r0 + (int64_t)g.nx * 5;
    const double* nodes[4] = {r0, r0 + 5, r1 + 5, r1};
    double px[4], py[4];
    if (g.spherical) {
        double cX[4], cY[4], cZ[4], eu[3], ev[3];
        for (int k = 0; k < 4; k++) { cX[k] = nodes[k][2]; cY[k] = nodes[k][3]; cZ[k] = nodes[k][4]; }
        spherical_project_cell(cX, cY, cZ, eu, ev, px, py);
    } else {
        for (int k = 0; k < 4; k++) { px[k] = nodes[k][0]; py[k] = nodes[k][1]; }
    }
    const double a1 = -px[0] + px[1], a2 = -px[0] + px[3], a3 = ((px[0] + -px[1]) + px[2]) + -px[3];
    const double b1 = -py[0] + py[1], b2 = -py[0] + py[3], b3 = ((py[0] + -py[1]) + py[2]) + -py[3];
    const double aa = a3 * b2 - a2 * b3;
    const double scale = fmax(fmax(fabs(a1 * b2), fabs(a2 * b1)), fmax(fabs(a3 * b2), fabs(a2 * b3)));
    if (fabs(aa) >= 1e-12 && fabs(aa) < 1e-9 * scale) atomicOr(flag, 1);
}

// A mesh can cover a region twice without repeating a node: a zonal mesh that spans more than 360 degrees in columns that do not line
// up with the first ones, say.  Two cells then hold the same point and, as on a mesh with coincident nodes, only the reference's table
// order decides between them, which the neighbour probe does not ask.  Such a mesh has a node strictly inside a cell it is not a corner
// of -- strictly by the probe's own margin.  One thread per node walks the faces of the node's hash cell the way a query at the node
// does (curvilinear_search), with the node's own table coordinates.  Runs before the cell table and the directory exist.
__global__ void node_in_foreign_cell_kernel(const pk::DGrid g, int* flag) {
    using namespace pk;
    const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= (int64_t)g.ny * g.nx) return;
    const double* r = g.node_tab + node * 5;
    QPoint q;
    q.x = r[0];
    q.y = r[1];
    q.qX = g.spherical ? r[2] : r[0];
    q.qY = g.spherical ? r[3] : r[1];
    q.qZ = g.spherical ? r[4] : 0.0;
    if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.qX) && isfinite(q.qY) && isfinite(q.qZ))) return;  // masked
    const int nj = (int)(node / g.nx), ni = (int)(node % g.nx);
    const uint32_t code = morton_code(g, q);
    int64_t lo = 0, hi = g.h_nkeys;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (g.h_keys[mid] < code) lo = mid + 1; else hi = mid;
    }
    if (lo >= g.h_nkeys || g.h_keys[lo] != code) return;
    const int64_t s = g.h_starts[lo], c = g.h_counts[lo];
    const uint32_t ncx = (uint32_t)(g.nx - 1);
    const double m = 1e-9;  // curvilinear_search's margin
    for (int64_t k = 0; k < c; k++) {
        const uint32_t face = g.h_faces[s + k];
        const int j = (int)(face / ncx), i = (int)(face % ncx);
        if (j < 0 || j >= g.ny - 1 || i < 0 || i >= g.nx - 1) continue;
        if ((j == nj || j == nj - 1) && (i == ni || i == ni - 1)) continue;  // one of its own four cells
        double xs, et;
        if (point_in_cell(g, q, j, i, xs, et) && xs > m && xs < 1 - m && et > m && et < 1 - m) {
            atomicOr(flag, 1);
            return;
        }
    }
}

template <class T>
static int32_t upload(pk_ctx* ctx, HostGrid& g, const T* host, size_t n, const T** dev) {
    *dev = nullptr;
    if (!host || n == 0) return 0;
    void* p = nullptr;
    PK_HIP(ctx, hipMalloc(&p, n * sizeof(T)));
    g.allocs.push_back(p);
    PK_HIP(ctx, hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    *dev = (const T*)p;
    return 0;
}

namespace pkapi { static void free_particles(pk_ctx* ctx); }  // the particles section

// ---- context -------------------------------------------------------------------------------------------
extern "C" {

int32_t pk_abi_version(void) { return PK_ABI_VERSION; }

const char* pk_last_error(const pk_ctx* ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

int32_t pk_init(int32_t device, pk_ctx** out) {
    if (!out) return -2;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_init_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        return -1;
    }
    if (device < 0 || device >= ndev) {
        g_init_error = "device index out of range";
        return -2;
    }
    pk_ctx* ctx = new pk_ctx();
    ctx->device = device;
    if (const char* e = getenv("PK_SORT_HORIZONTAL")) ctx->sort_horizontal_major = atoi(e);
    if (const char* e = getenv("PK_NO_SPECIAL")) ctx->no_special = atoi(e);
    if (const char* e = getenv("PK_NO_CELL_CACHE")) ctx->no_cell_cache = atoi(e);
    if (const char* e = getenv("PK_NO_HASH_DIR")) ctx->no_hash_dir = atoi(e);
    if (const char* e = getenv("PK_NO_CELL_TABLE")) ctx->no_cell_table = atoi(e);
    if (const char* e = getenv("PK_NO_FAST")) ctx->no_fast = atoi(e);
    if (const char* e = getenv("PK_NO_FAST_CGRID")) ctx->no_fast_cgrid = atoi(e);
    if (const char* e = getenv("PK_NO_VELOCITY_PAIRS")) ctx->no_velocity_pairs = atoi(e);
    if (const char* e = getenv("PK_VELOCITY_PAIRS")) ctx->no_velocity_pairs = !atoi(e);
    ctx->no_block_cache = getenv("PK_NO_BLOCK_CACHE") != nullptr;
    *out = ctx;
    PK_HIP(ctx, hipSetDevice(device));
    PK_HIP(ctx, hipGetDeviceProperties(&ctx->prop, device));
    PK_HIP(ctx, hipStreamCreateWithFlags(&ctx->compute, hipStreamNonBlocking));
    PK_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking));
    PK_HIP(ctx, hipEventCreate(&ctx->ev0));
    PK_HIP(ctx, hipEventCreate(&ctx->ev1));
    PK_HIP(ctx, hipEventCreate(&ctx->ev2));
    PK_HIP(ctx, hipEventCreate(&ctx->ev_p0));
    PK_HIP(ctx, hipEventCreate(&ctx->ev_p1));
    for (int k = 0; k < PK_STAGE_BUFFERS; k++) PK_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_counters, sizeof(DCounters)));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_twe, sizeof(unsigned long long) * PK_MAX_TWE));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_twe_found, sizeof(unsigned long long) * TWE_FOUND_SLOTS));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_twe_hit, sizeof(unsigned int) * PK_MAX_TWE));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_summary, sizeof(unsigned long long) * (PK_NUM_STATE_CODES + 2)));
    PK_HIP(ctx, hipHostMalloc((void**)&ctx->h_counters, sizeof(DCounters), hipHostMallocDefault));
    PK_HIP(ctx, hipHostMalloc((void**)&ctx->h_summary, sizeof(unsigned long long) * (PK_NUM_STATE_CODES + 2), hipHostMallocDefault));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_clk, sizeof(unsigned long long) * 32));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_tstats, sizeof(unsigned long long) * 3));
    PK_HIP(ctx, hipHostMalloc((void**)&ctx->h_clk, sizeof(unsigned long long) * 32, hipHostMallocDefault));
    return 0;
}

int32_t pk_set_option(pk_ctx* ctx, const char* name, int32_t value) {
    if (!ctx || !name) return -2;
    const std::string n(name);
    if (n == "fast_path") ctx->no_fast = !value;
    else if (n == "fast_cgrid") ctx->no_fast_cgrid = !value;
    else if (n == "velocity_pairs") ctx->no_velocity_pairs = !value;
    else if (n == "clock_probe") ctx->clock_probe = value;
    else if (n == "special_programs") ctx->no_special = !value;
    else if (n == "cell_cache") ctx->no_cell_cache = !value;
    else if (n == "hash_directory") ctx->no_hash_dir = !value;
    else if (n == "cell_table") ctx->no_cell_table = !value;
    else if (n == "sort_horizontal") ctx->sort_horizontal_major = value;
    else if (n == "eval_points_f32") ctx->eval_points_f32 = value != 0;
    else if (n == "block_cache") {
        if (value < -1 || value > 2) return ctx->fail("pk_set_option: block_cache is -1 (planned), 0 (none), 1 (stage-pair block) or 2 (level-pair cache)");
        ctx->block_cache = value;
    }
    else if (n == "miss_lanes") {
        if (value < -1 || value > 64) return ctx->fail("pk_set_option: miss_lanes is -1 (planned), 0 (never) or the most missing lanes of a wavefront, up to 64");
        ctx->miss_lanes = value;
    }
    else if (n == "fast_grid") {
        if (value < 0) return ctx->fail("pk_set_option: fast_grid is 0 (planned) or the largest number of workgroups of the persistent A-grid launch");
        ctx->fast_grid = value;
    }
    else if (n == "unpack_chunk_values") {
        if (value < 0) return ctx->fail("pk_set_option: unpack_chunk_values is 0 (what fits a staging chunk) or the most values per staged chunk of a packed level");
        ctx->unpack_chunk_values = value == 0 ? 0 : std::max(16, value / 16 * 16);
    }
    else if (n == "unpack_timing") ctx->unpack_timing = value != 0;
    else return ctx->fail("pk_set_option: unknown option '" + n + "'");
    return 0;
}

int32_t pk_upload_stats(pk_ctx* ctx, double* out4) {
    if (!ctx || !out4) return -2;
    out4[0] = ctx->stage_fill_s;       // host threads filling pinned chunks
    out4[1] = ctx->stage_wait_s;       // blocked on the DMA that still reads the chunk to be refilled
    out4[2] = ctx->stage_bytes_total;  // bytes handed to the DMA engine through the staging ring
    out4[3] = (double)pkhost::copy_threads();
    return 0;
}

static void free_snapshots(pk_ctx* ctx) {
    for (auto& sn : ctx->snap) {
        if (sn.in_flight && sn.done) (void)hipEventSynchronize(sn.done);
        for (int k = 0; k < PK_NCOLS; k++) {
            if (sn.dev[k]) (void)hipFree(sn.dev[k]);
            if (sn.host[k]) (void)hipHostFree(sn.host[k]);
            sn.dev[k] = sn.host[k] = nullptr;
        }
        sn.capacity = 0;
        sn.in_flight = false;
    }
}

int32_t pk_destroy(pk_ctx* ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& g : ctx->grids)
        for (void* p : g.allocs) (void)hipFree(p);
    for (auto& f : ctx->fields) {
        if (f.dev_data && f.owns_data) (void)hipFree(f.dev_data);
        if (f.dev_time) (void)hipFree(f.dev_time);
    }
    free_particles(ctx);
    free_snapshots(ctx);
    for (auto& sn : ctx->snap) {
        if (sn.ready) (void)hipEventDestroy(sn.ready);
        if (sn.done) (void)hipEventDestroy(sn.done);
    }
    if (ctx->d_pack_tmp) (void)hipFree(ctx->d_pack_tmp);
    if (ctx->d_unpack_tmp) (void)hipFree(ctx->d_unpack_tmp);
    for (hipEvent_t e : ctx->unpack_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->unpack_ev_free) (void)hipEventDestroy(e);
    if (ctx->tab_a.d) (void)hipFree(ctx->tab_a.d);
    if (ctx->tab_c.d) (void)hipFree(ctx->tab_c.d);
    if (ctx->d_ct2) (void)hipFree(ctx->d_ct2);
    if (ctx->d_vp) (void)hipFree(ctx->d_vp);
    if (ctx->d_sigma) (void)hipFree(ctx->d_sigma);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->d_twe) (void)hipFree(ctx->d_twe);
    if (ctx->d_twe_found) (void)hipFree(ctx->d_twe_found);
    if (ctx->d_twe_hit) (void)hipFree(ctx->d_twe_hit);
    if (ctx->d_desc) (void)hipFree(ctx->d_desc);
    if (ctx->h_desc) (void)hipHostFree(ctx->h_desc);
    if (ctx->d_summary) (void)hipFree(ctx->d_summary);
    if (ctx->h_counters) (void)hipHostFree(ctx->h_counters);
    if (ctx->h_summary) (void)hipHostFree(ctx->h_summary);
    (void)pk_comm_destroy(ctx);
    neighbors_free(ctx->nbr);
    interact_free(ctx->inter);
    if (ctx->sel.d_flag) (void)hipFree(ctx->sel.d_flag);
    if (ctx->sel.d_offs) (void)hipFree(ctx->sel.d_offs);
    if (ctx->sel.d_tmp) (void)hipFree(ctx->sel.d_tmp);
    if (ctx->d_clk) (void)hipFree(ctx->d_clk);
    if (ctx->d_tstats) (void)hipFree(ctx->d_tstats);
    if (ctx->h_clk) (void)hipHostFree(ctx->h_clk);
    for (int k = 0; k < PK_STAGE_BUFFERS; k++) {
        if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
        if (ctx->stage_ev[k]) (void)hipEventDestroy(ctx->stage_ev[k]);
    }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->ev_p0) (void)hipEventDestroy(ctx->ev_p0);
    if (ctx->ev_p1) (void)hipEventDestroy(ctx->ev_p1);
    if (ctx->compute) (void)hipStreamDestroy(ctx->compute);
    if (ctx->copy) (void)hipStreamDestroy(ctx->copy);
    if (ctx->probe) (void)hipStreamDestroy(ctx->probe);
    if (ctx->ev_probe) (void)hipEventDestroy(ctx->ev_probe);
    delete ctx;
    return 0;
}

int32_t pk_get_device_info(pk_ctx* ctx, pk_device_info* out) {
    if (!ctx || !out) return -2;
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s", ctx->prop.name);
    snprintf(out->arch, sizeof(out->arch), "%s", ctx->prop.gcnArchName);
    out->compute_units = ctx->prop.multiProcessorCount;
    out->wavefront_size = ctx->prop.warpSize;
    out->lds_bytes_per_block = (int32_t)ctx->prop.sharedMemPerBlock;
    out->clock_khz = ctx->prop.clockRate;
    size_t fr = 0, tot = 0;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    PK_HIP(ctx, hipMemGetInfo(&fr, &tot));
    out->total_mem = (int64_t)tot;
    out->free_mem = (int64_t)fr;
    return 0;
}

// ---- grids ---------------------------------------------------------------------------------------------
int32_t pk_grid_create(pk_ctx* ctx, const pk_grid_desc* desc, int32_t* grid_id) {
    if (!ctx || !desc || !grid_id) return -2;
    if ((int)ctx->grids.size() >= PK_MAX_GRIDS) return ctx->fail("too many grids (PK_MAX_GRIDS)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->grids.emplace_back();
    HostGrid& g = ctx->grids.back();
    g.desc = *desc;
    DGrid& d = g.d;
    memset(&d, 0, sizeof(d));
    d.kind = desc->kind;
    d.spherical = desc->spherical;
    d.has_x = desc->has_x; d.has_y = desc->has_y; d.has_z = desc->has_z;
    d.nx = desc->nx; d.ny = desc->ny; d.nz = desc->nz;
    d.xdim = desc->xdim; d.ydim = desc->ydim; d.zdim = desc->zdim;
    d.off_x = desc->off_x; d.off_y = desc->off_y; d.off_z = desc->off_z;
    d.lon_f32 = desc->lon_f32; d.lat_f32 = desc->lat_f32; d.depth_f32 = desc->depth_f32;
    d.deg2m = desc->deg2m;
    if (desc->depth && desc->nz > 0) { d.zfirst = desc->depth[0]; d.zlast = desc->depth[desc->nz - 1]; }
    if (desc->kind == 0) {
        if (desc->lat && desc->ny > 0) { d.yfirst = desc->lat[0]; d.ylast = desc->lat[desc->ny - 1]; }
        if (desc->lon && desc->nx > 0) { d.xfirst = desc->lon[0]; d.xlast = desc->lon[desc->nx - 1]; }
    }
    const size_t nlon = desc->kind == 1 ? (size_t)desc->ny * desc->nx : (size_t)desc->nx;
    const size_t nlat = desc->kind == 1 ? (size_t)desc->ny * desc->nx : (size_t)desc->ny;
    int32_t rc;
    if (desc->kind == 1) {
        // array-of-structs node table {lon, lat, X, Y, Z}: one or two cache lines per cell row instead of five planes
        if (desc->spherical && !desc->node_xyz) return ctx->fail("spherical curvilinear grid needs node_xyz (unit-sphere node coordinates)");
        std::vector<double> tab(nlon * 5);
        for (size_t k = 0; k < nlon; k++) {
            tab[5 * k + 0] = desc->lon[k];
            tab[5 * k + 1] = desc->lat[k];
            tab[5 * k + 2] = desc->spherical ? desc->node_xyz[k] : 0.0;
            tab[5 * k + 3] = desc->spherical ? desc->node_xyz[nlon + k] : 0.0;
            tab[5 * k + 4] = desc->spherical ? desc->node_xyz[2 * nlon + k] : 0.0;
        }
        if ((rc = upload(ctx, g, (const double*)tab.data(), tab.size(), &d.node_tab))) return rc;
    } else {
        if ((rc = upload(ctx, g, desc->lon, nlon, &d.lon))) return rc;
        if ((rc = upload(ctx, g, desc->lat, nlat, &d.lat))) return rc;
    }
    if ((rc = upload(ctx, g, desc->depth, (size_t)desc->nz, &d.depth))) return rc;
    if (desc->kind == 1) {
        if (desc->h_keys && desc->h_nkeys > 0) {  // table built by the caller (e.g. the reference's own SpatialHash)
            if ((rc = upload(ctx, g, desc->h_keys, (size_t)desc->h_nkeys, &d.h_keys))) return rc;
            if ((rc = upload(ctx, g, desc->h_starts, (size_t)desc->h_nkeys, &d.h_starts))) return rc;
            if ((rc = upload(ctx, g, desc->h_counts, (size_t)desc->h_nkeys, &d.h_counts))) return rc;
            if ((rc = upload(ctx, g, desc->h_faces, (size_t)desc->h_nentries, &d.h_faces))) return rc;
            d.h_nkeys = desc->h_nkeys;
            g.h_nentries = desc->h_nentries;
            d.h_bitwidth = desc->h_bitwidth;
            for (int k = 0; k < 6; k++) d.h_bbox[k] = desc->h_bbox[k];
        } else {  // built here, on the device, from the node table
            HashBuildResult hb;
            std::string msg;
            hipError_t e = build_spatial_hash(ctx->compute, d.node_tab, desc->ny, desc->nx, desc->spherical, &hb, &msg);
            if (e != hipSuccess) return ctx->fail("spatial hash build: " + msg);
            g.allocs.push_back(hb.keys); g.allocs.push_back(hb.starts); g.allocs.push_back(hb.counts); g.allocs.push_back(hb.faces);
            d.h_keys = hb.keys; d.h_starts = hb.starts; d.h_counts = hb.counts; d.h_faces = hb.faces;
            d.h_nkeys = hb.nkeys;
            g.h_nentries = hb.nentries;
            d.h_bitwidth = hb.bitwidth;
            for (int k = 0; k < 6; k++) d.h_bbox[k] = hb.bbox[k];
        }
        for (int k = 0; k < 3; k++) {  // reciprocal widths of the hash grid for quantize() (pk_device.h: div_by_recip)
            const double w = d.h_bbox[2 * k + 1] - d.h_bbox[2 * k], r = 1.0 / w;
            d.h_rinv[k] = (w >= 1e-100 && w <= 1e100 && std::isfinite(r)) ? r : 0.0;
        }
        // neighbour-first probing (pk_device.h: curvilinear_search) is exact only where cells cannot overlap
        int probe = desc->neighbour_probe;
        if (const char* e = getenv("PK_NEIGHBOUR_PROBE")) probe = atoi(e);
        if (probe == 0) {
            bool coincident = true;
            std::string msg;
            if (mesh_has_coincident_nodes(ctx->compute, d.node_tab, desc->ny, desc->nx, desc->spherical, d.h_bbox, &coincident, &msg) != hipSuccess)
                return ctx->fail("coincident-node scan: " + msg);
            d.walk_ok = coincident ? 0 : 1;
            if (d.walk_ok) {  // ... and only where the point-in-cell test itself is reliable on every cell
                int* d_flag = nullptr;
                int h_flag = 0;
                PK_HIP(ctx, hipMalloc((void**)&d_flag, sizeof(int)));
                PK_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), ctx->compute));
                const int64_t ncell = (int64_t)(desc->ny - 1) * desc->nx;
                if (ncell > 0) hipLaunchKernelGGL(illconditioned_cell_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, ctx->compute, d, d_flag);
                // ... and where no node lies inside a cell it is not a corner of (a mesh that overlaps itself without coincident nodes)
                const int64_t nnode = (int64_t)desc->ny * desc->nx;
                if (desc->ny >= 2 && desc->nx >= 2 && d.h_nkeys > 0)
                    hipLaunchKernelGGL(node_in_foreign_cell_kernel, dim3((unsigned)((nnode + 255) / 256)), dim3(256), 0, ctx->compute, d, d_flag);
                PK_HIP(ctx, hipGetLastError());
                PK_HIP(ctx, hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->compute));
                PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
                (void)hipFree(d_flag);
                if (h_flag) d.walk_ok = 0;
            }
        } else {
            d.walk_ok = probe > 0 ? 1 : 0;
        }
        if (!ctx->no_cell_table && (int64_t)desc->ny * desc->nx < INT32_MAX) {
            // optional: a grid that does not get its table (allocation failure on a crowded device) searches from node_tab
            const int64_t ncell = (int64_t)(desc->ny - 1) * desc->nx;
            double* ct = nullptr;
            const double t0 = now_s();
            if (ncell > 0 && hipMalloc((void**)&ct, (size_t)ncell * CT_STRIDE * sizeof(double)) == hipSuccess) {
                g.allocs.push_back(ct);
                const double t1 = now_s();
                hipLaunchKernelGGL(cell_table_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, ctx->compute, d, ct);
                PK_HIP(ctx, hipGetLastError());
                PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
                d.cell_tab = ct;
                if (pk::print_occupancy())
                    fprintf(stderr, "[pk] cell table: %lld cells, %.2f GB, hipMalloc %.3f s, build %.3f s\n", (long long)ncell,
                            (double)ncell * CT_STRIDE * 8 / 1e9, t1 - t0, now_s() - t1);
            } else {
                (void)hipGetLastError();
            }
        }
        if (!ctx->no_hash_dir) {
            int32_t* dir = nullptr;
            int32_t shift = 0;
            std::string msg;
            if (build_hash_directory(ctx->compute, d.h_keys, d.h_nkeys, &dir, &shift, &msg) != hipSuccess) return ctx->fail(msg);
            if (dir) g.allocs.push_back(dir);
            d.h_dir = dir;
            d.h_dir_shift = shift;
        }
    }
    *grid_id = (int32_t)ctx->grids.size() - 1;
    return 0;
}

// UxGrid (uxgrid.py:16-135): a DGrid of kind PK_UX_KIND (pk_ux.h) with the per-face records of the point-in-triangle test
int32_t pk_ugrid_create(pk_ctx* ctx, const pk_ugrid_desc* desc, int32_t* grid_id) {
    if (!ctx || !desc || !grid_id) return -2;
    if ((int)ctx->grids.size() >= PK_MAX_GRIDS) return ctx->fail("too many grids (PK_MAX_GRIDS)");
    if (desc->n_face < 1 || desc->n_node < 3 || desc->nz < 2) return ctx->fail("pk_ugrid_create: n_face >= 1, n_node >= 3 and nz >= 2 (zf levels) required");
    if (!desc->node_lon || !desc->node_lat || !desc->face_nodes || !desc->zf) return ctx->fail("pk_ugrid_create: node_lon, node_lat, face_nodes and zf are required");
    if (desc->spherical && !desc->node_xyz) return ctx->fail("pk_ugrid_create: a spherical mesh needs node_xyz");
    if (!desc->h_keys || !desc->h_starts || !desc->h_counts || !desc->h_faces || desc->h_nkeys < 1)
        return ctx->fail("pk_ugrid_create: the hash table (h_keys / h_starts / h_counts / h_faces) is required");
    const int64_t nf = desc->n_face, nn = desc->n_node;
    for (int64_t k = 0; k < 3 * nf; k++)
        if (desc->face_nodes[k] < 0 || desc->face_nodes[k] >= nn) return ctx->fail("pk_ugrid_create: face_nodes refers to a node that does not exist");
    for (int64_t k = 0; k < desc->h_nentries; k++)
        if (desc->h_faces[k] >= (uint32_t)nf) return ctx->fail("pk_ugrid_create: h_faces refers to a face that does not exist");
    for (int64_t k = 0; k < desc->h_nkeys; k++)
        if (desc->h_starts[k] < 0 || desc->h_counts[k] < 0 || desc->h_starts[k] + desc->h_counts[k] > desc->h_nentries)
            return ctx->fail("pk_ugrid_create: h_starts / h_counts exceed h_nentries");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->grids.emplace_back();
    HostGrid& g = ctx->grids.back();
    memset(&g.desc, 0, sizeof(g.desc));
    g.desc.kind = PK_UX_KIND;
    g.desc.spherical = desc->spherical;
    g.desc.nx = desc->n_face;  // (host-side bookkeeping: pk_field_create checks the lateral extent of a field against these)
    g.desc.ny = desc->n_node;
    DGrid& d = g.d;
    memset(&d, 0, sizeof(d));
    d.kind = PK_UX_KIND;
    d.spherical = desc->spherical;
    d.has_x = 1; d.has_y = 0; d.has_z = 1;
    d.nx = desc->n_face; d.ny = 1; d.nz = desc->nz;
    d.xdim = desc->n_face; d.ydim = 0; d.zdim = desc->nz;
    d.deg2m = desc->deg2m;
    d.zfirst = desc->zf[0];
    d.zlast = desc->zf[desc->nz - 1];
    int32_t rc;
    if ((rc = upload(ctx, g, desc->zf, (size_t)desc->nz, &d.depth))) return rc;
    // per-face records (pk_ux.h), the query-independent part of uxgrid_point_in_cell in the reference's operation order
    const int stride = desc->spherical ? UXF_SPH : UXF_FLAT;
    std::vector<double> rec((size_t)nf * stride, 0.0);
    for (int64_t f = 0; f < nf; f++) {
        double* r = rec.data() + f * stride;
        const int32_t* ids = desc->face_nodes + 3 * f;
        if (desc->spherical) {
            double V[3][3];
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) V[k][c] = desc->node_xyz[c * nn + ids[k]];
            const double r1[3] = {V[1][0] - V[0][0], V[1][1] - V[0][1], V[1][2] - V[0][2]};
            const double r2[3] = {V[2][0] - V[0][0], V[2][1] - V[0][1], V[2][2] - V[0][2]};
            const double c0 = r1[1] * r2[2] - r1[2] * r2[1], c1 = r1[2] * r2[0] - r1[0] * r2[2], c2 = r1[0] * r2[1] - r1[1] * r2[0];
            double nrm = std::sqrt((c0 * c0 + c1 * c1) + c2 * c2);  // np.linalg.norm (index_search.py:341-343)
            const double area = 0.5 * nrm;                             // _triangle_area(v0, v1, v2): the same cross product
            if (nrm == 0.0) nrm = 1.0;
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) r[3 * k + c] = V[k][c];
            r[9] = c0 / nrm;
            r[10] = c1 / nrm;
            r[11] = c2 / nrm;
            r[12] = area;
            memcpy(r + 13, ids, 3 * sizeof(int32_t));
        } else {
            for (int k = 0; k < 3; k++) {
                r[2 * k] = desc->node_lon[ids[k]];
                r[2 * k + 1] = desc->node_lat[ids[k]];
            }
            memcpy(r + 6, ids, 3 * sizeof(int32_t));
        }
    }
    if ((rc = upload(ctx, g, (const double*)rec.data(), rec.size(), &d.cell_tab))) return rc;
    if ((rc = upload(ctx, g, desc->h_keys, (size_t)desc->h_nkeys, &d.h_keys))) return rc;
    if ((rc = upload(ctx, g, desc->h_starts, (size_t)desc->h_nkeys, &d.h_starts))) return rc;
    if ((rc = upload(ctx, g, desc->h_counts, (size_t)desc->h_nkeys, &d.h_counts))) return rc;
    if ((rc = upload(ctx, g, desc->h_faces, (size_t)desc->h_nentries, &d.h_faces))) return rc;
    d.h_nkeys = desc->h_nkeys;
    g.h_nentries = desc->h_nentries;
    d.h_bitwidth = desc->h_bitwidth;
    for (int k = 0; k < 6; k++) d.h_bbox[k] = desc->h_bbox[k];
    *grid_id = (int32_t)ctx->grids.size() - 1;
    return 0;
}

int32_t pk_grid_hash_info(pk_ctx* ctx, int32_t grid, pk_hash_info* out) {
    if (!ctx || !out) return -2;
    if (grid < 0 || grid >= (int)ctx->grids.size()) return ctx->fail("unknown grid");
    const HostGrid& g = ctx->grids[grid];
    out->nkeys = g.d.h_nkeys;
    out->nentries = g.h_nentries;
    out->bitwidth = g.d.h_bitwidth;
    out->neighbour_probe = g.d.walk_ok;
    for (int k = 0; k < 6; k++) out->bbox[k] = g.d.h_bbox[k];
    return 0;
}

int32_t pk_grid_hash_download(pk_ctx* ctx, int32_t grid, uint32_t* keys, int64_t* starts, int64_t* counts, uint32_t* faces) {
    if (!ctx) return -2;
    if (grid < 0 || grid >= (int)ctx->grids.size()) return ctx->fail("unknown grid");
    const HostGrid& g = ctx->grids[grid];
    if (g.d.kind != 1 || g.d.h_nkeys <= 0) return ctx->fail("grid has no spatial-hash table");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    const size_t nk = (size_t)g.d.h_nkeys, ne = (size_t)g.h_nentries;
    if (keys) PK_HIP(ctx, hipMemcpy(keys, g.d.h_keys, nk * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (starts) PK_HIP(ctx, hipMemcpy(starts, g.d.h_starts, nk * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (counts) PK_HIP(ctx, hipMemcpy(counts, g.d.h_counts, nk * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (faces) PK_HIP(ctx, hipMemcpy(faces, g.d.h_faces, ne * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

// ---- fields --------------------------------------------------------------------------------------------
int32_t pk_field_create(pk_ctx* ctx, const pk_field_desc* desc, int32_t* field_id) {
    if (!ctx || !desc || !field_id) return -2;
    if ((int)ctx->fields.size() >= PK_MAX_FIELDS) return ctx->fail("too many fields (PK_MAX_FIELDS)");
    if (desc->grid < 0 || desc->grid >= (int)ctx->grids.size()) return ctx->fail("field refers to an unknown grid");
    if (desc->dtype != PK_F32 && desc->dtype != PK_F64) return ctx->fail("field dtype must be PK_F32 or PK_F64");
    if (desc->nt < 1 || desc->nz < 1 || desc->ny < 1 || desc->nx < 1) return ctx->fail("field extents must be >= 1");
    if (ctx->grids[desc->grid].d.kind == PK_UX_KIND) {  // (pk_ux.h: ux_interp reads float64 levels at face / node ids and zi, zi + 1)
        const HostGrid& g = ctx->grids[desc->grid];
        const int code = desc->is_const;
        if (code < 5 || code > 8) return ctx->fail("a field on a UxGrid needs a Ux* interpolator (is_const 5-8)");
        if (!desc->has_x || !desc->has_z || desc->has_y) return ctx->fail("a field on a UxGrid has the axes Z and X (= FACE | NODE), not Y");
        if (desc->dtype != PK_F64) return ctx->fail("fields on a UxGrid must be float64");
        const bool node = code >= 7, zf = code == 6 || code == 8;
        if (desc->ny != 1 || desc->nx != (node ? g.desc.ny : g.desc.nx)) return ctx->fail("a field on a UxGrid has ny = 1 and nx = n_face (face) or n_node (node)");
        if (desc->nz != (zf ? g.d.nz : g.d.nz - 1)) return ctx->fail("a field on a UxGrid has nz = number of zf levels (zf) or one less (zc)");
    }
    PK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->fields.emplace_back();
    HostField& f = ctx->fields.back();
    f.desc = *desc;
    const size_t esz = desc->dtype == PK_F64 ? 8 : 4;
    const size_t level_elems = (size_t)desc->nz * desc->ny * desc->nx;
    f.level_bytes = level_elems * esz;
    int nslots = desc->nslots;
    if (nslots <= 0 || nslots >= desc->nt) nslots = desc->nt;
    if (nslots < desc->nt && nslots < 2) nslots = 2;
    f.slot_level.assign(nslots, -1);
    f.slot_pending.assign(nslots, -1);
    f.slot_gen.assign(nslots, 0);
    int ncomp = 1, comp = 0;
    if (desc->pack_leader >= 0) {  // follower: share the leader's interleaved buffer
        if (desc->pack_leader >= (int)ctx->fields.size() - 1) return ctx->fail("pack_leader must be an existing field");
        HostField& L = ctx->fields[desc->pack_leader];
        if (L.d.ncomp <= 1 || L.pack_used >= L.d.ncomp) return ctx->fail("pack leader has no free component");
        if (L.desc.dtype != desc->dtype || L.desc.nt != desc->nt || L.desc.nz != desc->nz || L.desc.ny != desc->ny ||
            L.desc.nx != desc->nx || L.d.nslots != nslots)
            return ctx->fail("packed fields must share dtype, extents and nslots");
        ncomp = L.d.ncomp;
        comp = L.pack_used++;
        f.dev_data = L.dev_data;
        f.owns_data = false;
    } else {
        ncomp = desc->pack_count > 1 ? desc->pack_count : 1;
        PK_HIP(ctx, hipMalloc(&f.dev_data, f.level_bytes * nslots * ncomp));
        PK_HIP(ctx, hipMemset(f.dev_data, 0, f.level_bytes * nslots * ncomp));  // never expose NaN garbage (weight-0 reads)
    }
    if (nslots < desc->nt) {
        // a streamed field: pin the staging chunks now (at creation, not inside the first run), sized for the largest streamed level --
        // at most 3 x 256 MiB (pinning that costs ~0.2 s), a few MB for a small field: locked memory is scarce on shared nodes
        const size_t mib = (size_t)1 << 20;
        const size_t want_raw = f.level_bytes * (size_t)(desc->pack_count > 1 ? desc->pack_count : 1);
        size_t want = std::min(PK_STAGE_CHUNK_BYTES, (want_raw + mib - 1) / mib * mib);
        if (want > ctx->stage_chunk) {
            PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
            for (int k = 0; k < PK_STAGE_BUFFERS; k++)
                if (ctx->stage[k]) { (void)hipHostFree(ctx->stage[k]); ctx->stage[k] = nullptr; }
            ctx->stage_chunk = want;
        }
        for (int k = 0; k < PK_STAGE_BUFFERS; k++)
            if (!ctx->stage[k]) {
                hipError_t e = hipHostMalloc(&ctx->stage[k], ctx->stage_chunk, hipHostMallocDefault);
                while (e != hipSuccess && k == 0 && ctx->stage_chunk > 16 * mib) {  // pinning failed: smaller chunks (more DMA calls, same result)
                    (void)hipGetLastError();
                    ctx->stage_chunk /= 2;
                    e = hipHostMalloc(&ctx->stage[k], ctx->stage_chunk, hipHostMallocDefault);
                }
                if (e != hipSuccess) return ctx->fail("hipHostMalloc of a staging chunk", e);
                ctx->stage_bytes[k] = ctx->stage_chunk;
                PK_HIP(ctx, hipEventRecord(ctx->stage_ev[k], ctx->copy));
            }
    }
    f.time.assign(desc->nt, 0.0);
    if (desc->time) std::copy(desc->time, desc->time + desc->nt, f.time.begin());
    PK_HIP(ctx, hipMalloc((void**)&f.dev_time, sizeof(double) * desc->nt));
    PK_HIP(ctx, hipMemcpy(f.dev_time, f.time.data(), sizeof(double) * desc->nt, hipMemcpyHostToDevice));
    DField& d = f.d;
    memset(&d, 0, sizeof(d));
    d.grid = desc->grid;
    d.dtype = desc->dtype;
    d.nt = desc->nt; d.nz = desc->nz; d.ny = desc->ny; d.nx = desc->nx;
    d.has_time_interval = desc->has_time_interval && desc->nt > 1;
    d.is_const = desc->is_const;
    d.nslots = nslots;
    d.ncomp = ncomp;
    d.comp = comp;
    d.st_t = desc->has_t ? (int64_t)level_elems : 0;
    d.st_z = desc->has_z ? (int64_t)desc->ny * desc->nx : 0;
    d.st_y = desc->has_y ? (int64_t)desc->nx : 0;
    d.st_x = desc->has_x ? 1 : 0;
    d.data = f.dev_data;
    d.time = f.dev_time;
    d.tlen = f.time.back() - f.time.front();
    d.tfirst = f.time.front();
    d.tlast = f.time.back();
    if (level_elems >= (1ull << 31)) return ctx->fail("a field time level must hold < 2^31 elements");
    *field_id = (int32_t)ctx->fields.size() - 1;
    return 0;
}

int32_t pk_field_upload_level(pk_ctx* ctx, int32_t field_id, int32_t level, const void* host_data, int32_t async) {
    if (!ctx || !host_data) return -2;
    if (field_id < 0 || field_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    HostField& f = ctx->fields[field_id];
    if (level < 0 || level >= f.desc.nt) return ctx->fail("time level out of range");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int slot = level % f.d.nslots;
    const int ncomp = f.d.ncomp;
    const size_t esz = f.desc.dtype == PK_F64 ? 8 : 4;
    const int64_t level_elems = (int64_t)(f.level_bytes / esz);
    char* dst = (char*)f.dev_data + ((size_t)slot * f.level_bytes * ncomp) + (size_t)f.d.comp * esz;
    char* h2d_dst = dst;
    if (ncomp > 1) {  // packed group: land in a device staging buffer, then interleave on the copy stream
        if (ctx->pack_tmp_bytes < f.level_bytes) {
            PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
            if (ctx->d_pack_tmp) PK_HIP(ctx, hipFree(ctx->d_pack_tmp));
            PK_HIP(ctx, hipMalloc(&ctx->d_pack_tmp, f.level_bytes));
            ctx->pack_tmp_bytes = f.level_bytes;
        }
        h2d_dst = (char*)ctx->d_pack_tmp;
    }
    auto interleave = [&]() -> int32_t {
        if (ncomp <= 1) return 0;
        const unsigned grid = (unsigned)std::min<int64_t>((level_elems + 255) / 256, 256 * 32);
        if (esz == 8) hipLaunchKernelGGL((interleave_kernel<double>), dim3(grid), dim3(256), 0, ctx->copy, (const double*)ctx->d_pack_tmp, (double*)dst, level_elems, ncomp);
        else hipLaunchKernelGGL((interleave_kernel<float>), dim3(grid), dim3(256), 0, ctx->copy, (const float*)ctx->d_pack_tmp, (float*)dst, level_elems, ncomp);
        PK_HIP(ctx, hipGetLastError());
        return 0;
    };
    if (!async) {
        PK_HIP(ctx, hipMemcpyAsync(h2d_dst, host_data, f.level_bytes, hipMemcpyHostToDevice, ctx->copy));
        if (int32_t rc = interleave()) return rc;
        PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
    } else {
        // pageable NumPy memory cannot be DMA'd asynchronously: bounce it through the ring of pinned chunks
        const size_t chunk = ctx->stage_chunk ? ctx->stage_chunk : PK_STAGE_CHUNK_BYTES;
        for (size_t off = 0; off < f.level_bytes; off += chunk) {
            const size_t len = std::min(chunk, f.level_bytes - off);
            int k;
            if (int32_t rc = stage_acquire(ctx, &k)) return rc;
            const double t0 = now_s();
            parallel_memcpy(ctx->stage[k], (const char*)host_data + off, len);
            ctx->stage_fill_s += now_s() - t0;
            if (int32_t rc = stage_submit(ctx, k, h2d_dst + off, len)) return rc;
        }
        if (int32_t rc = interleave()) return rc;
    }
    f.slot_gen[slot] = ++ctx->upload_counter;
    if (async) {  // usable only after pk_field_sync(); the level that lived in this slot is gone as of now
        f.slot_level[slot] = -1;
        f.slot_pending[slot] = level;
        ctx->copy_pending = true;
    } else {
        f.slot_level[slot] = level;
        f.slot_pending[slot] = -1;
    }
    return 0;
}

int32_t pk_field_upload_group_level(pk_ctx* ctx, int32_t leader_id, int32_t level, const void* const* host_data, int32_t ncomp_given,
                                    int32_t async) {
    if (!ctx || !host_data) return -2;
    if (leader_id < 0 || leader_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    HostField& L = ctx->fields[leader_id];
    const int ncomp = L.d.ncomp;
    if (ncomp <= 1 || !L.owns_data) return ctx->fail("pk_field_upload_group_level: the field does not lead a packed group");
    if (ncomp_given != ncomp || L.pack_used != ncomp) return ctx->fail("pk_field_upload_group_level: one host level per component of the complete group is required");
    if (ncomp > 8) return ctx->fail("pk_field_upload_group_level: at most 8 components");
    if (level < 0 || level >= L.desc.nt) return ctx->fail("time level out of range");
    for (int k = 0; k < ncomp; k++)
        if (!host_data[k]) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int slot = level % L.d.nslots;
    const size_t esz = L.desc.dtype == PK_F64 ? 8 : 4;
    const size_t level_elems = L.level_bytes / esz;
    char* dst = (char*)L.dev_data + (size_t)slot * L.level_bytes * ncomp;
    const size_t chunk_elems = (ctx->stage_chunk ? ctx->stage_chunk : PK_STAGE_CHUNK_BYTES) / (esz * ncomp);
    for (size_t off = 0; off < level_elems; off += chunk_elems) {
        const size_t len = std::min(chunk_elems, level_elems - off);
        int k;
        if (int32_t rc = stage_acquire(ctx, &k)) return rc;
        const double t0 = now_s();
        if (esz == 8) {
            const double* src[8];
            for (int c = 0; c < ncomp; c++) src[c] = (const double*)host_data[c] + off;
            parallel_interleave((double*)ctx->stage[k], src, ncomp, len);
        } else {
            const float* src[8];
            for (int c = 0; c < ncomp; c++) src[c] = (const float*)host_data[c] + off;
            parallel_interleave((float*)ctx->stage[k], src, ncomp, len);
        }
        ctx->stage_fill_s += now_s() - t0;
        if (int32_t rc = stage_submit(ctx, k, dst + off * esz * ncomp, len * esz * ncomp)) return rc;
    }
    if (!async) PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
    for (size_t f = 0; f < ctx->fields.size(); f++) {  // the leader and its followers change slot state together
        HostField& F = ctx->fields[f];
        if ((int)f != leader_id && F.desc.pack_leader != leader_id) continue;
        F.slot_gen[slot] = ++ctx->upload_counter;
        F.slot_level[slot] = async ? -1 : level;
        F.slot_pending[slot] = async ? level : -1;
    }
    if (async) ctx->copy_pending = true;
    return 0;
}

int32_t pk_field_sync(pk_ctx* ctx) {
    if (!ctx) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
    for (auto& f : ctx->fields)
        for (size_t k = 0; k < f.slot_pending.size(); k++)
            if (f.slot_pending[k] >= 0) {
                f.slot_level[k] = f.slot_pending[k];
                f.slot_pending[k] = -1;
            }
    ctx->copy_pending = false;
    return 0;
}

int32_t pk_field_evict_outside(pk_ctx* ctx, int32_t field_id, int32_t lo_level, int32_t hi_level) {
    if (!ctx) return -2;
    if (field_id < 0 || field_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    if (ctx->in_flight) return ctx->fail("pk_field_evict_outside: a launch is in flight");
    HostField& f = ctx->fields[field_id];
    if (f.d.nslots >= f.desc.nt) return 0;  // all levels resident: nothing to evict
    for (size_t k = 0; k < f.slot_level.size(); k++)
        if (f.slot_level[k] >= 0 && (f.slot_level[k] < lo_level || f.slot_level[k] > hi_level)) f.slot_level[k] = -1;
    return 0;
}

int32_t pk_field_slots(pk_ctx* ctx, int32_t field_id, int32_t* levels, int32_t* nslots) {
    if (!ctx) return -2;
    if (field_id < 0 || field_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    HostField& f = ctx->fields[field_id];
    if (nslots) *nslots = f.d.nslots;
    if (levels)
        for (int k = 0; k < f.d.nslots; k++) levels[k] = f.slot_level[k];
    return 0;
}

}  // extern "C" (helpers with C++ linkage follow)

namespace pkapi {

// ---- particles -----------------------------------------------------------------------------------------
static size_t spatial_size(const pk_ctx* ctx) { return ctx->host.spatial_dtype == PK_F32 ? 4 : 8; }
std::vector<ColRef> particle_columns(pk_ctx* ctx) {
    const auto h = column_pointers(ctx->host), d = column_pointers(ctx->dev), a = column_pointers(ctx->alt);
    std::vector<ColRef> cols;
    for (int k = 0; k < PK_COL_EXTRA_FIRST; k++) {
        const ColInfo& c = PK_COL_INFO[k];
        cols.push_back({h[k], d[k], a[k], c.elem == COL_SPATIAL ? spatial_size(ctx) : (size_t)c.elem, c.per_grid ? ctx->host.ngrids : 1,
                        (c.bit & PK_LAUNCH_MASK) != 0});
    }
    for (int k = PK_COL_EXTRA_FIRST; k < PK_NCOLS; k++)
        cols.push_back({h[k], d[k], a[k], (size_t)(ctx->dev.extra_f32[k - PK_COL_EXTRA_FIRST] ? 4 : 8), 1, false});
    cols.push_back({nullptr, ctx->dev.iter, ctx->alt.iter, 4, 1, true});  // device only (index PK_NCOLS: beyond the column masks of the ABI)
    return cols;
}

// Allocate the columns of one set (`dev` or `alt`) for `cap` rows: the optional ones where the bound host descriptor has them (pk_particles_bind
// and pk_particles_compact keep `dev` and the host descriptor alike in that).  What was allocated before a failure stays in `set` for free_particles.
static int32_t alloc_column_set(pk_ctx* ctx, DParticles& set, int64_t cap) {
    const std::vector<ColRef> cols = particle_columns(ctx);
    void* p[PK_NCOLS + 1] = {};  // (the last one: `iter`)
    hipError_t e = hipSuccess;
    for (int k = 0; k <= PK_NCOLS && e == hipSuccess; k++) {
        const bool present = k == PK_NCOLS || (k >= PK_COL_EXTRA_FIRST ? k - PK_COL_EXTRA_FIRST < ctx->host.n_extra : !PK_COL_INFO[k].optional || cols[k].h);
        if (present) e = hipMalloc(&p[k], (size_t)cap * cols[k].elem * cols[k].width);
    }
    set_column_pointers(set, p, PK_NCOLS);
    set.iter = static_cast<int32_t*>(p[PK_NCOLS]);
    return e == hipSuccess ? 0 : ctx->fail("hipMalloc of a particle column", e);
}

static void free_particles(pk_ctx* ctx) {
    if (ctx->d_chk) (void)hipFree(ctx->d_chk);
    ctx->d_chk = nullptr;
    ctx->chk_bytes = 0;
    ctx->chk_valid = false;
    ctx->rerun_valid = false;
    for (const ColRef& c : particle_columns(ctx)) {
        if (c.d) (void)hipFree(c.d);
        if (c.a) (void)hipFree(c.a);
    }
    void* sort_buffers[] = {ctx->d_perm, ctx->d_perm_alt, ctx->d_keys, ctx->d_keys_alt, ctx->d_idx, ctx->d_idx_alt, ctx->d_sort_tmp};
    for (void* p : sort_buffers)
        if (p) (void)hipFree(p);
    ctx->d_perm = ctx->d_perm_alt = nullptr;
    ctx->d_keys = ctx->d_keys_alt = nullptr;
    ctx->d_idx = ctx->d_idx_alt = nullptr;
    ctx->d_sort_tmp = nullptr;
    ctx->sort_tmp_bytes = 0;
    ctx->dev = DParticles{};
    ctx->alt = DParticles{};
    ctx->capacity = 0;
}

// exchange the column pointers of `dev` and `alt` (sizes / flags stay): all of them, or only the columns a launch writes
static void swap_columns(pk_ctx* ctx, bool launch_outputs_only) {
    DParticles &d = ctx->dev, &a = ctx->alt;
#define X(m, bit, elem, per_grid, optional) if (!launch_outputs_only || ((bit) & PK_LAUNCH_MASK)) std::swap(d.m, a.m);
    PK_COLUMNS(X)
#undef X
    for (int k = 0; k < PK_MAX_EXTRA && !launch_outputs_only; k++) std::swap(d.extra[k], a.extra[k]);
    std::swap(d.iter, a.iter);
    if (!launch_outputs_only) ctx->rerun_valid = false;  // the second set no longer holds the state before the last launch
}
void swap_column_sets(pk_ctx* ctx) { swap_columns(ctx, false); }    // after the cell sort and the compaction wrote the new order into `alt`
static void swap_launch_outputs(pk_ctx* ctx) { swap_columns(ctx, true); }  // the launch read `dev` and wrote `alt`

// second column set + permutation buffers, allocated on first use (only when cell sorting is requested)
int32_t ensure_alt(pk_ctx* ctx) {
    if (ctx->alt.t) return 0;
    const int64_t cap = ctx->capacity;
    const int32_t rc = alloc_column_set(ctx, ctx->alt, cap);
    if (rc) return rc;
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_perm, cap * 8));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_perm_alt, cap * 8));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_keys, cap * 8));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_keys_alt, cap * 8));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_idx, cap * 4));
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_idx_alt, cap * 4));
    return 0;
}

// The row kernels (above, and select_rows_kernel of the write filter) are templates on the unsigned integer of the column's element size and take
// (const T* src, T* dst, ...): launch the instantiation that fits `elem`, one lane per row, on the compute stream.
#define PK_LAUNCH_ROWS(ctx, kernel, elem, n, src, dst, ...)                                                                                            \
    do {                                                                                                                                               \
        const dim3 grid_((unsigned)(((n) + 255) / 256));                                                                                               \
        if ((elem) == 8) hipLaunchKernelGGL((kernel<unsigned long long>), grid_, dim3(256), 0, (ctx)->compute, (const unsigned long long*)(src), (unsigned long long*)(dst), __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<uint32_t>), grid_, dim3(256), 0, (ctx)->compute, (const uint32_t*)(src), (uint32_t*)(dst), __VA_ARGS__);      \
    } while (0)

static int bits_for(unsigned long long v) {
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

// Reorder the device rows by cell key (host row order is restored by pk_particles_d2h through d_perm).
static int32_t sort_particles(pk_ctx* ctx, int main_grid, int horizontal_major) {
    const int64_t n = ctx->dev.n;
    if (n < 2) return 0;
    if (n >= (1ll << 32)) return ctx->fail("cell sort supports < 2^32 particles per device");
    int32_t rc = ensure_alt(ctx);
    if (rc) return rc;
    const DGrid& g = ctx->grids[main_grid].d;
    const dim3 grid((unsigned)((n + 255) / 256));
    sort_keys(ctx, g, horizontal_major);
    PK_HIP(ctx, hipGetLastError());
    unsigned long long kmax;
    const unsigned long long nzc = (g.has_z && g.nz >= 2) ? (unsigned long long)g.nz : 1ull;
    if (g.kind == 1) kmax = horizontal_major ? ((0x3FFFFFFFull << 12) | 0xFFFull) : ((nzc << 30) | 0x3FFFFFFFull);
    else kmax = nzc * (unsigned long long)std::max(g.ny, 1) * (unsigned long long)std::max(g.nx, 1);
    const unsigned end_bit = (unsigned)bits_for(kmax);
    size_t tmp_bytes = 0;
    PK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, ctx->d_keys, ctx->d_keys_alt, ctx->d_idx, ctx->d_idx_alt, (size_t)n, 0u, end_bit, ctx->compute));
    if (tmp_bytes > ctx->sort_tmp_bytes) {
        if (ctx->d_sort_tmp) PK_HIP(ctx, hipFree(ctx->d_sort_tmp));
        PK_HIP(ctx, hipMalloc(&ctx->d_sort_tmp, tmp_bytes));
        ctx->sort_tmp_bytes = tmp_bytes;
    }
    PK_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_sort_tmp, tmp_bytes, ctx->d_keys, ctx->d_keys_alt, ctx->d_idx, ctx->d_idx_alt, (size_t)n, 0u, end_bit, ctx->compute));
    const uint32_t* perm = ctx->d_idx_alt;
    for (const ColRef& c : particle_columns(ctx)) {
        if (!c.d || !c.a) continue;
        PK_LAUNCH_ROWS(ctx, gather_rows_kernel, c.elem, n, c.d, c.a, perm, n, c.width);
    }
    hipLaunchKernelGGL(compose_perm_kernel, grid, dim3(256), 0, ctx->compute, ctx->has_perm ? ctx->d_perm : nullptr, perm, ctx->d_perm_alt, n);
    PK_HIP(ctx, hipGetLastError());
    swap_column_sets(ctx);
    std::swap(ctx->d_perm, ctx->d_perm_alt);
    ctx->has_perm = true;
    return 0;
}

static int32_t copy_particles(pk_ctx* ctx, bool to_device, uint32_t mask = 0xFFFFFFFFu) {
    if (!ctx->bound) return ctx->fail("no particles bound");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = ctx->host.n;
    ctx->rerun_valid = false;  // d2h stages through the second column set, h2d replaces the state
    if (n == 0) return 0;
    if (to_device) ctx->has_perm = false;  // host order
    int bit = 0;
    for (const ColRef& c : particle_columns(ctx)) {
        const bool selected = (mask >> bit++) & 1u;
        if (!c.h || !c.d || !selected) continue;
        const size_t bytes = (size_t)n * c.elem * c.width;
        if (to_device) {
            PK_HIP(ctx, hipMemcpyAsync(c.d, c.h, bytes, hipMemcpyHostToDevice, ctx->compute));
        } else if (ctx->has_perm) {  // undo the cell sort: host row perm[i] <- device row i
            scatter_rows(ctx, c, c.a, n);
            PK_HIP(ctx, hipMemcpyAsync(c.h, c.a, bytes, hipMemcpyDeviceToHost, ctx->compute));
        } else {
            PK_HIP(ctx, hipMemcpyAsync(c.h, c.d, bytes, hipMemcpyDeviceToHost, ctx->compute));
        }
    }
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

// undo the cell sort for one column: dst[host row perm[i]] <- device row i of the n rows, on the compute stream (scatter_rows_kernel has
// its one home in this unit: the D2H copy, the snapshot and pk_interact_host_order of pk_api_analysis.hip all come through here)
void scatter_rows(pk_ctx* ctx, const ColRef& c, void* dst, int64_t n) {
    PK_LAUNCH_ROWS(ctx, scatter_rows_kernel, c.elem, n, c.d, dst, ctx->d_perm, n, c.width);
}

}  // namespace pkapi

// ---- write filter ----------------------------------------------------------------------------------------
// The write filter of ParticleFile (particlefile.py:198-221: `|t_p - t| <= |dt|/2`, finite t) on the DEVICE rows, and the
// packing of the rows that pass it in HOST row order (whatever the cell sort did to the device order).  Two callers: the filtered snapshot of
// the asynchronous write-out (pk_particles_snapshot_filtered: only the rows a table holds cross PCIe, and the writer thread has nothing to
// filter) and the multi-GPU exchange (pk_api_comm.hip: through pk_api_ctx.h).
namespace pk {

// flag[host row] = the device row passes the filter (apply = 0: every row)
__global__ void write_filter_kernel(const double* __restrict__ tp, const double* __restrict__ dt, const int64_t* __restrict__ perm, int64_t n,
                                    double t, int apply, uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 1u;
    if (apply) {
        const double p = tp[i], d = dt[i];
        const double h = fabs(d / 2);
        const bool sel = ((t - h <= p) && (t + h >= p)) || (d != d && p == t);
        f = (sel && isfinite(p)) ? 1u : 0u;
    }
    flag[perm ? perm[i] : i] = f;
}
// dst[offs[host row]] = src[device row] for the flagged rows: the selected rows in host row order, packed
template <class T>
__global__ void select_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, const int64_t* __restrict__ perm, const uint32_t* __restrict__ flag,
                                   const uint32_t* __restrict__ offs, int64_t n, int width) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t h = perm ? perm[i] : i;
    if (!flag[h]) return;
    const int64_t o = (int64_t)offs[h];
    for (int w = 0; w < width; w++) dst[o * width + w] = src[i * width + w];
}

}  // namespace pk

namespace pkapi {

// flags + exclusive scan of the bound device rows at output time t; -> the number of selected rows (one small read-back)
int32_t select_flags(pk_ctx* ctx, double t, int apply_filter, int64_t* n_sel) {
    using namespace pk;
    PkSelect& S = ctx->sel;
    const int64_t n = ctx->dev.n;
    *n_sel = 0;
    if (n >= (1ll << 31)) return ctx->fail("the device write filter supports < 2^31 particles per device");
    if (n == 0) return 0;
    if (S.cap < n) {
        if (S.d_flag) PK_HIP(ctx, hipFree(S.d_flag));
        if (S.d_offs) PK_HIP(ctx, hipFree(S.d_offs));
        S.d_flag = S.d_offs = nullptr;
        S.cap = 0;
        PK_HIP(ctx, hipMalloc((void**)&S.d_flag, sizeof(uint32_t) * (size_t)n));
        PK_HIP(ctx, hipMalloc((void**)&S.d_offs, sizeof(uint32_t) * (size_t)n));
        S.cap = n;
    }
    const int64_t* perm = ctx->has_perm ? ctx->d_perm : nullptr;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(write_filter_kernel, grid, dim3(256), 0, ctx->compute, (const double*)ctx->dev.t, (const double*)ctx->dev.dt, perm, n, t,
                       apply_filter, S.d_flag);
    PK_HIP(ctx, hipGetLastError());
    size_t tmp = 0;
    PK_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, S.d_flag, S.d_offs, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->compute));
    if (S.tmp_bytes < tmp || !S.d_tmp) {
        if (S.d_tmp) PK_HIP(ctx, hipFree(S.d_tmp));
        S.d_tmp = nullptr;
        PK_HIP(ctx, hipMalloc(&S.d_tmp, std::max<size_t>(tmp, 256)));
        S.tmp_bytes = std::max<size_t>(tmp, 256);
    }
    PK_HIP(ctx, rocprim::exclusive_scan(S.d_tmp, tmp, S.d_flag, S.d_offs, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->compute));
    uint32_t last[2] = {0, 0};
    PK_HIP(ctx, hipMemcpyAsync(&last[0], S.d_offs + (n - 1), 4, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(&last[1], S.d_flag + (n - 1), 4, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    *n_sel = (int64_t)last[0] + (int64_t)last[1];
    return 0;
}
// the selected rows of one column into `dst` (room for them: the caller's business), on the compute stream
void select_column(pk_ctx* ctx, const ColRef& c, void* dst) {
    using namespace pk;
    const int64_t n = ctx->dev.n;
    const int64_t* perm = ctx->has_perm ? ctx->d_perm : nullptr;
    PK_LAUNCH_ROWS(ctx, select_rows_kernel, c.elem, n, c.d, dst, perm, ctx->sel.d_flag, ctx->sel.d_offs, n, c.width);
}

}  // namespace pkapi

extern "C" {

int32_t pk_particles_bind(pk_ctx* ctx, const pk_particles_desc* host) {
    if (!ctx || !host) return -2;
    if (host->n < 0 || host->ngrids < 1 || host->ngrids > PK_MAX_GRIDS) return ctx->fail("bad particle descriptor");
    const auto hp = column_pointers(*host);
    for (int k = 0; k < PK_COL_EXTRA_FIRST; k++)
        if (host->n > 0 && !PK_COL_INFO[k].optional && !hp[k]) return ctx->fail("particle columns must not be NULL");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (host->n_extra < 0 || host->n_extra > PK_MAX_EXTRA) return ctx->fail("bad number of extra particle columns");
    bool extra_changed = host->n_extra != ctx->host.n_extra;
    for (int k = 0; k < host->n_extra && !extra_changed; k++) extra_changed = host->extra_dtype[k] != ctx->host.extra_dtype[k];
    for (int k = 0; k < host->n_extra; k++) {
        if (host->extra_dtype[k] != PK_F32 && host->extra_dtype[k] != PK_F64) return ctx->fail("extra particle columns must be PK_F32 or PK_F64");
        if (host->n > 0 && !host->extra[k]) return ctx->fail("particle columns must not be NULL");
    }
    const bool realloc_needed = !ctx->bound || host->n > ctx->capacity || host->ngrids != ctx->host.ngrids || extra_changed ||
                                host->spatial_dtype != ctx->host.spatial_dtype || (host->next_dt != nullptr) != (ctx->dev.next_dt != nullptr);
    ctx->host = *host;
    if (realloc_needed) free_particles(ctx);
    for (int k = 0; k < PK_MAX_EXTRA; k++) ctx->dev.extra_f32[k] = ctx->alt.extra_f32[k] = (k < host->n_extra && host->extra_dtype[k] == PK_F32);
    if (realloc_needed) {
        const int64_t cap = std::max<int64_t>(host->n, 1);
        const int32_t rc = alloc_column_set(ctx, ctx->dev, cap);
        if (rc) return rc;
        ctx->capacity = cap;
    }
    ctx->has_perm = false;
    ctx->rerun_valid = false;
    ctx->chk_valid = false;
    ctx->dev.n = host->n;
    ctx->dev.ngrids = host->ngrids;
    ctx->dev.spatial_f32 = host->spatial_dtype == PK_F32;
    ctx->bound = true;
    return 0;
}

int32_t pk_particles_h2d(pk_ctx* ctx) {
    if (!ctx) return -2;
    return copy_particles(ctx, true);
}
int32_t pk_particles_d2h(pk_ctx* ctx) {
    if (!ctx) return -2;
    return copy_particles(ctx, false);
}
int32_t pk_particles_set_mask(pk_ctx* ctx, const int32_t* mask) {
    if (!ctx || !mask) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->has_perm) return ctx->fail("pk_particles_set_mask: the device rows are cell-sorted (body_only launches run on host-ordered rows: pk_particles_h2d first)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->dev.n > 0) PK_HIP(ctx, hipMemcpyAsync(ctx->dev.iter, mask, (size_t)ctx->dev.n * 4, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

// The state of every device column (and the row order of the cell sort) as of now, kept on the device: what a Kernel.execute that
// spans several launches (streamed levels, re-sort horizons) goes back to when a particle errs in a later launch and the whole
// batch has to stop at that iteration (kernel.py:236-245).  One packed buffer of ~88 B per particle, allocated on first use.
static int32_t checkpoint_copy(pk_ctx* ctx, bool save) {
    const int64_t n = save ? ctx->dev.n : ctx->chk_n;
    size_t off = 0;
    for (const ColRef& c : particle_columns(ctx)) {
        if (!c.d) continue;
        const size_t bytes = (size_t)n * c.elem * c.width;
        if (bytes) {
            if (save) PK_HIP(ctx, hipMemcpyAsync(ctx->d_chk + off, c.d, bytes, hipMemcpyDeviceToDevice, ctx->compute));
            else PK_HIP(ctx, hipMemcpyAsync(c.d, ctx->d_chk + off, bytes, hipMemcpyDeviceToDevice, ctx->compute));
        }
        off += (bytes + 255) & ~(size_t)255;
    }
    if (save ? ctx->has_perm : ctx->chk_has_perm) {
        const size_t bytes = (size_t)n * 8;
        if (save) PK_HIP(ctx, hipMemcpyAsync(ctx->d_chk + off, ctx->d_perm, bytes, hipMemcpyDeviceToDevice, ctx->compute));
        else PK_HIP(ctx, hipMemcpyAsync(ctx->d_perm, ctx->d_chk + off, bytes, hipMemcpyDeviceToDevice, ctx->compute));
    }
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}
int32_t pk_particles_checkpoint(pk_ctx* ctx) {
    if (!ctx) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_checkpoint: a launch is in flight (call pk_execute_end)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = ctx->dev.n;
    size_t need = 0;
    for (const ColRef& c : particle_columns(ctx))
        if (c.d) need += ((size_t)n * c.elem * c.width + 255) & ~(size_t)255;
    need += (size_t)n * 8 + 256;  // the permutation
    if (need > ctx->chk_bytes) {
        if (ctx->d_chk) (void)hipFree(ctx->d_chk);
        ctx->d_chk = nullptr;
        ctx->chk_bytes = 0;
        PK_HIP(ctx, hipMalloc((void**)&ctx->d_chk, need));
        ctx->chk_bytes = need;
    }
    ctx->chk_valid = false;
    const int32_t rc = checkpoint_copy(ctx, true);
    if (rc) return rc;
    ctx->chk_n = n;
    ctx->chk_has_perm = ctx->has_perm;
    ctx->chk_valid = true;
    return 0;
}
int32_t pk_particles_restore(pk_ctx* ctx) {
    if (!ctx) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_restore: a launch is in flight (call pk_execute_end)");
    if (!ctx->chk_valid) return ctx->fail("pk_particles_restore: no checkpoint (pk_particles_checkpoint; binding new particles discards it)");
    if (ctx->chk_n != ctx->dev.n) return ctx->fail("pk_particles_restore: the particle count changed since the checkpoint");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->chk_has_perm && !ctx->d_perm) return ctx->fail("pk_particles_restore: permutation buffer missing (internal error)");
    const int32_t rc = checkpoint_copy(ctx, false);
    if (rc) return rc;
    ctx->has_perm = ctx->chk_has_perm;
    ctx->rerun_valid = false;
    return 0;
}

int32_t pk_particles_d2h_columns(pk_ctx* ctx, uint32_t mask) {
    if (!ctx) return -2;
    return copy_particles(ctx, false, mask);
}

int32_t pk_particles_h2d_columns(pk_ctx* ctx, uint32_t mask) {
    if (!ctx) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_h2d_columns: a launch is in flight (call pk_execute_end)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = ctx->host.n;
    ctx->rerun_valid = false;  // the staging below goes through the second column set
    ctx->chk_valid = false;    // a checkpoint no longer describes these columns
    if (n == 0) return 0;
    if (ctx->has_perm) {
        const int32_t rc = ensure_alt(ctx);
        if (rc) return rc;
    }
    int bit = 0;
    for (const ColRef& c : particle_columns(ctx)) {
        const bool selected = (mask >> bit++) & 1u;
        if (!c.h || !c.d || !selected) continue;
        const size_t bytes = (size_t)n * c.elem * c.width;
        if (!ctx->has_perm) {
            PK_HIP(ctx, hipMemcpyAsync(c.d, c.h, bytes, hipMemcpyHostToDevice, ctx->compute));
        } else {  // device row i holds host row perm[i]
            PK_HIP(ctx, hipMemcpyAsync(c.a, c.h, bytes, hipMemcpyHostToDevice, ctx->compute));
            PK_LAUNCH_ROWS(ctx, gather_rows64_kernel, c.elem, n, c.a, c.d, ctx->d_perm, n, c.width);
            PK_HIP(ctx, hipGetLastError());
        }
    }
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

int32_t pk_particles_fill_f64(pk_ctx* ctx, uint32_t mask, double value) {
    if (!ctx) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_fill_f64: a launch is in flight (call pk_execute_end)");
    if (mask & ~(PK_COL_T | PK_COL_DT | PK_COL_NEXT_DT)) return ctx->fail("pk_particles_fill_f64: float64 columns only (t, dt, next_dt)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = ctx->dev.n;
    ctx->rerun_valid = false;
    ctx->chk_valid = false;
    if (n == 0) return 0;
    const dim3 grid((unsigned)((n + 255) / 256));
    double* cols[3] = {(mask & PK_COL_T) ? ctx->dev.t : nullptr, (mask & PK_COL_DT) ? ctx->dev.dt : nullptr, (mask & PK_COL_NEXT_DT) ? ctx->dev.next_dt : nullptr};
    for (double* c : cols)
        if (c) hipLaunchKernelGGL(fill_f64_kernel, grid, dim3(256), 0, ctx->compute, c, n, value);
    PK_HIP(ctx, hipGetLastError());
    return 0;  // (stream order: the next launch sees it)
}

int32_t pk_particles_t_stats(pk_ctx* ctx, double* t_min, double* t_max, int64_t* n_nan) {
    if (!ctx || !t_min || !t_max || !n_nan) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_t_stats: a launch is in flight (call pk_execute_end)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = ctx->dev.n;
    *t_min = *t_max = NAN;
    *n_nan = 0;
    if (n == 0) return 0;
    const unsigned long long init[3] = {~0ull, 0ull, 0ull};
    PK_HIP(ctx, hipMemcpyAsync(ctx->d_tstats, init, sizeof(init), hipMemcpyHostToDevice, ctx->compute));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(t_stats_kernel, dim3(grid), dim3(256), 0, ctx->compute, ctx->dev.t, n, ctx->d_tstats);
    PK_HIP(ctx, hipGetLastError());
    unsigned long long got[3];
    PK_HIP(ctx, hipMemcpyAsync(got, ctx->d_tstats, sizeof(got), hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    auto unmap = [](unsigned long long b) {
        b = (b & 0x8000000000000000ull) ? (b & 0x7fffffffffffffffull) : ~b;
        double v;
        memcpy(&v, &b, 8);
        return v;
    };
    if (got[0] != ~0ull || got[1] != 0ull) {
        *t_min = unmap(got[0]);
        *t_max = unmap(got[1]);
    }
    *n_nan = (int64_t)got[2];
    return 0;
}

// ---- asynchronous write-out (particleset.py:436-459 / particlefile.py:142-180 overlapped with the next interval) -------------
static int32_t snapshot_begin(pk_ctx* ctx, uint32_t mask, int32_t slot, bool filtered, double t_out);
int32_t pk_particles_snapshot_begin(pk_ctx* ctx, uint32_t mask, int32_t slot) { return snapshot_begin(ctx, mask, slot, false, 0.0); }
int32_t pk_particles_snapshot_filtered(pk_ctx* ctx, uint32_t mask, int32_t slot, double t) { return snapshot_begin(ctx, mask, slot, true, t); }
}  // extern "C"
// filtered: only the rows that pass the write filter of particlefile.py:198-221 at output time t_out, packed in host row order (select_flags)
static int32_t snapshot_begin(pk_ctx* ctx, uint32_t mask, int32_t slot, bool filtered, double t_out) {
    if (!ctx) return -2;
    if (slot < 0 || slot > 1) return ctx->fail("snapshot slot must be 0 or 1");
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_snapshot_begin: a launch is in flight");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    pk_ctx::Snapshot& sn = ctx->snap[slot];
    if (sn.in_flight) return ctx->fail("snapshot slot still in flight (pk_particles_snapshot_wait first)");
    if (!sn.ready) {
        PK_HIP(ctx, hipEventCreateWithFlags(&sn.ready, hipEventDisableTiming));
        PK_HIP(ctx, hipEventCreateWithFlags(&sn.done, hipEventDisableTiming));
    }
    const int64_t n = ctx->dev.n;
    const std::vector<ColRef> cols = particle_columns(ctx);
    const size_t ss = spatial_size(ctx);
    bool fits = sn.capacity >= n && sn.ngrids == ctx->host.ngrids && sn.ss == ss;
    for (int k = 0; k < PK_MAX_EXTRA; k++) fits = fits && sn.extra_elem[k] == (cols[PK_COL_EXTRA_FIRST + k].d ? cols[PK_COL_EXTRA_FIRST + k].elem : 0);
    for (int k = 0; k < PK_NCOLS; k++)
        if (((mask >> k) & 1u) && cols[k].d && !sn.dev[k]) fits = false;  // a column the buffers were not sized for
    if (!fits) {  // (re)size the columns of this mask only: pinning costs ~0.3 s per GB
        for (int k = 0; k < PK_NCOLS; k++) {
            if (sn.dev[k]) PK_HIP(ctx, hipFree(sn.dev[k]));
            if (sn.host[k]) PK_HIP(ctx, hipHostFree(sn.host[k]));
            sn.dev[k] = sn.host[k] = nullptr;
        }
        const int64_t cap = std::max<int64_t>(n, 1);  // particle sets only shrink during a run (deletions)
        for (int k = 0; k < PK_NCOLS; k++) {
            if (!((mask >> k) & 1u) || !cols[k].d) continue;
            const size_t bytes = (size_t)cap * cols[k].elem * cols[k].width;
            PK_HIP(ctx, hipMalloc(&sn.dev[k], bytes));
            PK_HIP(ctx, hipHostMalloc(&sn.host[k], bytes, hipHostMallocDefault));
        }
        sn.capacity = cap;
        sn.ngrids = ctx->host.ngrids;
        sn.ss = ss;
        for (int k = 0; k < PK_MAX_EXTRA; k++) sn.extra_elem[k] = cols[PK_COL_EXTRA_FIRST + k].d ? cols[PK_COL_EXTRA_FIRST + k].elem : 0;
    }
    sn.n = n;
    sn.mask = mask;
    int64_t n_out = n;
    if (filtered && n > 0) {
        int32_t rc = select_flags(ctx, t_out, 1, &n_out);  // (one 8-byte read-back: the row count the D2H below needs)
        if (rc) return rc;
        for (int k = 0; k < PK_NCOLS && n_out > 0; k++) {
            const ColRef& c = cols[k];
            if (!((mask >> k) & 1u) || !c.d) continue;
            select_column(ctx, c, sn.dev[k]);
        }
        PK_HIP(ctx, hipGetLastError());
        sn.n = n_out;
    } else if (n > 0) {
        for (int k = 0; k < PK_NCOLS; k++) {
            const ColRef& c = cols[k];
            if (!((mask >> k) & 1u) || !c.d) continue;
            const size_t bytes = (size_t)n * c.elem * c.width;
            if (ctx->has_perm) {  // undo the cell sort: host row perm[i] <- device row i
                scatter_rows(ctx, c, sn.dev[k], n);
            } else {
                PK_HIP(ctx, hipMemcpyAsync(sn.dev[k], c.d, bytes, hipMemcpyDeviceToDevice, ctx->compute));
            }
        }
        PK_HIP(ctx, hipGetLastError());
    }
    PK_HIP(ctx, hipEventRecord(sn.ready, ctx->compute));  // the next launch may now overwrite the live columns
    PK_HIP(ctx, hipStreamWaitEvent(ctx->copy, sn.ready, 0));
    for (int k = 0; k < PK_NCOLS && n_out > 0; k++) {
        const ColRef& c = cols[k];
        if (!((mask >> k) & 1u) || !c.d) continue;
        PK_HIP(ctx, hipMemcpyAsync(sn.host[k], sn.dev[k], (size_t)n_out * c.elem * c.width, hipMemcpyDeviceToHost, ctx->copy));
    }
    PK_HIP(ctx, hipEventRecord(sn.done, ctx->copy));
    sn.in_flight = true;
    return 0;
}
extern "C" {

// Wait for the snapshot in `slot` and hand out its pinned host columns (valid until the next snapshot_begin on that slot).
// May be called from a second host thread while the first one drives the next launch: it only waits on an event.
int32_t pk_particles_snapshot_wait(pk_ctx* ctx, int32_t slot, pk_particles_desc* out) {
    if (!ctx || !out) return -2;
    if (slot < 0 || slot > 1) return -2;
    pk_ctx::Snapshot& sn = ctx->snap[slot];
    if (!sn.in_flight) return -3;  // (no ctx->fail here: the error string belongs to the driving thread)
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    if (hipEventSynchronize(sn.done) != hipSuccess) return -1;
    sn.in_flight = false;
    memset(out, 0, sizeof(*out));
    out->n = sn.n;
    out->ngrids = sn.ngrids;
    out->spatial_dtype = sn.ss == 4 ? PK_F32 : PK_F64;
    void* cols[PK_NCOLS];
    for (int k = 0; k < PK_NCOLS; k++) cols[k] = ((sn.mask >> k) & 1u) ? sn.host[k] : nullptr;
    set_column_pointers(*out, cols, PK_NCOLS);
    for (int k = 0; k < PK_MAX_EXTRA; k++) {
        out->extra_dtype[k] = sn.extra_elem[k] == 4 ? PK_F32 : PK_F64;
        if (sn.extra_elem[k]) out->n_extra = k + 1;
    }
    return 0;
}

int32_t pk_particles_device(pk_ctx* ctx, pk_particles_desc* dev, int64_t** perm) {
    if (!ctx || !dev) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    dev->n = ctx->dev.n;
    dev->ngrids = ctx->dev.ngrids;
    dev->spatial_dtype = ctx->host.spatial_dtype;
    set_column_pointers(*dev, column_pointers(ctx->dev).data(), PK_COL_EXTRA_FIRST);  // (the extras are not handed out)
    if (perm) *perm = ctx->has_perm ? ctx->d_perm : nullptr;
    return 0;
}

// Remove the rows whose state is Delete from the DEVICE-RESIDENT columns (order of the survivors kept, in device order and
// in host order) and re-point the host side at `new_host`, the caller's arrays of the surviving length: no column crosses
// PCIe.  Kernel.remove_deleted (kernel.py:98-106) without the round trip through NumPy.
int32_t pk_particles_compact(pk_ctx* ctx, const pk_particles_desc* new_host, int64_t* n_new) {
    if (!ctx || !new_host || !n_new) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_compact: a launch is in flight");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = ctx->dev.n;
    if (n >= (1ll << 32)) return ctx->fail("device compaction supports < 2^32 particles per device");
    if (new_host->ngrids != ctx->host.ngrids || new_host->spatial_dtype != ctx->host.spatial_dtype ||
        (new_host->next_dt != nullptr) != (ctx->host.next_dt != nullptr) || new_host->n_extra != ctx->host.n_extra)
        return ctx->fail("pk_particles_compact: the new host columns must have the bound schema");
    int64_t kept = 0;
    if (n > 0) {
        int32_t rc = ensure_alt(ctx);
        if (rc) return rc;
        const dim3 grid((unsigned)((n + 255) / 256));
        unsigned long long *keep = ctx->d_keys, *pos = ctx->d_keys_alt;
        uint32_t *keep_host = ctx->d_idx, *host_pos = ctx->d_idx_alt;
        const int64_t* perm = ctx->has_perm ? ctx->d_perm : nullptr;
        hipLaunchKernelGGL(keep_flags_kernel, grid, dim3(256), 0, ctx->compute, ctx->dev.state, perm, n, keep, keep_host);
        size_t tb1 = 0, tb2 = 0;
        PK_HIP(ctx, rocprim::exclusive_scan(nullptr, tb1, keep, pos, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), ctx->compute));
        PK_HIP(ctx, rocprim::exclusive_scan(nullptr, tb2, keep_host, host_pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->compute));
        const size_t tb = std::max(tb1, tb2);
        if (tb > ctx->sort_tmp_bytes) {
            if (ctx->d_sort_tmp) PK_HIP(ctx, hipFree(ctx->d_sort_tmp));
            PK_HIP(ctx, hipMalloc(&ctx->d_sort_tmp, tb));
            ctx->sort_tmp_bytes = tb;
        }
        PK_HIP(ctx, rocprim::exclusive_scan(ctx->d_sort_tmp, tb1, keep, pos, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), ctx->compute));
        PK_HIP(ctx, rocprim::exclusive_scan(ctx->d_sort_tmp, tb2, keep_host, host_pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->compute));
        unsigned long long last_pos = 0, last_keep = 0;
        PK_HIP(ctx, hipMemcpyAsync(&last_pos, pos + (n - 1), 8, hipMemcpyDeviceToHost, ctx->compute));
        PK_HIP(ctx, hipMemcpyAsync(&last_keep, keep + (n - 1), 8, hipMemcpyDeviceToHost, ctx->compute));
        for (const ColRef& c : particle_columns(ctx)) {
            if (!c.d || !c.a) continue;
            PK_LAUNCH_ROWS(ctx, compact_rows_kernel, c.elem, n, c.d, c.a, keep, pos, n, c.width);
        }
        if (perm) hipLaunchKernelGGL(compact_perm_kernel, grid, dim3(256), 0, ctx->compute, perm, keep, pos, host_pos, n, ctx->d_perm_alt);
        PK_HIP(ctx, hipGetLastError());
        PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
        kept = (int64_t)(last_pos + last_keep);
        swap_column_sets(ctx);
        if (perm) std::swap(ctx->d_perm, ctx->d_perm_alt);
    }
    if (new_host->n != kept) return ctx->fail("pk_particles_compact: new host columns hold " + std::to_string(new_host->n) + " rows, " +
                                              std::to_string(kept) + " particles survive");
    ctx->dev.n = kept;
    ctx->host = *new_host;
    *n_new = kept;
    return 0;
}

}  // extern "C" (the planner's helpers: C++ linkage, some are called from pk_api_sample.hip)

namespace pkapi {

// ---- execution -----------------------------------------------------------------------------------------
// pk_exec_stats.program of a launch that runs a dedicated kernel (other launches report their PROG_*, pk_kernels.h)
enum { PROGRAM_FAST_AGRID = 100, PROGRAM_FAST_CGRID = 101 };
// Which dedicated kernel runs a launch.  The values are the `prog` argument of a user module's launcher (pk_set_user_program), where
// DEDICATED_NONE is its kernel-list interpreter.
enum Dedicated { DEDICATED_NONE = 0, DEDICATED_A2 = 1, DEDICATED_A3 = 2, DEDICATED_C2 = 3, DEDICATED_C3 = 4 };

// Some grid stores a coordinate as float32: NumPy's float32 arithmetic on coordinate / barycentric arrays has to be reproduced
// (pk_device.h: TYPED), which only the PROG_TYPED program and the typed sampling kernels carry.
bool ctx_is_typed(const pk_ctx* ctx) {
    for (const HostGrid& g : ctx->grids)
        if (g.d.lon_f32 || g.d.lat_f32 || g.d.depth_f32) return true;
    return false;
}

// some grid of the context is a UxGrid (pk_ugrid_create)
bool ctx_has_ugrid(const pk_ctx* ctx) {
    for (const HostGrid& g : ctx->grids)
        if (g.d.kind == PK_UX_KIND) return true;
    return false;
}

// The kernel-list interpreter variant of a launch (include/parcels_hip.h: pk_generic_variant)
static int32_t interp_key(const pk_ctx* ctx, const pk_exec_params* prm, const KArgs& a) {
    if (ctx->grids[a.main_grid].d.kind == PK_UX_KIND) return PK_USER_KEY_UX;  // the step loop of pk_ux.h: no structured variant
    return (ctx->fields[prm->fU].d.dtype == PK_F32 ? 6 : 0) + (ctx->grids[a.main_grid].d.kind == 1 ? 3 : 0) + std::min<int>(prm->interp_uv, 2);
}

// The variant of the CROCO sigma loop (pk_sigma.h) a launch runs: what launch_sigma dispatches on, behind PK_USER_KEY_SIGMA
static int32_t sigma_key(const pk_ctx* ctx, const pk_exec_params* prm, const KArgs& a) {
    return PK_USER_KEY_SIGMA + (ctx->fields[prm->fU].d.dtype == PK_F32 ? 4 : 0) + (ctx->grids[a.main_grid].d.kind == 1 ? 2 : 0) + (prm->interp_uv ? 1 : 0);
}

// The launch arguments of `prm` apart from the descriptor tables (upload_descriptors): main field and grid, resident time window, LDS layout.
// planning: the arguments are wanted to name the program variant only (pk_generic_variant, asked before the first window of a streamed
// fieldset is committed): a ring without a resident level is no error then.
int32_t launch_args(pk_ctx* ctx, const pk_exec_params* prm, KArgs& a, size_t& lds_bytes, int& use_lds, bool planning) {
    memset(&a, 0, sizeof(a));
    a.p = ctx->dev;
    a.prm = *prm;
    a.counters = ctx->d_counters;
    a.twe_listed = ctx->d_twe;
    a.twe_found = ctx->d_twe_found;
    a.twe_hit = ctx->d_twe_hit;
    const int nf = (int)ctx->fields.size();
    auto valid = [&](int f) { return f >= 0 && f < nf; };
    if (!valid(prm->fU) || !valid(prm->fV)) return ctx->fail("params.fU/fV must name existing fields");
    if (prm->fW >= nf || prm->fKh_zonal >= nf || prm->fKh_meridional >= nf) return ctx->fail("params refer to unknown fields");
    a.main_field = prm->fU;
    a.main_grid = ctx->fields[prm->fU].d.grid;
    const HostField& mf = ctx->fields[prm->fU];
    const HostGrid& mg = ctx->grids[a.main_grid];
    // resident time window: the intersection over every time-varying field that lives in a ring of slots (each on its own
    // time axis).  A particle steps only while [t, t+dt] lies inside it, so no field is sampled on a level that is not there.
    a.win_lo = -INFINITY;
    a.win_hi = INFINITY;
    for (const HostField& f : ctx->fields) {
        if (!f.d.has_time_interval || f.d.nslots >= f.desc.nt) continue;
        int lo = 1 << 30, hi = -1, cnt = 0;
        for (int lv : f.slot_level)
            if (lv >= 0) { lo = std::min(lo, lv); hi = std::max(hi, lv); cnt++; }
        if (cnt == 0 && planning) continue;
        if (cnt == 0) return ctx->fail("no time level of a streamed field is resident (pk_field_upload_level)");
        if (hi - lo + 1 != cnt) return ctx->fail("resident time levels are not contiguous (pk_field_evict_outside)");
        // nothing earlier / later exists at the ends of the axis: let the kernels raise code 70 there
        if (lo > 0) a.win_lo = std::max(a.win_lo, f.time[lo]);
        if (hi < f.desc.nt - 1) a.win_hi = std::min(a.win_hi, f.time[hi]);
    }
    // soft horizon of the launch (re-sort cadence of a long fused run): same pause as at the edge of a level ring
    if (prm->horizon_lo < prm->horizon_hi) {  // (lo >= hi, e.g. a zeroed struct: no horizon)
        if (prm->horizon_lo > a.win_lo) a.win_lo = prm->horizon_lo;
        if (prm->horizon_hi < a.win_hi) a.win_hi = prm->horizon_hi;
    }
    // LDS staging of the main grid's 1-D vectors
    const int nt = mf.d.has_time_interval ? mf.d.nt : 0;
    const int nz = mg.d.has_z ? mg.d.nz : 0;
    const int ny = mg.d.kind == 0 ? mg.d.ny : 0;
    const int nx = mg.d.kind == 0 ? mg.d.nx : 0;
    a.lds_time = 0;
    a.lds_depth = a.lds_time + nt;
    a.lds_lat = a.lds_depth + nz;
    a.lds_lon = a.lds_lat + ny;
    a.lds_total = a.lds_lon + nx;
    lds_bytes = (size_t)std::max(a.lds_total, 1) * sizeof(double);
    use_lds = lds_bytes <= 64 * 1024;
    if (!use_lds) lds_bytes = 0;
    // per-lane cell cache of curvilinear grids (pk_device.h: CellCache): CC_NODE_ROWS doubles + 4 key ints per lane, plus the
    // 12 staggered field values of a C-grid evaluation when they still fit the 64 KiB of a workgroup
    a.lds_cc_nodes = a.lds_cc_keys = a.lds_cc_fvals = -1;
    const bool want_cc = use_lds && mg.d.kind == 1 && !ctx->no_cell_cache && (int64_t)mg.d.ny * mg.d.nx < INT32_MAX;
    if (want_cc) {
        const size_t node_b = CC_NODE_ROWS * CC_LANES * sizeof(double), key_b = 4 * CC_LANES * sizeof(int32_t);
        const size_t fval_b = 12 * CC_LANES * (size_t)(mf.desc.dtype == PK_F32 ? 4 : 8);
        if (lds_bytes + node_b + key_b <= 64 * 1024) {
            a.lds_cc_nodes = a.lds_total;
            a.lds_cc_keys = a.lds_cc_nodes + CC_NODE_ROWS * CC_LANES;
            int32_t end = a.lds_cc_keys + (int32_t)(key_b / sizeof(double));
            // (A/B on config 3: without the cached field values the RK4_3D launch takes 96.6 ms instead of 66.3 ms)
            if (prm->interp_uv == 1 && (size_t)end * sizeof(double) + fval_b <= 64 * 1024) {
                a.lds_cc_fvals = end;
                end += (int32_t)(fval_b / sizeof(double));
            }
            lds_bytes = (size_t)end * sizeof(double);
        }
    }
    return 0;
}

// Descriptor tables: [grids][fields] in one device buffer, refreshed on the compute stream when anything changed since the last launch (ring
// slots move with every streamed level).  In stream order, so a kernel still running keeps reading the old values.
int32_t upload_descriptors(pk_ctx* ctx, KArgs& a) {
    const size_t gb = ctx->grids.size() * sizeof(DGrid), fb = ctx->fields.size() * sizeof(DField);
    const size_t need = gb + fb;
    if (need > ctx->desc_bytes) {
        const size_t cap = (size_t)PK_MAX_GRIDS * sizeof(DGrid) + (size_t)PK_MAX_FIELDS * sizeof(DField);
        if (ctx->d_desc) (void)hipFree(ctx->d_desc);
        if (ctx->h_desc) (void)hipHostFree(ctx->h_desc);
        ctx->d_desc = ctx->h_desc = nullptr;
        ctx->desc_bytes = 0;
        PK_HIP(ctx, hipMalloc((void**)&ctx->d_desc, cap));
        PK_HIP(ctx, hipHostMalloc((void**)&ctx->h_desc, 2 * cap, hipHostMallocDefault));  // staged copy + what the device holds
        memset(ctx->h_desc, 0xFF, 2 * cap);
        ctx->desc_bytes = cap;
    }
    char* stage = ctx->h_desc;                    // what this launch needs
    char* mirror = ctx->h_desc + ctx->desc_bytes;  // what was uploaded last
    std::vector<char> cur(need);
    for (size_t g = 0; g < ctx->grids.size(); g++) memcpy(cur.data() + g * sizeof(DGrid), &ctx->grids[g].d, sizeof(DGrid));
    for (size_t f = 0; f < ctx->fields.size(); f++) memcpy(cur.data() + gb + f * sizeof(DField), &ctx->fields[f].d, sizeof(DField));
    if (need && memcmp(cur.data(), mirror, need) != 0) {
        // the previous upload from `stage` completed long ago unless a launch is still queued behind it: wait for the stream then
        PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
        memcpy(stage, cur.data(), need);
        PK_HIP(ctx, hipMemcpyAsync(ctx->d_desc, stage, need, hipMemcpyHostToDevice, ctx->compute));
        memcpy(mirror, cur.data(), need);
    }
    a.grids = (const PK_CONST_AS DGrid*)ctx->d_desc;
    a.fields = (const PK_CONST_AS DField*)(ctx->d_desc + gb);
    return 0;
}

// Two fields a dedicated kernel addresses with one set of offsets: same dtype, layout, time levels and ring
static bool same_layout(const DField& x, const DField& y) {
    return x.dtype == y.dtype && x.st_t == y.st_t && x.st_z == y.st_z && x.st_y == y.st_y && x.st_x == y.st_x && x.nt == y.nt && x.nz == y.nz &&
           x.ny == y.ny && x.nx == y.nx && x.nslots == y.nslots && x.has_time_interval == y.has_time_interval;
}

// Ravel strides of `ei` (basegrid.py:83-152), 0 for an axis the grid lacks
static void ravel_strides(const DGrid& g, uint32_t& ex, uint32_t& ey, uint32_t& ez) {
    uint32_t stride = 1;
    ex = ey = ez = 0;
    if (g.has_x) { ex = stride; stride *= (uint32_t)g.xdim; }
    if (g.has_y) { ey = stride; stride *= (uint32_t)g.ydim; }
    if (g.has_z) ez = stride;
}

// (Re)build `t` for (grid, field) unless it holds them already: {a, 1/width} rows of the host time axis time[0 .. nt), then of each device
// vector of `axes`.  t.ok when every width d has a well-scaled reciprocal and the table fits `max_bytes` of LDS.  An empty table is
// uploaded as one zero row (the kernel still binds it).
static int32_t coord_table(pk_ctx* ctx, CoordTable& t, int grid, int field, const double* time, int nt,
                           std::initializer_list<std::pair<const double*, int>> axes, size_t max_bytes) {
    if (t.grid == grid && t.field == field) return 0;
    t.grid = grid;
    t.field = field;
    t.ok = false;
    std::vector<double> tab, tmp;
    bool ok = true;
    auto push = [&](const double* arr, int n) {
        for (int i = 0; i < n; i++) {
            double r = 0.0;
            if (i + 1 < n) {
                const double d = arr[i + 1] - arr[i];
                r = 1.0 / d;
                if (!(d > 1e-100 && d < 1e100) || !std::isfinite(r)) ok = false;
            }
            tab.push_back(arr[i]);
            tab.push_back(r);
        }
    };
    int k = 0;
    t.off[k++] = 0;
    push(time, nt);
    for (const auto& [dev, n] : axes) {
        t.off[k++] = (int32_t)(tab.size() / 2);
        tmp.assign((size_t)std::max(n, 0), 0.0);
        if (n > 0) PK_HIP(ctx, hipMemcpy(tmp.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost));
        push(tmp.data(), n);
    }
    t.off[k] = (int32_t)(tab.size() / 2);
    if (tab.size() * sizeof(double) > max_bytes) ok = false;
    if (tab.empty()) tab.assign(2, 0.0);
    if (ok) {
        PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
        if (tab.size() > t.cap) {
            if (t.d) PK_HIP(ctx, hipFree(t.d));
            PK_HIP(ctx, hipMalloc((void**)&t.d, tab.size() * sizeof(double)));
            t.cap = tab.size();
        }
        PK_HIP(ctx, hipMemcpy(t.d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    t.ok = ok;
    return 0;
}

// Fold the descriptors of the velocity fields and their grid into the wave-uniform constants of the fast A-grid path for `prog` (PROG_RK4 /
// PROG_RK4_3D; pk_device.h: FastA, pk_fast_agrid.h) when its preconditions hold: rectilinear grid with float64 coordinates, XLinear_Velocity,
// U / V (/ W) plain arrays of one layout with adjacent x-corners, a time level below 4 GiB (32-bit lane offsets), and coordinate
// vectors whose cell widths have well-scaled reciprocals.  a.fast.ok == 0 otherwise (the general program runs).
static int32_t fill_fast(pk_ctx* ctx, const pk_exec_params* prm, KArgs& a, int prog) {
    FastA& F = a.fast;
    memset(&F, 0, sizeof(F));
    if (ctx->no_fast || prm->interp_uv != 0 || prm->rk45_mode) return 0;  // rk45_mode: dt follows the next_dt column (kernel.py:118-120)
    const bool want_w = prog == PROG_RK4_3D;
    const HostField& U = ctx->fields[prm->fU];
    const HostField& V = ctx->fields[prm->fV];
    const HostField* W = (want_w && prm->fW >= 0) ? &ctx->fields[prm->fW] : nullptr;
    if (want_w && !W) return 0;
    const HostGrid& g = ctx->grids[U.d.grid];
    if (g.d.kind != 0 || g.d.lon_f32 || g.d.lat_f32 || g.d.depth_f32) return 0;
    if (V.d.grid != U.d.grid || (W && W->d.grid != U.d.grid)) return 0;
    auto same = [](const DField& x, const DField& y) { return x.ncomp == 1 && y.ncomp == 1 && same_layout(x, y); };
    if (!same(U.d, V.d) || (W && !same(U.d, W->d))) return 0;
    if (V.time != U.time || (W && W->time != U.time)) return 0;
    const DField& f = U.d;
    const size_t esz = f.dtype == PK_F64 ? 8 : 4;
    if (!g.d.has_x || f.st_x != 1 || f.nx < 2 || f.nx != g.d.nx) return 0;
    // an axis the fields extend over must be the grid's axis (then an in-bounds cell index + 1 never needs clipping)
    const bool fy = f.ny >= 2 && f.st_y > 0, fz = f.nz >= 2 && f.st_z > 0;
    if (fy && !(g.d.has_y && f.ny == g.d.ny)) return 0;
    if (fz && !(g.d.has_z && f.nz == g.d.nz)) return 0;
    if (f.has_time_interval && (f.nt < 2 || U.time.front() != 0.0)) return 0;
    const uint64_t lvl_b = (uint64_t)f.st_t * esz;
    const uint64_t last_b = ((uint64_t)f.nz * (uint64_t)f.st_z + (uint64_t)f.ny * (uint64_t)f.st_y + (uint64_t)f.nx) * esz;
    if (lvl_b >= (1ull << 32) || last_b >= (1ull << 32)) return 0;
    const CoordTable& T = ctx->tab_a;
    if (int32_t rc = coord_table(ctx, ctx->tab_a, U.d.grid, prm->fU, U.time.data(), f.has_time_interval ? f.nt : 0,
                                 {{g.d.depth, g.d.has_z ? g.d.nz : 0}, {g.d.lat, g.d.has_y ? g.d.ny : 0}, {g.d.lon, g.d.nx}}, 60 * 1024))
        return rc;
    if (!T.ok) return 0;
    const double inv_deg2m = 1.0 / g.d.deg2m;
    if (!(g.d.deg2m > 1e-100 && g.d.deg2m < 1e100) || !std::isfinite(inv_deg2m)) return 0;
    F.grid = U.d.grid;
    F.has_ti = f.has_time_interval;
    F.has_z = g.d.has_z; F.has_y = g.d.has_y; F.has_x = g.d.has_x;
    F.spherical = g.d.spherical;
    F.nt = f.nt;
    F.nslots = f.nslots;
    F.gnz = g.d.nz; F.gny = g.d.ny; F.gnx = g.d.nx;
    ravel_strides(g.d, F.ex, F.ey, F.ez);
    F.st_z = (uint32_t)f.st_z;
    F.st_y = (uint32_t)f.st_y;
    F.dyb = fy ? (uint32_t)(f.st_y * esz) : 0u;
    F.dzb = fz ? (uint32_t)(f.st_z * esz) : 0u;
    F.lds_time = T.off[0]; F.lds_depth = T.off[1]; F.lds_lat = T.off[2]; F.lds_lon = T.off[3];
    F.lds_n = T.off[4];
    F.lvl_b = (int64_t)lvl_b;
    F.U = (const char*)U.d.data; F.V = (const char*)V.d.data; F.W = W ? (const char*)W->d.data : nullptr;
    F.tab = T.d;
    F.tlen = f.tlen; F.t0 = f.tfirst; F.t1 = f.tlast;
    F.z0 = g.d.zfirst; F.z1 = g.d.zlast; F.y0 = g.d.yfirst; F.y1 = g.d.ylast; F.x0 = g.d.xfirst; F.x1 = g.d.xlast;
    F.deg2m = g.d.deg2m;
    F.inv_deg2m = inv_deg2m;
    F.ok = 1;
    return 0;
}

// The pair copies of FastC::vp (2-D C-grid kernels) for the levels that are resident right now: allocated on first use (no memory for
// them: the kernels read the level rings), (re)packed on the compute stream -- ahead of the launch that is being prepared -- for every
// pair of adjacent committed levels whose copy is missing or older than one of the four uploads it was made from.
static void ensure_velocity_pairs(pk_ctx* ctx, const pk_exec_params* prm, FastC& F) {
    F.vp = nullptr;
    F.vp_slot_b = 0;
    F.vp_hi = 0;
    if (ctx->no_velocity_pairs) return;
    const HostField& U = ctx->fields[prm->fU];
    const HostField& V = ctx->fields[prm->fV];
    const DField& f = U.d;
    if (!f.has_time_interval || f.nt < 2 || f.st_t <= 0) return;
    const size_t esz = f.dtype == PK_F64 ? 8 : 4;
    const int ns = f.nslots;
    const size_t slot_b = (size_t)f.st_t * 8 * esz;
    const size_t need = slot_b * (size_t)ns;
    if (ctx->vp_fU != prm->fU || ctx->vp_fV != prm->fV || ctx->vp_bytes != need || (int)ctx->vp_level.size() != ns) {
        if (ctx->d_vp) {
            (void)hipStreamSynchronize(ctx->compute);
            (void)hipFree(ctx->d_vp);
            ctx->d_vp = nullptr;
        }
        ctx->vp_fU = prm->fU;
        ctx->vp_fV = prm->fV;
        ctx->vp_bytes = need;
        ctx->vp_level.assign(ns, -1);
        ctx->vp_gen.assign((size_t)ns * 4, 0);
        // an opportunistic allocation must not starve what the run needs later (checkpoints, snapshots, further fields): it is made only
        // while it leaves a quarter of the device memory -- and at least its own size again -- free
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + std::max(need, total_b / 4)) {
            (void)hipGetLastError();
            ctx->d_vp = nullptr;
        } else if (hipMalloc((void**)&ctx->d_vp, need) != hipSuccess) {
            (void)hipGetLastError();
            ctx->d_vp = nullptr;
        }
    }
    if (!ctx->d_vp) return;
    const int64_t cb = F.cb;
    // the resident levels must be ONE run lo..hi of at least two (a ring in steady state, or everything): else the level rings serve
    int lo = -1, hi = -1, count = 0;
    for (int L = 0; L < f.nt; L++) {
        const int sl = L % ns;
        if (U.slot_level[sl] != L || V.slot_level[sl] != L) continue;
        if (lo < 0) lo = L;
        hi = L;
        count++;
    }
    if (lo < 0 || hi == lo || count != hi - lo + 1) return;
    bool timing = false;
    for (int L = lo; L < hi; L++) {
        const int s0 = L % ns, s1 = (L + 1) % ns, ps = L % ns;
        const uint64_t g[4] = {U.slot_gen[s0], U.slot_gen[s1], V.slot_gen[s0], V.slot_gen[s1]};
        uint64_t* have = &ctx->vp_gen[(size_t)ps * 4];
        if (ctx->vp_level[ps] == L && have[0] == g[0] && have[1] == g[1] && have[2] == g[2] && have[3] == g[3]) continue;
        const int64_t n = f.st_t;
        const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 64);
        char* out = ctx->d_vp + (size_t)ps * slot_b;
        if (!timing) {
            (void)hipEventRecord(ctx->ev_p0, ctx->compute);
            timing = true;
        }
        const int64_t o0 = (int64_t)s0 * F.lvl_b, o1 = (int64_t)s1 * F.lvl_b;
        if (esz == 8)
            hipLaunchKernelGGL((cg_pack_pairs_kernel<double>), dim3(grid), dim3(256), 0, ctx->compute, F.U, F.V, F.dU0, F.dU1, F.dV0, F.dV1, cb, o0, o1, n,
                               (int32_t)f.ny, (int32_t)f.nx, (double*)out);
        else
            hipLaunchKernelGGL((cg_pack_pairs_kernel<float>), dim3(grid), dim3(256), 0, ctx->compute, F.U, F.V, F.dU0, F.dU1, F.dV0, F.dV1, cb, o0, o1, n,
                               (int32_t)f.ny, (int32_t)f.nx, (float*)out);
        if (hipGetLastError() != hipSuccess) return;  // (the level rings serve)
        ctx->vp_level[ps] = L;
        for (int k = 0; k < 4; k++) have[k] = g[k];
        ctx->fl_packs++;
    }
    if (timing) (void)hipEventRecord(ctx->ev_p1, ctx->compute);
    F.vp_hi = hi;
    // every pair inside the window a launch may touch is packed now: the resident window is made of committed levels only
    F.vp = ctx->d_vp;
    F.vp_slot_b = (int64_t)slot_b;
}

// Fold the descriptors of a C-grid velocity and its spherical curvilinear grid into the wave-uniform constants of the fast C-grid path for
// `prog` (PROG_RK4 / PROG_RK4_3D / PROG_RK45 / PROG_M1; pk_device.h: FastC, pk_fast_cgrid.h).  a.fastc.ok == 0 when a precondition fails
// (the general program runs): float64 node coordinates, spherical mesh, per-cell table present, U / V (/ W) of one shape on the grid's own
// node counts with staggering offsets in {0, 1} (then no staggered index needs clipping), a level below 2^31 elements, every search of
// the launch guessed (`guessed`).  The pair copies of a 2-D kernel are the launch's business (ensure_velocity_pairs).
static int32_t fill_fastc(pk_ctx* ctx, const pk_exec_params* prm, KArgs& a, int prog, bool guessed, size_t& lds_bytes) {
    FastC& F = a.fastc;
    memset(&F, 0, sizeof(F));
    const bool want_w = prog == PROG_RK4_3D, rk45 = prog == PROG_RK45, m1 = prog == PROG_M1;
    // the RK4 kernels reset dt every iteration (kernel.py:225-226); in RK45 mode (fieldset.RK45_tol present) dt follows next_dt, which
    // only the RK45 kernel implements -- and AdvectionRK45 itself always runs in that mode (Kernel.check_fieldsets_in_kernels)
    if (ctx->no_fast_cgrid || prm->interp_uv != 1 || (prm->rk45_mode != 0) != rk45) return 0;
    if (rk45 && !ctx->dev.next_dt) return 0;
    if (prm->reset_state && !guessed) return 0;  // an unguessed first search returns float32 (xsi, eta) ARRAYS (GPos::w32)
    const HostField& U = ctx->fields[prm->fU];
    const HostField& V = ctx->fields[prm->fV];
    const HostField* W = (want_w && prm->fW >= 0) ? &ctx->fields[prm->fW] : nullptr;
    if (want_w && !W) return 0;
    const int gid = U.d.grid;
    const HostGrid& g = ctx->grids[gid];
    if (g.d.kind != 1 || !g.d.spherical || g.d.lon_f32 || g.d.lat_f32 || g.d.depth_f32 || !g.d.cell_tab) return 0;
    if (V.d.grid != gid || (W && W->d.grid != gid)) return 0;
    auto same = [](const DField& x, const DField& y) { return x.ncomp == y.ncomp && same_layout(x, y); };
    if (!same(U.d, V.d) || (W && !same(U.d, W->d))) return 0;
    if (V.time != U.time || (W && W->time != U.time)) return 0;
    const DField& f = U.d;
    const int64_t esz = f.dtype == PK_F64 ? 8 : 4;
    if (!g.d.has_x || !g.d.has_y || f.st_x != 1 || f.nx != g.d.nx || f.ny != g.d.ny || g.d.nx < 2 || g.d.ny < 2) return 0;
    if (g.d.xdim <= 1) return 0;  // one cell column: no search is ever guessed (pk_device.h: grid_search)
    for (int o : {g.d.off_x, g.d.off_y, g.d.off_z})
        if (o != 0 && o != 1) return 0;
    if (g.d.has_z) {
        if (g.d.nz < 2 || f.nz < g.d.nz + (W ? g.d.off_z : 0) || g.d.nz >= 4096) return 0;
    } else if (W) {
        return 0;
    }
    if (f.has_time_interval && (f.nt < 2 || U.time.front() != 0.0)) return 0;
    if (f.nt >= (1 << 18)) return 0;
    if ((int64_t)f.st_t >= (1ll << 31)) return 0;
    // `ei` must not wrap (the guess of the next search is the cell itself)
    if ((int64_t)std::max(g.d.xdim, 1) * std::max(g.d.ydim, 1) * std::max(g.d.zdim, 1) >= (1ll << 31)) return 0;
    if (!(g.d.deg2m > 1e-100 && g.d.deg2m < 1e100)) return 0;
    // (next to the per-lane slots in the LDS of a one-wavefront workgroup)
    const CoordTable& T = ctx->tab_c;
    if (int32_t rc = coord_table(ctx, ctx->tab_c, gid, prm->fU, U.time.data(), f.has_time_interval ? f.nt : 0, {{g.d.depth, g.d.has_z ? g.d.nz : 0}},
                                 24 * 1024))
        return rc;
    if (!T.ok) return 0;
    // per-cell records, built once per grid (optional: without the memory for them the general program runs)
    if (ctx->ct2_grid != gid) {
        if (ctx->d_ct2) {
            PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
            (void)hipFree(ctx->d_ct2);
            ctx->d_ct2 = nullptr;
        }
        ctx->ct2_grid = gid;
        const int64_t ncell = (int64_t)(g.d.ny - 1) * g.d.nx;
        if (hipMalloc((void**)&ctx->d_ct2, (size_t)ncell * CT2_STRIDE * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            ctx->d_ct2 = nullptr;
        } else {
            int* d_wide = nullptr;
            int h_wide = 1;
            PK_HIP(ctx, hipMalloc((void**)&d_wide, sizeof(int)));
            PK_HIP(ctx, hipMemsetAsync(d_wide, 0, sizeof(int), ctx->compute));
            hipLaunchKernelGGL(cell_table2_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, ctx->compute, g.d, ctx->d_ct2, d_wide);
            PK_HIP(ctx, hipGetLastError());
            PK_HIP(ctx, hipMemcpyAsync(&h_wide, d_wide, sizeof(int), hipMemcpyDeviceToHost, ctx->compute));
            PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
            (void)hipFree(d_wide);
            ctx->ct2_near = h_wide ? 0 : 1;
        }
    }
    if (!ctx->d_ct2) return 0;
    F.grid = gid;
    F.has_ti = f.has_time_interval;
    F.has_z = g.d.has_z;
    F.walk_ok = g.d.walk_ok;
    F.near_edges = ctx->ct2_near;
    F.nt = f.nt;
    F.nslots = f.nslots;
    F.gnz = g.d.nz; F.gny = g.d.ny; F.gnx = g.d.nx;
    ravel_strides(g.d, F.ex, F.ey, F.ez);
    F.st_z = (int32_t)f.st_z;
    F.st_y = (int32_t)f.st_y;
    const int64_t cb = (int64_t)f.ncomp * esz;
    F.cb = (int32_t)cb;
    F.lvl_b = (int64_t)f.st_t * cb;
    const int64_t oz = g.d.has_z ? g.d.off_z : 0;
    F.dU0 = (int64_t)g.d.off_y * f.st_y * cb + (int64_t)U.d.comp * esz;
    F.dU1 = F.dU0 + cb;
    F.dV0 = (int64_t)g.d.off_x * cb + (int64_t)V.d.comp * esz;
    F.dV1 = F.dV0 + (int64_t)f.st_y * cb;
    if (W) {
        F.dW0 = (oz * f.st_z + (int64_t)g.d.off_y * f.st_y + g.d.off_x) * cb + (int64_t)W->d.comp * esz;
        F.dW1 = F.dW0 + (int64_t)f.st_z * cb;
    }
    F.U = (const char*)U.d.data; F.V = (const char*)V.d.data; F.W = W ? (const char*)W->d.data : nullptr;
    F.ct2 = ctx->d_ct2;
    F.tab = T.d;
    if (m1) {  // AdvectionDiffusionM1: Kh_zonal / Kh_meridional as XLinear fields on the nodes of the same grid
        const int ids[2] = {prm->fKh_zonal, prm->fKh_meridional};
        for (int k = 0; k < 2; k++) {
            if (ids[k] < 0 || ids[k] >= (int)ctx->fields.size()) return 0;
            const HostField& K = ctx->fields[ids[k]];
            const DField& kd = K.d;
            if (kd.grid != gid || kd.dtype != f.dtype || kd.ncomp != 1 || kd.is_const != 0 || kd.st_x != 1 || kd.nx != g.d.nx || kd.ny != g.d.ny) return 0;
            if (!(kd.nz == 1 || kd.nz == g.d.nz)) return 0;
            if (kd.has_time_interval && (K.time != U.time || kd.nt != f.nt)) return 0;
            if (!kd.has_time_interval && kd.nt != 1) return 0;
            if ((int64_t)kd.st_t * esz >= (1ll << 31)) return 0;
            F.kh[k] = (const char*)kd.data;
            F.kh_st[k] = (int32_t)(kd.st_t * esz);
            F.kh_sz[k] = (int32_t)(kd.st_z * esz);
            F.kh_sy[k] = (int32_t)(kd.st_y * esz);
            F.kh_nt[k] = kd.nt; F.kh_nz[k] = kd.nz; F.kh_ny[k] = kd.ny; F.kh_nx[k] = kd.nx;
            F.kh_has_ti[k] = kd.has_time_interval;
            F.kh_nslots[k] = kd.nslots;
        }
    }
    F.lds_time = T.off[0]; F.lds_depth = T.off[1]; F.lds_n = T.off[2];
    F.lds_rec = 2 * F.lds_n;
    const int cm = m1 ? CG_CACHE_M1 : (rk45 ? CG_CACHE_RK45 : CG_CACHE_RK4);  // which parts of a lane's cell cache the kernel keeps in registers
    F.lds_fv = F.lds_rec + fc_rec_rows(cm) * FC_LANES;
    lds_bytes = (size_t)F.lds_fv * sizeof(double) + (size_t)fc_fv_lds(cm) * FC_LANES * (size_t)esz;
    F.tlen = f.tlen; F.t0 = f.tfirst; F.t1 = f.tlast;
    F.z0 = g.d.zfirst; F.z1 = g.d.zlast;
    F.deg2m = g.d.deg2m;
    F.ok = 1;
    return 0;
}

// A kernel list WITH user kernels may still run in the dedicated A-grid kernel (the module carries an instantiation with the user kernels
// as side kernels, pk_kernels.h: side_kernel): exactly one AdvectionRK4 / AdvectionRK4_3D anywhere in the list, everything else a
// sampling-free recovery kernel or a user kernel, and a module whose user kernels sample no field.  -1: no; 0 / 1: yes, 2-D / 3-D.
static int user_fast_shape(const pk_exec_params* prm, int32_t user_flags) {
    if (!(user_flags & PK_USER_RIDE) || prm->body_only) return -1;
    int nadv = 0, d3 = 0;
    for (int k = 0; k < prm->nk; k++) {
        const int id = prm->kernels[k];
        if (id == PK_KERNEL_ADVECTION_RK4 || id == PK_KERNEL_ADVECTION_RK4_3D) {
            nadv++;
            d3 = id == PK_KERNEL_ADVECTION_RK4_3D;
        } else if (!(id == PK_KERNEL_DELETE_ON_ERROR || id == PK_KERNEL_DELETE_OUT_OF_BOUNDS || (id >= PK_KERNEL_USER0 && id < PK_KERNEL_USER0 + PK_MAX_USER_KERNELS))) {
            return -1;
        }
    }
    if (nadv != 1) return -1;
    if ((user_flags & PK_USER_SAMPLES_UVW) && !d3) return -1;  // a 2-D host kernel carries no W
    return d3;
}
// the scalar fields a riding module samples must look exactly like U to the dedicated A-grid kernel: same grid, dtype, layout, time axis,
// ring, XLinear -- then only the base pointer differs (FastA::S)
static bool fill_fast_scalars(pk_ctx* ctx, const pk_exec_params* prm, FastA& F, int nsample, const int32_t* fids) {
    if (nsample < 0 || nsample > 4) return false;
    const HostField& U = ctx->fields[prm->fU];
    F.ns = 0;
    for (int k = 0; k < nsample; k++) {
        const int fid = fids[k];
        if (fid < 0 || fid >= (int)ctx->fields.size()) return false;
        const HostField& S = ctx->fields[fid];
        if (S.d.grid != U.d.grid || S.d.ncomp != 1 || S.d.is_const != 0 || !same_layout(S.d, U.d) || S.time != U.time) return false;
        F.sfid[F.ns] = fid;
        F.S[F.ns] = (const char*)S.d.data;
        F.ns++;
    }
    return true;
}

// What is known about the user kernels when a launch is planned: pk_execute_begin plans the launch at hand with what pk_set_user_program
// registered; pk_generic_variant plans for the module about to be built, which has to serve every launch of its list.
struct UserShape {
    bool present;          // the list holds user kernels (only such a list may ride in a dedicated kernel)
    int32_t flags;         // PK_USER_RIDE | PK_USER_SAMPLES_* | PK_USER_UX | PK_USER_SIGMA
    int nsample;           // scalar fields the user kernels sample: fids[0 .. nsample)
    const int32_t* fids;
    bool assume_guessed;   // plan as if the first search were guessed (the module is also launched after the unguessed first launch)
    bool assume_unlisted;  // plan as if no time-error key were listed (a listed launch runs the interpreter every module carries)
};

struct LaunchPlan {
    int prog = PROG_GENERIC;             // PROG_* (pk_kernels.h)
    Dedicated kernel = DEDICATED_NONE;   // the dedicated kernel that runs it, if any (a.fast / a.fastc filled)
    bool ride = false;                   // the user kernels ride in that dedicated kernel (else they run in the interpreter)
    size_t lds = 0;                      // dynamic LDS bytes of the kernel that runs
    int lp = FAST_LP_OFF;                // DEDICATED_A2: FAST_LP_* mode of the kernel (pk_fast_agrid.h)
};

// Which program and which kernel run a launch with `prm`, given the launch arguments (launch_args) and what is known about the user kernels.
// Device work only for the one-time builds of the coordinate tables and of the C-grid cell table.
static int32_t plan_launch(pk_ctx* ctx, const pk_exec_params* prm, const UserShape& us, KArgs& a, size_t lds_bytes, int use_lds, LaunchPlan& p) {
    p = LaunchPlan{PROG_GENERIC, DEDICATED_NONE, false, lds_bytes, FAST_LP_OFF};
    if (ctx_has_ugrid(ctx)) {  // a fieldset on a UxGrid: the unstructured program (pk_ux.h) and nothing else
        if (ctx->grids[a.main_grid].d.kind != PK_UX_KIND) return ctx->fail("a launch on a context with a UxGrid needs its velocity on the UxGrid");
        if (us.present && (us.flags & PK_USER_SIGMA))
            return ctx->fail("the registered user program was built for the CROCO sigma loop: a launch on a UxGrid needs the UxGrid variant (PK_USER_UX)");
        if (us.present && !(us.flags & PK_USER_UX))
            return ctx->fail("the registered user program was built for a structured grid: a launch on a UxGrid needs the UxGrid variant (PK_USER_UX)");
        if (prm->rk45_mode) return ctx->fail("AdvectionRK45 is not implemented on a UxGrid");
        if (prm->interp_uv != 4) return ctx->fail("the velocity on a UxGrid is interpolated with Ux_Velocity (interp_uv 4)");
        for (int k = 0; k < prm->nk; k++) {
            const int id = prm->kernels[k];
            if (id == PK_KERNEL_ADVECTION_RK45 || id == PK_KERNEL_SUBMERGE_THROUGH_SURFACE)
                return ctx->fail("this built-in kernel is not implemented on a UxGrid");
        }
        p.prog = PROG_UX;
        p.lds = 0;
        return 0;
    }
    if (us.present && (us.flags & PK_USER_UX)) return ctx->fail("the registered user program was built for a UxGrid: it cannot run a launch on a structured grid");
    bool croco = false;
    for (int k = 0; k < prm->nk; k++) croco = croco || prm->kernels[k] == PK_KERNEL_ADVECTION_RK2_3D_CROCO || prm->kernels[k] == PK_KERNEL_SAMPLE_SIGMA_CROCO;
    // a user module that carries the sigma loop (its kernels may call convert_z_to_sigma_croco) makes its list one, CROCO id or not
    const bool sigma_module = us.present && (us.flags & PK_USER_SIGMA);
    if (sigma_module && !croco && !ctx->has_sigma)
        return ctx->fail("the registered user program was built for the CROCO sigma loop: it runs a list on a context with CROCO parameters only (pk_set_croco)");
    if (croco || sigma_module) {  // the sigma-grid program (pk_sigma.h), whatever built-in kernels stand beside the CROCO kernels
        if (!ctx->has_sigma) return ctx->fail("a CROCO kernel needs the CROCO parameters of the context (pk_set_croco)");
        if (us.present && !sigma_module)
            return ctx->fail("the registered user program was built for the kernel-list interpreter: a list with a CROCO kernel needs the sigma variant (PK_USER_SIGMA)");
        if (ctx_is_typed(ctx)) return ctx->fail("the CROCO kernels need float64 coordinate arrays");
        if (prm->interp_uv != 0 && prm->interp_uv != 1) return ctx->fail("the CROCO program interpolates the velocity with XLinear_Velocity or CGrid_Velocity");
        p.prog = PROG_SIGMA;
        p.lds = (size_t)ctx->sigma.n * 2 * sizeof(double);
        a.sigma = ctx->sigma;
        return 0;
    }
    bool rest_policy = true;  // entries after the first are the sampling-free recovery kernels
    for (int k = 1; k < prm->nk; k++)
        rest_policy = rest_policy && (prm->kernels[k] == PK_KERNEL_DELETE_ON_ERROR || prm->kernels[k] == PK_KERNEL_DELETE_OUT_OF_BOUNDS);
    if (rest_policy && use_lds) {
        if (prm->kernels[0] == PK_KERNEL_ADVECTION_RK4) p.prog = PROG_RK4;
        if (prm->kernels[0] == PK_KERNEL_ADVECTION_RK4_3D) p.prog = PROG_RK4_3D;
        if (prm->kernels[0] == PK_KERNEL_ADVECTION_RK45 && !ctx->no_special) p.prog = PROG_RK45;
        if (prm->kernels[0] == PK_KERNEL_ADVECTIONDIFFUSION_M1 && !ctx->no_special) p.prog = PROG_M1;
    }
    if (prm->body_only) p.prog = PROG_GENERIC;  // only the kernel-list interpreter knows the mode
    const bool typed = ctx_is_typed(ctx);
    if (typed) p.prog = PROG_TYPED;
    const bool curv = ctx->grids[a.main_grid].d.kind == 1;
    // A launch that knows samples which fail call-wide (pk_exec_params.twe_key: the repeat of a call in which some particle left a
    // field's time interval) runs the general programs: only they test the list (the dedicated kernels report such samples and pay
    // nothing else for it); same results otherwise, which the parity tests hold them to at rtol 0.  (Round 6 built the list test into the
    // dedicated kernels -- one scalar bit test per sample when nothing is listed -- held it bit-identical and measured it: +2.4 % on the
    // headline kernel, +0.6 % / +1 % on RK45 / M1 through the register allocation alone (profiles/r06e_summary.txt), for repeats that only
    // a run past the last time level makes.  Not kept.)
    const bool listed = prm->twe_n > 0 && !us.assume_unlisted;
    const int ufast = (us.present && use_lds && !listed && !typed) ? user_fast_shape(prm, us.flags) : -1;
    const bool user_samples = us.nsample > 0 || (us.flags & (PK_USER_SAMPLES_UV | PK_USER_SAMPLES_UVW));
    // the program a dedicated kernel is asked to run: the user kernels' advection kernel, or the program of a list without user kernels
    int fast_prog = -1;
    const bool ride = ufast >= 0 && (!curv || !user_samples);
    if (ride) fast_prog = ufast ? PROG_RK4_3D : PROG_RK4;
    else if (!listed && (p.prog == PROG_RK4 || p.prog == PROG_RK4_3D || (curv && (p.prog == PROG_RK45 || p.prog == PROG_M1)))) fast_prog = p.prog;
    if (fast_prog < 0) return 0;
    if (!curv) {
        if (int32_t rc = fill_fast(ctx, prm, a, fast_prog)) return rc;
        if (ride && a.fast.ok && !fill_fast_scalars(ctx, prm, a.fast, us.nsample, us.fids)) a.fast.ok = 0;
        if (!a.fast.ok) return 0;
        p.kernel = fast_prog == PROG_RK4_3D ? DEDICATED_A3 : DEDICATED_A2;
        // the A-grid kernel's LDS: the coordinate tables and, behind them (2-D kernels), the per-lane corner cache.  The level-pair cache
        // (128 bytes per lane, 512-lane workgroups) when two workgroups -- 16 waves, the residency of the kernel without it -- fit in the
        // CU's LDS (allocated in 2 KB steps at most); otherwise exactly the older choice: the stage-pair block (64 bytes per lane) when it fits
        // in the 64 KB a workgroup gets by default, else nothing.  Only the library's own lean 2-D kernel has the level-pair modes: the 3-D
        // kernel moves z, and a module that carries user kernels keeps the arithmetic order of the general program.
        p.lds = (size_t)a.fast.lds_n * 2 * sizeof(double);
        const bool lp_kernel = fast_prog == PROG_RK4 && !ride;
        const size_t lp_lds = (p.lds + (size_t)FAST_LP_BYTES + 2047) / 2048 * 2048;
        const bool lp_fits = 2 * lp_lds <= (size_t)160 * 1024;  // gfx950: 160 KiB per CU
        int mode = ctx->block_cache;
        if (ctx->no_block_cache && mode != 2) mode = 0;
        if (mode == 2 && !(lp_kernel && lp_fits))
            return ctx->fail(!lp_kernel ? "block_cache 2: only the library's 2-D A-grid kernel (AdvectionRK4 without user kernels) has the level-pair cache"
                                        : "block_cache 2: the coordinate tables leave no room for the level-pair cache at 16 waves per CU");
        if (mode < 0) mode = lp_kernel && lp_fits ? 2 : 1;
        if (mode == 2) {
            p.lp = FAST_LP_CACHE;
            a.fast.lds_blk = a.fast.lds_n;
            a.fast.miss_lanes = ctx->miss_lanes < 0 ? FAST_MISS_LANES_DEFAULT : ctx->miss_lanes;  // (same bits at every value: a speed knob)
            p.lds += (size_t)FAST_LP_BYTES;
        } else if (mode == 0 && lp_kernel && !ctx->no_block_cache) {
            p.lp = FAST_LP_REGS;  // the cache's arithmetic without the cache: on / off is bit-identical
            a.fast.lds_blk = 0;
        } else {
            const bool blk = mode == 1 && fast_prog != PROG_RK4_3D && p.lds + (size_t)FAST_BLK_BYTES <= 64 * 1024;
            a.fast.lds_blk = blk ? a.fast.lds_n : 0;
            if (blk) p.lds += (size_t)FAST_BLK_BYTES;
        }
    } else {
        if (int32_t rc = fill_fastc(ctx, prm, a, fast_prog, prm->have_guess0 || us.assume_guessed, p.lds)) return rc;
        if (!a.fastc.ok) return 0;
        p.kernel = fast_prog == PROG_RK4_3D ? DEDICATED_C3 : DEDICATED_C2;
    }
    p.prog = fast_prog;
    p.ride = ride;
    return 0;
}

// The programs without a dedicated kernel
static void launch_general(int prog, int field_f32, int curv, const pk_exec_params* prm, int use_lds, const KArgs& a, dim3 grid, size_t lds_bytes, hipStream_t s) {
    switch (prog) {
        case PROG_RK4: launch_program<PROG_RK4>(field_f32, curv, prm->interp_uv, use_lds, a, grid, lds_bytes, s); break;
        case PROG_RK4_3D: launch_program<PROG_RK4_3D>(field_f32, curv, prm->interp_uv, use_lds, a, grid, lds_bytes, s); break;
        case PROG_RK45: launch_program<PROG_RK45>(field_f32, curv, prm->interp_uv, use_lds, a, grid, lds_bytes, s); break;
        case PROG_M1: launch_program<PROG_M1>(field_f32, curv, prm->interp_uv, use_lds, a, grid, lds_bytes, s); break;
        case PROG_TYPED: launch_program<PROG_TYPED>(field_f32, curv, prm->interp_uv, use_lds, a, grid, lds_bytes, s); break;
        default: launch_program<PROG_GENERIC>(field_f32, curv, prm->interp_uv, use_lds, a, grid, lds_bytes, s); break;
    }
}

}  // namespace pkapi

extern "C" {

int32_t pk_execute_begin(pk_ctx* ctx, const pk_exec_params* prm) {
    if (!ctx || !prm) return -2;
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_execute_begin: a launch is already in flight (call pk_execute_end)");
    if (prm->nk < 1 || prm->nk > PK_MAX_KERNELS) return ctx->fail("params.nk out of range");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->fl_clock_probe = false;  // only the branch that launches a probe sets it: no launch path reports the clock of an older launch
    KArgs a;
    size_t lds_bytes = 0;
    int use_lds = 0;
    int32_t rc = launch_args(ctx, prm, a, lds_bytes, use_lds);
    if (rc) return rc;
    // A continued launch says "guessed" for the particles that have stepped; one that paused before its first step still has its first
    // evaluation ahead (pk_kernels.h: first_eval), and that one is guessed iff the call's batch held a guess
    if (prm->reset_state) ctx->call_have_guess0 = prm->have_guess0;
    else if (!prm->body_only) a.prm.have_guess0 = ctx->call_have_guess0;
    rc = upload_descriptors(ctx, a);
    if (rc) return rc;
    bool need_kh = false, has_user = false;
    for (int k = 0; k < prm->nk; k++) {
        const int id = prm->kernels[k];
        if (id == PK_KERNEL_ADVECTIONDIFFUSION_M1 || id == PK_KERNEL_ADVECTIONDIFFUSION_EM || id == PK_KERNEL_DIFFUSION_UNIFORM_KH)
            need_kh = true;
        if (id == PK_KERNEL_ADVECTION_RK45 && !ctx->dev.next_dt) return ctx->fail("AdvectionRK45 needs the next_dt column");
        if (id >= PK_KERNEL_USER0 && id < PK_KERNEL_USER0 + PK_MAX_USER_KERNELS) {
            has_user = true;
            if (!ctx->user_launch) return ctx->fail("a user kernel id without a registered program (pk_set_user_program)");
            if (prm->body_only) return ctx->fail("user kernels do not run in body_only launches");
        }
        if ((id == PK_KERNEL_ADVECTION_RK4_3D || id == PK_KERNEL_ADVECTION_RK2_3D) && prm->fW < 0)
            return ctx->fail("3-D advection needs the W field");
        if (id == PK_KERNEL_ADVECTION_RK2_3D_CROCO && prm->fW < 0) return ctx->fail("AdvectionRK2_3D_CROCO needs the W field");
        if (id == PK_KERNEL_SAMPLE_SIGMA_CROCO) {
            const int sf = prm->sample_field[k], v = prm->sample_var[k];
            if (sf < 0 || sf >= (int)ctx->fields.size()) return ctx->fail("PK_KERNEL_SAMPLE_SIGMA_CROCO: params.sample_field names no scalar field");
            if (v < 0 || v >= ctx->host.n_extra) return ctx->fail("PK_KERNEL_SAMPLE_SIGMA_CROCO: params.sample_var names no extra particle column");
        }
        if (id == PK_KERNEL_SAMPLE_FIELD) {
            const int sf = prm->sample_field[k];
            const bool vec = sf == PK_SAMPLE_UV || sf == PK_SAMPLE_UVW;
            if (!vec && (sf < 0 || sf >= (int)ctx->fields.size())) return ctx->fail("PK_KERNEL_SAMPLE_FIELD: params.sample_field names no field");
            if (sf == PK_SAMPLE_UVW && prm->fW < 0) return ctx->fail("PK_KERNEL_SAMPLE_FIELD: sampling UVW needs the W field");
            const int nv = vec ? (sf == PK_SAMPLE_UVW ? 3 : 2) : 1;
            int stored = 0;
            for (int j = 0; j < nv; j++) {
                const int v = vec ? ((prm->sample_var[k] >> (8 * j)) & 0xFF) : prm->sample_var[k];
                if (vec && v == PK_SAMPLE_DISCARD) continue;
                if (v < 0 || v >= ctx->host.n_extra) return ctx->fail("PK_KERNEL_SAMPLE_FIELD: params.sample_var names no extra particle column");
                stored++;
            }
            if (!stored) return ctx->fail("PK_KERNEL_SAMPLE_FIELD: every component is discarded");
        }
    }
    if (need_kh && (prm->fKh_zonal < 0 || prm->fKh_meridional < 0)) return ctx->fail("diffusion kernels need Kh_zonal/Kh_meridional");
    const HostField& U = ctx->fields[prm->fU];
    const int field_f32 = U.d.dtype == PK_F32;
    for (int f : {prm->fV, prm->fW})
        if (f >= 0 && ctx->fields[f].d.dtype != U.d.dtype) return ctx->fail("U, V, W must share one dtype");
    const int curv = ctx->grids[a.main_grid].d.kind == 1;
    const int64_t n = ctx->dev.n;
    if (prm->twe_n < 0 || prm->twe_n > PK_MAX_TWE || (prm->twe_n > 0 && !prm->twe_key)) return ctx->fail("params.twe_n / twe_key out of range");
    for (int k = 1; k < prm->twe_n; k++)
        if (!(prm->twe_key[k - 1] < prm->twe_key[k])) return ctx->fail("params.twe_key must be ascending");
    DCounters& counters0 = ctx->h_counters0;
    counters0 = DCounters{0ull, 0ull, 0ull, 0xFFFFFFFFu, 0u, ~0ull, 0u, 0u, {}, {}};  // (cursor: the persistent launch claims from chunk 0 of every share)
    PK_HIP(ctx, hipMemcpyAsync(ctx->d_counters, &counters0, sizeof(DCounters), hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemsetAsync(ctx->d_twe_found, 0, sizeof(unsigned long long) * TWE_FOUND_SLOTS, ctx->compute));
    if (prm->twe_n > 0) PK_HIP(ctx, hipMemsetAsync(ctx->d_twe_hit, 0, sizeof(unsigned int) * prm->twe_n, ctx->compute));
    ctx->fl_twe_n = prm->twe_n;
    if (prm->twe_key != ctx->rerun_keys.data()) ctx->rerun_keys.assign(prm->twe_key, prm->twe_key + prm->twe_n);  // (kept for pk_execute_rerun)
    if (prm->twe_n > 0)
        PK_HIP(ctx, hipMemcpyAsync(ctx->d_twe, ctx->rerun_keys.data(), sizeof(int64_t) * prm->twe_n, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemsetAsync(ctx->d_summary, 0, sizeof(unsigned long long) * PK_NUM_STATE_CODES, ctx->compute));
    const unsigned long long init_mm[2] = {~0ull, 0ull};
    PK_HIP(ctx, hipMemcpyAsync(ctx->d_summary + PK_NUM_STATE_CODES, init_mm, sizeof(init_mm), hipMemcpyHostToDevice, ctx->compute));
    int launches = 0;
    bool sorted = false;
    if (n > 0) {
        const dim3 grid((unsigned)((n + 255) / 256));
        LaunchPlan p;
        rc = plan_launch(ctx, prm, UserShape{has_user, ctx->user_flags, ctx->user_nsample, ctx->user_sample_fid, false, false}, a, lds_bytes, use_lds, p);
        if (rc) return rc;
        if (has_user && p.prog == PROG_TYPED) return ctx->fail("user kernels run in the plain kernel-list interpreter only (float32 coordinate arrays are not supported)");
        if (p.kernel == DEDICATED_C2) ensure_velocity_pairs(ctx, prm, a.fastc);
        if (prm->sort_by_cell && !prm->body_only && p.prog != PROG_UX) {
            PK_HIP(ctx, hipEventRecord(ctx->ev2, ctx->compute));
            // curvilinear sort order (measured on the NEMO-size grid): depth-major for 3-D advection (+4 %), horizontal-major
            // (water columns share node-table lines) for 2-D kernels (RK45 +18 %, M1 +28 %); PK_SORT_HORIZONTAL overrides
            int horizontal = 1;
            for (int k = 0; k < prm->nk; k++)
                if (prm->kernels[k] == PK_KERNEL_ADVECTION_RK4_3D || prm->kernels[k] == PK_KERNEL_ADVECTION_RK2_3D) horizontal = 0;
            if (ctx->sort_horizontal_major >= 0) horizontal = ctx->sort_horizontal_major;
            rc = sort_particles(ctx, a.main_grid, horizontal);
            if (rc) return rc;
            a.p = ctx->dev;  // the column pointers were swapped
            sorted = true;
        }
        // the launch reads `dev` and writes the second column set (pk_device.h: DPOut), which then becomes `dev`: the state before
        // the launch survives in `alt` at no cost, for pk_execute_rerun
        rc = ensure_alt(ctx);
        if (rc) return rc;
        a.p = ctx->dev;
#define X(m, bit, elem, per_grid, optional) a.po.m = ctx->alt.m;
        PK_LAUNCH_COLUMNS(X)
#undef X
        a.po.iter = ctx->alt.iter;
        if (!prm->reset_state || prm->body_only) {
            // a continued (paused) call or a masked body launch: some rows are not stepped -- they keep their values by this
            // device-to-device copy of the columns a launch writes (the kernels themselves carry no copy code: pk_kernels.h)
            for (const ColRef& c : particle_columns(ctx))
                if (c.launch_output && c.d && c.a)
                    PK_HIP(ctx, hipMemcpyAsync(c.a, c.d, (size_t)n * c.elem * c.width, hipMemcpyDeviceToDevice, ctx->compute));
        }
        if (ctx->clock_probe) {  // the probe may start once everything queued before the advection kernel is done
            if (!ctx->probe) {
                PK_HIP(ctx, hipStreamCreateWithFlags(&ctx->probe, hipStreamNonBlocking));
                PK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_probe, hipEventDisableTiming));
            }
            PK_HIP(ctx, hipMemsetAsync(ctx->d_clk, 0, sizeof(unsigned long long) * 32, ctx->compute));
            PK_HIP(ctx, hipEventRecord(ctx->ev_probe, ctx->compute));
            PK_HIP(ctx, hipStreamWaitEvent(ctx->probe, ctx->ev_probe, 0));
        }
        PK_HIP(ctx, hipEventRecord(ctx->ev0, ctx->compute));
        const int pf32 = ctx->dev.spatial_f32;
        if (p.ride) ctx->user_launch(&a, p.kernel, field_f32 * 2 + pf32, 1, (uint64_t)p.lds, (void*)ctx->compute);
        else switch (p.kernel) {
            case DEDICATED_A2:
                if (p.lp != FAST_LP_OFF) PK_HIP(ctx, launch_fast_lp(p.lp, field_f32, pf32, a, p.lds, ctx->prop.multiProcessorCount, ctx->fast_grid, ctx->compute));
                else launch_fast<PROG_RK4>(field_f32, pf32, a, grid, p.lds, ctx->compute);
                break;
            case DEDICATED_A3: launch_fast<PROG_RK4_3D>(field_f32, pf32, a, grid, p.lds, ctx->compute); break;
            case DEDICATED_C2:
                if (p.prog == PROG_RK45) launch_cgrid_rk45(field_f32, pf32, a, n, p.lds, ctx->compute);
                else if (p.prog == PROG_M1) launch_cgrid_m1(field_f32, pf32, a, n, p.lds, ctx->compute);
                else launch_cgrid(field_f32, pf32, 0, a, n, p.lds, ctx->compute);
                break;
            case DEDICATED_C3: launch_cgrid(field_f32, pf32, 1, a, n, p.lds, ctx->compute); break;
            case DEDICATED_NONE:
                if (p.prog == PROG_UX && has_user) ctx->user_launch(&a, DEDICATED_NONE, PK_USER_KEY_UX, 0, 0, (void*)ctx->compute);
                else if (p.prog == PROG_UX) launch_ux(pf32, a, n, ctx->compute);
                else if (p.prog == PROG_SIGMA && has_user) ctx->user_launch(&a, DEDICATED_NONE, sigma_key(ctx, prm, a), (int32_t)p.lds, (uint64_t)p.lds, (void*)ctx->compute);
                else if (p.prog == PROG_SIGMA) launch_sigma(field_f32, curv, prm->interp_uv, a, n, p.lds, ctx->compute);
                else if (has_user) ctx->user_launch(&a, DEDICATED_NONE, interp_key(ctx, prm, a), use_lds, (uint64_t)p.lds, (void*)ctx->compute);
                else launch_general(p.prog, field_f32, curv, prm, use_lds, a, grid, p.lds, ctx->compute);
                break;
        }
        PK_HIP(ctx, hipGetLastError());
        PK_HIP(ctx, hipEventRecord(ctx->ev1, ctx->compute));
        if (ctx->clock_probe) {  // beside the kernel that was just queued: spins for clock_probe microseconds (1 -> 1000) of the 100 MHz counter
            const unsigned long long us = ctx->clock_probe == 1 ? 1000ull : (unsigned long long)std::max(ctx->clock_probe, 20);
            hipLaunchKernelGGL(clock_probe_kernel, dim3(16), dim3(64), 0, ctx->probe, ctx->d_clk, us * 100ull);
            PK_HIP(ctx, hipMemcpyAsync(ctx->h_clk, ctx->d_clk, sizeof(unsigned long long) * 32, hipMemcpyDeviceToHost, ctx->probe));
        }
        ctx->fl_clock_probe = ctx->clock_probe != 0;
        launches = 1;
        ctx->fl_program = p.kernel == DEDICATED_NONE ? p.prog : (p.kernel <= DEDICATED_A3 ? PROGRAM_FAST_AGRID : PROGRAM_FAST_CGRID);
        swap_launch_outputs(ctx);
        ctx->rerun_valid = true;
        ctx->rerun_prm = *prm;
        ctx->rerun_prm.twe_key = nullptr;  // (the caller's array may be gone: the keys live in ctx->rerun_keys)
        const unsigned sgrid = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
        hipLaunchKernelGGL(summarize_kernel, dim3(sgrid), dim3(256), 0, ctx->compute, ctx->dev.state, ctx->dev.t, n, ctx->d_summary);
        PK_HIP(ctx, hipGetLastError());
    }
    PK_HIP(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(DCounters), hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(ctx->h_summary, ctx->d_summary, sizeof(unsigned long long) * (PK_NUM_STATE_CODES + 2), hipMemcpyDeviceToHost, ctx->compute));
    ctx->in_flight = true;
    ctx->fl_launches = launches;
    ctx->fl_sorted = sorted;
    ctx->fl_n = n;
    return 0;
}

int32_t pk_execute_end(pk_ctx* ctx, pk_exec_stats* stats) {
    if (!ctx) return -2;
    if (!ctx->in_flight) return ctx->fail("pk_execute_end: no launch in flight");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->in_flight = false;
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    if (ctx->fl_clock_probe && ctx->probe) PK_HIP(ctx, hipStreamSynchronize(ctx->probe));
    {
        // (whether or not the caller wants statistics -- ADVICE r5: pk_execute_twe_report after pk_execute_end(ctx, NULL) returned the keys of
        // an older launch)
        const DCounters& hc = *ctx->h_counters;
        // the cold path of the call-wide time error: every unlisted failing sample the general programs reported, and which listed samples a lane
        // justified (pk_execute_twe_report hands them out) -- copied only when there is something to report
        ctx->twe_found_host.clear();
        ctx->twe_hit_host.assign((size_t)ctx->fl_twe_n, 0);
        ctx->twe_overflow_host = hc.twe_overflow != 0;
        if (ctx->fl_launches && hc.twe_key != ~0ull) {
            std::vector<unsigned long long> slots(TWE_FOUND_SLOTS);
            PK_HIP(ctx, hipMemcpy(slots.data(), ctx->d_twe_found, sizeof(unsigned long long) * TWE_FOUND_SLOTS, hipMemcpyDeviceToHost));
            for (unsigned long long k : slots)
                if (k) ctx->twe_found_host.push_back((int64_t)k);
            std::sort(ctx->twe_found_host.begin(), ctx->twe_found_host.end());
        }
        if (ctx->fl_launches && ctx->fl_twe_n > 0) {
            std::vector<unsigned int> hit((size_t)ctx->fl_twe_n);
            PK_HIP(ctx, hipMemcpy(hit.data(), ctx->d_twe_hit, sizeof(unsigned int) * ctx->fl_twe_n, hipMemcpyDeviceToHost));
            for (int k = 0; k < ctx->fl_twe_n; k++) ctx->twe_hit_host[k] = hit[k] ? 1 : 0;
        }
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        const DCounters& hc = *ctx->h_counters;
        const unsigned long long* hs = ctx->h_summary;
        stats->steps = (int64_t)hc.steps;
        stats->attempts = (int64_t)hc.attempts;
        stats->paused = (int64_t)hc.paused;
        for (int k = 0; k < PK_NUM_STATE_CODES; k++) stats->state_counts[k] = (int64_t)hs[k];
        auto unorder = [](unsigned long long o) {
            unsigned long long b = (o & 0x8000000000000000ull) ? (o & 0x7fffffffffffffffull) : ~o;
            double v;
            memcpy(&v, &b, 8);
            return v;
        };
        const bool any_live = ctx->fl_n > 0 && hs[PK_EVALUATE] > 0;
        stats->t_min_live = any_live ? unorder(hs[PK_NUM_STATE_CODES]) : NAN;
        stats->t_max_live = any_live ? unorder(hs[PK_NUM_STATE_CODES + 1]) : NAN;
        float ms = 0.f;
        if (ctx->fl_launches) PK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        stats->kernel_ms = ms;
        float sms = 0.f;
        if (ctx->fl_sorted) PK_HIP(ctx, hipEventElapsedTime(&sms, ctx->ev2, ctx->ev0));
        stats->sort_ms = sms;
        stats->launches = ctx->fl_launches;
        stats->program = ctx->fl_launches ? ctx->fl_program : 0;
        stats->first_error_iter = (ctx->fl_launches && hc.err_iter != 0xFFFFFFFFu) ? (int64_t)hc.err_iter : 0;
        stats->first_time_error_key = (ctx->fl_launches && hc.twe_key != ~0ull) ? (int64_t)hc.twe_key : 0;
        // shader clock beside the advection kernel: cycles per 100 MHz tick of every probe wavefront (the median of the 16)
        double sclk = 0.0;
        int nx = 0;
        if (ctx->fl_launches && ctx->fl_clock_probe) {
            std::vector<double> v;
            for (int k = 0; k < 16; k++) {
                const unsigned long long dc = ctx->h_clk[k * 2], dr = ctx->h_clk[k * 2 + 1];
                if (dc && dr) v.push_back((double)dc / (double)dr * 100.0);
            }
            if (!v.empty()) {
                std::sort(v.begin(), v.end());
                sclk = v[v.size() / 2];
                nx = 1;
            }
        }
        stats->sclk_mhz = nx ? sclk / nx : 0.0;
        float pms = 0.f;
        if (ctx->fl_packs) PK_HIP(ctx, hipEventElapsedTime(&pms, ctx->ev_p0, ctx->ev_p1));
        stats->pack_ms = pms;
        stats->packs = ctx->fl_packs;
    }
    ctx->fl_packs = 0;
    return 0;
}

int32_t pk_execute_twe_report(pk_ctx* ctx, int64_t* found, int32_t cap, int32_t* n_found, uint8_t* listed_hit, int32_t n_listed) {
    if (!ctx || !n_found || cap < 0 || n_listed < 0 || (cap > 0 && !found) || (n_listed > 0 && !listed_hit)) return -2;
    if (ctx->in_flight) return ctx->fail("pk_execute_twe_report: a launch is in flight (call pk_execute_end)");
    const int32_t nf = (int32_t)ctx->twe_found_host.size();
    *n_found = ctx->twe_overflow_host ? -1 : nf;  // -1: more distinct keys than the set holds (trust pk_exec_stats.first_time_error_key only)
    for (int32_t k = 0; k < nf && k < cap; k++) found[k] = ctx->twe_found_host[k];
    for (int32_t k = 0; k < n_listed; k++) listed_hit[k] = k < (int32_t)ctx->twe_hit_host.size() ? ctx->twe_hit_host[k] : 0;
    return 0;
}

int32_t pk_generic_variant(pk_ctx* ctx, const pk_exec_params* prm, int32_t sample_flags, int32_t nsample, const int32_t* sample_fids, int32_t* key,
                           int32_t* lds, int32_t* typed, int32_t* fast) {
    if (!ctx || !prm || !key || !lds || !typed || !fast || (nsample > 0 && !sample_fids)) return -2;
    KArgs a;
    size_t lds_bytes = 0;
    int use_lds = 0;
    int32_t rc = launch_args(ctx, prm, a, lds_bytes, use_lds, true);
    if (rc) return rc;
    // the module serves every launch of the list: it is asked about as a list with user kernels that may ride
    const bool ux = ctx->grids[a.main_grid].d.kind == PK_UX_KIND;  // (the module about to be built is the one this context needs)
    // ... a list with a CROCO kernel, or user kernels that convert depths to sigma levels (sample_flags announces them: PK_USER_SIGMA), needs the sigma loop
    bool sigma = (sample_flags & PK_USER_SIGMA) != 0;
    for (int k = 0; k < prm->nk; k++) sigma = sigma || prm->kernels[k] == PK_KERNEL_ADVECTION_RK2_3D_CROCO || prm->kernels[k] == PK_KERNEL_SAMPLE_SIGMA_CROCO;
    sigma = sigma && !ux;
    const UserShape us{true, (ux ? PK_USER_UX : (sigma ? PK_USER_SIGMA : PK_USER_RIDE)) | (sample_flags & (PK_USER_SAMPLES_UV | PK_USER_SAMPLES_UVW)), nsample, sample_fids, true, true};
    LaunchPlan p;
    rc = plan_launch(ctx, prm, us, a, lds_bytes, use_lds, p);
    if (rc) return rc;
    *key = p.prog == PROG_SIGMA ? sigma_key(ctx, prm, a) : interp_key(ctx, prm, a);
    *lds = ux ? 0 : (p.prog == PROG_SIGMA ? (int32_t)p.lds : use_lds);
    *typed = ctx_is_typed(ctx) ? 1 : 0;
    *fast = p.ride ? p.kernel : DEDICATED_NONE;
    return 0;
}
int32_t pk_set_user_program(pk_ctx* ctx, void* launcher, int32_t flags, int32_t nsample, const int32_t* sample_fids) {
    if (!ctx) return -2;
    if (ctx->in_flight) return ctx->fail("pk_set_user_program: a launch is in flight (call pk_execute_end)");
    if (nsample < 0 || nsample > 4 || (nsample > 0 && !sample_fids)) return ctx->fail("pk_set_user_program: 0 .. 4 sampled scalar fields");
    ctx->user_launch = (void (*)(const void*, int32_t, int32_t, int32_t, uint64_t, void*))launcher;
    ctx->user_flags = launcher ? flags : 0;
    ctx->user_nsample = launcher ? nsample : 0;
    for (int k = 0; k < 4; k++) ctx->user_sample_fid[k] = (launcher && k < nsample) ? sample_fids[k] : 0;
    return 0;
}

int32_t pk_execute_rerun(pk_ctx* ctx, int32_t max_iters, pk_exec_stats* stats) {
    if (!ctx) return -2;
    if (ctx->in_flight) return ctx->fail("pk_execute_rerun: a launch is in flight (call pk_execute_end)");
    if (!ctx->rerun_valid) return ctx->fail("pk_execute_rerun: the state before the last launch is gone (it must directly follow pk_execute / pk_execute_end)");
    if (max_iters < 1) return ctx->fail("pk_execute_rerun: max_iters must be >= 1");
    swap_launch_outputs(ctx);  // `dev` is the state the launch read again (cell-sorted if it sorted: the permutation is unchanged)
    pk_exec_params prm = ctx->rerun_prm;
    prm.sort_by_cell = 0;
    prm.max_iters = max_iters;
    prm.twe_key = ctx->rerun_keys.data();  // (twe_n is the launch's)
    int32_t rc = pk_execute_begin(ctx, &prm);
    if (rc) return rc;
    return pk_execute_end(ctx, stats);
}

int32_t pk_execute_rerun_keys(pk_ctx* ctx, int32_t max_iters, int32_t n_keys, const int64_t* keys, pk_exec_stats* stats) {
    if (!ctx) return -2;
    if (ctx->in_flight) return ctx->fail("pk_execute_rerun_keys: a launch is in flight (call pk_execute_end)");
    if (!ctx->rerun_valid) return ctx->fail("pk_execute_rerun_keys: the state before the last launch is gone (it must directly follow pk_execute / pk_execute_end)");
    if (max_iters < 0) return ctx->fail("pk_execute_rerun_keys: max_iters must be >= 0");
    if (n_keys < 0 || n_keys > PK_MAX_TWE || (n_keys > 0 && !keys)) return ctx->fail("pk_execute_rerun_keys: 0 .. PK_MAX_TWE keys");
    swap_launch_outputs(ctx);  // (see pk_execute_rerun)
    pk_exec_params prm = ctx->rerun_prm;
    prm.sort_by_cell = 0;
    prm.max_iters = max_iters;
    prm.twe_n = n_keys;
    prm.twe_key = keys;
    int32_t rc = pk_execute_begin(ctx, &prm);
    if (rc) return rc;
    return pk_execute_end(ctx, stats);
}

int32_t pk_execute(pk_ctx* ctx, const pk_exec_params* prm, pk_exec_stats* stats) {
    int32_t rc = pk_execute_begin(ctx, prm);
    if (rc) return rc;
    return pk_execute_end(ctx, stats);
}

int32_t pk_measure_copy_bandwidth(pk_ctx* ctx, int64_t bytes, int32_t iters, double* gbps) {
    if (!ctx || !gbps || bytes < 16 || iters < 1) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    void *src = nullptr, *dst = nullptr;
    const int64_t n16 = bytes / 16;
    PK_HIP(ctx, hipMalloc(&src, n16 * 16));
    PK_HIP(ctx, hipMalloc(&dst, n16 * 16));
    PK_HIP(ctx, hipMemsetAsync(src, 1, n16 * 16, ctx->compute));
    const unsigned grid = (unsigned)((n16 + 1023) / 1024);
    hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, ctx->compute, (const float4*)src, (float4*)dst, n16);
    PK_HIP(ctx, hipEventRecord(ctx->ev0, ctx->compute));
    for (int k = 0; k < iters; k++)
        hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, ctx->compute, (const float4*)src, (float4*)dst, n16);
    PK_HIP(ctx, hipEventRecord(ctx->ev1, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    float ms = 0.f;
    PK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *gbps = (2.0 * (double)n16 * 16.0 * iters) / ((double)ms * 1e-3) / 1e9;
    PK_HIP(ctx, hipFree(src));
    PK_HIP(ctx, hipFree(dst));
    return 0;
}

}  // extern "C"
