// pk_density.hip -- particles per grid cell on the device-resident particle columns (pk_density.h).
//
// Two paths, because the two results have different algebra:
//   counts  integer adds commute, so the key kernel counts as it goes: the lanes of a wavefront whose neighbours share a cell form a run,
//           and one 64-bit atomic add per run carries the run length (after a cell sort most of a wavefront is one run).
//   sums    float64 adds do not commute and np.bincount adds in row order: the key kernel stores (cell + 1) << 32 | host row, a radix sort
//           over the bits in use orders them, and one wavefront per cell adds the cell's weights in ascending host row order.
// The cell rule (density_cell) lives in pk_density_cell.h, which pk_connectivity.hip includes too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pk_density_cell.h"

#include "pk_density.h"

namespace pk {

// One lane per device row.  COUNT: add the runs of equal cells to `counts`; else store the sort pair of the row.
// stats: {rows outside, atomic adds issued}, one add of each per workgroup.
// LDSH (counts only): the runs go into a workgroup-private histogram in LDS that is flushed with one global add per non-zero bin.
template <int PFM, bool COUNT, bool LDSH = false>
__global__ void __launch_bounds__(DENS_WG) density_key_kernel(const DGrid g, const DensityColumns c, int levels, int dx, int dy, int dz,
                                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ keys,
                                                              uint32_t* __restrict__ rows, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_out, s_atom;
    extern __shared__ unsigned int s_hist[];  // LDSH: one bin per cell
    if (threadIdx.x == 0) s_out = s_atom = 0ull;
    const int nbins = dx * dy * dz;
    if (LDSH)
        for (int k = threadIdx.x; k < nbins; k += DENS_WG) s_hist[k] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long n_out = 0, n_atom = 0;  // per wavefront, kept by lane 0
    const int64_t npad = (c.n + DENS_WG - 1) / DENS_WG * DENS_WG;
    for (int64_t i = (int64_t)blockIdx.x * DENS_WG + threadIdx.x; i < npad; i += (int64_t)gridDim.x * DENS_WG) {
        long long key = DENS_PAD;
        if (i < c.n) {
            const double x = PFM ? (double)((const float*)c.x)[i] : ((const double*)c.x)[i];
            const double y = PFM ? (double)((const float*)c.y)[i] : ((const double*)c.y)[i];
            double z = g.zfirst;  // without levels the column is not read: the X / Y / FACE indices do not depend on z
            if (levels) z = PFM ? (double)((const float*)c.z)[i] : ((const double*)c.z)[i];
            key = density_cell(g, levels != 0, z, y, x, dx, dy, dz);
        }
        const unsigned long long outside = __ballot(key == -1);
        if (COUNT) {
            // runs of equal keys inside the wavefront: a head is a lane whose key differs from the lane below it
            const long long prev = __shfl_up(key, 1);
            const bool head = lane == 0 || key != prev;
            const unsigned long long heads = __ballot(head);
            const unsigned long long adders = __ballot(head && key >= 0);
            if (head && key >= 0) {
                const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
                const int len = above ? __ffsll((long long)above) : 64 - lane;  // distance to the next head, or to the end of the wavefront
                if (LDSH) atomicAdd(&s_hist[key], (unsigned int)len);
                else atomicAdd(&counts[key], (unsigned long long)len);
            }
            if (!LDSH && lane == 0) n_atom += (unsigned long long)__popcll(adders);
        } else if (i < c.n) {
            const unsigned long long hrow = c.perm ? (unsigned long long)c.perm[i] : (unsigned long long)i;
            keys[i] = ((unsigned long long)(key + 1) << 32) | hrow;
            rows[i] = (uint32_t)i;
        }
        if (lane == 0) n_out += (unsigned long long)__popcll(outside);
    }
    if (lane == 0) {
        if (n_out) atomicAdd(&s_out, n_out);
        if (n_atom) atomicAdd(&s_atom, n_atom);
    }
    __syncthreads();
    if (LDSH) {
        unsigned long long flushed = 0;
        for (int k = threadIdx.x; k < nbins; k += DENS_WG) {
            const unsigned int v = s_hist[k];
            if (v) {
                atomicAdd(&counts[k], (unsigned long long)v);
                flushed++;
            }
        }
        if (flushed) atomicAdd(&s_atom, flushed);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_out) atomicAdd(&stats[0], s_out);
        if (s_atom) atomicAdd(&stats[1], s_atom);
    }
}

PK_DEV double density_weight(const DensityWeights& w, unsigned long long key, uint32_t row) {
    if (w.kind == PK_DENSITY_W_HOST) return w.host[(uint32_t)key];  // host row order: the low half of the key
    switch (w.dtype) {
        case PK_DENSITY_F32: return (double)((const float*)w.dev)[row];
        case PK_DENSITY_F64: return ((const double*)w.dev)[row];
        case PK_DENSITY_I32: return (double)((const int32_t*)w.dev)[row];
        default: return (double)((const int64_t*)w.dev)[row];
    }
}

// first index in [0, n) whose key is not below `bound`
PK_DEV int64_t density_lower_bound(const unsigned long long* __restrict__ keys, int64_t n, unsigned long long bound) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One wavefront per cell: the segment of the sorted keys that belongs to the cell is loaded 64 rows at a time (coalesced keys and rows, one
// gather of the weights) and added in segment order -- ascending host row -- by every lane alike, so a cell that holds every particle costs
// one pass over them.  out[cell] = 0.0 + w0 + w1 + ..., each add rounded on its own (the library is built with -ffp-contract=off).
__global__ void __launch_bounds__(DENS_WG) density_sum_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ rows,
                                                              int64_t n, const DensityWeights w, int64_t ncells, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * DENS_WG + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * DENS_WG) >> 6;
    for (int64_t cell = wave0; cell < ncells; cell += nwaves) {
        const int64_t b = density_lower_bound(keys, n, (unsigned long long)(cell + 1) << 32);
        const int64_t e = density_lower_bound(keys, n, (unsigned long long)(cell + 2) << 32);
        double acc = 0.0;
        for (int64_t j0 = b; j0 < e; j0 += 64) {
            const int64_t j = j0 + lane;
            const double v = j < e ? density_weight(w, keys[j], rows[j]) : 0.0;
            const int m = (int)((e - j0) < 64 ? (e - j0) : 64);
            for (int k = 0; k < m; k++) acc = acc + __shfl(v, k);
        }
        if (lane == 0) out[cell] = acc;
    }
}

namespace {
struct DensityScratch {  // per call: freed on every way out
    unsigned long long *counts = nullptr, *stats = nullptr, *keys = nullptr, *keys_alt = nullptr;
    uint32_t *rows = nullptr, *rows_alt = nullptr;
    double *sums = nullptr, *w_host = nullptr;
    void* sort_tmp = nullptr;
    hipEvent_t ev[4] = {};
    ~DensityScratch() {
        void* p[] = {counts, stats, keys, keys_alt, rows, rows_alt, sums, w_host, sort_tmp};
        for (void* q : p)
            if (q) (void)hipFree(q);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
}  // namespace

#define DENS_HIP(call)                                                      \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            if (err) *err = std::string(#call) + ": " + hipGetErrorString(e_); \
            return -1;                                                      \
        }                                                                   \
    } while (0)

int density_run(hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const DensityWeights& w, int64_t ncells, void* out,
                int64_t* n_outside, pk_density_info_t* info, std::string* err) {
    int dx, dy, dz;
    density_dims(g, levels, dx, dy, dz);
    if (ncells != (int64_t)dz * dy * dx) {
        if (err) *err = "pk_particles_density: ncells is not the number of cells of the grid";
        return -2;
    }
    if (c.n >= (1ll << 32) || ncells >= (1ll << 31)) {
        if (err) *err = "pk_particles_density: needs n < 2^32 rows and fewer than 2^31 cells (the sort key is (cell + 1) << 32 | host row)";
        return -2;
    }
    const bool weighted = w.kind != PK_DENSITY_W_NONE;
    const int64_t n = c.n;
    if (info) *info = pk_density_info_t{};
    if (n == 0) {
        memset(out, 0, (size_t)ncells * 8);
        *n_outside = 0;
        return 0;
    }
    DensityScratch s;
    for (hipEvent_t& e : s.ev) DENS_HIP(hipEventCreate(&e));
    DENS_HIP(hipMalloc((void**)&s.stats, 16));
    DENS_HIP(hipMemsetAsync(s.stats, 0, 16, stream));
    // grid-stride: enough workgroups to fill the device, few enough that the two per-workgroup statistics adds stay off the clock
    const unsigned blocks = (unsigned)std::min<int64_t>((n + DENS_WG - 1) / DENS_WG, 8192);
    unsigned long long hstats[2] = {0, 0};
    if (!weighted) {
        DENS_HIP(hipMalloc((void**)&s.counts, (size_t)ncells * 8));
        DENS_HIP(hipMemsetAsync(s.counts, 0, (size_t)ncells * 8, stream));
        DENS_HIP(hipEventRecord(s.ev[0], stream));
        // A map of at most DENS_LDS_BINS cells is counted in a workgroup-private LDS histogram: on the contended case (1e7 rows in host order
        // over 4096 cells) every run of it lay below every run without it.  PK_DENSITY_LDS=0 switches it off (A/B runs).
        const char* env = getenv("PK_DENSITY_LDS");
        if (!(env && atoi(env) == 0) && ncells <= DENS_LDS_BINS) {
            const unsigned lblocks = std::min(blocks, 1024u);  // every workgroup flushes up to ncells bins: few, long-lived workgroups
            const size_t lds = (size_t)ncells * 4;
            if (c.f32) hipLaunchKernelGGL((density_key_kernel<1, true, true>), dim3(lblocks), dim3(DENS_WG), lds, stream, g, c, levels, dx, dy, dz, s.counts, nullptr, nullptr, s.stats);
            else hipLaunchKernelGGL((density_key_kernel<0, true, true>), dim3(lblocks), dim3(DENS_WG), lds, stream, g, c, levels, dx, dy, dz, s.counts, nullptr, nullptr, s.stats);
        } else if (c.f32) hipLaunchKernelGGL((density_key_kernel<1, true>), dim3(blocks), dim3(DENS_WG), 0, stream, g, c, levels, dx, dy, dz, s.counts, nullptr, nullptr, s.stats);
        else hipLaunchKernelGGL((density_key_kernel<0, true>), dim3(blocks), dim3(DENS_WG), 0, stream, g, c, levels, dx, dy, dz, s.counts, nullptr, nullptr, s.stats);
        DENS_HIP(hipGetLastError());
        DENS_HIP(hipEventRecord(s.ev[1], stream));
        DENS_HIP(hipMemcpyAsync(out, s.counts, (size_t)ncells * 8, hipMemcpyDeviceToHost, stream));
        DENS_HIP(hipMemcpyAsync(hstats, s.stats, 16, hipMemcpyDeviceToHost, stream));
        DENS_HIP(hipStreamSynchronize(stream));
        float ms = 0.f;
        DENS_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        if (info) info->bin_ms = ms;
    } else {
        DensityWeights wd = w;
        if (w.kind == PK_DENSITY_W_HOST) {
            DENS_HIP(hipMalloc((void**)&s.w_host, (size_t)n * 8));
            DENS_HIP(hipMemcpyAsync(s.w_host, w.host, (size_t)n * 8, hipMemcpyHostToDevice, stream));
            wd.host = s.w_host;
        }
        DENS_HIP(hipMalloc((void**)&s.keys, (size_t)n * 8));
        DENS_HIP(hipMalloc((void**)&s.keys_alt, (size_t)n * 8));
        DENS_HIP(hipMalloc((void**)&s.rows, (size_t)n * 4));
        DENS_HIP(hipMalloc((void**)&s.rows_alt, (size_t)n * 4));
        DENS_HIP(hipMalloc((void**)&s.sums, (size_t)ncells * 8));
        int cell_bits = 1;  // bits of cell + 1 <= ncells
        while ((ncells >> cell_bits) != 0) cell_bits++;
        const unsigned end_bit = 32u + (unsigned)cell_bits;
        rocprim::double_buffer<unsigned long long> kb(s.keys, s.keys_alt);
        rocprim::double_buffer<uint32_t> vb(s.rows, s.rows_alt);
        size_t tmp_bytes = 0;
        DENS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, vb, (size_t)n, 0u, end_bit, stream));
        DENS_HIP(hipMalloc(&s.sort_tmp, tmp_bytes ? tmp_bytes : 16));
        DENS_HIP(hipEventRecord(s.ev[0], stream));
        if (c.f32) hipLaunchKernelGGL((density_key_kernel<1, false>), dim3(blocks), dim3(DENS_WG), 0, stream, g, c, levels, dx, dy, dz, nullptr, s.keys, s.rows, s.stats);
        else hipLaunchKernelGGL((density_key_kernel<0, false>), dim3(blocks), dim3(DENS_WG), 0, stream, g, c, levels, dx, dy, dz, nullptr, s.keys, s.rows, s.stats);
        DENS_HIP(hipGetLastError());
        DENS_HIP(hipEventRecord(s.ev[1], stream));
        DENS_HIP(rocprim::radix_sort_pairs(s.sort_tmp, tmp_bytes, kb, vb, (size_t)n, 0u, end_bit, stream));
        DENS_HIP(hipEventRecord(s.ev[2], stream));
        const unsigned sblocks = (unsigned)std::min<int64_t>((ncells + 3) / 4, 16384);  // 4 wavefronts = 4 cells per workgroup and pass
        hipLaunchKernelGGL(density_sum_kernel, dim3(sblocks), dim3(DENS_WG), 0, stream, kb.current(), vb.current(), n, wd, ncells, s.sums);
        DENS_HIP(hipGetLastError());
        DENS_HIP(hipEventRecord(s.ev[3], stream));
        DENS_HIP(hipMemcpyAsync(out, s.sums, (size_t)ncells * 8, hipMemcpyDeviceToHost, stream));
        DENS_HIP(hipMemcpyAsync(hstats, s.stats, 16, hipMemcpyDeviceToHost, stream));
        DENS_HIP(hipStreamSynchronize(stream));
        float ms[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; k++) DENS_HIP(hipEventElapsedTime(&ms[k], s.ev[k], s.ev[k + 1]));
        if (info) {
            info->bin_ms = ms[0];
            info->sort_ms = ms[1];
            info->sum_ms = ms[2];
        }
    }
    *n_outside = (int64_t)hstats[0];
    if (info) {
        info->n_inside = n - (int64_t)hstats[0];
        info->n_atomics = (int64_t)hstats[1];
    }
    return 0;
}

}  // namespace pk
