// pk_connectivity.hip -- labels of the device rows and origin-to-destination counts (pk_connectivity.h).
//
// One key kernel, three ways to count what it finds.  A row with origin label o in [0, n_origin) and destination label d (d = n_dest: in no
// destination) has key = o * (n_dest + 1) + d, so the rows that are outside ride along as one more column of the matrix.
//   LDS     the n_origin * (n_dest + 1) bins fit the workgroup-private histogram density uses: runs of equal keys of a wavefront are added to
//           it, and every workgroup flushes one 64-bit global add per non-zero bin.
//   global  the same runs, one 64-bit global add each (integer adds commute: exact).
//   sparse  the keys are stored (one sentinel above every valid key for the rows that contribute nothing), radix-sorted over the bits in use
//           and run-length encoded; the number of runs comes back first, then that many keys and counts -- np.unique(..., return_counts=True).
// The cell rule is density's: pk_density_cell.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pk_density_cell.h"

#include "pk_connectivity.h"

namespace pk {

constexpr int CONN_NSTATS = 5;  // rows tracked | tracked rows outside | atomic adds issued | rows with origin >= n_origin | rows whose region label is >= n_dest

struct ConnDev {  // ConnLabels as the kernels see them: every pointer is device memory
    const void* regions;
    const void* origin;
    int32_t regions_i64, origin_i64;
    int32_t origin_host_order;  // origin is indexed by HOST row (through perm); else by device row
    long long n_origin, n_dest;
};

// the label of a cell: the cell, or its entry of the region table; -1 = none
PK_DEV long long conn_label(const ConnDev& l, long long cell) {
    if (cell < 0) return -1;
    if (!l.regions) return cell;
    const long long r = l.regions_i64 ? ((const long long*)l.regions)[cell] : (long long)((const int32_t*)l.regions)[cell];
    return r < 0 ? -1 : r;
}

template <int PFM>
PK_DEV long long conn_row_cell(const DGrid& g, const DensityColumns& c, int levels, int dx, int dy, int dz, int64_t i) {
    const double x = PFM ? (double)((const float*)c.x)[i] : ((const double*)c.x)[i];
    const double y = PFM ? (double)((const float*)c.y)[i] : ((const double*)c.y)[i];
    double z = g.zfirst;  // without levels the column is not read (pk_density.hip)
    if (levels) z = PFM ? (double)((const float*)c.z)[i] : ((const double*)c.z)[i];
    return density_cell(g, levels != 0, z, y, x, dx, dy, dz);
}

// One lane per device row: out[host row] = label of the row.
template <int PFM>
__global__ void __launch_bounds__(DENS_WG) cells_kernel(const DGrid g, const DensityColumns c, const ConnDev l, int levels, int dx, int dy, int dz,
                                                        long long* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * DENS_WG + threadIdx.x; i < c.n; i += (int64_t)gridDim.x * DENS_WG)
        out[c.perm ? c.perm[i] : i] = conn_label(l, conn_row_cell<PFM>(g, c, levels, dx, dy, dz, i));
}

constexpr int CONN_LDS = 0, CONN_GLOBAL = 1, CONN_STORE = 2;

// One lane per device row.  PATH CONN_LDS / CONN_GLOBAL: add the runs of equal keys to the LDS histogram / to `counts` (nbins = n_origin *
// (n_dest + 1) bins); CONN_STORE: keys[i] = the key of the row, or nbins (the sentinel) for a row that contributes nothing.
// Rows with a negative origin and lanes past the last row contribute nothing; neither do rows whose origin is >= n_origin or whose region
// label is >= n_dest, which are counted in `stats` for the caller to refuse.
template <int PFM, int PATH>
__global__ void __launch_bounds__(DENS_WG) conn_key_kernel(const DGrid g, const DensityColumns c, const ConnDev l, int levels, int dx, int dy, int dz,
                                                           unsigned long long* __restrict__ counts, unsigned long long* __restrict__ keys,
                                                           unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_stats[CONN_NSTATS];
    extern __shared__ unsigned int s_hist[];  // CONN_LDS: one bin per key
    if (threadIdx.x < CONN_NSTATS) s_stats[threadIdx.x] = 0ull;
    const long long stride = l.n_dest + 1;
    const long long nbins = l.n_origin * stride;
    if (PATH == CONN_LDS)
        for (int k = threadIdx.x; k < (int)nbins; k += DENS_WG) s_hist[k] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long w_stats[CONN_NSTATS] = {0, 0, 0, 0, 0};  // per wavefront, kept by lane 0
    const int64_t npad = (c.n + DENS_WG - 1) / DENS_WG * DENS_WG;
    for (int64_t i = (int64_t)blockIdx.x * DENS_WG + threadIdx.x; i < npad; i += (int64_t)gridDim.x * DENS_WG) {
        long long key = DENS_PAD;
        bool out = false, above = false, bad = false;
        if (i < c.n) {
            const int64_t r = (l.origin_host_order && c.perm) ? c.perm[i] : i;
            const long long o = l.origin_i64 ? ((const long long*)l.origin)[r] : (long long)((const int32_t*)l.origin)[r];
            above = o >= l.n_origin;
            if (o >= 0 && !above) {
                long long d = conn_label(l, conn_row_cell<PFM>(g, c, levels, dx, dy, dz, i));
                out = d < 0;
                bad = d >= l.n_dest;
                if (out) d = l.n_dest;
                if (!bad) key = o * stride + d;  // < nbins: o < n_origin, d <= n_dest
            }
        }
        const unsigned long long b_in = __ballot(key >= 0), b_out = __ballot(out), b_above = __ballot(above), b_bad = __ballot(bad);
        if (PATH == CONN_STORE) {
            if (i < c.n) keys[i] = key >= 0 ? (unsigned long long)key : (unsigned long long)nbins;
        } else {
            // runs of equal keys inside the wavefront: a head is a lane whose key differs from the lane below it (pk_density.hip)
            const long long prev = __shfl_up(key, 1);
            const bool head = lane == 0 || key != prev;
            const unsigned long long heads = __ballot(head);
            const unsigned long long adders = __ballot(head && key >= 0);
            if (head && key >= 0) {
                const unsigned long long higher = lane == 63 ? 0ull : (heads >> (lane + 1));
                const int len = higher ? __ffsll((long long)higher) : 64 - lane;  // distance to the next head, or to the end of the wavefront
                if (PATH == CONN_LDS) atomicAdd(&s_hist[key], (unsigned int)len);
                else atomicAdd(&counts[key], (unsigned long long)len);
            }
            if (PATH == CONN_GLOBAL && lane == 0) w_stats[2] += (unsigned long long)__popcll(adders);
        }
        if (lane == 0) {
            w_stats[0] += (unsigned long long)__popcll(b_in);
            w_stats[1] += (unsigned long long)__popcll(b_out);
            w_stats[3] += (unsigned long long)__popcll(b_above);
            w_stats[4] += (unsigned long long)__popcll(b_bad);
        }
    }
    if (lane == 0)
        for (int k = 0; k < CONN_NSTATS; k++)
            if (w_stats[k]) atomicAdd(&s_stats[k], w_stats[k]);
    __syncthreads();
    if (PATH == CONN_LDS) {
        unsigned long long flushed = 0;
        for (int k = threadIdx.x; k < (int)nbins; k += DENS_WG) {
            const unsigned int v = s_hist[k];
            if (v) {
                atomicAdd(&counts[k], (unsigned long long)v);
                flushed++;
            }
        }
        if (flushed) atomicAdd(&s_stats[2], flushed);
        __syncthreads();
    }
    if (threadIdx.x < CONN_NSTATS && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

namespace {
struct ConnScratch {  // per call: freed on every way out
    void *regions = nullptr, *origin = nullptr, *sort_tmp = nullptr, *rle_tmp = nullptr;
    long long* labels = nullptr;
    unsigned long long *counts = nullptr, *stats = nullptr, *keys = nullptr, *keys_alt = nullptr, *uniq = nullptr, *runs = nullptr, *nruns = nullptr;
    hipEvent_t ev[4] = {};
    ~ConnScratch() {
        void* p[] = {regions, origin, sort_tmp, rle_tmp, labels, counts, stats, keys, keys_alt, uniq, runs, nruns};
        for (void* q : p)
            if (q) (void)hipFree(q);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
}  // namespace

#define CONN_HIP(call)                                                      \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            if (err) *err = std::string(#call) + ": " + hipGetErrorString(e_); \
            return -1;                                                      \
        }                                                                   \
    } while (0)

// the limits both calls share, the dims, and the device copy of the region table
static int conn_prepare(const char* who, hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const ConnLabels& l, int64_t ncells,
                        ConnScratch& s, ConnDev& d, int& dx, int& dy, int& dz, std::string* err) {
    density_dims(g, levels, dx, dy, dz);
    if (ncells != (int64_t)dz * dy * dx) {
        if (err) *err = std::string(who) + ": ncells is not the number of cells of the grid";
        return -2;
    }
    if (c.n >= (1ll << 32) || ncells >= (1ll << 31)) {
        if (err) *err = std::string(who) + ": needs n < 2^32 rows and fewer than 2^31 cells";
        return -2;
    }
    d = ConnDev{};
    d.n_origin = l.n_origin;
    d.n_dest = l.n_dest;
    if (l.regions) {
        d.regions_i64 = l.regions_dtype == PK_DENSITY_I64;
        const size_t bytes = (size_t)ncells * (d.regions_i64 ? 8 : 4);
        CONN_HIP(hipMalloc(&s.regions, bytes));
        CONN_HIP(hipMemcpyAsync(s.regions, l.regions, bytes, hipMemcpyHostToDevice, stream));
        d.regions = s.regions;
    }
    return 0;
}

int cells_run(hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const ConnLabels& l, int64_t ncells, int64_t* labels_out,
              std::string* err) {
    ConnScratch s;
    ConnDev d;
    int dx, dy, dz;
    if (c.n == 0) return 0;
    if (int rc = conn_prepare("pk_particles_cells", stream, g, c, levels, l, ncells, s, d, dx, dy, dz, err)) return rc;
    const int64_t n = c.n;
    CONN_HIP(hipMalloc((void**)&s.labels, (size_t)n * 8));
    const unsigned blocks = (unsigned)std::min<int64_t>((n + DENS_WG - 1) / DENS_WG, 8192);
    if (c.f32) hipLaunchKernelGGL((cells_kernel<1>), dim3(blocks), dim3(DENS_WG), 0, stream, g, c, d, levels, dx, dy, dz, s.labels);
    else hipLaunchKernelGGL((cells_kernel<0>), dim3(blocks), dim3(DENS_WG), 0, stream, g, c, d, levels, dx, dy, dz, s.labels);
    CONN_HIP(hipGetLastError());
    CONN_HIP(hipMemcpyAsync(labels_out, s.labels, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    CONN_HIP(hipStreamSynchronize(stream));
    return 0;
}

template <int PATH>
static void conn_launch(hipStream_t stream, unsigned blocks, size_t lds, const DGrid& g, const DensityColumns& c, const ConnDev& d, int levels, int dx, int dy,
                        int dz, unsigned long long* counts, unsigned long long* keys, unsigned long long* stats) {
    if (c.f32) hipLaunchKernelGGL((conn_key_kernel<1, PATH>), dim3(blocks), dim3(DENS_WG), lds, stream, g, c, d, levels, dx, dy, dz, counts, keys, stats);
    else hipLaunchKernelGGL((conn_key_kernel<0, PATH>), dim3(blocks), dim3(DENS_WG), lds, stream, g, c, d, levels, dx, dy, dz, counts, keys, stats);
}

int connectivity_run(hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const ConnLabels& l, int64_t ncells, int32_t path,
                     int64_t* dense_out, int64_t* keys_out, int64_t* counts_out, int64_t max_pairs, pk_connectivity_info_t* info, std::string* err) {
    const char* who = "pk_particles_connectivity";
    *info = pk_connectivity_info_t{};
    info->path = path;
    if (l.n_origin < 0 || l.n_dest < 0 || l.n_dest >= (1ll << 62) || (l.n_origin > 0 && l.n_dest + 1 > ((1ll << 62) - 1) / l.n_origin)) {
        if (err) *err = std::string(who) + ": needs 0 <= n_origin, 0 <= n_dest and n_origin * (n_dest + 1) < 2^62 (the key is origin * (n_dest + 1) + d)";
        return -2;
    }
    const int64_t nbins = l.n_origin * (l.n_dest + 1);
    const bool sparse = path == PK_CONN_SPARSE;
    if (path == PK_CONN_LDS ? nbins > DENS_LDS_BINS : (!sparse && nbins >= (1ll << 31))) {
        if (err) *err = std::string(who) + (path == PK_CONN_LDS ? ": PK_CONN_LDS needs n_origin * (n_dest + 1) <= 8192 bins" : ": PK_CONN_GLOBAL needs n_origin * (n_dest + 1) < 2^31 bins");
        return -2;
    }
    const int64_t n = c.n;
    if (!sparse) memset(dense_out, 0, (size_t)nbins * 8);
    if (n == 0) return 0;
    ConnScratch s;
    ConnDev d;
    int dx, dy, dz;
    if (int rc = conn_prepare(who, stream, g, c, levels, l, ncells, s, d, dx, dy, dz, err)) return rc;
    d.origin_i64 = l.origin_dtype == PK_DENSITY_I64;
    if (l.origin_dev) {
        d.origin = l.origin_dev;
    } else {
        const size_t bytes = (size_t)n * (d.origin_i64 ? 8 : 4);
        CONN_HIP(hipMalloc(&s.origin, bytes));
        CONN_HIP(hipMemcpyAsync(s.origin, l.origin_host, bytes, hipMemcpyHostToDevice, stream));
        d.origin = s.origin;
        d.origin_host_order = 1;
    }
    for (hipEvent_t& e : s.ev) CONN_HIP(hipEventCreate(&e));
    CONN_HIP(hipMalloc((void**)&s.stats, CONN_NSTATS * 8));
    CONN_HIP(hipMemsetAsync(s.stats, 0, CONN_NSTATS * 8, stream));
    // grid-stride, as density: enough workgroups to fill the device, few enough that the per-workgroup statistics adds stay off the clock
    const unsigned blocks = (unsigned)std::min<int64_t>((n + DENS_WG - 1) / DENS_WG, 8192);
    unsigned long long hstats[CONN_NSTATS] = {};
    float ms[3] = {0.f, 0.f, 0.f};
    int64_t pairs = 0;
    if (!sparse) {
        const size_t bytes = (size_t)std::max<int64_t>(nbins, 1) * 8;
        CONN_HIP(hipMalloc((void**)&s.counts, bytes));
        CONN_HIP(hipMemsetAsync(s.counts, 0, bytes, stream));
        CONN_HIP(hipEventRecord(s.ev[0], stream));
        // LDS: every workgroup flushes up to nbins bins -- few, long-lived workgroups (pk_density.hip)
        if (path == PK_CONN_LDS) conn_launch<CONN_LDS>(stream, std::min(blocks, 1024u), (size_t)nbins * 4, g, c, d, levels, dx, dy, dz, s.counts, nullptr, s.stats);
        else conn_launch<CONN_GLOBAL>(stream, blocks, 0, g, c, d, levels, dx, dy, dz, s.counts, nullptr, s.stats);
        CONN_HIP(hipGetLastError());
        CONN_HIP(hipEventRecord(s.ev[1], stream));
        CONN_HIP(hipMemcpyAsync(dense_out, s.counts, (size_t)nbins * 8, hipMemcpyDeviceToHost, stream));
        CONN_HIP(hipMemcpyAsync(hstats, s.stats, sizeof(hstats), hipMemcpyDeviceToHost, stream));
        CONN_HIP(hipStreamSynchronize(stream));
        CONN_HIP(hipEventElapsedTime(&ms[0], s.ev[0], s.ev[1]));
        for (int64_t k = 0; k < nbins; k++) pairs += dense_out[k] != 0;
    } else {
        CONN_HIP(hipMalloc((void**)&s.keys, (size_t)n * 8));
        CONN_HIP(hipMalloc((void**)&s.keys_alt, (size_t)n * 8));
        CONN_HIP(hipMalloc((void**)&s.uniq, (size_t)n * 8));
        CONN_HIP(hipMalloc((void**)&s.runs, (size_t)n * 8));
        CONN_HIP(hipMalloc((void**)&s.nruns, 8));
        unsigned end_bit = 1;  // bits of the sentinel nbins, the largest key stored
        while (end_bit < 63 && (nbins >> end_bit) != 0) end_bit++;
        rocprim::double_buffer<unsigned long long> kb(s.keys, s.keys_alt);
        size_t sort_bytes = 0, rle_bytes = 0;
        CONN_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, kb, (size_t)n, 0u, end_bit, stream));
        CONN_HIP(rocprim::run_length_encode(nullptr, rle_bytes, s.keys, (unsigned int)n, s.uniq, s.runs, s.nruns, stream));
        CONN_HIP(hipMalloc(&s.sort_tmp, sort_bytes ? sort_bytes : 16));
        CONN_HIP(hipMalloc(&s.rle_tmp, rle_bytes ? rle_bytes : 16));
        CONN_HIP(hipEventRecord(s.ev[0], stream));
        conn_launch<CONN_STORE>(stream, blocks, 0, g, c, d, levels, dx, dy, dz, nullptr, s.keys, s.stats);
        CONN_HIP(hipGetLastError());
        CONN_HIP(hipEventRecord(s.ev[1], stream));
        CONN_HIP(rocprim::radix_sort_keys(s.sort_tmp, sort_bytes, kb, (size_t)n, 0u, end_bit, stream));
        CONN_HIP(hipEventRecord(s.ev[2], stream));
        CONN_HIP(rocprim::run_length_encode(s.rle_tmp, rle_bytes, kb.current(), (unsigned int)n, s.uniq, s.runs, s.nruns, stream));
        CONN_HIP(hipEventRecord(s.ev[3], stream));
        unsigned long long nruns = 0, last = 0;
        CONN_HIP(hipMemcpyAsync(&nruns, s.nruns, 8, hipMemcpyDeviceToHost, stream));
        CONN_HIP(hipMemcpyAsync(hstats, s.stats, sizeof(hstats), hipMemcpyDeviceToHost, stream));
        CONN_HIP(hipStreamSynchronize(stream));
        if (nruns == 0 || nruns > (unsigned long long)n) {
            if (err) *err = std::string(who) + ": the run-length encode answered a number of runs outside [1, n]";
            return -1;
        }
        CONN_HIP(hipMemcpyAsync(&last, s.uniq + (nruns - 1), 8, hipMemcpyDeviceToHost, stream));
        CONN_HIP(hipStreamSynchronize(stream));
        pairs = (int64_t)nruns - (last == (unsigned long long)nbins ? 1 : 0);  // the sentinel sorts last: its run is no pair
        if (pairs > max_pairs) {
            if (err) *err = std::string(who) + ": " + std::to_string(pairs) + " pairs found, room for " + std::to_string(max_pairs);
            return -2;
        }
        if (pairs > 0) {
            CONN_HIP(hipMemcpyAsync(keys_out, s.uniq, (size_t)pairs * 8, hipMemcpyDeviceToHost, stream));
            CONN_HIP(hipMemcpyAsync(counts_out, s.runs, (size_t)pairs * 8, hipMemcpyDeviceToHost, stream));
            CONN_HIP(hipStreamSynchronize(stream));
        }
        for (int k = 0; k < 3; k++) CONN_HIP(hipEventElapsedTime(&ms[k], s.ev[k], s.ev[k + 1]));
    }
    if (hstats[4]) {
        if (err) *err = std::string(who) + ": the region table holds a label >= n_dest (" + std::to_string(hstats[4]) + " rows fell into such a cell)";
        return -2;
    }
    info->n_tracked = (int64_t)hstats[0];
    info->n_outside = (int64_t)hstats[1];
    info->n_atomics = (int64_t)hstats[2];
    info->n_above = (int64_t)hstats[3];
    info->n_pairs = pairs;
    info->key_ms = ms[0];
    info->sort_ms = ms[1];
    info->encode_ms = ms[2];
    return 0;
}

}  // namespace pk
