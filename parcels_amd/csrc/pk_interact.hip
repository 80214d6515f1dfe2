// Built-in interaction kernels on the device-resident particle columns: see pk_interact.h.
//
// Passes of one iteration (all on the caller's stream; no workgroup waits on another; every loop is bounded by a number computed
// beforehand -- a row's CSR range, whose end the count pass fixed):
//   prologue   one lane per row: mask, dt clip, two counters (wave reduction, one atomic per wavefront)
//   attract    pk_neighbors.hip: device-input build -> count -> scan -> fill -> row sort -> finish (dx, dy, dz, dist per pair, the values
//              pa.neighbors returns), then ia_reduce_kernel: one lane per row of the mask walks its pairs in order
//   merge      pk_neighbors.hip: device-input build -> nearest, then ia_merge_kernel: one lane per row; a row belongs to at most one
//              mutual pair and only the lower row of a pair writes, so no two lanes write one element
//   epilogue   one lane per row: position update, dt reset, EndofLoop, histogram of the states (LDS, then one atomic per code and block)
//
// The sums must not be contracted into fused multiply-adds (NumPy rounds every operation): built with -ffp-contract=off like
// pk_neighbors.hip, and this file repeats it.
#pragma clang fp contract(off)
#include "pk_interact.h"

#include <chrono>
#include <cmath>
#include <cstring>

#include "../../include/parcels_hip.h"

namespace pk {
namespace {

constexpr int IA_BLOCK = 256;
constexpr int IA_NCOUNT = 3 + PK_NUM_STATE_CODES;  // evaluated, active, steps, histogram

__device__ __forceinline__ double ia_ld(const void* col, int64_t i, bool f32) { return f32 ? (double)((const float*)col)[i] : ((const double*)col)[i]; }
__device__ __forceinline__ void ia_st(void* col, int64_t i, double v, bool f32) {
    if (f32) ((float*)col)[i] = (float)v;
    else ((double*)col)[i] = v;
}
// `column += float64 array` of a host kernel: NumPy adds in float64 and the assignment rounds to the storage dtype
__device__ __forceinline__ void ia_add_f64(void* col, int64_t i, double v, bool f32) { ia_st(col, i, ia_ld(col, i, f32) + v, f32); }
// `column[rows] += column2[rows]` of the position update: both operands have the storage dtype, so the sum is taken in it (pk_kernels.h: padd)
__device__ __forceinline__ double ia_padd(bool f32, double a, double b) { return f32 ? (double)((float)a + (float)b) : a + b; }
// np.minimum / np.maximum: a NaN operand gives NaN
__device__ __forceinline__ double np_minimum(double a, double b) { return (a != a || b != b) ? (double)NAN : (a < b ? a : b); }
__device__ __forceinline__ double np_maximum(double a, double b) { return (a != a || b != b) ? (double)NAN : (a > b ? a : b); }

__device__ __forceinline__ unsigned long long ia_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// what the loop condition (:190) and the mask (:193-195) count in a row of state s at time t
__device__ __forceinline__ void ia_count(int s, double t, double endtime, int sign, unsigned long long& ev, unsigned long long& active) {
    active = (s == PK_EVALUATE || s == PK_REPEAT) ? 1u : 0u;
    ev = ((s == PK_SUCCESS || s == PK_EVALUATE) && (double)sign * (endtime - t) >= 0.0) ? 1u : 0u;
}

__global__ void __launch_bounds__(IA_BLOCK) ia_prologue_kernel(InteractColumns c, double endtime, int sign, int reset, int clip,
                                                               unsigned long long* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * IA_BLOCK + threadIdx.x;
    unsigned long long ev = 0, active = 0;
    if (i < c.n) {
        int s = c.state[i];
        if (reset) c.state[i] = s = PK_EVALUATE;  // kernel.py:188
        const double t = c.t[i];
        ia_count(s, t, endtime, sign, ev, active);
        if (clip) {  // (the reference leaves the loop before it clips when the mask is empty, :196-197: the caller counts first)
            c.mask[i] = (int32_t)ev;
            const double tte = (double)sign * (endtime - t), dt = c.dt[i];  // :199-203, every row
            c.dt[i] = sign == 1 ? np_maximum(np_minimum(dt, tte), 0.0) : np_minimum(np_maximum(dt, -tte), 0.0);
        }
    }
    ev = ia_wave_sum(ev);
    active = ia_wave_sum(active);
    if ((threadIdx.x & 63) == 0) {
        if (ev) atomicAdd(&cnt[0], ev);
        if (active) atomicAdd(&cnt[1], active);
    }
}

__global__ void __launch_bounds__(IA_BLOCK) ia_epilogue_kernel(InteractColumns c, double endtime, double dt0, int sign, unsigned long long* __restrict__ cnt) {
    __shared__ unsigned int hist[PK_NUM_STATE_CODES];
    for (int k = threadIdx.x; k < PK_NUM_STATE_CODES; k += IA_BLOCK) hist[k] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * IA_BLOCK + threadIdx.x;
    unsigned long long steps = 0, ev = 0, active = 0;
    if (i < c.n) {
        const bool f32 = c.f32 != 0;
        int s = c.state[i];
        double t = c.t[i];
        if (c.mask[i] != 0 && (s == PK_EVALUATE || s == PK_SUCCESS)) {  // :219-222 -> _position_update :108-120
            const double dt = c.dt[i];
            if ((double)sign * (endtime - t) > 0.0 && t + dt == t) {
                s = PK_ERROR;  // the step would not advance t before endtime: the reference's loop spins forever (pk_kernels.h: advect_kernel)
            } else {
                ia_st(c.x, i, ia_padd(f32, ia_ld(c.x, i, f32), ia_ld(c.dx, i, f32)), f32);
                ia_st(c.y, i, ia_padd(f32, ia_ld(c.y, i, f32), ia_ld(c.dy, i, f32)), f32);
                ia_st(c.z, i, ia_padd(f32, ia_ld(c.z, i, f32), ia_ld(c.dz, i, f32)), f32);
                t += dt;
                c.t[i] = t;
                ia_st(c.dx, i, 0.0, f32);
                ia_st(c.dy, i, 0.0, f32);
                ia_st(c.dz, i, 0.0, f32);
                steps = 1;
            }
        }
        c.dt[i] = dt0;                                           // :225-226
        if (s == PK_EVALUATE && t == endtime) s = PK_ENDOFLOOP;  // :229-230
        c.state[i] = s;
        if (s >= 0 && s < PK_NUM_STATE_CODES) atomicAdd(&hist[s], 1u);
        ia_count(s, t, endtime, sign, ev, active);  // of the NEXT iteration
    }
    steps = ia_wave_sum(steps);
    ev = ia_wave_sum(ev);
    active = ia_wave_sum(active);
    if ((threadIdx.x & 63) == 0) {
        if (ev) atomicAdd(&cnt[0], ev);
        if (active) atomicAdd(&cnt[1], active);
        if (steps) atomicAdd(&cnt[2], steps);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PK_NUM_STATE_CODES; k += IA_BLOCK)
        if (hist[k]) atomicAdd(&cnt[3 + k], (unsigned long long)hist[k]);
}

// np.bincount(nb.i, weights=nb.dx / nb.dist): the sum starts from 0.0 and takes the pairs of the row in order, IEEE division
__device__ __forceinline__ double ia_row_sum(const double* __restrict__ num, const double* __restrict__ dist, int64_t pb, int64_t pe) {
    double s = 0.0;
    for (int64_t p = pb; p < pe; p++) s += num[p] / dist[p];
    return s;
}

__global__ void __launch_bounds__(IA_BLOCK) ia_reduce_kernel(InteractColumns c, NeighborsDeviceView v, double velocity, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * IA_BLOCK + threadIdx.x;
    if (i >= c.n || c.mask[i] == 0) return;
    int64_t pb = 0, pe = 0;
    if (v.total > 0) {  // (without a pair the pair arrays may not exist; every row still adds its 0.0)
        pb = v.starts[i];
        pe = v.starts[i + 1];
        if (pb < 0 || pe < pb || pe > v.total) {  // cannot happen after a clean scan; never read out of bounds
            *flag = 1;
            return;
        }
    }
    const bool f32 = c.f32 != 0;
    const double dt = c.dt[i];
    ia_add_f64(c.dx, i, (ia_row_sum(v.dx, v.dist, pb, pe) * velocity) * dt, f32);
    ia_add_f64(c.dy, i, (ia_row_sum(v.dy, v.dist, pb, pe) * velocity) * dt, f32);
    if (v.dz) ia_add_f64(c.dz, i, (ia_row_sum(v.dz, v.dist, pb, pe) * velocity) * dt, f32);
}

template <class T>
__global__ void __launch_bounds__(IA_BLOCK) ia_merge_kernel(int64_t n, const int32_t* __restrict__ mask, const int64_t* __restrict__ nn, T* __restrict__ mass,
                                                            int32_t* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * IA_BLOCK + threadIdx.x;
    if (i >= n || mask[i] == 0) return;
    const int64_t j = nn[i];
    if (j <= i || j >= n || nn[j] != i) return;  // the lower row of a mutual pair goes on (j == -1 without a neighbour)
    const T mi = mass[i], mj = mass[j];
    const bool j_keeps = mj > mi;  // equal masses: the lower index keeps
    const int64_t big = j_keeps ? j : i, small = j_keeps ? i : j;
    mass[big] = (j_keeps ? mj : mi) + (j_keeps ? mi : mj);  // m[big] += m[small] in the storage dtype
    state[small] = PK_DELETE;
}

inline unsigned ia_blocks(int64_t n) { return (unsigned)((n + IA_BLOCK - 1) / IA_BLOCK); }

#define IA_TRY(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            if (err) *err = std::string("interact: " #call ": ") + hipGetErrorString(e_); \
            return -1;                                                                \
        }                                                                             \
    } while (0)

inline double ia_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int ia_build(Neighbors* nb, hipStream_t stream, const InteractColumns& c, double radius, double sphere_radius, int32_t use_z, int32_t use_sources,
             std::string* err) {
    NeighborsDeviceInput in;
    in.x = c.x;
    in.y = c.y;
    in.z = use_z ? c.z : nullptr;
    in.f32 = c.f32;
    in.mask = c.mask;
    in.use_sources = use_sources;
    return neighbors_build_device(nb, stream, c.n, in, radius, sphere_radius, PK_NEIGHBORS_NO_COINCIDENT, err);
}

}  // namespace

struct Interact {
    unsigned long long* d_cnt = nullptr;
    unsigned long long* h_cnt = nullptr;  // pinned
};

Interact* interact_create() { return new Interact(); }

void interact_free(Interact* it) {
    if (!it) return;
    if (it->d_cnt) (void)hipFree(it->d_cnt);
    if (it->h_cnt) (void)hipHostFree(it->h_cnt);
    delete it;
}

namespace {
int ia_counters(Interact* it, hipStream_t stream, std::string* err) {
    if (!it->d_cnt) {
        IA_TRY(hipMalloc((void**)&it->d_cnt, sizeof(unsigned long long) * IA_NCOUNT));
        IA_TRY(hipHostMalloc((void**)&it->h_cnt, sizeof(unsigned long long) * IA_NCOUNT, hipHostMallocDefault));
    }
    IA_TRY(hipMemsetAsync(it->d_cnt, 0, sizeof(unsigned long long) * IA_NCOUNT, stream));
    return 0;
}
int ia_fetch(Interact* it, hipStream_t stream, std::string* err) {
    IA_TRY(hipGetLastError());
    IA_TRY(hipMemcpyAsync(it->h_cnt, it->d_cnt, sizeof(unsigned long long) * IA_NCOUNT, hipMemcpyDeviceToHost, stream));
    IA_TRY(hipStreamSynchronize(stream));
    return 0;
}
}  // namespace

int interact_prologue(Interact* it, hipStream_t stream, const InteractColumns& c, double endtime, double dt0, int32_t reset_state, int32_t clip,
                      int64_t* n_evaluated, int64_t* n_active, std::string* err) {
    *n_evaluated = *n_active = 0;
    if (c.n == 0) return 0;
    if (int rc = ia_counters(it, stream, err)) return rc;
    hipLaunchKernelGGL(ia_prologue_kernel, dim3(ia_blocks(c.n)), dim3(IA_BLOCK), 0, stream, c, endtime, dt0 > 0 ? 1 : -1, reset_state ? 1 : 0, clip ? 1 : 0,
                       it->d_cnt);
    if (int rc = ia_fetch(it, stream, err)) return rc;
    *n_evaluated = (int64_t)it->h_cnt[0];
    *n_active = (int64_t)it->h_cnt[1];
    return 0;
}

int interact_epilogue(Interact* it, hipStream_t stream, const InteractColumns& c, double endtime, double dt0, int64_t* steps,
                      int64_t* state_counts, int64_t* next_evaluated, int64_t* next_active, std::string* err) {
    *steps = *next_evaluated = *next_active = 0;
    memset(state_counts, 0, sizeof(int64_t) * PK_NUM_STATE_CODES);
    if (c.n == 0) return 0;
    if (int rc = ia_counters(it, stream, err)) return rc;
    hipLaunchKernelGGL(ia_epilogue_kernel, dim3(ia_blocks(c.n)), dim3(IA_BLOCK), 0, stream, c, endtime, dt0, dt0 > 0 ? 1 : -1, it->d_cnt);
    if (int rc = ia_fetch(it, stream, err)) return rc;
    *next_evaluated = (int64_t)it->h_cnt[0];
    *next_active = (int64_t)it->h_cnt[1];
    *steps = (int64_t)it->h_cnt[2];
    for (int k = 0; k < PK_NUM_STATE_CODES; k++) state_counts[k] = (int64_t)it->h_cnt[3 + k];
    return 0;
}

int interact_attract(Neighbors* nb, hipStream_t stream, const InteractColumns& c, double radius, double velocity, double sphere_radius,
                     int32_t use_z, int32_t use_sources, int64_t max_pairs, int64_t* total, double* phase_ms, std::string* err) {
    *total = 0;
    if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.0;
    if (c.n == 0) return 0;
    auto t0 = std::chrono::steady_clock::now();
    if (int rc = ia_build(nb, stream, c, radius, sphere_radius, use_z, use_sources, err)) return rc;
    if (phase_ms) phase_ms[0] = ia_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (int rc = neighbors_counts(nb, stream, nullptr, total, err)) return rc;
    if (*total > max_pairs) return 0;  // the caller raises: nothing was allocated for the pairs
    if (int rc = neighbors_pairs_device(nb, stream, *total, err)) return rc;
    if (phase_ms) phase_ms[1] = ia_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    NeighborsDeviceView v;
    neighbors_device_view(nb, &v);
    if (v.n != c.n || v.total != *total || !v.starts) {
        if (err) *err = "interact: the cell list does not describe the bound rows (internal error)";
        return -3;
    }
    int32_t* flag = v.flag;
    IA_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(ia_reduce_kernel, dim3(ia_blocks(c.n)), dim3(IA_BLOCK), 0, stream, c, v, velocity, flag);
    IA_TRY(hipGetLastError());
    int32_t f = 0;
    IA_TRY(hipMemcpyAsync(&f, flag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    IA_TRY(hipStreamSynchronize(stream));
    if (phase_ms) phase_ms[2] = ia_ms_since(t0);
    if (f) {
        if (err) *err = "interact: a row's pair range lies outside the pair list (nothing was read out of bounds)";
        return -3;
    }
    return 0;
}

int interact_merge(Neighbors* nb, hipStream_t stream, const InteractColumns& c, void* mass, int32_t mass_f32, double radius, double sphere_radius,
                   int32_t use_z, double* phase_ms, std::string* err) {
    if (phase_ms) phase_ms[0] = phase_ms[1] = 0.0;
    if (c.n == 0) return 0;
    if (!mass) {
        if (err) *err = "interact: the mass column is not on the device";
        return -2;
    }
    auto t0 = std::chrono::steady_clock::now();
    if (int rc = ia_build(nb, stream, c, radius, sphere_radius, use_z, 0, err)) return rc;
    if (phase_ms) phase_ms[0] = ia_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (int rc = neighbors_nearest_device(nb, stream, err)) return rc;
    NeighborsDeviceView v;
    neighbors_device_view(nb, &v);
    if (v.n != c.n || !v.near_j) {
        if (err) *err = "interact: the cell list does not describe the bound rows (internal error)";
        return -3;
    }
    if (mass_f32) hipLaunchKernelGGL((ia_merge_kernel<float>), dim3(ia_blocks(c.n)), dim3(IA_BLOCK), 0, stream, c.n, c.mask, v.near_j, (float*)mass, c.state);
    else hipLaunchKernelGGL((ia_merge_kernel<double>), dim3(ia_blocks(c.n)), dim3(IA_BLOCK), 0, stream, c.n, c.mask, v.near_j, (double*)mass, c.state);
    IA_TRY(hipGetLastError());
    IA_TRY(hipStreamSynchronize(stream));
    if (phase_ms) phase_ms[1] = ia_ms_since(t0);
    return 0;
}

}  // namespace pk
