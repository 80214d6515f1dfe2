// tools/cos_lean_check.hip -- accuracy of cos_lat_lean (parcels_amd/csrc/pk_fast_agrid.h), the cosine of the unit conversion in the lean build of
// the dedicated A-grid kernels, evaluated ON THE DEVICE over latitudes in degrees and compared on the host with cosl() of the same rounded
// argument lat * RN(pi / 180) in x87 extended precision (64-bit significand).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I parcels_amd/csrc tools/cos_lean_check.hip -o /tmp/cos_lean_check && /tmp/cos_lean_check
// (tests/test_gpu_fast_eval_lean.py does that on the GPU box)
//
// The bound it asserts is reasoned, not fitted: cos = RN(1 - 2 s^2) with one rounding (fma) and s = sin(h) (1 + e), |e| <= 2^-52 (the minimax
// kernel: < 1 ulp), so |error| <= (1 - cos) * 2 |e| + ulp(cos) / 2 <= 2^-51 + 2^-54 ABSOLUTE: 4.5 units of 2^-53.  In ulps of the result that
// is half an ulp near the equator and grows with 1 / cos towards the poles (2^-51 / cos(1.5) = 6.3e-15 relative at the switch to cos_lat).
// Beyond |lat * pi / 180| = 1.5 the routine is cos_lat (< 1 ulp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pk_fast_agrid.h"  // the routine under test, as shipped (-I parcels_amd/csrc)

__global__ void eval(const double* lat, double* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pk::cos_lat_lean(lat[i]);
}

static uint64_t rng(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double uni(uint64_t& s) { return (double)(rng(s) >> 11) * (1.0 / 9007199254740992.0); }

int main() {
    // bands of |lat| in degrees; the last one lies beyond 1.5 rad = 85.9437 degrees: the fallback
    const double edge[] = {0.0, 30.0, 60.0, 76.0, 80.0, 84.0, 85.9, 85.9436692696, 85.95, 90.0};
    const int nb = 9, per = 1 << 19;
    const int n = nb * per;
    std::vector<double> lat(n), got(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int b = 0; b < nb; b++)
        for (int k = 0; k < per; k++) lat[b * per + k] = (uni(s) < 0.5 ? -1.0 : 1.0) * (edge[b] + (edge[b + 1] - edge[b]) * uni(s));
    lat[0] = 0.0; lat[1] = -0.0; lat[2] = 1e-300; lat[3] = 45.0; lat[4] = -45.0;
    double *dl, *dg;
    if (hipMalloc(&dl, n * sizeof(double)) != hipSuccess || hipMalloc(&dg, n * sizeof(double)) != hipSuccess) return 2;
    if (hipMemcpy(dl, lat.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 2;
    hipLaunchKernelGGL(eval, dim3((n + 255) / 256), dim3(256), 0, 0, dl, dg, n);
    if (hipMemcpy(got.data(), dg, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    const double deg2rad = 3.14159265358979323846 / 180.0;
    double ulp[16] = {0}, ab[16] = {0};
    for (int i = 0; i < n; i++) {
        const double x = lat[i] * deg2rad;  // the argument the reference's np.cos(np.deg2rad(lat)) sees
        const long double want = cosl((long double)x);
        const long double err = fabsl((long double)got[i] - want);
        int e;
        frexp((double)want, &e);
        const int b = i / per;
        ulp[b] = fmax(ulp[b], (double)(err / ldexpl(1.0L, e - 53)));
        ab[b] = fmax(ab[b], (double)(err * 9007199254740992.0L));
    }
    printf("{\"samples\": %d, \"band_edges_deg\": [", n);
    for (int b = 0; b <= nb; b++) printf("%s%.10g", b ? ", " : "", edge[b]);
    printf("], \"max_ulp\": [");
    for (int b = 0; b < nb; b++) printf("%s%.2f", b ? ", " : "", ulp[b]);
    printf("], \"max_abs_err_in_2^-53\": [");
    for (int b = 0; b < nb; b++) printf("%s%.2f", b ? ", " : "", ab[b]);
    printf("]}\n");
    bool ok = true;
    for (int b = 0; b < nb - 1; b++) ok = ok && ab[b] <= 4.5;  // the lean region (the last of these bands straddles the switch)
    ok = ok && ulp[nb - 1] <= 1.0;                             // cos_lat
    return ok ? 0 : 1;
}
