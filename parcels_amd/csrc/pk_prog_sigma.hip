// Instantiations of the fused step loop and of the point conversion for CROCO sigma grids (pk_sigma.h): program PROG_SIGMA.
#define PK_SIGMA_KERNELS
#include "pk_sigma.h"
namespace pk {
#define PK_SIGMA_CASE(FT, KD, IN) hipLaunchKernelGGL((advect_sigma_kernel<FT, KD, IN>), grid, dim3(256), lds_bytes, stream, a)
void launch_sigma(int field_f32, int curvilinear, int interp, const KArgs& a, int64_t n, size_t lds_bytes, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 255) / 256));
    const int key = (field_f32 ? 4 : 0) + (curvilinear ? 2 : 0) + (interp ? 1 : 0);  // interp: 0 XLinear_Velocity, 1 CGrid_Velocity
    switch (key) {
        case 0: PK_SIGMA_CASE(double, 0, 0); break;
        case 1: PK_SIGMA_CASE(double, 0, 1); break;
        case 2: PK_SIGMA_CASE(double, 1, 0); break;
        case 3: PK_SIGMA_CASE(double, 1, 1); break;
        case 4: PK_SIGMA_CASE(float, 0, 0); break;
        case 5: PK_SIGMA_CASE(float, 0, 1); break;
        case 6: PK_SIGMA_CASE(float, 1, 0); break;
        default: PK_SIGMA_CASE(float, 1, 1); break;
    }
}
#undef PK_SIGMA_CASE
void launch_sigma_points(const KArgs& a, int64_t m, const double* t, const double* z, const double* y, const double* x, double* out,
                         size_t lds_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(sigma_points_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), lds_bytes, stream, a, m, t, z, y, x, out);
}
}  // namespace pk
