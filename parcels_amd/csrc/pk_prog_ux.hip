// Instantiations of the fused step loop, the point sampler and the search for launches whose main grid is a UxGrid (pk_ux.h).
#define PK_UX_KERNELS
#include "pk_ux.h"
namespace pk {
void launch_ux(int particles_f32, const KArgs& a, int64_t n, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (particles_f32) hipLaunchKernelGGL(advect_ux_kernel<1>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(advect_ux_kernel<0>, grid, dim3(256), 0, stream, a);
}
void launch_ux_eval(const KArgs& a, int what, int64_t m, const double* t, const double* z, const double* y, const double* x, double* ou,
                    double* ov, double* ow, int32_t* ost, hipStream_t stream) {
    hipLaunchKernelGGL(eval_ux_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, a, what, m, t, z, y, x, ou, ov, ow, ost);
}
void launch_ux_eval_attached(const KArgs& a, int what, int64_t m, const double* t, const double* z, const double* y, const double* x, int32_t* ei,
                             double* ou, double* ov, double* ow, int32_t* ost, hipStream_t stream) {
    hipLaunchKernelGGL(eval_ux_attached_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, a, what, m, t, z, y, x, ei, ou, ov, ow, ost);
}
void launch_ux_search(const DGrid& g, int64_t m, const double* z, const double* y, const double* x, int32_t* ei, hipStream_t stream) {
    hipLaunchKernelGGL(search_ux_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, g, m, z, y, x, ei);
}
}  // namespace pk
