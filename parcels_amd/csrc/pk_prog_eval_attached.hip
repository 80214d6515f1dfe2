// Field.eval / VectorField.eval at explicit points WITH the particles, on structured grids (pk_eval_attached): the sampler of pk_eval
// (pk_api_sample.hip: eval_kernel) with the particles' `ei` on the sampled field's grid in and out, so that the search starts from the cell
// the particle was in (field.py:173-176, index_search.py:269-285).  On a curvilinear grid a guessed search that hits keeps the float64
// (xsi, eta) of the point-in-cell test while an unguessed one returns the hash query's float32-rounded pair: a Python kernel on the host
// path that samples with the particles sees the reference's values only this way.  A unit of its own: the kernels of pk_api_sample.hip
// stay as they are.
#include "pk_api_ctx.h"

namespace pk {

template <class FT, int INTERP, bool TYPED>
__global__ void __launch_bounds__(256) eval_attached_kernel(const KArgs a, int what, int64_t m, const double* t, const double* z, const double* y,
                                                            const double* x, int32_t* ei, double* ou, double* ov, double* ow, int32_t* ost) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const DField& mf = kfield(a, a.main_field);
    const DGrid& mg = kgrid(a, a.main_grid);
    Coords mc{CellCache{nullptr, nullptr, nullptr}, mf.time, mg.depth, mg.lat, mg.lon, mf.tfirst, mf.tlast, mg.zfirst, mg.zlast, mg.yfirst, mg.ylast, mg.xfirst, mg.xlast};
    PCtx c;
    c.state = PK_EVALUATE;
    c.pf = false;
    c.hz = c.hy = c.hx = c.ht = 0;
    c.hyx_valid = false;
    c.first_eval = 0xFu;  // the one search of this call is guessed iff the batch holds a non-zero guess (a.prm.have_guess0)
    c.u32 = c.v32 = false;
    c.oob = false;
    c.ei0 = c.ei1 = c.ei2 = c.ei3 = 0;
    c.it = 0u;
    c.klo = 0;
    const bool pos_f32 = a.prm.reset_state != 0;  // (as in eval_kernel: option "eval_points_f32")
    c.zpos_f32 = pos_f32;
    const int g = kfield(a, what >= 0 ? what : a.prm.fU).grid;
    ei_set(c, g, ei[i]);
    if (what < 0) {
        double u, v, w;
        eval_uvw<FT, -1, INTERP, TYPED>(a, mc, c, what == -2, t[i], z[i], y[i], x[i], pos_f32, u, v, w);
        ou[i] = u;
        if (ov) ov[i] = v;
        if (ow) ow[i] = w;
    } else {
        ou[i] = eval_scalar<FT, TYPED>(a, mc, c, what, t[i], z[i], y[i], x[i], pos_f32);
    }
    ei[i] = ei_get(c, g);
    if (ost) ost[i] = c.state | (c.oob ? PK_EVAL_MASKED : 0);
}

}  // namespace pk

namespace pkapi {

void launch_eval_attached(bool f32, int ik, bool typed, const KArgs& a, int what, int64_t m, const double* t, const double* z, const double* y,
                          const double* x, int32_t* ei, double* ou, double* ov, double* ow, int32_t* ost, hipStream_t stream) {
    const dim3 grid((unsigned)((m + 255) / 256));
#define PK_EVAL(FT, IN, TY) hipLaunchKernelGGL((pk::eval_attached_kernel<FT, IN, TY>), grid, dim3(256), 0, stream, a, what, m, t, z, y, x, ei, ou, ov, ow, ost)
#define PK_EVAL_T(FT, IN) do { if (typed) PK_EVAL(FT, IN, true); else PK_EVAL(FT, IN, false); } while (0)
    if (f32) {
        if (ik == 2) PK_EVAL_T(float, 2); else if (ik == 1) PK_EVAL_T(float, 1); else PK_EVAL_T(float, 0);
    } else {
        if (ik == 2) PK_EVAL_T(double, 2); else if (ik == 1) PK_EVAL_T(double, 1); else PK_EVAL_T(double, 0);
    }
#undef PK_EVAL_T
#undef PK_EVAL
}

}  // namespace pkapi
