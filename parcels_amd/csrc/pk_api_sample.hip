// pk_api_sample.hip -- sampling at explicit points, without particles: Field.eval / VectorField.eval (pk_eval*), the index search of
// ParticleSet.populate_indices (pk_search) and the CROCO z-to-sigma conversion (pk_set_croco / pk_sigma_croco).
#include "pk_api_ctx.h"

using namespace pkapi;

namespace pk {

// Field.eval / VectorField.eval at explicit points (no particles): what >= 0 scalar field, -1 UV, -2 UVW
template <class FT, int INTERP, bool TYPED>
__global__ void __launch_bounds__(256) eval_kernel(const KArgs a, int what, int64_t m, const double* t, const double* z,
                                                   const double* y, const double* x, double* ou, double* ov, double* ow,
                                                   int32_t* ost) {
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
    c.first_eval = 0xFu;
    c.u32 = c.v32 = false;
    c.oob = false;
    c.ei0 = c.ei1 = c.ei2 = c.ei3 = 0;
    c.it = 0u;  // not inside the loop of kernel.py:190: the caller of pk_eval owns the batch (parcels_amd/field.py: _eval_key)
    c.klo = 0;
    const bool pos_f32 = a.prm.reset_state != 0;  // (pk_eval's own use of the field: option "eval_points_f32")
    c.zpos_f32 = pos_f32;
    if (what < 0) {
        double u, v, w;
        eval_uvw<FT, -1, INTERP, TYPED>(a, mc, c, what == -2, t[i], z[i], y[i], x[i], pos_f32, u, v, w);
        ou[i] = u;
        if (ov) ov[i] = v;
        if (ow) ow[i] = w;
    } else {
        ou[i] = eval_scalar<FT, TYPED>(a, mc, c, what, t[i], z[i], y[i], x[i], pos_f32);
    }
    if (ost) ost[i] = c.state | (c.oob ? PK_EVAL_MASKED : 0);
}

// One pk_eval call is one batch of the reference: lenT = 2 if np.any(tau > 0) else 1, lenZ likewise over the WHOLE batch
// (_xinterpolators.py:130-131,401-402,575-576).  flags: bit 0 any(tau > 0), bit 1 any(zeta > 0).
__global__ void __launch_bounds__(256) batch_len_kernel(const DField f, const DGrid g, int64_t m, const double* t, const double* z, unsigned* flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned fl = 0;
    if (i < m) {
        GPos p;
        if (time_search(f, f.time, t[i], 0, p) && p.tau > 0) fl |= 1u;
        if (g.has_z) {
            search_1d(g.depth, g.nz, g.depth[0], g.depth[g.nz - 1], z[i], g.depth_f32 != 0, false, 0, p.zi, p.zeta);
            if (p.zeta > 0) fl |= 2u;
        }
    }
    if (__any(fl & 1u) && (threadIdx.x & 63) == 0) atomicOr(flags, 1u);
    if (__any(fl & 2u) && (threadIdx.x & 63) == 0) atomicOr(flags, 2u);
}

// XGrid.search + ravel_index without a guess (ParticleSet.populate_indices, particleset.py:252-262)
__global__ void __launch_bounds__(256) search_kernel(const DGrid g, int64_t m, const double* z, const double* y, const double* x,
                                                     int32_t* ei_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    PCtx c;
    c.state = PK_EVALUATE;
    c.pf = false;
    c.hz = c.hy = c.hx = c.ht = 0;
    c.hyx_valid = false;
    c.zpos_f32 = false;
    GPos p;
    int32_t ei = 0;
    grid_search<-1, false>(g, nullptr, z[i], y[i], x[i], false, &ei, c, false, p);  // indices only: dtype emulation of the bcoords is irrelevant
    ei_out[i] = ei;
}

// ---- cell sort ----------------------------------------------------------------------------------------
// (The cell sort is pk_api.hip: sort_particles.  Its key kernel is compiled HERE, behind sort_keys below: the device compile
// specialises cell_index (pk_device.h) for the call sites of its module, and only next to the sampling kernels, which call it with other
// hints, does this kernel keep the instructions it has -- tools/kernel_code_diff.py shows other ones in a module of its own.)
// key = linear cell index of the particle's current position on the main grid (z-major like the field layout),
// so that the 64 lanes of a wavefront gather from neighbouring cells (coalesced, L2-friendly).
__global__ void __launch_bounds__(256) sort_key_kernel(const DGrid g, const DParticles P, unsigned long long* keys, uint32_t* idx,
                                                       int horizontal_major) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    const bool pf = P.spatial_f32 != 0;
    const double z = pf ? (double)((const float*)P.z)[i] : ((const double*)P.z)[i];
    const double y = pf ? (double)((const float*)P.y)[i] : ((const double*)P.y)[i];
    const double x = pf ? (double)((const float*)P.x)[i] : ((const double*)P.x)[i];
    unsigned long long zi = 0, h = 0;
    if (g.has_z && g.nz >= 2) zi = (unsigned long long)cell_index(g.depth, g.nz, z, 0);
    if (g.kind == 1) {
        // depth-major like the field layout, then the 30-bit Morton code of the hash grid (neighbouring codes = neighbouring
        // cells).  Measured on C3: depth-major 295 ms vs horizontal-major 308 ms per 3.6e8 particle-steps.
        h = morton_code(g, make_qpoint(g, y, x));
        keys[i] = horizontal_major ? ((h << 12) | (zi & 0xFFFull)) : ((zi << 30) | h);
    } else {
        unsigned long long yi = (g.has_y && g.ny >= 2) ? (unsigned long long)cell_index(g.lat, g.ny, y, 0) : 0;
        unsigned long long xi = (g.has_x && g.nx >= 2) ? (unsigned long long)cell_index(g.lon, g.nx, x, 0) : 0;
        keys[i] = (zi * (unsigned long long)g.ny + yi) * (unsigned long long)g.nx + xi;
    }
    idx[i] = (uint32_t)i;
}

}  // namespace pk

// keys and row numbers of the bound device rows on grid `g` into ctx->d_keys / d_idx, on the compute stream (sort_particles)
void pkapi::sort_keys(pk_ctx* ctx, const DGrid& g, int horizontal_major) {
    const dim3 grid((unsigned)((ctx->dev.n + 255) / 256));
    hipLaunchKernelGGL(sort_key_kernel, grid, dim3(256), 0, ctx->compute, g, ctx->dev, ctx->d_keys, ctx->d_idx, horizontal_major);
}

extern "C" {

// ---- sampling ------------------------------------------------------------------------------------------
// pk_eval (ei == nullptr) and pk_eval_attached (ei: the particles' `ei` on the sampled field's grid, in / out; have_guess: np.any(ei))
static int32_t eval_points(pk_ctx* ctx, const pk_exec_params* prm, int32_t what, int64_t m, const double* t, const double* z, const double* y,
                           const double* x, int32_t* ei, int32_t have_guess, double* out_u, double* out_v, double* out_w, int32_t* out_state) {
    if (!ctx || !prm || !t || !z || !y || !x || !out_u) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (m <= 0) return 0;
    pk_exec_params p2 = *prm;
    p2.twe_n = 0;
    p2.reset_state = ctx->eval_points_f32 ? 1 : 0;  // read by eval_kernel as "sample points are float32 columns"
    if (ei) p2.have_guess0 = have_guess ? 1 : 0;
    if (what >= 0) {  // scalar sampling: the main grid is the sampled field's grid
        if (what >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
        if (p2.fU < 0) { p2.fU = what; p2.fV = what; }
    }
    if (ei) {
        const int fs_ = what >= 0 ? what : p2.fU;
        if (what < -2 || fs_ < 0 || fs_ >= (int)ctx->fields.size()) return ctx->fail("pk_eval_attached: unknown field");
        if (ctx_has_ugrid(ctx) && ctx->grids[ctx->fields[fs_].d.grid].d.kind != PK_UX_KIND)
            return ctx->fail("pk_eval_attached: next to a UxGrid only fields on the UxGrid are sampled with the particles");
    }
    DParticles saved = ctx->dev;
    const bool was_bound = ctx->bound;
    KArgs a;
    size_t lds_bytes;
    int use_lds;
    ctx->bound = true;
    int32_t rc = launch_args(ctx, &p2, a, lds_bytes, use_lds);
    if (!rc) rc = upload_descriptors(ctx, a);
    ctx->bound = was_bound;
    ctx->dev = saved;
    if (rc) return rc;
    a.win_lo = -INFINITY;
    a.win_hi = INFINITY;
    double* d = nullptr;
    int32_t* ds = nullptr;
    PK_HIP(ctx, hipMalloc((void**)&d, sizeof(double) * m * 7));
    PK_HIP(ctx, hipMalloc((void**)&ds, sizeof(int32_t) * m * (ei ? 2 : 1)));
    int32_t* de = nullptr;  // attached samples only: the second half of ds
    if (ei) {
        de = ds + m;
        PK_HIP(ctx, hipMemcpyAsync(de, ei, sizeof(int32_t) * m, hipMemcpyHostToDevice, ctx->compute));
    }
    double *dt_ = d, *dz = d + m, *dy = d + 2 * m, *dx = d + 3 * m, *du = d + 4 * m, *dv = d + 5 * m, *dw = d + 6 * m;
    PK_HIP(ctx, hipMemcpyAsync(dt_, t, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(dz, z, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(dy, y, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(dx, x, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    const dim3 grid((unsigned)((m + 255) / 256));
    const int fsel = what >= 0 ? what : p2.fU;
    const bool f32 = ctx->fields[fsel].d.dtype == PK_F32;
    const bool ux = ctx_has_ugrid(ctx);
    if (!ux && ((what >= 0 && ctx->fields[fsel].d.is_const == 4) || (what < 0 && p2.interp_uv >= 2))) {  // batch-global lenT / lenZ
        unsigned* dflags = (unsigned*)ds;  // reused as the state output afterwards
        PK_HIP(ctx, hipMemsetAsync(dflags, 0, sizeof(unsigned), ctx->compute));
        hipLaunchKernelGGL(batch_len_kernel, grid, dim3(256), 0, ctx->compute, ctx->fields[fsel].d, ctx->grids[ctx->fields[fsel].d.grid].d, m, dt_, dz, dflags);
        unsigned hflags = 0;
        PK_HIP(ctx, hipMemcpyAsync(&hflags, dflags, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->compute));
        PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
        a.prm.force_lent = (hflags & 1u) ? 2 : 1;
        a.prm.force_lenz = (hflags & 2u) ? 2 : 1;
    }
    const bool typed = ctx_is_typed(ctx);
    if (ux) {
        const int eg = ctx->fields[what >= 0 ? what : p2.fU].d.grid;
        if (ctx->grids[eg].d.kind != PK_UX_KIND && what < 0) return ctx->fail("a vector field next to a UxGrid must live on the UxGrid");
        if (ei) launch_ux_eval_attached(a, what, m, dt_, dz, dy, dx, de, du, dv, dw, ds, ctx->compute);
        else launch_ux_eval(a, what, m, dt_, dz, dy, dx, du, dv, dw, ds, ctx->compute);
    } else {
#define PK_EVAL(FT, IN, TY) hipLaunchKernelGGL((eval_kernel<FT, IN, TY>), grid, dim3(256), 0, ctx->compute, a, what, m, dt_, dz, dy, dx, du, dv, dw, ds)
#define PK_EVAL_T(FT, IN) do { if (typed) PK_EVAL(FT, IN, true); else PK_EVAL(FT, IN, false); } while (0)
    const int ik = p2.interp_uv >= 2 ? 2 : p2.interp_uv;
    if (ei) launch_eval_attached(f32, ik, typed, a, what, m, dt_, dz, dy, dx, de, du, dv, dw, ds, ctx->compute);
    else if (f32) {
        if (ik == 2) PK_EVAL_T(float, 2); else if (ik == 1) PK_EVAL_T(float, 1); else PK_EVAL_T(float, 0);
    } else {
        if (ik == 2) PK_EVAL_T(double, 2); else if (ik == 1) PK_EVAL_T(double, 1); else PK_EVAL_T(double, 0);
    }
#undef PK_EVAL_T
#undef PK_EVAL
    }
    PK_HIP(ctx, hipGetLastError());
    PK_HIP(ctx, hipMemcpyAsync(out_u, du, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->compute));
    if (out_v) PK_HIP(ctx, hipMemcpyAsync(out_v, dv, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->compute));
    if (out_w) PK_HIP(ctx, hipMemcpyAsync(out_w, dw, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->compute));
    if (out_state) PK_HIP(ctx, hipMemcpyAsync(out_state, ds, sizeof(int32_t) * m, hipMemcpyDeviceToHost, ctx->compute));
    if (ei) PK_HIP(ctx, hipMemcpyAsync(ei, de, sizeof(int32_t) * m, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    PK_HIP(ctx, hipFree(d));
    PK_HIP(ctx, hipFree(ds));
    return 0;
}

int32_t pk_eval(pk_ctx* ctx, const pk_exec_params* prm, int32_t what, int64_t m, const double* t, const double* z,
                const double* y, const double* x, double* out_u, double* out_v, double* out_w, int32_t* out_state) {
    return eval_points(ctx, prm, what, m, t, z, y, x, nullptr, 0, out_u, out_v, out_w, out_state);
}

int32_t pk_eval_attached(pk_ctx* ctx, const pk_exec_params* prm, int32_t what, int32_t have_guess, int64_t m, const double* t, const double* z,
                         const double* y, const double* x, int32_t* ei, double* out_u, double* out_v, double* out_w, int32_t* out_state) {
    if (!ei) return -2;
    return eval_points(ctx, prm, what, m, t, z, y, x, ei, have_guess, out_u, out_v, out_w, out_state);
}

int32_t pk_search(pk_ctx* ctx, int32_t grid_id, int64_t m, const double* z, const double* y, const double* x, int32_t* ei_out) {
    if (!ctx || !z || !y || !x || !ei_out) return -2;
    if (grid_id < 0 || grid_id >= (int)ctx->grids.size()) return ctx->fail("unknown grid id");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (m <= 0) return 0;
    double* d = nullptr;
    int32_t* de = nullptr;
    PK_HIP(ctx, hipMalloc((void**)&d, sizeof(double) * m * 3));
    PK_HIP(ctx, hipMalloc((void**)&de, sizeof(int32_t) * m));
    PK_HIP(ctx, hipMemcpyAsync(d, z, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(d + m, y, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(d + 2 * m, x, sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute));
    if (ctx->grids[grid_id].d.kind == PK_UX_KIND) launch_ux_search(ctx->grids[grid_id].d, m, d, d + m, d + 2 * m, de, ctx->compute);
    else hipLaunchKernelGGL(search_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->compute, ctx->grids[grid_id].d, m, d, d + m, d + 2 * m, de);
    PK_HIP(ctx, hipGetLastError());
    PK_HIP(ctx, hipMemcpyAsync(ei_out, de, sizeof(int32_t) * m, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    PK_HIP(ctx, hipFree(d));
    PK_HIP(ctx, hipFree(de));
    return 0;
}

// ---- CROCO sigma grids (pk_sigma.h) ---------------------------------------------------------------------
int32_t pk_set_croco(pk_ctx* ctx, int32_t field_h, int32_t field_zeta, double hc, int32_t n, const double* sigma_levels, const double* cs_w,
                     int32_t cs_w_f32) {
    if (!ctx || !sigma_levels || !cs_w) return -2;
    const int nf = (int)ctx->fields.size();
    if (field_h < 0 || field_h >= nf || field_zeta < 0 || field_zeta >= nf) return ctx->fail("pk_set_croco: h / zeta name no field");
    if (n < 2) return ctx->fail("pk_set_croco: at least two sigma levels");
    if ((size_t)n * 16 > 48 * 1024) return ctx->fail("pk_set_croco: too many sigma levels for the workgroup's LDS");
    if (ctx->in_flight) return ctx->fail("pk_set_croco: a launch is in flight (call pk_execute_end)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> pairs((size_t)n * 2);
    for (int k = 0; k < n; k++) {
        pairs[2 * k] = sigma_levels[k];
        pairs[2 * k + 1] = cs_w[k];
    }
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    if (ctx->d_sigma) (void)hipFree(ctx->d_sigma);
    ctx->d_sigma = nullptr;
    ctx->has_sigma = false;
    PK_HIP(ctx, hipMalloc((void**)&ctx->d_sigma, pairs.size() * sizeof(double)));
    PK_HIP(ctx, hipMemcpy(ctx->d_sigma, pairs.data(), pairs.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->sigma = SigmaA{ctx->d_sigma, n, field_h, field_zeta, cs_w_f32 ? 1 : 0, hc};
    ctx->has_sigma = true;
    return 0;
}

int32_t pk_sigma_croco(pk_ctx* ctx, int64_t m, const double* t, const double* z, const double* y, const double* x, double* out_sigma) {
    if (!ctx || !t || !z || !y || !x || !out_sigma) return -2;
    if (!ctx->has_sigma) return ctx->fail("pk_sigma_croco needs the CROCO parameters of the context (pk_set_croco)");
    if (ctx_is_typed(ctx)) return ctx->fail("the CROCO conversion needs float64 coordinate arrays");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (m <= 0) return 0;
    pk_exec_params p2;
    memset(&p2, 0, sizeof(p2));
    p2.nk = 1;
    p2.fU = p2.fV = ctx->sigma.fh;
    p2.fW = p2.fKh_zonal = p2.fKh_meridional = -1;
    DParticles saved = ctx->dev;
    const bool was_bound = ctx->bound;
    KArgs a;
    size_t lds_bytes;
    int use_lds;
    ctx->bound = true;
    int32_t rc = launch_args(ctx, &p2, a, lds_bytes, use_lds);
    if (!rc) rc = upload_descriptors(ctx, a);
    ctx->bound = was_bound;
    ctx->dev = saved;
    if (rc) return rc;
    a.sigma = ctx->sigma;
    double* d = nullptr;
    PK_HIP(ctx, hipMalloc((void**)&d, sizeof(double) * m * 5));
    hipError_t e = hipSuccess;  // (no early return between hipMalloc and hipFree)
    const double* src[4] = {t, z, y, x};
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipMemcpyAsync(d + k * m, src[k], sizeof(double) * m, hipMemcpyHostToDevice, ctx->compute);
    if (e == hipSuccess) {
        launch_sigma_points(a, m, d, d + m, d + 2 * m, d + 3 * m, d + 4 * m, (size_t)ctx->sigma.n * 2 * sizeof(double), ctx->compute);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_sigma, d + 4 * m, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->compute);
    const hipError_t es = hipStreamSynchronize(ctx->compute);
    (void)hipFree(d);
    PK_HIP(ctx, e);
    PK_HIP(ctx, es);
    return 0;
}

}  // extern "C"
