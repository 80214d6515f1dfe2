// pk_sigma.h -- CROCO terrain-following (sigma) grids: convert_z_to_sigma_croco, AdvectionRK2_3D_CROCO and the sigma-level sampling kernel
// (src/parcels/kernels/_sigmagrids.py), with the fused step loop of a launch whose kernel list holds one of them.
//
// The vertical axis of a CROCO fieldset is the sigma coordinate s_w in [-1, 0]; every sample first turns the particle's depth z into a
// sigma level through the local bathymetry h, the free surface zeta and the stretching curve Cs_w (_sigmagrids.py:6-25).  Two kinds of
// sample appear in the kernels (field.py:145-195, 307-378):
//   attached  `F.eval(..., particles=particle)` / `F[t, z, y, x, particles]`: guess from `ei`, `ei` written back, error codes raised into `state`;
//   detached  `fieldset.h[t, 0, y, x]`: no guess (a curvilinear search goes through the spatial hash and returns float32 cell coordinates),
//             no `ei` write, no state change.  Out-of-bounds values are 0 in both.
// NumPy's dtype rules (NEP 50) along _sigmagrids.py: XLinear returns float64 whenever a barycentric array is float64, so on float64
// coordinates the only float32 ARRAY a sample can return is h (no time and no depth axis) of float32 data after an unguessed curvilinear
// search; `(h - hc) * Cs_w`, `z / h` and `sigma / h` are then float32 operations where both operands are float32 (sig_eval: v32).
#pragma once
#include "pk_kernels.h"

namespace pk {

constexpr int PROG_SIGMA = 7;  // the program of a launch with a CROCO kernel in its list (pk_exec_stats.program)

// launchers (pk_prog_sigma.hip: the library's translation unit that defines PK_SIGMA_KERNELS and so the kernels below; the only other one is
// the module parcels_amd/jit.py generates for a kernel list with user kernels on a CROCO fieldset, which instantiates advect_sigma_kernel
// with PK_USER_KERNELS)
#ifndef PK_USER_KERNELS
void launch_sigma(int field_f32, int curvilinear, int interp, const KArgs& a, int64_t n, size_t lds_bytes, hipStream_t stream);
void launch_sigma_points(const KArgs& a, int64_t m, const double* t, const double* z, const double* y, const double* x, double* out,
                         size_t lds_bytes, hipStream_t stream);
#endif

#ifdef PK_SIGMA_KERNELS

// {s_k, Cs_k} pairs of the sigma levels, staged once per workgroup (16 bytes per level)
PK_DEV const pk_tab2* sigma_stage(const SigmaA& S, double* smem, int wg) {
    pk_tab2* s_tab = reinterpret_cast<pk_tab2*>(smem);
    const pk_tab2* g_tab = reinterpret_cast<const pk_tab2*>(S.tab);
    for (int k = threadIdx.x; k < S.n; k += wg) s_tab[k] = g_tab[k];
    __syncthreads();
    return s_tab;
}

// convert_z_to_sigma_croco (_sigmagrids.py:6-25) for one particle.  tab: the {s_k, Cs_k} pairs in LDS; h32: h is a float32 array in the
// reference (see the head of this file).  The level is the reference's: zi = (first k with not zvec_k <= z) - 1, n - 2 when there is none,
// and -1 (Python's wrap-around in the gathers) when level 0 already qualifies.  Every lane reads level k at the same time (one broadcast
// LDS address); the trip count is the largest exit of the wavefront.
PK_DEV double croco_sigma(const pk_tab2* tab, const SigmaA& S, double h, bool h32, double zeta, double z) {
    const int n = S.n;
    const double hc = S.hc;
    const bool cs32 = S.cs_f32 != 0;
    const float hmf = (float)h - (float)hc;  // `h[:, None] - fieldset.hc`: hc is a Python float (weak), the difference keeps h's dtype
    const double hm = h32 ? (double)hmf : h - hc;
    auto zvec = [&](const pk_tab2 e) -> double {
        const double hmcs = (h32 && cs32) ? (double)(hmf * (float)e.y) : hm * e.y;
        const double z0 = hc * e.x + hmcs;
        return z0 + zeta * (1.0 + (z0 / h));
    };
    int kf = -1;
    for (int k = 0; k < n; k++) {
        const double zv = zvec(tab[k]);
        if (kf < 0 && !(zv <= z)) kf = k;  // np.argmin(zvec <= z): the first False, a NaN included
        if (__all(kf >= 0)) break;
    }
    const int zi = kf < 0 ? n - 2 : kf - 1;
    const pk_tab2 ea = tab[zi < 0 ? n - 1 : zi], eb = tab[zi + 1];
    const double zva = zvec(ea), zvb = zvec(eb);
    return ea.x + (z - zva) * (eb.x - ea.x) / (zvb - zva);
}

// Field.eval of a scalar field, attached or detached (see the head of this file).  v32: the value is a float32 array in the reference.
// The attached form is eval_scalar (pk_device.h) without the search memo.
// left_time (optional): set when THIS attached sample lies outside the field's time interval.
PK_DEV double sig_eval(const KArgs& a, const Coords& mc, PCtx& c, int fidx, double t, double z, double y, double x, bool pos_f32, bool detached,
                       bool& v32, bool* left_time = nullptr) {
    const DField& f = kfield(a, fidx);
    const DGrid& g = kgrid(a, f.grid);
    v32 = false;
    GPos p;
    bool on_main = false;
    const int state0 = c.state;
    const bool oob0 = c.oob;
    int32_t ei = 0;
    if (detached) {
        // (h, the only field the kernels sample detached, has no time axis -- checked on the host; pk_sigma_croco's callers check t against
        // zeta's interval, where the reference raises for the whole call: a point outside it gets NaN, no state is touched)
        if (!time_search(f, f.time, t, 0, p)) return NAN;
        grid_search<-1, false>(g, nullptr, z, y, x, pos_f32, &ei, c, false, p);
    } else {
        on_main = f.grid == a.main_grid;
        const double* time = (on_main && f.time == kfield(a, a.main_field).time) ? mc.time : f.time;
        const int klo = c.klo++;
        if (f.has_time_interval) {
            const int li = twe_listed_index(a, c.it, klo);
            if (li >= 0) {  // (see eval_uvw)
                twe_justify(a, li, t, f.tlen);
                c.state = PK_ERROROUTSIDETIMEINTERVAL;
                if (left_time) *left_time = true;
                return 0.0;
            }
        }
        if (!time_search(f, time, t, on_main ? c.ht : 0, p)) {
            c.state = PK_ERROROUTSIDETIMEINTERVAL;
            twe_note_all(a, c.it, klo);
            if (left_time) *left_time = true;
            return 0.0;
        }
        const bool use_guess = take_first_eval(c, f.grid) ? (a.prm.have_guess0 != 0) : true;
        ei = ei_get(c, f.grid);
        grid_search<-1, false>(g, on_main ? &mc : nullptr, z, y, x, pos_f32, &ei, c, use_guess, p);
        ei_set(c, f.grid, ei);
    }
    double v = 0.0;
    if (!(p.xi < 0 || p.yi < 0 || p.zi < 0)) {
        const bool f64 = f.dtype == PK_F64;
        switch (f.is_const) {
            case 1: v = f64 ? ((const double*)f.data)[f.comp] : (double)((const float*)f.data)[f.comp]; break;
            case 2: v = f64 ? xnearest<double>(f, p) : xnearest<float>(f, p); break;
            case 3: v = f64 ? cgrid_tracer<double>(g, f, p) : cgrid_tracer<float>(g, f, p); break;
            case 4: v = f64 ? xlinear_invdist<double>(f, p, a.prm.force_lent, a.prm.force_lenz) : xlinear_invdist<float>(f, p, a.prm.force_lent, a.prm.force_lenz); break;
            default: v = f64 ? xlinear<double>(f, make_corners(f, p), p, &v32) : xlinear<float>(f, make_corners(f, p), p, &v32); break;
        }
    }
    v = finish_value(c, p, v);
    if (detached) {  // no state change, no mark of a masked value
        c.state = state0;
        c.oob = oob0;
    }
    return v;
}

// what a stage of the CROCO kernels asks of the evaluation site beyond Request
struct SigRq {
    bool detached;  // a detached scalar sample
};
// registers of the CROCO kernels next to KLocal::r --
//   r[0] sigma  r[1] h of the conversion  r[2] w  r[3] u  r[4] v  r[5] dep2  r[6] x1  r[7] y1  r[8] sig_dep1  r[9] dep1  r[10] sig  r[11] x2  r[12] y2  r[13] sig_dep2
struct SigLocal {
    bool sigma32;  // `sigma = particles.z / h` is a float32 array
    bool h32;      // the h of the conversion is
};

PK_DEV bool is_croco_id(int kid) { return kid == PK_KERNEL_ADVECTION_RK2_3D_CROCO || kid == PK_KERNEL_SAMPLE_SIGMA_CROCO; }
// the stages whose sample is one of convert_z_to_sigma_croco's `fieldset.h.eval(...)` / `fieldset.zeta.eval(...)` (_sigmagrids.py:12-13): called
// directly, not through Field.__getitem__, so an OutsideTimeInterval there is not turned into a status code (field.py:187-195) but leaves the
// kernel and ParticleSet.execute -- no kernel later in the list (DeleteParticle, say) gets to see the particle
PK_DEV bool is_conversion_stage(int kid, int stage) {
    if (kid == PK_KERNEL_SAMPLE_SIGMA_CROCO) return stage <= 1;
    return stage == 1 || stage == 2 || stage == 7 || stage == 8;
}

// A stage of a translated user kernel whose sample is one of convert_z_to_sigma_croco's (Request::conv): the loop treats it like the
// conversion stages of the built-in kernels -- the OutsideTimeInterval of such a sample leaves the kernel list -- and folds the two samples
// into the sigma level, which it leaves in L.r[3], where a user stage finds the value of its latest sample.  (h and its dtype wait in
// L.r[1] / sl.h32 as in croco_consume: a generated stage never touches L.r.)  The library's own instantiations know no such stage.
#ifdef PK_USER_KERNELS
PK_DEV void user_stage_begin(Request& rq) { rq.conv = 0; }
PK_DEV bool user_conversion_stage(const Request& rq) { return rq.conv != 0; }
PK_DEV void user_conversion_consume(const KArgs& a, const pk_tab2* tab, const Request& rq, KLocal& L, SigLocal& sl, double u, bool v32) {
    if (rq.conv == 1) { L.r[1] = u; sl.h32 = v32; }
    else L.r[3] = croco_sigma(tab, a.sigma, L.r[1], sl.h32, u, rq.cz);
}
#else
PK_DEV void user_stage_begin(Request&) {}
PK_DEV bool user_conversion_stage(const Request&) { return false; }
PK_DEV void user_conversion_consume(const KArgs&, const pk_tab2*, const Request&, KLocal&, SigLocal&, double, bool) {}
#endif

// prepare() of the two CROCO kernels: true when the kernel is finished
PK_DEV bool croco_prepare(const KArgs& a, int kid, int stage, int kslot, PCtx& c, PState& p, KLocal& L, Request& rq, SigRq& sq) {
    const SigmaA& S = a.sigma;
    const bool pf = c.pf;
    rq.kind = RQ_SCALAR;
    rq.fidx = S.fh;
    rq.f32 = pf;
    rq.zf32 = pf;
    rq.reuse = false;
    rq.t = p.t; rq.z = 0.0; rq.y = p.y; rq.x = p.x;  // np.zeros_like(z): h and zeta live on the surface
    sq.detached = false;
    if (kid == PK_KERNEL_SAMPLE_SIGMA_CROCO) {  // _sigmagrids.py:28-35
        switch (stage) {
            case 0: return false;                     // h (conversion)
            case 1: rq.fidx = S.fzeta; return false;  // zeta
            case 2:
                rq.fidx = a.prm.sample_field[kslot];
                rq.z = L.r[10];
                rq.zf32 = false;
                return false;
            default: break;
        }
        L.r[0] = L.r[2];
        return prepare(a, PK_KERNEL_SAMPLE_FIELD, 1, kslot, c, p, L, rq);  // the assignment into the Variable
    }
    // AdvectionRK2_3D_CROCO, _sigmagrids.py:38-72
    const double th = p.t + 0.5 * p.dt;
    switch (stage) {
        case 0: sq.detached = true; return false;  // :50
        case 1: return false;                      // :52 h
        case 2: rq.fidx = S.fzeta; return false;   // :52 zeta
        case 3: rq.kind = RQ_UV; rq.z = L.r[10]; rq.zf32 = false; return false;                     // :53
        case 4: rq.fidx = a.prm.fW; rq.z = L.r[10]; rq.zf32 = false; return false;                  // :54
        case 5: sq.detached = true; return false;                                                   // :55
        case 6: sq.detached = true; rq.f32 = false; rq.y = L.r[7]; rq.x = L.r[6]; return false;     // :59
        case 7: rq.f32 = false; rq.t = th; rq.y = L.r[7]; rq.x = L.r[6]; return false;              // :61 h
        case 8: rq.fidx = S.fzeta; rq.f32 = false; rq.t = th; rq.y = L.r[7]; rq.x = L.r[6]; return false;  // :61 zeta
        case 9: rq.kind = RQ_UV; rq.f32 = false; rq.t = th; rq.z = L.r[10]; rq.zf32 = false; rq.y = L.r[7]; rq.x = L.r[6]; return false;  // :62
        case 10: rq.fidx = a.prm.fW; rq.f32 = false; rq.t = th; rq.z = L.r[10]; rq.zf32 = false; rq.y = L.r[7]; rq.x = L.r[6]; return false;  // :63
        case 11: sq.detached = true; rq.f32 = false; rq.t = th; rq.y = L.r[7]; rq.x = L.r[6]; return false;   // :64
        case 12: sq.detached = true; rq.f32 = false; rq.t = th; rq.y = L.r[12]; rq.x = L.r[11]; return false; // :68
        default: break;
    }
    p.dx = pstore(pf, p.dx + L.r[3] * p.dt);                          // :70-72
    p.dy = pstore(pf, p.dy + L.r[4] * p.dt);
    p.dz = pstore(pf, p.dz + ((L.r[9] - p.z) + (L.r[5] - p.z)));
    return true;
}

// consume() of the two CROCO kernels: u = the sampled value (v32: a float32 array in the reference), or (u, v) of a velocity sample
PK_DEV void croco_consume(const KArgs& a, const pk_tab2* tab, int kid, int stage, const PCtx& c, const PState& p, KLocal& L, SigLocal& sl, double u,
                          double v, bool v32) {
    const bool pf = c.pf;
    if (kid == PK_KERNEL_SAMPLE_SIGMA_CROCO) {
        if (stage == 0) { L.r[1] = u; sl.h32 = v32; }
        else if (stage == 1) L.r[10] = croco_sigma(tab, a.sigma, L.r[1], sl.h32, u, p.z);
        else L.r[2] = u;
        return;
    }
    switch (stage) {
        case 0:  // sigma = particles.z / h
            sl.sigma32 = pf && v32;
            L.r[0] = sl.sigma32 ? (double)((float)p.z / (float)u) : p.z / u;
            break;
        case 1: case 7: L.r[1] = u; sl.h32 = v32; break;
        case 2: L.r[10] = croco_sigma(tab, a.sigma, L.r[1], sl.h32, u, p.z); break;
        case 8: L.r[10] = croco_sigma(tab, a.sigma, L.r[1], sl.h32, u, L.r[9]); break;
        case 3: case 9: L.r[3] = u; L.r[4] = v; break;
        case 4: case 10: L.r[2] = u; break;
        case 5: {  // w1 *= sigma / h; x1, y1, sig_dep1
            const double q = (sl.sigma32 && v32) ? (double)((float)L.r[0] / (float)u) : L.r[0] / u;
            const double w1 = L.r[2] * q;
            L.r[6] = p.x + L.r[3] * 0.5 * p.dt;
            L.r[7] = p.y + L.r[4] * 0.5 * p.dt;
            L.r[8] = L.r[0] + w1 * 0.5 * p.dt;
            break;
        }
        case 6: L.r[9] = L.r[8] * u; break;  // dep1
        case 11: {  // w2 *= sig_dep1 / h; x2, y2, sig_dep2
            const double w2 = L.r[2] * (L.r[8] / u);
            L.r[11] = p.x + L.r[3] * 0.5 * p.dt;
            L.r[12] = p.y + L.r[4] * 0.5 * p.dt;
            L.r[13] = L.r[0] + w2 * 0.5 * p.dt;
            break;
        }
        default: L.r[5] = L.r[13] * u; break;  // dep2
    }
}

// The fused step loop of advect_kernel (pk_kernels.h) as a kernel-list interpreter that also carries the two CROCO kernels.  The 1-D
// coordinate vectors are searched in global memory; the dynamic LDS holds the {s_k, Cs_k} pairs.
// PK_SIGMA_MIN_WAVES: uncapped (1) the kernel wants 264 .. 282 vector registers and runs one wave per SIMD without scratch; at 2 waves per SIMD
// (256 registers) 14 .. 34 of them live in scratch across the evaluation (44 .. 124 bytes per lane).  Measured: DESIGN.md section 12.
#ifndef PK_SIGMA_MIN_WAVES
#define PK_SIGMA_MIN_WAVES 2
#endif
template <class FT, int KIND, int INTERP>
__global__ void __launch_bounds__(256, PK_SIGMA_MIN_WAVES) advect_sigma_kernel(const KArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const pk_tab2* tab = sigma_stage(a.sigma, smem, 256);
    const DField& mf = kfield(a, a.main_field);
    const DGrid& mg = kgrid(a, a.main_grid);
    Coords mc;
    mc.time = mf.time;
    mc.depth = mg.depth;
    mc.lat = mg.lat;
    mc.lon = mg.lon;
    mc.cc.nodes = nullptr;
    mc.cc.key = nullptr;
    mc.cc.fvals = nullptr;
    mc.t0 = mf.tfirst;
    mc.t1 = mf.tlast;
    mc.z0 = mg.zfirst; mc.z1 = mg.zlast;
    mc.y0 = mg.yfirst; mc.y1 = mg.ylast;
    mc.x0 = mg.xfirst; mc.x1 = mg.xlast;
    const int64_t i = (int64_t)xcd_swizzle(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    unsigned long long steps = 0, attempts = 0, paused = 0;
    if (i < a.p.n) {
        const DParticles& P = a.p;
        const DPOut& O = a.po;
        const pk_exec_params& prm = a.prm;
        PCtx c;
        const bool pf = P.spatial_f32 != 0;
        c.pf = pf;
        c.row = i;
        c.oob = false;
        const bool body = prm.body_only != 0;
        c.state = (prm.reset_state && !body) ? PK_EVALUATE : P.state[i];
        const bool run = body ? P.iter[i] != 0 : c.state == PK_EVALUATE;
        if (run) {
            unsigned it = (prm.reset_state || body) ? 0u : (unsigned)P.iter[i];
            c.it = 0u;
            c.klo = 0;
            c.hz = c.hy = c.hx = c.ht = 0;
            c.hyx_valid = false;
            c.first_eval = prm.reset_state ? 0xFu : 0u;
            c.u32 = c.v32 = false;
            PState p;
            p.t = P.t[i];
            p.z = ldp(P.z, i, pf);
            p.y = ldp(P.y, i, pf);
            p.x = ldp(P.x, i, pf);
            p.dz = ldp(P.dz, i, pf);
            p.dy = ldp(P.dy, i, pf);
            p.dx = ldp(P.dx, i, pf);
            p.dt = P.dt[i];
            p.next_dt = P.next_dt ? P.next_dt[i] : 0.0;
            p.id = P.particle_id[i];
            const int ng = P.ngrids;
            c.ei0 = P.ei[i * ng];
            c.ei1 = ng > 1 ? P.ei[i * ng + 1] : 0;
            c.ei2 = ng > 2 ? P.ei[i * ng + 2] : 0;
            c.ei3 = ng > 3 ? P.ei[i * ng + 3] : 0;
            const double endtime = prm.endtime;
            const int sign = prm.dt0 > 0 ? 1 : -1;
            const bool windowed = a.win_lo > -INFINITY || a.win_hi < INFINITY;
            bool once = body;
            while (once || (!body && (c.state == PK_EVALUATE || c.state == PK_REPEAT))) {  // kernel.py:190
                once = false;
                const double tte = sign * (endtime - p.t);
                if (!body && !(tte >= 0)) break;
                if (prm.max_iters > 0 && it >= (unsigned)prm.max_iters) break;
                double dtc;
                if (sign == 1) dtc = fmax(fmin(p.dt, tte), 0.0);
                else dtc = fmin(fmax(p.dt, -tte), 0.0);
                if (body) dtc = p.dt;
                if (windowed && !body) {
                    const double t1 = p.t + dtc;
                    const double lo = fmin(p.t, t1), hi = fmax(p.t, t1);
                    if (lo < a.win_lo || hi > a.win_hi) { paused = 1; break; }
                }
                it++;
                c.it = body ? 0u : it;
                p.dt = dtc;
                bool raised = false;  // (see is_conversion_stage)
                for (int k = 0; k < prm.nk && !raised; k++) {  // kernel.py:206-216
                    const int kid = prm.kernels[k];
                    const bool croco = is_croco_id(kid);
                    c.klo = k * 1000;
                    do {
                        KLocal L;
                        L.u1f = L.v1f = false;
                        SigLocal sl;
                        sl.sigma32 = sl.h32 = false;
                        Request rq;
                        SigRq sq;
                        sq.detached = false;
                        attempts++;
                        user_stage_begin(rq);
#pragma unroll 1
                        for (int stage = 0; !(croco ? croco_prepare(a, kid, stage, k, c, p, L, rq, sq) : prepare(a, kid, stage, k, c, p, L, rq)); stage++) {
                            double u, v = 0.0, w = 0.0;
                            bool v32 = false;
                            c.zpos_f32 = rq.zf32;
                            if (rq.kind == RQ_SCALAR) u = sig_eval(a, mc, c, rq.fidx, rq.t, rq.z, rq.y, rq.x, rq.f32, croco && sq.detached, v32, &raised);
                            else eval_uvw<FT, KIND, INTERP, false>(a, mc, c, rq.kind == RQ_UVW, rq.t, rq.z, rq.y, rq.x, rq.f32, u, v, w);
                            if (raised && !(croco ? is_conversion_stage(kid, stage) : user_conversion_stage(rq))) raised = false;
                            if (raised) break;  // the exception of the reference: the state stays ErrorOutsideTimeInterval
                            if (croco) croco_consume(a, tab, kid, stage, c, p, L, sl, u, v, v32);
                            else if (user_conversion_stage(rq)) user_conversion_consume(a, tab, rq, L, sl, u, v32);
                            else consume(kid, stage, c, L, u, v, w);
                            user_stage_begin(rq);
                        }
                    } while (c.state == PK_REPEAT && !raised);
                }
                if (body) break;
                if (c.state == PK_EVALUATE || c.state == PK_SUCCESS) {  // :219-222
                    if (tte > 0 && p.t + p.dt == p.t) {
                        c.state = PK_ERROR;  // (see advect_kernel: the reference would spin forever here)
                        break;
                    }
                    p.x = padd(pf, p.x, p.dx);
                    p.y = padd(pf, p.y, p.dy);
                    p.z = padd(pf, p.z, p.dz);
                    p.t += p.dt;
                    p.dx = p.dy = p.dz = 0.0;
                    if (prm.rk45_mode) p.dt = p.next_dt;
                    steps++;
                }
                if (!prm.rk45_mode) p.dt = prm.dt0;                                 // :225-226
                if (c.state == PK_EVALUATE && p.t == endtime) c.state = PK_ENDOFLOOP;  // :229-230
            }
            O.t[i] = p.t;
            stp(O.z, i, p.z, pf);
            stp(O.y, i, p.y, pf);
            stp(O.x, i, p.x, pf);
            stp(O.dz, i, p.dz, pf);
            stp(O.dy, i, p.dy, pf);
            stp(O.dx, i, p.dx, pf);
            O.dt[i] = p.dt;
            if (P.next_dt) O.next_dt[i] = p.next_dt;
            O.state[i] = c.state;
            O.ei[i * ng] = c.ei0;
            if (ng > 1) O.ei[i * ng + 1] = c.ei1;
            if (ng > 2) O.ei[i * ng + 2] = c.ei2;
            if (ng > 3) O.ei[i * ng + 3] = c.ei3;
            O.iter[i] = body ? P.iter[i] : (int32_t)it;
            if (!body) note_error_iteration(a, c.state, it);
        }
    }
    steps = wave_sum(steps);
    attempts = wave_sum(attempts);
    paused = wave_sum(paused);
    if ((threadIdx.x & 63) == 0) {
        if (steps) atomicAdd(&a.counters->steps, steps);
        if (attempts) atomicAdd(&a.counters->attempts, attempts);
        if (paused) atomicAdd(&a.counters->paused, paused);
    }
}

#ifndef PK_USER_KERNELS  // (a generated user module launches the step loop only)
// convert_z_to_sigma_croco(fieldset, t, z, y, x, None) at explicit points (pk_sigma_croco): both inner samples detached
__global__ void __launch_bounds__(256) sigma_points_kernel(const KArgs a, int64_t m, const double* t, const double* z, const double* y,
                                                           const double* x, double* out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const pk_tab2* tab = sigma_stage(a.sigma, smem, 256);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    PCtx c;
    c.state = PK_EVALUATE;
    c.pf = false;
    c.hz = c.hy = c.hx = c.ht = 0;
    c.hyx_valid = false;
    c.first_eval = 0xFu;
    c.u32 = c.v32 = false;
    c.oob = false;
    c.ei0 = c.ei1 = c.ei2 = c.ei3 = 0;
    c.it = 0u;
    c.klo = 0;
    c.row = i;
    c.zpos_f32 = false;
    Coords mc;  // (detached samples search the field's own grid arrays)
    mc.time = mc.depth = mc.lat = mc.lon = nullptr;
    mc.cc.nodes = nullptr;
    mc.cc.key = nullptr;
    mc.cc.fvals = nullptr;
    mc.t0 = mc.t1 = mc.z0 = mc.z1 = mc.y0 = mc.y1 = mc.x0 = mc.x1 = 0.0;
    bool h32 = false, z32 = false;
    const double h = sig_eval(a, mc, c, a.sigma.fh, t[i], 0.0, y[i], x[i], false, true, h32);
    const double zeta = sig_eval(a, mc, c, a.sigma.fzeta, t[i], 0.0, y[i], x[i], false, true, z32);
    out[i] = croco_sigma(tab, a.sigma, h, h32, zeta, z[i]);
}
#endif  // !PK_USER_KERNELS

#endif  // PK_SIGMA_KERNELS

}  // namespace pk
