// pk_ux.h -- unstructured triangle meshes (UxGrid, src/parcels/_core/uxgrid.py): the face search, the four Ux* interpolators,
// Ux_Velocity and the fused step loop for a launch whose main grid is a UxGrid.
//
// A UxGrid shares the DGrid descriptor of the structured grids (the descriptor table and KArgs keep their layout):
//   kind = PK_UX_KIND, nx = n_face, ny = 1, nz = number of zf levels, has_x = has_z = 1, has_y = 0, xdim = n_face, zdim = nz, depth = zf,
//   cell_tab = the per-face records below, h_* = the CSR Morton table of SpatialHash over the face bounding boxes (spatialhash.py:164-206),
//   lon = node_lon (flat) / unused, lat = unused.
// `ei` is the ravel over the axes ("Z", "FACE") (basegrid.py:83-152): zi * n_face + fi.
//
// Per-face record (built once by pk_ugrid_create, 64-byte aligned, read with one 64 / 128-byte gather per face test):
//   flat      (UXF_FLAT doubles):  lon0 lat0 lon1 lat1 lon2 lat2 | node ids n0 n1 n2 (int32) | pad
//   spherical (UXF_SPH doubles):   X0 Y0 Z0 X1 Y1 Z1 X2 Y2 Z2 | nhat (3) | area of the face | node ids (int32 x 3) | pad
// nhat is np.cross(r1, r2) / norm (norm 1 where it is 0) and the area 0.5 * norm(cross(v1 - v0, v2 - v0)) -- the query-independent part
// of uxgrid_point_in_cell (index_search.py:298-436), formed on the host with the reference's operation order.
#pragma once
#include "pk_kernels.h"

#define PK_UX_KIND 2

namespace pk {

constexpr int PROG_UX = 6;  // the program of a launch on a UxGrid (pk_exec_stats.program)

constexpr int UXF_FLAT = 8;
constexpr int UXF_SPH = 16;
constexpr double UX_BC_TOL = -1e-6;               // coords >= -1e-6 (index_search.py:376)
constexpr double UX_SUM_TOL = 1e-6 + 1e-3 * 1.0;  // np.isclose(sum, 1.0, rtol=1e-3, atol=1e-6): |sum - 1| <= atol + rtol * |1|

// launchers (pk_prog_ux.hip: the library's translation unit that defines PK_UX_KERNELS and so the kernels below; the only other one is the
// module parcels_amd/jit.py generates for a kernel list with user kernels, which instantiates advect_ux_kernel with PK_USER_KERNELS)
void launch_ux(int particles_f32, const KArgs& a, int64_t n, hipStream_t stream);
void launch_ux_eval(const KArgs& a, int what, int64_t m, const double* t, const double* z, const double* y, const double* x, double* ou,
                    double* ov, double* ow, int32_t* ost, hipStream_t stream);
void launch_ux_eval_attached(const KArgs& a, int what, int64_t m, const double* t, const double* z, const double* y, const double* x, int32_t* ei,
                             double* ou, double* ov, double* ow, int32_t* ost, hipStream_t stream);
void launch_ux_search(const DGrid& g, int64_t m, const double* z, const double* y, const double* x, int32_t* ei, hipStream_t stream);

#ifdef PK_UX_KERNELS
typedef double pk_ux_double2 __attribute__((ext_vector_type(2), aligned(16)));

// where a sample lies on a UxGrid
struct UxPos {
    int ti, zi, fi;
    double tau;
    double b[3];   // barycentric coordinates of the point in face fi (float32-rounded when the hash found it: spatialhash.py:511)
    bool hashed;   // the face came from the hash query (an unguessed search, or a guess that missed)
};

// the query point of UxGrid.search: x, y cast to float32 (uxgrid.py:107-109); on a sphere deg2rad / cos / sin in float32
struct UxQuery {
    float xf, yf;
    double qx, qy, qz;  // hash coordinates: (lon, lat, 0) flat, unit-sphere xyz spherical (widened float32 values)
};
PK_DEV UxQuery ux_query(const DGrid& g, double y, double x) {
    UxQuery q;
    q.xf = (float)x;
    q.yf = (float)y;
    if (g.spherical) {
        // float32 sin / cos correctly rounded (through double): NumPy's float32 loops are not, by an ulp for about one argument in six --
        // the one residual of the spherical search, and only a correctly rounded device side lets the tests name
        // the points it touches
        const float lat = q.yf * DEG2RADF, lon = q.xf * DEG2RADF;
        const float cl = (float)cos((double)lat);
        q.qx = (double)((float)cos((double)lon) * cl);
        q.qy = (double)((float)sin((double)lon) * cl);
        q.qz = (double)(float)sin((double)lat);
    } else {
        q.qx = (double)q.xf;
        q.qy = (double)q.yf;
        q.qz = 0.0;
    }
    return q;
}

PK_DEV double ux_area2(double ax, double ay, double bx, double by, double cx, double cy) {  // _triangle_area, 2-D (signed)
    const double d1x = bx - ax, d1y = by - ay, d2x = cx - ax, d2y = cy - ay;
    return 0.5 * (d1x * d2y - d1y * d2x);
}
PK_DEV double ux_area3(const double A[3], const double B[3], const double C[3]) {  // _triangle_area, 3-D: 0.5 * norm(cross)
    const double d1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const double d2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    const double c0 = d1[1] * d2[2] - d1[2] * d2[1];
    const double c1 = d1[2] * d2[0] - d1[0] * d2[2];
    const double c2 = d1[0] * d2[1] - d1[1] * d2[0];
    return 0.5 * sqrt((c0 * c0 + c1 * c1) + c2 * c2);
}

// the three int32 node ids stored in the bits of two record doubles
PK_DEV void ux_node_ids(double d0, double d1, int nodes[3]) {
    const unsigned long long b0 = (unsigned long long)__double_as_longlong(d0), b1 = (unsigned long long)__double_as_longlong(d1);
    nodes[0] = (int)(uint32_t)b0;
    nodes[1] = (int)(uint32_t)(b0 >> 32);
    nodes[2] = (int)(uint32_t)b1;
}

// uxgrid_point_in_cell for one (point, face): barycentric coordinates and the inside test; node ids of the face as a by-product
PK_DEV bool ux_point_in_face(const DGrid& g, const UxQuery& q, int face, double b[3], int nodes[3]) {
    if (g.spherical) {
        const pk_ux_double2* r = reinterpret_cast<const pk_ux_double2*>(g.cell_tab + (int64_t)face * UXF_SPH);
        pk_ux_double2 w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = r[k];
        const double V0[3] = {w[0].x, w[0].y, w[1].x}, V1[3] = {w[1].y, w[2].x, w[2].y}, V2[3] = {w[3].x, w[3].y, w[4].x};
        const double n[3] = {w[4].y, w[5].x, w[5].y};
        const double a = w[6].x;
        ux_node_ids(w[6].y, w[7].x, nodes);
        // points - v0, its normal component, the point with it removed (index_search.py:345-352)
        const double pt[3] = {q.qx - V0[0], q.qy - V0[1], q.qz - V0[2]};
        const double pd = (pt[0] * n[0] + pt[1] * n[1]) + pt[2] * n[2];
        const double P[3] = {(pt[0] - pd * n[0]) + V0[0], (pt[1] - pd * n[1]) + V0[1], (pt[2] - pd * n[2]) + V0[2]};
        b[0] = ux_area3(P, V1, V2) / a;
        b[1] = ux_area3(P, V2, V0) / a;
        b[2] = ux_area3(P, V0, V1) / a;
    } else {
        const pk_ux_double2* r = reinterpret_cast<const pk_ux_double2*>(g.cell_tab + (int64_t)face * UXF_FLAT);
        pk_ux_double2 w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = r[k];
        ux_node_ids(w[3].x, w[3].y, nodes);
        const double px = (double)q.xf, py = (double)q.yf;
        const double a = ux_area2(w[0].x, w[0].y, w[1].x, w[1].y, w[2].x, w[2].y);
        b[0] = ux_area2(px, py, w[1].x, w[1].y, w[2].x, w[2].y) / a;
        b[1] = ux_area2(px, py, w[2].x, w[2].y, w[0].x, w[0].y) / a;
        b[2] = ux_area2(px, py, w[0].x, w[0].y, w[1].x, w[1].y) / a;
    }
    const bool pos = b[0] >= UX_BC_TOL && b[1] >= UX_BC_TOL && b[2] >= UX_BC_TOL;
    const double s = (b[0] + b[1]) + b[2];
    return pos && (fabs(s - 1.0) <= UX_SUM_TOL || s == 1.0);
}

// UxGrid.search for one point (uxgrid.py:105-135): the guessed face first (use_guess: the reference's `np.any(ei)`, applied per particle),
// then the candidates of the query's hash cell in table order (SpatialHash.query, spatialhash.py:389-535); none -> GRID_SEARCH_ERROR
PK_DEV void ux_search(const DGrid& g, double z, double y, double x, bool use_guess, int32_t ei, UxPos& p, int nodes[3]) {
    // vertical: _search_1d_array(zf, float32(z)) (uxgrid.py:111)
    double zeta;
    const double zf = (double)(float)z;
    search_1d(g.depth, g.nz, g.zfirst, g.zlast, zf, false, false, 0, p.zi, zeta);
    p.fi = GRID_SEARCH_ERROR;
    p.b[0] = p.b[1] = p.b[2] = -1.0;
    p.hashed = true;
    nodes[0] = nodes[1] = nodes[2] = 0;
    const UxQuery q = ux_query(g, y, x);
    if (use_guess) {
        const int gf = (int)mod64((int64_t)ei, (int64_t)g.nx);  // unravel (basegrid.py:219-252): the FACE index of ei
        double b[3];
        if (ux_point_in_face(g, q, gf, b, nodes)) {
            p.fi = gf;
            p.b[0] = b[0]; p.b[1] = b[1]; p.b[2] = b[2];
            p.hashed = false;
            return;
        }
    }
    if (!(isfinite(q.xf) && isfinite(q.yf)) || g.h_nkeys <= 0) return;  // spatialhash.py:441 (finite float32 query)
    const uint32_t code = (dilate_bits(quantize(q.qz, g.h_bbox[4], g.h_bbox[5], g.h_bitwidth)) << 2) |
                          (dilate_bits(quantize(q.qy, g.h_bbox[2], g.h_bbox[3], g.h_bitwidth)) << 1) |
                          dilate_bits(quantize(q.qx, g.h_bbox[0], g.h_bbox[1], g.h_bitwidth));
    int64_t lo = 0, hi = g.h_nkeys;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (g.h_keys[mid] < code) lo = mid + 1; else hi = mid;
    }
    if (lo >= g.h_nkeys || g.h_keys[lo] != code) return;
    const int64_t s = g.h_starts[lo], c = g.h_counts[lo];
    for (int64_t k = 0; k < c; k++) {
        const int face = (int)g.h_faces[s + k];
        double b[3];
        if (ux_point_in_face(g, q, face, b, nodes)) {
            p.fi = face;
            p.b[0] = (double)(float)b[0];  // coords_best is a float32 array (spatialhash.py:511)
            p.b[1] = (double)(float)b[1];
            p.b[2] = (double)(float)b[2];
            return;
        }
    }
    nodes[0] = nodes[1] = nodes[2] = 0;
}

// the ei write and the state update of field.py:307-356 for a UxGrid sample
PK_DEV void ux_search_finish(const DGrid& g, int32_t* ei, PCtx& c, const UxPos& p) {
    *ei = (int32_t)((int64_t)p.zi * g.nx + p.fi);
    int s = c.state;
    if (p.fi == GRID_SEARCH_ERROR && s < PK_ERRORGRIDSEARCHING) s = PK_ERRORGRIDSEARCHING;
    if (p.zi == RIGHT_OUT_OF_BOUNDS && s < PK_ERROROUTOFBOUNDS) s = PK_ERROROUTOFBOUNDS;
    if (p.zi == LEFT_OUT_OF_BOUNDS && s < PK_ERRORTHROUGHSURFACE) s = PK_ERRORTHROUGHSURFACE;
    c.state = s;
}

// The Ux* interpolators (interpolators/_uxinterpolators.py) at level ti only: no interpolation in time.  kind: 5 UxConstantFaceConstantZC,
// 6 UxConstantFaceLinearZF, 7 UxLinearNodeConstantZC, 8 UxLinearNodeLinearZF.  zp: the particle's z as the reference hands it over
// (particle_positions["z"], not float32-cast).  float64 data only (the host refuses float32 data on a UxGrid).
PK_DEV double ux_interp(const DGrid& g, const DField& f, const UxPos& p, const int nodes[3], double zp) {
    const double* d = (const double*)f.data + slot_off(f, p.ti);
    const int kind = f.is_const;
    const bool zf = kind == 6 || kind == 8;
    const bool node = kind == 7 || kind == 8;
    auto level = [&](int zi) -> double {
        const double* lv = d + (int64_t)zi * f.st_z;
        if (!node) return lv[(int64_t)p.fi * f.st_x];
        // (node_data * bcoords).sum("nodes"), left to right
        return (lv[(int64_t)nodes[0] * f.st_x] * p.b[0] + lv[(int64_t)nodes[1] * f.st_x] * p.b[1]) + lv[(int64_t)nodes[2] * f.st_x] * p.b[2];
    };
    if (!zf) return level(p.zi);
    const double fzk = level(p.zi), fzkp1 = level(p.zi + 1);
    const double zk = g.depth[p.zi], zkp1 = g.depth[p.zi + 1];
    return (fzk * (zkp1 - zp) + fzkp1 * (zp - zk)) / (zkp1 - zk);
}

// the value of an out-of-bounds sample before _mask_outofbounds_values zeroes it: NaN only through non-finite vertical weights of a zf
// interpolator (face and node gathers of the reference wrap around to finite data) -> ErrorInterpolation
PK_DEV double ux_masked(const DField& f, double zp) {
    const bool zf = f.is_const == 6 || f.is_const == 8;
    return (zf && !isfinite(zp)) ? NAN : 0.0;
}

PK_DEV double ux_finish(PCtx& c, bool oob, double v) {
    if (v != v && c.state < PK_ERRORINTERPOLATION) c.state = PK_ERRORINTERPOLATION;
    if (oob) {
        v = 0.0;
        c.oob = true;
    }
    return v;
}

// time search + the call-wide OutsideTimeInterval of eval_uvw / eval_scalar (pk_device.h); false: the sample failed (state 70, value 0)
PK_DEV bool ux_time(const KArgs& a, PCtx& c, const DField& f, double t, UxPos& p) {
    const int klo = c.klo++;
    if (f.has_time_interval) {
        const int li = twe_listed_index(a, c.it, klo);
        if (li >= 0) {
            twe_justify(a, li, t, f.tlen);
            c.state = PK_ERROROUTSIDETIMEINTERVAL;
            return false;
        }
    }
    GPos gp;
    if (!time_search(f, f.time, t, 0, gp)) {
        c.state = PK_ERROROUTSIDETIMEINTERVAL;
        twe_note_all(a, c.it, klo);
        return false;
    }
    p.ti = gp.ti;
    p.tau = gp.tau;
    return true;
}

// VectorField.eval with Ux_Velocity (_uxinterpolators.py:209-229)
PK_DEV void ux_eval_uvw(const KArgs& a, PCtx& c, bool want_w, double t, double z, double y, double x, bool pos_f32, double& u, double& v,
                        double& w) {
    const DField& U = kfield(a, a.prm.fU);
    const DField& V = kfield(a, a.prm.fV);
    const DGrid& g = kgrid(a, U.grid);
    u = v = w = 0.0;
    c.u32 = c.v32 = false;
    UxPos p;
    if (!ux_time(a, c, U, t, p)) return;
    const bool use_guess = take_first_eval(c, U.grid) ? (a.prm.have_guess0 != 0) : true;
    int32_t ei = ei_get(c, U.grid);
    int nodes[3];
    ux_search(g, z, y, x, use_guess, ei, p, nodes);
    ux_search_finish(g, &ei, c, p);
    ei_set(c, U.grid, ei);
    const DField* W = (want_w && a.prm.fW >= 0) ? &kfield(a, a.prm.fW) : nullptr;
    const bool oob = p.fi < 0 || p.zi < 0;
    double uu, vv, ww = 0.0;
    if (!oob) {
        uu = ux_interp(g, U, p, nodes, z);
        vv = ux_interp(g, V, p, nodes, z);
        if (g.spherical) {  // u /= deg2m * cos(deg2rad(y)), v /= deg2m
            double conv;
            if (pos_f32) conv = (double)((float)g.deg2m * cosf((float)y * DEG2RADF));
            else conv = g.deg2m * cos_lat(y * DEG2RAD);
            uu /= conv;
            vv /= g.deg2m;
        }
        if (W) ww = ux_interp(g, *W, p, nodes, z);
    } else {
        uu = ux_masked(U, z);
        vv = ux_masked(V, z);
        if (W) ww = ux_masked(*W, z);
    }
    u = ux_finish(c, oob, uu);
    v = ux_finish(c, oob, vv);
    w = ux_finish(c, oob, ww);
}

// Field.eval of a scalar field: a Ux* interpolator on a UxGrid, or the structured path (XConstantField next to the mesh, ...)
PK_DEV double ux_eval_scalar(const KArgs& a, PCtx& c, int fidx, double t, double z, double y, double x, bool pos_f32) {
    const DField& f = kfield(a, fidx);
    const DGrid& g = kgrid(a, f.grid);
    if (g.kind != PK_UX_KIND) {  // (the field's own arrays: pk_eval of such a field makes its grid the main grid)
        const Coords mc{CellCache{nullptr, nullptr, nullptr}, f.time, g.depth, g.lat, g.lon, f.tfirst, f.tlast, g.zfirst, g.zlast, g.yfirst, g.ylast,
                        g.xfirst, g.xlast};
        return eval_scalar<double, false>(a, mc, c, fidx, t, z, y, x, pos_f32);
    }
    UxPos p;
    if (!ux_time(a, c, f, t, p)) return 0.0;
    const bool use_guess = take_first_eval(c, f.grid) ? (a.prm.have_guess0 != 0) : true;
    int32_t ei = ei_get(c, f.grid);
    int nodes[3];
    ux_search(g, z, y, x, use_guess, ei, p, nodes);
    ux_search_finish(g, &ei, c, p);
    ei_set(c, f.grid, ei);
    const bool oob = p.fi < 0 || p.zi < 0;
    return ux_finish(c, oob, oob ? ux_masked(f, z) : ux_interp(g, f, p, nodes, z));
}

// The fused step loop of advect_kernel (pk_kernels.h) with the evaluations of a UxGrid main grid: kernel-list interpreter over the
// built-in kernels whose stage machines sample U/V(/W) or scalar fields.  PFM: particle storage dtype (0 float64, 1 float32).
template <int PFM>
__global__ void __launch_bounds__(256, 2) advect_ux_kernel(const KArgs a) {
    const int64_t i = (int64_t)xcd_swizzle(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    unsigned long long steps = 0, attempts = 0, paused = 0;
    if (i < a.p.n) {
        const DParticles& P = a.p;
        const DPOut& O = a.po;
        const pk_exec_params& prm = a.prm;
        PCtx c;
        const bool pf = PFM == 1;
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
                for (int k = 0; k < prm.nk; k++) {  // kernel.py:206-216
                    const int kid = prm.kernels[k];
                    c.klo = k * 1000;
                    do {
                        KLocal L;
                        L.u1f = L.v1f = false;
                        Request rq;
                        attempts++;
                        for (int stage = 0; !prepare(a, kid, stage, k, c, p, L, rq); stage++) {
                            double u, v = 0.0, w = 0.0;
                            c.zpos_f32 = rq.zf32;
                            if (rq.kind == RQ_SCALAR) u = ux_eval_scalar(a, c, rq.fidx, rq.t, rq.z, rq.y, rq.x, rq.f32);
                            else ux_eval_uvw(a, c, rq.kind == RQ_UVW, rq.t, rq.z, rq.y, rq.x, rq.f32, u, v, w);
                            consume(kid, stage, c, L, u, v, w);
                        }
                    } while (c.state == PK_REPEAT);
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
                    steps++;
                }
                p.dt = prm.dt0;                                                     // :225-226
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
// Field.eval / VectorField.eval at explicit points on a UxGrid (pk_eval): what >= 0 scalar field, -1 UV, -2 UVW.  No guess (ei = None).
__global__ void __launch_bounds__(256) eval_ux_kernel(const KArgs a, int what, int64_t m, const double* t, const double* z, const double* y,
                                                      const double* x, double* ou, double* ov, double* ow, int32_t* ost) {
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
    const bool pos_f32 = a.prm.reset_state != 0;  // option "eval_points_f32" (pk_eval)
    c.zpos_f32 = pos_f32;
    if (what < 0) {
        double u, v, w;
        ux_eval_uvw(a, c, what == -2, t[i], z[i], y[i], x[i], pos_f32, u, v, w);
        ou[i] = u;
        if (ov) ov[i] = v;
        if (ow) ow[i] = w;
    } else {
        ou[i] = ux_eval_scalar(a, c, what, t[i], z[i], y[i], x[i], pos_f32);
    }
    if (ost) ost[i] = c.state | (c.oob ? PK_EVAL_MASKED : 0);
}

// The same WITH the particles the points belong to (pk_eval_attached; field.py:394-405): the search starts from the particles' `ei` on the
// sampled field's grid when the batch has a guess (a.prm.have_guess0: the reference's np.any(ei)), and `ei` returns the cell of the sample
// point -- what one evaluation of the step loop above does for its particle.
__global__ void __launch_bounds__(256) eval_ux_attached_kernel(const KArgs a, int what, int64_t m, const double* t, const double* z, const double* y,
                                                               const double* x, int32_t* ei, double* ou, double* ov, double* ow, int32_t* ost) {
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
    const int grid = kfield(a, what < 0 ? a.prm.fU : what).grid;
    ei_set(c, grid, ei[i]);
    const bool pos_f32 = a.prm.reset_state != 0;  // option "eval_points_f32" (pk_eval)
    c.zpos_f32 = pos_f32;
    if (what < 0) {
        double u, v, w;
        ux_eval_uvw(a, c, what == -2, t[i], z[i], y[i], x[i], pos_f32, u, v, w);
        ou[i] = u;
        if (ov) ov[i] = v;
        if (ow) ow[i] = w;
    } else {
        ou[i] = ux_eval_scalar(a, c, what, t[i], z[i], y[i], x[i], pos_f32);
    }
    ei[i] = ei_get(c, grid);
    if (ost) ost[i] = c.state | (c.oob ? PK_EVAL_MASKED : 0);
}

// UxGrid.search + ravel_index with no guess (pk_search)
__global__ void __launch_bounds__(256) search_ux_kernel(const DGrid g, int64_t m, const double* z, const double* y, const double* x, int32_t* ei) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    UxPos p;
    int nodes[3];
    ux_search(g, z[i], y[i], x[i], false, 0, p, nodes);
    ei[i] = (int32_t)((int64_t)p.zi * g.nx + p.fi);
}
#endif  // !PK_USER_KERNELS

#endif  // PK_UX_KERNELS

}  // namespace pk
