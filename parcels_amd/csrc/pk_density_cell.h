// pk_density_cell.h -- the cell rule of ParticleSet.density, shared by pk_density.hip and pk_connectivity.hip (DESIGN.md sections 14, 15).
// The rule is not restated here: grid_search<-1, false> (pk_device.h) and ux_search (pk_ux.h) are the searches pk_search runs.
//
// pk_ux.h defines the device functions of the UxGrid search only in a translation unit that asks for them (PK_UX_KERNELS) and keeps the
// library's own point kernels out of a unit that carries PK_USER_KERNELS -- the pair of switches a run-time compiled user module sets.  This
// header sets both for the same reason (its units want the functions, not a second copy of the kernels); they have no user kernel, so the
// locals struct is empty and user_prepare is never called.  Include it before any other project header.
#pragma once
#include <hip/hip_runtime.h>

struct PkUserLocals {};
#pragma clang diagnostic ignored "-Wundefined-inline"  // user_prepare: declared for the user modules, never called here
#define PK_UX_KERNELS
#define PK_USER_KERNELS
#include "pk_ux.h"

namespace pk {

constexpr int DENS_WG = 256;
constexpr int64_t DENS_LDS_BINS = 8192;  // 32 KiB of uint32 bins per workgroup
constexpr long long DENS_PAD = -2;  // key of a lane past the last row: a run of its own that adds nothing

// The cell of one point, or -1 (outside).  levels: the Z index counts too.  dims: max(xdim, 1), max(ydim, 1), max(zdim, 1).
PK_DEV long long density_cell(const DGrid& g, bool levels, double z, double y, double x, int dx, int dy, int dz) {
    if (!(isfinite(x) && isfinite(y) && (!levels || isfinite(z)))) return -1;  // before the search: a NaN is in no cell (pk_density.h)
    int zi, yi, xi;
    if (g.kind == PK_UX_KIND) {
        UxPos p;
        int nodes[3];
        ux_search(g, z, y, x, false, 0, p, nodes);
        zi = p.zi; yi = 0; xi = p.fi;
    } else {
        PCtx c;
        c.state = PK_EVALUATE;
        c.pf = false;
        c.hz = c.hy = c.hx = c.ht = 0;
        c.hyx_valid = false;
        c.zpos_f32 = false;
        GPos p;
        int32_t ei = 0;
        grid_search<-1, false>(g, nullptr, z, y, x, false, &ei, c, false, p);
        zi = p.zi; yi = p.yi; xi = p.xi;
    }
    if (!levels) zi = 0;
    // error codes are negative; an index past the map cannot come out of the searches and would be a write out of bounds
    if (xi < 0 || yi < 0 || zi < 0 || xi >= dx || yi >= dy || zi >= dz) return -1;
    return ((long long)zi * dy + yi) * dx + xi;
}

// The grid dims the cell is ravelled over (density_shape of engine.py).
inline void density_dims(const DGrid& g, int32_t levels, int& dx, int& dy, int& dz) {
    dx = g.xdim > 0 ? g.xdim : 1;
    dy = (g.has_y && g.ydim > 0) ? g.ydim : 1;
    dz = (levels && g.has_z && g.zdim > 0) ? g.zdim : 1;
}

}  // namespace pk
