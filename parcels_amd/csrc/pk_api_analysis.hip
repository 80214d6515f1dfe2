// pk_api_analysis.hip -- the entry points of the analyses on the device-resident columns, each a thin caller of a unit of its own: neighbour
// search (pk_neighbors.hip), built-in interaction kernels (pk_interact.hip), density (pk_density.hip), cells / connectivity (pk_connectivity.hip).
#include "pk_api_ctx.h"

using namespace pkapi;

extern "C" {

// ---- neighbour search (pk_neighbors.hip) ---------------------------------------------------------------
int32_t pk_neighbors_build(pk_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources, double radius,
                           int32_t flags) {
    if (!ctx) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->nbr) ctx->nbr = neighbors_create();
    std::string msg;
    if (neighbors_build(ctx->nbr, ctx->compute, n, x, y, z, sources, radius, flags, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_neighbors_counts(pk_ctx* ctx, int64_t* counts, int64_t* total) {
    if (!ctx) return -2;
    if (!ctx->nbr) return ctx->fail("pk_neighbors_counts: no cell list (pk_neighbors_build first)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    std::string msg;
    if (neighbors_counts(ctx->nbr, ctx->compute, counts, total, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_neighbors_nearest(pk_ctx* ctx, int64_t* j, double* dist) {
    if (!ctx) return -2;
    if (!ctx->nbr) return ctx->fail("pk_neighbors_nearest: no cell list (pk_neighbors_build first)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    std::string msg;
    if (neighbors_nearest(ctx->nbr, ctx->compute, j, dist, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_neighbors_pairs(pk_ctx* ctx, int64_t total, int64_t* starts, int64_t* j, double* dx, double* dy, double* dz, double* dist) {
    if (!ctx) return -2;
    if (!ctx->nbr) return ctx->fail("pk_neighbors_pairs: no cell list (pk_neighbors_build first)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    std::string msg;
    if (neighbors_pairs(ctx->nbr, ctx->compute, total, starts, j, dx, dy, dz, dist, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_neighbors_info(pk_ctx* ctx, pk_neighbors_info_t* out) {
    if (!ctx || !out) return -2;
    NeighborsInfo i;
    neighbors_info(ctx->nbr, &i);
    out->n = i.n;
    out->nvalid = i.nvalid;
    out->ncx = i.ncx;
    out->ncy = i.ncy;
    out->total = i.total;
    out->cell_size = i.h;
    out->doublings = i.doublings;
    out->reserved0 = 0;
    return 0;
}

int32_t pk_neighbors_build_spherical(pk_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, const uint8_t* sources,
                                     double radius_m, double sphere_radius_m, int32_t flags) {
    if (!ctx) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->nbr) ctx->nbr = neighbors_create();
    std::string msg;
    if (neighbors_build_spherical(ctx->nbr, ctx->compute, n, x, y, z, sources, radius_m, sphere_radius_m, flags, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_neighbors_info_spherical(pk_ctx* ctx, pk_neighbors_info_spherical_t* out) {
    if (!ctx || !out) return -2;
    NeighborsSphInfo i;
    neighbors_info_spherical(ctx->nbr, &i);
    out->n = i.n;
    out->nvalid = i.nvalid;
    out->bands = i.bands;
    out->cells = i.cells;
    out->total = i.total;
    out->band_height = i.band_height;
    out->periodic = i.periodic;
    out->doublings = i.doublings;
    return 0;
}

int32_t pk_neighbors_release(pk_ctx* ctx) {
    if (!ctx) return -2;
    if (!ctx->nbr) return 0;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    neighbors_release(ctx->nbr);
    return 0;
}

// ---- built-in interaction kernels on the device-resident columns (pk_interact.hip) ------------------------
static int32_t interact_ready(pk_ctx* ctx, const char* who, bool host_order) {
    if (!ctx->bound) return ctx->fail(std::string(who) + ": no particles bound");
    if (ctx->in_flight) return ctx->fail(std::string(who) + ": a launch is in flight (call pk_execute_end)");
    if (host_order && ctx->has_perm) return ctx->fail(std::string(who) + ": the device rows are cell-sorted (pk_interact_host_order first)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->nbr) ctx->nbr = neighbors_create();
    if (!ctx->inter) ctx->inter = interact_create();
    ctx->rerun_valid = false;  // the columns change in place
    ctx->chk_valid = false;
    return 0;
}
static InteractColumns interact_columns(const pk_ctx* ctx) {
    const DParticles& d = ctx->dev;
    InteractColumns c;
    c.n = d.n;
    c.f32 = d.spatial_f32;
    c.t = d.t;
    c.x = d.x; c.y = d.y; c.z = d.z;
    c.dx = d.dx; c.dy = d.dy; c.dz = d.dz;
    c.dt = d.dt;
    c.state = d.state;
    c.mask = d.iter;
    return c;
}

int32_t pk_interact_host_order(pk_ctx* ctx) {
    if (!ctx) return -2;
    int32_t rc = interact_ready(ctx, "pk_interact_host_order", false);
    if (rc) return rc;
    const int64_t n = ctx->dev.n;
    if (!ctx->has_perm) return 0;
    if (n > 0) {
        rc = ensure_alt(ctx);
        if (rc) return rc;
        for (const ColRef& c : particle_columns(ctx)) {  // host row perm[i] <- device row i, as pk_particles_d2h does on its way out
            if (!c.d || !c.a) continue;
            scatter_rows(ctx, c, c.a, n);
        }
        PK_HIP(ctx, hipGetLastError());
        PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
        swap_column_sets(ctx);
    }
    ctx->has_perm = false;
    return 0;
}

int32_t pk_interact_sources(pk_ctx* ctx, const uint8_t* sources) {
    if (!ctx) return -2;
    int32_t rc = interact_ready(ctx, "pk_interact_sources", false);
    if (rc) return rc;
    std::string msg;
    if (neighbors_set_sources(ctx->nbr, ctx->compute, ctx->dev.n, sources, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_interact_prologue(pk_ctx* ctx, double endtime, double dt0, int32_t reset_state, int32_t clip, int64_t* n_evaluated, int64_t* n_active) {
    if (!ctx || !n_evaluated || !n_active) return -2;
    int32_t rc = interact_ready(ctx, "pk_interact_prologue", true);
    if (rc) return rc;
    std::string msg;
    if (interact_prologue(ctx->inter, ctx->compute, interact_columns(ctx), endtime, dt0, reset_state, clip, n_evaluated, n_active, &msg))
        return ctx->fail(msg);
    return 0;
}

int32_t pk_interact_epilogue(pk_ctx* ctx, double endtime, double dt0, int64_t* steps, int64_t* state_counts, int64_t* next_evaluated,
                             int64_t* next_active) {
    if (!ctx || !steps || !state_counts || !next_evaluated || !next_active) return -2;
    int32_t rc = interact_ready(ctx, "pk_interact_epilogue", true);
    if (rc) return rc;
    std::string msg;
    if (interact_epilogue(ctx->inter, ctx->compute, interact_columns(ctx), endtime, dt0, steps, state_counts, next_evaluated, next_active, &msg))
        return ctx->fail(msg);
    return 0;
}

int32_t pk_interact_attract(pk_ctx* ctx, double radius, double velocity, double sphere_radius_m, int32_t use_z, int32_t use_sources, int64_t max_pairs,
                            int64_t* total, double* phase_ms) {
    if (!ctx || !total) return -2;
    int32_t rc = interact_ready(ctx, "pk_interact_attract", true);
    if (rc) return rc;
    if (!(velocity == velocity) || std::isinf(velocity)) return ctx->fail("pk_interact_attract: velocity must be finite");
    if (max_pairs < 0) return ctx->fail("pk_interact_attract: max_pairs must not be negative");
    std::string msg;
    if (interact_attract(ctx->nbr, ctx->compute, interact_columns(ctx), radius, velocity, sphere_radius_m, use_z, use_sources, max_pairs, total, phase_ms,
                         &msg))
        return ctx->fail(msg);
    return 0;
}

int32_t pk_interact_merge(pk_ctx* ctx, double radius, double sphere_radius_m, int32_t use_z, int32_t mass_extra, double* phase_ms) {
    if (!ctx) return -2;
    int32_t rc = interact_ready(ctx, "pk_interact_merge", true);
    if (rc) return rc;
    if (mass_extra < 0 || mass_extra >= PK_MAX_EXTRA || !ctx->dev.extra[mass_extra])
        return ctx->fail("pk_interact_merge: mass_extra must name a device Variable of the bound particles (pk_particles_desc.extra)");
    std::string msg;
    if (interact_merge(ctx->nbr, ctx->compute, interact_columns(ctx), ctx->dev.extra[mass_extra], ctx->dev.extra_f32[mass_extra], radius, sphere_radius_m,
                       use_z, phase_ms, &msg))
        return ctx->fail(msg);
    return 0;
}

// ---- particles per grid cell on the device-resident columns (pk_density.hip) ------------------------------
int32_t pk_particles_density(pk_ctx* ctx, int32_t grid_id, int32_t levels, int32_t weight_kind, int32_t weight_extra, int32_t weight_dtype,
                             const double* weights_host, int64_t ncells, void* out, int64_t* n_outside, pk_density_info_t* info) {
    if (!ctx || !out || !n_outside) return -2;
    if (!ctx->bound) return ctx->fail("pk_particles_density: no particles bound");
    if (ctx->in_flight) return ctx->fail("pk_particles_density: a launch is in flight (call pk_execute_end)");
    if (grid_id < 0 || grid_id >= (int)ctx->grids.size()) return ctx->fail("pk_particles_density: unknown grid id");
    if (ncells <= 0) return ctx->fail("pk_particles_density: ncells must be positive");
    DensityWeights w;
    w.kind = weight_kind;
    w.dtype = weight_dtype;
    if (weight_kind == PK_DENSITY_W_EXTRA) {
        if (weight_extra < 0 || weight_extra >= PK_MAX_EXTRA || !ctx->dev.extra[weight_extra])
            return ctx->fail("pk_particles_density: weight_extra must name a device Variable of the bound particles (pk_particles_desc.extra)");
        if (weight_dtype < PK_DENSITY_F32 || weight_dtype > PK_DENSITY_I64)
            return ctx->fail("pk_particles_density: weight_dtype must be PK_DENSITY_F32, _F64, _I32 or _I64");
        const bool four = weight_dtype == PK_DENSITY_F32 || weight_dtype == PK_DENSITY_I32;
        if (four != (ctx->dev.extra_f32[weight_extra] != 0))
            return ctx->fail("pk_particles_density: weight_dtype does not have the element size of the device Variable");
        w.dev = ctx->dev.extra[weight_extra];
    } else if (weight_kind == PK_DENSITY_W_HOST) {
        if (!weights_host && ctx->dev.n > 0) return ctx->fail("pk_particles_density: PK_DENSITY_W_HOST needs weights_host");
        w.host = weights_host;
    } else if (weight_kind != PK_DENSITY_W_NONE) {
        return ctx->fail("pk_particles_density: weight_kind must be PK_DENSITY_W_NONE, _EXTRA or _HOST");
    }
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const DParticles& d = ctx->dev;  // the column set that is current (a launch leaves what it wrote there)
    DensityColumns c;
    c.n = d.n;
    c.f32 = d.spatial_f32;
    c.x = d.x; c.y = d.y; c.z = d.z;
    c.perm = ctx->has_perm ? ctx->d_perm : nullptr;
    std::string msg;
    if (density_run(ctx->compute, ctx->grids[grid_id].d, c, levels, w, ncells, out, n_outside, info, &msg)) return ctx->fail(msg);
    return 0;
}

// ---- labels of the bound rows and origin-to-destination counts (pk_connectivity.hip) ------------------------
static int32_t conn_ready(pk_ctx* ctx, const char* who, int32_t grid_id, int32_t regions_dtype, const void* regions_host, int64_t ncells) {
    const std::string w(who);
    if (!ctx->bound) return ctx->fail(w + ": no particles bound");
    if (ctx->in_flight) return ctx->fail(w + ": a launch is in flight (call pk_execute_end)");
    if (grid_id < 0 || grid_id >= (int)ctx->grids.size()) return ctx->fail(w + ": unknown grid id");
    if (ncells <= 0) return ctx->fail(w + ": ncells must be positive");
    if (regions_host && regions_dtype != PK_DENSITY_I32 && regions_dtype != PK_DENSITY_I64)
        return ctx->fail(w + ": regions_dtype must be PK_DENSITY_I32 or PK_DENSITY_I64");
    return 0;
}

static DensityColumns conn_columns(pk_ctx* ctx) {
    const DParticles& d = ctx->dev;  // the column set that is current (a launch leaves what it wrote there)
    DensityColumns c;
    c.n = d.n;
    c.f32 = d.spatial_f32;
    c.x = d.x; c.y = d.y; c.z = d.z;
    c.perm = ctx->has_perm ? ctx->d_perm : nullptr;
    return c;
}

int32_t pk_particles_cells(pk_ctx* ctx, int32_t grid_id, int32_t levels, int32_t regions_dtype, const void* regions_host, int64_t ncells,
                           int64_t* labels_out) {
    if (!ctx) return -2;
    if (int32_t rc = conn_ready(ctx, "pk_particles_cells", grid_id, regions_dtype, regions_host, ncells)) return rc;
    if (!labels_out && ctx->dev.n > 0) return ctx->fail("pk_particles_cells: labels_out is NULL");
    ConnLabels l;
    l.regions = regions_host;
    l.regions_dtype = regions_dtype;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    std::string msg;
    if (cells_run(ctx->compute, ctx->grids[grid_id].d, conn_columns(ctx), levels, l, ncells, labels_out, &msg)) return ctx->fail(msg);
    return 0;
}

int32_t pk_particles_connectivity(pk_ctx* ctx, int32_t grid_id, int32_t levels, int32_t regions_dtype, const void* regions_host, int64_t ncells,
                                  int32_t origin_kind, int32_t origin_extra, int32_t origin_dtype, const void* origin_host, int64_t n_origin,
                                  int64_t n_dest, int32_t path, int64_t* dense_out, int64_t* keys_out, int64_t* counts_out, int64_t max_pairs,
                                  pk_connectivity_info_t* info) {
    if (!ctx || !info) return -2;
    if (int32_t rc = conn_ready(ctx, "pk_particles_connectivity", grid_id, regions_dtype, regions_host, ncells)) return rc;
    if (origin_dtype != PK_DENSITY_I32 && origin_dtype != PK_DENSITY_I64)
        return ctx->fail("pk_particles_connectivity: origin_dtype must be PK_DENSITY_I32 or PK_DENSITY_I64");
    ConnLabels l;
    l.regions = regions_host;
    l.regions_dtype = regions_dtype;
    l.origin_dtype = origin_dtype;
    l.n_origin = n_origin;
    l.n_dest = n_dest;
    if (origin_kind == PK_DENSITY_W_EXTRA) {
        if (origin_extra < 0 || origin_extra >= PK_MAX_EXTRA || !ctx->dev.extra[origin_extra])
            return ctx->fail("pk_particles_connectivity: origin_extra must name a device Variable of the bound particles (pk_particles_desc.extra)");
        if ((origin_dtype == PK_DENSITY_I32) != (ctx->dev.extra_f32[origin_extra] != 0))
            return ctx->fail("pk_particles_connectivity: origin_dtype does not have the element size of the device Variable");
        l.origin_dev = ctx->dev.extra[origin_extra];
    } else if (origin_kind == PK_DENSITY_W_HOST) {
        if (!origin_host && ctx->dev.n > 0) return ctx->fail("pk_particles_connectivity: PK_DENSITY_W_HOST needs origin_host");
        l.origin_host = origin_host;
    } else {
        return ctx->fail("pk_particles_connectivity: origin_kind must be PK_DENSITY_W_EXTRA or PK_DENSITY_W_HOST");
    }
    if (path == PK_CONN_SPARSE) {
        if (max_pairs < 0 || (max_pairs > 0 && (!keys_out || !counts_out))) return ctx->fail("pk_particles_connectivity: PK_CONN_SPARSE needs keys_out and counts_out with room for max_pairs");
    } else if (path == PK_CONN_LDS || path == PK_CONN_GLOBAL) {
        if (!dense_out && n_origin > 0) return ctx->fail("pk_particles_connectivity: PK_CONN_LDS / PK_CONN_GLOBAL need dense_out");
    } else {
        return ctx->fail("pk_particles_connectivity: path must be PK_CONN_LDS, PK_CONN_GLOBAL or PK_CONN_SPARSE");
    }
    PK_HIP(ctx, hipSetDevice(ctx->device));
    std::string msg;
    if (connectivity_run(ctx->compute, ctx->grids[grid_id].d, conn_columns(ctx), levels, l, ncells, path, dense_out, keys_out, counts_out, max_pairs, info,
                         &msg))
        return ctx->fail(msg);
    return 0;
}

}  // extern "C"
