"""Curvilinear mesh families for the search-layer tests (tests/test_curv_search_host.py, tests/test_gpu_curv_search.py).

Pure NumPy.  Every mesh is a legal input that the reference accepts; each family is about one thing the smooth regional patch of
oracle/cases.py::curvilinear_grid does not have: the antimeridian, a pole row, an east-west halo (stored exactly or as lon + 360), a
mesh that covers a band twice without repeating a node, masked nodes, cells so coarse that the hash box does not cover the curved
cell, and meshes one cell wide.  Shapes are (ny, nx) nodes.
"""

from __future__ import annotations

import numpy as np

from oracle import cases

# name -> shape (ny, nx), mesh kinds, `band`: (lon_lo, lon_hi, lat_lo, lat_hi) of the region the family is about (a quarter of the
# particles of a trajectory case is released there, or in `release` where that is given; None: the whole mesh), vel / vel_flat / dt /
# nsteps: velocity scale (m/s) and time step (s) of the trajectory case -- chosen so that a particle changes cell every few steps
# on that family's cell size -- and its number of steps (30 where not given)
FAMILIES = {
    "warped": dict(shape=(28, 40), meshes=("spherical", "flat"), band=None, vel=6.0, vel_flat=0.3, dt=3600.0),
    "fine_patch": dict(shape=(28, 40), meshes=("spherical",), band=None, vel=1.5, dt=3600.0),
    "antimeridian_continuous": dict(shape=(28, 40), meshes=("spherical",), band=(176.0, 184.0, -25.0, 20.0), vel=6.0, dt=3600.0),
    "antimeridian_wrapped": dict(shape=(28, 40), meshes=("spherical",), band=(176.0, 184.0, -25.0, 20.0), vel=6.0, dt=3600.0),
    "halo_exact": dict(shape=(26, 50), meshes=("spherical",), band=(-180.0, -165.5, -55.0, 55.0), vel=8.0, dt=7200.0),
    "halo_plus360": dict(shape=(26, 50), meshes=("spherical",), band=(-180.0, -165.5, -55.0, 55.0), vel=8.0, dt=7200.0),
    # (band: the doubly covered longitudes; release: from column 49 west of it, which only that column covers, into the band)
    "self_overlap": dict(shape=(24, 52), meshes=("spherical",), band=(175.0, 187.3, -58.0, 58.0), release=(172.7, 181.0, -50.0, 50.0), vel=16.0,
                         dt=7200.0, nsteps=36),
    "pole_row": dict(shape=(20, 36), meshes=("spherical",), band=(-70.0, 70.0, 84.0, 89.5), vel=6.0, dt=3600.0),
    "masked": dict(shape=(28, 40), meshes=("spherical", "flat"), band="mask", vel=6.0, vel_flat=0.3, dt=3600.0),
    "coarse_global": dict(shape=(8, 12), meshes=("spherical",), band=None, vel=10.0, dt=4 * 3600.0),
    # (one cell wide: slow across so that no particle leaves -- see trajectory_case -- and, on two_columns, fast along: a row every few steps)
    "one_cell": dict(shape=(2, 2), meshes=("spherical",), band=None, vel=0.3, dt=3600.0),
    "two_columns": dict(shape=(30, 2), meshes=("spherical", "flat"), band=None, vel=0.02, vel_v=0.7, vel_flat=0.01, vel_v_flat=0.3, dt=3600.0),
}
MASK_ROWS, MASK_COLS = slice(12, 16), slice(18, 23)  # the 4 x 5 NaN block of `masked`

FAMILY_MESHES = [(n, m) for n, f in FAMILIES.items() for m in f["meshes"]]


def _unit(n):
    return np.arange(n, dtype=np.float64) / (n - 1)


def halo_exact_mesh():
    """A global, zonally cyclic mesh whose last two node columns repeat the first two (an ORCA-style east-west halo): cells
    (j, nx-2) and (j, 0) coincide, so a point there lies in two cells and the table order decides."""
    nxb, ny = 48, 26
    i = np.arange(nxb)[None, :] / nxb
    j = np.arange(ny)[:, None] / (ny - 1)
    lon = 360.0 * i + 3.0 * np.sin(2 * np.pi * i) * np.sin(np.pi * j) - 180.0
    lat = -66.0 + 132.0 * j + 2.5 * np.cos(2 * np.pi * i) * np.sin(np.pi * j)
    return lon, lat


def halo(a):
    """Append the first two columns of the last axis (what the halo of `halo_exact` does to the nodes and to the fields)."""
    return np.ascontiguousarray(np.concatenate([a, a[..., :2]], axis=-1))


def family(name, mesh="spherical"):
    """(lon, lat) of the family, float64, C-contiguous, shape FAMILIES[name]["shape"]."""
    fam = FAMILIES[name]
    if mesh not in fam["meshes"]:
        raise ValueError(f"family {name} has no {mesh} mesh")
    ny, nx = fam["shape"]
    i, j = _unit(nx)[None, :], _unit(ny)[:, None]
    if name in ("warped", "masked"):
        lon, lat = cases.curvilinear_grid(nx, ny, mesh=mesh)
        if name == "masked":
            lon, lat = lon.copy(), lat.copy()
            lon[MASK_ROWS, MASK_COLS] = np.nan
            lat[MASK_ROWS, MASK_COLS] = np.nan
    elif name == "fine_patch":
        lon = 10.0 + 6.0 * i + 0.3 * np.sin(2 * np.pi * j) * (0.3 + i) + 0.4 * j
        lat = 30.0 + 4.0 * j + 0.2 * np.sin(2 * np.pi * i) * (0.5 + 0.5 * j) - 0.3 * i
    elif name in ("antimeridian_continuous", "antimeridian_wrapped"):
        lon = 150.0 + 65.0 * i + 3.0 * np.sin(2 * np.pi * j) * (0.3 + i) + 0 * j
        lon = 150.0 + (lon - lon.min()) * (65.0 / (lon.max() - lon.min()))  # lon 150 ... 215
        lat = -35.0 + 60.0 * j + 3.0 * np.sin(2 * np.pi * i) * (0.5 + 0.5 * j) - 4.0 * i
        if name == "antimeridian_wrapped":
            lon = np.where(lon > 180.0, lon - 360.0, lon)
    elif name in ("halo_exact", "halo_plus360"):
        lon, lat = halo_exact_mesh()
        lon, lat = halo(lon), halo(lat)
        if name == "halo_plus360":
            lon[:, -2:] += 360.0
    elif name == "self_overlap":
        ii = np.arange(nx, dtype=np.float64)[None, :]
        jj = np.arange(ny, dtype=np.float64)[:, None]
        lon = -185.0 + 7.3 * ii + 0 * jj
        lat = -60.0 + 120.0 * jj / 23.0 + 1.5 * np.sin(2 * np.pi * ii / 51.0)
    elif name == "pole_row":
        lon = -80.0 + 160.0 * i + 4.0 * np.sin(np.pi * j) * (i - 0.5)
        lat = 40.0 + 50.0 * j + 2.0 * np.sin(2 * np.pi * i) * np.sin(np.pi * j)
        lat[-1, :] = 90.0
    elif name == "coarse_global":
        lon = -170.0 + 340.0 * i + 2.0 * np.sin(2 * np.pi * j) * (0.3 + i) + 3.0 * j
        lat = -75.0 + 150.0 * j + 1.5 * np.sin(2 * np.pi * i) * (0.5 + 0.5 * j) - 2.0 * i
        lon = -170.0 + (lon - lon.min()) * (340.0 / (lon.max() - lon.min()))
        lat = -75.0 + (lat - lat.min()) * (150.0 / (lat.max() - lat.min()))
    elif name == "one_cell":
        lon = np.array([[0.0, 2.0], [0.3, 2.4]])
        lat = np.array([[10.0, 10.2], [12.0, 12.5]])
    elif name == "two_columns":
        if mesh == "spherical":
            # (narrow: every search on this mesh is the unguessed hash query, and a face is listed only in the hash cells its xyz
            # corner box overlaps -- the bulge of a wide, flat cell beyond that box is in no cell for the reference)
            lon = -20.0 + 0.3 * i + 0.03 * np.sin(np.pi * j)
            lat = 5.0 + 4.0 * j + 0.01 * i
        else:
            # (rows that widen northwards: a flat cell in metres that is a parallelogram to rounding loses some of its own points to
            # the cancelling bilinear inverse of index_search.py:122-177, and a lost particle raises in the reference on this mesh)
            lon = 1.0e4 * i * (1.0 + 0.5 * j) + 6.0e3 * np.sin(np.pi * j)
            lat = 1.0e5 * j + 2.0e3 * i
    else:
        raise KeyError(name)
    lon = np.ascontiguousarray(np.broadcast_to(lon, (ny, nx)), dtype=np.float64)
    lat = np.ascontiguousarray(np.broadcast_to(lat, (ny, nx)), dtype=np.float64)
    return lon, lat


def coordinate_scale(lon, lat):
    return float(max(np.nanmax(np.abs(lon)), np.nanmax(np.abs(lat))))


def _clip_lat(y, spherical):
    # no query exactly at a pole: the longitude of such a point is arbitrary and its cell a matter of rounding
    return np.clip(y, -89.99, 89.99) if spherical else y


def _rel(a, a0, spherical):
    """a as the longitude nearest to a0 (spherical meshes store longitudes modulo 360: wrapped meshes, lon + 360 halos)."""
    return a0 + (np.mod(a - a0 + 180.0, 360.0) - 180.0) if spherical else a


def bilinear_points(lon, lat, fi, fj, j0, i0, spherical=True):
    """Bilinear blend of the corners of cells (j0, i0) at the cell coordinates (fi, fj); corner longitudes relative to the first."""
    w = ((1 - fi) * (1 - fj), fi * (1 - fj), (1 - fi) * fj, fi * fj)
    idx = ((j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1))
    x = sum(wk * _rel(lon[k], lon[idx[0]], spherical) for wk, k in zip(w, idx))
    y = sum(wk * lat[k] for wk, k in zip(w, idx))
    return x, y


def query_points(lon, lat, n, seed, mesh="spherical"):
    """Query set of a mesh: a dict of (x, y) pairs by kind.

      random    n points over the bounding box plus 3 degrees (flat: 4 % of the extent) on each side
      interior  25 bilinear interior points per cell with four finite corners
      nodes     every finite node
      edges     every midpoint of an edge between two finite nodes
      far       points 30 degrees (flat: 40 % of the extent) away from the box
      nonfinite nan and inf in either coordinate

    `random` and `interior` are the ones a stable-point comparison with the oracle uses; nodes and edge midpoints lie on cell
    boundaries by construction and serve the A/B comparisons only."""
    spherical = mesh == "spherical"
    rng = np.random.default_rng(seed)
    fin = np.isfinite(lon) & np.isfinite(lat)
    # the box of the longitudes as stored or relative to the first node, whichever is narrower (a wrapped mesh is stored in two pieces)
    lons = [lon[fin]] + ([_rel(lon[fin], lon[fin][0], True)] if spherical else [])
    lonb = min(lons, key=lambda a: a.max() - a.min())
    x0, x1, y0, y1 = lonb.min(), lonb.max(), np.nanmin(lat), np.nanmax(lat)
    padx, pady = (3.0, 3.0) if spherical else (0.04 * (x1 - x0), 0.04 * (y1 - y0))
    farx, fary = (30.0, 30.0) if spherical else (0.4 * (x1 - x0), 0.4 * (y1 - y0))
    out = {}
    out["random"] = (rng.uniform(x0 - padx, x1 + padx, n), _clip_lat(rng.uniform(y0 - pady, y1 + pady, n), spherical))
    ny, nx = lon.shape
    jj, ii = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    ok = fin[:-1, :-1] & fin[:-1, 1:] & fin[1:, :-1] & fin[1:, 1:]
    j0, i0 = np.repeat(jj[ok], 25), np.repeat(ii[ok], 25)
    fi, fj = rng.uniform(0.02, 0.98, j0.size), rng.uniform(0.02, 0.98, j0.size)
    bx, by = bilinear_points(lon, lat, fi, fj, j0, i0, spherical)
    out["interior"] = (bx, _clip_lat(by, spherical))
    out["nodes"] = (lon[fin], _clip_lat(lat[fin], spherical))
    ex, ey = [], []
    for a, b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        m = fin[a] & fin[b]
        ex.append(0.5 * (lon[a][m] + _rel(lon[b][m], lon[a][m], spherical)))
        ey.append(0.5 * (lat[a][m] + lat[b][m]))
    out["edges"] = (np.concatenate(ex), _clip_lat(np.concatenate(ey), spherical))
    cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    far = []  # (on the sphere: only where such a point exists -- not east or west of a global mesh, not beyond a pole)
    if not spherical or (x1 - x0) + 2 * farx <= 330.0:
        far += [(x0 - farx, cy), (x1 + farx, cy)]
    if not spherical or y0 - fary >= -89.99:
        far.append((cx, y0 - fary))
    if not spherical or y1 + fary <= 89.99:
        far.append((cx, y1 + fary))
    out["far"] = (np.array([p[0] for p in far]), np.array([p[1] for p in far]))
    out["nonfinite"] = (np.array([np.nan, cx, np.inf, cx, -np.inf, np.nan]), np.array([cy, np.nan, cy, np.inf, cy, np.nan]))
    for k, (x, y) in out.items():
        assert x.shape == y.shape, k
        if spherical:
            assert not np.any(np.abs(y[np.isfinite(y)]) == 90.0), k
    return out


def flatten_queries(q):
    """All kinds back to back: (x, y, {kind: slice})."""
    xs, ys, sl, o = [], [], {}, 0
    for k, (x, y) in q.items():
        xs.append(x)
        ys.append(y)
        sl[k] = slice(o, o + x.size)
        o += x.size
    return np.ascontiguousarray(np.concatenate(xs)), np.ascontiguousarray(np.concatenate(ys)), sl


# ---- the lattice rule of csrc/pk_hashbuild.h (mesh_has_coincident_nodes), restated on the host -----------------------------------
def lattice_coincident(lon, lat, mesh="spherical"):
    """Do two finite nodes fall into one cell of the 2^-20 lattice of the unit sphere (flat: 2^-30 of the bounding box), in the
    lattice itself or in the one offset by half a cell?"""
    fin = np.isfinite(lon) & np.isfinite(lat)
    if mesh == "spherical":
        lonr, latr = np.deg2rad(lon[fin]), np.deg2rad(lat[fin])
        c = np.stack((np.cos(lonr) * np.cos(latr), np.sin(lonr) * np.cos(latr), np.sin(latr)), axis=1)
        scaled = (c + 1.0) * 1048576.0
    else:
        x, y = lon[fin], lat[fin]
        dx, dy = x.max() - x.min(), y.max() - y.min()
        scaled = np.stack(((x - x.min()) / dx if dx else 0 * x, (y - y.min()) / dy if dy else 0 * y), axis=1) * 1073741824.0
    for offset in (0.0, 0.5):
        q = (scaled + offset).astype(np.uint64)
        if len(np.unique(q, axis=0)) < len(q):
            return True
    return False


COINCIDENT = {"halo_exact", "halo_plus360", "pole_row"}  # by the lattice rule; every other family is not


# ---- the oracle's unguessed search and the stability of its answer -----------------------------------------------------------
def mesh_case(name, mesh="spherical"):
    """The minimal case dict the oracle's search needs (no fields)."""
    from case_utils import attach_hash_table

    lon, lat = family(name, mesh)
    case = dict(name=name, mesh=mesh, lon=lon, lat=lat, depth=None, fields={}, field_dims={})
    return attach_hash_table(case)


def oracle_search(case, x, y):
    """po_hash_query at the points: (yi, xi) int32, GRID_SEARCH_ERROR where no listed face holds the point."""
    import ctypes as C

    from oracle import c_oracle as co

    mc = case.get("_marshalled")
    if mc is None:
        mc = case["_marshalled"] = co.MarshalledCase(case)
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = x.shape[0]
    yi, xi = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xs, et = np.zeros(n), np.zeros(n)
    if n:
        co.lib().po_hash_query(C.byref(mc.grids[0]), C.c_int64(n), co._ptr(y), co._ptr(x), co._ptr(yi), co._ptr(xi), co._ptr(xs), co._ptr(et))
    return yi, xi


def stable_mask(case, x, y):
    """Stable points: the oracle gives the same (yi, xi) at the point and at its four neighbours shifted by 1e-9 * (coordinate
    scale) in x and in y.  A property of the oracle alone."""
    h = 1e-9 * coordinate_scale(case["lon"], case["lat"])
    yi, xi = oracle_search(case, x, y)
    ok = np.isfinite(x) & np.isfinite(y)
    for dx, dy in ((h, 0.0), (-h, 0.0), (0.0, h), (0.0, -h)):
        y2, x2 = oracle_search(case, x + dx, y + dy)
        ok &= (y2 == yi) & (x2 == xi)
    return ok, yi, xi


# ---- trajectory cases --------------------------------------------------------------------------------------------------------
def in_band(name, x, y):
    """Is (x, y) inside the band the family is about?  (longitudes modulo 360 on the spherical families)"""
    band = FAMILIES[name]["band"]
    if band is None:
        return np.ones(np.shape(x), bool)
    if band == "mask":
        raise ValueError("the band of `masked` is a set of cells: use trajectory_case(...)['band_release']")
    lo, hi, ylo, yhi = band
    return (np.mod(np.asarray(x) - lo, 360.0) <= hi - lo) & (np.asarray(y) >= ylo) & (np.asarray(y) <= yhi)


def trajectory_case(name, mesh="spherical", *, npart=2000, seed=0, nsteps=None, cgrid=False, kernels=None):
    """A-grid AdvectionRK4 + DeleteParticle on U, V from cases.smooth_random_field (nz = 3, nt = 3), populate_indices() first; a
    quarter of the particles is released inside the family's band.  cgrid: C-grid U, V, W and AdvectionRK4_3D instead (the leg that
    runs the dedicated kernels)."""
    fam = FAMILIES[name]
    lon, lat = family(name, mesh)
    ny, nx = lon.shape
    rng = np.random.default_rng(1000 + seed)
    nz, nt = 3, 3
    vel = fam["vel"] if mesh == "spherical" else fam["vel_flat"]
    vel_v = fam.get("vel_v" if mesh == "spherical" else "vel_v_flat", 0.6 * vel)
    nsteps = nsteps or fam.get("nsteps", 30)
    shp = (nt, nz, ny, nx)
    if name in ("halo_exact", "halo_plus360"):  # the halo columns carry the data of the columns they repeat
        shp = (nt, nz, ny, nx - 2)
        U, V = halo(cases.smooth_random_field(rng, shp, vel)), halo(cases.smooth_random_field(rng, shp, vel_v))
    else:
        U, V = cases.smooth_random_field(rng, shp, vel), cases.smooth_random_field(rng, shp, vel_v)
    fields = {"U": U, "V": V}
    if cgrid:
        dims = {"U": ("time", "ZC", "YC", "XG"), "V": ("time", "ZC", "YG", "XC"), "W": ("time", "depth", "YC", "XC")}
        fields = {"U": U.astype(np.float32), "V": V.astype(np.float32), "W": cases.smooth_random_field(rng, shp, 0.0005 * vel, np.float32)}
    else:
        dims = {"U": cases.TZYX_NODE, "V": cases.TZYX_NODE}
    # release: bilinear points of cells with finite corners, away from the rim
    fin = np.isfinite(lon) & np.isfinite(lat)
    ok = fin[:-1, :-1] & fin[:-1, 1:] & fin[1:, :-1] & fin[1:, 1:]
    jj, ii = np.nonzero(ok)
    lo_f, hi_f = 0.02, 0.98
    if nx > 6 and ny > 6:
        keep = (jj >= 2) & (jj < ny - 3) & (ii >= 2) & (ii < nx - 3) if name != "pole_row" else (jj >= 2) & (ii >= 2) & (ii < nx - 3)
        if name in ("halo_exact", "halo_plus360", "self_overlap"):
            keep = (jj >= 2) & (jj < ny - 3)
        jj, ii = jj[keep], ii[keep]
    elif nx == 2:
        # A mesh one cell wide: the reference indexes the node axes with the failed search's xi = -3, which wraps around silently on a
        # wider mesh and raises IndexError on a 2-node axis.  No particle may leave such a mesh: released in the middle, slow across.
        lo_f, hi_f = 0.25, 0.75
        if ny > 20:
            keep = (jj >= 8) & (jj < ny - 9)
            jj, ii = jj[keep], ii[keep]
    spherical = mesh == "spherical"
    pick = rng.integers(0, jj.size, npart)
    fi, fj = rng.uniform(lo_f, hi_f, npart), rng.uniform(lo_f, hi_f, npart)
    x, y = bilinear_points(lon, lat, fi, fj, jj[pick], ii[pick], spherical)
    nb = npart // 4
    band = fam.get("release", fam["band"])
    band_release = np.zeros(npart, bool)
    if band == "mask":  # around the NaN block: the ring of cells next to the cells that touch it
        ring = np.zeros_like(ok)
        ring[MASK_ROWS.start - 3:MASK_ROWS.stop + 2, MASK_COLS.start - 3:MASK_COLS.stop + 2] = True
        rj, ri = np.nonzero(ring & ok)
        pk = rng.integers(0, rj.size, nb)
        x[:nb], y[:nb] = bilinear_points(lon, lat, rng.uniform(0.02, 0.98, nb), rng.uniform(0.02, 0.98, nb), rj[pk], ri[pk], spherical)
        band_release[:nb] = True
    elif band is not None:
        lo, hi, ylo, yhi = band
        x[:nb] = rng.uniform(lo, hi, nb)
        y[:nb] = rng.uniform(ylo, yhi, nb)
        band_release[:nb] = True
    y = _clip_lat(y, spherical)
    dt = fam["dt"]
    kernels = list(kernels) if kernels is not None else (["AdvectionRK4_3D", "DeleteParticle"] if cgrid else ["AdvectionRK4", "DeleteParticle"])
    return dict(
        name=f"{name}_{mesh}" + ("_cgrid" if cgrid else ""), mesh=mesh, lon=lon, lat=lat, depth=np.linspace(0, 1000, nz), x_pad="low", y_pad="low",
        z_pad="high" if cgrid else "both", time_s=np.arange(nt) * (0.55 * nsteps * dt), fields=fields, field_dims=dims, cgrid=cgrid, kernels=kernels,
        spatial_dtype="float64", x=x, y=y, z=rng.uniform(50, 900, npart), t0=None, dt=dt, runtime=nsteps * dt, seed=seed, populate=True,
        band_release=band_release,
    )
