"""Fixtures of ParticleSet.density: tests/golden/density/dens_*.npz.

The reference has no density method (Parcels dropped it with v4), so a fixture's expected map is put together from what the reference does
have: the cell of every particle is what its own ``grid.search(z, y, x)`` answers with no guess (what ParticleSet.populate_indices stores,
particleset.py:252-262) and the map is ``np.bincount`` over those cells.  A fixture holds data only: the mesh, the positions in their storage
dtype, float64 weights, per particle the expected cell (or -1), and the expected counts, weighted sums and outside counts, each without and
with ``levels``.

A case is only written when every particle can be compared (``generate`` raises otherwise):

* on curvilinear and unstructured meshes an inside point is built from bilinear / barycentric weights in [0.05, 0.95] of a chosen cell and the
  reference must answer exactly that cell (a point near an edge would turn the 1e-12-class difference between device and NumPy arithmetic,
  and the float32 trigonometry of the spherical UxGrid search, into another cell), and an outside point lies at least one cell width
  beyond the hull and must be answered with an error code;
* on rectilinear grids points exactly ON nodes are part of the cases -- comparisons there are exact on both sides -- so the reference's
  right-closed rule (x = node k lies in cell k - 1, the first node in cell 0) is in the fixture;
* non-finite positions are in no fixture: their rule is a deliberate difference from the reference and is tested on its own.

Usage: python tools/make_density_golden.py [case ...]
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "density")

from tools import make_ux_golden as mg  # noqa: E402


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def _irregular(lo, n, seed, step=1.0):
    """n strictly increasing nodes from `lo` with irregular widths (multiples of 1/8: representable in float32)"""
    rng = np.random.default_rng(seed)
    return lo + np.concatenate([[0.0], np.cumsum(step * rng.integers(4, 13, n - 1) / 8.0)])


def _rect(nx, ny, nz, mesh, seed):
    lon = _irregular(-3.0 if mesh == "flat" else 10.0, nx, seed) if nx > 1 else np.array([2.5])
    lat = _irregular(1.0 if mesh == "flat" else -4.0, ny, seed + 1)
    depth = _irregular(0.0, nz, seed + 2, step=10.0) if nz else None
    return dict(kind="xgrid", mesh=mesh, lon=lon, lat=lat, depth=depth)


def _curv(nx, ny, mesh):
    """nx x ny sheared nodes: every row is shifted east and the columns lean north"""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    lon = 20.0 + 1.0 * i + 0.3 * j + 0.02 * i * j
    lat = 40.0 + 0.8 * j + 0.15 * i - 0.01 * i * j
    return dict(kind="xgrid", mesh=mesh, lon=lon, lat=lat, depth=None)


def _ux(mesh, zf):
    if mesh == "flat":
        lon, lat, faces = mg.lattice_mesh(11, 11, 0.0, 20.0, 0.0, 20.0, jitter=0.25, seed=21)
    else:
        lon, lat, faces = mg.lattice_mesh(11, 11, -20.0, 0.0, 35.0, 50.0, jitter=0.25, seed=22)
    return dict(kind="ux", mesh=mesh, node_lon=lon, node_lat=lat, faces=faces, zf=np.asarray(zf, dtype=np.float64))


# ---- particles -----------------------------------------------------------------------------------------------------------------------
def _weights(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 3.0, n)


def _rect_points(g, n, seed):
    """interior points, points exactly on nodes, points outside on each of the four sides; z above, below, on and between the levels"""
    rng = np.random.default_rng(seed)
    lon, lat, depth = g["lon"], g["lat"], g["depth"]
    x = rng.uniform(lon[0], lon[-1], n) if lon.size > 1 else rng.uniform(-50.0, 50.0, n)
    y = rng.uniform(lat[0], lat[-1], n)
    z = rng.uniform(depth[0], depth[-1], n) if depth is not None else np.zeros(n)
    k = 0
    if lon.size > 1:
        for xv in (lon[0], lon[-1], lon[1], lon[lon.size // 2], lon[-2]):  # on nodes of X (y inside)
            x[k] = xv
            k += 1
    for yv in (lat[0], lat[-1], lat[1], lat[lat.size // 2]):  # on nodes of Y
        y[k] = yv
        k += 1
    if lon.size > 1:
        for xv, yv in ((lon[0], lat[0]), (lon[-1], lat[-1]), (lon[2], lat[3]), (lon[0], lat[-1])):  # on a node of both
            x[k], y[k] = xv, yv
            k += 1
        x[k], x[k + 1] = lon[0] - 0.5, lon[-1] + 0.5  # outside west / east
        k += 2
    y[k], y[k + 1] = lat[0] - 0.5, lat[-1] + 0.5  # outside south / north
    k += 2
    if lon.size > 1:
        x[k], y[k] = lon[-1] + 3.0, lat[0] - 3.0  # outside in both
        k += 1
    if depth is not None:
        for zv in (depth[0], depth[-1], depth[1], depth[-2], depth[0] - 1.0, depth[-1] + 1.0, depth[0] - 1e-9, depth[-1] * (1 + 1e-12)):
            z[n - 1 - k] = zv  # (rows from the other end: they meet every horizontal kind above only by chance)
            k += 1
        z[0], z[1] = depth[0] - 5.0, depth[-1] + 5.0  # a node point of X that is also above / below
    assert k < n
    return x, y, z


def _curv_points(g, n_in, n_out, seed):
    rng = np.random.default_rng(seed)
    lon, lat = g["lon"], g["lat"]
    ny, nx = lon.shape
    cj, ci = rng.integers(0, ny - 1, n_in), rng.integers(0, nx - 1, n_in)
    a, b = rng.uniform(0.05, 0.95, n_in), rng.uniform(0.05, 0.95, n_in)

    def bil(f):
        return (1 - a) * (1 - b) * f[cj, ci] + a * (1 - b) * f[cj, ci + 1] + a * b * f[cj + 1, ci + 1] + (1 - a) * b * f[cj + 1, ci]

    x, y = bil(lon), bil(lat)
    want = cj * (nx - 1) + ci
    # outside: beyond the hull by one to three cell widths, on every side
    w = max(np.abs(np.diff(lon, axis=1)).max(), np.abs(np.diff(lat, axis=0)).max())
    ang = np.linspace(0.0, 2 * np.pi, n_out, endpoint=False) + 0.3
    cx, cy = lon.mean(), lat.mean()
    r = 0.5 * np.hypot(np.ptp(lon), np.ptp(lat)) + w * rng.uniform(1.0, 3.0, n_out)
    x = np.concatenate([x, cx + r * np.cos(ang)])
    y = np.concatenate([y, cy + r * np.sin(ang)])
    want = np.concatenate([want, np.full(n_out, -1)])
    perm = rng.permutation(x.size)
    return x[perm], y[perm], np.zeros(x.size), want[perm]


def _ux_points(g, n_in, n_out, seed, zf):
    rng = np.random.default_rng(seed)
    lon, lat, faces = g["node_lon"], g["node_lat"], g["faces"]
    f = rng.integers(0, faces.shape[0], n_in)
    b = rng.uniform(0.05, 0.95, (n_in, 3))
    b = b / b.sum(axis=1, keepdims=True)
    while (b.min(axis=1) < 0.05).any() or (b.max(axis=1) > 0.95).any():  # (normalising moves the weights: draw again where they left the band)
        bad = (b.min(axis=1) < 0.05) | (b.max(axis=1) > 0.95)
        nb = rng.uniform(0.05, 0.95, (int(bad.sum()), 3))
        b[bad] = nb / nb.sum(axis=1, keepdims=True)
    x = (b * lon[faces[f]]).sum(axis=1)
    y = (b * lat[faces[f]]).sum(axis=1)
    want = f.copy()
    w = 2.0 * max(np.ptp(lon), np.ptp(lat)) / 10.0
    side = np.arange(n_out) % 4
    t = rng.uniform(0.1, 0.9, n_out)
    d = w * rng.uniform(1.0, 2.0, n_out)
    ox = np.where(side == 0, lon.min() - d, np.where(side == 1, lon.max() + d, lon.min() + t * np.ptp(lon)))
    oy = np.where(side == 2, lat.min() - d, np.where(side == 3, lat.max() + d, lat.min() + t * np.ptp(lat)))
    x, y, want = np.concatenate([x, ox]), np.concatenate([y, oy]), np.concatenate([want, np.full(n_out, -1)])
    n = x.size
    z = rng.uniform(zf[0], zf[-1], n)
    if zf.size > 2:  # on, above and below the interfaces
        z[:6] = [zf[0], zf[-1], zf[1], zf[0] - 1.0, zf[-1] + 1.0, zf[-2]]
    perm = rng.permutation(n)
    return x[perm], y[perm], z[perm], want[perm]


def _cell_points(g, cells, seed):
    """one point strictly inside each of the given cells (row by row) of a rectilinear grid"""
    rng = np.random.default_rng(seed)
    lon, lat = g["lon"], g["lat"]
    cj, ci = np.divmod(np.asarray(cells), lon.size - 1)
    a, b = rng.uniform(0.1, 0.9, len(cells)), rng.uniform(0.1, 0.9, len(cells))
    return lon[ci] + a * (lon[ci + 1] - lon[ci]), lat[cj] + b * (lat[cj + 1] - lat[cj]), np.zeros(len(cells))


def cases() -> dict:
    out = {}
    rng = np.random.default_rng(77)
    g = _rect(8, 6, 4, "flat", 1)
    x, y, z = _rect_points(g, 257, 2)
    out["dens_rect_flat"] = dict(g, x=x, y=y, z=z, w=_weights(rng, 257), spatial_dtype="float64")
    out["dens_n1"] = dict(g, x=x[40:41], y=y[40:41], z=z[40:41], w=_weights(rng, 1), spatial_dtype="float64")
    out["dens_n0"] = dict(g, x=x[:0], y=y[:0], z=z[:0], w=_weights(rng, 0), spatial_dtype="float64")
    g = _rect(8, 6, 4, "spherical", 3)
    x, y, z = _rect_points(g, 65, 4)
    out["dens_rect_sph_f32"] = dict(g, x=x, y=y, z=z, w=_weights(rng, 65), spatial_dtype="float32")
    g = _rect(1, 6, 0, "flat", 5)
    x, y, z = _rect_points(g, 64, 6)
    out["dens_rect_len1"] = dict(g, x=x, y=y, z=z, w=_weights(rng, 64), spatial_dtype="float64")
    g = _curv(7, 6, "spherical")
    x, y, z, want = _curv_points(g, 65, 8, 7)
    out["dens_curv_sph"] = dict(g, x=x, y=y, z=z, want=want, w=_weights(rng, 73), spatial_dtype="float64")
    g = _ux("flat", [0.0, 1.0])
    x, y, z, want = _ux_points(g, 257, 12, 8, g["zf"])
    out["dens_ux_flat"] = dict(g, x=x, y=y, z=z, want=want, w=_weights(rng, 269), spatial_dtype="float64")
    g = _ux("spherical", [0.0, 10.0, 25.0, 50.0])
    x, y, z, want = _ux_points(g, 57, 6, 9, g["zf"])
    out["dens_ux_sph_levels"] = dict(g, x=x, y=y, z=z, want=want, w=_weights(rng, 63), spatial_dtype="float64")
    # every particle in one cell; weights over 30 orders of magnitude with both signs: any order of adding other than ascending row shows
    g = _rect(7, 5, 0, "flat", 10)
    n = 4099
    x, y, z = _cell_points(g, np.full(n, 9), 11)
    w = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15.0, 15.0, n)
    out["dens_one_cell"] = dict(g, x=x, y=y, z=z, w=w, spatial_dtype="float64", order_sensitive=True)
    # runs of equal cells of length 1, 2, 63, 64, 65, 129 row by row (they end inside, on and across 64-lane boundaries), then a tail
    # that alternates between two cells
    ncell = (g["lon"].size - 1) * (g["lat"].size - 1)
    cells, c = [], 0
    while len(cells) < 3600:
        for ln in (1, 2, 63, 64, 65, 129):
            cells += [c % ncell] * ln
            c += 5
    cells = cells[:3600]
    cells += [3 + 7 * (k % 2) for k in range(n - len(cells))]
    x, y, z = _cell_points(g, cells, 12)
    out["dens_runs"] = dict(g, x=x, y=y, z=z, want=np.asarray(cells), w=_weights(rng, n), spatial_dtype="float64")
    return out


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def ref_grid(case):
    if case["kind"] == "ux":
        m, DA = mg.reference()
        return mg.ref_grid(m, DA, case)
    from oracle import ref_shim

    return ref_shim.make_ref_grid(lon=case["lon"], lat=case["lat"], depth=case["depth"], mesh=case["mesh"])


def storage(case, name):
    return np.ascontiguousarray(case[name], dtype=np.dtype(case["spatial_dtype"]))


def map_shape(grid, levels):
    """(Z,) Y, X or (Z,) FACE dims of the grid (get_axis_dim); an axis it does not have, or one of length 1, counts 1"""
    dim = lambda a: max(int(grid.get_axis_dim(a)), 1) if a in grid.axes else 1  # noqa: E731
    lateral = (dim("FACE"),) if "FACE" in grid.axes else (dim("Y"), dim("X"))
    return ((dim("Z"),) if levels else ()) + lateral


def reference_cells(case):
    """per particle the cell the reference's unguessed search answers, or -1: (without levels, with levels, shape, shape with levels)"""
    grid = ref_grid(case)
    x, y, z = storage(case, "x"), storage(case, "y"), storage(case, "z")
    shape, shape_lv = map_shape(grid, False), map_shape(grid, True)
    if x.size == 0:
        e = np.zeros(0, np.int64)
        return e, e, shape, shape_lv
    pos = grid.search(z, y, x)
    zi = np.asarray(pos["Z"]["index"], dtype=np.int64)
    if "FACE" in pos:
        hi = np.asarray(pos["FACE"]["index"], dtype=np.int64)
        bad = hi < 0
        assert np.all(hi[~bad] < shape[-1])
    else:
        yi, xi = np.asarray(pos["Y"]["index"], dtype=np.int64), np.asarray(pos["X"]["index"], dtype=np.int64)
        bad = (yi < 0) | (xi < 0)
        assert np.all(yi[~bad] < shape[0]) and np.all(xi[~bad] < shape[1])
        hi = yi * shape[1] + xi
    cell = np.where(bad, -1, hi)
    bad_lv = bad | (zi < 0)
    assert np.all(zi[~bad_lv] < shape_lv[0])
    cell_lv = np.where(bad_lv, -1, zi * int(np.prod(shape)) + hi)
    return cell, cell_lv, shape, shape_lv


def _bincount(cell, ncells, w=None):
    inside = cell >= 0
    return np.bincount(cell[inside], weights=None if w is None else w[inside], minlength=ncells)


def generate(name, case) -> dict:
    cell, cell_lv, shape, shape_lv = reference_cells(case)
    n = cell.size
    w = np.asarray(case["w"], dtype=np.float64)
    assert w.shape == (n,) and np.isfinite(w).all()
    for k in ("x", "y", "z"):
        assert np.isfinite(case[k]).all(), "non-finite positions are not part of a reference-derived fixture"
    if "want" in case:  # constructed cells: the reference must answer them (module docstring)
        if not np.array_equal(cell, np.asarray(case["want"])):
            raise RuntimeError(f"{name}: the reference answers another cell than the one a point was built in for {np.count_nonzero(cell != case['want'])} points")
    ncells, ncells_lv = int(np.prod(shape)), int(np.prod(shape_lv))
    arrs = {k: np.asarray(case[k]) for k in ("lon", "lat", "depth", "node_lon", "node_lat", "faces", "zf") if case.get(k) is not None}
    arrs.update(x=storage(case, "x"), y=storage(case, "y"), z=storage(case, "z"), w=w, cell=cell, cell_levels=cell_lv,
                counts=_bincount(cell, ncells).astype(np.int64), counts_levels=_bincount(cell_lv, ncells_lv).astype(np.int64),
                sums=_bincount(cell, ncells, w), sums_levels=_bincount(cell_lv, ncells_lv, w),
                n_outside=np.int64(np.count_nonzero(cell < 0)), n_outside_levels=np.int64(np.count_nonzero(cell_lv < 0)))
    if case.get("order_sensitive"):
        c = int(cell[0])
        assert np.all(cell == c)
        fwd = arrs["sums"][c]
        rev = _bincount(cell[::-1], ncells, w[::-1])[c]
        if fwd == rev or fwd == float(np.sum(w)):  # (np.sum adds pairwise)
            raise RuntimeError(f"{name}: the weights do not tell the order of adding apart")
    meta = dict(kind=case["kind"], mesh=case["mesh"], spatial_dtype=case["spatial_dtype"], shape=list(shape), shape_levels=list(shape_lv))
    arrs["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrs


def load(path) -> dict:
    with np.load(path, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    out.update(json.loads(out.pop("meta").tobytes().decode()))
    for k in ("depth",):
        out.setdefault(k, None)
    return out


def main(names=None):
    os.makedirs(GOLDEN, exist_ok=True)
    todo = cases()
    for name in names or sorted(todo):
        arrs = generate(name, todo[name])
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **arrs)
        print(f"{name}: n={arrs['cell'].size} outside={int(arrs['n_outside'])} / {int(arrs['n_outside_levels'])} with levels, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
