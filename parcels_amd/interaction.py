"""Neighbour search for particle-particle interaction kernels.

The reference's interaction kernels (docs/user_guide/examples/tutorial_interaction.ipynb) build dense all-pairs distance
matrices in NumPy inside ``def kernel(particles, fieldset)``; that is N x N memory and time.  The functions here give the
same numbers -- bit for bit -- from a cell list on the GPU (csrc/pk_neighbors.hip):

    nb = pa.neighbors(particles, radius)        # CSR pair list: nb.i, nb.j, nb.dx, nb.dy, nb.dist, nb.count, nb.starts
    pa.neighbor_counts(particles, radius)       # the counts alone, no pair list
    pa.nearest_neighbor(particles, radius)      # (index, distance) of the nearest neighbour, -1 / inf without one

Semantics: points are float64 (float32 columns are widened, which is exact), flat Euclidean;
``dx = x[j] - x[i]``, ``dist = np.sqrt(dx**2 + dy**2 [+ dz**2])``; j is a neighbour of i iff ``i != j``, ``dist < radius``
(strict), ``sources[j]`` when a mask is given and ``dist > 0`` with ``include_coincident=False``.  A particle with a
non-finite coordinate has no neighbours and is nobody's neighbour.  Rows are ordered by i, j ascends within a row; the nearest
neighbour is the smallest dist, ties to the smallest j.  Indices are local to the view passed in.

Spherical meshes: ``mesh="spherical"``, a ``SphericalMesh`` or the ``fieldset`` of a kernel body (``mesh=fieldset``: the mesh of its
first grid) switch to great-circle distances.  ``x`` is then the longitude and ``y`` the latitude in degrees -- longitudes are
equivalent modulo 360, so -180..180, 0..360 and values past either end mix freely -- and ``radius``, ``z`` and ``dist`` are in metres;
``radius`` must stay below a quarter of the circumference.  With ``rad = pi / 180`` and R the mesh's radius::

    dx   = d - 360*rint(d/360),  d = x[j] - x[i]          # degrees, in [-180, 180]: wrapped across the antimeridian
    dy   = y[j] - y[i]
    a    = sin(0.5*rad*dy)**2 + cos(rad*y[i])*cos(rad*y[j])*sin(0.5*rad*dx)**2
    dh   = 2*R*arcsin(min(1, sqrt(a)))
    dist = dh            (z=False)      sqrt(dh*dh + dz*dz)   (z=True)

``dx``, ``dy``, ``dz`` equal the NumPy expressions bit for bit; ``dist`` passes through ``sin``, ``cos`` and ``arcsin``, whose device
versions differ from NumPy's by ulps (the package's parity bar of 1e-12 relative holds with room).  A particle with ``|y| > 90`` is
treated like one with a non-finite coordinate.  ``mesh="flat"``, the default, is the Euclidean search above for every particle set,
also one on a spherical fieldset: the mesh is never guessed.

There is no CPU path: without a GPU every call raises ``HipLibraryError`` like every other device call of the package.
"""

from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

__all__ = ["Neighbors", "neighbors", "neighbor_counts", "nearest_neighbor", "MAX_PAIRS_MEMORY_SHARE"]

# default max_pairs: the pair list (device scratch + outputs) may take this share of the free device memory
MAX_PAIRS_MEMORY_SHARE = 0.5
_MAX_PAIRS_HARD = 2**31 - 1  # one call lists at most this many pairs (csrc/pk_neighbors.hip: NB_MAX_PAIRS)

_contexts: dict = {}  # device index -> _hip.Context, created on first use


def device_bytes_per_pair(z: bool) -> int:
    """Device memory one listed pair takes: row and column index as uint32 (fill), the sorted column index (uint32), and the
    outputs j (int64), dx, dy, dist (+ dz) as float64."""
    return 3 * 4 + 8 + (4 if z else 3) * 8


def _context(device: int = 0):
    from . import _hip

    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = _hip.Context(device)
    return ctx


class Neighbors:
    """A neighbour list in CSR form: row i holds the neighbours of particle i, ``j`` ascending."""

    def __init__(self, count, starts, j, dx, dy, dz, dist):
        self.count, self.starts, self.j, self.dx, self.dy, self.dist = count, starts, j, dx, dy, dist
        if dz is not None:
            self.dz = dz
        self._i = None

    @property
    def n(self) -> int:
        return len(self.count)

    @property
    def total(self) -> int:
        return len(self.j)

    @property
    def i(self):
        if self._i is None:
            self._i = np.repeat(np.arange(self.n, dtype=np.int64), self.count)
        return self._i

    def sum(self, per_pair_values):
        """Row sums of one value per pair, added in pair order: ``np.bincount(nb.i, weights=values, minlength=n)``."""
        v = np.asarray(per_pair_values, dtype=np.float64)
        if v.shape != (self.total,):
            raise ValueError(f"per_pair_values: expected one value per pair, shape ({self.total},), got {v.shape}")
        return np.bincount(self.i, weights=v, minlength=self.n).astype(np.float64, copy=False)

    def __repr__(self):
        return f"Neighbors({self.n} particles, {self.total} pairs)"


def _columns(particles, z: bool):
    """(x, y, z | None) as contiguous float64 arrays of one length."""
    if isinstance(particles, (tuple, list)):
        if len(particles) not in (2, 3):
            raise TypeError(f"particles: a tuple of arrays must be (x, y) or (x, y, z), got {len(particles)} entries")
        if z and len(particles) < 3:
            raise ValueError("z: z=True needs a z array, particles is (x, y)")
        raw = list(particles[: 3 if z else 2])
    else:
        names = ("x", "y", "z") if z else ("x", "y")
        raw = []
        for name in names:
            try:
                raw.append(getattr(particles, name))
            except AttributeError:
                if name == "z":
                    raise ValueError("z: z=True needs a z column, particles has none") from None
                raise TypeError(f"particles: expected a particle view, a ParticleSet or a tuple of arrays; {type(particles).__name__} "
                                f"has no column {name!r}") from None
    cols = []
    for name, a in zip("xyz", raw):
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError(f"particles: {name} must be 1-D, got shape {a.shape}")
        if a.dtype.kind not in "fiu":
            raise TypeError(f"particles: {name} must be a real numeric array, got dtype {a.dtype}")
        cols.append(np.ascontiguousarray(a, dtype=np.float64))
    n = len(cols[0])
    for name, a in zip("xyz", cols):
        if len(a) != n:
            raise ValueError(f"particles: x has length {n}, {name} has length {len(a)}")
    return cols[0], cols[1], (cols[2] if z else None)


def _validate(particles, radius, z, sources, max_pairs=None, mesh="flat"):
    if isinstance(radius, bool) or not isinstance(radius, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f"radius: expected a finite positive number, got {type(radius).__name__}")
    radius = float(radius)
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError(f"radius: expected a finite positive number, got {radius!r}")
    x, y, zz = _columns(particles, bool(z))
    src = None
    if sources is not None:
        s = np.asarray(sources)
        if s.dtype != np.bool_:
            raise TypeError(f"sources: expected a boolean mask, got dtype {s.dtype}")
        if s.shape != (len(x),):
            raise ValueError(f"sources: expected shape ({len(x)},), got {s.shape}")
        src = np.ascontiguousarray(s).view(np.uint8)
    if max_pairs is not None:
        if isinstance(max_pairs, bool) or not isinstance(max_pairs, (numbers.Integral, np.integer)):
            raise TypeError(f"max_pairs: expected a non-negative integer or None, got {type(max_pairs).__name__}")
        if max_pairs < 0:
            raise ValueError(f"max_pairs: expected a non-negative integer or None, got {max_pairs}")
    return radius, x, y, zz, src, _sphere_radius(mesh, radius)


def _sphere_radius(mesh, radius):
    """None for a flat mesh, else the radius of the sphere; checks ``radius`` against a quarter of its circumference."""
    from .fieldset import FieldSet
    from .xgrid import FlatMesh, SphericalMesh, get_mesh

    if isinstance(mesh, FieldSet):
        fields = list(mesh.fields.values())
        if not fields:
            raise ValueError("mesh: the FieldSet has no field, so no grid to take the mesh from")
        mesh = fields[0].grid._mesh  # the first grid of fieldset.gridset
    if not isinstance(mesh, (str, FlatMesh, SphericalMesh)):  # get_mesh compares with ==, which an array answers element-wise
        raise ValueError(f"mesh must be 'flat', 'spherical', or a SphericalMesh object. Got {mesh=!r}")
    mesh = get_mesh(mesh)
    if not mesh.is_spherical():
        return None
    sphere = float(mesh.radius)
    if not radius < 0.5 * math.pi * sphere:
        raise ValueError(f"radius: {radius!r} is not below a quarter of the circumference of the mesh's sphere, {0.5 * math.pi * sphere!r} "
                         f"(sphere radius {sphere!r}); great-circle neighbour search needs radius < (pi / 2) R")
    return sphere


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _build(ctx, radius, x, y, z, src, include_coincident, sphere=None):
    from . import _hip

    flags = 0 if include_coincident else _hip.PK_NEIGHBORS_NO_COINCIDENT
    if sphere is not None:
        ctx.check(ctx.lib.pk_neighbors_build_spherical(ctx.handle, len(x), _ptr(x), _ptr(y), _ptr(z), _ptr(src), radius, sphere, flags),
                  "pk_neighbors_build_spherical")
        return
    ctx.check(ctx.lib.pk_neighbors_build(ctx.handle, len(x), _ptr(x), _ptr(y), _ptr(z), _ptr(src), radius, flags), "pk_neighbors_build")


def neighbor_counts(particles, radius, *, z=False, sources=None, include_coincident=True, mesh="flat"):
    """Number of neighbours of every particle, int64[n]; builds no pair list."""
    radius, x, y, zz, src, sphere = _validate(particles, radius, z, sources, mesh=mesh)
    ctx = _context()
    _build(ctx, radius, x, y, zz, src, include_coincident, sphere)
    count = np.zeros(len(x), dtype=np.int64)
    total = C.c_int64()
    ctx.check(ctx.lib.pk_neighbors_counts(ctx.handle, _ptr(count), C.byref(total)), "pk_neighbors_counts")
    return count


def nearest_neighbor(particles, radius, *, z=False, sources=None, include_coincident=True, mesh="flat"):
    """(j, dist): index (int64[n], -1 without a neighbour) and distance (float64[n], inf without one) of the nearest neighbour
    within ``radius``; ties go to the smallest index."""
    radius, x, y, zz, src, sphere = _validate(particles, radius, z, sources, mesh=mesh)
    ctx = _context()
    _build(ctx, radius, x, y, zz, src, include_coincident, sphere)
    j = np.full(len(x), -1, dtype=np.int64)
    dist = np.full(len(x), np.inf, dtype=np.float64)
    ctx.check(ctx.lib.pk_neighbors_nearest(ctx.handle, _ptr(j), _ptr(dist)), "pk_neighbors_nearest")
    return j, dist


def neighbors(particles, radius, *, z=False, sources=None, include_coincident=True, max_pairs=None, mesh="flat"):
    """Every ordered pair (i, j) with j a neighbour of i, as a ``Neighbors`` CSR list.

    The total is known after the count pass; when it exceeds ``max_pairs`` a ``ValueError`` states the total and the cap, and
    nothing is allocated or fetched.  Default cap: what fits in ``MAX_PAIRS_MEMORY_SHARE`` of the free device memory."""
    radius, x, y, zz, src, sphere = _validate(particles, radius, z, sources, max_pairs, mesh)
    ctx = _context()
    _build(ctx, radius, x, y, zz, src, include_coincident, sphere)
    n = len(x)
    count = np.zeros(n, dtype=np.int64)
    total = C.c_int64()
    ctx.check(ctx.lib.pk_neighbors_counts(ctx.handle, _ptr(count), C.byref(total)), "pk_neighbors_counts")
    total = int(total.value)
    if max_pairs is None:
        free = ctx.device_info()["free_mem"]
        cap, why = int(MAX_PAIRS_MEMORY_SHARE * free) // device_bytes_per_pair(zz is not None), (
            f"the default: {MAX_PAIRS_MEMORY_SHARE:.0%} of the {free} free bytes of device memory at {device_bytes_per_pair(zz is not None)} bytes per pair")
    else:
        cap, why = int(max_pairs), "max_pairs"
    if total > cap:
        raise ValueError(f"max_pairs: {total} neighbour pairs exceed the cap of {cap} ({why}); use a smaller radius, neighbor_counts / "
                         "nearest_neighbor, or raise max_pairs")
    if total > _MAX_PAIRS_HARD:
        raise ValueError(f"max_pairs: {total} neighbour pairs exceed the {_MAX_PAIRS_HARD} one call can list")
    starts = np.zeros(n + 1, dtype=np.int64)
    j = np.empty(total, dtype=np.int64)
    dx = np.empty(total, dtype=np.float64)
    dy = np.empty(total, dtype=np.float64)
    dz = np.empty(total, dtype=np.float64) if zz is not None else None
    dist = np.empty(total, dtype=np.float64)
    ctx.check(ctx.lib.pk_neighbors_pairs(ctx.handle, total, _ptr(starts), _ptr(j), _ptr(dx), _ptr(dy), _ptr(dz), _ptr(dist)), "pk_neighbors_pairs")
    return Neighbors(count, starts, j, dx, dy, dz, dist)


def cell_list_info() -> dict:
    """What the last build on the default context chose: points, finite points, cells, cell size, doublings, announced total."""
    from . import _hip

    ctx = _context()
    info = _hip.NeighborsInfo()
    ctx.check(ctx.lib.pk_neighbors_info(ctx.handle, C.byref(info)), "pk_neighbors_info")
    return {k: getattr(info, k) for k in ("n", "nvalid", "ncx", "ncy", "total", "cell_size", "doublings")}


def cell_list_info_spherical() -> dict:
    """What the last spherical build on the default context chose: points, valid points, latitude bands, longitude cells summed over
    them, band height in degrees, whether the bands wrap over 360 degrees, doublings, announced total.  Zeros after a flat build."""
    from . import _hip

    ctx = _context()
    info = _hip.NeighborsSphInfo()
    ctx.check(ctx.lib.pk_neighbors_info_spherical(ctx.handle, C.byref(info)), "pk_neighbors_info_spherical")
    out = {k: getattr(info, k) for k in ("n", "nvalid", "bands", "cells", "total", "band_height", "doublings")}
    out["periodic"] = bool(info.periodic)
    return out


def release():
    """Free the device scratch of the default context's cell list (it is otherwise kept for the next call)."""
    ctx = _contexts.get(0)
    if ctx is not None:
        ctx.check(ctx.lib.pk_neighbors_release(ctx.handle), "pk_neighbors_release")
