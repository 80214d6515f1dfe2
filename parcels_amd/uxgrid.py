"""Unstructured triangle meshes (mirrors src/parcels/_core/uxgrid.py and the UGRID half of _core/model.py).

``UxMesh`` is the small mesh container that stands in for ``uxarray.Grid``: node coordinates and the triangle connectivity.
``UxGrid`` wraps it with the vertical interfaces ``zf`` exactly like the reference; the face search itself runs on the GPU
(csrc/pk_ux.h) over the host-built Morton table of ``get_spatial_hash``.
"""

from __future__ import annotations

import numpy as np

from .dataset import DataArray, Dataset
from .spatialhash import SpatialHash, latlon_rad_to_xyz
from .xgrid import get_mesh

__all__ = ["UxMesh", "UxGrid", "UnstructuredModelData"]


class UxMesh:
    """A UGRID triangle mesh: ``node_lon``, ``node_lat`` (n_node,) and ``face_node_connectivity`` (n_face, 3), zero-based.
    Coordinates are kept as float64."""

    def __init__(self, node_lon, node_lat, face_node_connectivity):
        self.node_lon = np.ascontiguousarray(node_lon, dtype=np.float64)
        self.node_lat = np.ascontiguousarray(node_lat, dtype=np.float64)
        fnc = np.asarray(face_node_connectivity)
        if fnc.ndim != 2:
            raise ValueError("face_node_connectivity must be a 2-D array (n_face, n_max_face_nodes)")
        if self.node_lon.shape != self.node_lat.shape or self.node_lon.ndim != 1:
            raise ValueError("node_lon and node_lat must be 1-D arrays of the same length")
        self.face_node_connectivity = np.ascontiguousarray(fnc, dtype=np.int64)
        if fnc.size and (self.face_node_connectivity.min() < 0 or self.face_node_connectivity.max() >= self.n_node):
            raise ValueError("face_node_connectivity refers to nodes that do not exist")

    @property
    def n_face(self) -> int:
        return int(self.face_node_connectivity.shape[0])

    @property
    def n_node(self) -> int:
        return int(self.node_lon.shape[0])

    @property
    def n_max_face_nodes(self) -> int:
        return int(self.face_node_connectivity.shape[1])

    def node_xyz(self):
        """unit-sphere coordinates of the nodes (index_search.py:439-450 on deg2rad of lat / lon)"""
        return latlon_rad_to_xyz(np.deg2rad(self.node_lat), np.deg2rad(self.node_lon))

    def __repr__(self):
        return f"UxMesh(n_node={self.n_node}, n_face={self.n_face})"


class UxGrid:
    """uxgrid.py:16-135.  ``grid``: a UxMesh; ``z``: the 1-D layer interfaces (zf) as a DataArray or array; ``mesh``: "flat" or
    "spherical"."""

    def __init__(self, grid: UxMesh, z, mesh):
        if grid.n_max_face_nodes > 3:  # uxgrid.py:39
            raise ValueError("Provided ux.grid.Grid must contain only triangular cells (n_max_face_nodes=3)")
        if grid.n_max_face_nodes < 3:
            raise ValueError("Provided ux.grid.Grid must contain only triangular cells (n_max_face_nodes=3)")
        self.uxgrid = grid
        if not isinstance(z, DataArray):
            if isinstance(z, (np.ndarray, list, tuple)):
                z = np.asarray(z)
                z = DataArray(tuple(f"zf{i}" if i else "zf" for i in range(z.ndim)), z)
            else:
                raise TypeError("z must be an instance of ux.UxDataArray")
        if z.ndim != 1:
            raise ValueError("z must be a 1D array of vertical coordinates")
        self.z = z
        self._mesh = get_mesh(mesh)
        self._spatialhash = None

    @property
    def depth(self):
        return np.asarray(self.z.values)

    @property
    def axes(self) -> list[str]:
        return ["Z", "FACE"]

    def get_axis_dim(self, axis: str) -> int:
        if axis not in self.axes:
            raise ValueError(f"Axis {axis!r} is not part of this grid. Available axes: {self.axes}")
        if axis == "Z":
            return len(self.z.values)
        return self.uxgrid.n_face

    @property
    def deg2m(self) -> float:
        if self._mesh.is_spherical():
            return self._mesh.deg2m
        return 1.0

    @property
    def is_curvilinear(self) -> bool:
        return False

    def ravel_index(self, axis_indices: dict) -> np.ndarray:  # basegrid.py:83-118, 254-278
        dims = np.array([self.get_axis_dim(a) for a in self.axes], dtype=int)
        idx = np.array([axis_indices[a] for a in self.axes], dtype=int)
        return idx[0] * dims[1] + idx[1]

    def unravel_index(self, ei) -> dict:  # basegrid.py:120-152, 219-252
        dims = np.array([self.get_axis_dim(a) for a in self.axes], dtype=int)
        ei = np.asarray(ei)
        return {"Z": ei // dims[1], "FACE": ei % dims[1]}

    def cell_areas(self) -> np.ndarray:
        """Area of every triangle, shape ``(n_face,)``.  Flat mesh: the planar area in mesh units squared.  Spherical mesh: the nodes are
        put on the sphere of radius ``deg2m * 180 / pi`` and the area of the planar triangle through them is taken, in m**2 -- the *chordal*
        approximation of the spherical triangle (low by about (edge angle)**2 / 12 relative)."""
        from .xgrid import _chordal_area, _sphere_xyz

        m = self.uxgrid
        f = m.face_node_connectivity
        if self._mesh.is_spherical():
            xyz = _sphere_xyz(m.node_lon, m.node_lat, self.deg2m * 180.0 / np.pi)
            return _chordal_area([xyz[f[:, k]] for k in range(3)])
        x, y = m.node_lon[f], m.node_lat[f]
        return np.abs(0.5 * ((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])))

    def get_spatial_hash(self) -> SpatialHash:
        if self._spatialhash is None:
            self._spatialhash = SpatialHash.from_triangles(self.uxgrid.node_lon, self.uxgrid.node_lat, self.uxgrid.face_node_connectivity,
                                                           self._mesh.is_spherical())
        return self._spatialhash

    def __repr__(self):
        return f"UxGrid(n_face={self.uxgrid.n_face}, n_zf={self.get_axis_dim('Z')}, mesh={self._mesh!r})"


_LATERAL = ("n_face", "n_node")
_VERTICAL = ("zf", "zc")


def select_uxinterpolator(da: DataArray):
    """model.py:468-500: the Ux* interpolator of a field from its (vertical, lateral) dims, None when no pair matches"""
    from .interpolators import UxConstantFaceConstantZC, UxConstantFaceLinearZF, UxLinearNodeConstantZC, UxLinearNodeLinearZF

    mapping = {"zc,n_face": UxConstantFaceConstantZC, "zc,n_node": UxLinearNodeConstantZC, "zf,n_node": UxLinearNodeLinearZF,
               "zf,n_face": UxConstantFaceLinearZF}
    spatial = tuple(d for d in da.dims if d not in ("time",))
    if len(spatial) != 2:
        raise ValueError("Fields on unstructured grids must have two spatial dimensions, one vertical (zf or zc) and one lateral (n_face, n_edge, or n_node)")
    vdim = next((d for d in spatial if d in _VERTICAL), None)
    ldim = next((d for d in spatial if d in _LATERAL), None)
    if vdim and ldim:
        return mapping.get(f"{vdim},{ldim}")
    return None


def discover_ux_u_and_v(ds: Dataset) -> Dataset:
    """model.py: _discover_ux_U_and_V -- (unod, vnod) / (u, v) become U / V, w becomes W"""
    dv = ds.data_vars
    rename = {}
    if "W" not in dv and "w" in dv:
        rename["w"] = "W"
    if "U" in dv and "V" in dv:
        pass
    elif "U" in dv or "V" in dv:
        raise ValueError("Dataset has only one of the two variables 'U' and 'V'. Please rename the appropriate variable in your dataset to have both 'U' and 'V' for Parcels simulation.")
    else:
        for cu, cv in (("unod", "vnod"), ("u", "v")):
            if cu in dv:
                if cv not in dv:
                    raise ValueError(f"Dataset has variable with standard name {cu!r}, but not the matching variable with standard name {cv!r}. "
                                     "Please rename the appropriate variables in your dataset to have both 'U' and 'V' for Parcels simulation.")
                rename[cu], rename[cv] = "U", "V"
                break
            if cv in dv:
                raise ValueError(f"Dataset has variable with standard name {cv!r}, but not the matching variable with standard name {cu!r}. "
                                 "Please rename the appropriate variables in your dataset to have both 'U' and 'V' for Parcels simulation.")
    if not rename:
        return ds
    out = ds.copy()
    out.data_vars = {rename.get(k, k): v for k, v in ds.data_vars.items()}
    return out


class UnstructuredModelData:
    """Dataset + UxGrid + interpolator registry (model.py:320-380).  Field data is kept as (time, z, 1, lateral) float64 arrays, the
    layout of a device field on a UxGrid (include/parcels_hip.h: pk_field_desc)."""

    def __init__(self, ds: Dataset, grid: UxGrid, vector_field_components: dict):
        from .field import to_seconds

        self.data = ds
        self.grid = grid
        self.vector_field_components = dict(vector_field_components)
        self.field_to_interpolator: dict = {}
        self._fields = None
        self.time_values = None
        self.time_flt = None
        if "time" in ds.coords and ds.coords["time"].data.size > 1:
            tv = np.asarray(ds.coords["time"].data)
            self.time_values = tv
            if np.issubdtype(tv.dtype, np.datetime64) or np.issubdtype(tv.dtype, np.timedelta64):
                self.time_flt = to_seconds(tv - tv[0])
            else:
                self.time_flt = tv.astype(np.float64) - float(tv[0])
            if not np.all(np.diff(self.time_flt) > 0):
                raise ValueError("time levels must be strictly increasing")
        self._tzyx = {}

    @property
    def time_interval(self):
        from .field import TimeInterval

        if self.time_values is None:
            return None
        tv = self.time_values
        if np.issubdtype(tv.dtype, np.datetime64) or np.issubdtype(tv.dtype, np.timedelta64):
            return TimeInterval(tv[0], tv[-1])
        return TimeInterval(np.timedelta64(int(round(float(tv[0]) * 1e9)), "ns"), np.timedelta64(int(round(float(tv[-1]) * 1e9)), "ns"))

    def field_data(self, name):
        return self.data.data_vars[name]

    def device_layout(self, name) -> np.ndarray:
        """(nt, nz, 1, n_lateral) view of a field's data (time first, vertical second, lateral last)"""
        if name not in self._tzyx:
            da = self.data.data_vars[name]
            dims = list(da.dims)
            data = np.asarray(da.data)
            if "time" not in dims:
                data = data[None]
                dims = ["time"] + dims
            v = next(d for d in dims if d in _VERTICAL)
            lat = next(d for d in dims if d in _LATERAL)
            data = np.transpose(data, [dims.index("time"), dims.index(v), dims.index(lat)])
            if np.issubdtype(data.dtype, np.floating) and np.isnan(data).any():  # model.py:135-143 fillna(0)
                data = np.nan_to_num(data, nan=0.0)
            self._tzyx[name] = data[:, :, None, :]
        return self._tzyx[name]

    def construct_fields(self):
        from .field import Field, VectorField
        from .interpolators import Ux_Velocity

        single = {name: Field(str(name), self) for name in self.data.data_vars}
        vectors = {vname: VectorField(vname, *[single[c] for c in comps], interp_method=Ux_Velocity())
                   for vname, comps in self.vector_field_components.items()}
        return list({**single, **vectors}.values())

    @classmethod
    def from_ugrid_conventions(cls, ds: Dataset, *, mesh, vector_fields):
        """model.py:357-380"""
        dims = sorted(ds.dims)
        if not all(d in dims for d in ("time", "zf", "zc")):
            raise ValueError(f"Dataset missing one of the required dimensions 'time', 'zf', or 'zc' for uxDataset. Found dimensions {dims}")
        if getattr(ds, "uxgrid", None) is None:
            raise ValueError("Dataset carries no unstructured mesh (Dataset(..., uxgrid=UxMesh(...)))")
        grid = UxGrid(ds.uxgrid, z=ds.coords["zf"], mesh=mesh)
        ds = discover_ux_u_and_v(ds)
        if vector_fields is None:  # model.py:404-412
            vector_fields = {}
            names = set(ds.data_vars)
            if {"U", "V"} <= names:
                vector_fields["UV"] = ("U", "V")
            if {"U", "V", "W"} <= names:
                vector_fields["UVW"] = ("U", "V", "W")
        if not isinstance(vector_fields, dict):
            raise ValueError(f"vector_fields must be a dictionary. Got {type(vector_fields)=!r}.")
        for vname, comps in vector_fields.items():
            if not (2 <= len(comps) <= 3):
                raise ValueError(f"Vector field {vname} must have 2 or 3 components")
            for c in comps:
                if c not in ds.data_vars:
                    raise ValueError(f"Field component '{c}' not present in the source dataset")
        for name, da in ds.data_vars.items():
            for d, n in zip(da.dims, da.shape):
                want = {"n_face": grid.uxgrid.n_face, "n_node": grid.uxgrid.n_node}.get(d)
                if want is not None and n != want:
                    raise ValueError(f"field '{name}': dimension {d!r} has {n} entries, the mesh has {want}")
        from .field import Field

        model = cls(ds, grid, vector_fields)
        model._fields = model.construct_fields()
        for f in model._fields:
            if isinstance(f, Field):
                interp = select_uxinterpolator(model.data[f.name])
                if interp is not None:
                    f.interp_method = interp()
        return model

