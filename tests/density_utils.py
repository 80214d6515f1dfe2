"""Helpers shared by tests/test_density_host.py and tests/test_gpu_density.py: a fixture of tools/make_density_golden.py as a parcels_amd
FieldSet / ParticleSet, and a NumPy restatement of ParticleSet.density that turns expected cells into maps."""

import glob
import os

import numpy as np

import parcels_amd as pa
from case_utils import build_fieldset
from tools import make_density_golden as dg
from ux_utils import ux_fieldset

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(dg.GOLDEN, "dens_*.npz")))
_CACHE = {}


def fixture(name):
    """the committed fixture (loaded once, shared, never changed by a test)"""
    if name not in _CACHE:
        _CACHE[name] = dg.load(os.path.join(dg.GOLDEN, name + ".npz"))
    return _CACHE[name]


def density_fieldset(case):
    """zero velocity on the fixture's mesh (float64 data; the density map only looks at the grid)"""
    if case["kind"] == "ux":
        nf, nn = case["faces"].shape[0], case["node_lon"].size
        zf = np.asarray(case["zf"])
        zc = 0.5 * (zf[:-1] + zf[1:])
        fields = {"U": (np.zeros((2, zc.size, nf)), ("time", "zc", "n_face")), "V": (np.zeros((2, zc.size, nf)), ("time", "zc", "n_face")),
                  "T": (np.zeros((2, zf.size, nn)), ("time", "zf", "n_node"))}
        return ux_fieldset(dict(case, fields=fields, zc=zc, time_s=np.array([0.0, 86400.0])))
    lon, lat, depth = case["lon"], case["lat"], case["depth"]
    full = ("time", "depth" if depth is not None else "mockZ", "YG", "XG")
    z = np.zeros((2, depth.size if depth is not None else 1, lat.shape[0], lon.shape[-1]))
    return build_fieldset(dict(mesh=case["mesh"], lon=lon, lat=lat, depth=depth, time_s=np.array([0.0, 86400.0]),
                               fields={"U": z, "V": z.copy()}, field_dims={"U": full, "V": full}))


def density_pset(case, fs, pclass=None, **kw):
    sdt = np.dtype(case["spatial_dtype"]).type
    pclass = pclass if pclass is not None else pa.get_default_particle(sdt)
    n = len(case["x"])
    return pa.ParticleSet(fs, pclass=pclass, x=np.array(case["x"]), y=np.array(case["y"]), z=np.array(case["z"]), t=np.zeros(n), **kw)


def density_numpy(cell, shape, weights=None, relative=False, areas=None, return_outside=False):
    """ParticleSet.density restated: `cell` is per particle its ravelled cell over `shape`, or -1 (outside)"""
    cell = np.asarray(cell, dtype=np.int64)
    inside = cell >= 0
    ncells = int(np.prod(shape))
    if weights is None:
        m = np.bincount(cell[inside], minlength=ncells).astype(np.int64)
    else:
        m = np.bincount(cell[inside], weights=np.asarray(weights, dtype=np.float64)[inside], minlength=ncells)
    m = m.reshape(shape)
    if relative:
        m = m.astype(np.float64)
        total = m.sum()
        m = m / total if total != 0 else np.zeros_like(m)
    if areas is not None:
        m = m / (areas if m.ndim == np.ndim(areas) else np.asarray(areas)[None])
    return (m, int(np.count_nonzero(~inside))) if return_outside else m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
