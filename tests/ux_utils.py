"""Helpers shared by the unstructured-mesh tests (tests/test_gpu_ux.py, tests/test_gpu_ux_fuzz.py, tests/test_ux_oracle.py): a case dict of
tools/make_ux_golden.py as a parcels_amd FieldSet, its ParticleSet.execute on the device, and the tolerance classes of DESIGN.md section 11."""

import warnings

import numpy as np

import parcels_amd as pa
from case_utils import OutputRecorder

ERRORS = (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.FieldInterpolationError, pa.GridSearchingError, pa.OutsideTimeInterval,
          pa.GeneralError)


def ux_dataset(case):
    mesh = pa.UxMesh(case["node_lon"], case["node_lat"], case["faces"])
    coords = {"time": (("time",), np.asarray(case["time_s"], dtype=np.float64)), "zf": (("zf",), case["zf"]), "zc": (("zc",), case["zc"])}
    return pa.Dataset({n: (dims, arr) for n, (arr, dims) in case["fields"].items()}, coords, uxgrid=mesh)


def ux_fieldset(case, nslots=None):
    fs = pa.FieldSet.from_ugrid_conventions(ux_dataset(case), mesh=case["mesh"])
    for k, v in (case.get("constants") or {}).items():
        fs.add_constant_field(k, v, mesh="flat")
    if nslots is not None:
        fs.to_device(nslots=nslots)
    return fs


def run_ux(case, fs=None):
    """the fixture's ParticleSet.execute on the device -> (SoA dict, error name or None, output recorder or None)"""
    fs = fs if fs is not None else ux_fieldset(case, nslots=case.get("nslots"))
    pclass = pa.get_default_particle(np.float32 if case["spatial_dtype"] == "float32" else np.float64)
    kernels = []
    for k in case["kernels"]:
        if k == "SampleField":
            kernels.append(pa.SampleField(case["sample"], into="sampled"))
        elif k == "SampleConst":
            kernels.append(pa.SampleField("Kconst", into="kc"))
        else:
            kernels.append(getattr(pa, k))
    if {"SampleField", "SampleConst"} & set(case["kernels"]):
        pclass = pclass.add_variable(pa.Variable("sampled", dtype=np.float64, initial=0)).add_variable(pa.Variable("kc", dtype=np.float64, initial=0))
    n = len(case["x"])
    t = np.zeros(n) if case.get("t0") is None else np.broadcast_to(np.asarray(case["t0"], dtype=np.float64), (n,)).copy()
    pset = pa.ParticleSet(fs, pclass=pclass, x=np.asarray(case["x"]), y=np.asarray(case["y"]), z=np.asarray(case["z"]), t=t)
    kw = {"runtime": float(case["runtime"])}
    rec = None
    if case.get("outputdt"):
        kw["output_file"] = rec = OutputRecorder(float(case["outputdt"]))
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute(kernels, dt=float(case["dt"]), **kw)
        except ERRORS as e:
            err = type(e).__name__
    return {k: np.array(v) for k, v in pset._data.items()}, err, rec


def coordinate_scale(case):
    return max(float(np.max(np.abs(case["node_lon"]))), float(np.max(np.abs(case["node_lat"]))), float(np.max(np.abs(case["zf"]))))


# The one fixture whose positions are held to the float32 class: a spherical mesh with NODE-registered velocity.  UxGrid.search forms the
# query point with float32 deg2rad / cos / sin (uxgrid.py:107-109, index_search.py:298-312); NumPy's float32 sin / cos are not correctly
# rounded (about one argument in six is off by an ulp) and the device's are (csrc/pk_ux.h: ux_query), so the projected point -- and with it the barycentric weights of
# a node-registered field -- moves by ~1e-7 relative at some of the ~150 searches of every trajectory: 2e-9 relative in position after
# 36 RK4 steps.  Discrete results (state, ei, t) stay exact.  test_field_eval_matches_the_reference pins the attribution point by point.
FLOAT32_TRIG_FIXTURES = {"ux_sph_node_rk4_3d": 1e-8}


def tolerance_for(name, case):
    """relative tolerance of a fixture's positions"""
    if case["spatial_dtype"] == "float32":
        return 5e-7  # one float32 ulp of a stored position (case_utils.tolerance_for: device cosf vs NumPy's float32 cos)
    return FLOAT32_TRIG_FIXTURES.get(name, 1e-12)


def numpy_f32_trig_differs(y, x):
    """the query points whose float32 deg2rad / sin / cos NumPy does NOT round correctly -- where a spherical search of the reference
    differs from the device's by an ulp of the float32 unit-sphere point"""
    lat, lon = np.deg2rad(np.asarray(y, np.float32)), np.deg2rad(np.asarray(x, np.float32))
    bad = np.zeros(lat.shape, bool)
    for a in (lat, lon):
        for f in (np.sin, np.cos):
            bad |= f(a) != f(a.astype(np.float64)).astype(np.float32)
    return bad
