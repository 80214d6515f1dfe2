"""Helpers shared by tests/test_gpu_ux_kernels.py and tests/test_ux_kernels_host.py: a case dict of tools/make_ux_kernels_golden.py (the
case dicts of tools/make_ux_golden.py plus seed, context and the mesh of the constant fields) as a parcels_amd FieldSet, and its run."""

import warnings

import numpy as np

import parcels_amd as pa
from case_utils import OutputRecorder
from ux_utils import ERRORS, ux_dataset


def uxk_fieldset(case):
    fs = pa.FieldSet.from_ugrid_conventions(ux_dataset(case), mesh=case["mesh"])
    for k, v in (case.get("constants") or {}).items():
        fs.add_constant_field(k, v, mesh=case.get("const_mesh") or "flat")
    for k, v in (case.get("context") or {}).items():
        fs.add_context(k, v)
    return fs


def uxk_pset(case, fs, pclass=None, **variables):
    if pclass is None:
        pclass = pa.get_default_particle(np.float32 if case["spatial_dtype"] == "float32" else np.float64)
    n = len(case["x"])
    t = np.zeros(n) if case.get("t0") is None else np.broadcast_to(np.asarray(case["t0"], dtype=np.float64), (n,)).copy()
    return pa.ParticleSet(fs, pclass=pclass, x=np.asarray(case["x"]), y=np.asarray(case["y"]), z=np.asarray(case["z"]), t=t,
                          seed=int(case.get("seed") or 0), **variables)


def run_uxk(case, kernels=None, pclass=None, **variables):
    """ParticleSet.execute of the case on the device -> (SoA dict, error name or None, output recorder or None, the ParticleSet)"""
    fs = uxk_fieldset(case)
    pset = uxk_pset(case, fs, pclass, **variables)
    if kernels is None:
        kernels = [getattr(pa, k) for k in case["kernels"]]
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
    return {k: np.array(v) for k, v in pset._data.items()}, err, rec, pset
