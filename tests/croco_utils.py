"""What the GPU tests of the CROCO sigma-grid program share (tests/test_gpu_croco.py, tests/test_gpu_croco_fuzz.py): the fieldset built the
way a user builds it (parcels_amd.convert.croco_to_sgrid + FieldSet.from_sgrid_conventions), the run of a case on the device, and the
comparison in the project's tolerance classes."""

import warnings

import numpy as np

import parcels_amd as pa
from case_utils import OutputRecorder
from tools import make_croco_golden as mg

ERRORS = (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.FieldInterpolationError, pa.GridSearchingError, pa.OutsideTimeInterval,
          pa.GeneralError)
PROG_SIGMA = 7  # include/parcels_hip.h: pk_exec_stats.program


def croco_fieldset(case, nslots=None):
    """croco_to_sgrid + from_sgrid_conventions, hc as context"""
    co = case["coords"]
    two_d = np.asarray(co["x_rho"]).ndim == 2
    coords = {"x_rho": (("eta_rho", "xi_rho") if two_d else ("xi_rho",), co["x_rho"]),
              "y_rho": (("eta_rho", "xi_rho") if two_d else ("eta_rho",), co["y_rho"]),
              "s_w": (("s_w",), co["s_w"]), "time": (("time",), np.asarray(co["time"], dtype=np.float64))}
    fields = {mg.FIELD_NAMES.get(k, k): (mg.case_dims(case)[k], a) for k, a in case["fields"].items()}
    fs = pa.FieldSet.from_sgrid_conventions(pa.convert.croco_to_sgrid(fields=fields, coords=coords), mesh=case["mesh"])
    fs.add_context("hc", case["hc"])
    if nslots is not None:
        fs.to_device(nslots=nslots)
    return fs


def host_recipe(field, var):
    """the documented recipe for other fields (kernels/_sigmagrids.py:28-35) as the Python kernel a user writes"""

    def kernel(particles, fieldset):
        sigma = pa.convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
        setattr(particles, var, getattr(fieldset, field)[particles.t, sigma, particles.y, particles.x, particles])

    kernel.__name__ = f"Recipe_{field}"
    return kernel


def kernels_of(case):
    """(kernel list, names of the float64 Variables it writes)"""
    out, variables = [], []
    for k in case["kernels"]:
        if k.startswith("SampleFieldCroco:"):
            _, field, var = k.split(":")
            out.append(pa.SampleFieldCroco(field, into=var))
            variables.append(var)
        elif k.startswith("HostRecipe:"):
            _, field, var = k.split(":")
            out.append(host_recipe(field, var))
            variables.append(var)
        else:
            out.append(getattr(pa, k))
            if k == "SampleOmegaCroco":
                variables.append("omega")
    return out, variables


def run_croco(case, fs=None, calls=None, **pset_kw):
    """the fixture's ParticleSet.execute on the device -> (SoA dict, error name or None, output recorder or None, statistics)"""
    fs = fs if fs is not None else croco_fieldset(case)
    kernels, variables = kernels_of(case)
    pclass = pa.get_default_particle(np.float32 if case["spatial_dtype"] == "float32" else np.float64)
    for v in variables:
        pclass = pclass.add_variable(pa.Variable(v, dtype=np.float64, initial=0))
    n = len(case["x"])
    t = np.zeros(n) if case.get("t0") is None else np.broadcast_to(np.asarray(case["t0"], dtype=np.float64), (n,)).copy()
    pset = pa.ParticleSet(fs, pclass=pclass, x=np.asarray(case["x"]), y=np.asarray(case["y"]), z=np.asarray(case["z"]), t=t, **pset_kw)
    rec = None
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            for runtime in (calls or [float(case["runtime"])]):
                kw = {"runtime": runtime}
                if case.get("outputdt"):
                    kw["output_file"] = rec = rec or OutputRecorder(float(case["outputdt"]))
                pset.execute(kernels, dt=float(case["dt"]), **kw)
        except ERRORS as e:
            err = type(e).__name__
    return {k: np.array(v) for k, v in pset._data.items()}, err, rec, pset._last_stats


def scales(case):
    """what `rtol` is relative to beside |reference value|: the largest |x_rho|, |y_rho| for x, y, the largest h for z, the largest |field|
    for a sampled value"""
    co, f = case["coords"], case["fields"]
    xy = max(float(np.max(np.abs(co["x_rho"]))), float(np.max(np.abs(co["y_rho"]))))
    s = {"x": xy, "y": xy, "dx": xy, "dy": xy, "z": float(np.max(f["h"])), "dz": float(np.max(f["h"]))}
    for k in case["kernels"]:
        if ":" in k:
            _, field, var = k.split(":")
            s[var] = float(np.max(np.abs(f[field])))
        elif k == "SampleOmegaCroco":
            s["omega"] = float(np.max(np.abs(f["omega"])))
    return s


def tolerance_for(case):
    """the project's classes (tests/case_utils.py: tolerance_for): 1e-12 for float64 particles, 5e-7 for float32 storage"""
    return 5e-7 if case["spatial_dtype"] == "float32" else 1e-12


def assert_matches(got, ref, case, label):
    """ids, state, ei, t exact; every float column as |a - b| <= rtol (|b| + scale); every particle"""
    rtol = tolerance_for(case)
    np.testing.assert_array_equal(got["particle_id"], ref["particle_id"], err_msg=f"{label}: ids")
    np.testing.assert_array_equal(got["state"], ref["state"], err_msg=f"{label}: state")
    np.testing.assert_array_equal(got["ei"], ref["ei"], err_msg=f"{label}: ei")
    np.testing.assert_array_equal(got["t"], ref["t"], err_msg=f"{label}: t")
    report = {}
    for k, scale in scales(case).items():
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        with np.errstate(invalid="ignore"):
            d = np.abs(a - b)
            ok = (d <= rtol * (np.abs(b) + scale)) | (np.isnan(a) & np.isnan(b)) | (a == b)
        report[k] = float(np.nanmax(np.where(np.isfinite(d), d / (np.abs(b) + scale), 0.0))) if a.size else 0.0
        print(f"{label}: {k}: max |a - b| / (|b| + {scale:g}) = {report[k]:.3e} (rtol {rtol:g})")
        assert ok.all(), f"{label}: {k} differs at {np.flatnonzero(~ok)[:8]}: {a[~ok][:4]} vs {b[~ok][:4]} (max {report[k]:.3e}, rtol {rtol:g})"
    return report
