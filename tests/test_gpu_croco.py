"""GPU: CROCO sigma grids (csrc/pk_sigma.h) against the fixtures the reference generated (tools/make_croco_golden.py), every fieldset
built the way a user builds it: parcels_amd.convert.croco_to_sgrid + FieldSet.from_sgrid_conventions.  Needs no reference."""

import glob
import os
import warnings

import numpy as np
import pytest

import parcels_amd as pa
from croco_utils import ERRORS, PROG_SIGMA, assert_matches, croco_fieldset, run_croco, scales, tolerance_for
from tools import make_croco_golden as mg

pytestmark = pytest.mark.gpu

ALL = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mg.GOLDEN, "croco_*.npz")))
POINTS = [n for n in ALL if n.startswith("croco_sigma_points")]
HOSTED = ["croco_host_recipe"]
TRAJECTORIES = [n for n in ALL if n not in POINTS and n not in HOSTED]
@pytest.mark.parametrize("name", TRAJECTORIES)
def test_fixture_matches_the_reference(gpu, name):
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    ref = case["ref"]
    got, err, rec, stats = run_croco(case)
    assert err == case["err"], (err, case["err"])
    assert_matches(got, ref, case, name)
    if any("CROCO" in k.upper() for k in case["kernels"]):
        assert stats["program"] == PROG_SIGMA
    if "obs_x" in ref:
        assert rec is not None and len(rec.obs) == len(ref["obs_time"])
        rtol, sc = tolerance_for(case), scales(case)
        for k, (_, ids, x, y, z, t) in enumerate(rec.obs):
            np.testing.assert_array_equal(ids, ref["obs_particle_id"][k])
            np.testing.assert_array_equal(t, ref["obs_t"][k])
            for a, col in ((x, "x"), (y, "y"), (z, "z")):
                b = np.asarray(ref["obs_" + col][k], np.float64)
                assert np.all(np.abs(np.asarray(a, np.float64) - b) <= rtol * (np.abs(b) + sc[col])), f"{name}: observation {k}: {col}"


@pytest.mark.parametrize("name", POINTS)
def test_sigma_at_points_matches_the_reference(gpu, name):
    """convert_z_to_sigma_croco(fieldset, t, z, y, x, None) through the public function (pk_sigma_croco), NaN where the reference has NaN"""
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    fs = croco_fieldset(case)
    want = case["ref"]["sigma"]
    got = pa.convert_z_to_sigma_croco(fs, case["t"], case["z"], case["y"], case["x"], None)
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    rtol = 1e-12  # the float64 class (the points are float64 arrays)
    d = np.abs(got[fin] - want[fin]) / (np.abs(want[fin]) + 1.0)
    print(name, "max |a - b| / (|b| + 1) =", d.max())
    assert np.all(d <= rtol), (name, d.max(), np.flatnonzero(d > rtol)[:8])


@pytest.mark.parametrize("name", HOSTED)
def test_host_recipe_matches_the_reference(gpu, name):
    """a Python kernel that calls convert_z_to_sigma_croco(..., particles) and samples with the result: the host path"""
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    got, err, _, _ = run_croco(case)
    assert err == case["err"]
    assert_matches(got, case["ref"], case, name)


def Count(particles, fieldset):  # a Python function in the list: the loop runs on the host, the built-in kernels as body_only launches
    particles.count = particles.count + 1


@pytest.mark.parametrize("name", ["croco_rect_flat_f64data_f64part", "croco_curv_flat_f32data_f32part", "croco_edges"])
def test_croco_kernels_beside_a_python_kernel_run_on_the_host_path(gpu, name):
    """[AdvectionRK2_3D_CROCO, SampleOmegaCroco, <Python function>]: user kernels are not compiled next to a CROCO kernel, so every
    iteration is one body_only launch of the sigma program; the result is the reference's (the error stop of croco_edges included)"""
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    fs = croco_fieldset(case)
    pclass = pa.get_default_particle(np.float32 if case["spatial_dtype"] == "float32" else np.float64)
    pclass = pclass.add_variable(pa.Variable("omega", dtype=np.float64, initial=0)).add_variable(pa.Variable("count", dtype=np.int32, initial=0))
    n = len(case["x"])
    pset = pa.ParticleSet(fs, pclass=pclass, x=case["x"], y=case["y"], z=case["z"], t=np.zeros(n))
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute([pa.AdvectionRK2_3D_CROCO, pa.SampleOmegaCroco, Count], dt=float(case["dt"]), runtime=float(case["runtime"]))
        except ERRORS as e:
            err = type(e).__name__
    assert err == case["err"]
    got = {k: np.array(v) for k, v in pset._data.items()}
    assert_matches(got, case["ref"], case, name + " (host loop)")
    assert got["count"].max() == (1 if case["err"] else round(case["runtime"] / case["dt"]))


def test_a_float32_variable_receives_the_rounded_sample(gpu):
    """SampleOmegaCroco into a float32 Variable: the float64 run's value, rounded once"""
    case = mg.load(os.path.join(mg.GOLDEN, "croco_rect_flat_f64data_f64part.npz"))
    fs = croco_fieldset(case)
    pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("omega", dtype=np.float32, initial=0))
    n = len(case["x"])
    pset = pa.ParticleSet(fs, pclass=pclass, x=case["x"], y=case["y"], z=case["z"], t=np.zeros(n))
    pset.execute([pa.AdvectionRK2_3D_CROCO, pa.SampleOmegaCroco], dt=float(case["dt"]), runtime=float(case["runtime"]))
    got = np.array(pset._data["omega"])
    assert got.dtype == np.float32
    ref32 = case["ref"]["omega"].astype(np.float32)
    # (the float64 value agrees with the reference's to 1e-12 relative: the rounded one may differ by one float32 ulp at a tie at most)
    assert np.all(np.abs(got.astype(np.float64) - ref32) <= np.spacing(np.abs(ref32)))
    np.testing.assert_array_equal(pset._data["x"], case["ref"]["x"])


VARIANT_CASES = ["croco_rect_flat_f32data_f64part", "croco_curv_flat_f32data_f64part", "croco_edges_delete"]


@pytest.mark.parametrize("name", VARIANT_CASES)
def test_streamed_sorted_and_split_runs_are_bit_identical(gpu, name):
    """the same run with a ring of 3 level slots, cell-sorted, and split into two execute() calls gives the plain run's bits"""
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    case["runtime"] = 7000.0  # across the time levels at 3000 s and 6000 s: a ring of 3 slots has to be refilled behind the clock
    plain, err, _, _ = run_croco(case, sort_by_cell=False)
    variants = {
        "ring of 3 slots": lambda: run_croco(case, fs=croco_fieldset(case).to_windowed_arrays(), sort_by_cell=False),
        "cell-sorted": lambda: run_croco(case, sort_by_cell=True),
        "two execute calls": lambda: run_croco(case, calls=[1200.0, float(case["runtime"]) - 1200.0], sort_by_cell=False),
    }
    for label, run in variants.items():
        got, err2, _, stats = run()
        assert err2 == err, label
        if label.startswith("ring"):
            assert stats["launches"] > 1  # the levels really streamed
        assert stats["program"] == PROG_SIGMA
        order_a, order_b = np.argsort(plain["particle_id"]), np.argsort(got["particle_id"])
        for k in plain:
            np.testing.assert_array_equal(np.asarray(got[k])[order_b], np.asarray(plain[k])[order_a], err_msg=f"{name}: {label}: {k}")


def test_leaving_the_time_interval_raises(gpu):
    """zeta is sampled directly in the reference, so leaving its time interval raises out of the kernel: here the run ends with
    OutsideTimeInterval raised from execute (the particle columns after it are unspecified)"""
    case = mg.load(os.path.join(mg.GOLDEN, "croco_rect_flat_f64data_f64part.npz"))
    case["runtime"] = float(case["coords"]["time"][-1]) + 1000.0
    _, err, _, _ = run_croco(case)
    assert err == "OutsideTimeInterval"


def test_sigma_is_z_over_h_without_stretching(gpu):
    """A known answer that does not come from the reference: with zeta = 0 and Cs_w = s_w,  z0_k = hc s_k + (h - hc) s_k = h s_k up to
    rounding, so sigma = z / h.

    The bound is absolute (sigma lies in [-1, 0]; relative to z / h the error is unbounded near the surface, where z - zvec_zi cancels).
    With u = eps / 2 the unit roundoff: zvec_k = h s_k (1 + d_k) with |d_k| <= 4 u (the roundings of hc s_k, h - hc, (h - hc) s_k and of
    their sum; zeta = 0 adds exact zeros).  Write sigma = s_a + theta (s_b - s_a) with theta = (z - zvec_a) / (zvec_b - zvec_a) in [0, 1]:
    the errors of zvec_a and zvec_b move sigma by at most (1 - theta) |s_a| |d_a| + theta |s_b| |d_b| <= 4 u = 2 eps; the roundings of
    z - zvec_a, s_b - s_a, their product, zvec_b - zvec_a and the quotient are five relative errors u of a term of size <= s_b - s_a <= 1:
    2.5 eps; the final sum and the rounding of the comparison value z / h add 0.5 eps each (|sigma| <= 1).  Total 5.5 eps: asserted as
    8 eps, independent of the level spacing and not fitted to the device's result."""
    coords, fields = mg.croco_output(nx=21, ny=17, nw=9, nt=4, hmin=30.0)
    fields["zeta"] = np.zeros_like(fields["zeta"])
    fields["Cs_w"] = np.array(coords["s_w"], dtype=np.float64)
    case = dict(coords=coords, fields={k: fields[k] for k in ("u", "v", "h", "zeta", "Cs_w")}, mesh="flat", hc=20.0)
    fs = croco_fieldset(case)
    rng = np.random.default_rng(31)
    n = 100_000
    x, y = rng.uniform(0.0, 20000.0, n), rng.uniform(0.0, 16000.0, n)
    t = rng.uniform(0.0, 9000.0, n)
    h = fs.h.eval(t, np.zeros(n), y, x)  # the device's own detached sample of h: the conversion reads exactly this value
    assert h.min() > 20.0
    z = -rng.uniform(0.0, 1.0, n) * h
    sigma = pa.convert_z_to_sigma_croco(fs, t, z, y, x, None)
    err = np.abs(sigma - z / h)
    eps = np.finfo(np.float64).eps
    print("max |sigma - z / h| =", err.max() / eps, "eps")
    assert err.max() <= 8 * eps
