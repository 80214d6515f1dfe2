"""GPU: the kernel list on an unstructured mesh (UxGrid, csrc/pk_ux.h) -- the three diffusion kernels against the fixtures the reference
generated (tools/make_ux_kernels_golden.py), and user-written kernels compiled into the UxGrid step loop (parcels_amd/jit.py) against the
same list in the host loop, bit for bit."""

import glob
import os

import numpy as np
import pytest

import parcels_amd as pa
from case_utils import compare
from parcels_amd import StatusCode
from tools import make_ux_kernels_golden as gk
from ux_kernels_utils import run_uxk
from ux_utils import coordinate_scale, tolerance_for

pytestmark = pytest.mark.gpu

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gk.GOLDEN, "uxk_*.npz")))
PROG_UX = 6  # csrc/pk_ux.h: pk_exec_stats.program of a launch on a UxGrid


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_matches_the_reference(gpu, name):
    case = gk.load(os.path.join(gk.GOLDEN, name + ".npz"))
    ref = case["ref"]
    got, err, rec, pset = run_uxk(case)
    assert err == case["err"], (err, case["err"])
    assert pset._last_stats["program"] == PROG_UX
    tol = tolerance_for(name, case) * coordinate_scale(case)  # 1e-12 of the coordinate scale (float64 particles), 5e-7 of it (float32 particles)
    dev = max(float(np.max(np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64)), initial=0.0)) for k in ("x", "y", "z", "dx", "dy", "dz"))
    identical = all(got[k].tobytes() == ref[k].tobytes() for k in ("x", "y", "z", "dx", "dy", "dz", "t", "state", "ei", "particle_id"))
    print(f"{name}: largest deviation {dev:.3e} (bound {tol:.3e}), bit-identical: {identical}")
    compare(got, ref, rtol=0.0, atol_pos=tol, label=name, skip=("dt",))  # (|got - ref| <= tol; state, ei, t, particle order exactly)
    if case["spatial_dtype"] == "float32":  # float32 storage: z is not advected by the 2-D kernels
        np.testing.assert_array_equal(got["z"], ref["z"])
    if case.get("outputdt"):
        assert rec is not None and "obs_x" in ref and len(rec.obs) == len(ref["obs_time"])
        for k, (time, ids, x, y, z, t) in enumerate(rec.obs):
            assert time == ref["obs_time"][k]
            np.testing.assert_array_equal(ids, ref["obs_particle_id"][k])
            np.testing.assert_array_equal(t, ref["obs_t"][k])
            for a, c in ((x, "x"), (y, "y"), (z, "z")):
                np.testing.assert_allclose(a, ref["obs_" + c][k], rtol=0.0, atol=tol)


# ---- user kernels: the compiled list against the host loop -----------------------------------------------------------------------------
def Age(particles, fieldset):  # noqa: N802  (README.md)
    particles.age += particles.dt
    particles.state = np.where(particles.age > fieldset.max_age, StatusCode.Delete, particles.state)


def SampleT(particles, fieldset):  # noqa: N802  -- node-registered into a float64 Variable, face-registered into a float32 one
    particles.temp = fieldset.Tn[particles]
    particles.tf = fieldset.Tf[particles]


def Upstream(particles, fieldset):  # noqa: N802  -- a sample at a computed point
    u, v = fieldset.UV[particles.t, particles.z, particles.y, particles.x - 0.1, particles]
    particles.dx += u * particles.dt


def Unbeach(particles, fieldset):  # noqa: N802  (README.md: selections of the particles, samples for a selection and at computed points)
    ashore = particles[particles.temp < fieldset.land_value]
    u, v = fieldset.UV[ashore.t, ashore.z, ashore.y, ashore.x - 0.1, ashore]
    ashore.dx -= np.abs(u) * ashore.dt


def DetachedT(particles, fieldset):  # noqa: N802  -- a sample WITHOUT the particles: not translated on a UxGrid
    particles.temp = fieldset.Tn[particles.t, particles.z, particles.y, particles.x]


LISTS = {
    "rk4_age": ([pa.AdvectionRK4, Age], "float64"),
    "rk2_samplet": ([pa.AdvectionRK2, SampleT], "float64"),
    "upstream": ([Upstream], "float32"),  # (a sample at a point computed from float32 columns)
    "rk4_samplet_unbeach": ([pa.AdvectionRK4, SampleT, Unbeach], "float64"),
    "m1_age_delete_f32": ([pa.AdvectionDiffusionM1, Age, pa.DeleteParticle], "float32"),
    "rk4_age_samplet": ([pa.AdvectionRK4, Age, SampleT], "float32"),  # the list of README.md with the default (float32) Particle
}


def _user_case(mesh, n, spatial_dtype, edge=False):
    """the flat / spherical mesh of the fixtures with face-registered U, V, Kh, a node- and a face-registered T; edge: some particles within
    dres of the east edge (their +dres sample finds no face)"""
    base = dict(gk.cases()["uxk_flat_face_em" if mesh == "flat" else "uxk_sph_face_m1"])
    lon, lat, faces = base["node_lon"], base["node_lat"], base["faces"]
    fcx, fcy = lon[faces].mean(axis=1), lat[faces].mean(axis=1)
    two = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None, None, :], 2, 0)  # noqa: E731
    fields = dict(base["fields"])
    fields["Tn"] = (two(10.0 + 0.3 * (lon - lon.min()) - 0.2 * (lat - lat.min())), ("time", "zc", "n_node"))
    fields["Tf"] = (two(5.0 + np.sin(fcx / 3.0) + 0.1 * fcy), ("time", "zc", "n_face"))
    rng = np.random.default_rng(100 + n)
    w, h = lon.max() - lon.min(), lat.max() - lat.min()
    x = lon.min() + rng.uniform(0.2, 0.65, n) * w
    y = lat.min() + rng.uniform(0.2, 0.8, n) * h
    if edge:
        x[: n // 8] = lon.max() - rng.uniform(0.1, 0.9, n // 8) * base["context"]["dres"]
    steps = 10
    return dict(base, fields=fields, x=x, y=y, z=np.full(n, 0.5), spatial_dtype=spatial_dtype, seed=5, runtime=steps * base["dt"],
                outputdt=5 * base["dt"], context=dict(base["context"], max_age=11.5 * base["dt"], land_value=12.0))


def _user_pclass(spatial_dtype):
    P = pa.get_default_particle(np.float32 if spatial_dtype == "float32" else np.float64)  # noqa: N806
    return P.add_variable([pa.Variable("age", dtype=np.float32, initial=0), pa.Variable("temp", dtype=np.float64, initial=0),
                           pa.Variable("tf", dtype=np.float32, initial=0)])


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ux_user_kernel_cache"))  # (one directory for the module: a list is compiled once for both meshes)


def _run_list(case, kernels, monkeypatch, jit):
    monkeypatch.setenv("PARCELS_AMD_JIT", "1" if jit else "0")
    n = len(case["x"])
    age0 = (np.arange(n) % 5).astype(np.float32) * np.float32(case["dt"])  # (so that Age deletes at different steps)
    return run_uxk(case, kernels=kernels, pclass=_user_pclass(case["spatial_dtype"]), age=age0)


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("mesh", ["flat", "spherical"])
@pytest.mark.parametrize("which", list(LISTS))
def test_compiled_list_equals_the_host_loop_to_the_bit(gpu, monkeypatch, jit_cache, which, mesh, n):
    monkeypatch.setenv("PARCELS_AMD_JIT_CACHE", jit_cache)
    kernels, spatial_dtype = LISTS[which]
    case = _user_case(mesh, n, spatial_dtype, edge=which == "m1_age_delete_f32")
    dj, ej, rj, pj = _run_list(case, kernels, monkeypatch, jit=True)
    k = pj._kernel
    assert str(k.jit_report).startswith("compiled"), k.jit_report
    assert k.host_functions == [] and k.user_program is not None and k.user_program.ux
    assert pj._last_stats["program"] == PROG_UX
    dh, eh, rh, ph = _run_list(case, kernels, monkeypatch, jit=False)
    assert ph._kernel.jit_report == "PARCELS_AMD_JIT=0" and ph._kernel.host_functions
    assert ej == eh
    assert sorted(dj) == sorted(dh) and {"age", "temp", "tf"} <= set(dj)
    for col in dj:
        assert dj[col].dtype == dh[col].dtype and dj[col].shape == dh[col].shape, col
        assert dj[col].tobytes() == dh[col].tobytes(), f"{which} on {mesh}: column '{col}' differs at {np.flatnonzero((dj[col] != dh[col]).reshape(len(dj[col]), -1).any(axis=1))[:8]}"
    assert len(rj.obs) == len(rh.obs) >= 1
    for oj, oh in zip(rj.obs, rh.obs):
        assert oj[0] == oh[0]
        for a, b in zip(oj[1:], oh[1:]):
            assert a.tobytes() == b.tobytes()
    assert 0 < len(dj["x"]) <= n
    if "age" in which:  # Age deleted the particles that started old, DeleteParticle those whose +dres sample found no face
        assert len(dj["x"]) < n
    print(f"{which} on {mesh}, n={n}: {len(dj['x'])} particles left, states {sorted(set(dj['state'].tolist()))}, error {ej}")


def test_sample_without_particles_runs_in_the_host_loop(gpu, monkeypatch, jit_cache):
    monkeypatch.setenv("PARCELS_AMD_JIT_CACHE", jit_cache)
    monkeypatch.setenv("PARCELS_AMD_JIT", "1")
    case = _user_case("flat", 65, "float64")
    case = dict(case, outputdt=None)
    d, err, _, pset = run_uxk(case, kernels=[pa.AdvectionRK4, DetachedT], pclass=_user_pclass("float64"))
    k = pset._kernel
    assert err is None and k.user_program is None and k.host_functions == ["DetachedT"]
    assert "UxGrid" in k.jit_report and "without particles" in k.jit_report
    assert np.all(d["state"] == StatusCode.EndofLoop) and np.all(d["t"] == case["runtime"])
    assert np.all(d["temp"] > 0) and len(np.unique(d["temp"])) > 1  # the samples were taken
