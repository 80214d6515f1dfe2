"""GPU: unstructured triangle meshes (UxGrid, csrc/pk_ux.h) against the fixtures the reference generated (tools/make_ux_golden.py), and
properties at full size.  Needs neither the reference nor scipy: the large meshes are NumPy lattices split into triangles."""

import glob
import os
import warnings

import numpy as np
import pytest

import parcels_amd as pa
from case_utils import compare
from tools import make_ux_golden as mg
from ux_utils import coordinate_scale, numpy_f32_trig_differs, run_ux, tolerance_for, ux_fieldset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mg.GOLDEN, "ux_*.npz")))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_matches_the_reference(gpu, name):
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    ref = case["ref"]
    got, err, rec = run_ux(case)
    assert err == case["err"], (err, case["err"])
    rtol = tolerance_for(name, case)
    rep = compare(got, ref, rtol=rtol, atol_pos=rtol * coordinate_scale(case), label=name,
                  skip=("dt",) + (("z", "dz") if case["spatial_dtype"] == "float32" else ()))
    if case["spatial_dtype"] == "float32":  # float32 storage: z is not advected by the 2-D kernels, compare it exactly
        np.testing.assert_array_equal(got["z"], ref["z"])
    if "obs_x" in ref:
        assert rec is not None and len(rec.obs) == len(ref["obs_time"])
        for k, (_, ids, x, y, z, t) in enumerate(rec.obs):
            np.testing.assert_array_equal(ids, ref["obs_particle_id"][k])
            np.testing.assert_array_equal(t, ref["obs_t"][k])
            np.testing.assert_allclose(x, ref["obs_x"][k], rtol=rtol, atol=rtol * coordinate_scale(case))
            np.testing.assert_allclose(y, ref["obs_y"][k], rtol=rtol, atol=rtol * coordinate_scale(case))
    print(name, {k: f"{v:.1e}" for k, v in rep.items()})


def test_uniform_flow_gives_x_8_6(gpu):
    """the reference's tests/test_uxadvection.py: uniform face-registered flow of 0.001 deg/s, 1 h -> x = 8.6"""
    for integ in ("ee", "rk2", "rk4"):
        case = mg.load(os.path.join(mg.GOLDEN, f"ux_flat_uniform_{integ}.npz"))
        got, err, _ = run_ux(case)
        assert err is None
        np.testing.assert_allclose(got["x"], 8.6, atol=1e-5)


@pytest.mark.parametrize("name", [n for n in FIXTURES if mg.with_eval(n)])
def test_field_eval_matches_the_reference(gpu, name):
    """Field.eval / VectorField.eval at scattered points, some outside the mesh (value 0 there), through pk_eval"""
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    ev = case["eval"]
    fs = ux_fieldset(case)
    # points where NumPy's float32 trigonometry of a spherical query is off by an ulp: float32 class (5e-7), every other point 1e-12
    f32 = numpy_f32_trig_differs(ev["y"], ev["x"]) if case["mesh"] == "spherical" else np.zeros(ev["x"].shape, bool)
    rtol = np.where(f32, 5e-7, 1e-12)

    def check(got, want, what):
        scale = np.max(np.abs(want))
        bad = ~(np.abs(got - want) <= rtol * (np.abs(want) + scale))
        assert not bad.any(), f"{what}: {bad.sum()} points differ, first {np.flatnonzero(bad)[:5]} ({got[bad][:3]} vs {want[bad][:3]})"

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fname in case["fields"]:
            check(getattr(fs, fname).eval(ev["t"], ev["z"], ev["y"], ev["x"]), ev["val_" + fname], fname)
        u, v = fs.UV.eval(ev["t"], ev["z"], ev["y"], ev["x"])
    check(u, ev["val_UV_u"], "UV.u")
    check(v, ev["val_UV_v"], "UV.v")
    outside = (ev["x"] < case["node_lon"].min()) | (ev["x"] > case["node_lon"].max()) | (ev["y"] < case["node_lat"].min()) | (ev["y"] > case["node_lat"].max())
    assert outside.any() and np.all(u[outside] == 0)


# ---- properties at full size ------------------------------------------------------------------------------------------------------
N_BIG = 1_000_000


def big_mesh(spherical=False):
    """~1e6 triangles: a 708 x 708 jittered lattice split into two triangles per quad"""
    if spherical:
        return mg.lattice_mesh(708, 708, -40.0, 40.0, -40.0, 40.0, jitter=0.3, seed=11)
    return mg.lattice_mesh(708, 708, 0.0, 70.7, 0.0, 70.7, jitter=0.3, seed=11)


def big_case(fields, lon, lat, faces, time_s=(0.0, 1e6), mesh="flat"):
    return dict(mesh=mesh, node_lon=lon, node_lat=lat, faces=faces, zf=np.array([0.0, 1.0]), zc=np.array([0.5]),
                time_s=np.asarray(time_s, dtype=np.float64), fields=fields)


def test_uniform_face_flow_gives_exact_displacement_at_full_size(gpu):
    lon, lat, faces = big_mesh()
    nf, nt = faces.shape[0], 2
    case = big_case({"U": (np.full((nt, 1, nf), 0.002), ("time", "zc", "n_face")), "V": (np.full((nt, 1, nf), -0.001), ("time", "zc", "n_face"))},
                    lon, lat, faces)
    fs = ux_fieldset(case)
    rng = np.random.default_rng(1)
    x0, y0 = rng.uniform(5.0, 60.0, N_BIG), rng.uniform(15.0, 65.0, N_BIG)
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x0, y=y0, z=np.full(N_BIG, 0.5), t=np.zeros(N_BIG))
    pset.execute(pa.AdvectionRK4, dt=300.0, runtime=3600.0)
    x, y = x0.copy(), y0.copy()
    for _ in range(12):  # _advection.py:42-75 with u1 = u2 = u3 = u4, then the position update
        x = x + (0.002 + 2 * 0.002 + 2 * 0.002 + 0.002) / 6.0 * 300.0
        y = y + (-0.001 + 2 * -0.001 + 2 * -0.001 + -0.001) / 6.0 * 300.0
    np.testing.assert_array_equal(pset.x, x)
    np.testing.assert_array_equal(pset.y, y)
    assert np.all(pset.state == pa.StatusCode.EndofLoop)


def test_linear_node_field_reproduces_a_linear_function(gpu):
    """UxLinearNode*: barycentric interpolation of a + b x + c y is a + b x + c y (the idea of the reference's test_icon_evals).  A search
    without a guess takes its barycentric coordinates from the hash query's float32 buffer (spatialhash.py:511), so the reproduction
    is exact to float32 rounding of the weights: 1e-6 relative."""
    lon, lat, faces = big_mesh()
    a, b, c = 3.0, 0.25, -0.5
    P = np.repeat((a + b * lon + c * lat)[None, None, :], 2, 0)
    Pz = np.repeat(np.stack([a + b * lon + c * lat, 2 * (a + b * lon + c * lat)])[None], 2, 0)
    case = big_case({"U": (np.zeros((2, 1, faces.shape[0])), ("time", "zc", "n_face")), "V": (np.zeros((2, 1, faces.shape[0])), ("time", "zc", "n_face")),
                     "P": (P, ("time", "zc", "n_node")), "Q": (Pz, ("time", "zf", "n_node"))}, lon, lat, faces)
    fs = ux_fieldset(case)
    rng = np.random.default_rng(2)
    x, y = rng.uniform(1.0, 69.0, N_BIG), rng.uniform(1.0, 69.0, N_BIG)
    z = rng.uniform(0.0, 1.0, N_BIG)
    t = np.full(N_BIG, 10.0)
    want = a + b * x.astype(np.float32).astype(np.float64) + c * y.astype(np.float32).astype(np.float64)  # the search runs on float32 positions
    got = fs.P.eval(t, z, y, x)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(fs.Q.eval(t, z, y, x), want * (1.0 + z), rtol=1e-6, atol=1e-6)


def test_face_field_is_constant_per_face(gpu):
    lon, lat, faces = big_mesh(spherical=True)
    nf = faces.shape[0]
    vals = np.random.default_rng(3).standard_normal(nf)
    case = big_case({"U": (np.zeros((2, 1, nf)), ("time", "zc", "n_face")), "V": (np.zeros((2, 1, nf)), ("time", "zc", "n_face")),
                     "F": (np.repeat(vals[None, None, :], 2, 0), ("time", "zc", "n_face"))}, lon, lat, faces, mesh="spherical")
    fs = ux_fieldset(case)
    rng = np.random.default_rng(4)
    x, y = rng.uniform(-39.0, 39.0, N_BIG), rng.uniform(-39.0, 39.0, N_BIG)
    z = np.full(N_BIG, 0.5)
    got = fs.F.eval(np.zeros(N_BIG), z, y, x)
    eng = fs._engine_or_create()
    ei = eng.search(0, z, y, x)
    found = ei >= 0  # (a point of the sphere just outside the xyz boxes of its face's nodes is not found: GRID_SEARCH_ERROR, value 0)
    assert found.mean() > 0.999
    np.testing.assert_array_equal(got[found], vals[ei[found] % nf])
    np.testing.assert_array_equal(got[~found], 0.0)


def test_streamed_levels_equal_resident_levels(gpu):
    """nslots < nt (a ring of levels refilled behind the clock) gives exactly what a fully resident fieldset gives"""
    lon, lat, faces = mg.lattice_mesh(120, 120, 0.0, 20.0, 0.0, 20.0, jitter=0.3, seed=9)
    fcx, fcy = mg.face_centres(lon, lat, faces)
    nt = 8
    U = np.stack([0.01 + 0.002 * k + 0.0005 * np.sin(fcy + k) for k in range(nt)])[:, None, :]
    V = np.stack([0.005 * np.cos(fcx - k) for k in range(nt)])[:, None, :]
    case = big_case({"U": (U, ("time", "zc", "n_face")), "V": (V, ("time", "zc", "n_face"))}, lon, lat, faces, time_s=np.arange(nt) * 100.0)
    rng = np.random.default_rng(5)
    x, y = rng.uniform(3.0, 8.0, 100_000), rng.uniform(3.0, 17.0, 100_000)
    out = []
    for nslots in (None, 3):
        fs = ux_fieldset(case, nslots=nslots)
        pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x, y=y, z=np.full(x.size, 0.5), t=np.zeros(x.size))
        pset.execute(pa.AdvectionRK4, dt=10.0, runtime=650.0)
        out.append({k: np.array(pset._data[k]) for k in ("x", "y", "t", "state", "ei")})
    assert fs._engine.windowed
    for k in out[0]:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
