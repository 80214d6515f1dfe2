"""CPU: the unstructured-mesh (UxGrid) host side -- API, validation, interpolator selection, the triangle hash table, the C ABI mirror and
the fixtures of tools/make_ux_golden.py against the live reference."""

import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import parcels_amd as pa
from oracle import ref_shim
from tools import make_ux_golden as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mg.GOLDEN, "ux_*.npz")))
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference sources not present")


def _fixture(name):
    return mg.load(os.path.join(mg.GOLDEN, name + ".npz"))


def ux_dataset(case):
    """parcels_amd.Dataset of a fixture: the mesh, time / zf / zc coordinates and the fields with their UGRID dims"""
    mesh = pa.UxMesh(case["node_lon"], case["node_lat"], case["faces"])
    coords = {"time": (("time",), np.asarray(case["time_s"], dtype=np.float64)), "zf": (("zf",), case["zf"]), "zc": (("zc",), case["zc"])}
    return pa.Dataset({n: (dims, arr) for n, (arr, dims) in case["fields"].items()}, coords, uxgrid=mesh)


def test_fixtures_exist_and_are_small():
    assert len(FIXTURES) >= 15
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(mg.GOLDEN, n + ".npz")) < 1 << 20, n


def test_from_ugrid_conventions_builds_a_uxgrid_fieldset():
    case = _fixture("ux_flat_3d_rk4")
    fs = pa.FieldSet.from_ugrid_conventions(ux_dataset(case), mesh="flat")
    g = fs.U.grid
    assert isinstance(g, pa.UxGrid)
    assert g.axes == ["Z", "FACE"]
    assert g.get_axis_dim("Z") == 4 and g.get_axis_dim("FACE") == case["faces"].shape[0]
    assert g.deg2m == 1.0
    np.testing.assert_array_equal(g.depth, case["zf"])
    assert isinstance(fs.UV.interp_method, pa.Ux_Velocity) and isinstance(fs.UVW.interp_method, pa.Ux_Velocity)
    assert isinstance(fs.U.interp_method, pa.UxConstantFaceConstantZC)
    assert isinstance(fs.W.interp_method, pa.UxLinearNodeLinearZF)
    # ravel over (Z, FACE), basegrid.py:83-152
    ei = g.ravel_index({"Z": np.array([0, 2]), "FACE": np.array([5, 7])})
    np.testing.assert_array_equal(ei, [5, 2 * g.get_axis_dim("FACE") + 7])
    back = g.unravel_index(ei)
    np.testing.assert_array_equal(back["Z"], [0, 2])
    np.testing.assert_array_equal(back["FACE"], [5, 7])
    with pytest.raises(ValueError, match="Axis 'X' is not part of this grid"):
        g.get_axis_dim("X")
    sph = pa.FieldSet.from_ugrid_conventions(ux_dataset(_fixture("ux_sph_node_rk4_3d")))  # mesh="spherical" is the default
    assert sph.U.grid.deg2m == pytest.approx(1852 * 60)


def test_particleset_default_z_is_the_top_interface():
    fs = pa.FieldSet.from_ugrid_conventions(ux_dataset(_fixture("ux_flat_3d_rk4")), mesh="flat")
    pset = pa.ParticleSet(fs, x=[5.0, 6.0], y=[5.0, 6.0])
    np.testing.assert_array_equal(pset.z, [0.0, 0.0])


def test_validation_messages():
    case = _fixture("ux_flat_uniform_rk4")
    # uxgrid.py:39
    quad = pa.UxMesh(np.arange(4.0), np.arange(4.0), np.array([[0, 1, 2, 3]]))
    with pytest.raises(ValueError, match=r"must contain only triangular cells \(n_max_face_nodes=3\)"):
        pa.UxGrid(quad, np.array([0.0, 1.0]), "flat")
    with pytest.raises(ValueError, match="z must be a 1D array of vertical coordinates"):
        pa.UxGrid(pa.UxMesh(case["node_lon"], case["node_lat"], case["faces"]), np.zeros((2, 2)), "flat")
    # model.py:361-370
    ds = ux_dataset(case)
    del ds.coords["zf"]
    with pytest.raises(ValueError, match="Dataset missing one of the required dimensions 'time', 'zf', or 'zc' for uxDataset"):
        pa.FieldSet.from_ugrid_conventions(ds, mesh="flat")
    # model.py:480-500
    ds = ux_dataset(case)
    ds["P"] = (("time", "zc", "n_face", "extra"), np.zeros((2, 1, case["faces"].shape[0], 2)))
    with pytest.raises(ValueError, match="Fields on unstructured grids must have two spatial dimensions"):
        pa.FieldSet.from_ugrid_conventions(ds, mesh="flat")
    # U without V (model.py: _discover_ux_U_and_V)
    ds = ux_dataset(case)
    del ds.data_vars["V"]
    with pytest.raises(ValueError, match="Dataset has only one of the two variables 'U' and 'V'"):
        pa.FieldSet.from_ugrid_conventions(ds, mesh="flat")


@needs_reference
def test_validation_message_matches_the_reference():
    m, DA = mg.reference()  # noqa: N806
    lon, lat, faces = mg.lattice_mesh(3, 3, 0.0, 1.0, 0.0, 1.0)
    quad = mg.RefMesh(DA, lon, lat, np.concatenate([faces, faces[:, :1]], axis=1))
    with pytest.raises(ValueError) as ref:
        m["uxgrid"].UxGrid(quad, DA(np.array([0.0, 1.0]), dims=("zf",)), "flat")
    with pytest.raises(ValueError) as ours:
        pa.UxGrid(pa.UxMesh(lon, lat, np.concatenate([faces, faces[:, :1]], axis=1)), np.array([0.0, 1.0]), "flat")
    assert str(ours.value) == str(ref.value)


def test_common_ugrid_variable_names_are_discovered():
    case = _fixture("ux_flat_uniform_rk4")
    ds = ux_dataset(case)
    ds.data_vars = {{"U": "u", "V": "v"}[k]: v for k, v in ds.data_vars.items()}
    fs = pa.FieldSet.from_ugrid_conventions(ds, mesh="flat")
    assert "UV" in fs.fields and fs.U.name == "U"


def test_interpolator_selection_by_dims():
    from parcels_amd.uxgrid import select_uxinterpolator

    table = {("zc", "n_face"): pa.UxConstantFaceConstantZC, ("zc", "n_node"): pa.UxLinearNodeConstantZC,
             ("zf", "n_node"): pa.UxLinearNodeLinearZF, ("zf", "n_face"): pa.UxConstantFaceLinearZF}
    for (v, lat), cls in table.items():
        assert select_uxinterpolator(pa.DataArray(("time", v, lat), np.zeros((1, 1, 1)))) is cls
        assert select_uxinterpolator(pa.DataArray((lat, v), np.zeros((1, 1)))) is cls  # order does not matter, time is optional
    assert select_uxinterpolator(pa.DataArray(("time", "zc", "n_edge"), np.zeros((1, 1, 1)))) is None
    with pytest.raises(ValueError, match="two spatial dimensions"):
        select_uxinterpolator(pa.DataArray(("time", "n_face"), np.zeros((1, 1))))
    assert [c.kind for c in (pa.UxConstantFaceConstantZC, pa.UxConstantFaceLinearZF, pa.UxLinearNodeConstantZC, pa.UxLinearNodeLinearZF,
                             pa.Ux_Velocity)] == [5, 6, 7, 8, 4]  # include/parcels_hip.h: is_const 5-8, interp_uv 4


@needs_reference
def test_interpolator_selection_matches_the_reference():
    try:
        import importlib

        mg.reference()
        model = importlib.import_module("parcels._core.model")
    except Exception as e:  # model.py needs more of xarray than the shim stands in for
        pytest.skip(f"parcels._core.model not importable under the shim: {e}")
    from parcels_amd.uxgrid import select_uxinterpolator

    for dims in (("time", "zc", "n_face"), ("time", "zc", "n_node"), ("time", "zf", "n_node"), ("time", "zf", "n_face"), ("time", "zf", "n_edge")):
        ref = model._select_uxinterpolator(ref_shim.DA(np.zeros((1, 1, 1)), dims=dims))
        ours = select_uxinterpolator(pa.DataArray(dims, np.zeros((1, 1, 1))))
        assert (ref.__name__ if ref else None) == (ours.__name__ if ours else None), dims


@pytest.mark.parametrize("name", FIXTURES)
def test_hash_table_equals_the_reference(name):
    """SpatialHash.from_triangles gives the reference's table (keys, starts, counts, faces, bitwidth, bounds) for every fixture mesh"""
    case = _fixture(name)
    h = pa.spatialhash.SpatialHash.from_triangles(case["node_lon"], case["node_lat"], case["faces"], case["mesh"] == "spherical")
    assert h.checksum() == case["hash_checksum"]


def test_kernels_without_a_uxgrid_form_raise():
    fs = pa.FieldSet.from_ugrid_conventions(ux_dataset(_fixture("ux_flat_uniform_rk4")), mesh="flat")
    pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("next_dt", dtype=np.float64, initial=1.0))
    pset = pa.ParticleSet(fs, pclass=pclass, x=[5.0], y=[5.0])
    with pytest.raises(NotImplementedError, match="AdvectionRK45 is not implemented on a UxGrid"):
        pset.execute(pa.AdvectionRK45, dt=1.0, runtime=1.0)
    with pytest.raises(NotImplementedError, match="SubmergeParticle is not implemented on a UxGrid"):
        pset.execute([pa.AdvectionRK4, pa.SubmergeParticle], dt=1.0, runtime=1.0)


def test_ctypes_mirror_of_pk_ugrid_desc(tmp_path):
    from parcels_amd import _hip

    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "parcels_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu\\n", sizeof(pk_ugrid_desc), offsetof(pk_ugrid_desc, h_nkeys), offsetof(pk_ugrid_desc, h_bbox));'
                   "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_nkeys, off_bbox = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert C.sizeof(_hip.UGridDesc) == size
    assert _hip.UGridDesc.h_nkeys.offset == off_nkeys and _hip.UGridDesc.h_bbox.offset == off_bbox
    assert "pk_ugrid_create" in _hip.ABI_SYMBOLS


@needs_reference
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_regenerates_from_the_reference(name):
    """tools/make_ux_golden.py run on the live reference gives the committed arrays"""
    arrs = mg.generate(name, mg.cases()[name])
    with np.load(os.path.join(mg.GOLDEN, name + ".npz"), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(arrs)
        for k in z.files:
            assert np.array_equal(z[k], arrs[k], equal_nan=z[k].dtype.kind == "f"), (name, k)
