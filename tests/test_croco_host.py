"""CPU: the CROCO sigma-grid surface -- fixtures, croco_to_sgrid, kernel tokens and ids, validation at Kernel construction."""

import glob
import os
import re
import types

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import kernels as K
from parcels_amd.kernel import Kernel
from tools import make_croco_golden as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(mg.GOLDEN, "croco_*.npz")))
REQUIRED = ["croco_rect_flat_f64data_f64part", "croco_rect_flat_f64data_f32part", "croco_rect_flat_f32data_f64part", "croco_rect_flat_f32data_f32part",
            "croco_curv_flat_f32data_f64part", "croco_curv_flat_f32data_f32part", "croco_rect_sph_f64", "croco_edges", "croco_edges_delete",
            "croco_backward", "croco_outputdt", "croco_rk2_2d", "croco_sample_tracer", "croco_sigma_points", "croco_host_recipe",
            "croco_curv_flat_f64data_f64part", "croco_curv_sph_f32data_f64part", "croco_agrid_rect_f64", "croco_agrid_curv_f32", "croco_two_levels",
            "croco_many_levels", "croco_three_waves"]


def croco_dataset(coords, fields):
    two_d = np.asarray(coords["x_rho"]).ndim == 2
    co = {"x_rho": (("eta_rho", "xi_rho") if two_d else ("xi_rho",), coords["x_rho"]),
          "y_rho": (("eta_rho", "xi_rho") if two_d else ("eta_rho",), coords["y_rho"]),
          "s_w": (("s_w",), coords["s_w"]), "time": (("time",), np.asarray(coords["time"], dtype=np.float64))}
    return pa.convert.croco_to_sgrid(fields={mg.FIELD_NAMES.get(k, k): (mg.CROCO_DIMS[k], a) for k, a in fields.items()}, coords=co), co


def croco_fs(use=("u", "v", "w", "omega", "h", "zeta", "Cs_w"), hc=20.0, dtype=np.float64, **change):
    coords, fields = mg.croco_output(dtype=dtype)
    fields = {k: fields[k] for k in use}
    fields.update(change)
    ds, _ = croco_dataset(coords, fields)
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="flat")
    if hc is not None:
        fs.add_context("hc", hc)
    return fs


def kernel_of(fs, funcs, variables=("omega",), dtype=np.float64):
    pclass = pa.get_default_particle(np.float64)
    for v in variables:
        pclass = pclass.add_variable(pa.Variable(v, dtype=dtype, initial=0))
    return Kernel(list(funcs), types.SimpleNamespace(fieldset=fs, _pclass=pclass))


def test_every_required_fixture_is_there():
    names = {os.path.basename(p)[:-4] for p in FIXTURES}
    assert set(REQUIRED) <= names, sorted(set(REQUIRED) - names)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_loads_and_holds_only_arrays(path):
    assert os.path.getsize(path) < 1024 * 1024
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            assert z[k].dtype != object, k
    case = mg.load(path)
    assert case["name"] == os.path.basename(path)[:-4]
    assert {"h", "zeta", "Cs_w", "u", "v"} <= set(case["fields"])
    assert float(np.min(case["fields"]["h"])) > 0
    if case.get("kind") == "sigma_points":
        assert len(case["ref"]["sigma"]) == len(case["x"]) >= 200
    else:
        assert len(case["x"]) >= 40 and abs(case["runtime"] / case["dt"]) >= 30
        assert len(case["coords"]["time"]) >= 3 and np.ptp(case["fields"]["zeta"], axis=0).max() > 0


def test_one_fixture_has_a_bathymetry_shallower_than_hc():
    cases = [mg.load(p) for p in FIXTURES]
    assert any(float(np.min(c["fields"]["h"])) < c["hc"] for c in cases)
    assert any(float(np.min(c["fields"]["h"])) > c["hc"] for c in cases)


def test_croco_to_sgrid_names_dims_paddings_and_offsets():
    coords, fields = mg.croco_output()
    ds, _ = croco_dataset(coords, fields)
    assert {"lon", "lat", "depth", "time"} <= set(ds.coords) and "x_rho" not in ds and "s_w" not in ds.coords
    assert ds["depth"].dims == ("depth",) and ds["W"].dims == ("time", "depth", "eta_rho", "xi_rho")
    assert ds["U"].dims == ("time", "s_rho", "eta_rho", "xi_u") and ds["V"].dims == ("time", "s_rho", "eta_v", "xi_rho")
    assert ds["Cs_w"].dims == ("depth",) and ds["h"].dims == ("eta_rho", "xi_rho")
    assert np.issubdtype(ds["time"].data.dtype, np.timedelta64)
    np.testing.assert_array_equal(ds["time"].data / np.timedelta64(1, "s"), coords["time"])
    md = ds.sgrid
    fx, fy = md.face_dimensions
    assert (fx.face, fx.node, fx.padding) == ("xi_u", "xi_rho", pa.Padding.HIGH)
    assert (fy.face, fy.node, fy.padding) == ("eta_v", "eta_rho", pa.Padding.HIGH)
    fz = md.vertical_dimensions[0]
    assert (fz.face, fz.node, fz.padding) == ("s_rho", "depth", pa.Padding.HIGH)
    assert md.node_coordinates == ("lon", "lat")
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="flat")
    assert fs.U.grid.offsets() == {"X": 0, "Y": 0, "Z": 0}
    assert isinstance(fs.UV.interp_method, pa.CGrid_Velocity) and isinstance(fs.UVW.interp_method, pa.CGrid_Velocity)
    for name in ("U", "V", "W", "omega", "temp", "h", "zeta", "Cs_w"):
        assert isinstance(fs.fields[name].interp_method, pa.XLinear), name
    assert len(fs.gridset) == 1 and fs.U.grid.axes == ["Z", "Y", "X"]
    np.testing.assert_array_equal(fs.U.grid.depth, coords["s_w"])


def test_croco_to_sgrid_time_units_and_dataset_input():
    coords, fields = mg.croco_output()
    _, co = croco_dataset(coords, fields)
    co["time"] = (("time",), np.array([0.0, 1.0, 2.0, 3.0]), {"units": "hours since start"})
    ds = pa.convert.croco_to_sgrid(fields={"h": pa.Dataset({"h": (mg.CROCO_DIMS["h"], fields["h"])})}, coords=pa.Dataset({}, co))
    np.testing.assert_array_equal(ds["time"].data / np.timedelta64(1, "s"), [0.0, 3600.0, 7200.0, 10800.0])
    assert ds["h"].dims == ("eta_rho", "xi_rho")


@pytest.mark.parametrize("missing", ["x_rho", "y_rho", "s_w", "time"])
def test_croco_to_sgrid_names_a_missing_coordinate(missing):
    coords, fields = mg.croco_output()
    _, co = croco_dataset(coords, fields)
    del co[missing]
    with pytest.raises(ValueError, match=re.escape(f"Expected coordinate '{missing}' not found in provided coords dataset.")):
        pa.convert.croco_to_sgrid(fields={"h": (mg.CROCO_DIMS["h"], fields["h"])}, coords=co)


def test_kernel_ids_names_and_exports():
    assert K.kernel_id(pa.AdvectionRK2_3D_CROCO) == 11 and K.kernel_id(pa.SampleOmegaCroco) == 12
    tok = pa.SampleFieldCroco("temp", into="tracer")
    assert K.kernel_id(tok) == 12 and tok.__name__ == "SampletempCroco" and tok._pk_sample_sigma == ("temp", "tracer")
    assert pa.AdvectionRK2_3D_CROCO.__name__ == "AdvectionRK2_3D_CROCO" and pa.SampleOmegaCroco.__name__ == "SampleOmegaCroco"
    assert pa.SampleOmegaCroco._pk_sample_sigma == ("omega", "omega")
    for name in ("AdvectionRK2_3D_CROCO", "SampleOmegaCroco", "SampleFieldCroco", "convert_z_to_sigma_croco"):
        assert name in K.__all__ and getattr(pa, name) is getattr(K, name)
    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    assert re.search(r"#define PK_KERNEL_ADVECTION_RK2_3D_CROCO 11\b", header) and re.search(r"#define PK_KERNEL_SAMPLE_SIGMA_CROCO 12\b", header)
    with pytest.raises(RuntimeError, match="device kernel"):
        pa.AdvectionRK2_3D_CROCO(None, None)
    with pytest.raises(TypeError):
        pa.SampleFieldCroco("omega", into=("a", "b"))


def test_a_complete_croco_list_is_accepted():
    fs = croco_fs()
    k = kernel_of(fs, [pa.AdvectionRK2_3D_CROCO, pa.SampleOmegaCroco, pa.DeleteParticle])
    assert k.kernel_ids == [11, 12, 20] and k.samples == {1: ("omega", 0)} and k.device_variables == ["omega"] and not k.host_functions


@pytest.mark.parametrize("drop", ["h", "zeta", "Cs_w"])
def test_a_missing_croco_field_is_named_at_construction(drop):
    fs = croco_fs(use=[f for f in ("u", "v", "w", "omega", "h", "zeta", "Cs_w") if f != drop])
    for funcs in ([pa.AdvectionRK2_3D_CROCO], [pa.AdvectionRK2, pa.SampleOmegaCroco]):
        with pytest.raises(ValueError, match=rf"needs the field {drop}\b"):
            kernel_of(fs, funcs)


def test_missing_hc_w_field_and_variable_are_named():
    with pytest.raises(ValueError, match="add_context\\('hc'"):
        kernel_of(croco_fs(hc=None), [pa.AdvectionRK2_3D_CROCO])
    with pytest.raises(ValueError, match="needs a W field"):
        kernel_of(croco_fs(use=("u", "v", "omega", "h", "zeta", "Cs_w")), [pa.AdvectionRK2_3D_CROCO])
    with pytest.raises(ValueError, match="'salt' is not a scalar field"):
        kernel_of(croco_fs(), [pa.SampleFieldCroco("salt", into="omega")])
    with pytest.raises(ValueError, match="no user Variable 'omega'"):
        kernel_of(croco_fs(), [pa.SampleOmegaCroco], variables=())
    with pytest.raises(ValueError, match="must be float32 or float64"):
        kernel_of(croco_fs(), [pa.SampleOmegaCroco], dtype=np.int32)


def test_cs_w_must_be_the_depth_axis():
    coords, fields = mg.croco_output()
    ds, _ = croco_dataset(coords, {k: fields[k] for k in ("u", "v", "w", "omega", "h", "zeta")})
    ds["Cs_w"] = (("eta_rho",), np.linspace(-1.0, 0.0, fields["h"].shape[0]))
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="flat")
    fs.add_context("hc", 20.0)
    with pytest.raises(ValueError, match="Cs_w must be a field whose only non-singleton axis is the depth axis"):
        kernel_of(fs, [pa.AdvectionRK2_3D_CROCO])


def test_mixed_dtypes_are_refused_by_name():
    coords, fields = mg.croco_output()
    fs = croco_fs(zeta=fields["zeta"].astype(np.float32))
    with pytest.raises(NotImplementedError, match="field zeta is float32"):
        kernel_of(fs, [pa.AdvectionRK2_3D_CROCO])


def test_unsupported_configurations_are_refused_at_construction():
    fs = croco_fs()
    fs.UV.interp_method = pa.XFreeslip()
    with pytest.raises(NotImplementedError, match="XLinear_Velocity or CGrid_Velocity"):
        kernel_of(fs, [pa.AdvectionRK2_3D_CROCO])
    coords, fields = mg.croco_output()
    coords["x_rho"] = coords["x_rho"].astype(np.float32)
    ds, _ = croco_dataset(coords, {k: fields[k] for k in ("u", "v", "w", "omega", "h", "zeta", "Cs_w")})
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="flat")
    fs.add_context("hc", 20.0)
    with pytest.raises(NotImplementedError, match="float64 coordinate arrays"):
        kernel_of(fs, [pa.SampleOmegaCroco])
    coords, fields = mg.croco_output()
    ds, _ = croco_dataset(coords, {k: fields[k] for k in ("u", "v", "w", "omega", "zeta", "Cs_w")})
    ds["h"] = (("time", "eta_rho", "xi_rho"), np.repeat(fields["h"][None], 4, 0))
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="flat")
    fs.add_context("hc", 20.0)
    with pytest.raises(NotImplementedError, match="time-varying bathymetry"):
        kernel_of(fs, [pa.AdvectionRK2_3D_CROCO])


def test_abi_lists_the_croco_entry_points():
    from parcels_amd import _hip

    assert {"pk_set_croco", "pk_sigma_croco"} <= set(_hip.ABI_SYMBOLS) and _hip.PK_ABI_VERSION == 9
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pk_set_croco" in text and "pk_sigma_croco" in text
