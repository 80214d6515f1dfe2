"""GPU: user kernels that sample NAMED vector fields (`fieldset.Wind[particles]`, `fieldset.UVstokes[...]`, `fieldset.Disp[t, z, y, x - 0.1,
ashore]`) compiled into the fused step loop.  Every case runs as one compiled list in the kernel-list interpreter, matches the fixture the
reference's own ParticleSet.execute wrote (tools/make_named_vector_golden.py) in the project's tolerance classes -- state, `ei` of every
grid, t and the particle order exactly --, and gives bit for bit the columns of the same run on the host path (PARCELS_AMD_JIT=0)."""
import warnings

import numpy as np
import pytest

import named_vector_kernels as nk
import named_vector_utils as nu
import parcels_amd as pa
from case_utils import compare, tolerance_for

pytestmark = pytest.mark.gpu
SPECS = nu.all_cases()
PROG_GENERIC = 2  # include/parcels_hip.h: pk_exec_stats.program -- the kernel-list interpreter
_runs = {}


def _run(name, jit=True, nslots=None):
    key = (name, jit, nslots)
    if key not in _runs:
        _runs[key] = nu.run_case(SPECS[name], jit=jit, nslots=nslots)
    return _runs[key]


def _check(name, *, nslots=None, host_path=True):
    """The compiled run of a case against its fixture and against the host path; returns the compiled run."""
    spec = SPECS[name]
    pset, got, err = _run(name, nslots=nslots)
    k = pset._kernel
    assert k.jit_report.startswith("compiled") and k.host_functions == [], k.jit_report
    prog = k.user_program
    assert prog.vectors and "PK_USER_VECTORS" in prog.source and not prog.flags & 1
    assert pset._last_stats["program"] == PROG_GENERIC and not pset._last_stats.get("hosted"), pset._last_stats
    ref, rerr = nu.load_fixture(name)
    assert err == rerr, (err, rerr)  # (the reference's exception classes and this project's share their names)
    assert got["ei"].shape == ref["ei"].shape and got["ei"].shape[1] == (2 if spec.get("second") else 1)
    compare(got, ref, rtol=tolerance_for(name, spec["currents"]), check_state="all", label=name, skip=())
    if not host_path:
        return pset, got
    ph, host, herr = _run(name, jit=False, nslots=nslots)
    assert ph._kernel.user_program is None and ph._kernel.jit_report == "PARCELS_AMD_JIT=0" and herr == err
    assert set(host) == set(got)
    for c in got:
        assert got[c].dtype == host[c].dtype and np.array_equal(got[c], host[c], equal_nan=True), (name, c, np.flatnonzero(got[c] != host[c])[:5])
    return pset, got


@pytest.mark.parametrize("name", ["nv_a_adv_wind", "nv_a_wind_adv"])
def test_a_documented_wind_example(gpu, name):
    _check(name)
    a, b = _run("nv_a_adv_wind")[1], _run("nv_a_wind_adv")[1]
    for c in a:  # either order of the two kernels adds the same two displacements
        assert np.array_equal(a[c], b[c], equal_nan=True), c


@pytest.mark.parametrize("name", ["nv_b_stokes_65", "nv_b_stokes_2"])
def test_b_stokes_drift_from_a_second_fieldset(gpu, name):
    """currents on the curvilinear C-grid, `fs + fs2` with the Stokes drift on a small rectilinear grid with another time axis"""
    pset, got = _check(name)
    assert len(pset.fieldset.gridset) == 2 and pset.fieldset.UVstokes.igrid == 1
    assert np.any(got["ei"][:, 1] != 0) and np.any(got["ei"][:, 0] != 0)
    assert pset._kernel.user_program.vectors[0][0] == "UVstokes" and pset._kernel.user_program.vectors[0][5] == 0  # rectilinear, next to a curvilinear main grid


def test_c_three_components_next_to_rk4_3d(gpu):
    pset, got = _check("nv_c_three")
    assert pset._kernel.user_program.vectors[0][3] >= 0 and np.any(got["w2"] != 0) and np.any(got["u2"] != 0)


@pytest.mark.parametrize("name", ["nv_d_f32_65", "nv_d_f32_2"])
def test_d_float32_particles(gpu, name):
    pset, got = _check(name)
    assert got["x"].dtype == np.float32 and pset._kernel.user_program.vectors[0][4] == "float"


def test_e_unbeaching_a_selection_at_shifted_points(gpu):
    pset, got = _check("nv_e_unbeach")
    assert pset._kernel.user_program.sources[0].counter is not None  # a conditional sample: the kernel keeps its own stage counter
    assert 0 < np.count_nonzero(got["beached"]) < len(got["beached"])


def test_f_leaving_the_wind_grid(gpu):
    pset, got = _check("nv_f_leaves")
    assert got["state"][0] == pa.StatusCode.ErrorOutOfBounds and np.count_nonzero(got["state"] >= 50) == 1
    lon = np.asarray(pset.fieldset.U.grid.lon)
    assert lon[0] < got["x"][0] < lon[-1]  # still inside the currents' grid
    pset, got = _check("nv_f_leaves_delete")
    assert len(got["x"]) == 64 and 0 not in got["particle_id"] and np.all(got["state"] < 50)


def test_g_wind_time_axis_ends_before_the_run(gpu):
    pset, got = _check("nv_g_wind_ends")
    assert np.all(got["state"] == pa.StatusCode.ErrorOutsideTimeInterval)


def test_h_levels_streaming_through_a_ring_of_two(gpu):
    """the wind's levels (every 2 h, its own time axis) bound the resident window more tightly than the currents' (every 4 h); the host
    loop calls the library launch by launch and streams nothing, so the ring is compared with the resident run (which is compared with
    the host path)"""
    _check("nv_h_stream")
    pset, got = _check("nv_h_stream", nslots=2, host_path=False)
    eng = pset.fieldset._engine
    assert eng.windowed and eng.field_nslots["UWind"] == 2 and eng.field_nslots["U"] == 2 and pset._last_stats["launches"] > 1
    resident = _run("nv_h_stream")[1]
    for c in got:
        assert np.array_equal(got[c], resident[c], equal_nan=True), c


def test_j_cgrid_wind_on_the_curvilinear_main_grid(gpu):
    """CGrid_Velocity for a named vector: staggered components packed on the device, on the curvilinear grid the currents use (the
    lane's cache of the currents' staggered values must not answer for the wind)"""
    pset, got = _check("nv_j_cgrid_wind")
    v = pset._kernel.user_program.vectors[0]
    assert v[5] == 1 and v[6] == 1 and "eval_vec<double, 1, 1>" in pset._kernel.user_program.source
    eng = pset.fieldset._engine
    assert eng.pack_leader_of.get("UWind") is not None and eng.pack_leader_of.get("UWind") == eng.pack_leader_of.get("VWind")


@pytest.mark.parametrize("slip,kind", [("free", 2), ("partial", 3)])
def test_k_wind_with_a_slip_interpolator(gpu, slip, kind):
    pset, got = _check(f"nv_k_{slip}slip")
    assert pset._kernel.user_program.vectors[0][6] == kind and f"eval_vec<double, 0, 2>(a, mc, c, " in pset._kernel.user_program.source
    other = _run("nv_k_partialslip" if slip == "free" else "nv_k_freeslip")[1]
    assert not np.array_equal(got["x"], other["x"])  # (the literal interp_uv tells the two apart)


def test_l_time_axis_ends_for_some_particles_of_a_view(gpu):
    """releases 2700 s apart, dt 3600 s: in the iteration with the early releases at 10800 s and the late ones at 13500 s the midpoint sample
    (12600 s / 15300 s) is past the wind's last level (14400 s) for the late ones only -- the reference gives the whole view the code.  The
    early releases stop at 10800 s, one step before a per-particle rule would stop them (at 14400 s): the t values tell the rules apart"""
    pset, got = _check("nv_l_partial_time_end")
    early = np.arange(65) % 3 == 0
    assert np.all(got["state"] == pa.StatusCode.ErrorOutsideTimeInterval)
    assert np.all(got["t"][early] == 10800.0) and np.all(got["t"][~early] == 13500.0)
    ref = nu.load_fixture("nv_l_partial_time_end")[0]
    assert np.all(ref["t"][early] == 10800.0) and np.all(ref["t"][~early] == 13500.0)


def test_m_two_vectors_in_one_list(gpu):
    pset, got = _check("nv_m_two_vectors")
    prog = pset._kernel.user_program
    assert got["ei"].shape == (65, 2) and np.ptp(got["ei"][:, 0]) > 0 and np.ptp(got["ei"][:, 1]) > 0
    assert not np.array_equal(got["ei"], np.zeros_like(got["ei"]))
    assert [v[0] for v in prog.vectors] == ["Wind", "UVstokes"] and prog.vectors[0][5] == 1 and prog.vectors[1][5] == 0
    assert "case 0: eval_vec<double, 1, 1>(" in prog.source and "case 1: eval_vec<double, 0, 0>(" in prog.source
    moved = _run("nv_j_cgrid_wind")[1]  # (the same currents and wind without the Stokes drift)
    assert not np.array_equal(got["x"], moved["x"])


def test_n_vector_on_a_second_curvilinear_grid_of_a_flat_mesh(gpu):
    pset, got = _check("nv_n_second_curvilinear")
    v = pset._kernel.user_program.vectors[0]
    assert v[0] == "UVstokes" and v[5] == 1 and v[6] == 0 and "eval_vec<double, 1, 0>(" in pset._kernel.user_program.source
    assert pset.fieldset.UVstokes.igrid == 1 and not pset.fieldset.U.grid.is_curvilinear
    assert 100 < len(got["x"]) < 130 and np.all(got["state"] < 50) and np.any(got["ei"][:, 1] != 0)


def test_o_deletions_in_the_first_a_middle_and_the_last_wavefront(gpu):
    pset, got = _check("nv_o_blocks")
    assert np.array_equal(got["particle_id"], np.array([i for i in range(257) if i not in (3, 130, 256)]))
    spec = dict(SPECS["nv_o_blocks"])
    gone = []
    for steps in (2, 5, 8):  # each of the three leaves on a step of its own
        spec["currents"] = dict(SPECS["nv_o_blocks"]["currents"], runtime=steps * 3600.0)
        ids = nu.run_case(spec)[1]["particle_id"]
        gone.append(sorted(set(range(257)) - set(ids.tolist())))
    assert gone == [[3], [3, 130], [3, 130, 256]]


def test_p_detached_sample(gpu):
    """`fieldset.Wind[t, z, y, x]` without the particles in the key: the wind moves them, and neither `ei` of the wind's grid nor the state
    is touched -- a list with only the detached kernel leaves both as a list that samples nothing does"""
    pset, got = _check("nv_p_detached")
    assert np.all(got["ei"][:, 1] == 0) and np.any(got["ei"][:, 0] != 0)
    plain = _run("nv_h_stream")  # (not the same wind: only to see that an attached sample does move the second grid's ei)
    assert np.any(plain[1]["ei"][:, 1] != 0)
    spec = SPECS["nv_p_detached"]
    only = nu.run_case(dict(spec, kernels=["WindDetached"]))
    nothing = nu.run_case(dict(spec, kernels=["NoSample"]))
    assert only[0]._kernel.jit_report.startswith("compiled") and only[2] is None and nothing[2] is None
    for c in ("ei", "state", "t", "particle_id"):
        assert np.array_equal(only[1][c], nothing[1][c]), c
    assert not np.array_equal(only[1]["x"], nothing[1]["x"])


def _report_of(fs, kernels, spatial=np.float64, **where):
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(spatial), **where)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute(kernels, runtime=60.0, dt=60.0)
        except tuple(getattr(pa, e) for e in nu.ERRORS):  # (what the host loop then makes of the sample is not what is looked at here)
            pass
    return pset._kernel


def test_i_refused_on_a_uxgrid(gpu):
    from oracle import ux_cases
    from ux_utils import ux_dataset

    case = ux_cases.draw_case(3)
    names = set(case["fields"])
    vf = {"UV": ("U", "V"), "UVstokes": ("U", "V")}
    if "W" in names:
        vf["UVW"] = ("U", "V", "W")
    fs = pa.FieldSet.from_ugrid_conventions(ux_dataset(case), mesh=case["mesh"], vector_fields=vf)
    k = _report_of(fs, [pa.kernels.AdvectionEE, nk.StokesEuler], x=np.asarray(case["x"])[:2], y=np.asarray(case["y"])[:2], z=np.asarray(case["z"])[:2],
                   t=np.zeros(2))
    assert k.jit_report.startswith("vector field 'UVstokes'") and "UxGrid" in k.jit_report and k.host_functions == ["StokesEuler"]


def test_i_refused_in_a_croco_list(gpu):
    from croco_utils import croco_fieldset
    from oracle import croco_cases
    from tools import make_croco_golden as mg

    case = croco_cases.draw_case(1)
    co = case["coords"]
    two_d = np.asarray(co["x_rho"]).ndim == 2
    coords = {"x_rho": (("eta_rho", "xi_rho") if two_d else ("xi_rho",), co["x_rho"]), "y_rho": (("eta_rho", "xi_rho") if two_d else ("eta_rho",), co["y_rho"]),
              "s_w": (("s_w",), co["s_w"]), "time": (("time",), np.asarray(co["time"], dtype=np.float64))}
    fields = {mg.FIELD_NAMES.get(k, k): (mg.case_dims(case)[k], a) for k, a in case["fields"].items()}
    plain = croco_fieldset(case)
    vf = {n: tuple(c.name for c in (f.U, f.V, f.W) if c is not None) for n, f in plain.fields.items() if isinstance(f, pa.VectorField)}
    vf["UVstokes"] = vf["UV"]
    fs = pa.FieldSet.from_sgrid_conventions(pa.convert.croco_to_sgrid(fields=fields, coords=coords), mesh=case["mesh"], vector_fields=vf)
    fs.add_context("hc", case["hc"])
    k = _report_of(fs, [pa.kernels.AdvectionRK2_3D_CROCO, nk.StokesEuler], x=np.asarray(case["x"])[:2], y=np.asarray(case["y"])[:2],
                   z=np.asarray(case["z"])[:2], t=np.zeros(2))
    assert k.jit_report.startswith("vector field 'UVstokes'") and "CROCO" in k.jit_report and k.host_functions == ["StokesEuler"]


def test_i_refused_with_float32_coordinate_arrays(gpu):
    from oracle import cases as oc

    c = oc.rect_agrid_case("typed", mesh="spherical", kernels=["AdvectionRK2", "WindMidpoint"], seed=3, nx=12, ny=9, nz=3, nt=3, npart=4,
                           coord_dtype=np.float32, margin=0.3)
    c = nu._same_grid_vector(c, ("UWind", "VWind"), scale=8.0, seed=11)
    fs = nu.build_fieldset(dict(currents=c, vectors={"Wind": ("UWind", "VWind")}, context={"windage": 0.03}))
    k = _report_of(fs, [pa.kernels.AdvectionRK2, nk.WindMidpoint], x=c["x"], y=c["y"], z=c["z"], t=np.zeros(4))
    assert k.jit_report.startswith("vector field 'Wind': float32 coordinate arrays") and k.host_functions == ["WindMidpoint"]


def test_i_a_vector_without_device_interpolator_keeps_the_host_path(gpu):
    spec = SPECS["nv_a_adv_wind"]
    fs = nu.build_fieldset(spec)

    fs.Wind.interp_method = pa.interpolators.Ux_Velocity()  # (an interpolator of unstructured meshes: nothing a structured module can call)
    pset = nu.build_pset(spec, fs)
    from parcels_amd import jit

    with pytest.raises(jit.NotTranslatable, match="^vector field 'Wind': its interpolator Ux_Velocity has no device code"):
        jit.compile_kernel_list(nu.kernel_list(spec), pa.kernels.kernel_id, pset._pclass, fs, pset._engine())


def test_a_sum_with_too_many_grids_names_the_cap(gpu):
    fs = nu._pa_fieldset_of(SPECS["nv_a_adv_wind"]["currents"], {})
    for j in range(4):
        s = nu._second_grid((f"UA{j}", f"VA{j}"), lon=(0.0, 360.0), lat=(-80.0, 80.0), time_s=np.arange(3) * 7200.0, scale=1.0, seed=j)
        fs += nu._pa_fieldset_of(s, {f"Extra{j}": (f"UA{j}", f"VA{j}")})
    assert len(fs.gridset) == 5
    with pytest.raises(Exception, match="PK_MAX_GRIDS"):
        fs._engine_or_create()
