"""GPU: Python kernels of a CROCO kernel list compiled into the fused sigma loop (csrc/pk_sigma.h, parcels_amd/jit.py: _TEMPLATE_SIGMA)
-- the tutorial's list, the documented sampling recipe with its convert_z_to_sigma_croco call -- against the reference's fixtures and,
bit for bit, against the same list on the host path (PARCELS_AMD_JIT=0)."""

import ctypes as C
import os
import warnings

import numpy as np
import pytest

import croco_user_kernels as uk
import parcels_amd as pa
from croco_utils import ERRORS, PROG_SIGMA, assert_matches, croco_fieldset
from parcels_amd import StatusCode, _hip
from parcels_amd.kernel import Kernel
from tools import make_croco_golden as mg

pytestmark = pytest.mark.gpu

TUTORIAL = [pa.AdvectionRK2_3D_CROCO, uk.DeleteParticle]
RECIPE = [pa.AdvectionRK2_3D_CROCO, uk.OmegaRecipe]
NO_CROCO_ID = [pa.AdvectionRK2, uk.TracerRecipe]
AROUND = [uk.Age, pa.AdvectionRK2_3D_CROCO, uk.DeleteOld]
VARIABLES = {"omega": np.float64, "tracer": np.float64, "age": np.float32}
RECT, CURV = "croco_rect_flat_f64data_f64part", "croco_curv_flat_f64data_f64part"


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("croco_user_kernel_cache"))  # (one directory for the module: a list is compiled once per variant)


def _case(name, **changes):
    return dict(mg.load(os.path.join(mg.GOLDEN, name + ".npz")), **changes)


def _tiled(case, n):
    reps = -(-n // len(case["x"]))
    return dict(case, **{k: np.tile(np.asarray(case[k]), reps)[:n] for k in "xyz"})


def _run(case, kernels, monkeypatch, jit_cache, jit=True, fs=None, calls=None, **pset_kw):
    """the list on the case's fieldset and particles -> (SoA dict, error name or None, the ParticleSet)"""
    monkeypatch.setenv("PARCELS_AMD_JIT_CACHE", jit_cache)
    monkeypatch.setenv("PARCELS_AMD_JIT", "1" if jit else "0")
    fs = fs if fs is not None else croco_fieldset(case)
    fs.add_context("max_age", 4000.0)
    pclass = pa.get_default_particle(np.float32 if case["spatial_dtype"] == "float32" else np.float64)
    pclass = pclass.add_variable([pa.Variable(v, dtype=dt, initial=0) for v, dt in VARIABLES.items()])
    n = len(case["x"])
    t = np.zeros(n) if case.get("t0") is None else np.broadcast_to(np.asarray(case["t0"], dtype=np.float64), (n,)).copy()
    age0 = (np.arange(n) % 5).astype(np.float32) * np.float32(500.0)  # (so that DeleteOld deletes at different steps, and not everybody)
    pset = pa.ParticleSet(fs, pclass=pclass, x=np.asarray(case["x"]), y=np.asarray(case["y"]), z=np.asarray(case["z"]), t=t, age=age0, **pset_kw)
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            for runtime in (calls or [float(case["runtime"])]):
                pset.execute(list(kernels), dt=float(case["dt"]), runtime=runtime)
        except ERRORS as e:
            err = type(e).__name__
    return {k: np.array(v) for k, v in pset._data.items()}, err, pset


def _assert_compiled(pset):
    k = pset._kernel
    assert str(k.jit_report).startswith("compiled"), k.jit_report
    assert k.host_functions == [] and k.user_program is not None
    assert k.user_program.sigma and k.user_program.flags & _hip.PK_USER_SIGMA and not k.user_program.flags & _hip.PK_USER_RIDE
    assert pset._last_stats["program"] == PROG_SIGMA and not pset._last_stats.get("hosted")


@pytest.mark.parametrize("name", ["croco_edges_delete", RECT, CURV])
def test_the_tutorial_list_runs_fused(gpu, monkeypatch, jit_cache, name):
    """[AdvectionRK2_3D_CROCO, DeleteParticle] with the tutorial's own two-line DeleteParticle: the fixture's trajectories (generated with
    the built-in DeleteParticle where the list deletes; the fixtures' SampleOmegaCroco moves nobody and is left out, so is its column)"""
    case = _case(name)
    got, err, pset = _run(case, TUTORIAL, monkeypatch, jit_cache)
    assert err == case["err"]
    _assert_compiled(pset)
    assert_matches(got, case["ref"], dict(case, kernels=["AdvectionRK2_3D_CROCO", "DeleteParticle"]), name)
    if name == "croco_edges_delete":
        assert 0 < len(got["x"]) < len(case["x"])  # some were deleted


@pytest.mark.parametrize("name", ["croco_rect_flat_f32data_f32part", "croco_rect_flat_f32data_f64part", "croco_rect_flat_f64data_f32part", RECT, CURV])
def test_the_static_recipe_samples_what_sample_omega_croco_samples(gpu, monkeypatch, jit_cache, name):
    """the conversion call and the sample at its result, next to AdvectionRK2_3D_CROCO: the omega column is the reference's SampleOmegaCroco's"""
    case = _case(name)
    got, err, pset = _run(case, RECIPE, monkeypatch, jit_cache)
    assert err == case["err"]
    _assert_compiled(pset)
    assert_matches(got, case["ref"], case, name)
    assert np.any(got["omega"] != 0)


def test_a_list_without_a_croco_kernel_runs_the_sigma_loop(gpu, monkeypatch, jit_cache):
    """[AdvectionRK2, <recipe>]: the conversion call alone makes the module a sigma module and the launch program 7"""
    case = _case("croco_host_recipe")
    got, err, pset = _run(case, NO_CROCO_ID, monkeypatch, jit_cache)
    assert err == case["err"]
    _assert_compiled(pset)
    assert_matches(got, case["ref"], case, "croco_host_recipe")


def _ring(case):
    return croco_fieldset(case).to_windowed_arrays()


COMPARISONS = {
    "tutorial list": lambda: (_case("croco_edges_delete"), TUTORIAL, {}),
    "tutorial list, curvilinear": lambda: (_case(CURV), TUTORIAL, {}),
    "static recipe": lambda: (_case("croco_rect_flat_f32data_f32part"), RECIPE, {}),
    "no CROCO id": lambda: (_case("croco_host_recipe"), NO_CROCO_ID, {}),
    "two user kernels around the CROCO kernel": lambda: (_case(RECT), AROUND, {}),
    "error stop": lambda: (_case("croco_edges"), RECIPE, {}),
    "257 particles": lambda: (_tiled(_case(RECT), 257), RECIPE, {}),
    "two execute calls": lambda: (_case(RECT), RECIPE, {"calls": [1200.0, 1800.0]}),
    "ring of 3 level slots": lambda: (_case(RECT, runtime=7000.0), RECIPE, {"ring": True}),
}


@pytest.mark.parametrize("which", list(COMPARISONS))
def test_compiled_list_equals_the_host_path_to_the_bit(gpu, monkeypatch, jit_cache, which):
    """every column, the raised error, where every particle stands after an error stop.

    Two properties of the HOST path shape the cases.  A Python kernel's sample WITH the particles is searched there without their `ei`
    (field.py: _attached_guess gives a guess on a UxGrid only); on a curvilinear grid such a search goes through the spatial hash and
    returns float32-rounded cell coordinates, so the recipe's samples differ from the reference's -- and from the compiled list's, which
    searches from `ei` and is held to the reference's fixture above -- at the float32 level (measured on croco_curv_flat_f64data_f64part:
    omega differs by up to 3.6e-7 relative).  The curvilinear grid is therefore compared with the list that samples nothing in Python.
    And the host path runs with every time level resident only (its body_only launches do not stream): the compiled run on a ring of three
    slots is compared with the host path on the plain fieldset, whose result cannot depend on a ring."""
    case, kernels, kw = COMPARISONS[which]()
    ring = kw.pop("ring", False)
    dj, ej, pj = _run(case, kernels, monkeypatch, jit_cache, jit=True, fs=_ring(case) if ring else None, sort_by_cell=False, **kw)
    _assert_compiled(pj)
    if ring:
        assert pj._last_stats["launches"] > 1  # the levels really streamed
    dh, eh, ph = _run(case, kernels, monkeypatch, jit_cache, jit=False, sort_by_cell=False, **kw)
    assert ph._kernel.jit_report == "PARCELS_AMD_JIT=0" and ph._kernel.host_functions
    assert ph._last_stats.get("hosted") if eh is None else ph._last_stats is None  # (an error leaves the host loop before its statistics)
    assert ej == eh
    if which == "error stop":
        assert ej is not None
    assert sorted(dj) == sorted(dh)
    for col in dj:
        assert dj[col].dtype == dh[col].dtype, col
        np.testing.assert_array_equal(dj[col], dh[col], err_msg=f"{which}: column '{col}'")
    if which.startswith("two user kernels"):
        assert 0 < len(dj["x"]) < len(case["x"]) and dj["age"].dtype == np.float32 and np.all(dj["age"] > 0)
    print(f"{which}: {len(dj['x'])} of {len(case['x'])} particles, states {sorted(set(dj['state'].tolist()))}, error {ej}")


@pytest.mark.parametrize("jit", [True, False])
def test_a_conversion_outside_the_time_interval_raises_out_of_execute(gpu, monkeypatch, jit_cache, jit):
    """convert_z_to_sigma_croco calls fieldset.zeta.eval directly: leaving zeta's time interval there is no status code for the kernels
    behind it but an exception -- the DeleteParticle behind the recipe deletes nobody"""
    case = _case(RECT)
    last = float(case["coords"]["time"][-1])
    case = dict(case, t0=last - 450.0, runtime=1000.0)
    got, err, pset = _run(case, [uk.OmegaRecipe, pa.DeleteParticle], monkeypatch, jit_cache, jit=jit)
    if jit:
        assert str(pset._kernel.jit_report).startswith("compiled"), pset._kernel.jit_report
    assert err == "OutsideTimeInterval"
    assert len(got["x"]) == len(case["x"]) and not np.any(got["state"] == StatusCode.Delete)


def test_the_detached_conversion_stays_on_the_host_path_on_a_curvilinear_grid(gpu, monkeypatch, jit_cache):
    case = _case(CURV)
    kernels = [pa.AdvectionRK2_3D_CROCO, uk.DetachedRecipe]
    got, err, pset = _run(case, kernels, monkeypatch, jit_cache)
    k = pset._kernel
    assert k.user_program is None and k.host_functions == ["DetachedRecipe"] and pset._last_stats.get("hosted")
    assert "without particles on a curvilinear grid" in k.jit_report
    want, err2, _ = _run(case, kernels, monkeypatch, jit_cache, jit=False)
    assert err == err2
    for col in want:
        np.testing.assert_array_equal(got[col], want[col], err_msg=col)
    assert np.any(got["omega"] != 0)


@pytest.mark.parametrize("func", [uk.WrongFirstArgument, uk.WrongArity])
def test_a_malformed_call_is_named_in_the_report(gpu, monkeypatch, jit_cache, func):
    monkeypatch.setenv("PARCELS_AMD_JIT_CACHE", jit_cache)
    monkeypatch.setenv("PARCELS_AMD_JIT", "1")
    case = _case(RECT)
    fs = croco_fieldset(case)
    pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("omega", dtype=np.float64, initial=0))
    pset = pa.ParticleSet(fs, pclass=pclass, x=case["x"], y=case["y"], z=case["z"], t=np.zeros(len(case["x"])))
    k = Kernel([pa.AdvectionRK2_3D_CROCO, func], pset)
    k._try_jit(pset)
    assert k.user_program is None and k.host_functions == [func.__name__] and "convert_z_to_sigma_croco" in k.jit_report


LAUNCHER = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p)
K_RK4, K_CROCO, USER0 = 4, 11, 40


def _begin_with_module(fs, pset, ids, flags):
    """pk_execute_begin of the list with a module of the given kind registered -> (error message, calls of the module's launcher)"""
    engine = pset._engine()
    engine.set_user_program(None)
    engine.bind_particles(pset._data)
    engine.h2d()
    calls = []
    launcher = LAUNCHER(lambda *a: calls.append(a))
    lib, handle = engine.lib, engine.ctx.handle
    engine.ctx.check(lib.pk_set_user_program(handle, C.cast(launcher, C.c_void_p), flags, 0, None), "pk_set_user_program")
    try:
        prm = engine.make_params(ids, endtime=float(100.0), dt0=100.0, context=fs.context)
        rc = lib.pk_execute_begin(handle, C.byref(prm))
        msg = lib.pk_last_error(handle).decode() if rc else ""
        if rc == 0:
            lib.pk_execute_end(handle, None)
    finally:
        engine.ctx.check(lib.pk_set_user_program(handle, None, 0, 0, None), "pk_set_user_program")
    return rc, msg, calls


def test_the_library_refuses_a_module_of_the_wrong_kind(gpu):
    """a sigma module on a structured context without CROCO parameters, a structured module on a list with a CROCO kernel: an error code
    with its own message each, and nothing is launched"""
    from case_utils import build_fieldset, build_pset
    from oracle import cases

    plain = cases.rect_agrid_case("sigma_refusal", mesh="spherical", kernels=["AdvectionRK4"], seed=3, npart=64, runtime=3600.0)
    fs = build_fieldset(plain)
    fs.to_device()
    rc, msg, calls = _begin_with_module(fs, build_pset(plain, fs), [K_RK4, USER0], _hip.PK_USER_SIGMA)
    assert rc != 0 and "built for the CROCO sigma loop" in msg and "pk_set_croco" in msg and calls == []
    case = _case(RECT)
    fs = croco_fieldset(case)
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=case["x"], y=case["y"], z=case["z"], t=np.zeros(len(case["x"])))
    rc, msg, calls = _begin_with_module(fs, pset, [K_CROCO, USER0], 0)
    assert rc != 0 and "built for the kernel-list interpreter" in msg and "PK_USER_SIGMA" in msg and calls == []
    rc, msg, calls = _begin_with_module(fs, pset, [K_CROCO, USER0], _hip.PK_USER_UX)
    assert rc != 0 and "built for a UxGrid" in msg and calls == []
