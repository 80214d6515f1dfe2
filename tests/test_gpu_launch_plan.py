"""Which program a launch runs (pk_exec_stats.program: PROG_* 0 .. 5 of pk_kernels.h, 100 the dedicated A-grid kernel, 101 the
dedicated C-grid kernels) and what pk_generic_variant answers for a kernel list with user kernels -- pinned over a small matrix of
fieldsets, kernel lists and options, so that the host code that makes the choice (pk_api.hip: the launch planner) can change shape
without changing the choice."""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

from case_utils import build_fieldset, build_pset

pytestmark = pytest.mark.gpu

RK4, RK4_3D, GENERIC, RK45, M1, TYPED = 0, 1, 2, 3, 4, 5
FAST_A, FAST_C = 100, 101
K_RK4, K_RK4_3D, K_DELETE, USER0 = 4, 5, 20, 40
SAMPLES_UV, SAMPLES_UVW = 2, 4  # PK_USER_SAMPLES_*
RK45_CONTEXT = {"RK45_tol": 30.0, "RK45_min_dt": 60.0, "RK45_max_dt": 4 * 3600.0}


def _fieldset(case, options=()):
    fs = build_fieldset(case)
    fs.to_device()
    for name, value in options:
        fs._engine.ctx.set_option(name, value)
    return fs


def _program(case, options=(), populate=True):
    import parcels_amd as pa

    fs = _fieldset(case, options)
    pset = build_pset(case, fs)
    if populate:
        pset.populate_indices()
    kernels = [getattr(pa.kernels, k) for k in case["kernels"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute(kernels, dt=float(case["dt"]), runtime=float(case["runtime"]))
        except (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.OutsideTimeInterval, pa.GridSearchingError):
            pass  # (raised after the launches: the statistics are those of the last one)
    return pset._last_stats


def _agrid(kernels, **kw):
    from oracle import cases

    kw.setdefault("runtime", 4 * 3600.0)
    return cases.rect_agrid_case("plan_agrid", mesh="spherical", kernels=kernels, seed=3, npart=256, **kw)


def _cgrid(kernels, **kw):
    from oracle import cases

    case = cases.curv_cgrid_case("plan_cgrid", mesh="spherical", kernels=kernels, seed=5, npart=256, dt=1800.0, runtime=4 * 3600.0, **kw)
    if "AdvectionRK45" in kernels:
        case["context"] = dict(RK45_CONTEXT)
    return case


def _cgrid_m1():
    from oracle import cases

    return cases.curv_cgrid_diffusion_case("plan_cgrid_m1", mesh="spherical", kernels=["AdvectionDiffusionM1", "DeleteParticle"], seed=6, npart=256,
                                           runtime=4 * 3600.0)


def _agrid_m1():
    from oracle import cases

    return cases.diffusion_case("plan_agrid_m1", mesh="spherical", kernels=["AdvectionDiffusionM1"], seed=7, npart=256, runtime=2 * 3600.0)


@pytest.mark.parametrize("kernel,with_w,prog", [("AdvectionRK4", False, RK4), ("AdvectionRK4_3D", True, RK4_3D)])
def test_agrid_rk4_runs_the_dedicated_kernel_unless_switched_off(gpu, kernel, with_w, prog):
    case = _agrid([kernel], with_w=with_w)
    assert _program(case)["program"] == FAST_A
    assert _program(case, [("fast_path", 0)])["program"] == prog


@pytest.mark.parametrize("make,prog", [(lambda: _cgrid(["AdvectionRK45", "DeleteParticle"], with_w=False), RK45), (_cgrid_m1, M1)])
def test_cgrid_rk45_m1_run_the_dedicated_kernels_unless_switched_off(gpu, make, prog):
    case = make()
    assert _program(case)["program"] == FAST_C
    assert _program(case, [("fast_cgrid", 0)])["program"] == prog


@pytest.mark.parametrize("which", ["rk45", "m1"])
def test_agrid_rk45_m1_without_special_programs_run_the_interpreter(gpu, which):
    if which == "rk45":
        case = _agrid(["AdvectionRK45"], runtime=3 * 3600.0)
        case["context"] = dict(RK45_CONTEXT)
        special = RK45
    else:
        case = _agrid_m1()
        special = M1
    assert _program(case)["program"] == special
    assert _program(case, [("special_programs", 0)])["program"] == GENERIC


def test_float32_coordinates_run_the_typed_program(gpu):
    assert _program(_agrid(["AdvectionRK4"], coord_dtype=np.float32))["program"] == TYPED


def test_listed_time_error_keys_run_the_general_program(gpu):
    """A call in which particles leave the fields' time interval is repeated with the failing samples listed (twe_n > 0): the last launch
    is such a repeat, and it runs the general RK4 program instead of the dedicated kernel."""
    case = _agrid(["AdvectionRK4"], nt=2, runtime=30 * 3600.0)
    st = _program(case)
    assert st["time_error_keys"], "no sample failed call-wide: the test does not test a listed launch"
    assert st["program"] == RK4


def test_body_only_launch_runs_the_interpreter(gpu):
    case = _agrid(["AdvectionRK4"])
    fs = _fieldset(case)
    pset = build_pset(case, fs)
    engine = pset._engine()
    engine.bind_particles(pset._data)
    engine.h2d()
    mask = np.ones(len(pset._data["x"]), dtype=np.int32)
    engine.ctx.check(engine.lib.pk_particles_set_mask(engine.ctx.handle, mask.ctypes.data_as(C.c_void_p)), "pk_particles_set_mask")
    prm = engine.make_params([K_RK4], endtime=float(case["runtime"]), dt0=float(case["dt"]))
    prm.body_only = 1
    from parcels_amd import _hip

    st = _hip.ExecStats()
    engine.ctx.check(engine.lib.pk_execute(engine.ctx.handle, C.byref(prm), C.byref(st)), "pk_execute")
    assert st.launches == 1 and st.program == GENERIC


def test_unguessed_first_cgrid_launch_does_not_run_the_dedicated_kernel(gpu):
    case = _cgrid(["AdvectionRK4", "DeleteParticle"], with_w=False)
    assert _program(case, populate=False)["program"] != FAST_C
    assert _program(case)["program"] == FAST_C


def _variant(fs, ids, sflags=0, fids=()):
    engine = fs._engine
    prm = engine.make_params(ids, endtime=0.0, dt0=1.0, context=fs.context)
    out = [C.c_int32() for _ in range(4)]
    cf = (C.c_int32 * 4)(*(list(fids) + [0] * 4)[:4])
    engine.ctx.check(engine.lib.pk_generic_variant(engine.ctx.handle, C.byref(prm), sflags, len(fids), cf, *[C.byref(o) for o in out]),
                     "pk_generic_variant")
    return tuple(o.value for o in out)


def _check_variants(fs, table):
    got = [_variant(fs, ids, sflags, fids) for ids, sflags, fids, _ in table]
    assert got == [want for *_, want in table]


def test_generic_variant_agrid(gpu):
    """(key, lds, typed, fast): key = float32 fields * 6 + curvilinear * 3 + interp_uv; fast 1 / 2 = the A-grid kernel 2-D / 3-D, for
    user kernels whose sampled scalar fields are laid out like U."""
    case = _agrid(["AdvectionRK4"], with_w=True)
    rng = np.random.default_rng(1)
    case["fields"]["P"] = rng.standard_normal(case["fields"]["U"].shape)  # laid out like U
    case["field_dims"]["P"] = case["field_dims"]["U"]
    case["fields"]["Q"] = rng.standard_normal(case["fields"]["U"].shape).astype(np.float32)  # another dtype
    case["field_dims"]["Q"] = case["field_dims"]["U"]
    fs = _fieldset(case)
    fid = fs._engine.field_ids
    _check_variants(fs, [
        ([K_RK4, USER0], 0, (), (0, 1, 0, 1)),
        ([USER0, K_RK4, K_DELETE], 0, (), (0, 1, 0, 1)),
        ([K_RK4_3D, USER0], 0, (), (0, 1, 0, 2)),
        ([K_RK4, K_RK4, USER0], 0, (), (0, 1, 0, 0)),
        ([USER0], 0, (), (0, 1, 0, 0)),
        ([K_RK4, USER0], 0, (fid["P"],), (0, 1, 0, 1)),
        ([K_RK4, USER0], 0, (fid["U"], fid["P"]), (0, 1, 0, 1)),
        ([K_RK4, USER0], 0, (fid["Q"],), (0, 1, 0, 0)),
        ([K_RK4, USER0], SAMPLES_UV, (), (0, 1, 0, 1)),
        ([K_RK4, USER0], SAMPLES_UVW, (), (0, 1, 0, 0)),  # (a 2-D kernel carries no W)
        ([K_RK4_3D, USER0], SAMPLES_UVW, (), (0, 1, 0, 2)),
    ])
    fs._engine.ctx.set_option("fast_path", 0)
    _check_variants(fs, [([K_RK4, USER0], 0, (), (0, 1, 0, 0))])


def test_generic_variant_float32_fields_and_coordinates(gpu):
    _check_variants(_fieldset(_agrid(["AdvectionRK4"], field_dtype=np.float32)), [([K_RK4, USER0], 0, (), (6, 1, 0, 1))])
    _check_variants(_fieldset(_agrid(["AdvectionRK4"], coord_dtype=np.float32)), [([K_RK4, USER0], 0, (), (0, 1, 1, 0))])


def test_generic_variant_cgrid(gpu):
    """fast 3 / 4 = the C-grid kernel 2-D / 3-D, only for user kernels that sample nothing.  Asked before the first launch, whose search is
    not guessed, the answer is the one for the launches after it."""
    case = _cgrid(["AdvectionRK4", "DeleteParticle"], with_w=False)
    fs = _fieldset(case)
    fid = fs._engine.field_ids
    _check_variants(fs, [
        ([K_RK4, USER0], 0, (), (10, 1, 0, 3)),
        ([K_RK4, USER0, K_DELETE], 0, (), (10, 1, 0, 3)),
        ([K_RK4_3D, USER0], 0, (), (10, 1, 0, 0)),  # (no W field)
        ([K_RK4, USER0], 0, (fid["U"],), (10, 1, 0, 0)),
        ([K_RK4, USER0], SAMPLES_UV, (), (10, 1, 0, 0)),
        ([USER0], 0, (), (10, 1, 0, 0)),
    ])
    fs._engine.ctx.set_option("fast_cgrid", 0)
    _check_variants(fs, [([K_RK4, USER0], 0, (), (10, 1, 0, 0))])
    fs3 = _fieldset(_cgrid(["AdvectionRK4_3D"], with_w=True))
    _check_variants(fs3, [([K_RK4_3D, USER0, K_DELETE], 0, (), (10, 1, 0, 4))])
