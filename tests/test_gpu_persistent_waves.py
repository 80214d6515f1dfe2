"""The persistent launch of the level-pair-cache A-grid kernel (csrc/pk_kernels.h: advect_fast_kernel, fast_claim; option "fast_grid").

The launch starts only as many workgroups as are resident at once; every wavefront claims chunks of 64 consecutive rows -- from its XCD's
eighth of the chunks first, then from the other XCDs' -- until none is left.  Which lane steps a particle changes nothing a particle
computes, so every column, the steps / attempts / paused counters, the first error iteration and the first time-error key must equal, in
every bit, what the one-shot launch of "block_cache" 0 gives (the same arithmetic without the cache, already held bit-identical to it by
tests/test_gpu_level_pair_cache.py), whatever the grid: 1 workgroup (one workgroup walks all eight shares), 2 (XCDs 0 and 1 take the other
six shares), 9, or the planned one."""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

from case_utils import build_fieldset, build_pset, compare, endtime_of

pytestmark = pytest.mark.gpu

GRIDS = (0, 1, 2, 9)  # "fast_grid": 0 = planned
SUCCESS, EVALUATE, DELETE, STOP = 0, 10, 30, 40
STAT_KEYS = ("steps", "attempts", "first_error_iter", "time_error_keys", "launches")


def _case(name, npart, **kw):
    from oracle import cases

    args = dict(mesh="spherical", kernels=["AdvectionRK4"], seed=17, nx=40, ny=24, nz=6, nt=4, npart=npart, runtime=12 * 3600.0)
    args.update(kw)
    return cases.rect_agrid_case(name, **args)


def _options(eng, cache, grid):
    eng.ctx.set_option("block_cache", cache)
    eng.ctx.set_option("fast_grid", grid)


def _execute(case, fs, cache, grid, *, endtime=None, calls=1):
    """ParticleSet.execute through the product path -> (columns, error name, the statistics that must agree)"""
    import parcels_amd as pa

    _options(fs._engine_or_create(), cache, grid)
    pset = build_pset(case, fs)
    kernels = [getattr(pa.kernels, k) for k in case["kernels"]]
    kw = {"endtime": endtime_of(endtime)} if endtime is not None else {"runtime": float(case["runtime"])}
    err, stats = None, []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            for _ in range(calls):
                pset.execute(kernels, dt=float(case["dt"]), **kw)
                stats.append({k: pset._last_stats.get(k) for k in STAT_KEYS})
        except (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.FieldInterpolationError, pa.OutsideTimeInterval, pa.GeneralError) as e:
            err = type(e).__name__
            stats.append({k: pset._last_stats.get(k) for k in STAT_KEYS})
    return {k: np.array(v) for k, v in pset._data.items()}, err, stats


def _all_grids_equal_one_shot(case, *, nslots=None, endtime=None, calls=1, grids=GRIDS):
    fs = build_fieldset(case)
    fs.to_device(nslots=nslots)
    ref, rerr, rstats = _execute(case, fs, 0, 0, endtime=endtime, calls=calls)
    for g in grids:
        got, gerr, gstats = _execute(case, fs, 2, g, endtime=endtime, calls=calls)
        assert gerr == rerr, (g, gerr, rerr)
        assert gstats == rstats, (g, gstats, rstats)
        compare(got, ref, rtol=0.0, check_state="all", label=f"{case['name']}: persistent (fast_grid {g}) vs one-shot", skip=())
    return ref, rerr, rstats


# ---- launches on columns of the test's own making (pk_execute_begin / _end): every counter of the launch ------------------------------

def _columns(case, eng, sdt=np.float64, *, dz=None, state=None):
    n = len(case["x"])
    t0 = case.get("t0")
    d = {
        "t": np.zeros(n) if t0 is None else np.asarray(t0, np.float64).copy(),
        "z": np.asarray(case["z"]).astype(sdt), "y": np.asarray(case["y"]).astype(sdt), "x": np.asarray(case["x"]).astype(sdt),
        "dz": (np.zeros(n) if dz is None else np.asarray(dz)).astype(sdt), "dy": np.zeros(n, sdt), "dx": np.zeros(n, sdt),
        "dt": np.full(n, float(case["dt"])),
        "state": np.full(n, EVALUATE, np.int32) if state is None else np.asarray(state, np.int32).copy(),
        "ei": np.zeros((n, 1), np.int32),
        "particle_id": np.arange(n, dtype=np.int64),
    }
    d["ei"][:, 0] = eng.search(0, d["z"], d["y"], d["x"])
    return d


def _launch(eng, kernel_names, *, endtime, dt0, reset_state=1, horizon=None):
    import parcels_amd as pa
    from parcels_amd import _hip
    from parcels_amd import kernels as _k

    prm = eng.make_params([_k.kernel_id(getattr(pa.kernels, k)) for k in kernel_names], endtime=endtime, dt0=dt0, reset_state=reset_state, horizon=horizon)
    st = _hip.ExecStats()
    eng.ctx.check(eng.lib.pk_execute_begin(eng.ctx.handle, C.byref(prm)), "pk_execute_begin")
    eng.ctx.check(eng.lib.pk_execute_end(eng.ctx.handle, C.byref(st)), "pk_execute_end")
    return dict(steps=int(st.steps), attempts=int(st.attempts), paused=int(st.paused), err_iter=int(st.first_error_iter), twe_key=int(st.first_time_error_key),
                program=int(st.program))


def _launches(eng, cols, launches, cache, grid):
    """the launches (keyword sets of _launch) one behind the other on a fresh upload of `cols` -> (columns, statistics per launch)"""
    _options(eng, cache, grid)
    data = {k: v.copy() for k, v in cols.items()}
    eng.bind_particles(data)
    eng.h2d()
    stats = [_launch(eng, **kw) for kw in launches]
    eng.d2h()
    return data, stats


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _launches_equal_one_shot(eng, cols, launches, grids=GRIDS):
    ref, rstats = _launches(eng, cols, launches, 0, 0)
    for g in grids:
        got, gstats = _launches(eng, cols, launches, 2, g)
        assert gstats == rstats, (g, gstats, rstats)
        for k in ref:
            assert _same_bits(got[k], ref[k]), (g, k)
    return ref, rstats


def _device(case, nslots=None):
    fs = build_fieldset(case)
    fs.to_device(nslots=nslots)
    return fs, fs._engine


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 512, 513, 4097])
def test_every_grid_equals_the_one_shot_launch(gpu, n):
    """One row, one row short of a chunk, a full chunk, one row more, one workgroup of the one-shot launch, one row more, 65 chunks (more
    chunks than shares, a remainder of one): the planned grid and the caps 1, 2 and 9 against block_cache 0 -- and so with each other."""
    case = _case(f"pw_n{n}", n)
    ref, err, stats = _all_grids_equal_one_shot(case)
    assert err is None and stats[0]["steps"] == n * 12


def test_counters_of_the_launch_agree(gpu):
    """The same through pk_execute_begin / _end: steps, attempts, paused, first error iteration and first time-error key of the launch."""
    case = _case("pw_counters", 1000, kernels=["AdvectionRK4"])
    fs, eng = _device(case)
    ref, stats = _launches_equal_one_shot(eng, _columns(case, eng), [dict(kernel_names=["AdvectionRK4"], endtime=12 * 3600.0, dt0=3600.0)])
    assert stats[0]["steps"] == 12 * 1000 and stats[0]["paused"] == 0 and np.all(ref["t"] == 12 * 3600.0)


def test_rows_that_are_not_evaluated_come_back_untouched(gpu):
    """A continued launch (reset_state 0): rows in another state than Evaluate -- whole chunks of them, and scattered ones -- keep every bit."""
    case = _case("pw_states", 1300)
    fs, eng = _device(case)
    rng = np.random.default_rng(4)
    state = rng.choice(np.array([SUCCESS, EVALUATE, STOP], np.int32), 1300)
    state[128:320] = STOP  # three chunks without a row to step
    cols = _columns(case, eng, state=state)
    cols["dx"][:] = 1e-9 * (1 + np.arange(1300))  # (values a launch would change)
    ref, stats = _launches_equal_one_shot(eng, cols, [dict(kernel_names=["AdvectionRK4"], endtime=6 * 3600.0, dt0=3600.0, reset_state=0)])
    still = state != EVALUATE
    assert stats[0]["steps"] == 6 * int((~still).sum()) > 0
    for k in cols:
        assert _same_bits(ref[k][still], cols[k][still]), k
    assert np.all(ref["t"][~still] == 6 * 3600.0)


@pytest.mark.parametrize("recovery", [[], ["DeleteParticle"]], ids=["raise", "delete"])
def test_out_of_bounds(gpu, recovery):
    """A fast flow out of a small flat domain, with and without the recovery kernel"""
    case = _case("pw_oob", 1500, mesh="flat", kernels=["AdvectionRK4"] + recovery, nx=24, ny=16, nz=5, vel=3.0, margin=0.02, runtime=36 * 3600.0, seed=21)
    ref, err, stats = _all_grids_equal_one_shot(case)
    if recovery:
        assert err is None and 0 < len(ref["x"]) < 1500
    else:
        assert err == "FieldOutOfBoundError" and stats[0]["first_error_iter"] > 0
    fs, eng = _device(case)
    _, lst = _launches_equal_one_shot(eng, _columns(case, eng), [dict(kernel_names=case["kernels"], endtime=36 * 3600.0, dt0=3600.0)], grids=(0, 2))
    assert lst[0]["err_iter"] > 0 or recovery


@pytest.mark.parametrize("recovery", [[], ["DeleteParticle"]], ids=["raise", "delete"])
def test_time_errors(gpu, recovery):
    """A run past the last time level: the first time-error key of the launch and what the call makes of it"""
    case = _case("pw_twe", 700, kernels=["AdvectionRK4"] + recovery, nt=3, dt=21600.0, runtime=3 * 86400.0)
    n = len(case["x"])
    case["t0"] = np.where(np.arange(n) % 5 == 0, 43200.0, 0.0)
    ref, err, stats = _all_grids_equal_one_shot(case)
    assert err == "OutsideTimeInterval" or recovery
    fs, eng = _device(case)
    _, lst = _launches_equal_one_shot(eng, _columns(case, eng), [dict(kernel_names=case["kernels"], endtime=3 * 86400.0, dt0=21600.0)], grids=(0, 1))
    assert lst[0]["twe_key"] > 0


def test_ring_launches_pause_and_resume(gpu):
    """A ring of three levels: several launches per call, particles pause at the edge of the resident window and resume.  Then one pause and one
    resumption by hand (a horizon, then a continued launch), where the paused counter shows."""
    case = _case("pw_ring", 2500, nt=6, level_dt=43200.0, runtime=None)
    case["endtime"] = 5 * 43200.0
    ref, err, stats = _all_grids_equal_one_shot(case, nslots=3, endtime=case["endtime"], grids=(0, 1, 2))
    assert err is None and stats[0]["launches"] > 1
    fs, eng = _device(case)
    half = dict(kernel_names=["AdvectionRK4"], endtime=24 * 3600.0, dt0=3600.0, horizon=(0.0, 10.5 * 3600.0))
    rest = dict(kernel_names=["AdvectionRK4"], endtime=24 * 3600.0, dt0=3600.0, reset_state=0)
    out, lst = _launches_equal_one_shot(eng, _columns(case, eng), [half, rest])
    assert lst[0]["paused"] == 2500 and lst[0]["steps"] == 10 * 2500 and lst[1]["steps"] == 14 * 2500 and np.all(out["t"] == 24 * 3600.0)


def test_staggered_release_times_inside_a_wavefront(gpu):
    case = _case("pw_stagger", 3000, nt=6, level_dt=43200.0, runtime=None, seed=8)
    n = len(case["x"])
    case["t0"] = np.random.default_rng(1).uniform(0, 4 * 43200.0, n)
    case["t0"][::7] = 43200.0 * (np.arange(len(case["t0"][::7])) % 4)
    _, err, _ = _all_grids_equal_one_shot(case, endtime=5 * 43200.0)
    assert err is None


@pytest.mark.parametrize("fdt", [np.float64, np.float32], ids=["fields64", "fields32"])
def test_float32_particle_storage(gpu, fdt):
    case = _case("pw_f32", 1100, field_dtype=fdt, spatial_dtype="float32")
    _, err, stats = _all_grids_equal_one_shot(case, grids=(0, 1, 9))
    assert err is None and stats[0]["steps"] == 1100 * 12


def test_float32_fields(gpu):
    case = _case("pw_ff32", 1100, field_dtype=np.float32)
    _, err, _ = _all_grids_equal_one_shot(case, grids=(0, 2))
    assert err is None


def test_a_dz_brought_into_the_launch(gpu):
    """Some rows arrive with a dz: the first position update moves z, the depth search runs again (and may end outside the grid)"""
    case = _case("pw_dz", 900)
    fs, eng = _device(case)
    n = 900
    dz = np.where(np.arange(n) % 3 == 0, np.random.default_rng(2).uniform(-1500.0, 1500.0, n), 0.0)
    dz[5] = 1e5  # through the bottom
    ref, stats = _launches_equal_one_shot(eng, _columns(case, eng, dz=dz), [dict(kernel_names=["AdvectionRK4"], endtime=8 * 3600.0, dt0=3600.0)])
    assert stats[0]["err_iter"] > 0 and np.any(ref["z"] != np.asarray(case["z"]))


def test_back_to_back_launches_and_a_launch_after_compaction(gpu):
    """The cursors start from zero in every launch: two calls on one set, with rows deleted (and the set compacted) in between"""
    case = _case("pw_twice", 2000, mesh="flat", kernels=["AdvectionRK4", "DeleteParticle"], nx=24, ny=16, nz=5, vel=3.0, margin=0.02, runtime=10 * 3600.0, seed=21)
    ref, err, stats = _all_grids_equal_one_shot(case, calls=3)
    assert err is None and len(stats) == 3 and 0 < len(ref["x"]) < 2000
    assert stats[0]["steps"] > stats[1]["steps"] > stats[2]["steps"] > 0  # fewer rows every time
    one = dict(kernel_names=["AdvectionRK4"], endtime=3 * 3600.0, dt0=3600.0)
    two = dict(kernel_names=["AdvectionRK4"], endtime=6 * 3600.0, dt0=3600.0)
    small = _case("pw_twice_b", 700)
    fs2, eng2 = _device(small)
    _, lst = _launches_equal_one_shot(eng2, _columns(small, eng2), [one, two, dict(two, endtime=7 * 3600.0)])
    assert [s["steps"] for s in lst] == [3 * 700, 3 * 700, 700]


def test_the_planned_launch_is_the_persistent_one(gpu):
    """The default plan runs the cache, and with it the persistent launch: "fast_grid" must be accepted, and negative values refused"""
    case = _case("pw_plan", 600)
    fs, eng = _device(case)
    with pytest.raises(Exception, match="fast_grid"):
        eng.ctx.set_option("fast_grid", -1)
    planned, perr, pst = _execute(case, fs, -1, 0)
    forced, ferr, fst = _execute(case, fs, 2, 1)
    assert perr is None and ferr is None and pst == fst
    compare(planned, forced, rtol=0.0, check_state="all", label="planned vs forced cache on one workgroup", skip=())
