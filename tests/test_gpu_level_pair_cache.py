"""The level-pair cache of the dedicated 2-D A-grid kernel (csrc/pk_fast_agrid.h: FAST_LP_CACHE, option "block_cache").

The kernel keeps, per lane and in LDS, the z-lerped corner values of the two time levels around t (Z0 and D = Z1 - Z0 of U and V) for
the cell the particle sits in, and only re-fetches them when the cell, the depth or the level pair changes.  Option 2 forces the cache, 0
runs the same arithmetic with Z0 / D formed in registers in every evaluation: the two must agree in every bit (rtol 0), whoever shares a
wavefront, however the launches are split, ring or resident.  Each case is also held to the general program and to the CPU oracle with the
tolerances of tests/test_gpu_fast_path.py (discrete columns and counters exact).  A CPU-only test pins the premise: how often a lane's
cell changes between consecutive evaluations of the headline workload."""

from __future__ import annotations

import numpy as np
import pytest

from case_utils import build_fieldset, build_pset, compare, endtime_of, run_oracle

FAST_VS_GENERAL_RTOL = 1e-12  # tests/test_gpu_fast_path.py


def _scale(case):
    return float(max(np.abs(np.asarray(case["lon"])).max(), np.abs(np.asarray(case["lat"])).max()))


def _run(case, mode, *, fast=True, nslots=None, endtime=None):
    """mode: the "block_cache" option (-1 planned, 0 none, 1 stage-pair block, 2 level-pair cache forced); fast=False: the general program"""
    import warnings

    import parcels_amd as pa

    fs = build_fieldset(case)
    fs.to_device(nslots=nslots)
    fs._engine.ctx.set_option("fast_path", 1 if fast else 0)
    fs._engine.ctx.set_option("block_cache", mode)
    pset = build_pset(case, fs)
    kernels = [getattr(pa.kernels, k) for k in case["kernels"]]
    kw = {"endtime": endtime_of(endtime)} if endtime is not None else {"runtime": float(case["runtime"])}
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute(kernels, dt=float(case["dt"]), **kw)
        except (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.FieldInterpolationError, pa.OutsideTimeInterval, pa.GeneralError) as e:
            err = type(e).__name__
    return {k: np.array(v) for k, v in pset._data.items()}, err, pset._last_stats


def _check(case, *, nslots=None, endtime=None, rtol=1e-12, expect_error=None):
    """cache vs registers at rtol 0; cache vs general program; cache vs oracle"""
    on, eon, son = _run(case, 2, nslots=nslots, endtime=endtime)
    off, eoff, soff = _run(case, 0, nslots=nslots, endtime=endtime)
    assert eon == eoff == expect_error
    assert son["steps"] == soff["steps"] and son["attempts"] == soff["attempts"]
    compare(on, off, rtol=0.0, check_state="all", label=case["name"] + ": cache vs registers", skip=())
    gen, egen, sgen = _run(case, -1, fast=False, nslots=nslots, endtime=endtime)
    assert egen == eon
    assert son["steps"] == sgen["steps"] and son["attempts"] == sgen["attempts"]
    grtol = 5e-7 if case.get("spatial_dtype", "float64") == "float32" else FAST_VS_GENERAL_RTOL
    compare(on, gen, rtol=grtol, atol_pos=grtol * _scale(case), check_state="all", label=case["name"] + ": cache vs general", skip=())
    ref, eref, _ = run_oracle(case, endtime=endtime)
    assert eref == eon
    if eon is None:
        compare(on, ref, rtol=rtol, atol_pos=rtol * _scale(case), check_state="all", label=case["name"] + ": cache vs oracle", skip=())
    return on, son


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["spherical", "flat"])
@pytest.mark.parametrize("fdt,sdt", [(np.float64, "float64"), (np.float32, "float64"), (np.float64, "float32"), (np.float32, "float32")])
def test_cache_equals_registers_general_and_oracle(gpu, mesh, fdt, sdt):
    from oracle import cases

    case = cases.rect_agrid_case("lp_" + mesh, mesh=mesh, kernels=["AdvectionRK4"], seed=11, nx=40, ny=24, nz=7, nt=5, npart=3000, field_dtype=fdt,
                                 spatial_dtype=sdt, runtime=30 * 3600.0)
    _check(case, rtol=5e-7 if sdt == "float32" else 1e-12)


@pytest.mark.gpu
def test_points_on_nodes_and_time_levels(gpu):
    """x, y, z exactly on nodes, t exactly on level times: lenT / lenZ (bits of the block's key) switch inside one wavefront and, for one
    lane, from one evaluation to the next in the same cell."""
    from oracle import cases

    case = cases.rect_agrid_case("lp_nodes", mesh="spherical", kernels=["AdvectionRK4"], seed=3, nx=37, ny=19, nz=6, nt=4, npart=4096,
                                 runtime=2 * 86400.0, dt=21600.0, level_dt=86400.0)
    lon, lat, depth = case["lon"], case["lat"], case["depth"]
    rng = np.random.default_rng(0)
    n = len(case["x"])
    case["x"] = np.where(rng.random(n) < 0.5, lon[rng.integers(2, len(lon) - 2, n)], case["x"])
    case["y"] = np.where(rng.random(n) < 0.5, lat[rng.integers(2, len(lat) - 2, n)], case["y"])
    case["z"] = np.where(rng.random(n) < 0.5, depth[rng.integers(0, len(depth), n)], case["z"])
    _check(case)


@pytest.mark.gpu
def test_staggered_release_times_and_ring(gpu):
    """Release times spread over all levels, unsorted: the waterfall over the key runs inside the miss branch.  Then a ring of 3 levels with
    several launches: the blocks do not survive a launch, the results do not notice."""
    from oracle import cases

    case = cases.rect_agrid_case("lp_stagger", mesh="spherical", kernels=["AdvectionRK4"], seed=8, nx=30, ny=20, nz=5, nt=6, npart=5000,
                                 runtime=None, dt=3600.0, level_dt=43200.0)
    n = len(case["x"])
    case["t0"] = np.random.default_rng(1).uniform(0, 4 * 43200.0, n)
    case["t0"][::7] = 43200.0 * (np.arange(len(case["t0"][::7])) % 4)  # some exactly on a level
    case["endtime"] = 5 * 43200.0
    case["runtime"] = None
    on, _ = _check(case, endtime=case["endtime"])
    ring, rerr, rstats = _run(case, 2, nslots=3, endtime=case["endtime"])
    assert rerr is None and rstats["launches"] > 1
    compare(ring, on, rtol=0.0, check_state="all", label="ring (cache) vs resident (cache)", skip=())
    ring0, rerr0, _ = _run(case, 0, nslots=3, endtime=case["endtime"])
    assert rerr0 is None
    compare(ring, ring0, rtol=0.0, check_state="all", label="ring: cache vs registers", skip=())


@pytest.mark.gpu
def test_domain_exits_and_backward_time(gpu):
    """Fast flow out of a small flat domain with the recovery kernel appended, forwards and backwards in time"""
    from oracle import cases

    for sign in (1.0, -1.0):
        case = cases.rect_agrid_case("lp_exit", mesh="flat", kernels=["AdvectionRK4", "DeleteParticle"], seed=21, nx=24, ny=16, nz=5, nt=4, npart=4000,
                                     vel=3.0, margin=0.02, runtime=36 * 3600.0, dt=sign * 3600.0)
        if sign < 0:
            case["t0"] = np.full(len(case["x"]), float(case["time_s"][-1]))
        on, _ = _check(case)
        assert len(on["x"]) < 4000, "nothing left the domain: the test does not test"


@pytest.mark.gpu
def test_cells_change_in_every_stage(gpu):
    """A flow that carries a particle across a cell or more per half step: (nearly) every evaluation misses"""
    from oracle import cases

    case = cases.rect_agrid_case("lp_fastflow", mesh="spherical", kernels=["AdvectionRK4", "DeleteParticle"], seed=5, nx=240, ny=120, nz=4, nt=4,
                                 npart=6000, vel=60.0, runtime=20 * 3600.0, dt=3600.0)
    _check(case)


@pytest.mark.gpu
def test_headline_shaped_case(gpu):
    """The benchmark's field set with three levels and 2e5 of its particles, across a level boundary"""
    from bench import c2_case

    case = c2_case(nt=3, hi=200_000)
    case["name"] = "lp_c2"
    case["runtime"] = 30 * 3600.0
    on, stats = _check(case)
    assert stats["steps"] == 200_000 * 30
    planned, perr, _ = _run(case, -1)  # the planner picks the cache for this grid
    assert perr is None
    compare(planned, on, rtol=0.0, check_state="all", label="planned vs forced cache", skip=())


@pytest.mark.gpu
def test_forced_cache_raises_where_the_plan_cannot_give_it(gpu):
    """3-D advection (z moves) and a grid whose coordinate tables leave no room for two 512-lane workgroups per CU: option 2 fails with a
    message; the default runs those launches as before (equal to option 1 in every bit)."""
    from oracle import cases

    case3 = cases.rect_agrid_case("lp_3d", mesh="flat", kernels=["AdvectionRK4_3D"], seed=2, nx=30, ny=20, nz=6, nt=4, npart=2000, with_w=True,
                                  runtime=12 * 3600.0)
    big = cases.rect_agrid_case("lp_big_tables", mesh="spherical", kernels=["AdvectionRK4"], seed=2, nx=1100, ny=40, nz=4, nt=3, npart=2000,
                                runtime=12 * 3600.0)  # 1147 table entries: 18 KB
    for case in (case3, big):
        with pytest.raises(Exception, match="block_cache 2"):
            _run(case, 2)
        dflt, derr, dst = _run(case, -1)
        one, oerr, ost = _run(case, 1)
        assert derr == oerr is None and dst["steps"] == ost["steps"] > 0
        compare(dflt, one, rtol=0.0, check_state="all", label=case["name"] + ": default vs stage-pair block", skip=())


# ---- the premise, on the CPU -------------------------------------------------------------------------------------------------------

def _rk4_cells(case, steps):
    """Plain NumPy AdvectionRK4 (XLinear, spherical mesh) that records the ravelled cell of every evaluation: [step, stage, particle]"""
    lon, lat, depth, time_s = case["lon"], case["lat"], case["depth"], case["time_s"]
    U, V = case["fields"]["U"], case["fields"]["V"]
    x, y, z = case["x"].copy(), case["y"].copy(), case["z"].copy()
    dt = float(case["dt"])

    def cell(a, v):
        i = np.clip(np.searchsorted(a, v, side="left") - 1, 0, len(a) - 2)
        return i, (v - a[i]) / (a[i + 1] - a[i])

    zi, zeta = cell(depth, z)

    def sample(t, yy, xx):
        ti, tau = cell(time_s, np.full(1, t))
        ti, tau = int(ti[0]), float(tau[0])
        yi, eta = cell(lat, yy)
        xi, xsi = cell(lon, xx)

        def interp(F):
            def lvl(k):
                def plane(zz):
                    return ((1 - xsi) * (1 - eta) * F[k, zz, yi, xi] + xsi * (1 - eta) * F[k, zz, yi, xi + 1]
                            + (1 - xsi) * eta * F[k, zz, yi + 1, xi] + xsi * eta * F[k, zz, yi + 1, xi + 1])
                return plane(zi) * (1 - zeta) + plane(zi + 1) * zeta
            return lvl(ti) * (1 - tau) + lvl(ti + 1) * tau

        deg2m = 1852.0 * 60.0
        u = interp(U) / (deg2m * np.cos(np.deg2rad(yy)))
        v = interp(V) / deg2m
        return u, v, (zi * (len(lat) * len(lon)) + yi * len(lon) + xi)

    cells = np.empty((steps, 4, len(x)), dtype=np.int64)
    for s in range(steps):
        t = s * dt
        u1, v1, cells[s, 0] = sample(t, y, x)
        u2, v2, cells[s, 1] = sample(t + 0.5 * dt, y + v1 * 0.5 * dt, x + u1 * 0.5 * dt)
        u3, v3, cells[s, 2] = sample(t + 0.5 * dt, y + v2 * 0.5 * dt, x + u2 * 0.5 * dt)
        u4, v4, cells[s, 3] = sample(t + dt, y + v3 * dt, x + u3 * dt)
        x = x + (u1 + 2 * u2 + 2 * u3 + u4) / 6.0 * dt
        y = y + (v1 + 2 * v2 + 2 * v3 + v4) / 6.0 * dt
    return cells


def test_cell_changes_between_evaluations_are_rare():
    """The premise of the level-pair cache on the headline workload (first 1e5 particle ids, 24 steps, cell-sorted, wavefronts of 64): the
    share of lanes whose cell differs from that of the previous evaluation, and of wavefronts with at least one such lane.  Derived when the
    cache was designed: stage 1 (against stage 4 of the step before) 0.0000 / 0.0000, stage 2 0.0087 / 0.424, stage 3 0.0000 / 0.0016,
    stage 4 0.0086 / 0.422.  Asserted with room: the odd stages miss in fewer than 1 % of the wavefronts, the even ones in fewer than 60 %."""
    from bench import c2_case

    case = c2_case(nt=3, hi=100_000)
    steps = 24
    cells = _rk4_cells(case, steps)
    order = np.argsort(cells[0, 0], kind="stable")  # cell-sorted, as the launch sorts
    seq = cells[:, :, order].reshape(steps * 4, -1)
    n = seq.shape[1] // 64 * 64
    miss = (seq[1:, :n] != seq[:-1, :n])  # evaluation k against evaluation k - 1
    stage = (np.arange(1, steps * 4) % 4)
    shares = {}
    for st in range(4):
        m = miss[stage == st]
        lane = float(m.mean())
        wave = float(m.reshape(m.shape[0], -1, 64).any(axis=2).mean())
        shares[st + 1] = (lane, wave)
        print(f"stage {st + 1}: lanes with a new cell {lane:.4f}, wavefronts with such a lane {wave:.4f}")
    assert shares[1][1] < 0.01 and shares[3][1] < 0.01, shares
    assert shares[2][1] < 0.60 and shares[4][1] < 0.60, shares
