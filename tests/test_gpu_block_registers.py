"""The block in registers of the level-pair kernel (csrc/pk_fast_agrid.h: fast_held, FCtx::fu).

With the level-pair cache (option "block_cache" 2) and the cell record, a lane keeps Z0 / D of U and V -- the sixteen doubles of its LDS slot
-- in registers from one evaluation to the next and from one step to the next; a wave-evaluation without a missing lane reads nothing of
the slot.  When some lane of the wavefront misses, the missing lanes fetch and write their slot and ALL lanes load their block from
their slot again.  Option 0 forms Z0 / D in every evaluation on the same arithmetic, so the two agree in every bit: each case goes through
tests/test_gpu_level_pair_cache.py::_check (cache vs registers at rtol 0; cache vs the general program and vs the CPU oracle at that file's
tolerances; status, ei, t, step and attempt counts exact).  The cases are those in which a held block, or a held time cell, could be stale
or wrongly trusted: hit lanes beside missing lanes, steps that land exactly on time levels (forward, backward, resident, ring), lanes of one
wavefront in different time cells, split launches, degenerate time axes, partial wavefronts, non-finite positions, a dz brought into the
launch, both storage dtypes."""

from __future__ import annotations

import numpy as np
import pytest

from case_utils import compare
from test_gpu_level_pair_cache import _check, _run


def _small(name, **kw):
    from oracle import cases

    args = dict(mesh="spherical", kernels=["AdvectionRK4"], nx=12, ny=9, nz=3, nt=4, npart=600, seed=9)
    args.update(kw)
    return cases.rect_agrid_case(name, **args)


@pytest.mark.gpu
@pytest.mark.parametrize("sdt", ["float64", "float32"])
def test_hit_lanes_beside_missing_lanes(gpu, sdt):
    """Unsorted rows, alternately a particle in a flow of a 33-degree cell or more per half step and one that hardly moves: while the fast
    ones are inside the grid every wavefront misses in every evaluation, and half of its lanes never leave their cell -- their blocks
    have to survive each of those miss branches.  The fast ones leave through the east side within a few steps and are deleted."""
    case = _small("br_mixed_" + sdt, kernels=["AdvectionRK4", "DeleteParticle"], spatial_dtype=sdt, runtime=5 * 3600.0)
    n = len(case["x"])
    lon, lat = case["lon"], case["lat"]
    fast = np.arange(n) % 2 == 0
    # U: 2000 m/s (65 degrees per step at the equator, more further out) in the eastern half, 1e-3 m/s (1e-5 of a cell in the whole run) in the west
    U, V = case["fields"]["U"], case["fields"]["V"]
    east = lon >= lon[len(lon) // 2]
    U[...] = np.where(east, 2000.0, 1e-3)[None, None, None, :] * (1.0 + 0.1 * np.cos(np.arange(len(lat)))[None, None, :, None])
    V[...] *= 1e-3
    rng = np.random.default_rng(2)
    case["x"] = np.where(fast, rng.uniform(lon[len(lon) // 2], lon[len(lon) // 2 + 1], n), rng.uniform(lon[1], lon[len(lon) // 2 - 2], n))
    case["y"] = rng.uniform(lat[2], lat[-3], n)
    x0, y0 = case["x"].copy(), case["y"].copy()
    on, stats = _check(case, rtol=5e-7 if sdt == "float32" else 1e-12)
    ids = on["particle_id"]
    cx0, cy0 = np.searchsorted(lon, x0[ids]), np.searchsorted(lat, y0[ids])
    cx1, cy1 = np.searchsorted(lon, on["x"].astype(np.float64)), np.searchsorted(lat, on["y"].astype(np.float64))
    stay = (cx0 == cx1) & (cy0 == cy1)
    assert stay[~fast[ids]].all() and (~fast[ids]).sum() == (~fast).sum(), "the slow particles were to stay in their cells"
    gone = n - len(ids)
    assert gone + (~stay).sum() > 0.8 * fast.sum(), "the fast particles were to cross cells"


def _on_levels(name, sign, **kw):
    """Level spacing 3 dt: every third step lands exactly on a level, forward from level 0 or backward from the last one, across three level
    boundaries in one launch"""
    case = _small(name, nt=5, dt=sign * 3600.0, level_dt=3 * 3600.0, runtime=11 * 3600.0, **kw)
    if sign < 0:
        case["t0"] = np.full(len(case["x"]), float(case["time_s"][-1]))
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_steps_land_exactly_on_time_levels(gpu, sign):
    """t on a node belongs to the time cell on its left and has tau of that cell's end (forward) or start; the key of the block changes there
    for the whole wavefront.  Resident, and through a ring of three slots (several launches)."""
    case = _on_levels("br_levels_%s" % ("fwd" if sign > 0 else "bwd"), sign)
    on, stats = _check(case)
    assert stats["steps"] == 11 * len(on["x"]) and stats["launches"] == 1
    ring, rerr, rstats = _run(case, 2, nslots=3)
    assert rerr is None and rstats["launches"] > 1
    compare(ring, on, rtol=0.0, check_state="all", label="ring (cache) vs resident (cache)", skip=())
    ring0, rerr0, _ = _run(case, 0, nslots=3)
    assert rerr0 is None
    compare(ring, ring0, rtol=0.0, check_state="all", label="ring: cache vs registers", skip=())


def _staggered(whole_steps=False):
    """Release times over four time cells (six steps each); whole_steps: all of them multiples of dt, so that a launch that ends on a level cuts no step"""
    case = _small("br_stagger", nt=6, npart=520, dt=3600.0, level_dt=6 * 3600.0, runtime=None)
    n = len(case["x"])
    t0 = np.random.default_rng(5).uniform(0, 4 * 21600.0, n)
    t0[::7] = 21600.0 * (np.arange(len(t0[::7])) % 4)  # exactly on a level ...
    t0[3] = 0.0                                         # ... one of them (and lane 0) at t == 0
    t0[1::11] = 21600.0 * (np.arange(len(t0[1::11])) % 4) + 1800.0  # stages 2 / 3 on a level never, stage 4 neither: between
    t0[2::13] = 21600.0 * (1 + np.arange(len(t0[2::13])) % 3) - 3600.0  # the first step ends on a level
    case["t0"] = np.floor(t0 / 3600.0) * 3600.0 if whole_steps else t0
    case["endtime"] = 5 * 21600.0
    return case


@pytest.mark.gpu
def test_staggered_particle_times(gpu):
    """Lanes of one wavefront in different time cells, some exactly on a level, one at t == 0: a time record for the wavefront has to leave
    those lanes outside, and a lane's own record must not outlive its cell"""
    case = _staggered()
    assert (case["t0"] == 0).sum() >= 2 and len(np.unique(np.floor(case["t0"][:64] / 21600.0))) == 4
    on, stats = _check(case, endtime=case["endtime"])
    assert len(on["x"]) == 520 and (on["t"] == case["endtime"]).all()


@pytest.mark.gpu
def test_split_launches(gpu):
    """One launch against five (the columns carried from one execute to the next): registers and record are rebuilt by each launch's first
    evaluation.  Launches that end between two steps shorten one step per particle: cache against table search only.  Launches that end on the
    levels, with every release time a multiple of dt, run the steps of the single launch: equal to it in every bit."""
    import warnings

    import parcels_amd as pa
    from case_utils import build_fieldset, build_pset, endtime_of

    case = _staggered(whole_steps=True)
    case["name"] = "br_split"
    assert len(np.unique(np.floor(case["t0"][:64] / 21600.0))) == 4 and (case["t0"] % 21600.0 == 0).sum() > 50
    one, err, sone = _run(case, 2, endtime=case["endtime"])
    assert err is None
    res = {}
    for mode in (2, 0):
        fs = build_fieldset(case)
        fs.to_device()
        fs._engine.ctx.set_option("fast_path", 1)
        fs._engine.ctx.set_option("block_cache", mode)
        pset = build_pset(case, fs)
        steps = 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k in range(1, 6):
                pset.execute([pa.kernels.AdvectionRK4], dt=float(case["dt"]), endtime=endtime_of(k * 21600.0 - (1800.0 if k < 5 else 0.0)))
                steps += pset._last_stats["steps"]
        res[mode] = {k: np.array(v) for k, v in pset._data.items()}
        assert steps >= sone["steps"]  # (a split that ends between two steps adds one shortened step per particle that was under way)
    compare(res[2], res[0], rtol=0.0, check_state="all", label="split launches: cache vs registers", skip=())
    whole = {}
    for mode in (2, 0):
        fs = build_fieldset(case)
        fs.to_device()
        fs._engine.ctx.set_option("fast_path", 1)
        fs._engine.ctx.set_option("block_cache", mode)
        pset = build_pset(case, fs)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k in range(1, 6):  # splits on the levels themselves: the same steps as the single launch
                pset.execute([pa.kernels.AdvectionRK4], dt=float(case["dt"]), endtime=endtime_of(k * 21600.0))
        whole[mode] = {k: np.array(v) for k, v in pset._data.items()}
    compare(whole[2], one, rtol=0.0, check_state="all", label="five launches vs one (cache)", skip=())
    compare(whole[2], whole[0], rtol=0.0, check_state="all", label="five launches: cache vs registers", skip=())


@pytest.mark.gpu
@pytest.mark.parametrize("axis", ["one_level", "none"])
def test_degenerate_time_axes(gpu, axis):
    """A field with a single time level, and one without a time axis: no time cell exists, tau is 0 and the second level is never read"""
    case = _small("br_time_" + axis, nt=1, runtime=8 * 3600.0)
    if axis == "none":
        case["time_s"] = None
        case["field_dims"] = {k: ("mockT",) + tuple(v[1:]) for k, v in case["field_dims"].items()}
    on, stats = _check(case)
    assert stats["steps"] == 8 * 600


@pytest.mark.gpu
@pytest.mark.parametrize("npart", [1, 63, 65, 513])
def test_partial_wavefronts(gpu, npart):
    """One lane, a wavefront short of one lane, one lane in a second wavefront, one lane in a second workgroup; steps onto levels included"""
    case = _on_levels("br_n%d" % npart, 1.0, npart=npart)
    on, stats = _check(case)
    assert stats["steps"] == 11 * npart


@pytest.mark.gpu
def test_non_finite_positions_in_healthy_wavefronts(gpu):
    """NaN and infinite coordinates in a few lanes end as errors and are deleted; they take the early returns, which leave the registers and the
    slot alone, while their neighbours go on through level boundaries"""
    case = _on_levels("br_nan", 1.0, npart=200, kernels=["AdvectionRK4", "DeleteParticle"])
    case["x"][3] = np.nan
    case["y"][70] = np.nan
    case["x"][71] = case["y"][71] = np.nan
    case["x"][130] = np.inf
    case["y"][131] = -np.inf
    on, stats = _check(case)
    assert len(on["x"]) == 200 - 5 and stats["steps"] == 195 * 11


@pytest.mark.gpu
@pytest.mark.parametrize("sdt", ["float64", "float32"])
def test_displacement_in_z_on_entry(gpu, sdt):
    """A dz brought into the launch moves z in the first position update: depth, record and block are re-armed, and the registers must be
    loaded again from the slot the second step fills -- beside lanes with dz = 0 that keep theirs"""
    from test_gpu_cell_registers import _oracle_with_dz, _run_with_dz

    case = _small("br_dz_" + sdt, nz=5, nt=3, npart=520, spatial_dtype=sdt, level_dt=3 * 3600.0, runtime=6 * 3600.0)
    n = len(case["x"])
    depth = case["depth"]
    dz = np.random.default_rng(3).uniform(-2500.0, 2500.0, n)
    dz[::3] = 0.0
    dz[1::30] = 1e-30
    dz[2::40] = depth[-1]    # below the bottom after the first step
    dz = dz.astype(sdt)
    z1 = (case["z"].astype(sdt) + dz).astype(np.float64)
    inside = (z1 >= depth[0]) & (z1 <= depth[-1])
    assert (inside & (np.searchsorted(depth, z1) != np.searchsorted(depth, case["z"]))).sum() > 50 and (~inside).sum() > 10
    case["kernels"] = ["AdvectionRK4", "DeleteParticle"]
    on, son = _run_with_dz(case, dz, 2)
    off, soff = _run_with_dz(case, dz, 0)
    assert son["steps"] == soff["steps"] and son["attempts"] == soff["attempts"]
    compare(on, off, rtol=0.0, check_state="all", label="dz on entry: cache vs registers", skip=())
    assert np.array_equal(np.sort(on["particle_id"]), np.flatnonzero(inside))
    rtol = 5e-7 if sdt == "float32" else 1e-12
    scale = float(max(np.abs(case["lon"]).max(), np.abs(case["lat"]).max()))
    gen, sgen = _run_with_dz(case, dz, -1, fast=False)
    assert son["steps"] == sgen["steps"] and son["attempts"] == sgen["attempts"]
    compare(on, gen, rtol=rtol, atol_pos=rtol * scale, check_state="all", label="dz on entry: cache vs general", skip=())
    ref = _oracle_with_dz(case, dz)
    compare(on, ref, rtol=rtol, atol_pos=rtol * scale, check_state="all", label="dz on entry: cache vs oracle", skip=())
