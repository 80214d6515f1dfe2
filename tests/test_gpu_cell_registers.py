"""The cell record of the level-pair kernel (csrc/pk_fast_agrid.h: eval_uvw_lp, FCtx::ya).

With the level-pair cache (option "block_cache" 2) a lane keeps the coordinate-table entries of its cell -- first node, second node and
1 / width of lat and of lon -- in registers, and an evaluation inside that cell touches neither the tables nor the cell index; depth is
searched only when the step loop has moved z.  Option 0 runs the table search in every evaluation on the same arithmetic, so the two must agree in every bit:
each case goes through tests/test_gpu_level_pair_cache.py::_check (cache vs registers at rtol 0; cache vs the general program and vs the
CPU oracle at that file's tolerances; status, ei, t, step and attempt counts exact).  The cases are the ones in which a held record
could be stale or wrongly trusted: neighbouring cells of very different width, points exactly on nodes, particles that leave the grid
or never were inside, non-finite positions, an axis of one cell, partial wavefronts, launches that have to rebuild the record, and
particles that enter the launch with a displacement in z."""

from __future__ import annotations

import numpy as np
import pytest

from case_utils import compare, run_oracle
from test_gpu_level_pair_cache import _check, _run


def _small(name, **kw):
    from oracle import cases

    args = dict(mesh="flat", kernels=["AdvectionRK4", "DeleteParticle"], nx=12, ny=9, nz=3, nt=3, npart=600, seed=4)
    args.update(kw)
    return cases.rect_agrid_case(name, **args)


def _alternating(first, widths, n):
    """n nodes from `first` whose cell widths alternate between the two given ones"""
    w = np.where(np.arange(n - 1) % 2 == 0, widths[0], widths[1]).astype(np.float64)
    return first + np.concatenate([[0.0], np.cumsum(w)])


@pytest.mark.gpu
def test_strongly_non_uniform_spacing(gpu):
    """Neighbouring cells 12 x (lon) and 11.25 x (lat) apart in width, and a flow of ~2 degrees per step across the 1-degree cells: most
    evaluations leave the cell, and a bound or a 1 / width that stayed behind from the neighbour would move the particle at once."""
    case = _small("cr_widths", mesh="spherical", vel=60.0, dt=3600.0, runtime=10 * 3600.0)
    case["lon"] = _alternating(10.0, (1.0, 12.0), 12)
    case["lat"] = _alternating(-20.0, (0.8, 9.0), 9)
    assert min(np.diff(case["lon"]).max() / np.diff(case["lon"]).min(), np.diff(case["lat"]).max() / np.diff(case["lat"]).min()) >= 10
    rng = np.random.default_rng(7)
    n = len(case["x"])
    case["x"] = rng.uniform(case["lon"][2], case["lon"][-3], n)
    case["y"] = rng.uniform(case["lat"][2], case["lat"][-3], n)
    on, stats = _check(case)
    assert stats["steps"] > 5 * len(on["x"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["flat", "spherical"])
def test_points_exactly_on_nodes(gpu, mesh):
    """Every particle starts with x, y or both on a node, the first and the last node of each axis among them (and z on the first and the last
    depth): a point on a node belongs to the cell on its left, which the strict test of the record refuses, so the table path has to answer --
    and the lane must not keep the record of the cell it has just left."""
    case = _small("cr_nodes_" + mesh, mesh=mesh, runtime=8 * 3600.0)
    lon, lat, depth = case["lon"], case["lat"], case["depth"]
    n = len(case["x"])
    k = np.arange(n)
    case["x"] = np.where(k % 3 != 1, lon[k % len(lon)], case["x"])
    case["y"] = np.where(k % 3 != 0, lat[(k // 3) % len(lat)], case["y"])
    case["z"] = np.where(k % 2 == 0, depth[(k // 2) % len(depth)], case["z"])
    for a, v in ((lon, case["x"]), (lat, case["y"]), (depth, case["z"])):
        assert (v == a[0]).any() and (v == a[-1]).any()
    on, stats = _check(case)
    assert stats["steps"] > 0 and len(on["x"]) > n // 2


def _diverging(case, sign):
    """U, V: a flow away from the centre of the domain at 2e-5 per second of the distance on both axes (run backwards in time it would point
    towards it, so the fields change sign with dt): a particle leaves through the side its start point is nearest to, relative to the
    extent of the domain.  Returns those relative start coordinates, -1 .. 1."""
    lon, lat = case["lon"], case["lat"]
    xc, yc, hx, hy = 0.5 * (lon[0] + lon[-1]), 0.5 * (lat[0] + lat[-1]), 0.5 * (lon[-1] - lon[0]), 0.5 * (lat[-1] - lat[0])
    U, V = case["fields"]["U"], case["fields"]["V"]
    U[...] = (sign * 2e-5 * (lon - xc))[None, None, None, :]
    V[...] = (sign * 2e-5 * (lat - yc))[None, None, :, None]
    return (case["x"] - xc) / hx, (case["y"] - yc) / hy


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("delete", [True, False])
def test_exits_through_every_side(gpu, sign, delete):
    """Particles leave through each of the four sides, and some start above the surface or below the bottom: their searches answer codes, not
    cells, and no record may be kept from them.  With DeleteParticle those in error go; without it the run ends with the reference's error."""
    case = _small("cr_exit", kernels=["AdvectionRK4", "DeleteParticle"] if delete else ["AdvectionRK4"], margin=0.05, runtime=30 * 3600.0,
                  dt=sign * 3600.0)
    n = len(case["x"])
    if sign < 0:
        case["t0"] = np.full(n, float(case["time_s"][-1]))
    rx, ry = _diverging(case, sign)
    case["z"][5::97] = -5.0                       # above the surface
    case["z"][11::97] = case["depth"][-1] + 10.0  # below the bottom
    outside_z = (case["z"] < 0) | (case["z"] > case["depth"][-1])
    if delete:
        on, _ = _check(case)
        gone = np.ones(n, bool)
        gone[on["particle_id"]] = False
        assert gone[outside_z].all()
        # past the last node of x or y a particle is out of bounds and goes; past the first one the search answers the code that is an error for
        # depth only: the particle stays, outside the grid, with zero velocity -- and takes the table path in every evaluation from then on
        for name, m in {"east": rx > abs(ry), "north": ry > abs(rx)}.items():
            assert (gone & m & ~outside_z).sum() > 10, f"nothing left through the {name} side: the test does not test"
        assert (on["x"] < case["lon"][0]).sum() > 10 and (on["y"] < case["lat"][0]).sum() > 10, "nothing left through the west / south side"
        assert not gone[(np.maximum(abs(rx), abs(ry)) < 0.05) & ~outside_z].any()
    else:
        _, eref, _ = run_oracle(case)
        assert eref is not None, "no error in the reference: the test does not test"
        _check(case, expect_error=eref)


@pytest.mark.gpu
def test_non_finite_positions_in_healthy_wavefronts(gpu):
    """NaN and infinite coordinates in a few lanes: a NaN fails every compare of the record's test, lands in the last cell of the table search
    and ends as an interpolation error; an infinity is out of bounds.  Their neighbours in the wavefront do not notice."""
    case = _small("cr_nan", mesh="spherical", npart=200, runtime=6 * 3600.0)
    case["x"][3] = np.nan
    case["y"][70] = np.nan
    case["x"][71] = case["y"][71] = np.nan
    case["x"][130] = np.inf
    case["y"][131] = -np.inf
    on, stats = _check(case)
    assert len(on["x"]) == 200 - 5 and stats["steps"] == 195 * 6


@pytest.mark.gpu
def test_two_node_latitude_axis(gpu):
    """One cell in y: cell 0 is the first and the last cell, so both edge rules apply to it"""
    case = _small("cr_ny2", ny=2, vel=2.0, margin=0.1, runtime=24 * 3600.0)
    on, stats = _check(case)
    assert 0 < len(on["x"]) < 600, "every particle or none left: the test does not test"


@pytest.mark.gpu
@pytest.mark.parametrize("npart", [1, 63, 65, 513])
def test_partial_wavefronts(gpu, npart):
    """One lane, a wavefront short of one lane, one lane in a second wavefront, one lane in a second workgroup"""
    case = _small("cr_n%d" % npart, mesh="spherical", npart=npart, runtime=6 * 3600.0)
    on, stats = _check(case)
    assert stats["steps"] == 6 * npart


@pytest.mark.gpu
def test_staggered_release_times_and_ring(gpu):
    """Release times over all levels; then a ring of 3 level slots, which takes several launches: a record does not survive a launch and is
    rebuilt by the first evaluation of the next one.  Ring against resident at rtol 0."""
    case = _small("cr_stagger", mesh="spherical", kernels=["AdvectionRK4"], nt=6, npart=700, dt=3600.0, level_dt=43200.0)
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


def _run_with_dz(case, dz, mode, *, fast=True):
    """_run of tests/test_gpu_level_pair_cache.py for particles that bring a displacement `dz` into the launch"""
    import warnings

    import parcels_amd as pa
    from case_utils import build_fieldset, build_pset

    fs = build_fieldset(case)
    fs.to_device()
    fs._engine.ctx.set_option("fast_path", 1 if fast else 0)
    fs._engine.ctx.set_option("block_cache", mode)
    pset = build_pset(case, fs, dz=dz)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pset.execute([getattr(pa.kernels, k) for k in case["kernels"]], dt=float(case["dt"]), runtime=float(case["runtime"]))
    return {k: np.array(v) for k, v in pset._data.items()}, pset._last_stats


def _oracle_with_dz(case, dz):
    """One Kernel.execute of the CPU oracle from t = 0 on the same particles"""
    from oracle import c_oracle as co

    mc = co.MarshalledCase(case)
    data = co.initial_particles(case, mc.ngrids)
    data["dz"][:] = dz
    data["dt"][:] = float(case["dt"])
    co.execute(mc, data, kernels=case["kernels"], endtime=float(case["runtime"]), dt0=float(case["dt"]), context=co.rk45_context_defaults(case),
               seed=case.get("seed", 0))
    assert not np.any(data["state"] >= 50)
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("sdt", ["float64", "float32"])
def test_displacement_in_z_on_entry(gpu, sdt):
    """The 2-D stages never move z, but the step loop adds whatever dz a particle brings into the launch (ParticleSet(..., dz=...), or one an
    earlier kernel left) in its first position update: from the second step on the particle sits at another depth, several depth cells
    away or outside the grid, and depth index, depth weight, `ei` and the cached block of the first step must all go.  Lanes with dz = 0,
    and with a dz too small to change z, share the wavefronts."""
    case = _small("cr_dz_" + sdt, mesh="spherical", nz=7, npart=520, spatial_dtype=sdt, runtime=8 * 3600.0)
    n = len(case["x"])
    depth = case["depth"]
    rng = np.random.default_rng(12)
    dz = rng.uniform(-2500.0, 2500.0, n)       # up to three of the six depth cells
    dz[::5] = 0.0
    dz[1::25] = 1e-30                          # z + dz == z
    dz[2::40] = depth[-1]                      # below the bottom after the first step
    dz[3::40] = -depth[-1]                     # above the surface
    k = np.arange(4, n, 40)
    dz[k] = depth[k % len(depth)] - case["z"][k]  # onto a depth node, the first and the last among them
    dz = dz.astype(sdt)
    z1 = (case["z"].astype(sdt) + dz).astype(np.float64)
    inside = (z1 >= depth[0]) & (z1 <= depth[-1])
    cell0, cell1 = np.searchsorted(depth, case["z"]), np.searchsorted(depth, z1)
    assert (inside & (abs(cell1 - cell0) >= 2)).sum() > 50 and (~inside).sum() > 20 and (z1 == depth[0]).any() and (z1 == depth[-1]).any()
    on, son = _run_with_dz(case, dz, 2)
    off, soff = _run_with_dz(case, dz, 0)
    assert son["steps"] == soff["steps"] and son["attempts"] == soff["attempts"]
    compare(on, off, rtol=0.0, check_state="all", label="dz on entry: cache vs registers", skip=())
    assert np.array_equal(np.sort(on["particle_id"]), np.flatnonzero(inside)), "the particles left are those whose z + dz is inside the grid"
    assert np.array_equal(on["z"].astype(np.float64), z1[on["particle_id"]]) and not on["dz"].any()
    rtol = 5e-7 if sdt == "float32" else 1e-12
    scale = float(max(np.abs(case["lon"]).max(), np.abs(case["lat"]).max()))
    gen, sgen = _run_with_dz(case, dz, -1, fast=False)
    assert son["steps"] == sgen["steps"] and son["attempts"] == sgen["attempts"]
    compare(on, gen, rtol=rtol, atol_pos=rtol * scale, check_state="all", label="dz on entry: cache vs general", skip=())
    ref = _oracle_with_dz(case, dz)
    compare(on, ref, rtol=rtol, atol_pos=rtol * scale, check_state="all", label="dz on entry: cache vs oracle", skip=())
