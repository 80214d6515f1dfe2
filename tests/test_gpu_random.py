"""GPU: the counter-based random stream of user kernels on the device -- pk_random_fill against the NumPy restatement of
parcels_amd/random.py, `pa.random.*(pset)` on device-resident columns, and kernel lists with stochastic Python kernels compiled into the
fused step loop (structured interpreter, dedicated A-grid kernel with riders, UxGrid loop, CROCO sigma loop) against the same lists on the
host path (PARCELS_AMD_JIT=0): ONE launch per execute, the same particles deleted at the same times, positions bit-identical where only
`random` / `uniform` / `integers` enter and within the float64 parity bar where `normal` does."""
import os
import warnings

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import StatusCode
from parcels_amd import random as prandom
from parcels_amd.random import _variates

pytestmark = pytest.mark.gpu

EDGE_IDS = np.array([0, 1, 2**31, 2**32 + 5, 2**63 - 1, -1], dtype=np.int64)
EDGE_TIMES = np.array([0.0, -0.0, 600.0, -600.0, 1e9 + 0.5])
PROG_GENERIC, PROG_FAST_AGRID, PROG_UX, PROG_SIGMA = 2, 100, 6, 7  # include/parcels_hip.h: pk_exec_stats.program


def _ulps(a, b):
    """distance of two float64 arrays in units in the last place (ordered-integer difference)"""
    def key(v):
        i = np.asarray(v, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2**63) - i, i)
    return np.abs(key(a) - key(b))


@pytest.fixture(scope="module")
def engine(gpu):
    from test_gpu_jit_kernels import _fieldset

    fs = _fieldset("flat")
    return fs._engine_or_create()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_fill_equals_restatement(engine, n):
    ids = np.concatenate([EDGE_IDS, np.arange(300, dtype=np.int64) * 11 + 7])[:n]
    t = np.concatenate([np.repeat(EDGE_TIMES, 2)[: len(EDGE_IDS) + 3], np.arange(300) * 600.0])[:n]
    if n == 300:  # every edge id at every edge time
        ii, tt = (a.ravel() for a in np.meshgrid(EDGE_IDS, EDGE_TIMES, indexing="ij"))
        ids[:30], t[:30] = ii, tt
    worst = {"normal": 0, "exponential": 0}
    for seed, slot, draw in ((1, 0, 0), (2**40 + 7, 7, 3), (0, -1, 2)):
        w = prandom.words(seed, slot, draw, ids, t)
        fill = lambda dist, **kw: engine.random_fill(dist, seed, slot, draw, ids=ids, t=t, **kw)  # noqa: E731
        got = fill(prandom.PK_RANDOM_WORDS)
        assert got.shape == (n, 4) and got.dtype == np.uint32 and np.array_equal(got, w)
        assert np.array_equal(fill(prandom.PK_RANDOM_RANDOM), _variates(1, w))
        assert np.array_equal(fill(prandom.PK_RANDOM_UNIFORM, p0=-2.5, p1=3.5), _variates(2, w, np.float64(-2.5), np.float64(3.5)))
        for low, span in ((0, 10), (-7, 1), (-2**31, 2**32), (2**63 - 1, 1)):
            got = fill(prandom.PK_RANDOM_INTEGERS, ilow=low, span=span)
            assert got.dtype == np.int64 and np.array_equal(got, _variates(6, w, np.int64(low), np.uint64(span)))
        for name, dist, p0, p1 in (("normal", 3, 0.0, 0.0), ("normal", 4, 1.5, 0.25), ("exponential", 5, 2.0, 0.0)):
            got, want = fill(dist, p0=p0, p1=p1), _variates(dist, w, np.float64(p0), np.float64(p1))
            assert np.abs(got - want).max() <= 1e-12, (name, np.abs(got - want).max())
            worst[name] = max(worst[name], int(_ulps(got, want).max()))
    print(f"pk_random_fill, n = {n}: largest ulp distance to the restatement {worst}")


def test_fill_refuses_what_the_host_refuses(engine):
    from parcels_amd import _hip

    ids, t = np.arange(4, dtype=np.int64), np.zeros(4)
    with pytest.raises(_hip.HipLibraryError, match="1 <= span <= 2\\^32"):
        engine.random_fill(prandom.PK_RANDOM_INTEGERS, 1, 0, 0, ilow=0, span=2**32 + 1, ids=ids, t=t)
    with pytest.raises(_hip.HipLibraryError, match="1 <= span <= 2\\^32"):
        engine.random_fill(prandom.PK_RANDOM_INTEGERS, 1, 0, 0, ilow=0, span=0, ids=ids, t=t)
    with pytest.raises(_hip.HipLibraryError, match="draw must not be negative"):
        engine.random_fill(prandom.PK_RANDOM_RANDOM, 1, 0, -1, ids=ids, t=t)


# ---- the kernels (module level: the translator reads their source) ------------------------------------------------------------------------------
def Mortality(particles, fieldset):
    particles.state = np.where(pa.random.random(particles) < fieldset.p_die, StatusCode.Delete, particles.state)


def RandomWalk(particles, fieldset):
    particles.dx += pa.random.normal(0.0, fieldset.sigma, particles)
    particles.dy += pa.random.normal(0.0, fieldset.sigma, particles)


def DrawSelection(particles, fieldset):
    """a draw for a selection, a draw kept across a field sample (of the float32 field S: the kernel-list interpreter), integers"""
    kept = pa.random.random(particles)
    east = particles[particles.x > fieldset.x0]
    east.acc = prandom.uniform(1.0, 2.0, east)
    s = fieldset.S[particles]
    particles.speed = kept * s + pa.random.uniform(s, s + 1.0, particles)
    particles.flag = pa.random.integers(-3, 12, particles)
    particles[kept < 0.02].state = StatusCode.Delete


CONTEXT = {"p_die": 0.03, "sigma": 50.0, "x0": 2.0e4}


def _run(kernels, *, jit, spatial=np.float64, n=300, steps=12, dt=600.0, late=True, seed=5, sort=False, calls=1):
    from test_gpu_jit_kernels import _fieldset, _pclass

    old = os.environ.get("PARCELS_AMD_JIT")
    os.environ["PARCELS_AMD_JIT"] = "1" if jit else "0"
    try:
        fs = _fieldset("flat")
        for k, v in CONTEXT.items():
            fs.add_context(k, v)
        rng = np.random.default_rng(1)
        lon, lat = np.asarray(fs.U.grid.lon), np.asarray(fs.U.grid.lat)
        x = lon[0] + (0.15 + 0.7 * rng.uniform(size=n)) * (lon[-1] - lon[0])
        y = lat[0] + (0.15 + 0.7 * rng.uniform(size=n)) * (lat[-1] - lat[0])
        t0 = np.where(np.arange(n) % 4 == 0, abs(dt), 0.0) if late else np.zeros(n)  # (a quarter of the particles start one step late)
        pset = pa.ParticleSet(fs, pclass=_pclass(spatial), x=x, y=y, t=t0, seed=seed, sort_by_cell=sort)
        stats = []
        for _ in range(calls):
            pset.execute(kernels, runtime=steps * abs(dt) / calls, dt=dt)
            stats.append(dict(pset._last_stats))
        return pset, {k: np.array(v) for k, v in pset._data.items()}, stats
    finally:
        if old is None:
            os.environ.pop("PARCELS_AMD_JIT", None)
        else:
            os.environ["PARCELS_AMD_JIT"] = old


def _by_id(d):
    o = np.argsort(d["particle_id"], kind="stable")
    return {k: v[o] for k, v in d.items()}


def _assert_same(dj, dh, exact, rtol=None, scale=None):
    """the same particles left, in the same states at the same times; float columns bit for bit or as |a - b| <= rtol * scale"""
    dj, dh = _by_id(dj), _by_id(dh)
    assert np.array_equal(dj["particle_id"], dh["particle_id"])
    for k in ("state", "t", "dt"):
        assert np.array_equal(dj[k], dh[k]), k
    for k in dj:
        assert dj[k].dtype == dh[k].dtype, k
        if exact or dj[k].dtype.kind != "f":
            assert np.array_equal(dj[k], dh[k], equal_nan=True), (k, np.flatnonzero(dj[k] != dh[k])[:5])
        else:
            err = float(np.abs(dj[k].astype(np.float64) - dh[k].astype(np.float64)).max()) if len(dj[k]) else 0.0
            print(f"{k}: largest |compiled - host| = {err:.3g} (bound {rtol * scale:.3g})")
            assert err <= rtol * scale, (k, err)


def _both(kernels, exact, program=None, spatial=np.float64, **kw):
    pj, dj, sj = _run(kernels, jit=True, spatial=spatial, **kw)
    ph, dh, sh = _run(kernels, jit=False, spatial=spatial, **kw)
    assert pj._kernel.user_program is not None and not pj._kernel.host_functions, pj._kernel.jit_report
    assert all(s["launches"] == 1 and not s.get("hosted") for s in sj), sj  # ONE launch per execute
    assert ph._kernel.user_program is None and all(s.get("hosted") for s in sh), ph._kernel.jit_report
    if program is not None:
        assert sj[-1]["program"] == program, sj[-1]
    # (tests/case_utils.py: tolerance_for -- 1e-12 of the coordinate scale for float64 storage, one float32 ulp, 5e-7, for float32)
    _assert_same(dj, dh, exact, rtol=5e-7 if spatial == np.float32 else 1e-12, scale=4.0e4)
    return pj, dj


@pytest.mark.parametrize("spatial", [np.float32, np.float64])
def test_mortality_rides_in_the_dedicated_agrid_kernel(gpu, spatial):
    """[AdvectionRK4, Mortality] on a rectilinear A-grid: ONE launch of the dedicated A-grid kernel, the user kernel riding along (it samples
    no field); `random` is bit-identical on both paths, so every column is."""
    p, d = _both([pa.AdvectionRK4, Mortality], exact=True, program=PROG_FAST_AGRID, spatial=spatial)
    assert p._kernel.user_program.flags & 1
    assert 0 < len(p) < 300  # some died, at the steps the host path killed them


@pytest.mark.parametrize("spatial", [np.float32, np.float64])
def test_random_walk_and_mortality(gpu, spatial):
    p, d = _both([pa.AdvectionRK4, RandomWalk, Mortality], exact=False, spatial=spatial)
    assert 0 < len(p) < 300


def test_selection_and_draw_kept_across_a_sample(gpu):
    """the kernel-list interpreter (S is float32, U float64: no dedicated kernel); random / uniform / integers only: bit for bit"""
    p, d = _both([pa.AdvectionRK4, DrawSelection], exact=True, program=PROG_GENERIC)
    assert 0 < len(p) < 300 and len(np.unique(d["flag"])) > 5 and d["flag"].min() >= -3 and d["flag"].max() < 12
    drawn = d["acc"] != 0  # (who was east of x0 at some step)
    assert drawn.any() and not drawn.all() and np.all((d["acc"][drawn] >= 1.0) & (d["acc"][drawn] < 2.0))


def test_backward_run_from_t_zero(gpu):
    """dt < 0 from t = 0: negative times in the counter (and t = 0 itself, where -0.0 and 0.0 are one time)"""
    p, d = _both([RandomWalk, Mortality], exact=False, dt=-600.0, late=False)
    assert 0 < len(p) < 300 and np.all(d["t"] == -7200.0)


def test_cell_sort_and_call_cuts_do_not_change_the_numbers(gpu):
    """the stream is a function of (seed, kernel position, draw, id, t): the cell sort reorders the device rows, two execute calls cut the
    launch in two -- per id nothing changes, bit for bit; another seed does"""
    kernels = [pa.AdvectionRK4, RandomWalk, Mortality]
    _, plain, _ = _run(kernels, jit=True)
    ps, sorted_, stats = _run(kernels, jit=True, sort=True)
    assert ps.sort_by_cell and all(s["launches"] == 1 for s in stats)
    _assert_same(sorted_, plain, exact=True)
    _, cut, stats = _run(kernels, jit=True, calls=2)
    assert len(stats) == 2 and all(s["launches"] == 1 for s in stats)
    _assert_same(cut, plain, exact=True)
    _, other, _ = _run(kernels, jit=True, seed=6)
    assert not np.array_equal(np.sort(other["particle_id"]), np.sort(plain["particle_id"])) or not np.array_equal(_by_id(other)["x"], _by_id(plain)["x"])


def test_draws_for_a_resident_particleset(gpu):
    """pa.random.uniform(0, 1, pset) on device-resident columns (pk_random_fill reads particle_id and t where they are) equals the
    restatement on the downloaded columns -- before and after an execute that cell-sorts the device rows; nothing is downloaded for it."""
    from parcels_amd.columns import LazyColumns
    from test_gpu_jit_kernels import _fieldset, _pclass

    fs = _fieldset("flat")
    n = 300
    rng = np.random.default_rng(2)
    lon, lat = np.asarray(fs.U.grid.lon), np.asarray(fs.U.grid.lat)
    pset = pa.ParticleSet(fs, pclass=_pclass(np.float64), x=lon[0] + (0.2 + 0.6 * rng.uniform(size=n)) * (lon[-1] - lon[0]),
                          y=lat[0] + (0.2 + 0.6 * rng.uniform(size=n)) * (lat[-1] - lat[0]), t=np.where(np.arange(n) % 4 == 0, 600.0, 0.0),
                          particle_ids=rng.permutation(n).astype(np.int64) * 3 + 1, seed=9, sort_by_cell=False)
    pset.resident_columns = True
    host = pa.random.uniform(0.0, 1.0, pset)  # not resident yet: the restatement
    assert np.array_equal(host, _variates(1, prandom.words(9, -1, 0, pset._data["particle_id"], pset._data["t"])))
    pset.execute([pa.AdvectionRK4], runtime=1800.0, dt=600.0)
    for sort in (False, True):
        if sort:
            pset.sort_by_cell = True
            pset.execute([pa.AdvectionRK4], runtime=1800.0, dt=600.0)
        data = pset._data
        assert isinstance(data, LazyColumns) and data.resident() and "t" in data._stale
        u = pa.random.uniform(0.0, 1.0, pset)
        k = pa.random.integers(0, 10, pset, stream=3)
        z = pa.random.normal(np.linspace(-1, 1, n), 2.0, pset, stream=1)
        assert "t" in data._stale  # (drawn on the device: the time column was not downloaded)
        ids, t = np.array(data["particle_id"]), np.array(data["t"])
        assert np.array_equal(u, _variates(1, prandom.words(9, -1, 0, ids, t)))
        assert np.array_equal(k, _variates(6, prandom.words(9, -1, 3, ids, t), np.int64(0), np.uint64(10)))
        assert np.abs(z - _variates(4, prandom.words(9, -1, 1, ids, t), np.linspace(-1, 1, n), np.float64(2.0))).max() <= 1e-12
        assert not np.array_equal(u, host)  # (everybody stands at another time now)


# ---- the other two step loops ------------------------------------------------------------------------------------------------------------------
def _ux_run(monkeypatch, jit):
    from tools import make_ux_kernels_golden as gk
    from ux_kernels_utils import run_uxk

    monkeypatch.setenv("PARCELS_AMD_JIT", "1" if jit else "0")
    base = dict(gk.cases()["uxk_flat_face_em"])
    lon, lat = base["node_lon"], base["node_lat"]
    n = 130
    rng = np.random.default_rng(230)
    x = lon.min() + rng.uniform(0.2, 0.65, n) * (lon.max() - lon.min())
    y = lat.min() + rng.uniform(0.2, 0.8, n) * (lat.max() - lat.min())
    case = dict(base, x=x, y=y, z=np.full(n, 0.5), spatial_dtype="float64", seed=5, runtime=10 * base["dt"], outputdt=None,
                context=dict(base["context"], p_die=0.03))
    d, err, _, pset = run_uxk(case, kernels=[pa.AdvectionRK4, Mortality])
    assert err is None
    return d, pset, n


def test_mortality_in_the_uxgrid_loop(gpu, monkeypatch):
    dj, pj, n = _ux_run(monkeypatch, jit=True)
    k = pj._kernel
    assert str(k.jit_report).startswith("compiled") and k.host_functions == [] and k.user_program.ux, k.jit_report
    assert pj._last_stats["program"] == PROG_UX and pj._last_stats["launches"] == 1 and not pj._last_stats.get("hosted")
    dh, ph, _ = _ux_run(monkeypatch, jit=False)
    assert ph._kernel.user_program is None and ph._last_stats.get("hosted")
    _assert_same(dj, dh, exact=True)
    assert 0 < len(dj["x"]) < n


def _croco_run(monkeypatch, jit):
    from croco_utils import croco_fieldset
    from tools import make_croco_golden as mg

    monkeypatch.setenv("PARCELS_AMD_JIT", "1" if jit else "0")
    case = mg.load(os.path.join(mg.GOLDEN, "croco_rect_flat_f64data_f64part.npz"))
    reps = -(-130 // len(case["x"]))
    x, y, z = (np.tile(np.asarray(case[k]), reps)[:130] for k in "xyz")
    fs = croco_fieldset(case)
    fs.add_context("p_die", 0.03)
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x, y=y, z=z, t=np.zeros(130), seed=5, sort_by_cell=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pset.execute([pa.AdvectionRK2_3D_CROCO, Mortality], dt=float(case["dt"]), runtime=float(case["runtime"]))
    return {k: np.array(v) for k, v in pset._data.items()}, pset


def test_mortality_in_the_croco_sigma_loop(gpu, monkeypatch):
    dj, pj = _croco_run(monkeypatch, jit=True)
    k = pj._kernel
    assert str(k.jit_report).startswith("compiled") and k.host_functions == [] and k.user_program.sigma, k.jit_report
    assert pj._last_stats["program"] == PROG_SIGMA and pj._last_stats["launches"] == 1 and not pj._last_stats.get("hosted")
    dh, ph = _croco_run(monkeypatch, jit=False)
    assert ph._kernel.user_program is None and ph._last_stats.get("hosted")
    _assert_same(dj, dh, exact=True)
    assert 0 < len(dj["x"]) < 130
