"""GPU: the built-in interaction kernels pa.AttractTowards / pa.MergeNearest on the device-resident particle columns
(parcels_amd/interactkernels.py, csrc/pk_interact.hip) against two yardsticks written here, independent of the new code:

(a) the same kernels as Python functions on pa.neighbors / pa.nearest_neighbor, run through the host loop (hostkernels.execute_hosted);
(b) dense all-pairs NumPy in float64 (the formulation of attract_dense / merge_dense in tests/test_gpu_interaction.py, with the merge
    rule "the heavier of a mutual pair keeps the mass, equal masses: the lower index").

On flat meshes the device path equals both EXACTLY (np.array_equal) in every column: particle order and ids after deletion, user
Variables, dtype and shape.  On spherical meshes the discrete columns are exact and positions and mass are compared to 1e-12 of the
coordinate scale (the bar of tests/test_gpu_interaction_sph.py), after the preconditions of that file were asserted on (b) alone."""

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd.statuscodes import StatusCode
from parcels_amd.xgrid import EARTH_RADIUS

pytestmark = pytest.mark.gpu

RAD = np.pi / 180


# ---- yardstick (a): Python kernels on the search calls, typed out again ---------------------------------------------------------------
def attract_py(sources, radius, velocity, z=False, mesh="flat", max_pairs=None):
    def attract(particles, fieldset):
        nb = pa.neighbors(particles, radius, z=z, mesh=mesh, max_pairs=max_pairs, sources=np.asarray(getattr(particles, sources)) != 0,
                          include_coincident=False)
        particles.dx += nb.sum(nb.dx / nb.dist) * velocity * particles.dt
        particles.dy += nb.sum(nb.dy / nb.dist) * velocity * particles.dt
        if z:
            particles.dz += nb.sum(nb.dz / nb.dist) * velocity * particles.dt

    return attract


def _merge_rule(particles, j, mass):
    i = np.arange(len(j))
    mutual = (j >= 0) & (j[np.where(j >= 0, j, 0)] == i) & (i < j)
    pi, pj = i[mutual], j[mutual]
    m = getattr(particles, mass)
    big = np.where(m[pj] > m[pi], pj, pi)
    small = np.where(m[pj] > m[pi], pi, pj)
    m[big] += m[small]
    particles.state[small] = int(StatusCode.Delete)


def merge_py(mass, radius, z=False, mesh="flat"):
    def merge(particles, fieldset):
        j, _ = pa.nearest_neighbor(particles, radius, z=z, mesh=mesh, include_coincident=False)
        _merge_rule(particles, j, mass)

    return merge


# ---- yardstick (b): dense all-pairs NumPy ------------------------------------------------------------------------------------------------
DENSE_LOG = []  # (distance matrix, radius) of every dense call on a sphere: the preconditions are asserted on these


def _dense(particles, z, sphere):
    """(dx, dy, dz | None, dist) as n x n float64 matrices, entry [i, j] = from i to j; invalid pairs have dist = inf"""
    x, y = np.asarray(particles.x, dtype=np.float64), np.asarray(particles.y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dy = y[None, :] - y[:, None]
        d = x[None, :] - x[:, None]
        if sphere is None:
            dx = d
            s = dx * dx + dy * dy
            dz = None
            if z:
                zz = np.asarray(particles.z, dtype=np.float64)
                dz = zz[None, :] - zz[:, None]
                s = s + dz * dz
            dist = np.sqrt(s)
        else:
            dx = d - 360 * np.rint(d / 360)
            a = np.sin(0.5 * RAD * dy) ** 2 + np.cos(RAD * y[:, None]) * np.cos(RAD * y[None, :]) * np.sin(0.5 * RAD * dx) ** 2
            dist = 2 * sphere * np.arcsin(np.minimum(1, np.sqrt(a)))
            dz = None
            if z:
                zz = np.asarray(particles.z, dtype=np.float64)
                dz = zz[None, :] - zz[:, None]
                dist = np.sqrt(dist * dist + dz * dz)
            valid = np.isfinite(x) & np.isfinite(y) & (np.abs(y) <= 90)
            dist = np.where(valid[:, None] & valid[None, :], dist, np.inf)
        dist = np.where(np.isnan(dist), np.inf, dist)
    np.fill_diagonal(dist, np.inf)
    return dx, dy, dz, dist


def attract_dense(sources, radius, velocity, z=False, sphere=None):
    def attract(particles, fieldset):
        dx, dy, dz, dist = _dense(particles, z, sphere)
        if sphere is not None:
            DENSE_LOG.append((dist, radius))
        n = dist.shape[0]
        pull = (dist < radius) & (dist > 0) & (np.asarray(getattr(particles, sources)) != 0)[None, :]
        i, j = np.nonzero(pull)  # row-major: i ascends, j ascends within a row
        particles.dx += np.bincount(i, weights=dx[i, j] / dist[i, j], minlength=n) * velocity * particles.dt
        particles.dy += np.bincount(i, weights=dy[i, j] / dist[i, j], minlength=n) * velocity * particles.dt
        if z:
            particles.dz += np.bincount(i, weights=dz[i, j] / dist[i, j], minlength=n) * velocity * particles.dt

    return attract


def merge_dense(mass, radius, z=False, sphere=None):
    def merge(particles, fieldset):
        _, _, _, dist = _dense(particles, z, sphere)
        if sphere is not None:
            DENSE_LOG.append((dist, radius))
        masked = np.where((dist < radius) & (dist > 0), dist, np.inf)
        j = np.argmin(masked, axis=1).astype(np.int64)  # the first minimum: ties to the smallest j
        j[np.isinf(masked[np.arange(len(j)), j])] = -1
        _merge_rule(particles, j, mass)

    return merge


# ---- harness ---------------------------------------------------------------------------------------------------------------------------
_FS = {}


def fieldset(name="agrid_flat_rk4_f64"):
    from case_utils import build_fieldset, load_golden

    if name not in _FS:
        case, _, _ = load_golden(name)
        _FS[name] = (build_fieldset(case), np.asarray(case["lon"], dtype=np.float64), np.asarray(case["lat"], dtype=np.float64))
    return _FS[name]


def pclass(spatial=np.float64, mass=np.float64, source=np.bool_):
    return pa.get_default_particle(spatial).add_variable([pa.Variable("attractor", dtype=source, initial=0),
                                                          pa.Variable("mass", dtype=mass, initial=1.0)])


def run(kernels, x, y, *, fs=None, P=None, z=None, t=None, attractor=None, mass=None, dt=1.0, runtime=5.0, output=None):
    fs = fieldset()[0] if fs is None else fs
    P = pclass() if P is None else P
    n = len(x)
    kw = {} if z is None else {"z": np.array(z)}
    pset = pa.ParticleSet(fs, pclass=P, x=np.array(x), y=np.array(y), t=np.zeros(n) if t is None else np.array(t, dtype=np.float64), **kw)
    if attractor is not None:
        pset._data["attractor"][:] = attractor
    if mass is not None:
        pset._data["mass"][:] = mass
    pset.execute(kernels, dt=dt, runtime=runtime, **({} if output is None else {"output_file": output}))
    out = {k: np.array(pset._data[k]) for k in pset._data}
    out["_stats"] = dict(pset._last_stats) if getattr(pset, "_last_stats", None) else None
    return out


def assert_same(a, b, what):
    assert sorted(k for k in a if k != "_stats") == sorted(k for k in b if k != "_stats"), what
    for k in a:
        if k == "_stats":
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k], equal_nan=(a[k].dtype.kind == "f")), (what, k)


def three_ways(before, tokens, x, y, **kw):
    """`before` (built-in kernels) + the interaction kernels of `tokens` = [("attract", kwargs) | ("merge", kwargs)] as the device path and
    as both yardsticks; asserts exact equality and returns the device result."""
    make = {"attract": (pa.AttractTowards, attract_py, attract_dense), "merge": (pa.MergeNearest, merge_py, merge_dense)}
    lists = [list(before) + [make[kind][w](**args) for kind, args in tokens] for w in range(3)]
    dev = run(lists[0], x, y, **kw)
    assert dev["_stats"]["hosted"] is False
    for name, kernels in (("python kernels on the search calls", lists[1]), ("dense NumPy", lists[2])):
        ref = run(kernels, x, y, **kw)
        assert ref["_stats"]["hosted"] is True
        assert_same(dev, ref, name)
    return dev


def square(n, seed):
    _, lon, lat = fieldset()
    rng = np.random.default_rng(seed)
    return lon.min() + rng.random(n), lat.min() + rng.random(n), rng


ATTRACT = {"sources": "attractor", "radius": 0.12, "velocity": 0.004}
MERGE = {"mass": "mass", "radius": 0.03}


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_sizes(gpu, n):
    x, y, rng = square(n, 100 + n)
    src = rng.random(n) < 0.3
    src[0] = True
    dev = three_ways([pa.MoveEast], [("attract", dict(ATTRACT, radius=0.3))], x, y, attractor=src, runtime=3.0)
    assert len(dev["x"]) == n and np.all(dev["t"] == 3.0)
    if n > 2:
        assert np.any(dev["y"] != y)  # MoveEast leaves y alone: the attraction moved it


def test_end_to_end(gpu):
    x, y, rng = square(400, 12)
    src = np.zeros(400, dtype=bool)
    src[rng.choice(400, 12, replace=False)] = True
    kernels = [pa.AdvectionRK4, pa.AttractTowards(**ATTRACT), pa.MergeNearest(**MERGE)]
    dev = three_ways([pa.AdvectionRK4], [("attract", ATTRACT), ("merge", MERGE)], x, y, attractor=src, runtime=10.0)
    # particles merged, and went on merging after the first step, on views that had shrunk.  No lower bound on the survivors: one merge pass
    # can delete up to half of the rows, and how many of 400 the flow and the 12 sources bring within 0.03 of each other is what the
    # yardsticks say (three_ways compared every column with them), not something to guess here
    first = run(kernels, x, y, attractor=src, runtime=1.0)
    assert 200 <= len(first["particle_id"]) < 400  # one pass deletes one row of a mutual pair: at most half
    assert 1 <= len(dev["particle_id"]) < len(first["particle_id"])
    assert dev["mass"].sum() == 400.0 and dev["mass"].max() >= 2.0
    only_advected = run([pa.AdvectionRK4], x, y, runtime=10.0)
    moved = np.abs(dev["x"] - only_advected["x"][dev["particle_id"]]).max()
    assert moved > 5 * ATTRACT["velocity"]  # and were attracted


def test_strict_radius_and_cell_edges(gpu):
    _, lon, lat = fieldset()
    gy, gx = np.divmod(np.arange(36), 6)
    x, y = lon.min() + 0.25 * gx, lat.min() + 0.25 * gy  # multiples of 0.25: exact, so the lattice neighbours sit exactly at the radius
    # sources in the adjacent cell and just across a cell edge (cells are a hair wider than the radius, from the smallest coordinate)
    eps = 2.0 ** -20
    x = np.concatenate([x, lon.min() + np.array([0.25 - eps, 0.25 + eps, 0.5 + eps, 0.76])])
    y = np.concatenate([y, lat.min() + np.array([0.25 + eps, 0.25 - eps, 0.49, 0.5 - eps])])
    src = np.ones(len(x), dtype=bool)
    dev = three_ways([pa.DoNothing], [("attract", dict(ATTRACT, radius=0.25))], x, y, attractor=src, runtime=2.0)
    # the far corner of the lattice has only lattice neighbours, all exactly at the radius: excluded, it did not move
    assert dev["x"][35] == x[35] and dev["y"][35] == y[35]
    assert np.any(dev["x"][:35] != x[:35])


def test_coincident_points(gpu):
    x, y, rng = square(40, 31)
    x[10:20], y[10:20] = x[:10], y[:10]  # ten particles on top of ten others, sources among them
    src = np.zeros(40, dtype=bool)
    src[5:15] = True
    dev = three_ways([pa.DoNothing], [("attract", dict(ATTRACT, radius=0.4))], x, y, attractor=src, runtime=2.0)
    assert np.isfinite(dev["x"]).all() and np.isfinite(dev["y"]).all()


def test_non_finite_coordinates(gpu):
    x, y, rng = square(50, 32)
    x[7] = np.nan
    src = np.ones(50, dtype=bool)
    dev = three_ways([pa.DoNothing], [("attract", dict(ATTRACT, radius=0.4))], x, y, attractor=src, runtime=2.0)
    assert np.isnan(dev["x"][7]) and np.isfinite(np.delete(dev["x"], 7)).all() and np.isfinite(dev["y"]).all()
    alone = run([pa.DoNothing, pa.AttractTowards(**dict(ATTRACT, radius=0.4))], np.delete(x, 7), np.delete(y, 7), attractor=np.delete(src, 7), runtime=2.0)
    assert np.array_equal(np.delete(dev["x"], 7), alone["x"]) and np.array_equal(np.delete(dev["y"], 7), alone["y"])  # nobody's neighbour


@pytest.mark.parametrize("dt", [1.0, -1.0])
def test_shrinking_views(gpu, dt):
    x, y, rng = square(120, 33)
    t = rng.integers(0, 5, 120).astype(np.float64)  # staggered: particles reach endtime in different iterations
    if dt < 0:
        t = 10.0 - t
    src = rng.random(120) < 0.2
    dev = three_ways([pa.DoNothing], [("attract", dict(ATTRACT, radius=0.2)), ("merge", dict(MERGE, radius=0.06))], x, y, t=t, attractor=src, dt=dt,
                     runtime=6.0)
    assert np.all(dev["t"] == (6.0 if dt > 0 else 4.0)) and len(dev["x"]) < 120


@pytest.mark.parametrize("mdt", [np.float32, np.float64])
def test_merge_rules(gpu, mdt):
    _, lon, lat = fieldset()
    x0, y0 = lon.min() + 0.5, lat.min() + 0.5
    # one mutual pair (0, 1); a chain 2-3-4 where 3 and 4 are mutual and 2's nearest is 3; equal distances 5-6-7-8 on a line: the smallest j;
    # 9 alone.  Offsets are multiples of 2^-10: the distances that must tie do so exactly.
    u = 2.0 ** -10
    x = x0 + np.array([0, 4 * u, 0.1, 0.1 + 6 * u, 0.1 + 10 * u, 0.2, 0.2 + 4 * u, 0.2 + 8 * u, 0.2 + 12 * u, 0.4])
    y = y0 + np.array([0, 0, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 0.2, 0.4])
    mass = np.array([1, 3, 1, 2, 2, 1, 1, 1, 1, 5], dtype=mdt) + mdt(0.1)  # 0.1: the sums round differently in float32 and float64
    dev = three_ways([pa.DoNothing], [("merge", dict(MERGE, radius=0.02))], x, y, P=pclass(mass=mdt), mass=mass, runtime=1.0)
    assert dev["mass"].dtype == mdt
    # 0-1: the heavier (1) keeps; 3-4: equal masses, the lower index (3) keeps, 2 is left alone; 5-6 mutual (6's nearest: 5 before 7), then
    # 7-8 mutual (7's nearest is 6 -- the smallest j of its two equal distances -- so 7 is NOT mutual with 8; 8's nearest is 7): only 5-6
    assert dev["particle_id"].tolist() == [1, 2, 3, 5, 7, 8, 9]
    assert dev["mass"].tolist() == [mass[1] + mass[0], mass[2], mass[3] + mass[4], mass[5] + mass[6], mass[7], mass[8], mass[9]]


def test_deleted_particle_is_absent_from_the_next_search(gpu):
    _, lon, lat = fieldset()
    u = 2.0 ** -10
    # 0 and 1 merge in iteration 1 (1 is deleted).  2's nearest is 1 while 1 exists, so 2 merges with 3 only from iteration 2 on
    x = lon.min() + 0.5 + np.array([0, 4 * u, 10 * u, 18 * u])
    y = lat.min() + 0.5 + np.zeros(4)
    mass = np.array([4.0, 1.0, 2.0, 1.0])
    dev = three_ways([pa.DoNothing], [("merge", dict(MERGE, radius=0.01))], x, y, mass=mass, runtime=1.0)
    assert dev["particle_id"].tolist() == [0, 2, 3] and dev["mass"].tolist() == [5.0, 2.0, 1.0]
    dev = three_ways([pa.DoNothing], [("merge", dict(MERGE, radius=0.01))], x, y, mass=mass, runtime=2.0)
    assert dev["particle_id"].tolist() == [0, 2] and dev["mass"].tolist() == [5.0, 3.0]


@pytest.mark.parametrize("z", [False, True])
def test_float32_storage(gpu, z):
    x, y, rng = square(150, 34 + z)
    zz = (rng.random(150) * 0.2).astype(np.float32)
    src = rng.random(150) < 0.2
    P = pclass(spatial=np.float32, mass=np.float32, source=np.int32)  # the default particle class stores positions in float32
    dev = three_ways([pa.MoveNorth], [("attract", dict(ATTRACT, radius=0.2, z=z)), ("merge", dict(MERGE, radius=0.05, z=z))],
                     x.astype(np.float32), y.astype(np.float32), z=zz, P=P, attractor=src.astype(np.int32), runtime=4.0)
    assert dev["x"].dtype == np.float32 and dev["dx"].dtype == np.float32 and len(dev["x"]) < 150
    if z:
        assert np.any(dev["z"] != zz[dev["particle_id"]])


def test_particlefile_tables(gpu, tmp_path):
    x, y, rng = square(100, 36)
    src = rng.random(100) < 0.2
    tables = []
    for w, (mk_a, mk_m) in enumerate(((pa.AttractTowards, pa.MergeNearest), (attract_py, merge_py))):
        pf = pa.ParticleFile(tmp_path / f"out{w}.parquet", outputdt=2.0)
        got = run([pa.MoveEast, mk_a(**ATTRACT), mk_m(**dict(MERGE, radius=0.05))], x, y, attractor=src, runtime=10.0, output=pf)
        assert got["_stats"]["hosted"] is bool(w)
        tables.append(pa.read_particlefile(tmp_path / f"out{w}.parquet"))
    a, b = tables
    assert len(a) > 300  # a table every 2 steps of the 10-step run, the first at the start
    assert list(a.columns) == list(b.columns) and a.equals(b)


def test_no_column_crosses_pcie_inside_launch(gpu, monkeypatch):
    from parcels_amd.engine import DeviceEngine
    from parcels_amd.kernel import Kernel

    x, y, rng = square(200, 37)
    src = rng.random(200) < 0.2
    calls = []
    inside = []
    for name in ("h2d", "d2h", "h2d_columns"):
        orig = getattr(DeviceEngine, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if inside:
                calls.append(_name)
            return _orig(self, *a, **k)

        monkeypatch.setattr(DeviceEngine, name, counted)
    launch = Kernel.launch

    def watched(self, *a, **k):
        inside.append(1)
        try:
            return launch(self, *a, **k)
        finally:
            inside.pop()

    monkeypatch.setattr(Kernel, "launch", watched)
    got = run([pa.AdvectionRK4, pa.AttractTowards(**ATTRACT), pa.MergeNearest(**MERGE)], x, y, attractor=src, runtime=5.0)
    assert got["_stats"]["hosted"] is False and calls == []
    calls.clear()
    run([pa.AdvectionRK4, attract_py(**ATTRACT), merge_py(**MERGE)], x, y, attractor=src, runtime=2.0)
    assert "h2d" in calls and "d2h" in calls  # the counter sees the host loop's round trips


def test_list_with_a_python_function_runs_hosted(gpu):
    def age(particles, fieldset):
        particles.mass += 0.0 * particles.dt

    x, y, rng = square(90, 38)
    src = rng.random(90) < 0.2
    a = run([pa.MoveEast, pa.AttractTowards(**ATTRACT), age, pa.MergeNearest(**dict(MERGE, radius=0.05))], x, y, attractor=src, runtime=4.0)
    b = run([pa.MoveEast, attract_py(**ATTRACT), age, merge_py(**dict(MERGE, radius=0.05))], x, y, attractor=src, runtime=4.0)
    assert a["_stats"]["hosted"] is True and b["_stats"]["hosted"] is True
    assert_same(a, b, "token bodies in the host loop")
    assert len(a["x"]) < 90


def test_max_pairs(gpu):
    x, y, rng = square(100, 39)
    src = np.ones(100, dtype=bool)
    with pytest.raises(ValueError, match=r"max_pairs: \d+ neighbour pairs exceed the cap of 5 \(max_pairs\)"):
        run([pa.DoNothing, pa.AttractTowards(**dict(ATTRACT, radius=0.3, max_pairs=5))], x, y, attractor=src, runtime=1.0)


# ---- spherical ---------------------------------------------------------------------------------------------------------------------------
def assert_preconditions():
    """on yardstick (b) alone: membership and the arg-min do not hinge on the last ulps of sin / cos / arcsin"""
    assert DENSE_LOG
    for dist, radius in DENSE_LOG:
        finite = np.isfinite(dist)
        assert not (np.abs(dist[finite] / radius - 1) <= 1e-9).any(), "a pair sits within 1e-9 of a radius: choose another seed"
        if dist.shape[0] < 3:
            continue
        two = np.sort(np.where((dist < radius) & (dist > 0), dist, np.inf), axis=1)[:, :2]
        d1, d2 = two[:, 0], two[:, 1]
        both = np.isfinite(d2)
        d2 = np.where(both, d2, 1.0)
        d1 = np.where(both, d1, 0.0)
        assert not (both & (np.abs(d2 - d1) <= 1e-9 * d2) & (d1 != d2)).any(), "a row's two nearest are within 1e-9: choose another seed"


def sphere_points(which):
    rng = np.random.default_rng({"antimeridian": 41, "antimeridian_mixed": 42, "north": 43}[which])
    n = 150
    if which == "north":
        return rng.uniform(-180, 180, n), rng.uniform(88.6, 89.4, n), rng
    x = 180 + rng.uniform(-0.5, 0.5, n)  # straddles 180 E
    if which == "antimeridian_mixed":
        x = np.where(rng.random(n) < 0.5, x, x - 360)  # the same meridians written as -180.5 .. -179.5
    else:
        x = np.where(x > 180, x - 360, x)
    return x, rng.uniform(-0.5, 0.5, n), rng


@pytest.mark.parametrize("which", ["antimeridian", "antimeridian_mixed", "north"])
def test_spherical(gpu, which):
    fs, _, _ = fieldset("agrid_sph_rk4_f64")
    x, y, rng = sphere_points(which)
    src = rng.random(len(x)) < 0.2
    a_args = {"sources": "attractor", "radius": 20e3, "velocity": 300.0}
    m_args = {"mass": "mass", "radius": 5e3}
    kw = dict(fs=fs, attractor=src, runtime=5.0)
    del DENSE_LOG[:]
    dense = run([pa.DoNothing, attract_dense(**a_args, sphere=EARTH_RADIUS), merge_dense(**m_args, sphere=EARTH_RADIUS)], x, y, **kw)
    assert_preconditions()
    assert len(dense["x"]) < len(x) and np.abs(dense["y"] - y[dense["particle_id"]]).max() > 1e-3  # merged and moved
    dev = run([pa.DoNothing, pa.AttractTowards(**a_args, mesh=fs), pa.MergeNearest(**m_args, mesh=fs)], x, y, **kw)
    assert dev["_stats"]["hosted"] is False
    py = run([pa.DoNothing, attract_py(**a_args, mesh=fs), merge_py(**m_args, mesh=fs)], x, y, **kw)
    for name, ref in (("python kernels on the search calls", py), ("dense NumPy", dense)):
        identical = True
        for k in dev:
            if k == "_stats":
                continue
            assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (name, k)
            if k in ("x", "y", "z", "mass"):
                scale = {"x": 360.0, "y": 90.0, "z": 1.0, "mass": float(np.abs(ref["mass"]).max())}[k]
                dxy = dev[k] - ref[k]
                if k == "x":
                    dxy = dxy - 360 * np.rint(dxy / 360)
                assert np.abs(dxy).max() <= 1e-12 * scale, (name, k, np.abs(dxy).max())
                identical = identical and np.array_equal(dev[k], ref[k])
            else:
                assert np.array_equal(dev[k], ref[k]), (name, k)
        print(f"{which} vs {name}: bit-identical = {identical}")
