"""GPU: ParticleSet.cells / ParticleSet.connectivity (csrc/pk_connectivity.hip).  Destination cells come from the density fixtures of
tools/make_density_golden.py -- the reference's own answers -- and the expected matrix from the NumPy restatement of connectivity_utils;
every comparison is exact."""

from __future__ import annotations

import numpy as np
import pytest

import parcels_amd as pa
from case_utils import build_fieldset
from connectivity_utils import connectivity_numpy, same_arrays, sparse_to_dense
from density_utils import FIXTURES, density_fieldset, density_pset, fixture, same_bits
from parcels_amd import StatusCode

pytestmark = pytest.mark.gpu

_FS = {}
PATHS = ["lds", "global", "sparse"]


def _fieldset(name):
    """one device FieldSet per fixture, shared by the tests of this module"""
    if name not in _FS:
        _FS[name] = density_fieldset(fixture(name))
    return _FS[name]


def _sorted_launch(pset, case, sort):
    """a launch that moves nothing: with sort_by_cell it reorders the device rows by cell, so the calls after it go through the permutation"""
    pset.execute([pa.DoNothing], dt=60.0, runtime=60.0)
    if case["kind"] == "xgrid":  # (a launch on a UxGrid does not sort)
        assert (pset._last_stats["sort_ms"] > 0) == sort


def _regions(shape, seed, lo=-2, hi=5):
    return np.random.default_rng(seed).integers(lo, hi, size=tuple(shape)).astype(np.int32)


def _labels(cell, regions):
    """the label of every particle from its fixture cell: regions.ravel()[cell], -1 kept and negative labels -1"""
    cell = np.asarray(cell, dtype=np.int64)
    if regions is None:
        return cell
    lab = np.where(cell >= 0, regions.ravel()[np.maximum(cell, 0)].astype(np.int64), -1)
    return np.where(lab < 0, -1, lab)


def _origins(n, n_origin, seed):
    """seeded origin labels in [-2, n_origin): blocks of 37 equal labels (runs across wavefront boundaries) with a third of the rows redrawn"""
    rng = np.random.default_rng(seed)
    o = np.repeat(rng.integers(-2, n_origin, n // 37 + 1), 37)[:n]
    redraw = rng.random(n) < 0.3
    o[redraw] = rng.integers(-2, n_origin, int(redraw.sum()))
    return o.astype(np.int64)


# ---- cells -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_cells_equal_the_fixture_cells(gpu, name):
    """the reference's own cells without and with levels, and through a region map with negative labels -- on rows in host order and, after a
    launch that cell-sorted them, through the row permutation"""
    case = fixture(name)
    pset = density_pset(case, _fieldset(name), sort_by_cell=True)
    n = len(case["x"])
    for launched in (False, True):
        if launched:
            if n == 0:
                break
            _sorted_launch(pset, case, True)
            stale = set(pset._data._stale)
        for lv, sfx in ((False, ""), (True, "_levels")):
            got = pset.cells(levels=lv)
            print(f"{name}{sfx} launched={launched}: {np.count_nonzero(got != case['cell' + sfx])} of {n} labels differ")
            assert got.dtype == np.int64 and got.shape == (n,)
            assert np.array_equal(got, case["cell" + sfx])
            regions = _regions(case["shape" + sfx], seed=3)
            assert (regions < 0).any() and (regions >= 0).any()
            for reg in (regions, regions.astype(np.int64), regions.astype(np.int16)):
                assert same_arrays(pset.cells(levels=lv, regions=reg), _labels(case["cell" + sfx], regions))
        if launched:
            assert set(pset._data._stale) == stale and pset._data.resident()


def test_cells_field_argument(gpu):
    case = fixture("dens_ux_sph_levels")
    fs = _fieldset("dens_ux_sph_levels")
    pset = density_pset(case, fs)
    for f in ("U", "T", fs.U, fs.UV, None):
        assert np.array_equal(pset.cells(f), case["cell"])


# ---- connectivity, dense ---------------------------------------------------------------------------------------------------------------------
def _case_levels(name):
    return name == "dens_ux_sph_levels"


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["dens_runs", "dens_one_cell", "dens_rect_flat", "dens_ux_sph_levels"])
def test_dense_matrix_through_every_path(gpu, name, path, sort, monkeypatch):
    """the same matrix and the same outside vector as NumPy through the LDS histogram, the global adds and the sort (converted to dense), on
    rows in host order and through the permutation of the cell sort; cell-to-cell and through a region map"""
    monkeypatch.setenv("PK_CONNECTIVITY_PATH", path)
    case = fixture(name)
    lv = _case_levels(name)
    cell = case["cell_levels" if lv else "cell"]
    shape = tuple(case["shape_levels" if lv else "shape"])
    ncells = int(np.prod(shape))
    n = len(cell)
    n_origin = 6
    origin = _origins(n, n_origin, seed=len(name))
    assert (origin < 0).any() and len(np.unique(origin[origin >= 0])) == n_origin
    pset = density_pset(case, _fieldset(name), sort_by_cell=sort)
    for launched in (False, True):
        if launched:
            _sorted_launch(pset, case, sort)
        t, outside = pset.connectivity(origin, levels=lv, n_origin=n_origin, return_outside=True)
        want, want_out = connectivity_numpy(origin, cell, n_origin, ncells, return_outside=True)
        info = pset._last_connectivity_info
        print(f"{name} {path} sort={sort} launched={launched}: {int(np.count_nonzero(t != want))} entries differ, outside {outside.tolist()} / {want_out.tolist()}, info {info}")
        assert info["path"] == path
        assert same_arrays(t, want) and same_arrays(outside, want_out)
        assert t.shape == (n_origin, ncells) and t.sum() + outside.sum() == np.count_nonzero(origin >= 0) == info["n_tracked"]
        assert info["n_outside"] == want_out.sum() and info["n_pairs"] == np.count_nonzero(want) + np.count_nonzero(want_out)
        regions = _regions(shape, seed=9)
        n_dest = int(regions.max()) + 1
        t, outside = pset.connectivity(origin, levels=lv, regions=regions, n_origin=n_origin, return_outside=True)
        want, want_out = connectivity_numpy(origin, _labels(cell, regions), n_origin, n_dest, return_outside=True)
        assert same_arrays(t, want) and same_arrays(outside, want_out)
        assert same_arrays(pset.connectivity(origin, levels=lv, regions=regions.astype(np.int64), n_origin=n_origin), want)
        norm = pset.connectivity(origin, levels=lv, regions=regions, n_origin=n_origin, normalize="origin")
        assert same_bits(norm, connectivity_numpy(origin, _labels(cell, regions), n_origin, n_dest, normalize="origin"))


def test_one_add_per_run_of_equal_keys(gpu, monkeypatch):
    """dens_one_cell in host order, every row of one origin: 4099 rows of one pair are one add per wavefront without the LDS histogram,
    and one per non-zero bin of every 256-row workgroup with it"""
    case = fixture("dens_one_cell")
    n = len(case["x"])
    assert n == 4099
    pset = density_pset(case, _fieldset("dens_one_cell"), sort_by_cell=False)
    origin = np.full(n, 3, np.int32)
    want = connectivity_numpy(origin, case["cell"], 5, 24)
    assert np.count_nonzero(want) == 1 and want.sum() == n
    monkeypatch.setenv("PK_CONNECTIVITY_PATH", "global")
    assert same_arrays(pset.connectivity(origin, n_origin=5), want)
    assert pset._last_connectivity_info["n_atomics"] == 65  # ceil(4099 / 64) wavefronts, one run each
    monkeypatch.setenv("PK_CONNECTIVITY_PATH", "lds")
    assert same_arrays(pset.connectivity(origin, n_origin=5), want)
    assert pset._last_connectivity_info["n_atomics"] == 17  # ceil(4099 / 256) workgroups, one non-zero bin each
    monkeypatch.setenv("PK_CONNECTIVITY_PATH", "sparse")
    assert same_arrays(pset.connectivity(origin, n_origin=5), want)
    assert pset._last_connectivity_info["n_atomics"] == 0 and pset._last_connectivity_info["n_pairs"] == 1
    # two origins alternating every 96 rows: the runs of a wavefront end where the origin changes
    origin = ((np.arange(n) // 96) % 2).astype(np.int64)
    runs = np.count_nonzero(np.r_[True, origin[1:] != origin[:-1]] | (np.arange(n) % 64 == 0))
    monkeypatch.setenv("PK_CONNECTIVITY_PATH", "global")
    assert same_arrays(pset.connectivity(origin, n_origin=2), connectivity_numpy(origin, case["cell"], 2, 24))
    assert pset._last_connectivity_info["n_atomics"] == runs


# ---- both sides of the LDS threshold ---------------------------------------------------------------------------------------------------------
def _host_cells(pset, fs):
    """what a script does today on a flat rectilinear grid: read the positions, pk_search them, unravel"""
    grid = fs.U.grid
    z, y, x = np.array(pset.z), np.array(pset.y), np.array(pset.x)
    lon, lat = np.asarray(grid.lon), np.asarray(grid.lat)
    inside = (x >= lon[0]) & (x <= lon[-1]) & (y >= lat[0]) & (y <= lat[-1]) & np.isfinite(x) & np.isfinite(y)
    ei = fs._engine.search(0, np.where(np.isfinite(z), z, 0.0), y, x).astype(np.int64)
    idx = grid.unravel_index(np.where(inside, ei, 0))
    return np.where(inside, idx["Y"] * grid.xdim + idx["X"], -1)


@pytest.mark.parametrize("nx", [128, 129])
def test_both_sides_of_the_lds_threshold(gpu, nx, monkeypatch):
    """64 origins times (nx - 1) + 1 columns: 8192 keys fit the LDS histogram, 8256 do not; both equal the host route exactly"""
    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    lon, lat = np.linspace(0.0, 10.0, nx), np.array([-5.0, 5.0])
    fs = density_fieldset(dict(kind="xgrid", mesh="flat", lon=lon, lat=lat, depth=None))
    rng = np.random.default_rng(nx)
    n = 5003
    x, y = rng.uniform(-0.5, 10.5, n), rng.uniform(-5.5, 5.5, n)
    x[:40], y[:40] = lon[-1 - np.arange(40)], 0.0  # on nodes, the last column included
    pset = density_pset(dict(spatial_dtype="float64", x=x, y=y, z=np.zeros(n)), fs, sort_by_cell=False)
    origin = rng.integers(-1, 64, n)
    t, outside = pset.connectivity(origin, n_origin=64, return_outside=True)
    assert t.shape == (64, nx - 1)
    assert pset._last_connectivity_info["path"] == ("lds" if nx == 128 else "global")
    cell = _host_cells(pset, fs)
    want, want_out = connectivity_numpy(origin, cell, 64, nx - 1, return_outside=True)
    assert same_arrays(t, want) and same_arrays(outside, want_out)
    assert outside.sum() > 0 and t[:, -1].sum() > 0 and t[-1].sum() > 0


# ---- sparse ----------------------------------------------------------------------------------------------------------------------------------
def _assert_sparse(got, want):
    for g, w in zip(got, want):
        assert same_arrays(g, w)


@pytest.mark.parametrize("sort", [True, False])
def test_sparse_keys_wider_than_32_bits(gpu, sort, monkeypatch):
    """origins {0, 5, 2**31 - 2} with n_origin = 2**31 - 1: the keys need more than 32 bits and the sort's end bit has to cover them;
    (i, j, count) equals np.unique exactly and in order"""
    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    case = fixture("dens_rect_flat")
    n = len(case["x"])
    rng = np.random.default_rng(31)
    origin = np.array([0, 5, 2**31 - 2, -1], np.int64)[rng.integers(0, 4, n)]
    n_origin, n_dest = 2**31 - 1, int(np.prod(case["shape"]))
    assert (n_origin - 1) * (n_dest + 1) > 2**32
    pset = density_pset(case, _fieldset("dens_rect_flat"), sort_by_cell=sort)
    _sorted_launch(pset, case, sort)
    got, got_out = pset.connectivity(origin, n_origin=n_origin, sparse=True, return_outside=True)
    want, want_out = connectivity_numpy(origin, case["cell"], n_origin, n_dest, sparse=True, return_outside=True)
    print(f"pairs {len(got[0])} / {len(want[0])}, outside {got_out} / {want_out}, info {pset._last_connectivity_info}")
    _assert_sparse(got, want)
    _assert_sparse(got_out, want_out)
    assert set(np.unique(got[0]).tolist()) == {0, 5, 2**31 - 2} and len(got_out[0]) > 0
    ok = (origin >= 0) & (case["cell"] >= 0)
    keys, counts = np.unique(origin[ok] * n_dest + case["cell"][ok], return_counts=True)
    assert np.array_equal(np.divmod(keys, n_dest), got[:2]) and np.array_equal(counts, got[2])
    assert pset.connectivity(origin, n_origin=n_origin, sparse=True)[2].dtype == np.int64
    norm = pset.connectivity(origin, n_origin=n_origin, sparse=True, normalize="origin")
    _assert_sparse(norm, connectivity_numpy(origin, case["cell"], n_origin, n_dest, sparse=True, normalize="origin"))
    with pytest.raises(ValueError, match="max_dense"):
        pset.connectivity(origin, n_origin=n_origin)


@pytest.mark.parametrize("name", ["dens_runs", "dens_ux_sph_levels"])
def test_sparse_equals_numpy_on_the_fixtures(gpu, name, monkeypatch):
    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    case = fixture(name)
    lv = _case_levels(name)
    cell = case["cell_levels" if lv else "cell"]
    n_dest = int(np.prod(case["shape_levels" if lv else "shape"]))
    origin = _origins(len(cell), 9, seed=2)
    pset = density_pset(case, _fieldset(name))
    got, got_out = pset.connectivity(origin, levels=lv, sparse=True, n_origin=9, return_outside=True)
    want, want_out = connectivity_numpy(origin, cell, 9, n_dest, sparse=True, return_outside=True)
    _assert_sparse(got, want)
    _assert_sparse(got_out, want_out)
    assert pset._last_connectivity_info["path"] == "sparse" and pset._last_connectivity_info["n_pairs"] == len(want[0]) + len(want_out[0])
    assert same_arrays(sparse_to_dense(*got, 9, n_dest), pset.connectivity(origin, levels=lv, n_origin=9))


def test_sparse_edge_cases(gpu, monkeypatch):
    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    case = fixture("dens_rect_flat")
    fs = _fieldset("dens_rect_flat")
    n = len(case["x"])
    pset = density_pset(case, fs)
    empty = np.zeros(0, np.int64)
    # all rows untracked: empty arrays, nothing outside
    got, got_out = pset.connectivity(np.full(n, -3, np.int32), sparse=True, return_outside=True)
    _assert_sparse(got, (empty, empty, empty))
    _assert_sparse(got_out, (empty, empty))
    assert pset._last_connectivity_info["n_tracked"] == 0 and pset._last_connectivity_info["n_pairs"] == 0
    t, outside = pset.connectivity(np.full(n, -3, np.int32), return_outside=True)
    assert not t.any() and not outside.any()
    # all rows outside
    away = density_pset(dict(case, x=case["x"] + 1.0e6), fs)
    origin = (np.arange(n) % 3).astype(np.int64)
    got, got_out = away.connectivity(origin, sparse=True, return_outside=True)
    _assert_sparse(got, (empty, empty, empty))
    _assert_sparse(got_out, (np.arange(3), np.bincount(origin).astype(np.int64)))
    t, outside = away.connectivity(origin, n_origin=3, return_outside=True)
    assert not t.any() and same_arrays(outside, np.bincount(origin).astype(np.int64))
    # n = 0
    none = density_pset(fixture("dens_n0"), _fieldset("dens_n0"))
    got, got_out = none.connectivity(empty, sparse=True, return_outside=True)
    _assert_sparse(got, (empty, empty, empty))
    _assert_sparse(got_out, (empty, empty))
    t, outside = none.connectivity(empty, n_origin=4, return_outside=True)
    assert t.shape == (4, 35) and t.dtype == np.int64 and not t.any() and outside.shape == (4,) and not outside.any()
    assert none.cells().shape == (0,) and none.cells().dtype == np.int64


# ---- origin sources --------------------------------------------------------------------------------------------------------------------------
def TouchOrigins(particles, fieldset):  # noqa: N802
    particles.src += 0
    particles.src64 += 0


def _origin_pclass():
    return pa.get_default_particle(np.float64).add_variable([pa.Variable("src", dtype=np.int32, initial=0), pa.Variable("src64", dtype=np.int64, initial=0)])


@pytest.mark.parametrize("sort", [True, False])
def test_origin_sources_give_the_same_matrix(gpu, sort, monkeypatch):
    """an int32 Variable, an int64 Variable and a host array; host-only Variables first, then -- a compiled elementwise kernel touches them
    -- device-resident ones that are read in place, in the row order of the cell sort"""
    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    case = fixture("dens_rect_flat")
    fs = density_fieldset(case)
    n = len(case["x"])
    origin = _origins(n, 7, seed=4)
    pset = density_pset(case, fs, pclass=_origin_pclass(), src=origin, src64=origin, sort_by_cell=sort)
    want = connectivity_numpy(origin, case["cell"], 7, 35, return_outside=True)
    for path in PATHS:
        monkeypatch.setenv("PK_CONNECTIVITY_PATH", path)
        for src in ("src", "src64", origin, origin.astype(np.int32), origin.astype(np.int8)):
            _assert_sparse(pset.connectivity(src, n_origin=7, return_outside=True), want)
    pset.execute([pa.DoNothing, TouchOrigins], dt=60.0, runtime=120.0)
    eng = fs._engine
    assert pset._kernel.user_program is not None and not pset._kernel.host_functions, pset._kernel.jit_report
    assert {"src", "src64"} <= set(eng.device_variables) and {"src", "src64"} <= set(pset._data._stale)
    before = dict(eng.transfers)
    for path in PATHS:
        monkeypatch.setenv("PK_CONNECTIVITY_PATH", path)
        for src in ("src", "src64", origin):
            _assert_sparse(pset.connectivity(src, n_origin=7, return_outside=True), want)
    assert eng.transfers == before and {"src", "src64"} <= set(pset._data._stale)  # read in place: nothing came down
    assert np.array_equal(pset.src, origin) and np.array_equal(pset.src64, origin)


def test_label_above_the_range_is_refused_with_its_count(gpu, monkeypatch):
    case = fixture("dens_rect_flat")
    pset = density_pset(case, _fieldset("dens_rect_flat"))
    n = len(case["x"])
    origin = np.zeros(n, np.int64)
    origin[[3, 77, 200]] = [4, 9, 2**40]
    for path in PATHS:
        monkeypatch.setenv("PK_CONNECTIVITY_PATH", path)
        with pytest.raises(ValueError, match=r"3 rows have an origin label >= n_origin = 4"):
            pset.connectivity(origin, n_origin=4)
        with pytest.raises(ValueError, match=r"1 rows have an origin label >= n_origin = 35"):
            pset.connectivity(origin, sparse=True)
    monkeypatch.delenv("PK_CONNECTIVITY_PATH")
    assert pset.connectivity(np.minimum(origin, 3), n_origin=4).sum() == np.count_nonzero(case["cell"] >= 0)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def DeleteNorthEast(particles, fieldset):  # noqa: N802
    particles.state = np.where((particles.x > fieldset.cut) | (particles.y > fieldset.cut), StatusCode.Delete, particles.state)


def _rotation_case():
    """8 x 8 cells of 1 km, a steady solid-body rotation about the centre"""
    lon = lat = np.linspace(0.0, 8000.0, 9)
    omega = 1.0e-5
    yy, xx = np.meshgrid(lat, lon, indexing="ij")
    u = np.broadcast_to(-omega * (yy - 4000.0), (2, 1, 9, 9)).copy()
    v = np.broadcast_to(omega * (xx - 4000.0), (2, 1, 9, 9)).copy()
    dims = ("time", "mockZ", "YG", "XG")
    return dict(mesh="flat", lon=lon, lat=lat, depth=None, time_s=np.array([0.0, 86400.0]), fields={"U": u, "V": v}, field_dims={"U": dims, "V": dims},
                context={"cut": 6400.0})


def test_release_advect_delete_and_count(gpu, monkeypatch):
    """one particle per cell, cells() stored in a Variable at release, RK4 in a rotation plus a kernel that deletes the two eastern columns and the two northern rows:
    connectivity by Variable equals NumPy on the host-read columns, the call leaves the set as it was, and a further execute gives the bits
    of a twin run that never called cells / connectivity"""
    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    case = _rotation_case()
    points = np.arange(950.0, 8000.0, 1000.0)  # near the north-east corner of every cell: 0.03 rad of rotation carries some into the next cell
    yy, xx = np.meshgrid(points, points, indexing="ij")
    pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("src", dtype=np.int32, initial=-1))
    runs = []
    released = None
    for twin in (False, True):
        fs = build_fieldset(case)
        pset = pa.ParticleSet(fs, pclass=pclass, x=xx.ravel(), y=yy.ravel(), z=np.zeros(64), t=np.zeros(64), sort_by_cell=True)
        if not twin:
            released = pset.cells()
            assert np.array_equal(released, np.arange(64))  # one particle in cell k, in row order
        pset.src = released
        pset.execute([pa.AdvectionRK4, DeleteNorthEast], dt=600.0, runtime=5 * 600.0)
        assert len(pset) == 36
        if not twin:
            data, eng = pset._data, fs._engine
            stale, dirty, before = set(data._stale), set(data._dirty), dict(eng.transfers)
            assert {"x", "y"} <= stale and data.resident()
            t, outside = pset.connectivity("src", return_outside=True)
            (si, sj, sc), _ = pset.connectivity("src", sparse=True, return_outside=True)
            now = pset.cells()
            regions = (np.arange(64).reshape(8, 8) // 16).astype(np.int64)  # four bands of two rows of cells
            by_band = pset.connectivity("src", regions=regions, n_origin=64)
            assert eng.transfers == before, "a particle column crossed PCIe"
            assert set(data._stale) == stale and set(data._dirty) == dirty and data.resident() and data._engine is eng
            src = np.array(pset.src)
            cell = _host_cells(pset, fs)  # (reads x, y, z: only now do they come down)
            assert np.array_equal(now, cell)
            want, want_out = connectivity_numpy(src, cell, 64, 64, return_outside=True)
            assert same_arrays(t, want) and same_arrays(outside, want_out)
            assert same_arrays(sparse_to_dense(si, sj, sc, 64, 64), want)
            assert same_arrays(by_band, connectivity_numpy(src, regions.ravel()[cell], 64, 4))
            assert t.sum() == 36 and not outside.any()
            assert np.array_equal(np.sort(src), np.sort(released[(released % 8 < 6) & (released // 8 < 6)]))  # the Variable followed the deletions
            moved = int(t.sum() - np.trace(t))
            print(f"{moved} of 36 particles changed cell")
            assert 0 < moved < 36
        pset.execute([pa.AdvectionRK4, DeleteNorthEast], dt=600.0, runtime=3 * 600.0)
        runs.append({k: np.array(v) for k, v in pset._data.items()})
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), k
