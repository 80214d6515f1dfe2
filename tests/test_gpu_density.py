"""GPU: ParticleSet.density (csrc/pk_density.hip) against the fixtures of tools/make_density_golden.py -- the reference's own cells plus
np.bincount -- to the bit, the non-finite rule, and the resident, read-only behaviour of the call."""

from __future__ import annotations

import numpy as np
import pytest

import parcels_amd as pa
from case_utils import build_fieldset, build_pset, compare
from density_utils import FIXTURES, density_fieldset, density_numpy, density_pset, fixture, same_bits

pytestmark = pytest.mark.gpu

_FS = {}


def _fieldset(name):
    """one device FieldSet per fixture, shared by the tests of this module"""
    if name not in _FS:
        _FS[name] = density_fieldset(fixture(name))
    return _FS[name]


def _check_fixture(pset, case, weights_arg, w):
    for lv, sfx in ((False, ""), (True, "_levels")):
        shape = tuple(case["shape" + sfx])
        counts, n_out = pset.density(levels=lv, return_outside=True)
        print(f"counts{sfx}: got sum {int(counts.sum())} outside {n_out}; expected {int(case['counts' + sfx].sum())} / {int(case['n_outside' + sfx])}")
        assert counts.dtype == np.int64 and counts.shape == shape
        assert np.array_equal(counts.ravel(), case["counts" + sfx])
        assert n_out == int(case["n_outside" + sfx])
        sums, n_out_w = pset.density(particle_val=weights_arg, levels=lv, return_outside=True)
        expected = np.bincount(case["cell" + sfx][case["cell" + sfx] >= 0], weights=w[case["cell" + sfx] >= 0], minlength=int(np.prod(shape)))
        print(f"sums{sfx}: max |got - expected| = {np.abs(sums.ravel() - expected).max() if expected.size else 0.0:.3e}")
        assert sums.dtype == np.float64 and sums.shape == shape and n_out_w == n_out
        assert sums.ravel().tobytes() == expected.tobytes()  # bit for bit: no tolerance
        assert same_bits(expected, case["sums" + sfx])


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_counts_and_sums_are_exact(gpu, name, sort, lds, monkeypatch):
    """counts without / with levels exactly, weighted sums with np.bincount's bits, n_outside exactly -- on rows in host order and, after a
    launch that cell-sorted them, through the row permutation; counts through the workgroup-private LDS histogram (every fixture's map
    fits it) and, switched off, through the global adds a larger map gets"""
    monkeypatch.setenv("PK_DENSITY_LDS", "1" if lds else "0")
    case = fixture(name)
    fs = _fieldset(name)
    pset = density_pset(case, fs, sort_by_cell=sort)
    _check_fixture(pset, case, case["w"], case["w"])
    if len(pset):
        pset.execute([pa.DoNothing], dt=60.0, runtime=60.0)  # moves nothing: with sort_by_cell the launch reorders the device rows by cell
        if case["kind"] == "xgrid":  # (a launch on a UxGrid does not sort: both runs take the identity path there)
            assert (pset._last_stats["sort_ms"] > 0) == sort
        stale = set(pset._data._stale)
        assert {"x", "y"} <= stale
        _check_fixture(pset, case, case["w"], case["w"])
        assert set(pset._data._stale) == stale and pset._data.resident() and pset._data._engine is fs._engine


def _wave_runs(cell):
    """runs of equal cells inside the 64-row wavefronts of rows in host order: the adds the count kernel issues without the LDS histogram"""
    cell = np.asarray(cell)
    heads = np.r_[True, cell[1:] != cell[:-1]] | (np.arange(cell.size) % 64 == 0)
    return int(np.count_nonzero(heads & (cell >= 0)))


@pytest.mark.parametrize("name", ["dens_runs", "dens_one_cell", "dens_rect_flat"])
def test_one_add_per_run_of_equal_cells(gpu, name, monkeypatch):
    """rows in host order: without the LDS histogram one global add per run of equal cells inside a wavefront; with it one per non-zero
    bin of a 256-row workgroup"""
    case = fixture(name)
    pset = density_pset(case, _fieldset(name), sort_by_cell=False)
    cell = case["cell"]
    monkeypatch.setenv("PK_DENSITY_LDS", "0")
    assert np.array_equal(pset.density().ravel(), case["counts"])
    assert pset._last_density_info["n_atomics"] == _wave_runs(cell)
    if name == "dens_one_cell":
        assert _wave_runs(cell) == 65  # 4099 rows of one cell: one add per wavefront
    monkeypatch.setenv("PK_DENSITY_LDS", "1")
    assert np.array_equal(pset.density().ravel(), case["counts"])
    bins = sum(len(np.unique(c[c >= 0])) for c in np.array_split(cell, np.arange(256, cell.size, 256)))
    assert pset._last_density_info["n_atomics"] == bins
    assert pset._last_density_info["n_inside"] == int(case["counts"].sum())


@pytest.mark.parametrize("nx", [129, 130])
def test_both_sides_of_the_lds_threshold(gpu, nx):
    """(nx - 1) x 64 cells: 8192 fit the LDS histogram, 8256 do not; both equal the host route (pk_search + np.bincount) exactly"""
    lon, lat = np.linspace(0.0, 10.0, nx), np.linspace(-5.0, 5.0, 65)
    fs = density_fieldset(dict(kind="xgrid", mesh="flat", lon=lon, lat=lat, depth=None))
    rng = np.random.default_rng(nx)
    n = 5003
    x, y = rng.uniform(-0.5, 10.5, n), rng.uniform(-5.5, 5.5, n)
    x[:40], y[:40] = lon[-1 - np.arange(40)], lat[np.arange(40)]  # on nodes, the last column included
    pset = density_pset(dict(spatial_dtype="float64", x=x, y=y, z=np.zeros(n)), fs, sort_by_cell=False)
    counts, n_out = pset.density(return_outside=True)
    assert counts.shape == (64, nx - 1)
    cell = _host_route(pset, fs)
    assert np.array_equal(counts, density_numpy(cell, counts.shape)) and n_out == np.count_nonzero(cell < 0) > 0
    assert counts[:, -1].sum() > 0 and counts[-1].sum() > 0


@pytest.mark.parametrize("name", ["dens_runs", "dens_ux_sph_levels"])
def test_weight_sources_give_the_same_bits(gpu, name):
    """a float64, a float32 and an int32 Variable and a host array: each equals np.bincount of the same values"""
    case = fixture(name)
    rng = np.random.default_rng(5)
    n = len(case["x"])
    w64 = case["w"]
    w32 = w64.astype(np.float32)
    i32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    i64 = rng.integers(-2**62, 2**62, n).astype(np.int64)
    pclass = pa.get_default_particle(np.float64).add_variable([pa.Variable("m64", dtype=np.float64, initial=0), pa.Variable("m32", dtype=np.float32, initial=0),
                                                               pa.Variable("k32", dtype=np.int32, initial=0), pa.Variable("k64", dtype=np.int64, initial=0)])
    pset = density_pset(case, _fieldset(name), pclass=pclass, m64=w64, m32=w32, k32=i32, k64=i64)
    inside = case["cell"] >= 0
    ncells = int(np.prod(case["shape"]))
    for var, vals in (("m64", w64), ("m32", w32), ("k32", i32), ("k64", i64)):
        expected = np.bincount(case["cell"][inside], weights=vals[inside], minlength=ncells)
        assert pset.density(particle_val=var).ravel().tobytes() == expected.tobytes(), var
        assert pset.density(particle_val=vals).ravel().tobytes() == expected.tobytes(), var + " as a host array"


def Age(particles, fieldset):  # noqa: N802
    particles.age += particles.dt


def test_variable_written_by_a_compiled_kernel(gpu):
    """`age` lives on the device (a compiled user kernel writes it): density reads it there; the same values as a host array give the same bits"""
    case = _agrid_case()
    fs = build_fieldset(case)
    pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("age", dtype=np.float32, initial=0))
    n = len(case["x"])
    pset = pa.ParticleSet(fs, pclass=pclass, x=np.asarray(case["x"]), y=np.asarray(case["y"]), z=case.get("z"), t=np.zeros(n), age=np.arange(n) * 0.37)
    pset.execute([pa.AdvectionRK4, Age], dt=float(case["dt"]), runtime=4 * float(case["dt"]))
    eng = fs._engine
    assert "age" in eng.device_variables and "age" in pset._data._stale
    before = dict(eng.transfers)
    from_device = pset.density(particle_val="age")
    assert eng.transfers == before and "age" in pset._data._stale  # read in place: nothing came down
    age = np.array(pset.age)
    assert age.dtype == np.float32 and np.all(age >= 4 * float(case["dt"])) and len(np.unique(age)) == n
    assert from_device.tobytes() == pset.density(particle_val=age).tobytes()
    cell = _host_route(pset, fs)
    assert same_bits(from_device, density_numpy(cell, from_device.shape, weights=age))
    # another set of the same FieldSet whose class has no `age`, never executed: bound without the device Variable of the last kernel list
    other = build_pset(case, fs)
    assert np.array_equal(other.density(), density_numpy(_host_route(other, fs), from_device.shape))
    assert same_bits(pset.density(particle_val="age"), from_device)  # and back: `age` goes up again with the set


@pytest.mark.parametrize("name", ["dens_rect_flat", "dens_rect_sph_f32", "dens_curv_sph", "dens_ux_flat"])
def test_non_finite_positions_are_outside(gpu, name):
    """NaN / +-inf in x or y (z with levels) puts a row into n_outside and into no cell -- the reference's searchsorted would put a NaN
    longitude into the last cell; without levels a non-finite z does not matter"""
    case = fixture(name)
    sdt = np.dtype(case["spatial_dtype"])
    x, y, z = case["x"].copy(), case["y"].copy(), case["z"].copy()
    rows = np.flatnonzero(case["cell_levels"] >= 0)[:9]
    assert len(rows) == 9
    bad = [np.nan, np.inf, -np.inf]
    for k in range(3):
        x[rows[k]] = bad[k]
        y[rows[3 + k]] = bad[k]
        z[rows[6 + k]] = bad[k]
    assert x.dtype == sdt
    pset = density_pset(dict(case, x=x, y=y, z=z), _fieldset(name))
    cell = case["cell"].copy()
    cell[rows[:6]] = -1
    counts, n_out = pset.density(return_outside=True)
    assert np.array_equal(counts, density_numpy(cell, case["shape"])) and n_out == int(case["n_outside"]) + 6
    cell_lv = case["cell_levels"].copy()
    cell_lv[rows] = -1
    counts, n_out = pset.density(levels=True, return_outside=True)
    assert np.array_equal(counts, density_numpy(cell_lv, case["shape_levels"])) and n_out == int(case["n_outside_levels"]) + 9
    sums = pset.density(particle_val=case["w"], levels=True)
    assert same_bits(sums, density_numpy(cell_lv, case["shape_levels"], weights=case["w"]))


def _agrid_case():
    from oracle import cases

    return cases.rect_agrid_case("density_a", mesh="spherical", kernels=["AdvectionRK4"], seed=11, npart=3000, runtime=None)


def _host_route(pset, fs):
    """what a script does today: read the positions, pk_search them, np.bincount"""
    grid = fs.U.grid
    z, y, x = np.array(pset.z), np.array(pset.y), np.array(pset.x)
    lon, lat = np.asarray(grid.lon), np.asarray(grid.lat)
    inside = (x >= lon[0]) & (x <= lon[-1]) & (y >= lat[0]) & (y <= lat[-1]) & np.isfinite(x) & np.isfinite(y)
    ei = fs._engine.search(0, np.where(np.isfinite(z), z, 0.0), y, x).astype(np.int64)
    idx = grid.unravel_index(np.where(inside, ei, 0))
    cell = np.where(inside, idx["Y"] * grid.xdim + idx["X"], -1)
    return cell


@pytest.mark.parametrize("sort", [True, False])
def test_resident_path_equals_the_host_route_and_downloads_nothing(gpu, sort):
    case = _agrid_case()
    fs = build_fieldset(case)
    pset = build_pset(case, fs, sort_by_cell=sort)
    pset.execute([pa.AdvectionRK4], dt=float(case["dt"]), runtime=6 * float(case["dt"]))
    eng = fs._engine
    data = pset._data
    stale, dirty, before = set(data._stale), set(data._dirty), dict(eng.transfers)
    assert {"x", "y", "z"} <= stale
    counts, n_out = pset.density(return_outside=True)
    assert eng.transfers == before, "density moved a particle column across PCIe"
    assert set(data._stale) == stale and set(data._dirty) == dirty and data.resident()
    assert pset._last_density_info["n_inside"] == counts.sum() and pset._last_density_info["n_atomics"] <= counts.sum()
    cell = _host_route(pset, fs)  # (reads x, y, z: only now do they come down)
    assert np.array_equal(counts, density_numpy(cell, counts.shape)) and n_out == np.count_nonzero(cell < 0)
    assert counts.sum() + n_out == len(pset) and counts.sum() > 0.9 * len(pset)


def test_density_between_two_executes_changes_nothing(gpu):
    """execute -> density -> execute gives the bits of execute -> execute in every column"""
    case = _agrid_case()
    out = []
    for with_density in (False, True):
        fs = build_fieldset(case)
        pset = build_pset(case, fs, sort_by_cell=True)
        pset.execute([pa.AdvectionRK4], dt=float(case["dt"]), runtime=5 * float(case["dt"]))
        if with_density:
            pset.density()
            pset.density(particle_val=np.ones(len(pset)), levels=True)
        pset.execute([pa.AdvectionRK4], dt=float(case["dt"]), runtime=5 * float(case["dt"]))
        out.append({k: np.array(v) for k, v in pset._data.items()})
    compare(out[1], out[0], rtol=0.0, check_state="all", label="execute-density-execute vs execute-execute", skip=())
    for k in out[0]:
        assert same_bits(out[0][k], out[1][k]), k


def test_host_edits_before_density_are_uploaded(gpu):
    """columns the host touched since the last launch are uploaded first, by the path execute uses"""
    case = fixture("dens_rect_flat")
    fs = _fieldset("dens_rect_flat")
    pset = density_pset(case, fs)
    assert np.array_equal(pset.density().ravel(), case["counts"])
    row = int(np.flatnonzero(case["cell"] >= 0)[0])
    pset.x[row] = case["lon"][-1] + 10.0  # out through the east side
    counts, n_out = pset.density(return_outside=True)
    assert n_out == int(case["n_outside"]) + 1 and counts.ravel()[case["cell"][row]] == case["counts"][case["cell"][row]] - 1


@pytest.mark.parametrize("name", ["dens_rect_sph_f32", "dens_curv_sph", "dens_ux_flat", "dens_ux_sph_levels"])
def test_relative_and_area_scale(gpu, name):
    case = fixture(name)
    fs = _fieldset(name)
    pset = density_pset(case, fs)
    areas = fs.U.grid.cell_areas()
    assert areas.shape == tuple(case["shape"])
    for lv, sfx in ((False, ""), (True, "_levels")):
        shape = tuple(case["shape" + sfx])
        assert same_bits(pset.density(relative=True, levels=lv), density_numpy(case["cell" + sfx], shape, relative=True))
        assert same_bits(pset.density(area_scale=True, levels=lv), density_numpy(case["cell" + sfx], shape, areas=areas))
        got = pset.density(particle_val=case["w"], relative=True, area_scale=True, levels=lv)
        assert same_bits(got, density_numpy(case["cell" + sfx], shape, weights=case["w"], relative=True, areas=areas))
    assert np.isclose(pset.density(relative=True).sum(), 1.0)


def test_field_argument_and_an_empty_set(gpu):
    case = fixture("dens_ux_sph_levels")
    fs = _fieldset("dens_ux_sph_levels")
    pset = density_pset(case, fs)
    base = pset.density()
    for f in ("U", "T", fs.U, fs.UV, None):
        assert np.array_equal(pset.density(f), base)
    empty = density_pset(fixture("dens_n0"), _fieldset("dens_n0"))
    for lv, shape in ((False, tuple(fixture("dens_n0")["shape"])), (True, tuple(fixture("dens_n0")["shape_levels"]))):
        m, n_out = empty.density(levels=lv, return_outside=True)
        assert m.shape == shape and m.dtype == np.int64 and not m.any() and n_out == 0
        m = empty.density(particle_val=np.zeros(0), levels=lv, relative=True)
        assert m.shape == shape and m.dtype == np.float64 and not m.any()
