"""CPU: ParticleSet.density -- the fixtures of tools/make_density_golden.py against the live reference, the NumPy restatement of the map
rules, cell_areas against closed forms, the C ABI of the export, and the refusals that are raised before the device is touched."""

import os
import re

import numpy as np
import pytest

import parcels_amd as pa
from density_utils import FIXTURES, density_fieldset, density_numpy, density_pset, fixture, same_bits
from oracle import ref_shim
from parcels_amd import _hip
from tools import make_density_golden as dg
from tools.make_ux_golden import lattice_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference sources not present")


def test_fixtures_cover_the_cases_and_are_small():
    assert FIXTURES == sorted(dg.cases())
    assert len(FIXTURES) == 10
    sizes = {}
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(dg.GOLDEN, n + ".npz")) < 128 << 10, n
        case = fixture(n)
        sizes[n] = len(case["x"])
        for k in ("x", "y", "z", "w"):
            assert np.isfinite(case[k]).all(), (n, k)  # the non-finite rule is no reference result: tested on its own, on the GPU
        assert case["x"].dtype == np.dtype(case["spatial_dtype"])
    assert sizes == {"dens_rect_flat": 257, "dens_n1": 1, "dens_n0": 0, "dens_rect_sph_f32": 65, "dens_rect_len1": 64, "dens_curv_sph": 73,
                     "dens_ux_flat": 269, "dens_ux_sph_levels": 63, "dens_one_cell": 4099, "dens_runs": 4099}
    assert fixture("dens_rect_sph_f32")["spatial_dtype"] == "float32"
    for k in ("lon", "lat", "depth"):  # float32-representable nodes: the comparisons of float32 positions with them are exact
        a = fixture("dens_rect_sph_f32")[k]
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert fixture("dens_rect_len1")["lon"].shape == (1,) and fixture("dens_rect_len1")["depth"] is None
    assert len(np.unique(fixture("dens_one_cell")["cell"])) == 1


def test_rectilinear_fixture_holds_the_right_closed_node_rule():
    """x on node k lies in cell k - 1, on the first node in cell 0; a point outside on any side, or above / below with levels, is outside"""
    case = fixture("dens_rect_flat")
    lon, lat, depth = case["lon"], case["lat"], case["depth"]
    nx = lon.size - 1
    x, y, z, cell, cell_lv = case["x"], case["y"], case["z"], case["cell"], case["cell_levels"]
    seen = set()
    for k in range(lon.size):
        for r in np.flatnonzero((x == lon[k]) & (cell >= 0)):
            assert cell[r] % nx == max(k - 1, 0)
            seen.add(k)
    assert {0, 1, lon.size - 1} <= seen
    on_lat = [k for k in range(lat.size) if np.any((y == lat[k]) & (cell >= 0))]
    assert {0, 1, lat.size - 1} <= set(on_lat)
    for k in on_lat:
        assert np.all(cell[(y == lat[k]) & (cell >= 0)] // nx == max(k - 1, 0))
    out = (x < lon[0]) | (x > lon[-1]) | (y < lat[0]) | (y > lat[-1])
    assert np.array_equal(cell < 0, out) and np.count_nonzero(x < lon[0]) and np.count_nonzero(x > lon[-1])
    assert np.count_nonzero(y < lat[0]) and np.count_nonzero(y > lat[-1])
    zout = (z < depth[0]) | (z > depth[-1])
    assert np.array_equal(cell_lv < 0, out | zout) and np.count_nonzero(z < depth[0]) and np.count_nonzero(z > depth[-1])
    assert np.any(z == depth[0]) and np.any(z == depth[-1]) and np.any(z == depth[1])
    assert np.any(zout & ~out & (cell >= 0))  # a particle above the surface still counts in its column without levels


def test_runs_fixture_has_the_run_lengths_and_one_cell_tells_the_order_apart():
    cell = fixture("dens_runs")["cell"]
    starts = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    lengths = np.diff(np.r_[starts, cell.size])
    assert {1, 2, 63, 64, 65, 129} <= set(lengths.tolist())
    ends = starts + lengths
    assert np.any(ends % 64 == 0) and np.any(ends % 64 == 1) and np.any(ends % 64 == 63)
    assert np.all(lengths[-400:] == 1)  # the alternating tail
    one = fixture("dens_one_cell")
    c, w = int(one["cell"][0]), one["w"]
    assert one["sums"][c] != np.bincount(one["cell"][::-1], weights=w[::-1])[c]
    assert one["sums"][c] != float(np.sum(w))  # (pairwise)
    assert np.log10(np.abs(w).max() / np.abs(w).min()) > 29 and (w > 0).any() and (w < 0).any()


@needs_reference
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_regenerates_from_the_reference(name):
    """tools/make_density_golden.py run on the live reference gives the committed arrays (and holds the generator's conditions)"""
    arrs = dg.generate(name, dg.cases()[name])
    with np.load(os.path.join(dg.GOLDEN, name + ".npz"), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(arrs)
        for k in z.files:
            assert np.array_equal(z[k], arrs[k]), (name, k)
            assert z[k].dtype == arrs[k].dtype, (name, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_restatement_matches_the_fixtures(name):
    """shape rule, levels, relative and return_outside of the restatement the GPU tests compare with"""
    case = fixture(name)
    grid = density_fieldset(case).U.grid
    from parcels_amd.engine import density_shape

    for lv, sfx in ((False, ""), (True, "_levels")):
        shape = tuple(case["shape" + sfx])
        assert density_shape(grid, lv) == shape
        counts, n_out = density_numpy(case["cell" + sfx], shape, return_outside=True)
        assert counts.dtype == np.int64 and counts.shape == shape
        assert np.array_equal(counts.ravel(), case["counts" + sfx]) and n_out == int(case["n_outside" + sfx])
        assert counts.sum() + n_out == len(case["x"])
        sums = density_numpy(case["cell" + sfx], shape, weights=case["w"])
        assert same_bits(sums.ravel(), case["sums" + sfx])
        rel = density_numpy(case["cell" + sfx], shape, relative=True)
        assert rel.dtype == np.float64 and (np.isclose(rel.sum(), 1.0) if counts.sum() else not rel.any())
    if case["kind"] == "ux":
        assert tuple(case["shape"]) == (case["faces"].shape[0],) and tuple(case["shape_levels"]) == (case["zf"].size, case["faces"].shape[0])
    elif case["depth"] is None:
        assert case["shape_levels"] == [1] + case["shape"]  # levels on a grid without a vertical axis: a leading 1, no error
    if name == "dens_rect_len1":
        assert tuple(case["shape"]) == (5, 1)


# ---- cell_areas ------------------------------------------------------------------------------------------------------------------------
def _rect_grid(lon, lat, mesh):
    return density_fieldset(dict(kind="xgrid", mesh=mesh, lon=np.asarray(lon, float), lat=np.asarray(lat, float), depth=None)).U.grid


def test_cell_areas_of_a_spherical_rectilinear_grid():
    g = _rect_grid([10.0, 11.0, 12.5], [0.0, 1.0, 30.0, 31.0], "spherical")
    a = g.cell_areas()
    assert a.shape == (3, 2)
    radius = g.deg2m * 180.0 / np.pi
    one_deg = radius**2 * np.deg2rad(1.0) * (np.sin(np.deg2rad(1.0)) - 0.0)  # the 1 x 1 degree cell on the equator
    assert np.isclose(a[0, 0], one_deg, rtol=1e-14) and np.isclose(one_deg, g.deg2m**2 * np.sin(np.deg2rad(1.0)) * 180.0 / np.pi, rtol=1e-14)
    box = radius**2 * np.deg2rad(2.5) * (np.sin(np.deg2rad(31.0)) - np.sin(np.deg2rad(0.0)))  # the cells tile the lat-lon box
    assert np.isclose(a.sum(), box, rtol=1e-14)
    flat = _rect_grid([10.0, 11.0, 12.5], [0.0, 1.0, 30.0, 31.0], "flat").cell_areas()
    assert np.array_equal(flat, np.outer([1.0, 29.0, 1.0], [1.0, 1.5]))


def test_cell_areas_of_curvilinear_grids():
    case = fixture("dens_curv_sph")
    flat = density_fieldset(dict(case, mesh="flat")).U.grid.cell_areas()
    lon, lat = case["lon"], case["lat"]
    assert flat.shape == tuple(case["shape"])
    # the cells tile the hull: shoelace over the boundary nodes
    bx = np.r_[lon[0, :-1], lon[:-1, -1], lon[-1, :0:-1], lon[:0:-1, 0]]
    by = np.r_[lat[0, :-1], lat[:-1, -1], lat[-1, :0:-1], lat[:0:-1, 0]]
    hull = 0.5 * abs(np.sum(bx * np.roll(by, -1) - np.roll(bx, -1) * by))
    assert np.isclose(flat.sum(), hull, rtol=1e-13)
    # chordal areas on the sphere: a rectilinear 1-degree mesh given as 2-D arrays agrees with the exact lat-lon boxes to (1 degree)^2 / 12
    lo, la = np.meshgrid(np.arange(5.0, 9.0), np.arange(40.0, 44.0))
    curv = density_fieldset(dict(kind="xgrid", mesh="spherical", lon=lo, lat=la, depth=None)).U.grid
    assert curv.is_curvilinear
    exact = _rect_grid(lo[0], la[:, 0], "spherical").cell_areas()
    rel = curv.cell_areas() / exact - 1.0
    assert np.all(np.abs(rel) < 1e-4) and np.all(np.abs(rel) > 1e-7)  # an approximation, and documented as one


def test_cell_areas_of_triangle_meshes():
    lon, lat, faces = lattice_mesh(9, 7, 2.0, 10.0, -3.0, 3.0, jitter=0.3, seed=4)  # jitter moves interior nodes only: the hull is the box
    flat = pa.UxGrid(pa.UxMesh(lon, lat, faces), z=np.array([0.0, 1.0]), mesh="flat").cell_areas()
    assert flat.shape == (faces.shape[0],) and np.all(flat > 0)
    assert np.isclose(flat.sum(), 8.0 * 6.0, rtol=1e-13)
    sph = pa.UxGrid(pa.UxMesh(lon, lat, faces), z=np.array([0.0, 1.0]), mesh="spherical")
    radius = sph.deg2m * 180.0 / np.pi
    box = radius**2 * np.deg2rad(8.0) * (np.sin(np.deg2rad(3.0)) - np.sin(np.deg2rad(-3.0)))
    assert np.isclose(sph.cell_areas().sum(), box, rtol=2e-3)  # chordal facets under a 1-degree mesh near the equator


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_documented_and_bound():
    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    assert int(re.search(r"#define\s+PK_ABI_VERSION\s+(\d+)", header).group(1)) == 9 == _hip.PK_ABI_VERSION
    assert "pk_particles_density" in _hip.ABI_SYMBOLS
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct \{[^}]*\}\s*pk_density_info_t;\s*)*int32_t pk_particles_density\(", header, re.S)
    assert m, "the declaration follows its comment"
    doc = m.group(1)
    for word in ("np.bincount", "grid.search", "populate_indices", "pset.x", "HOST row", "non-finite", "n_outside"):
        assert word in doc, word  # what host code the export replaces, and its rules
    for name, value in (("PK_DENSITY_W_NONE", 0), ("PK_DENSITY_W_EXTRA", 1), ("PK_DENSITY_W_HOST", 2), ("PK_DENSITY_F32", 0), ("PK_DENSITY_F64", 1),
                        ("PK_DENSITY_I32", 2), ("PK_DENSITY_I64", 3)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value == getattr(_hip, name)
    fields = re.search(r"typedef struct \{([^}]*)\}\s*pk_density_info_t;", header).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names == [n for n, _ in _hip.DensityInfo._fields_] and __import__("ctypes").sizeof(_hip.DensityInfo) == 40
    mk = open(os.path.join(ROOT, "parcels_amd", "csrc", "Makefile")).read()
    assert "pk_density.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1) and "pk_density.h" in re.search(r"^%\.o: (.*)$", mk, re.M).group(1)


# ---- refusals raised before the device is touched ------------------------------------------------------------------------------------------
def test_density_refusals_name_the_reason():
    case = fixture("dens_rect_flat")
    fs = density_fieldset(case)
    pclass = pa.get_default_particle(np.float64).add_variable([pa.Variable("mass", dtype=np.float64, initial=1.0), pa.Variable("flag", dtype=np.int16, initial=1)])
    pset = density_pset(case, fs, pclass=pclass)
    n = len(pset)
    with pytest.raises(ValueError, match="no Variable 'nope'"):
        pset.density(particle_val="nope")
    with pytest.raises(TypeError, match="int16"):
        pset.density(particle_val="flag")
    with pytest.raises(ValueError, match=rf"expected \({n},\)"):
        pset.density(particle_val=np.ones(n + 1))
    with pytest.raises(ValueError, match="one weight per particle"):
        pset.density(particle_val=np.ones((n, 1)))
    with pytest.raises(TypeError, match="complex128"):
        pset.density(particle_val=np.ones(n, complex))
    with pytest.raises(ValueError, match="no field 'W'"):
        pset.density("W")
    with pytest.raises(TypeError, match="field must be"):
        pset.density(3)
    other = density_fieldset(case)
    for f in (other.U, other.UV):
        with pytest.raises(ValueError, match="not a field of this ParticleSet's FieldSet"):
            pset.density(f)
    sharded = density_pset(case, fs, shard=(0, 2))
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.density()
