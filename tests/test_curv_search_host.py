"""The mesh families of tests/curv_mesh_families.py on the host: the table builds, the oracle's unguessed search answers the query
set and its answer is stable on (nearly) all random and interior points, the lattice rule of csrc/pk_hashbuild.h classifies the
families as stated, and the oracle runs every family's trajectory case to its end.  The GPU side is tests/test_gpu_curv_search.py."""

from __future__ import annotations

import numpy as np
import pytest

import curv_mesh_families as cmf
from case_utils import run_oracle

GRID_SEARCH_ERROR = -3
STATE_GRID_SEARCHING = 52
N_RANDOM = 4000


@pytest.mark.parametrize("name", list(cmf.FAMILIES))
def test_family_has_the_stated_shape_and_lattice_class(name):
    for mesh in cmf.FAMILIES[name]["meshes"]:
        lon, lat = cmf.family(name, mesh)
        assert lon.shape == lat.shape == cmf.FAMILIES[name]["shape"]
        assert lon.dtype == lat.dtype == np.float64 and lon.flags.c_contiguous and lat.flags.c_contiguous
        assert np.array_equal(np.isnan(lon), np.isnan(lat))
        assert cmf.lattice_coincident(lon, lat, mesh) == (name in cmf.COINCIDENT), (name, mesh)
    if name == "pole_row":
        assert np.all(cmf.family(name)[1][-1] == 90.0)
    if name == "masked":
        assert np.isnan(cmf.family(name)[0]).sum() == 20
    if name == "self_overlap":  # no node repeats, yet the mesh spans more than 360 degrees
        lon, lat = cmf.family(name)
        assert lon.max() - lon.min() > 360.0
        pts = np.stack((np.mod(lon, 360.0).ravel(), lat.ravel()), axis=1)
        assert len(np.unique(np.round(pts, 6), axis=0)) == len(pts)
    if name == "fine_patch":  # FastC::near_edges stays on: every cell spans under 2^-8 rad of latitude
        lat = cmf.family(name)[1]
        c = np.stack((lat[:-1, :-1], lat[:-1, 1:], lat[1:, :-1], lat[1:, 1:]))
        assert np.deg2rad(c.max(axis=0) - c.min(axis=0)).max() < 2.0 ** -8
    if name == "halo_plus360":
        a, b = cmf.family("halo_exact"), cmf.family(name)
        assert np.array_equal(b[0][:, -2:], a[0][:, -2:] + 360.0) and np.array_equal(b[0][:, :-2], a[0][:, :-2]) and np.array_equal(a[1], b[1])
    if name == "antimeridian_wrapped":
        a, b = cmf.family("antimeridian_continuous"), cmf.family(name)
        assert a[0].min() == 150.0 and abs(a[0].max() - 215.0) < 1e-9 and b[0].max() <= 180.0 and b[0].min() < -144.0
        assert np.array_equal(np.where(a[0] > 180.0, a[0] - 360.0, a[0]), b[0])


@pytest.mark.parametrize("name,mesh", cmf.FAMILY_MESHES)
def test_oracle_search_is_stable_on_the_query_set(name, mesh):
    """The host table builds, po_hash_query answers every query kind, and at least 99 % of the random and interior points are
    stable (a condition on the query generator and the meshes: the comparison of pk_search with the oracle runs on stable points)."""
    case = cmf.mesh_case(name, mesh)
    assert case["hash_table"]["keys"].size > 0
    q = cmf.query_points(case["lon"], case["lat"], N_RANDOM, seed=11, mesh=mesh)
    x, y, sl = cmf.flatten_queries(q)
    ok, yi, xi = cmf.stable_mask(case, x, y)
    ny, nx = case["lon"].shape
    found = yi != GRID_SEARCH_ERROR
    assert np.all((yi[found] >= 0) & (yi[found] < ny - 1) & (xi[found] >= 0) & (xi[found] < nx - 1))
    assert np.all((yi == GRID_SEARCH_ERROR) == (xi == GRID_SEARCH_ERROR))
    for kind in ("far", "nonfinite"):
        assert not found[sl[kind]].any(), kind
    ri = np.r_[np.arange(x.size)[sl["random"]], np.arange(x.size)[sl["interior"]]]
    frac = ok[ri].mean()
    print(f"{name}/{mesh}: {ri.size} random + interior points, {found[ri].sum()} found, stable fraction {frac:.5f}")
    assert frac >= 0.99, frac
    if name != "coarse_global":  # (there a face's hash box does not cover the whole curved cell: see below)
        # (on a flat mesh in metres a near-parallelogram cell's bilinear inverse cancels and misses some of its own points, index_search.py:122-177)
        assert found[sl["interior"]].mean() > (0.99 if mesh == "spherical" else 0.9)
    if name == "masked":  # faces with a NaN corner are not listed: a point in the block is in no cell
        lon, lat = cmf.family("warped", mesh)
        j, i = cmf.MASK_ROWS.start, cmf.MASK_COLS.start
        cy, cx = oracle_at(case, lon[j:j + 2, i:i + 2].mean(), lat[j:j + 2, i:i + 2].mean())
        assert cy == cx == GRID_SEARCH_ERROR


def oracle_at(case, x, y):
    yi, xi = cmf.oracle_search(case, np.array([x]), np.array([y]))
    return int(yi[0]), int(xi[0])


def test_coarse_global_has_unlisted_parts_of_cells():
    """Bit width bisected to about 200, and interior points of a cell that the oracle cannot find there: the xyz box of the four
    corners does not cover the whole curved cell (the `listed` rule of the neighbour probe)."""
    case = cmf.mesh_case("coarse_global")
    assert 100 < case["hash_table"]["bitwidth"] < 400, case["hash_table"]["bitwidth"]
    q = cmf.query_points(case["lon"], case["lat"], N_RANDOM, seed=11)
    yi, _ = cmf.oracle_search(case, *q["interior"])
    assert (yi == GRID_SEARCH_ERROR).sum() >= 1


def _band_end(name, ref):
    return cmf.in_band(name, ref["x"], ref["y"])


@pytest.mark.parametrize("name,mesh", cmf.FAMILY_MESHES)
def test_oracle_runs_the_trajectory_case(name, mesh):
    case = cmf.trajectory_case(name, mesh)
    n = len(case["x"])
    assert case["band_release"].sum() == (n // 4 if cmf.FAMILIES[name]["band"] is not None else 0)
    ref, err, stats = run_oracle(case)
    assert err is None, err  # DeleteParticle removes what leaves the mesh
    assert stats["steps"] > 10 * n
    assert len(ref["x"]) >= 0.3 * n, len(ref["x"])
    assert np.all(ref["state"] < 50)
    if case["lon"].shape[1] == 2:  # a particle that leaves a mesh one cell wide raises IndexError in the reference (trajectory_case)
        assert len(ref["x"]) == n
    if name == "self_overlap":
        assert _band_end(name, ref).sum() >= 100
        assert handed_to_the_first_columns(case, ref) >= 20
    if name == "masked":
        c2 = dict(case, kernels=["AdvectionRK4"])
        ref2, err2, _ = run_oracle(c2)
        assert err2 == "GridSearchingError" and (ref2["state"] == STATE_GRID_SEARCHING).sum() >= 1


def handed_to_the_first_columns(case, ref):
    """Particles of `self_overlap` released in column 49 west of the doubly covered band (lon < 175, a cell only column 49 covers)
    that end in columns 0 / 1: they left their guessed cell inside the band, where columns 49 / 50 hold the point as well and the
    table order hands it to the lowest face id.  These are the particles a neighbour probe would keep in columns 49 / 50."""
    nx = case["lon"].shape[1]
    ids = ref["particle_id"]
    x0 = np.asarray(case["x"])[ids]
    xi_end = np.mod(ref["ei"][:, 0].astype(np.int64), nx - 1)
    return int(((x0 >= 172.7) & (x0 < 175.0) & (xi_end <= 1)).sum())


# ---- against the reference itself (where its tree is present) ------------------------------------------------------------------
def _reference_available():
    from oracle import ref_shim

    return ref_shim.reference_available()


needs_reference = pytest.mark.skipif(not _reference_available(), reason="reference tree not present")


@needs_reference
@pytest.mark.parametrize("name,mesh", [("one_cell", "spherical"), ("two_columns", "spherical"), ("two_columns", "flat")])
def test_a_mesh_one_cell_wide_is_never_searched_with_a_guess(name, mesh):
    """"Have a guess" is np.any(xi) over the guesses (index_search.py:269).  On a mesh one cell wide every xi is 0, so the reference
    runs the unguessed hash query -- table order, float32 (xsi, eta) -- at EVERY evaluation, not only the first.  The oracle (and
    pk_device.h: grid_search) once took the guess from the second evaluation on: 1e-8 relative in the positions of these cases."""
    from oracle import make_golden as mg

    case = cmf.trajectory_case(name, mesh, npart=400)
    ref, rerr, _ = mg.ref_run_case(case)
    got, oerr, _ = run_oracle(case)
    assert rerr is None and oerr is None and len(ref["x"]) == len(case["x"])
    for k in ("particle_id", "x", "y", "z", "t", "state", "ei"):
        assert np.array_equal(got[k], ref[k]), k


@needs_reference
def test_self_overlap_oracle_equals_the_reference():
    """In the doubly covered band the reference returns the first listed face in table order (the lowest face id), and so does the
    oracle: the trajectories that the GPU test compares with are the reference's."""
    from oracle import make_golden as mg

    case = cmf.trajectory_case("self_overlap", npart=800)
    ref, rerr, _ = mg.ref_run_case(case)
    got, oerr, _ = run_oracle(case)
    assert rerr == oerr and np.array_equal(got["particle_id"], ref["particle_id"])
    assert handed_to_the_first_columns(case, ref) >= 5
    assert np.array_equal(got["ei"], ref["ei"]) and np.array_equal(got["state"], ref["state"]) and np.array_equal(got["t"], ref["t"])
    for k in ("x", "y", "z"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=1e-12 * 187.3)
