"""The curvilinear search layer (csrc/pk_device.h: curvilinear_search) on the mesh families of tests/curv_mesh_families.py.

Four accelerators sit around the plain table walk -- the key directory ("hash_directory"), the per-cell records ("cell_table"), the
per-lane LDS copy of the last cell ("cell_cache") and the neighbour probe -- and each claims to return exactly what the walk returns.
Here every one of them is switched off against the all-on engine, bit for bit (rtol 0): all paths call the same inline functions
(spherical_project_cell, bilinear_inverse, quantize), the library is built with -ffp-contract=off, and a probe hit is rounded like a
hash hit.  pk_search is compared with the CPU oracle's po_hash_query point for point on the stable points of a query set, and every
family's trajectories with the oracle at the 1e-12 class of the populated curvilinear runs, discrete columns exactly.

General programs only (fast_path = 0, fast_cgrid = 0) except in the last test, which runs the defaults on C-grid fields."""

from __future__ import annotations

import functools
import warnings

import numpy as np
import pytest

import curv_mesh_families as cmf
from case_utils import build_fieldset, build_pset, compare, run_hip, run_oracle

pytestmark = pytest.mark.gpu

GRID_SEARCH_ERROR = -3
STATE_GRID_SEARCHING = 52
N_RANDOM = 3000
GENERAL = {"fast_path": 0, "fast_cgrid": 0}
# what each comparison switches off: options for pk_set_option before the grid exists, and the neighbour_probe keyword
SEARCH_VARIANTS = {
    "hash_directory=0": dict(options={"hash_directory": 0}),
    "cell_table=0": dict(options={"cell_table": 0}),
    "both off": dict(options={"hash_directory": 0, "cell_table": 0}),
    "host-built table": dict(hash_build="host"),
}
TRAJECTORY_VARIANTS = {
    "hash_directory=0": dict(options={"hash_directory": 0}),
    "cell_table=0": dict(options={"cell_table": 0}),
    "cell_cache=0": dict(options={"cell_cache": 0}),
    "neighbour_probe=-1": dict(neighbour_probe=-1),
    "all four off": dict(options={"hash_directory": 0, "cell_table": 0, "cell_cache": 0}, neighbour_probe=-1),
}
PROBE_CLASS = {"halo_exact": 0, "halo_plus360": 0, "pole_row": 0, "self_overlap": 0,
               "warped": 1, "fine_patch": 1, "antimeridian_continuous": 1, "antimeridian_wrapped": 1}


def _engine(case, *, options=None, **kw):
    from parcels_amd.engine import DeviceEngine

    fs = build_fieldset(case)
    fs.__dict__["_engine"] = DeviceEngine(fs, options=dict(GENERAL, **(options or {})), **kw)  # what FieldSet.to_device does, plus the switches
    return fs


def _xdim(case):
    return case["lon"].shape[1] - 1  # A-grid: one cell per node interval


def _ravel(case, yi, xi):
    return (xi.astype(np.int64) + yi.astype(np.int64) * _xdim(case)).astype(np.int32)  # z = 10 m lies in level 0


# ---- pk_search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mesh", cmf.FAMILY_MESHES)
def test_search_switches_return_the_plain_walk_and_the_oracle(gpu, name, mesh):
    case = cmf.trajectory_case(name, mesh, npart=8)
    x, y, sl = cmf.flatten_queries(cmf.query_points(case["lon"], case["lat"], N_RANDOM, seed=11, mesh=mesh))
    z = np.full(x.size, 10.0)
    eng = _engine(case)._engine
    base = eng.search(0, z, y, x)
    assert base.shape == x.shape
    for label, kw in SEARCH_VARIANTS.items():
        other = _engine(case, **kw)._engine.search(0, z, y, x)
        assert np.array_equal(other, base), f"{name}/{mesh}: {label}: pk_search differs at {np.flatnonzero(other != base)[:8]}"
    # the oracle, on the stable points (nodes and edge midpoints lie on cell boundaries: A/B only)
    mcase = cmf.mesh_case(name, mesh)
    ok, yi, xi = cmf.stable_mask(mcase, x, y)
    want = _ravel(case, yi, xi)
    use = np.zeros(x.size, bool)
    for kind in ("random", "interior", "far"):
        use[sl[kind]] = ok[sl[kind]]
    use[sl["nonfinite"]] = True  # in no cell for the oracle, stable or not
    assert use[sl["random"]].mean() >= 0.99 and use[sl["interior"]].mean() >= 0.99
    bad = np.flatnonzero(use & (base != want))
    assert bad.size == 0, f"{name}/{mesh}: pk_search differs from po_hash_query at {bad[:8]}: x {x[bad[:4]]}, y {y[bad[:4]]}, got {base[bad[:4]]}, want {want[bad[:4]]}"
    if name == "coarse_global":  # interior points of a cell that its hash box does not cover: in no cell for the reference, and for pk_search
        lost = use & (yi == GRID_SEARCH_ERROR)
        lost[: sl["interior"].start] = False
        lost[sl["interior"].stop:] = False
        assert lost.sum() >= 1 and np.array_equal(base[lost], want[lost])
    for n in (1, 63, 64, 65, 0):  # query counts around the wavefront size
        got = eng.search(0, z[:n], y[:n], x[:n])
        assert got.shape == (n,) and np.array_equal(got, base[:n]), n


@pytest.mark.parametrize("name,mesh", cmf.FAMILY_MESHES)
def test_neighbour_probe_classification(gpu, name, mesh):
    """hash_table(0)["neighbour_probe"]: off on the meshes that cover a point twice, on where they cannot.  (The other families are
    printed: their class follows from the same three scans and no test depends on it.)"""
    got = _engine(cmf.trajectory_case(name, mesh, npart=8))._engine.hash_table(0)["neighbour_probe"]
    print(f"{name}/{mesh}: neighbour_probe {got}")
    if name in PROBE_CLASS:
        assert got == PROBE_CLASS[name]


# ---- trajectories -------------------------------------------------------------------------------------------------------------
def _run(case, *, options=None, neighbour_probe=0):
    import parcels_amd as pa

    fs = _engine(case, options=options, neighbour_probe=neighbour_probe)
    pset = build_pset(case, fs)
    pset.populate_indices()
    kernels = [getattr(pa.kernels, k) for k in case["kernels"]]
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute(kernels, dt=float(case["dt"]), runtime=float(case["runtime"]))
        except (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.FieldInterpolationError, pa.GridSearchingError,
                pa.OutsideTimeInterval, pa.GeneralError) as e:
            err = type(e).__name__
    return {k: np.array(v) for k, v in pset._data.items()}, err, dict(pset._last_stats)


@functools.lru_cache(maxsize=None)
def _baseline(name, mesh):
    """The all-on run of a family and the oracle's: computed once, shared by the tests below, never modified."""
    case = cmf.trajectory_case(name, mesh)
    got = _run(case)
    ref = run_oracle(case)
    for d in (got[0], ref[0]):
        for a in d.values():
            a.setflags(write=False)
    return case, got, ref


@pytest.mark.parametrize("name,mesh", cmf.FAMILY_MESHES)
def test_trajectory_switches_are_bit_exact(gpu, name, mesh):
    case, (base, berr, bstats), _ = _baseline(name, mesh)
    assert bstats["steps"] > 10 * len(case["x"])
    for label, kw in TRAJECTORY_VARIANTS.items():
        got, gerr, gstats = _run(case, **kw)
        assert gerr == berr, label
        assert gstats["steps"] == bstats["steps"], (label, gstats["steps"], bstats["steps"])
        compare(got, base, rtol=0.0, check_state="all", skip=(), label=f"{name}/{mesh}: {label} vs all on")


def _band_of(case, name, ref):
    if cmf.FAMILIES[name]["band"] == "mask":
        return case["band_release"][ref["particle_id"]]
    return cmf.in_band(name, ref["x"], ref["y"])


@pytest.mark.parametrize("name,mesh", cmf.FAMILY_MESHES)
def test_trajectories_equal_the_oracle(gpu, name, mesh):
    case, (got, gerr, _), (ref, rerr, _) = _baseline(name, mesh)
    assert gerr == rerr
    scale = cmf.coordinate_scale(case["lon"], case["lat"])
    rep = compare(got, ref, rtol=1e-12, atol_pos=1e-12 * scale, check_state="all", skip=(), label=f"{name}/{mesh} vs oracle")
    assert np.array_equal(got["particle_id"], ref["particle_id"])  # the deleted set
    band = _band_of(case, name, ref)
    if cmf.FAMILIES[name]["band"] is not None:
        assert band.sum() >= 50, band.sum()
    assert np.array_equal(got["ei"][band], ref["ei"][band]), rep
    print(f"{name}/{mesh}: {len(ref['x'])} of {len(case['x'])} particles left, {band.sum()} in the band, max rel diff {max(rep.values()):.2e}")


def test_masked_mesh_stops_with_the_grid_searching_error(gpu):
    """Without the recovery kernel a particle that walks into the NaN block ends with the grid-searching error code, in the oracle
    and on the device, and the run stops where the reference's batch loop stops."""
    for mesh in cmf.FAMILIES["masked"]["meshes"]:
        case = cmf.trajectory_case("masked", mesh, kernels=["AdvectionRK4"])
        ref, rerr, _ = run_oracle(case)
        assert rerr == "GridSearchingError" and (ref["state"] == STATE_GRID_SEARCHING).sum() >= 1
        got, gerr, _ = _run(case)
        assert gerr == rerr
        scale = cmf.coordinate_scale(case["lon"], case["lat"])
        compare(got, ref, rtol=1e-12, atol_pos=1e-12 * scale, check_state="all", skip=(), label=f"masked/{mesh} without DeleteParticle")


def test_self_overlap_differs_from_the_oracle_with_the_probe_forced_on(gpu):
    """The overlap case has teeth: with neighbour_probe = 1 a particle that leaves its cell inside the doubly covered band is handed
    the neighbour (columns 49 / 50) where the reference's table order gives the lowest face id (columns 0 / 1).  The automatic
    setting finds the overlap (a node strictly inside a cell it is not a corner of) and keeps the table order."""
    case, (auto, _, _), (ref, _, _) = _baseline("self_overlap", "spherical")
    forced, ferr, _ = _run(case, neighbour_probe=1)
    both = np.intersect1d(forced["particle_id"], ref["particle_id"])
    f = forced["ei"][np.searchsorted(forced["particle_id"], both)]
    r = ref["ei"][np.searchsorted(ref["particle_id"], both)]
    band = cmf.in_band("self_overlap", ref["x"], ref["y"])[np.searchsorted(ref["particle_id"], both)]
    differ = (f != r).any(axis=1)
    print(f"self_overlap, probe forced on: ei differs from the oracle for {differ.sum()} particles, {(differ & band).sum()} of them in the band")
    assert (differ & band).sum() >= 1
    band_auto = cmf.in_band("self_overlap", ref["x"], ref["y"])
    assert np.array_equal(auto["particle_id"], ref["particle_id"]) and np.array_equal(auto["ei"][band_auto], ref["ei"][band_auto])


# ---- one leg with the defaults ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["warped", "fine_patch", "antimeridian_continuous", "coarse_global"])
def test_defaults_on_cgrid_fields_equal_the_oracle(gpu, name):
    """The dedicated kernels on (whatever the launch plan picks for C-grid U, V, W and AdvectionRK4_3D), against the oracle at the
    class of tests/test_gpu_fast_cgrid.py::_check.  Which program ran is printed, not asserted."""
    case = cmf.trajectory_case(name, "spherical", cgrid=True)
    got, gerr, stats = run_hip(case)
    ref, rerr, _ = run_oracle(case)
    print(f"{name}: program {stats['program']}, {len(ref['x'])} of {len(case['x'])} particles left")
    assert gerr == rerr
    scale = cmf.coordinate_scale(case["lon"], case["lat"])
    compare(got, ref, rtol=1e-12, atol_pos=1e-12 * scale, check_state="all", skip=(), label=f"{name} C-grid, defaults vs oracle")
