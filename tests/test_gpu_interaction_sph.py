"""GPU: great-circle neighbour search on spherical meshes (parcels_amd/interaction.py with mesh=..., csrc/pk_neighbors.hip) against
brute force over all pairs, written here in NumPy from the semantics of DESIGN.md section 13.  dx / dy / dz use only IEEE operations and
must match bit for bit; dist goes through sin, cos and arcsin, which differ by ulps between the device and NumPy, so it is held to the
package's parity bar of 1e-12 relative (exact zeros stay exact).  Membership and the arg-min are only defined up to that tolerance: every
case first asserts on the oracle alone that no pair sits within 1e-9 (relative) of the radius and that no row's two smallest distances
are within 1e-9 of each other unless they are bit-identical.  Nothing is left out of a comparison."""

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import interaction
from parcels_amd.xgrid import EARTH_RADIUS, FlatMesh, SphericalMesh

pytestmark = pytest.mark.gpu

RAD = np.pi / 180
RTOL = 1e-12


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def brute(x, y, z, radius, R=EARTH_RADIUS, sources=None, include_coincident=True):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(x)
    out = {"n": n, "radius": radius}
    if n == 0:
        e = np.zeros(0)
        out.update(count=np.zeros(0, np.int64), starts=np.zeros(1, np.int64), i=np.zeros(0, np.int64), j=np.zeros(0, np.int64), dx=e, dy=e, dz=e,
                   dist=e, near_j=np.zeros(0, np.int64), near_d=e, all_dist=np.zeros((0, 0)), member=np.zeros((0, 0), bool))
        return out
    valid = np.isfinite(x) & np.isfinite(y) & (np.abs(y) <= 90)
    if z is not None:
        z = np.asarray(z, dtype=np.float64)
        valid &= np.isfinite(z)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[None, :] - x[:, None]
        dx = d - 360 * np.rint(d / 360)
        dy = y[None, :] - y[:, None]
        a = np.sin(0.5 * RAD * dy) ** 2 + np.cos(RAD * y[:, None]) * np.cos(RAD * y[None, :]) * np.sin(0.5 * RAD * dx) ** 2
        dist = 2 * R * np.arcsin(np.minimum(1, np.sqrt(a)))
        dz = None
        if z is not None:
            dz = z[None, :] - z[:, None]
            dist = np.sqrt(dist * dist + dz * dz)
    pair_ok = valid[:, None] & valid[None, :]
    np.fill_diagonal(pair_ok, False)
    dist = np.where(pair_ok, dist, np.inf)
    m = dist < radius
    if not include_coincident:
        m &= dist > 0
    if sources is not None:
        m &= np.asarray(sources, dtype=bool)[None, :]
    i, j = np.nonzero(m)  # row-major: i ascends, j ascends within a row
    count = m.sum(axis=1).astype(np.int64)
    masked = np.where(m, dist, np.inf)
    near_j = np.argmin(masked, axis=1).astype(np.int64)  # the first minimum: ties to the smallest j
    near_d = masked[np.arange(n), near_j]
    near_j[np.isinf(near_d)] = -1
    out.update(count=count, starts=np.concatenate([[0], np.cumsum(count)]).astype(np.int64), i=i.astype(np.int64), j=j.astype(np.int64), dx=dx[i, j],
               dy=dy[i, j], dz=dz[i, j] if dz is not None else None, dist=dist[i, j], near_j=near_j, near_d=near_d, all_dist=dist, member=masked)
    return out


def assert_preconditions(ref):
    """on the oracle alone: membership and the arg-min do not hinge on the last ulps of sin / cos / arcsin"""
    if ref["n"] < 2:
        return
    d = ref["all_dist"]
    finite = np.isfinite(d)
    assert not (np.abs(d[finite] / ref["radius"] - 1) <= 1e-9).any(), "a pair sits within 1e-9 of the radius: choose another seed"
    two = np.sort(ref["member"], axis=1)[:, :2]
    d1, d2 = two[:, 0], two[:, 1]
    both = np.isfinite(d2)
    with np.errstate(invalid="ignore"):
        d2 = np.where(both, d2, 1.0)
        d1 = np.where(both, d1, 0.0)
    close = both & (np.abs(d2 - d1) <= 1e-9 * d2) & (d1 != d2)
    assert not close.any(), "a row's two nearest candidates are within 1e-9 but not identical: choose another seed"


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def close(got, ref):
    """within 1e-12 relative; zeros and infinities exactly"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != np.float64 or got.shape != ref.shape:
        return False
    special = (ref == 0) | np.isinf(ref)
    if not np.array_equal(got[special], ref[special]):
        return False
    err = np.abs(got[~special] - ref[~special]) / ref[~special]
    if err.size:
        print(f"max relative difference of dist: {err.max():.3e}")
    return bool((err <= RTOL).all())


def check_all(points, radius, mesh="spherical", R=EARTH_RADIUS, **kw):
    """neighbors + neighbor_counts + nearest_neighbor of `points` against brute force; returns (Neighbors, oracle)."""
    z = points[2] if kw.get("z") else None
    ref = brute(points[0], points[1], z, radius, R, kw.get("sources"), kw.get("include_coincident", True))
    assert_preconditions(ref)
    n = ref["n"]
    nb = pa.neighbors(points, radius, mesh=mesh, **kw)
    assert nb.count.dtype == np.int64 and nb.starts.dtype == np.int64 and nb.i.dtype == np.int64 and nb.j.dtype == np.int64
    assert nb.count.shape == (n,) and nb.starts.shape == (n + 1,)
    assert np.array_equal(nb.count, ref["count"])
    assert np.array_equal(nb.starts, ref["starts"])
    assert np.array_equal(nb.i, ref["i"])
    assert np.array_equal(nb.j, ref["j"])
    assert same_bits(nb.dx, ref["dx"]) and same_bits(nb.dy, ref["dy"])
    assert close(nb.dist, ref["dist"])
    if z is not None:
        assert same_bits(nb.dz, ref["dz"])
    else:
        assert not hasattr(nb, "dz")
    counts = pa.neighbor_counts(points, radius, mesh=mesh, **kw)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref["count"])
    nj, nd = pa.nearest_neighbor(points, radius, mesh=mesh, **kw)
    assert nj.dtype == np.int64 and np.array_equal(nj, ref["near_j"])
    assert close(nd, ref["near_d"])
    return nb, ref


def on_sphere(rng, n):
    return rng.uniform(-180, 180, n), np.degrees(np.arcsin(rng.uniform(-1, 1, n)))


# ---- 1. the issue's seeded sets ------------------------------------------------------------------------------------------------
def global_points():
    return on_sphere(np.random.default_rng(11), 1500)


def test_global(gpu):
    nb, _ = check_all(global_points(), 300e3)
    assert nb.total == 1254
    info = interaction.cell_list_info_spherical()
    assert info["periodic"] and info["n"] == info["nvalid"] == 1500
    assert info["bands"] > 30 and info["cells"] > info["bands"]
    assert interaction.cell_list_info()["ncx"] == 0  # the flat report is empty after a spherical build


POLE_PAIRS = 13718


def pole_points():
    """Seed 23, not 12: the two points at the pole are equally far from everything up to the ulps of cos(pi / 2), so a particle whose
    nearest neighbour is the pole breaks the second precondition.  With colatitudes uniform in (0, 3) degrees most seeds have one
    (12 has particle 160); 23 is the first from 12 on with none, north and south."""
    rng = np.random.default_rng(23)
    colat = rng.uniform(0, 3, 600)
    x = rng.uniform(0, 360, 600)
    y = 90 - colat
    x[0], y[0] = 0.0, 90.0
    x[1], y[1] = 123.0, 90.0
    return x, y


@pytest.mark.parametrize("south", [False, True])
def test_poles(gpu, south):
    x, y = pole_points()
    nb, ref = check_all((x, -y if south else y), 50e3)
    assert nb.total == POLE_PAIRS
    k = nb.starts[0] + np.searchsorted(nb.j[nb.starts[0]:nb.starts[1]], 1)
    assert nb.j[k] == 1 and nb.dist[k] < 1e-6 and nb.dx[k] == 123.0  # the pole twice: one place up to cos(pi / 2) = 6e-17, whatever dx


def antimeridian_points():
    rng = np.random.default_rng(13)
    x = rng.uniform(179, 181, 800)
    x = x + 360.0 * (rng.integers(0, 3, 800) - 1)
    y = rng.uniform(-2, 2, 800)
    return x, y


def test_antimeridian_mixed_representations(gpu):
    x, y = antimeridian_points()
    assert x.min() < -179 and x.max() > 539
    nb, _ = check_all((x, y), 20e3)
    assert nb.total == 7458
    assert np.abs(nb.dx).max() < 1.0 and np.abs(x[nb.j] - x[nb.i]).max() > 700  # wrapped: the direction an Attract kernel needs
    info = interaction.cell_list_info_spherical()
    assert not info["periodic"] and info["cells"] > 20  # a 2-degree arc across the antimeridian, not the globe


def test_metres_scale_regional_set(gpu):
    rng = np.random.default_rng(14)
    deg = 1.0 / (EARTH_RADIUS * RAD)  # degrees of latitude per metre
    x = 10.0 + rng.uniform(0, 100, 500) * deg / np.cos(60 * RAD)
    y = 60.0 + rng.uniform(0, 100, 500) * deg
    nb, _ = check_all((x, y), 5.0)
    assert nb.total == 1814
    info = interaction.cell_list_info_spherical()
    assert info["cells"] >= 100 and not info["periodic"]  # the cell list of the box, not one cell of a global grid
    assert info["cells"] <= 21 * 21 and info["bands"] <= 21


def test_three_dimensional(gpu):
    rng = np.random.default_rng(15)
    x, y, z = rng.uniform(-0.5, 0.5, 700), rng.uniform(44.5, 45.5, 700), rng.uniform(-6000, 0, 700)
    nb3, _ = check_all((x, y, z), 8e3, z=True)
    nb2, _ = check_all((x, y, z), 8e3)
    assert nb3.total == 9610 and nb2.total == 10584
    assert np.any(nb3.dz != 0.0)


def test_large_radius(gpu):
    x, y = on_sphere(np.random.default_rng(16), 400)
    nb, _ = check_all((x, y), 9.0e6)  # the limit is (pi / 2) R = 1.00008e7
    assert nb.total == 67436
    info = interaction.cell_list_info_spherical()
    assert info["bands"] <= 3 and info["cells"] <= 2 * info["bands"]  # every band one or two cells wide: none is visited twice


# ---- 2. ties, coincident points -------------------------------------------------------------------------------------------------
def test_mirrored_points_tie_exactly(gpu):
    x = np.array([10.5, 10.0, 9.5, 200.0])  # 0 and 2 mirrored east and west of 1
    y = np.array([37.0, 37.0, 37.0, 0.0])
    nb, ref = check_all((x, y), 60e3)
    assert np.array_equal(nb.count, [1, 2, 1, 0])
    row = slice(nb.starts[1], nb.starts[2])
    assert np.array_equal(nb.j[row], [0, 2]) and nb.dist[row][0] == nb.dist[row][1] and ref["dist"][1] == ref["dist"][2]
    nj, nd = pa.nearest_neighbor((x, y), 60e3, mesh="spherical")
    assert nj[1] == 0 and nj[3] == -1 and np.isinf(nd[3])


@pytest.mark.parametrize("include_coincident", [True, False])
def test_coincident_points_modulo_360(gpu, include_coincident):
    rng = np.random.default_rng(21)
    x = np.round(rng.uniform(-20, 20, 200) * 64) / 64  # on a lattice of 1/64: x +- 360 is exact
    y = rng.uniform(50, 60, 200)
    x = np.concatenate([x, x[:40] + 360.0, x[40:80] - 360.0, x[80:100]])
    y = np.concatenate([y, y[:100]])
    nb, ref = check_all((x, y), 150e3, include_coincident=include_coincident)
    zeros = int((nb.dist == 0).sum())
    assert zeros == (200 if include_coincident else 0) and int((ref["dist"] == 0).sum()) == zeros
    if include_coincident:
        nj, nd = pa.nearest_neighbor((x, y), 150e3, mesh="spherical")
        assert np.array_equal(nj[:100], np.arange(200, 300)) and np.all(nd[:100] == 0.0)


# ---- 3. masks, invalid points, sizes --------------------------------------------------------------------------------------------
def test_sources_mask(gpu):
    x, y = global_points()
    src = np.zeros(1500, dtype=bool)
    src[np.random.default_rng(22).choice(1500, 300, replace=False)] = True
    nb, _ = check_all((x, y), 300e3, sources=src)
    assert 100 < nb.total < 1254 and src[nb.j].all() and not src[nb.i].all()


def test_invalid_points(gpu):
    x, y = (a.copy() for a in global_points())
    bad = np.arange(0, 1500, 15)
    in_x = [np.nan, np.inf, -np.inf]
    in_y = [np.nan, np.inf, -np.inf, 90.5, -91.0, 1e300, np.nextafter(90.0, 91.0)]
    for k, b in enumerate(bad):  # the ten kinds in turn, ten times each
        if k % 10 < 3:
            x[b] = in_x[k % 10]
        else:
            y[b] = in_y[k % 10 - 3]
    assert np.isposinf(x).sum() == np.isneginf(x).sum() == np.isnan(x).sum() == 10 and (np.abs(y) > 90).sum() == 60
    nb, ref = check_all((x, y), 300e3)
    nj, nd = pa.nearest_neighbor((x, y), 300e3, mesh="spherical")
    assert np.all(nb.count[bad] == 0) and np.all(nj[bad] == -1) and np.all(np.isinf(nd[bad]))
    assert not np.isin(nb.j, bad).any() and nb.total > 800
    assert interaction.cell_list_info_spherical()["nvalid"] == 1500 - len(bad)
    z = np.zeros(1500)
    z[7] = np.nan
    nb3, _ = check_all((x, y, z), 300e3, z=True)
    assert nb3.count[7] == 0 and not (nb3.j == 7).any()


def test_large_finite_longitudes(gpu):
    """Longitudes near 8e14 are valid: x = lon + 360 * 2^41 is exact for lon on a lattice of 1/8, the spacing of float64 there.  The
    cell list then widens its longitude cells by the 5.6 degrees such a set's normalised longitudes may be off by."""
    rng = np.random.default_rng(25)
    lon = rng.integers(0, 81, 600) / 8.0
    x = lon + np.where(rng.integers(0, 2, 600) == 1, 360.0 * 2.0**41, 0.0)
    y = rng.uniform(0, 10, 600)
    assert np.array_equal(x - np.where(x > 1e3, 360.0 * 2.0**41, 0.0), lon) and x.max() > 7.9e14
    nb, _ = check_all((x, y), 30e3)
    assert nb.total > 500 and np.abs(nb.dx).max() <= 0.375 and np.abs(x[nb.j] - x[nb.i]).max() > 7.9e14
    info = interaction.cell_list_info_spherical()
    assert info["periodic"] and info["nvalid"] == 600 and info["cells"] < 64 * info["bands"]


def test_doubled_bands(gpu):
    """A radius of 1 m on the global set: 2e7 bands at the starting height, so the band height is doubled, and the longitude cells
    coarsen with it, until bands and cells are under their caps.  Partners half a metre away give the pairs."""
    x, y = global_points()
    deg = 1.0 / (EARTH_RADIUS * RAD)  # degrees of latitude per metre
    k = np.arange(0, 1500, 30)
    ang = np.random.default_rng(26).uniform(0, 2 * np.pi, len(k))
    x = np.concatenate([x, x[k] + 0.5 * deg * np.cos(ang) / np.cos(y[k] * RAD)])
    y = np.concatenate([y, y[k] + 0.5 * deg * np.sin(ang)])
    nb, _ = check_all((x, y), 1.0)
    assert nb.total == 2 * len(k)
    info = interaction.cell_list_info_spherical()
    assert info["doublings"] >= 8 and 10000 < info["cells"] <= 2**20 and 100 < info["bands"] <= 2**17
    assert info["band_height"] == (1.0 / EARTH_RADIUS) / RAD * (1 + 2.0**-16) * 2.0 ** info["doublings"]


def test_no_valid_point(gpu):
    nb, _ = check_all((np.array([np.nan, 5.0, np.inf]), np.array([0.0, 91.0, 0.0])), 1e5)
    assert nb.total == 0


@pytest.mark.parametrize("n", [0, 1, 2])
def test_sizes(gpu, n):
    x, y = np.array([3.0, 3.5])[:n], np.array([-40.0, -40.25])[:n]
    nb, _ = check_all((x, y), 100e3)
    assert nb.n == n and nb.total == (2 if n == 2 else 0)


def test_band_and_cell_edges(gpu):
    """pairs astride the edge of a band and of a longitude cell, each 0.9 radius apart; the nearest lattice points are 2 radii away"""
    radius = 10e3
    ddeg = radius / (EARTH_RADIUS * RAD)  # the angular radius in degrees: bands are a hair higher than this
    info_pts = np.arange(12) * 2.0 * ddeg
    gx, gy = np.meshgrid(info_pts / np.cos(20 * RAD), 20.0 + info_pts)
    x, y = gx.ravel(), gy.ravel()
    for k in range(1, 10):  # a partner north, one east of lattice points whose band / cell edges fall at ever different offsets
        x = np.append(x, [gx[k, k], gx[k, k + 1] + 0.9 * ddeg / np.cos(y[12 * k + k + 1] * RAD)])
        y = np.append(y, [gy[k, k] + 0.9 * ddeg, gy[k, k + 1]])
    nb, _ = check_all((x, y), radius)
    assert nb.total == 2 * 18
    info = interaction.cell_list_info_spherical()
    assert info["bands"] >= 20 and info["cells"] >= 200


def test_max_pairs(gpu):
    x, y = pole_points()
    with pytest.raises(ValueError, match="max_pairs") as ei:
        pa.neighbors((x, y), 50e3, mesh="spherical", max_pairs=1000)
    assert str(POLE_PAIRS) in str(ei.value) and "1000" in str(ei.value)
    assert pa.neighbors((x, y), 50e3, mesh="spherical", max_pairs=POLE_PAIRS).total == POLE_PAIRS  # the cap itself is allowed


# ---- 4. the mesh argument --------------------------------------------------------------------------------------------------------
def spherical_fieldset():
    from case_utils import build_fieldset, load_golden

    case, _, _ = load_golden("agrid_sph_rk4_f64")
    return build_fieldset(case), np.asarray(case["lon"], dtype=np.float64), np.asarray(case["lat"], dtype=np.float64)


def test_mesh_as_fieldset_and_unit_sphere(gpu):
    fs, _, _ = spherical_fieldset()
    x, y = pole_points()
    ref = brute(x, y, None, 50e3)
    for mesh in (fs, SphericalMesh(), "spherical"):
        nb = pa.neighbors((x, y), 50e3, mesh=mesh)
        assert np.array_equal(nb.j, ref["j"]) and close(nb.dist, ref["dist"])
    unit, _ = check_all((x, y), 50e3 / EARTH_RADIUS, mesh=SphericalMesh(radius=1.0), R=1.0)  # distances in radians
    assert unit.total == POLE_PAIRS and unit.dist.max() < 0.008


def test_flat_is_the_default_and_unchanged(gpu):
    from test_gpu_interaction import brute as flat_brute

    fs, _, _ = spherical_fieldset()
    rng = np.random.default_rng(23)
    x, y = rng.random(700), rng.random(700)
    ref = flat_brute(x, y, None, 0.05)
    pa.neighbors((x, y), 5e3, mesh=fs)  # a spherical list in the context does not leak into the next flat call
    for kw in ({}, {"mesh": "flat"}, {"mesh": FlatMesh()}):
        nb = pa.neighbors((x, y), 0.05, **kw)
        assert np.array_equal(nb.count, ref["count"]) and np.array_equal(nb.j, ref["j"])
        assert same_bits(nb.dx, ref["dx"]) and same_bits(nb.dy, ref["dy"]) and same_bits(nb.dist, ref["dist"])
        assert np.array_equal(pa.neighbor_counts((x, y), 0.05, **kw), ref["count"])
        nj, nd = pa.nearest_neighbor((x, y), 0.05, **kw)
        assert np.array_equal(nj, ref["near_j"]) and same_bits(nd, ref["near_d"])
    assert interaction.cell_list_info()["ncx"] > 1 and interaction.cell_list_info_spherical()["bands"] == 0


# ---- 5. inside a kernel ----------------------------------------------------------------------------------------------------------
R_COUNT = 10e3
SEEN = []


def drift(particles, fieldset):
    particles.dx += np.where(np.asarray(particles.particle_id) % 2 == 0, 0.01, -0.005)


def count_neighbours(particles, fieldset):
    SEEN.append((np.array(particles.x, dtype=np.float64), np.array(particles.y, dtype=np.float64),
                 pa.neighbor_counts(particles, R_COUNT, mesh=fieldset)))


def test_counts_inside_execute(gpu):
    fs, lon, lat = spherical_fieldset()
    rng = np.random.default_rng(24)
    cx, cy = 0.5 * (lon.min() + lon.max()), 0.5 * (lat.min() + lat.max())
    x0, y0 = cx + rng.uniform(-0.4, 0.4, 300), cy + rng.uniform(-0.4, 0.4, 300)
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x0, y=y0, t=np.zeros(300))
    del SEEN[:]
    pset.execute([count_neighbours, drift], dt=1.0, runtime=4.0)
    assert len(SEEN) >= 4
    for x, y, counts in SEEN:
        ref = brute(x, y, None, R_COUNT)
        assert_preconditions(ref)
        assert np.array_equal(counts, ref["count"]) and ref["count"].sum() > 500
    assert not np.array_equal(SEEN[0][0], SEEN[-1][0])  # the positions moved between the steps
