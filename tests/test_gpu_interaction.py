"""GPU: neighbour search for particle-particle interaction kernels (parcels_amd/interaction.py, csrc/pk_neighbors.hip) against brute
force over all pairs, written here in NumPy from the semantics of DESIGN.md section 13.  Within the stated arithmetic brute force is
exact, so every comparison asks for equality: counts, starts and j exactly, dx / dy / dz / dist bit for bit, nearest in index and
distance."""

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import interaction

pytestmark = pytest.mark.gpu


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def brute(x, y, z, radius, sources=None, include_coincident=True):
    """All pairs: dx = x[j] - x[i], dist = sqrt(dx*dx + dy*dy [+ dz*dz]) left to right; neighbour iff i != j, dist < radius,
    sources[j], (dist > 0).  NaN / inf coordinates fall out of `dist < radius` by themselves."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(x)
    out = {"n": n}
    if n == 0:
        e = np.zeros(0)
        out.update(count=np.zeros(0, np.int64), starts=np.zeros(1, np.int64), i=np.zeros(0, np.int64), j=np.zeros(0, np.int64), dx=e, dy=e, dz=e,
                   dist=e, near_j=np.zeros(0, np.int64), near_d=e)
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        dx = x[None, :] - x[:, None]
        dy = y[None, :] - y[:, None]
        s = dx * dx + dy * dy
        dz = None
        if z is not None:
            z = np.asarray(z, dtype=np.float64)
            dz = z[None, :] - z[:, None]
            s = s + dz * dz
        dist = np.sqrt(s)
        m = dist < radius
        if not include_coincident:
            m &= dist > 0
    np.fill_diagonal(m, False)
    if sources is not None:
        m &= np.asarray(sources, dtype=bool)[None, :]
    i, j = np.nonzero(m)  # row-major: i ascends, j ascends within a row
    count = m.sum(axis=1).astype(np.int64)
    masked = np.where(m, dist, np.inf)
    near_j = np.argmin(masked, axis=1).astype(np.int64)  # the first minimum: ties to the smallest j
    near_d = masked[np.arange(n), near_j]
    near_j[np.isinf(near_d)] = -1
    out.update(count=count, starts=np.concatenate([[0], np.cumsum(count)]).astype(np.int64), i=i.astype(np.int64), j=j.astype(np.int64), dx=dx[i, j],
               dy=dy[i, j], dz=dz[i, j] if dz is not None else None, dist=dist[i, j], near_j=near_j, near_d=near_d)
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_all(points, radius, expect=None, **kw):
    """neighbors + neighbor_counts + nearest_neighbor of `points` against brute force; returns (Neighbors, oracle)."""
    z = points[2] if kw.get("z") else None
    ref = expect if expect is not None else brute(points[0], points[1], z, radius, kw.get("sources"), kw.get("include_coincident", True))
    n = ref["n"]
    nb = pa.neighbors(points, radius, **kw)
    assert nb.count.dtype == np.int64 and nb.starts.dtype == np.int64 and nb.i.dtype == np.int64 and nb.j.dtype == np.int64
    assert nb.count.shape == (n,) and nb.starts.shape == (n + 1,)
    assert np.array_equal(nb.count, ref["count"])
    assert np.array_equal(nb.starts, ref["starts"])
    assert np.array_equal(nb.i, ref["i"])
    assert np.array_equal(nb.j, ref["j"])
    assert same_bits(nb.dx, ref["dx"]) and same_bits(nb.dy, ref["dy"]) and same_bits(nb.dist, ref["dist"])
    if z is not None:
        assert same_bits(nb.dz, ref["dz"])
    else:
        assert not hasattr(nb, "dz")
    counts = pa.neighbor_counts(points, radius, **kw)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref["count"])
    nj, nd = pa.nearest_neighbor(points, radius, **kw)
    assert nj.dtype == np.int64 and np.array_equal(nj, ref["near_j"])
    assert same_bits(nd, ref["near_d"])
    return nb, ref


# ---- 1. uniform ----------------------------------------------------------------------------------------------------------------
def test_uniform(gpu):
    rng = np.random.default_rng(1)
    x, y = rng.random(1500), rng.random(1500)
    nb, ref = check_all((x, y), 0.05)
    assert 5000 < nb.total < 30000  # ~ n^2 pi r^2
    assert same_bits(nb.sum(nb.dist), np.bincount(ref["i"], weights=ref["dist"], minlength=1500))


# ---- 2. clusters and ties ------------------------------------------------------------------------------------------------------
def cluster_points():
    rng = np.random.default_rng(2)
    radius = 0.02
    centres = rng.random((40, 2))
    which = rng.integers(0, 40, 1000 - 64)
    p = centres[which] + rng.uniform(-radius / 3, radius / 3, (1000 - 64, 2))
    dup = p[rng.integers(0, len(p), 64)]  # exact duplicates of other points
    p = np.concatenate([p, dup])
    p = p[rng.permutation(1000)]
    return p[:, 0].copy(), p[:, 1].copy(), radius


@pytest.mark.parametrize("include_coincident", [True, False])
def test_clusters_and_duplicates(gpu, include_coincident):
    x, y, radius = cluster_points()
    nb, ref = check_all((x, y), radius, include_coincident=include_coincident)
    zero = int((ref["dist"] == 0).sum())
    assert (zero >= 128) if include_coincident else (zero == 0)
    assert nb.total > 10000


def test_lattice_ties_go_to_the_smallest_index(gpu):
    gy, gx = np.divmod(np.arange(400), 20)
    x, y = gx.astype(np.float64), gy.astype(np.float64)
    nb, ref = check_all((x, y), 1.5)
    nj, nd = pa.nearest_neighbor((x, y), 1.5)
    interior = (gx > 0) & (gx < 19) & (gy > 0) & (gy < 19)
    assert np.all(nb.count[interior] == 8)
    assert np.all(nd[interior] == 1.0)
    assert np.array_equal(nj[interior], np.arange(400)[interior] - 20)  # of the four at distance 1, (gy - 1, gx) has the smallest index


# ---- 3. boundaries -------------------------------------------------------------------------------------------------------------
def test_cell_edges_and_the_strict_radius(gpu):
    r = 0.25
    below = np.nextafter(0.25, 0)
    k = np.arange(9)
    lx, ly = np.meshgrid(-1.0 + k * r, 2.0 + k * r)  # every point on a cell edge, neighbours at exactly the radius
    extra = np.array([
        [0.0, 8.0], [below, 8.0],             # 0 - 1: just inside in x (the difference is exact)
        [5.0, 0.0], [5.0, below],             # 2 - 3: just inside in y
        [7.0, 5.125], [7.25, 5.125],          # 4 - 5: exactly the radius
        [7.0, 5.375],                         # 4 - 6: exactly the radius
        [-1.2499, 2.0], [-1.0, 1.7501],       # inside of the lattice corner (-1, 2), moving the bounding box off the lattice
    ])
    x = np.concatenate([lx.ravel(), extra[:, 0]])
    y = np.concatenate([ly.ravel(), extra[:, 1]])
    nb, ref = check_all((x, y), r)
    pairs = set(zip(nb.i.tolist(), nb.j.tolist()))
    e = 81
    assert (e, e + 1) in pairs and (e + 1, e) in pairs and (e + 2, e + 3) in pairs and (e + 3, e + 2) in pairs
    assert (e + 4, e + 5) not in pairs and (e + 4, e + 6) not in pairs
    assert (0, e + 7) in pairs and (0, e + 8) in pairs
    assert (0, 1) not in pairs and (0, 9) not in pairs  # lattice neighbours sit at exactly 0.25
    assert np.all(nb.count[:81] <= 2)


# ---- 4. coarsened cells --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0.0, 1.0e9])
def test_coarsened_cells(gpu, base):
    """Two groups 1e7 radii apart: the cell count at the starting cell size is far over the cap, so the cells are doubled.  radius =
    2^-24 is half the float64 spacing near 1e9 (2^-23): after the shift a point moved by the radius alone would coincide with its
    neighbour, so x sits on that lattice (neighbours share their x) and the radius is resolved in y only."""
    radius = 2.0**-24
    rng = np.random.default_rng(4)
    xs, ys = [], []
    for g in range(2):
        gx = base + g * np.round(1.0e7 * radius / 2.0**-23) * 2.0**-23 + rng.integers(0, 4, 256) * 2.0**-23
        xs.append(gx)
        ys.append(rng.uniform(0.0, 8.0 * radius, 256))
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert np.all(np.diff(np.unique(x)) >= 2 * radius)  # the lattice survived the shift
    ref = brute(x, y, None, radius)
    assert ref["count"].sum() > 1000 and (ref["count"] < 255).all()  # both neighbours and non-neighbours
    check_all((x, y), radius, expect=ref)
    info = interaction.cell_list_info()
    assert info["doublings"] > 0 and info["ncx"] * info["ncy"] <= max(2**20, 4 * 512)
    assert info["cell_size"] == radius * (1 + 2.0**-16) * 2.0 ** info["doublings"]


# ---- 5. non-finite coordinates -------------------------------------------------------------------------------------------------
def test_non_finite_coordinates(gpu):
    rng = np.random.default_rng(5)
    x, y = rng.random(500), rng.random(500)
    bad = np.arange(0, 500, 10)
    vals = np.array([np.nan, np.inf, -np.inf])
    for k, b in enumerate(bad):
        (x if k % 2 else y)[b] = vals[k % 3]
    nb, ref = check_all((x, y), 0.08)
    nj, nd = pa.nearest_neighbor((x, y), 0.08)
    assert np.all(nb.count[bad] == 0) and np.all(nj[bad] == -1) and np.all(np.isinf(nd[bad]))
    assert not np.isin(nb.j, bad).any() and nb.total > 1000
    z = rng.random(500) * 0.01
    z[7] = np.nan  # finite in (x, y), not in z
    nb3, _ = check_all((x, y, z), 0.08, z=True)
    assert nb3.count[7] == 0 and not (nb3.j == 7).any()
    assert interaction.cell_list_info()["nvalid"] == 500 - len(bad) - 1


def test_all_points_non_finite(gpu):
    x = np.array([np.nan, np.inf, 1.0])
    y = np.array([0.0, 0.0, np.nan])
    nb, _ = check_all((x, y), 1.0)
    assert nb.total == 0


# ---- 6. sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_sizes(gpu, n):
    rng = np.random.default_rng(60 + n)
    x, y = rng.random(n), rng.random(n)
    nb, _ = check_all((x, y), 0.2)
    assert nb.n == n and nb.sum(np.ones(nb.total)).shape == (n,)


def all_pairs_points():
    rng = np.random.default_rng(6)
    return rng.random(300), rng.random(300)


def test_radius_larger_than_the_domain(gpu):
    x, y = all_pairs_points()
    nb, _ = check_all((x, y), 10.0)
    assert nb.total == 300 * 299 and np.all(nb.count == 299)


# ---- 7. masks and z ------------------------------------------------------------------------------------------------------------
def test_sources_mask(gpu):
    rng = np.random.default_rng(7)
    x, y = rng.random(800), rng.random(800)
    src = np.zeros(800, dtype=bool)
    src[rng.choice(800, 5, replace=False)] = True
    nb, _ = check_all((x, y), 0.2, sources=src)
    assert nb.total > 50 and src[nb.j].all() and not src[nb.i].all()
    none, _ = check_all((x, y), 0.2, sources=np.zeros(800, dtype=bool))
    assert none.total == 0


def test_z_separates_points_close_in_xy(gpu):
    rng = np.random.default_rng(8)
    x, y = rng.random(600), rng.random(600)
    z = rng.integers(0, 3, 600) * 0.5  # three layers further apart than the radius
    nb3, _ = check_all((x, y, z), 0.1, z=True)
    nb2, _ = check_all((x, y, z), 0.1)  # z ignored
    assert 0 < nb3.total < nb2.total and np.all(nb3.dz == 0.0)
    zc = rng.random(600) * 0.1
    nbc, _ = check_all((x, y, zc), 0.1, z=True, include_coincident=False)
    assert np.any(nbc.dz != 0.0)


def test_float32_columns_are_widened(gpu):
    rng = np.random.default_rng(9)
    x32, y32, z32 = (rng.random(700).astype(np.float32) for _ in range(3))
    wide = (x32.astype(np.float64), y32.astype(np.float64), z32.astype(np.float64))
    nb32, _ = check_all((x32, y32, z32), 0.07, expect=brute(*wide, 0.07), z=True)
    nb64 = pa.neighbors(wide, 0.07, z=True)
    assert np.array_equal(nb32.j, nb64.j) and same_bits(nb32.dist, nb64.dist) and same_bits(nb32.dz, nb64.dz)


# ---- 8. max_pairs --------------------------------------------------------------------------------------------------------------
def test_max_pairs(gpu):
    x, y = all_pairs_points()
    with pytest.raises(ValueError, match="max_pairs") as ei:
        pa.neighbors((x, y), 10.0, max_pairs=1000)
    assert str(300 * 299) in str(ei.value) and "1000" in str(ei.value)
    check_all((x, y), 0.1)  # the context is still good
    assert pa.neighbors((x, y), 10.0, max_pairs=300 * 299).total == 300 * 299  # the cap itself is allowed


# ---- 9. buffer reuse -----------------------------------------------------------------------------------------------------------
def test_buffer_reuse(gpu):
    rng = np.random.default_rng(10)
    for n, radius in ((2000, 0.05), (10, 0.5), (3000, 0.03)):
        x, y = rng.random(n), rng.random(n)
        check_all((x, y), radius)
    a = pa.neighbors((x, y), 0.03)
    b = pa.neighbors((x, y), 0.03)
    for name in ("count", "starts", "i", "j", "dx", "dy", "dist"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    interaction.release()  # and after the scratch was freed
    check_all((x[:100], y[:100]), 0.2)


def test_particle_views_and_sets_are_accepted(gpu):
    from parcels_amd.hostkernels import HostParticles

    rng = np.random.default_rng(11)
    data = {"x": rng.random(50).astype(np.float32), "y": rng.random(50).astype(np.float32), "z": np.zeros(50, np.float32),
            "particle_id": np.arange(50)}
    rows = np.arange(0, 50, 2)
    view = HostParticles(data, rows, by_mask=True)
    ref = brute(data["x"][rows], data["y"][rows], None, 0.3)
    check_all(view, 0.3, expect=ref)  # indices are local to the view


# ---- 10. end to end ------------------------------------------------------------------------------------------------------------
R_ATTRACT, R_MERGE, SPEED = 0.12, 0.03, 0.004


def attract_with_neighbors(particles, fieldset):
    """every particle moves with unit speed towards each attractor within R_ATTRACT"""
    nb = pa.neighbors(particles, R_ATTRACT, sources=np.asarray(particles.attractor, dtype=bool), include_coincident=False)
    particles.dx += SPEED * nb.sum(nb.dx / nb.dist)
    particles.dy += SPEED * nb.sum(nb.dy / nb.dist)


def attract_dense(particles, fieldset):
    x, y = np.asarray(particles.x, dtype=np.float64), np.asarray(particles.y, dtype=np.float64)
    n = len(x)
    dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]
    dist = np.sqrt(dx * dx + dy * dy)
    pull = (dist < R_ATTRACT) & (dist > 0) & np.asarray(particles.attractor, dtype=bool)[None, :]
    np.fill_diagonal(pull, False)
    i, j = np.nonzero(pull)
    particles.dx += SPEED * np.bincount(i, weights=dx[i, j] / dist[i, j], minlength=n)
    particles.dy += SPEED * np.bincount(i, weights=dy[i, j] / dist[i, j], minlength=n)


def _merge(particles, j):
    """mutual nearest neighbours merge: the lower index takes the mass, the higher is deleted"""
    idx = np.arange(len(j))
    mutual = (j >= 0) & (j[np.where(j >= 0, j, 0)] == idx)
    keep, gone = mutual & (idx < j), mutual & (idx > j)
    mass = np.asarray(particles.mass).copy()
    mass[keep] += mass[j[keep]]
    particles.mass = mass
    particles.state = np.where(gone, int(pa.StatusCode.Delete), np.asarray(particles.state))


def merge_with_neighbors(particles, fieldset):
    j, _ = pa.nearest_neighbor(particles, R_MERGE)
    _merge(particles, j)


def merge_dense(particles, fieldset):
    x, y = np.asarray(particles.x, dtype=np.float64), np.asarray(particles.y, dtype=np.float64)
    dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]
    dist = np.sqrt(dx * dx + dy * dy)
    np.fill_diagonal(dist, np.inf)
    dist[~(dist < R_MERGE)] = np.inf
    j = np.argmin(dist, axis=1)
    j[np.isinf(dist[np.arange(len(j)), j])] = -1
    _merge(particles, j)


def test_interaction_kernels_end_to_end(gpu):
    from case_utils import build_fieldset, load_golden

    case, _, _ = load_golden("agrid_flat_rk4_f64")
    fs = build_fieldset(case)
    lon, lat = np.asarray(case["lon"], dtype=np.float64), np.asarray(case["lat"], dtype=np.float64)
    rng = np.random.default_rng(12)
    # unit square of the kernels' radii, placed inside the grid (no kernel of the list samples a field)
    x0 = lon.min() + rng.random(400)
    y0 = lat.min() + rng.random(400)
    attractor = np.zeros(400, dtype=bool)
    attractor[rng.choice(400, 12, replace=False)] = True
    P = pa.get_default_particle(np.float64).add_variable([pa.Variable("attractor", dtype=np.bool_, initial=False),
                                                          pa.Variable("mass", dtype=np.float64, initial=1.0)])
    results = []
    for kernels in ([attract_with_neighbors, merge_with_neighbors], [attract_dense, merge_dense]):
        pset = pa.ParticleSet(fs, pclass=P, x=x0.copy(), y=y0.copy(), t=np.zeros(400))
        pset._data["attractor"][:] = attractor
        pset.execute(kernels, dt=1.0, runtime=10.0)
        results.append({k: np.array(pset._data[k]) for k in pset._data})
    a, b = results
    assert 50 < len(a["particle_id"]) < 400  # particles merged, the views shrank between steps
    assert a["mass"].sum() == 400.0 and a["mass"].max() >= 2.0
    assert np.abs(a["x"] - x0[a["particle_id"]]).max() > 5 * SPEED  # and were attracted
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k], equal_nan=True), k
