"""TEST INFRASTRUCTURE ONLY -- seeded random configurations of the unstructured-mesh path: draw_case(seed) for a ParticleSet.execute,
draw_points(seed) for Field.eval / UxGrid.search at explicit points.  The case dicts have the layout of tools/make_ux_golden.py, so the
same dict runs through the reference (make_ux_golden.run_case), the NumPy oracle (oracle/ux_oracle.py) and the device (tests/ux_utils.py).

Every concern draws from a generator of its own (np.random.default_rng((concern, seed))), so a later addition to one concern does not
change what the other concerns draw for a seed.

Bounds the `slim` margins of the oracle rest on: the lateral extent E = min(width, height) of a mesh is a tenth of
the coordinate scale or more, and every face has an altitude of E / 40 or more -- a position that is right to 1e-12 of the coordinate
scale then moves a barycentric coordinate by 4e-10 at the most.
"""

from __future__ import annotations

import numpy as np

from tools.make_ux_golden import face_centres, lattice_mesh

MESH, FIELDS, AXES, KERNELS, RUN, PARTICLES, POINTS, SMALL = range(8)  # the concerns
ADVECTION_2D = ["AdvectionEE", "AdvectionRK2", "AdvectionRK4"]
ADVECTION_3D = ["AdvectionRK2_3D", "AdvectionRK4_3D"]
STAGES = {"AdvectionEE": 1, "AdvectionRK2": 2, "AdvectionRK4": 4, "AdvectionRK2_3D": 2, "AdvectionRK4_3D": 4, "SampleField": 1}
SMALL_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257]  # both sides of a wavefront and of a 256-lane workgroup
KINDS = {"fc": ("zc", "n_face"), "ff": ("zf", "n_face"), "nc": ("zc", "n_node"), "nf": ("zf", "n_node")}
# Every search rounds x and y (and, where a 3-D kernel moves it, z) to float32, and a rounding is a close call (`slim`) with probability
# 2e-4: 240 searches of a 30-step RK4 run would mark 10 % of the particles.  On spherical meshes, the only ones where `slim` excludes a
# particle from a comparison, a run is cut to this many roundings per particle: an expected share of 0.8 %, under half the cap of 2 %.
MAX_SPHERICAL_ROUNDINGS = 40


def _rng(concern, seed):
    return np.random.default_rng((int(concern), int(seed)))


def min_altitude(lon, lat, faces):
    p = np.stack([lon[faces], lat[faces]], axis=-1)
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], axis=1)
    area2 = np.abs(e[:, 0, 0] * e[:, 1, 1] - e[:, 0, 1] * e[:, 1, 0])
    return float(np.min(area2 / np.max(np.hypot(e[..., 0], e[..., 1]), axis=1)))


def draw_mesh(seed, three_levels=False):
    """-> dict(mesh, node_lon, node_lat, faces, zf, zc, box=(lon0, lon1, lat0, lat1), region, hole=(lon lo, hi, lat lo, hi) or None)"""
    rng = _rng(MESH, seed)
    spherical = bool(rng.random() < 0.5)
    nx, ny = int(rng.integers(6, 41)), int(rng.integers(5, 31))
    jitter = float(rng.choice([0.0, 0.1, 0.2, 0.3]))
    graded = bool(rng.random() < 0.3)
    hole = bool(rng.random() < 0.3)
    region = "flat"
    if spherical:
        w, h = float(rng.uniform(20.0, 45.0)), float(rng.uniform(20.0, 45.0))
        region = str(rng.choice(["dateline", "dateline_west", "polar", "polar_south", "origin", "lon90", "midlat"]))
        u, v = float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.7))
        lat0 = float(rng.uniform(-60.0, 60.0 - h))
        lon0 = float(rng.uniform(-170.0, 170.0 - w))
        if region == "dateline":
            lon0 = 180.0 - u * w
        elif region == "dateline_west":
            lon0 = -180.0 - u * w
        elif region == "polar":
            lat0 = float(rng.uniform(85.0, 89.0)) - h
        elif region == "polar_south":
            lat0 = -float(rng.uniform(85.0, 89.0))
        elif region == "origin":  # x = cos(lon) cos(lat) peaks inside the mesh
            lon0, lat0 = -u * w, -v * h
        elif region == "lon90":  # y = sin(lon) cos(lat) peaks inside the mesh
            lon0, lat0 = 90.0 - u * w, -v * h
    else:
        e = float(rng.choice([1.0, 20.0, 1000.0]))
        w, h = e * float(rng.uniform(1.0, 2.0)), e * float(rng.uniform(1.0, 2.0))
        lon0, lat0 = float(rng.choice([0.0, -0.5, 3.0])) * w, float(rng.choice([0.0, -0.5, 3.0])) * h
    warp = float(rng.uniform(0.8, 1.6))
    mesh_seed = int(rng.integers(0, 2**31))
    ext = min(w, h)
    while True:
        lon, lat, faces = lattice_mesh(nx, ny, 0.0, 1.0, 0.0, 1.0, jitter=jitter, seed=mesh_seed)
        if graded:  # spacing grows geometrically along both axes: by e ** warp from one side to the other
            lon, lat = np.expm1(warp * lon) / np.expm1(warp), np.expm1(warp * lat) / np.expm1(warp)
        lon, lat = lon0 + w * lon, lat0 + h * lat
        if min_altitude(lon, lat, faces) >= ext / 40.0:
            break
        nx, ny = max(6, (nx * 4) // 5), max(5, (ny * 4) // 5)  # coarser, until every face is E / 40 high
        if nx == 6 and ny == 5:
            jitter, graded = min(jitter, 0.1), False
    hole_box = None
    if hole:  # a rectangular block of quads taken out of the interior
        i0, j0 = int(rng.integers(1, nx - 3)), int(rng.integers(1, ny - 3))
        i1, j1 = min(i0 + int(rng.integers(1, 4)), nx - 2), min(j0 + int(rng.integers(1, 4)), ny - 2)
        j, i = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
        gone = ((i >= i0) & (i < i1) & (j >= j0) & (j < j1)).ravel()
        keep = ~np.repeat(gone, 2)
        lost = faces[~keep]
        hole_box = (float(lon[lost].min()), float(lon[lost].max()), float(lat[lost].min()), float(lat[lost].max()))
        faces = faces[keep]
    rax = _rng(AXES, seed)
    nz = int(rax.integers(3 if three_levels else 2, 7))
    depth = float(rax.uniform(0.2, 1.0)) * ext * (2.0 if spherical else 1.0)
    zf = np.concatenate([[0.0], np.cumsum(rax.uniform(0.5, 2.0, nz - 1))])
    zf = (zf / zf[-1] * depth).astype(np.float32).astype(np.float64)  # float32 values: a start exactly on a level stays on it under the cast
    return dict(mesh="spherical" if spherical else "flat", node_lon=lon, node_lat=lat, faces=faces, zf=zf, zc=0.5 * (zf[:-1] + zf[1:]),
                box=(lon0, lon0 + w, lat0, lat0 + h), region=region, hole=hole_box)


def _pattern(rng, s, r):
    a = rng.uniform(-1.0, 1.0, 4)
    f = rng.uniform(0.5, 2.5, 2)
    return a[0] + 0.6 * a[1] * np.sin(2 * np.pi * (f[0] * s + a[2])) + 0.6 * a[3] * np.cos(2 * np.pi * f[1] * r) + 0.3 * (r - s)


def draw_field(rng, m, kind, nt, amp):
    """(array, dims) of one field of registration `kind` on the mesh: smooth in space, a factor per level and per time level"""
    vert, lateral = KINDS[kind]
    lon0, lon1, lat0, lat1 = m["box"]
    px, py = face_centres(m["node_lon"], m["node_lat"], m["faces"]) if lateral == "n_face" else (m["node_lon"], m["node_lat"])
    lateral_part = _pattern(rng, (px - lon0) / (lon1 - lon0), (py - lat0) / (lat1 - lat0))
    nlev = len(m["zf"]) if vert == "zf" else len(m["zc"])
    arr = amp * lateral_part[None, None, :] * rng.uniform(0.5, 1.5, nlev)[None, :, None] * rng.uniform(0.6, 1.4, nt)[:, None, None]
    if m["mesh"] == "spherical" and amp != 1.0:  # keep the zonal displacement in degrees moderate next to a pole
        arr = arr * np.cos(np.deg2rad(py))[None, None, :]
    return np.ascontiguousarray(arr), ("time", vert, lateral)


def draw_case(seed):
    seed = int(seed)
    m = draw_mesh(seed)
    spherical = m["mesh"] == "spherical"
    lon0, lon1, lat0, lat1 = m["box"]
    ext = min(lon1 - lon0, lat1 - lat0)
    zf = m["zf"]
    nz = len(zf)

    rk = _rng(KERNELS, seed)
    three_d = bool(rk.random() < 0.5) and nz > 2  # (one layer: a zc field has no level for the reference to wrap to above the surface)
    kernels = [str(rk.choice(ADVECTION_3D if three_d else ADVECTION_2D))]
    if rk.random() < 0.3:
        kernels.append(str(rk.choice(ADVECTION_2D + (ADVECTION_3D if three_d else []))))
    sample = None
    if rk.random() < 0.35:
        sample = str(rk.choice(sorted(KINDS)))
        kernels.insert(int(rk.integers(0, len(kernels) + 1)), "SampleField")
    constants = None
    if rk.random() < 0.25:
        constants = {"Kconst": 2.5}
        kernels.insert(int(rk.integers(0, len(kernels) + 1)), "SampleConst")
    if rk.random() < 0.4:
        kernels.append("DeleteParticle")
    if rk.random() < 0.15:
        kernels.insert(0, str(rk.choice(["MoveEast", "DoNothing", "MoveNorth"])))

    rr = _rng(RUN, seed)
    backward = bool(rr.random() < 0.25)
    dt = float(rr.choice([600.0, 1800.0, 3600.0] if spherical else [1.0, 5.0, 60.0]))
    nsteps = int(rr.integers(5, 31))
    if spherical:  # see MAX_SPHERICAL_ROUNDINGS
        per_step = sum(STAGES.get(k, 0) for k in kernels) * (3 if any(k in ADVECTION_3D for k in kernels) else 2)
        nsteps = max(1, min(nsteps, MAX_SPHERICAL_ROUNDINGS // per_step))
    stagger = bool(rr.random() < 0.3)
    outputdt = float(dt * rr.choice([2.0, 2.5, 3.7])) if rr.random() < 0.3 else None
    vel = float(rr.choice([0.003, 0.01, 0.03]))  # of the extent, per step
    short_axis = bool(rr.random() < 0.08)  # the run leaves the time axis: OutsideTimeInterval

    rax = _rng(AXES, 10_000_019 + seed)
    nt = int(rax.integers(1, 6))
    span = (nsteps + (4 if stagger else 0)) * dt
    total = float(np.ceil(span * (0.6 if short_axis else 1.25)))
    if nt == 1:  # no time axis: the fields hold for all time
        time_s = np.array([0.0])
    else:  # unequal levels on whole seconds
        cuts = np.round(np.sort(rax.uniform(0.05, 0.95, nt - 2)) * total)
        time_s = np.unique(np.concatenate([[0.0], cuts, [total]]))
    nt = len(time_s)
    nslots = 3 if (nt >= 4 and rax.random() < 0.5) else None
    if nslots is not None and np.min(np.diff(time_s)) < dt:
        nslots = None  # a step must fit into the resident levels: the engine refuses a ring of 3 where a step crosses two levels

    rf = _rng(FIELDS, seed)
    amp = vel * ext / dt * (1852 * 60.0 if spherical else 1.0)
    uv_kind = str(rf.choice(sorted(KINDS)))
    fields = {"U": draw_field(rf, m, uv_kind, nt, amp), "V": draw_field(rf, m, uv_kind, nt, amp)}
    if three_d or rf.random() < 0.2:
        wamp = vel * (zf[-1] - zf[0]) / dt
        arr, dims = draw_field(rf, m, str(rf.choice(["nf", "ff"])), nt, 1.0)
        fields["W"] = (arr * wamp, dims)
    if sample is not None:
        fields["P"] = draw_field(rf, m, sample, nt, 1.0)

    rp = _rng(PARTICLES, seed)
    n = int(rp.choice(SMALL_COUNTS)) if rp.random() < 0.25 else int(rp.integers(200, 1501))
    if spherical and n < 200:  # two slim particles of 65 are 3 %: the counts at a wavefront boundary go to flat meshes, which are compared
        n = int(_rng(SMALL, seed).choice([255, 256, 257]))  # without exclusions; spherical ones keep the workgroup boundary
    margin = float(rp.choice([0.15, 0.05, 0.01]))
    faces, lon, lat = m["faces"], m["node_lon"], m["node_lat"]
    fcx, fcy = face_centres(lon, lat, faces)
    inner = np.flatnonzero((fcx > lon0 + margin * (lon1 - lon0)) & (fcx < lon1 - margin * (lon1 - lon0)) &
                           (fcy > lat0 + margin * (lat1 - lat0)) & (fcy < lat1 - margin * (lat1 - lat0)))
    if n <= 2:
        inner = inner[inner != 0]  # a lone particle never starts in face 0: every ei would stay 0 (the guess rules part ways there)
    f = rp.choice(inner, n)
    b = rp.dirichlet(np.ones(3), n)
    share = 0.03 if spherical else 0.1
    pick = rp.random(n)
    on_node, on_edge = pick < share, (pick >= share) & (pick < 2 * share)
    b[on_node] = np.array([1.0, 0.0, 0.0])
    b[on_edge] = np.array([0.5, 0.5, 0.0])
    x = np.sum(lon[faces[f]] * b, axis=1)
    y = np.sum(lat[faces[f]] * b, axis=1)
    x[on_node], y[on_node] = lon[faces[f[on_node], 0]], lat[faces[f[on_node], 0]]
    zm = margin * (zf[-1] - zf[0])
    z = rp.uniform(zf[0] + zm, zf[-1] - zm, n)
    on_level = rp.random(n) < 0.1
    z[on_level] = zf[rp.integers(0 if not three_d else 1, nz - (0 if not three_d else 1), int(on_level.sum()))]
    offs = rp.integers(0, 5, n) * dt if stagger else np.zeros(n)
    t0 = (time_s[-1] if nt > 1 else total) - offs if backward else offs
    sdt = "float32" if (not spherical and _rng(SMALL, 7_000_003 + seed).random() < 0.25) else "float64"

    return dict(name=f"ux_fuzz_{seed}", mesh=m["mesh"], node_lon=lon, node_lat=lat, faces=faces.astype(np.int64), zf=zf, zc=m["zc"], time_s=time_s,
                fields=fields, x=x, y=y, z=z, t0=t0, dt=-dt if backward else dt, runtime=nsteps * dt, outputdt=outputdt, kernels=kernels,
                sample=("P" if sample is not None else None), constants=constants, spatial_dtype=sdt, nslots=nslots, region=m["region"],
                hole=m["hole"])


def draw_points(seed, n=400):
    """-> (case, points): a mesh with a scalar field of each of the four kinds and U, V, W, and points (t, z, y, x) for Field.eval /
    UxGrid.search: interior, exact nodes, edge midpoints, outside the mesh, in the hole, z on / above / below the levels, NaN and +-inf"""
    seed = int(seed)
    m = draw_mesh(500_000 + seed, three_levels=True)
    rf = _rng(FIELDS, 500_000 + seed)
    rax = _rng(AXES, 510_000_019 + seed)
    nt = int(rax.integers(1, 5))
    time_s = np.concatenate([[0.0], np.cumsum(np.round(rax.uniform(50.0, 500.0, nt - 1)))]) if nt > 1 else np.array([0.0])
    uv_kind = str(rf.choice(sorted(KINDS)))
    amp = 1852 * 60.0 if m["mesh"] == "spherical" else 2.0
    fields = {"U": draw_field(rf, m, uv_kind, nt, amp), "V": draw_field(rf, m, uv_kind, nt, amp), "W": draw_field(rf, m, str(rf.choice(["nf", "ff"])), nt, 1.0)}
    for kind in sorted(KINDS):
        fields["P_" + kind] = draw_field(rf, m, kind, nt, 1.0)
    rp = _rng(POINTS, seed)
    lon0, lon1, lat0, lat1 = m["box"]
    lon, lat, faces, zf = m["node_lon"], m["node_lat"], m["faces"], m["zf"]
    w, h = lon1 - lon0, lat1 - lat0
    f = rp.integers(0, len(faces), n)
    b = rp.dirichlet(np.ones(3), n)
    grp = rp.integers(0, 10, n)  # 0..4 interior, 5 node, 6 edge midpoint, 7 outside, 8 hole (or outside), 9 anywhere in the box
    b[grp == 5] = np.array([0.0, 1.0, 0.0])
    b[grp == 6] = np.array([0.5, 0.0, 0.5])
    x, y = np.sum(lon[faces[f]] * b, axis=1), np.sum(lat[faces[f]] * b, axis=1)
    x[grp == 5], y[grp == 5] = lon[faces[f[grp == 5], 1]], lat[faces[f[grp == 5], 1]]
    k = grp == 7
    x[k], y[k] = rp.uniform(lon0 - 0.2 * w, lon1 + 0.2 * w, k.sum()), rp.uniform(lat0 - 0.2 * h, lat1 + 0.2 * h, k.sum())
    k = grp == 8
    hb = m["hole"] or (lon0 - 0.1 * w, lon0, lat0, lat1)
    x[k], y[k] = rp.uniform(hb[0], hb[1], k.sum()), rp.uniform(hb[2], hb[3], k.sum())
    k = grp == 9
    x[k], y[k] = rp.uniform(lon0, lon1, k.sum()), rp.uniform(lat0, lat1, k.sum())
    z = rp.uniform(zf[0], zf[-1], n)
    zg = rp.integers(0, 8, n)  # 5 on a level, 6 above the surface, 7 below the bottom
    z[zg == 5] = zf[rp.integers(0, len(zf), int((zg == 5).sum()))]
    z[zg == 6] = zf[0] - rp.uniform(0.0, 1.0, int((zg == 6).sum())) * (zf[-1] - zf[0])
    z[zg == 7] = zf[-1] + rp.uniform(0.0, 1.0, int((zg == 7).sum())) * (zf[-1] - zf[0])
    bad = rp.choice(n, 18, replace=False)  # NaN, +inf, -inf in each of x, y, z (two points each)
    for j, (col, val) in enumerate((c, v) for c in (x, y, z) for v in (np.nan, np.inf, -np.inf)):
        col[bad[2 * j: 2 * j + 2]] = val
    t = rp.uniform(0.0, time_s[-1], n) if nt > 1 else rp.uniform(0.0, 1000.0, n)
    if nt > 1:
        on_t = rp.random(n) < 0.15
        t[on_t] = time_s[rp.integers(0, nt, int(on_t.sum()))]
    case = dict(name=f"ux_points_{seed}", mesh=m["mesh"], node_lon=lon, node_lat=lat, faces=faces.astype(np.int64), zf=zf, zc=m["zc"], time_s=time_s,
                fields=fields, constants=None, spatial_dtype="float64", kernels=[], sample=None, region=m["region"], hole=m["hole"])
    return case, dict(t=t, z=z, y=y, x=x)
