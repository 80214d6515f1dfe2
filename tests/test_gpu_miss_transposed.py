"""The transposed block fetch of the level-pair cache (csrc/pk_fast_agrid.h: lp_fetch_xposed, option "miss_lanes").

When at most `miss_lanes` lanes of a complete wavefront miss their block, sixteen helper lanes per missing lane fetch its corner rows in one
round trip and form lp_field's values with three cross-lane exchanges (tests/test_lp_transposed_model.py pins the lane map); every other
wave-evaluation with a missing lane takes the waterfall.  Both give the same bits, so every case here runs under four settings -- `block_cache`
0 (the block formed in registers in every evaluation), `block_cache` 2 with `miss_lanes` 0 (waterfall only), 64 (always transposed when the
wavefront is complete) and -1 (the planned default) -- and all columns, `ei`, states and launch counters must be equal at rtol 0.

The field set is 12 x 10 x 4 x 3 (lon, lat, depth, time) with an independent random value at every node (a block of another cell, level, depth
row or field is another set of numbers), U > 0.  The launches are not cell-sorted, so row i is lane i % 64 of wavefront i // 64.  Most lanes sit
where they stay in their cell for the whole launch; chosen lanes ("movers") start a quarter of a step's displacement short of a cell edge and
cross it in stage 2 of a chosen step.  Which path a wave-evaluation takes is recounted on the CPU (a NumPy RK4 that records every lane's cell and
level pair in every evaluation) and asserted per case: the kernel is not asked."""

from __future__ import annotations

import warnings

import numpy as np
import pytest

from case_utils import build_fieldset, build_pset, compare, endtime_of

DEFAULT_MISS_LANES = 4  # FAST_MISS_LANES_DEFAULT of pk_fast_agrid.h (what "miss_lanes" -1 plans)
DEG2M = 1852.0 * 60.0
DIMS = ("time", "depth", "YG", "XG")


# ---- cases -----------------------------------------------------------------------------------------------------------------------------

def _case(name, mesh, fdt, n, *, seed=0, nz=4, nt=3, dt=3600.0, level_dt=86400.0, steps=4, t0=900.0, kernels=("AdvectionRK4",), diverge=False):
    rng = np.random.default_rng(seed)
    nx, ny = 12, 10
    if mesh == "spherical":
        lon, lat, vel = np.linspace(0.0, 360.0, nx), np.linspace(-80.0, 80.0, ny), 1.0
    else:
        lon, lat, vel = np.linspace(0.0, 4.0e5, nx), np.linspace(0.0, 2.0e5, ny), 0.4
    depth = np.linspace(0.0, 5000.0, nz) if nz > 1 else np.zeros(1)
    shp = (nt, nz, ny, nx)
    U = vel * rng.uniform(0.7, 1.3, shp)
    V = vel * rng.uniform(-0.3, 0.3, shp)
    if diverge:  # outward on every side (the exit case)
        U = U * np.where(np.arange(nx) >= nx // 2, 1.0, -1.0)[None, None, None, :]
        V = vel * rng.uniform(0.1, 0.3, shp) * np.where(np.arange(ny) >= ny // 2, 1.0, -1.0)[None, None, :, None]
    sgn = 1.0 if dt > 0 else -1.0
    # stayers: the lower-left part of an interior cell (the upper-right part for backward time): U > 0 carries them less than 0.25 of a cell
    xi, yi = rng.integers(1, nx - 2, n), rng.integers(1, ny - 2, n)
    fx = rng.uniform(0.15, 0.45, n) if sgn > 0 else rng.uniform(0.55, 0.85, n)
    fy = rng.uniform(0.35, 0.65, n)
    case = dict(name=name, mesh=mesh, lon=lon, lat=lat, depth=depth, x_pad="low", y_pad="low", z_pad="both", time_s=np.arange(nt) * level_dt,
                fields={"U": U.astype(fdt), "V": V.astype(fdt)}, field_dims={"U": DIMS, "V": DIMS}, cgrid=False, kernels=list(kernels),
                spatial_dtype="float64", x=lon[xi] + fx * (lon[xi + 1] - lon[xi]), y=lat[yi] + fy * (lat[yi + 1] - lat[yi]),
                z=rng.uniform(200.0, 4800.0, n) if nz > 1 else np.zeros(n), t0=np.full(n, float(t0)), dt=dt, runtime=steps * abs(dt), seed=seed)
    case["_steps"] = np.full(n, steps)
    return case


def _fields64(case):
    return np.asarray(case["fields"]["U"], dtype=np.float64), np.asarray(case["fields"]["V"], dtype=np.float64)


def _cell(a, v):
    i = np.clip(np.searchsorted(a, v, side="left") - 1, 0, len(a) - 2)
    return i, (v - a[i]) / (a[i + 1] - a[i])


def _sample(case, t, z, y, x):
    """U, V in coordinate units per second at the points, the key (cell, level pair, lenT) of the block the evaluation needs, out of bounds"""
    lon, lat, depth, ts = case["lon"], case["lat"], case["depth"], case["time_s"]
    U, V = _fields64(case)
    n = len(x)
    with np.errstate(invalid="ignore"):
        oob = ~((x >= lon[0]) & (x <= lon[-1]) & (y >= lat[0]) & (y <= lat[-1]))
    xs, ys = np.where(oob, lon[1], x), np.where(oob, lat[1], y)
    ti, tau = _cell(ts, t) if len(ts) > 1 else (np.zeros(n, dtype=np.int64), np.zeros(n))
    zi, zeta = _cell(depth, z) if len(depth) > 1 else (np.zeros(n, dtype=np.int64), np.zeros(n))
    yi, eta = _cell(lat, ys)
    xi, xsi = _cell(lon, xs)
    t1 = np.minimum(ti + 1, len(ts) - 1)
    z1 = np.minimum(zi + 1, len(depth) - 1)

    def interp(F):
        def plane(tt, zz):
            return ((1 - xsi) * (1 - eta) * F[tt, zz, yi, xi] + xsi * (1 - eta) * F[tt, zz, yi, xi + 1] + (1 - xsi) * eta * F[tt, zz, yi + 1, xi]
                    + xsi * eta * F[tt, zz, yi + 1, xi + 1])

        def lvl(tt):
            return np.where(zeta > 0, plane(tt, zi) * (1 - zeta) + plane(tt, z1) * zeta, plane(tt, zi))
        return np.where(tau > 0, lvl(ti) * (1 - tau) + lvl(t1) * tau, lvl(ti))

    u, v = interp(U), interp(V)
    if case["mesh"] == "spherical":
        u, v = u / (DEG2M * np.cos(np.deg2rad(ys))), v / DEG2M
    cellid = (zi * len(lat) + yi) * len(lon) + xi
    key = (ti * 2 + (tau > 0)) * (len(depth) * len(lat) * len(lon)) + cellid
    return u, v, key, oob, ti


def _advance(case, rows, x, y, steps):
    """Positions of `rows` after `steps` whole RK4 steps from (x, y)"""
    dt = float(case["dt"])
    t, z = case["t0"][rows].copy(), case["z"][rows]
    for _ in range(steps):
        su = sv = 0.0
        px, py = x, y
        for ct, cw, nct in ((0.0, 1.0, 0.5), (0.5, 2.0, 0.5), (0.5, 2.0, 1.0), (1.0, 1.0, 0.0)):
            u, v, _, _, _ = _sample(case, t + ct * dt, z, py, px)
            su, sv = su + cw * u, sv + cw * v
            px, py = x + u * nct * dt, y + v * nct * dt
        x, y, t = x + su / 6.0 * dt, y + sv / 6.0 * dt, t + dt
    return x, y, t


def _movers(case, rows, step, *, axis="x"):
    """Move `rows` along `axis` so that step `step` (0-based) starts a quarter of a step's displacement short of the edge their flow carries them
    to: they cross it in stage 2 of that step and stay across for the rest of the launch"""
    rows = np.asarray(rows)
    lon, lat, dt = case["lon"], case["lat"], float(case["dt"])
    x, y = case["x"], case["y"]
    xi, _ = _cell(lon, x[rows])
    yi, _ = _cell(lat, y[rows])
    for _ in range(4):  # (the start point that arrives there: a fixed point in two or three rounds)
        px, py, pt = _advance(case, rows, x[rows], y[rows], step)
        u, v, _, _, _ = _sample(case, pt, case["z"][rows], py, px)
        if axis == "x":
            x[rows] += np.where(u * dt > 0, lon[xi + 1], lon[xi]) - 0.25 * u * dt - px
        else:
            y[rows] += np.where(v * dt > 0, lat[yi + 1], lat[yi]) - 0.25 * v * dt - py


def _recount(case):
    """Per evaluation e (4 per step) and row: `miss` -- the lane needs another block than in its previous evaluation (always in its first one);
    `active` -- the lane takes part in the miss branch of that evaluation (still stepping, inside the grid); `ti` -- its time level"""
    n = len(case["x"])
    dt = float(case["dt"])
    nst = case["_steps"]
    E = 4 * int(nst.max())
    x, y, z, t = case["x"].copy(), case["y"].copy(), case["z"], case["t0"].copy()
    alive = np.ones(n, dtype=bool)
    last = np.full(n, -1, dtype=np.int64)
    miss, active, tis = np.zeros((E, n), dtype=bool), np.zeros((E, n), dtype=bool), np.zeros((E, n), dtype=np.int64)
    for s in range(E // 4):
        alive &= s < nst
        su = sv = 0.0
        px, py = x, y
        for st, (ct, cw) in enumerate(((0.0, 1.0), (0.5, 2.0), (0.5, 2.0), (1.0, 1.0))):
            with np.errstate(invalid="ignore"):
                u, v, key, oob, ti = _sample(case, t + ct * dt, z, py, px)
            e = 4 * s + st
            active[e] = alive & ~oob
            miss[e] = active[e] & (key != last)
            tis[e] = ti
            last = np.where(active[e], key, last)
            alive &= ~oob & ~(np.isnan(u) | np.isnan(v))  # (a NaN corner: the evaluation runs, the step loop ends behind it)
            su, sv = su + cw * u, sv + cw * v
            nct = (0.5, 0.5, 1.0, 0.0)[st]
            px, py = x + u * nct * dt, y + v * nct * dt
        x, y, t = x + su / 6.0 * dt, y + sv / 6.0 * dt, t + dt
    return miss, active, tis


def _wave_evals(case):
    """[(evaluation, wavefront, missing lanes, complete wavefront, time levels of the missing lanes)] of every wave-evaluation with a missing lane"""
    miss, active, tis = _recount(case)
    n = miss.shape[1]
    out = []
    for e in range(miss.shape[0]):
        for w in range((n + 63) // 64):
            lanes = np.flatnonzero(miss[e, 64 * w:64 * w + 64])
            if len(lanes):
                full = 64 * w + 64 <= n and bool(active[e, 64 * w:64 * w + 64].all())
                out.append((e, w, lanes, full, set(tis[e, 64 * w + lanes].tolist())))
    return out


def _transposed(wes, thr, *, ring=False):
    return [we for we in wes if we[3] and len(we[2]) <= thr and not ring]


# ---- runs ------------------------------------------------------------------------------------------------------------------------------

def _fieldset_keeping_nan(case):
    """build_fieldset for these cases without the NaN -> 0 of the field data validation"""
    import parcels_amd as pa

    md = pa.SGrid2DMetadata(node_dimensions=("XG", "YG"), node_coordinates=("lon", "lat"),
                            face_dimensions=(pa.FaceNodePadding("XC", "XG", pa.Padding.LOW), pa.FaceNodePadding("YC", "YG", pa.Padding.LOW)),
                            vertical_dimensions=(pa.FaceNodePadding("ZC", "depth", pa.Padding.BOTH),))
    coords = {"lon": (("XG",), case["lon"]), "lat": (("YG",), case["lat"]), "depth": (("depth",), case["depth"]), "time": (("time",), case["time_s"])}
    ds = pa.Dataset({k: (DIMS, v) for k, v in case["fields"].items()}, coords, sgrid=md)
    return pa.FieldSet.from_sgrid_conventions(ds, mesh=case["mesh"], skip_field_data_validation=True)


def _run(case, block_cache, miss_lanes, nslots=None):
    import parcels_amd as pa

    fs = _fieldset_keeping_nan(case) if case.get("keep_nan") else build_fieldset(case)
    fs.to_device(nslots=nslots)
    fs._engine.ctx.set_option("fast_path", 1)
    fs._engine.ctx.set_option("block_cache", block_cache)
    fs._engine.ctx.set_option("miss_lanes", miss_lanes)
    pset = build_pset(case, fs, sort_by_cell=False)
    kernels = [getattr(pa.kernels, k) for k in case["kernels"]]
    kw = {"endtime": endtime_of(case["endtime"])} if case.get("endtime") is not None else {"runtime": float(case["runtime"])}
    err = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            pset.execute(kernels, dt=float(case["dt"]), **kw)
        except (pa.FieldOutOfBoundError, pa.FieldOutOfBoundSurfaceError, pa.FieldInterpolationError, pa.OutsideTimeInterval, pa.GeneralError) as e:
            err = type(e).__name__
    return {k: np.array(v) for k, v in pset._data.items()}, err, pset._last_stats


def _check(case, *, nslots=None, expect_error=None):
    ref, eref, sref = _run(case, 0, 0, nslots)
    assert eref == expect_error
    for ml in (0, 64, -1):
        got, egot, sgot = _run(case, 2, ml, nslots)
        assert egot == eref
        for k in ("steps", "attempts", "launches"):
            assert sgot[k] == sref[k], (case["name"], ml, k, sgot[k], sref[k])
        compare(got, ref, rtol=0.0, check_state="all", label=f"{case['name']}: block_cache 2, miss_lanes {ml} vs block_cache 0", skip=())
    return ref, sref


def _rows_of(lanes):
    return {int(l) >> 4 for l in lanes}


MESHES = [("spherical", np.float64), ("spherical", np.float32), ("flat", np.float64), ("flat", np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,fdt", MESHES)
def test_missing_lane_counts_rows_and_passes(gpu, mesh, fdt):
    """193 rows: three complete wavefronts and one lane.  One missing lane; three and five in one 16-lane row; four (the threshold) and five (one
    above) in different rows; nine and sixteen (three and four passes at miss_lanes 64); a partial wavefront (waterfall)."""
    case = _case("xp_counts_" + mesh, mesh, fdt, 193, seed=1)
    w0, w1, w2 = 0, 64, 128
    _movers(case, [w0 + 37], 0)
    _movers(case, [w0 + 16, w0 + 17, w0 + 18], 1)
    _movers(case, [w0 + 32, w0 + 33, w0 + 34, w0 + 35, w0 + 36], 2)
    _movers(case, [w0 + 1, w0 + 20, w0 + 40, w0 + 60], 3)
    _movers(case, [w1 + 2, w1 + 50], 0)
    _movers(case, [w1 + 3, w1 + 19, w1 + 35, w1 + 51, w1 + 52], 1)
    _movers(case, [w1 + 4, w1 + 5, w1 + 6, w1 + 7], 2, axis="y")
    _movers(case, w1 + np.array([8, 9, 10, 24, 25, 40, 41, 56, 63]), 3)
    _movers(case, w2 + np.arange(0, 64, 4), 0)
    _movers(case, [w2 + 30, w2 + 33], 2)
    _movers(case, [192], 1)
    wes = _wave_evals(case)
    full = {(e, w): lanes for e, w, lanes, f, _ in wes if f}
    assert [l.tolist() for (e, w), l in full.items() if (e, w) == (1, 0)] == [[37]]
    assert full[(5, 0)].tolist() == [16, 17, 18] and full[(9, 0)].tolist() == [32, 33, 34, 35, 36] and len(_rows_of(full[(13, 0)])) == 4
    assert len(full[(1, 1)]) == 2 and len(full[(5, 1)]) == 5 and len(_rows_of(full[(5, 1)])) == 4
    assert full[(9, 1)].tolist() == [4, 5, 6, 7] and len(full[(13, 1)]) == 9 and len(full[(1, 2)]) == 16 and full[(9, 2)].tolist() == [30, 33]
    counts = sorted(len(l) for (e, w), l in full.items() if e > 0)
    assert counts == [1, 2, 2, 3, 4, 4, 5, 5, 9, 16], counts
    assert DEFAULT_MISS_LANES in counts and DEFAULT_MISS_LANES + 1 in counts
    assert len(_transposed(wes, DEFAULT_MISS_LANES)) == 6 and len(_transposed(wes, 64)) == 10 + 3  # (+ the three first evaluations: 64 lanes, 16 passes)
    assert any(not f and w == 3 and e == 5 for e, w, _, f, _ in wes)
    ref, stats = _check(case)
    assert stats["steps"] == 4 * 193 and len(ref["x"]) == 193


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65])
def test_short_and_complete_wavefronts(gpu, n):
    """63 rows: no complete wavefront, every miss takes the waterfall; 64: one; 65: a complete one beside a single lane"""
    case = _case("xp_n%d" % n, "spherical", np.float64, n, seed=2)
    _movers(case, [5, 40], 0)
    _movers(case, [n - 1], 1)
    wes = _wave_evals(case)
    assert len(_transposed(wes, DEFAULT_MISS_LANES)) == (0 if n == 63 else 2 if n == 64 else 1)
    assert len([we for we in wes if not we[3]]) == (3 if n == 63 else 0 if n == 64 else 2)
    _check(case)


@pytest.mark.gpu
def test_lane_deleted_mid_launch(gpu):
    """A lane of the second wavefront leaves the grid in stage 2 of step 0 and is deleted: from then on that wavefront is incomplete and its missing
    lanes take the waterfall, while the first wavefront's take the transposed fetch"""
    case = _case("xp_deleted", "flat", np.float64, 128, seed=3, kernels=("AdvectionRK4", "DeleteParticle"))
    case["x"][64 + 9] = case["lon"][-1] - 1.0  # (one metre inside; U > 0.28 m/s carries it 500 m in half a step)
    _movers(case, [7, 64 + 20], 0)
    _movers(case, [30, 31, 64 + 40], 2)
    wes = _wave_evals(case)
    assert [(e, w) for e, w, *_ in _transposed(wes, DEFAULT_MISS_LANES)] == [(1, 0), (9, 0)]
    assert [(e, w, len(l)) for e, w, l, f, _ in wes if not f] == [(1, 1, 1), (9, 1, 1)]
    ref, _ = _check(case)
    assert len(ref["x"]) == 127 and 64 + 9 not in ref["particle_id"]


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,fdt", [("spherical", np.float32), ("flat", np.float64)])
def test_one_wavefront_on_two_level_pairs(gpu, mesh, fdt):
    """Release times two hours apart on a two-hourly time axis: even lanes sit on level pair 0, odd lanes on pair 1, and one pass serves missing lanes
    of both.  The early lanes step across level 1 in step 3 (32 missing lanes: waterfall by default); the late ones finish first (incomplete wavefront)."""
    case = _case("xp_stagger_" + mesh, mesh, fdt, 128, seed=4, dt=900.0, level_dt=7200.0)
    late = np.arange(128) % 2 == 1
    case["t0"] = np.where(late, 7200.0 + 900.0, 4500.0)
    case["endtime"] = 8100.0 + 4 * 900.0
    case["_steps"] = np.where(late, 4, 8)
    _movers(case, [6, 9, 64 + 33], 0)
    _movers(case, [64 + 2, 64 + 3, 64 + 17, 64 + 20], 1)
    _movers(case, [20, 22], 6)  # (early lanes only: behind the late lanes' last step)
    wes = _wave_evals(case)
    both = [we for we in _transposed(wes, DEFAULT_MISS_LANES) if len(we[4]) == 2]
    assert [(e, w, l.tolist()) for e, w, l, _, _ in both] == [(1, 0, [6, 9]), (5, 1, [2, 3, 17, 20])]
    assert [(e, len(l)) for e, w, l, f, _ in wes if f and w == 0 and e > 5] == [(13, 32)] and any(not f and l.tolist() == [20, 22] for _, _, l, f, _ in wes)
    _, stats = _check(case)
    assert stats["steps"] == 64 * 4 + 64 * 8


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_steps_onto_time_levels(gpu, sign):
    """t exactly on a level at the start and after every second step, forwards and backwards: lenT and the level pair switch for all 64 lanes at once
    (waterfall by default, sixteen passes at miss_lanes 64), with movers crossing a cell edge in between"""
    case = _case("xp_levels_%+d" % sign, "spherical", np.float64, 64, seed=5, dt=sign * 3600.0, level_dt=7200.0, t0=0.0 if sign > 0 else 14400.0)
    _movers(case, [11], 0)
    _movers(case, [12, 44], 1)
    _movers(case, [3, 19, 35], 3)
    wes = _wave_evals(case)
    assert sorted(len(l) for _, _, l, f, _ in _transposed(wes, DEFAULT_MISS_LANES)) == ([2, 3] if sign > 0 else [1, 2, 3])  # (forwards the first mover crosses where lenT switches on)
    assert sum(1 for _, _, l, f, _ in wes if f and len(l) >= 63) >= 3  # the first evaluation and every switch of lenT or of the level pair
    _check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,fdt", [("spherical", np.float64), ("flat", np.float32)])
def test_depth_nodes_and_surface(gpu, mesh, fdt):
    """z at the surface (zeta = 0: the lower depth row is not read, its helpers are masked out), on a depth node (zeta = 1) and between nodes, side by
    side in one pass"""
    case = _case("xp_depth_" + mesh, mesh, fdt, 64, seed=6)
    case["z"][[8, 24, 25]] = 0.0
    case["z"][[9, 40]] = case["depth"][2]
    case["z"][41] = case["depth"][-1]
    _movers(case, [8, 9, 10, 41], 0)
    _movers(case, [24, 40], 1)
    _movers(case, [25], 2, axis="y")
    wes = _wave_evals(case)
    assert [(e, l.tolist()) for e, _, l, _, _ in _transposed(wes, DEFAULT_MISS_LANES)] == [(1, [8, 9, 10, 41]), (5, [24, 40]), (9, [25])]
    _check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("nt,nz", [(1, 4), (3, 1), (1, 1)])
def test_one_level_axes(gpu, nt, nz):
    """A single time level (level ti + 1 does not exist: its helpers are masked out) and a single depth level (no depth stride)"""
    case = _case("xp_axes_%d_%d" % (nt, nz), "flat", np.float64, 64, seed=7, nt=nt, nz=nz, t0=0.0 if nt == 1 else 900.0)
    _movers(case, [1, 17, 62], 0)
    _movers(case, [30], 2)
    wes = _wave_evals(case)
    assert [(e, l.tolist()) for e, _, l, _, _ in _transposed(wes, DEFAULT_MISS_LANES)] == [(1, [1, 17, 62]), (9, [30])]
    _check(case)


@pytest.mark.gpu
def test_ring_launch_takes_the_waterfall(gpu):
    """Two slots for three levels: the level bases wrap, the transposed fetch stands back at every threshold; the results are those of the resident run"""
    case = _case("xp_ring", "spherical", np.float64, 64, seed=8)
    _movers(case, [13, 14], 0)
    _movers(case, [50], 1)
    wes = _wave_evals(case)
    assert len(_transposed(wes, 64)) == 3 and _transposed(wes, 64, ring=True) == []
    resident, _ = _check(case)
    ring, _ = _check(case, nslots=2)
    compare(ring, resident, rtol=0.0, check_state="all", label="ring vs resident", skip=())


@pytest.mark.gpu
def test_nan_corner(gpu):
    """A mover crosses into a cell with a NaN corner of V: the transposed fetch hands the NaN on, the evaluation answers ErrorInterpolation"""
    case = _case("xp_nan", "flat", np.float64, 64, seed=9)
    case["x"][21], case["y"][21] = case["lon"][4] + 0.3 * (case["lon"][5] - case["lon"][4]), case["lat"][3] + 0.5 * (case["lat"][4] - case["lat"][3])
    xi, yi = _cell(case["lon"], case["x"])[0], _cell(case["lat"], case["y"])[0]
    near = (xi >= 4) & (xi <= 6) & (yi >= 3) & (yi <= 4)  # nobody else in, or on the way into, the four cells of the NaN node
    near[21] = False
    case["x"][near] += 3 * (case["lon"][1] - case["lon"][0])
    _movers(case, [21, 45], 0)
    case["keep_nan"] = True
    case["fields"]["V"][:, :, 4, 6] = np.nan  # a corner of cell (yi 3, xi 5), the cell lane 21 enters, and of no cell it was in
    wes = _wave_evals(case)
    assert [(e, l.tolist()) for e, _, l, _, _ in _transposed(wes, DEFAULT_MISS_LANES)][:1] == [(1, [21, 45])]
    ref, _ = _check(case, expect_error="FieldInterpolationError")
    assert ref["state"][21] != ref["state"][20]


@pytest.mark.gpu
def test_exit_through_each_side(gpu):
    """Outward flow, one lane a step short of each side of the grid among movers and stayers: four lanes leave, one side after the other.  East and north answer ErrorOutOfBounds and are deleted; west and south carry the reference's
    left-out-of-bounds code, which is no error for x and y: such a lane returns early from every evaluation from then on and stays in the set"""
    case = _case("xp_exits", "flat", np.float64, 128, seed=10, kernels=("AdvectionRK4", "DeleteParticle"), diverge=True, steps=6)
    lon, lat = case["lon"], case["lat"]
    n = 128
    # stayers of an outward flow: the inner half of a cell of the outer ring but one
    xi = np.where(case["x"] > lon[6], np.random.default_rng(0).integers(6, 10, n), np.random.default_rng(1).integers(1, 5, n))
    fx = np.where(xi >= 6, 0.2, 0.8)
    case["x"] = lon[xi] + fx * (lon[xi + 1] - lon[xi])
    _movers(case, [3, 64 + 5], 0)
    _movers(case, [17, 18, 64 + 40], 1)
    east, west, north, south = 64 + 10, 64 + 11, 64 + 12, 64 + 13
    case["x"][east], case["x"][west] = lon[-1] - 1.0, lon[0] + 1.0
    for step, r in enumerate((east, west)):
        _movers(case, [r], step)
    case["y"][north], case["y"][south] = lat[-1] - 1.0, lat[0] + 1.0
    case["x"][[north, south]] = lon[7] + 0.2 * (lon[8] - lon[7])
    for step, r in enumerate((north, south)):
        _movers(case, [r], step + 2, axis="y")
    miss, active, _ = _recount(case)
    gone = [int(np.flatnonzero(~active[:, r])[0]) for r in (east, west, north, south)]
    assert gone == [1, 5, 9, 13], gone
    wes = _wave_evals(case)
    assert [(e, w) for e, w, *_ in _transposed(wes, DEFAULT_MISS_LANES)] == [(1, 0), (5, 0)] and any(not f and w == 1 for _, w, _, f, _ in wes)
    ref, _ = _check(case)
    left = set(ref["particle_id"].tolist())
    assert len(left) == 126 and not left & {east, north} and {west, south} <= left
