"""TEST INFRASTRUCTURE ONLY -- seeded CROCO sigma-grid configurations for tests/test_croco_oracle.py (the C oracle's CROCO kernels against the
live reference) and tests/test_gpu_croco_fuzz.py (the device's sigma program against the oracle), and the oracle's side of both.

`draw_case(seed)` returns a case in the terms of tools/make_croco_golden.py (coords + fields the way a CROCO user holds them, particles,
kernel names, the execute() call), so one dict feeds the reference (make_croco_golden.run_case), the oracle (`run_oracle`) and the device
(tests/croco_utils.py: run_croco).  `draw_points(seed)` returns such a case with `kind = "sigma_points"` and the points of one
`convert_z_to_sigma_croco(fieldset, t, z, y, x, None)` call.

Every seed draws: the grid (rectilinear | curvilinear, flat | spherical, float32 | float64 field data, C-grid | all fields on the nodes --
the eight instantiations of the device's launcher), the number of sigma levels, the stretching, hc below / inside / above the range of h,
the amplitude of zeta, the particles (counts on both sides of a wavefront and of a workgroup, storage dtype, common or scattered release
times, a share of starts outside the water column, next to a lateral edge, or exactly on a level / the floor / the surface), the kernel
list, dt of either sign, the number of steps, an output interval or a split into two execute() calls now and then, a ring of level slots
or cell-sorted particles now and then (the device's switches; the expected result is the same), and a few runs that leave zeta's time
interval.

Out of scope: diffusion kernels beside a CROCO kernel (their random numbers are drawn differently by the reference, the oracle and the device;
the structured fuzz covers them without a sigma axis).

The reference's two known batch properties (profiles/r04_fuzz_oracle_vs_reference.txt) are kept out of the draws: no batch has a single
particle left alone on a curvilinear grid without a twin (count 1 is drawn on rectilinear grids only, where no NumPy reduction depends on
the batch), and no curvilinear batch sits in grid column 0 (the particles start at 12 % of the width or further in)."""

from __future__ import annotations

import numpy as np

from oracle import c_oracle
from tools import make_croco_golden as mg

NW = (2, 3, 9, 33, 64, 65, 300)
COUNTS = (1, 2, 63, 64, 65, 200, 255, 256, 257, 600)
POINT_COUNTS = (1, 64, 255, 257, 1000)
ADV, OMEGA = "AdvectionRK2_3D_CROCO", "SampleOmegaCroco"
KERNEL_LISTS = (
    (ADV,),
    (ADV, OMEGA),
    (ADV, "DeleteParticle"),
    (ADV, "DeleteOutOfBounds"),
    (ADV, OMEGA, "DeleteParticle"),
    (ADV, OMEGA, "DeleteOutOfBounds"),
    ("AdvectionRK2", "SampleFieldCroco:omega:omega", "SampleFieldCroco:temp:tracer"),
    ("AdvectionEE", OMEGA),
    (ADV, "SampleFieldCroco:temp:tracer", OMEGA),
)
TSTEP = 3000.0  # seconds between the time levels of croco_output


def launch_key(case) -> int:
    """the device launcher's instantiation (csrc/pk_prog_sigma.hip: field_f32 * 4 + curvilinear * 2 + C-grid)"""
    f32 = int(np.asarray(case["fields"]["h"]).dtype == np.float32)
    return f32 * 4 + int(np.asarray(case["coords"]["x_rho"]).ndim == 2) * 2 + int(not case.get("agrid"))


def draw_grid(rng) -> dict:
    """the fieldset half of a case"""
    nw = int(rng.choice(NW))
    nx, ny = (5, 4) if nw == 300 else (int(rng.integers(5, 22)), int(rng.integers(4, 18)))
    curvilinear, spherical, agrid = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
    if nw == 2:  # (a C-grid's u, v have nw - 1 = 1 level: the reference's gather raises IndexError at the wrapped index -2 of a particle over the surface)
        agrid = True
    dtype = np.float32 if rng.integers(2) else np.float64
    hmin = float(rng.choice([12.0, 40.0, 90.0]))
    hc = float(rng.choice([0.5 * hmin, hmin + 50.0, hmin + 200.0]))  # below, inside, above [hmin, hmin + 120]
    nt = int(rng.integers(3, 5))
    theta_s = float(rng.choice([0.0, rng.uniform(0.5, 7.0)]))
    zeta_amp = float(rng.choice([0.02, 0.4, hmin / 4.0 / (1.0 + 0.25 * (nt - 1))]))
    coords, fields = mg.croco_output(nx=nx, ny=ny, nw=nw, nt=nt, spherical=spherical, curvilinear=curvilinear, dtype=dtype, hmin=hmin,
                                     tstep=TSTEP, theta_s=theta_s, zeta_amp=zeta_amp, agrid=agrid)
    return dict(coords=coords, fields=fields, hc=hc, mesh="spherical" if spherical else "flat", agrid=agrid, zeta_amp=zeta_amp, theta_s=theta_s)


def _nodes(coords):
    xr, yr = np.asarray(coords["x_rho"]), np.asarray(coords["y_rho"])
    return (xr, yr) if xr.ndim == 2 else tuple(np.meshgrid(xr, yr))


def _place(X, Y, h, zeta, jy, ix, centre):
    """(x, y, h, zeta) of node (jy, ix), where the samples of h and zeta at a time level are the data values and a level's depth can be
    met exactly.  centre: on a spherical curvilinear grid, where the search projects onto the unit sphere and no sample is exact, the
    centre of cell (jy, ix) with the means of its corners instead -- a node lies on the boundary of four cells there, and which of them
    (or none) the search settles on is decided within the rounding of a sine; the level is then met to rounding, not exactly"""
    if not centre:
        return X[jy, ix], Y[jy, ix], h[jy, ix], zeta[jy, ix]
    box = (slice(jy, jy + 2), slice(ix, ix + 2))
    return X[box].mean(), Y[box].mean(), h[box].mean(), zeta[box].mean()


def _zvec(fields, hc, s_w, h, zeta):
    """the depths of the sigma levels under one node in float64 (kernels/_sigmagrids.py:17-18)"""
    cs = np.asarray(fields["Cs_w"], dtype=np.float64)
    z0 = hc * s_w + (h - hc) * cs
    return z0 + zeta * (1.0 + (z0 / h))


def _found(coords, mesh, x, y):
    """which (x, y) the curvilinear search finds without a guess.  The reference's spatial hash misses a few per cent of the interior
    points of these small distorted lattices (GridSearchingError, in the reference, the oracle and on the device alike); a run whose
    particles start there ends in its first iteration, so the interior starts are drawn from the points it finds."""
    import ctypes as C

    from parcels_amd.spatialhash import SpatialHash

    lon, lat = np.asarray(coords["x_rho"]), np.asarray(coords["y_rho"])
    mc = c_oracle.MarshalledCase(dict(lon=lon, lat=lat, depth=None, mesh=mesh, fields={}, field_dims={}, time_s=None,
                                      hash_table=SpatialHash(lon, lat, mesh == "spherical").table()))
    n = len(x)
    xs, ys = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    yi, xi, a, b = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n), np.zeros(n)
    c_oracle.lib().po_hash_query(C.byref(mc.grids[0]), C.c_int64(n), c_oracle._ptr(ys), c_oracle._ptr(xs), c_oracle._ptr(yi), c_oracle._ptr(xi),
                                 c_oracle._ptr(a), c_oracle._ptr(b))
    return xi >= 0


def draw_case(seed: int) -> dict:
    rng = np.random.default_rng([seed, 0xC0C0])
    g = draw_grid(rng)
    coords, fields = g["coords"], g["fields"]
    curvilinear = np.asarray(coords["x_rho"]).ndim == 2
    X, Y = _nodes(coords)
    n = int(rng.choice(COUNTS))
    kernels = list(KERNEL_LISTS[int(rng.integers(len(KERNEL_LISTS)))])
    two_d = ADV not in kernels
    if two_d and g["zeta_amp"] > 0.02:  # the 2-D lists keep their particles within a metre of the surface: a flat one
        zeta = np.asarray(fields["zeta"])
        fields["zeta"] = (zeta * (0.02 / g["zeta_amp"])).astype(zeta.dtype)
    use = ["u", "v", "w", "h", "zeta", "Cs_w"] + (["omega"] if any("mega" in k for k in kernels) else []) + (["temp"] if any(":temp:" in k for k in kernels) else [])
    sign = -1.0 if rng.integers(2) else 1.0
    dt = sign * float(rng.choice([50.0, 100.0, 150.0]))
    nt = len(coords["time"])
    tlen = TSTEP * (nt - 1)
    steps = int(rng.integers(8, 41))
    steps = min(steps, int(tlen / abs(dt)) - 4)  # the whole run, scattered releases included, inside zeta's time interval ...
    leaves = rng.random() < 0.06                 # ... but for a few
    if leaves:
        steps = int(tlen / abs(dt)) + 3
    base = 0.0 if sign > 0 else tlen
    # where the particles start: on a C-grid below the last row and left of the last column of cells, where the reference's gather of V
    # (eta_v has one row less than eta_rho) raises IndexError; a batch of one or two on a curvilinear grid far from grid column 0, where
    # the reference drops every guess (np.any(xi), index_search.py:269)
    nyc, nxc = X.shape[0] - 1, X.shape[1] - 1
    xfrac, yfrac = [0.12, 0.70], [0.15, 0.85]
    if not g["agrid"]:
        xfrac[1], yfrac[1] = min(0.70, (nxc - 1) / nxc - 0.15), min(0.85, (nyc - 1) / nyc - 0.10)
    if curvilinear:
        xfrac[0] = max(xfrac[0], 1.0 / nxc + 0.03)
        if n <= 2:
            xfrac[0] = 0.45
    xfrac[1] = max(xfrac[1], xfrac[0] + 0.05)
    x, y, z = mg.interior_particles(coords, fields, n, seed=int(rng.integers(1 << 30)), xfrac=xfrac, yfrac=yfrac)
    if curvilinear:  # (the storage dtype decides what the search sees: test the float32 positions too)
        ok = _found(coords, g["mesh"], x, y) & _found(coords, g["mesh"], x.astype(np.float32), y.astype(np.float32))
        if ok.any() and not ok.all():
            src = rng.choice(np.flatnonzero(ok), int((~ok).sum()))
            x[~ok], y[~ok], z[~ok] = x[src], y[src], z[src]
    if two_d:
        z = rng.uniform(-0.95, -0.05, n)
    t0 = np.full(n, base)
    scattered = bool(rng.integers(2))
    if scattered:
        t0 = base + dt * rng.integers(0, 5, n)
        t0[0] = base
    # the edge starts: a drawn share of 0 to 10 %, of six kinds in turn
    share = 0.0 if rng.random() < 0.4 else float(rng.uniform(0.0, 0.10))
    ne = int(round(share * n))
    h64, s_w = np.asarray(fields["h"], dtype=np.float64), np.asarray(coords["s_w"], dtype=np.float64)
    zeta64 = np.asarray(fields["zeta"], dtype=np.float64)
    rows = rng.choice(n, ne, replace=False) if ne else np.zeros(0, int)
    kinds = []
    for j, r in enumerate(rows):
        kind = ("floor_under", "surface_above", "edge", "on_level", "on_floor", "on_surface")[(j + seed) % 6]
        kinds.append(kind)
        hcol = float(mg.water_column(coords, fields, x[r:r + 1], y[r:r + 1])[0])
        if kind == "floor_under":
            z[r] = -hcol - float(rng.uniform(0.5, 8.0))
        elif kind == "surface_above":
            z[r] = float(np.max(np.abs(zeta64))) + float(rng.uniform(0.6, 5.0))
        elif kind == "edge":  # within one step of the east edge (u > 0 everywhere: forward runs leave, backward runs come in)
            xr = np.asarray(coords["x_rho"])
            x[r] = xr.max() - (xr.max() - xr.min()) * float(rng.uniform(1e-4, 1e-3))
            if curvilinear:
                x[r] -= 0.013 * (xr.max() - xr.min())  # (inside the distorted east edge at every y)
        else:  # on a node at a time level, where the samples of h and zeta are the data values: z = zvec_k exactly (float64 storage)
            jy, ix = int(rng.integers(1, X.shape[0] - 2)), int(rng.integers(1, X.shape[1] - 2))
            xn, yn, hn, zn = _place(X, Y, h64, zeta64[0 if sign > 0 else nt - 1], jy, ix, curvilinear and g["mesh"] == "spherical")
            x[r], y[r], t0[r] = xn, yn, base
            zv = _zvec(fields, g["hc"], s_w, hn, zn)
            z[r] = {"on_level": zv[int(rng.integers(len(zv)))], "on_floor": -hn, "on_surface": zn}[kind]
    case = dict(coords=coords, fields={k: fields[k] for k in use}, x=x, y=y, z=z, kernels=kernels, mesh=g["mesh"], hc=g["hc"], agrid=g["agrid"],
                spatial_dtype="float32" if rng.integers(2) else "float64", dt=dt, runtime=steps * abs(dt), t0=t0,
                outputdt=None, split=None, kind=None, name=f"fuzz_{seed}", leaves=bool(leaves), edge_kinds=kinds, edge_rows=rows,
                theta_s=g["theta_s"], seed=seed)
    extra = rng.random()
    if extra < 0.15:
        case["outputdt"] = abs(dt) * int(rng.integers(2, 6))
    elif extra < 0.30 and steps > 12:
        case["split"] = abs(dt) * int(rng.integers(6, steps - 2))
    case["device"] = (None, None, None, "ring", "sorted")[int(rng.integers(5))]  # a ring of 3 level slots | cell-sorted particles
    return case


def draw_points(seed: int) -> dict:
    """one convert_z_to_sigma_croco(fieldset, t, z, y, x, None) call: interior points, points outside the domain, under the floor, above the
    surface, exactly on levels, z of NaN and +-inf"""
    rng = np.random.default_rng([seed, 0x9017])
    g = draw_grid(rng)
    coords, fields = g["coords"], g["fields"]
    n = int(rng.choice(POINT_COUNTS))
    xr, yr = np.asarray(coords["x_rho"]), np.asarray(coords["y_rho"])
    w, hgt = xr.max() - xr.min(), yr.max() - yr.min()
    x, y = rng.uniform(xr.min() - 0.05 * w, xr.max() + 0.05 * w, n), rng.uniform(yr.min() - 0.05 * hgt, yr.max() + 0.05 * hgt, n)
    z = rng.uniform(-1.0, 0.0, n) * mg.water_column(coords, fields, x, y)
    nt = len(coords["time"])
    t = rng.uniform(0.0, TSTEP * (nt - 1), n)
    X, Y = _nodes(coords)
    h64, s_w = np.asarray(fields["h"], dtype=np.float64), np.asarray(coords["s_w"], dtype=np.float64)
    zeta64 = np.asarray(fields["zeta"], dtype=np.float64)
    for r in range(0, n, 7):  # a seventh of the points: the edges, in turn
        kind = (r // 7) % 6
        if kind == 0:
            z[r] -= 200.0
        elif kind == 1:
            z[r] = float(rng.uniform(1.0, 30.0)) + float(np.max(np.abs(zeta64)))
        elif kind == 2:
            z[r] = (np.nan, np.inf, -np.inf)[(r // 42) % 3]
        else:  # on a node at a time level: exactly on a level, the floor, the surface
            jy, ix, ti = int(rng.integers(0, X.shape[0])), int(rng.integers(0, X.shape[1])), int(rng.integers(nt))
            jy, ix = min(jy, X.shape[0] - 2), min(ix, X.shape[1] - 2)
            xn, yn, hn, zn = _place(X, Y, h64, zeta64[ti], jy, ix, np.asarray(coords["x_rho"]).ndim == 2 and g["mesh"] == "spherical")
            x[r], y[r], t[r] = xn, yn, TSTEP * ti
            zv = _zvec(fields, g["hc"], s_w, hn, zn)
            z[r] = (zv[int(rng.integers(len(zv)))], -hn, zn)[kind - 3]
    return dict(coords=coords, fields={k: fields[k] for k in ("u", "v", "h", "zeta", "Cs_w")}, kind="sigma_points", x=x, y=y, z=z, t=t, hc=g["hc"],
                mesh=g["mesh"], agrid=g["agrid"], kernels=[], spatial_dtype="float64", dt=0.0, runtime=0.0, name=f"points_{seed}", seed=seed)


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------------
def oracle_case(case, variant=None) -> dict:
    """the case in the terms of oracle.c_oracle (make_croco_golden.ref_case is the same dict the reference's fieldset is built from)"""
    c = mg.ref_case(case)
    runtime, more = float(case["runtime"]), None
    if case.get("split"):
        runtime, more = float(case["split"]), [{"dt": float(case["dt"]), "runtime": float(case["runtime"]) - float(case["split"])}]
    c.update(kernels=list(case["kernels"]), x=np.asarray(case["x"]), y=np.asarray(case["y"]), z=np.asarray(case["z"]), dt=float(case["dt"]),
             runtime=runtime, more_calls=more, spatial_dtype=case["spatial_dtype"], t0=case.get("t0"), outputdt=case.get("outputdt"), variant=variant)
    if np.asarray(c["lon"]).ndim == 2:
        from parcels_amd.spatialhash import SpatialHash  # (the host builder, pinned to the reference's table by tests/test_host_logic.py)

        c["hash_table"] = SpatialHash(c["lon"], c["lat"], case["mesh"] == "spherical").table()
    return c


def run_oracle(case, variant=None) -> dict:
    """{"out": the SoA dict, "err": the raised error's name or None, "obs": [(time, columns)], "slim": per-particle flags}.  `slim` marks
    the particles a comparison with the device may leave out; no rule has been needed so far, so every flag is False."""
    c = oracle_case(case, variant)
    if case.get("kind") == "sigma_points":
        return {"sigma": c_oracle.sigma_points(c, case["t"], case["z"], case["y"], case["x"], variant=variant), "slim": np.zeros(len(case["x"]), bool)}
    with np.errstate(all="ignore"):
        out, err, stats = c_oracle.run_case(c)
    return {"out": out, "err": err, "obs": stats.get("observations", []), "slim": np.zeros(len(case["x"]), bool)}


# ---- the live reference ----------------------------------------------------------------------------------------------------------------
def run_reference(case):
    """(SoA dict, error name) of the reference on `case` with EVERY particle given a twin (the same release, ids n .. 2n - 1), the twins'
    rows dropped again.  A batch of one is the reference's known batch property (profiles/r04_fuzz_oracle_vs_reference.txt, item 10 b; here
    it shows as the spatial-hash query of the ONE particle that changed its cell in an evaluation, profiles/croco_oracle_vs_reference.txt):
    with twins no NumPy reduction ever sees a single column, and every particle still behaves as if it were alone."""
    n = len(case["x"])
    if case.get("kind") == "sigma_points":  # ({"sigma": ...}, None): the points twinned likewise
        with np.errstate(all="ignore"):
            ref, err = mg.run_case(dict(case, **{k: np.concatenate([np.asarray(case[k]), np.asarray(case[k])]) for k in ("x", "y", "z", "t")}))
        return {"sigma": ref["sigma"][:n]}, err
    twin = dict(case, **{k: np.concatenate([np.asarray(case[k]), np.asarray(case[k])]) for k in ("x", "y", "z", "t0")})
    ref, err = mg.run_case(twin)
    keep = ref["particle_id"] < n
    out = {k: v[keep] for k, v in ref.items() if not k.startswith("obs_")}
    if "obs_time" in ref:
        out["obs_time"] = ref["obs_time"]
        if "obs_offsets" in ref:
            off = ref["obs_offsets"]
            rows = [slice(off[j], off[j + 1]) for j in range(len(off) - 1)]
        else:
            rows = [j for j in range(len(ref["obs_time"]))]
        ids = [ref["obs_particle_id"][r] for r in rows]
        for k in ("particle_id", "t", "z", "y", "x"):
            out["obs_" + k] = [ref["obs_" + k][r][i < n] for r, i in zip(rows, ids)]
    return out, err


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.all((a == b) | ((a != a) & (b != b)))) if a.dtype.kind == "f" else bool(np.all(a == b))


def differences(case, res, ref, err) -> list:
    """what of the oracle's result `res` is not the reference's (`ref`, `err` of run_reference) to the bit: [] when nothing.  A run drawn
    to leave zeta's time interval is compared by the raised error's name alone (the columns are unspecified there)."""
    out = []
    if res["err"] != err:
        out.append(f"error {res['err']} vs {err}")
    if case.get("leaves") and err == "OutsideTimeInterval":
        return out
    for k, v in ref.items():
        if k.startswith("obs_"):
            continue
        if k not in res["out"]:
            out.append(f"column {k} missing")
        elif not same_bits(res["out"][k], v):
            a = res["out"][k]
            rows = "shape" if a.shape != v.shape else np.flatnonzero(~((a == v) | ((a != a) & (v != v))).reshape(len(v), -1).all(axis=1))[:5].tolist()
            out.append(f"{k} differs ({rows})")
    if "obs_time" in ref:
        if len(res["obs"]) != len(ref["obs_time"]):
            out.append(f"{len(res['obs'])} observations vs {len(ref['obs_time'])}")
        else:
            if not same_bits(np.array([tm for tm, _ in res["obs"]]), ref["obs_time"]):
                out.append("observation times differ")
            for j, (_, o) in enumerate(res["obs"]):
                for k in ("particle_id", "t", "z", "y", "x"):
                    if not same_bits(o[k], ref["obs_" + k][j]):
                        out.append(f"observation {j}: {k} differs")
    return out
