"""A seeded generator of named-vector-field cases, in the spec format of named_vector_utils.all_cases(): what the fixtures of
tests/golden/named_vectors_fuzz were drawn from (tools/make_named_vector_golden.py --fuzz runs them through the reference) and what the
GPU fuzz runs through the compiled list and the host path.

Every distinct (kernel sources, vector table, interpreter variant) is one hipcc build of a user module, so the MODULE SHAPE of a draw --
the kind and dtype of the currents, the vectors with their placement / interpolator / components / data dtype, and the kernel list, with
the fields in a fixed order -- comes from the table SHAPES (16 rows, seed % 16).  Everything else is drawn freely: mesh, grids, data,
particle dtype and positions, time axes, the sign of dt, release times, whether particles leave the vector's grid.

A draw the reference cannot be compared on (tools/make_named_vector_golden.py: _Watch, or an exception that is not a particle error) is
refused; `draw_spec(seed)` without `sub` reads the sub-draw that was used from the manifest next to the fixtures."""
from __future__ import annotations

import json
import os

import numpy as np

import named_vector_utils as nu
from oracle import cases as oc

FUZZ_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "named_vectors_fuzz")
MANIFEST = os.path.join(FUZZ_DIR, "manifest.json")
SEEDS = tuple(range(64))
COUNTS = (2, 63, 64, 65, 130, 255, 256, 257, 300)  # a wavefront edge (64) and a 256-lane block edge from either side
MAX_SUB = 4
MAX_STEPS = 12
HOUR = 3600.0


def _v(name, place, interp, ncomp, dtype):
    """place: 'main' (the currents' grid and time axis) | 'rect2' | 'rect2z' (a second rectilinear dataset without / with a depth axis) |
    'curv2' (a second curvilinear dataset); interp: 'lin' | 'cgrid' | 'free' | 'partial'"""
    return dict(name=name, place=place, interp=interp, ncomp=ncomp, dtype=dtype)


# cur: 'rectA' | 'curvA' | 'curvC' (rectilinear A-grid, curvilinear A-grid, curvilinear C-grid), fdt: the currents' data dtype, w: with W
SHAPES = (
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("Wind", "main", "lin", 2, "f64")], kernels=["AdvectionRK2", "WindMidpoint"]),
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("Wind", "main", "lin", 2, "f32")], kernels=["WindMidpoint", "AdvectionRK2", "DeleteParticle"]),
    dict(cur="rectA", fdt="f32", w=True, vecs=[_v("UVW2", "main", "free", 3, "f32")], kernels=["AdvectionRK4_3D", "SampleThree"]),
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("Wind", "main", "partial", 2, "f64")], kernels=["AdvectionRK2", "WindMidpoint", "DeleteParticle"]),
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("UVstokes", "rect2", "cgrid", 2, "f64")], kernels=["AdvectionRK4", "StokesEuler"]),
    dict(cur="rectA", fdt="f32", w=False, vecs=[_v("UVstokes", "rect2z", "cgrid", 2, "f32")], kernels=["AdvectionRK4", "StokesEuler", "DeleteParticle"]),
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("Wind", "rect2z", "lin", 2, "f64")], kernels=["AdvectionRK2", "WindDetached"]),
    dict(cur="curvA", fdt="f64", w=False, vecs=[_v("Wind", "main", "lin", 2, "f64")], kernels=["AdvectionRK4", "WindMidpoint"]),
    dict(cur="curvA", fdt="f32", w=False, vecs=[_v("Disp", "main", "lin", 2, "f32")], kernels=["AdvectionRK2", "Unbeach", "DeleteParticle"]),
    dict(cur="curvC", fdt="f64", w=True, vecs=[_v("UVW2", "main", "cgrid", 3, "f64")], kernels=["AdvectionRK4_3D", "SampleThree"]),
    dict(cur="curvC", fdt="f32", w=False, vecs=[_v("Wind", "main", "cgrid", 2, "f32")], kernels=["AdvectionRK4", "WindMidpoint", "DeleteParticle"]),
    dict(cur="curvA", fdt="f64", w=False, vecs=[_v("Wind", "main", "free", 2, "f64")], kernels=["AdvectionRK4", "WindMidpoint"]),
    dict(cur="curvA", fdt="f32", w=True, vecs=[_v("UVW2", "main", "partial", 3, "f32")], kernels=["AdvectionRK4_3D", "SampleThree", "DeleteParticle"]),
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("UVstokes", "curv2", "lin", 2, "f64")], kernels=["AdvectionRK2", "StokesEuler", "DeleteParticle"]),
    dict(cur="curvC", fdt="f64", w=False, vecs=[_v("Wind", "main", "cgrid", 2, "f64"), _v("UVstokes", "rect2", "lin", 2, "f32")],
         kernels=["AdvectionRK4", "WindMidpoint", "StokesEuler"]),
    dict(cur="rectA", fdt="f64", w=False, vecs=[_v("Wind", "main", "lin", 2, "f64"), _v("UVstokes", "curv2", "cgrid", 2, "f32")],
         kernels=["AdvectionRK2", "StokesEuler", "WindMidpoint", "DeleteParticle"]),
)
COMPONENTS = {"Wind": ("UWind", "VWind"), "UVstokes": ("Ustokes", "Vstokes"), "UVW2": ("U2", "V2", "W2"), "Disp": ("UDisp", "VDisp")}
_DT = {"f32": np.float32, "f64": np.float64}


def vector_kind(shape, vec):
    """KIND of eval_vec: 1 on a curvilinear grid"""
    return int(shape["cur"] != "rectA") if vec["place"] == "main" else int(vec["place"] == "curv2")


def vector_interp(vec):
    """INTERP of eval_vec"""
    return {"lin": 0, "cgrid": 1, "free": 2, "partial": 2}[vec["interp"]]


def _second(vec, *, lon, lat, depth, time_s, scale, rng, mesh):
    """A dataset of its own for one vector: its grid, its time axis, its components (staggered where CGrid_Velocity reads them)."""
    names = COMPONENTS[vec["name"]]
    ny, nx = (len(lat), len(lon)) if np.ndim(lon) == 1 else np.shape(lon)
    shp = (len(time_s), 1 if depth is None else len(depth), ny, nx)
    zc, zn = ("mockZ", "mockZ") if depth is None else ("ZC", "depth")
    cg = vec["interp"] == "cgrid"
    dims = [("time", zc, "YC", "XG"), ("time", zc, "YG", "XC")] if cg else [("time", zn, "YG", "XG")] * 2
    fields = {n: oc.smooth_random_field(rng, shp, scale).astype(_DT[vec["dtype"]]) for n in names}
    s = dict(mesh=mesh, lon=np.asarray(lon, dtype=np.float64), lat=np.asarray(lat, dtype=np.float64), depth=depth, time_s=np.asarray(time_s, dtype=float),
             fields=fields, field_dims=dict(zip(names, dims)), x_pad="low", y_pad="low", z_pad="high" if cg else "both", vectors={vec["name"]: names})
    if cg:
        s["interp"] = {vec["name"]: "cgrid"}
    return s


def draw(seed, sub):
    """-> (spec, the drawn dimensions as a JSON-able dict)"""
    shape = SHAPES[seed % len(SHAPES)]
    rng = np.random.default_rng([977, seed, sub])
    n = COUNTS[seed % len(COUNTS)]
    # (on the warped spherical mesh the reference's point-in-cell test gives up on about one interior particle in a hundred; a list without
    # DeleteParticle ends there, so those lists mostly draw the flat mesh and run to the end)
    ends_early = shape["cur"] != "rectA" and "DeleteParticle" not in shape["kernels"]
    mesh = str(rng.choice(["flat", "spherical"], p=[0.75, 0.25] if ends_early else [0.5, 0.5]))
    pdt = str(rng.choice(["float32", "float64"]))
    backward = bool(rng.random() < 0.3)
    stagger = bool(n >= 63 and rng.random() < 0.4)
    oob = bool(n >= 63 and rng.random() < 0.4)
    dt = 1800.0
    nsteps = int(rng.integers(8, MAX_STEPS + 1))
    runtime = nsteps * dt
    cur_ldt, cur_nt = float(rng.choice([3.0, 4.0])) * HOUR, int(rng.integers(3, 5))
    if stagger:  # (staggered releases need a ring of 3 slots: four levels keep that ring a ring on the currents' axis too)
        cur_nt = 4
    name = f"nvf_{seed}"
    kernels = list(shape["kernels"])
    kw = dict(mesh=mesh, kernels=kernels, seed=int(rng.integers(1 << 30)), nz=3, nt=cur_nt, npart=n, field_dtype=_DT[shape["fdt"]], spatial_dtype=pdt,
              with_w=shape["w"], dt=dt, runtime=runtime)
    if shape["cur"] == "rectA":
        c = oc.rect_agrid_case(name, nx=12, ny=9, vel=20.0 if mesh == "spherical" else 2.0, margin=0.3, level_dt=cur_ldt, **kw)
    else:
        c = oc.curv_cgrid_case(name, nx=14, ny=11, vel=5.0 if mesh == "spherical" else 0.3, cgrid=shape["cur"] == "curvC", **kw)
        c["time_s"] = np.arange(cur_nt) * cur_ldt
    spec = dict(currents=c, vectors={}, kernels=kernels, context={}, interp={})
    lon, lat = np.asarray(c["lon"]), np.asarray(c["lat"])
    spans, first = [float(c["time_s"][-1])], cur_ldt
    curv2 = next((v for v in shape["vecs"] if v["place"] == "curv2"), None)
    if curv2 is not None:  # the release moves into the second, curvilinear grid (itself moved inside the currents' rectilinear one)
        lon2, lat2 = oc.curvilinear_grid(9, 8, mesh=mesh)
        lon2, lat2 = (lon2 + 150.0, lat2) if mesh == "spherical" else (lon2 + 1.5e5, lat2 + 0.5e5)
        ci, cj = rng.uniform(0.15, 0.85, n) * 8, rng.uniform(0.15, 0.85, n) * 7
        i0, j0 = ci.astype(int), cj.astype(int)
        fi, fj = ci - i0, cj - j0
        blend = lambda a: a[j0, i0] * (1 - fi) * (1 - fj) + a[j0, i0 + 1] * fi * (1 - fj) + a[j0 + 1, i0] * (1 - fi) * fj + a[j0 + 1, i0 + 1] * fi * fj  # noqa: E731
        c["x"], c["y"] = blend(lon2), blend(lat2)
    x0, x1, y0, y1 = float(np.min(c["x"])), float(np.max(c["x"])), float(np.min(c["y"])), float(np.max(c["y"]))
    leavers = np.sort(rng.choice(n, size=max(2, n // 12), replace=False)) if oob else np.zeros(0, int)
    left_main = False
    for vec in shape["vecs"]:
        comps = COMPONENTS[vec["name"]][:vec["ncomp"]]
        scale = {"Wind": 8.0, "UVstokes": 0.2 if mesh == "spherical" else 0.05, "UVW2": 0.5, "Disp": 2.0}[vec["name"]] * (1.0 if mesh == "spherical" else 0.2)
        vseed = int(rng.integers(1 << 30))
        if vec["place"] == "main":
            like = ("U", "V", "W") if vec["interp"] == "cgrid" else None
            if like is not None and vec["ncomp"] == 3 and "W" not in c["fields"]:
                raise AssertionError("a three-component C-grid vector needs currents with W")
            nu._same_grid_vector(c, comps, scale=scale, seed=vseed, dtype=_DT[vec["dtype"]], like=like, land=vec["interp"] in ("free", "partial"))
            spec["vectors"][vec["name"]] = comps
            if vec["interp"] != "lin":
                spec["interp"][vec["name"]] = vec["interp"]
            if oob and len(shape["vecs"]) == 1:  # some particles are released beyond the grid's eastern edge
                c["x"] = np.array(c["x"], dtype=np.float64)
                c["x"][leavers] = float(lon.max()) + 0.03 * float(lon.max() - lon.min())
                left_main = True
            continue
        ldt2, nt2 = float(rng.choice([2.0, 3.0])) * HOUR, int(rng.integers(4, 6))
        time2 = np.arange(nt2) * ldt2
        spans.append(float(time2[-1]))
        first = ldt2
        depth2 = np.linspace(0.0, float(np.asarray(c["depth"])[-1]), 3) if vec["place"] == "rect2z" else None
        if vec["place"] == "curv2":
            s = _second(vec, lon=lon2, lat=lat2, depth=None, time_s=time2, scale=scale, rng=np.random.default_rng(vseed), mesh=mesh)
            if oob:  # beyond the second grid's eastern edge, inside the currents' grid
                c["x"] = np.array(c["x"], dtype=np.float64)
                c["x"][leavers] = float(lon2.max()) + 0.02 * float(lon2.max() - lon2.min())
        else:  # around the release area, or (for particles to leave it) a little smaller than that
            pad = -0.06 if oob else 0.2
            s = _second(vec, lon=np.linspace(x0 - pad * (x1 - x0), x1 + pad * (x1 - x0), 7), lat=np.linspace(y0 - pad * (y1 - y0), y1 + pad * (y1 - y0), 6),
                        depth=depth2, time_s=time2, scale=scale, rng=np.random.default_rng(vseed), mesh=mesh)
        spec["second"] = s
    if not spec["interp"]:
        del spec["interp"]
    # time: forward from 0 or backward from the end of the shortest axis (a level of it); staggered releases cover the first level interval
    # of the vector's axis in quarters, so some sit exactly on a level
    tend = min(spans)
    t0 = np.zeros(n) if not backward else np.full(n, tend)
    if stagger:
        t0 = t0 + (-1.0 if backward else 1.0) * rng.integers(0, 5, n) * (first / 4.0)
    c["t0"] = t0
    if backward:
        c["dt"] = -dt
    if "Unbeach" in kernels:
        spec["context"]["shore"] = float(np.median(c["x"]))
        spec["variables"] = [("beached", "int32")]
    if "SampleThree" in kernels:
        spec["variables"] = [("u2", "float64"), ("v2", "float64"), ("w2", "float64")]
    if any(k.startswith("Wind") for k in kernels):
        spec["context"]["windage"] = 0.03
    dims = dict(seed=seed, sub=sub, shape=seed % len(SHAPES), currents=shape["cur"], currents_dtype=shape["fdt"], with_w=shape["w"], mesh=mesh, particles=pdt,
                npart=n, backward=backward, staggered=stagger, leavers=int(len(leavers)), left_main=left_main, nsteps=nsteps, kernels=kernels,
                delete="DeleteParticle" in kernels, detached="WindDetached" in kernels, time_levels=[len(c["time_s"])] + ([len(spec["second"]["time_s"])] if "second" in spec else []),
                vectors=[dict(name=v["name"], place=v["place"], FT={"f32": "float", "f64": "double"}[v["dtype"]], KIND=vector_kind(shape, v), INTERP=vector_interp(v),
                              interp=v["interp"], ncomp=v["ncomp"]) for v in shape["vecs"]])
    return spec, dims


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def draw_spec(seed, sub=None):
    """The spec of a seed: sub-draw `sub`, or the one the manifest says the fixture was written from."""
    if sub is None:
        row = load_manifest()["seeds"][str(seed)] if os.path.exists(MANIFEST) else {"sub": 0}
        sub = row["sub"]
        if sub is None:
            raise LookupError(f"seed {seed}: every sub-draw was refused")
    return draw(seed, sub)[0]


def fixture_path(seed):
    return os.path.join(FUZZ_DIR, f"nvf_{seed}.npz")
