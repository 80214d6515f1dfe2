"""Shared by the named-vector-field tests and tools/make_named_vector_golden.py: the cases (grids, data, particles, kernel lists), the
parcels_amd FieldSet of a case, the fixtures' names, and a host harness for the translator (the idea of tests/test_jit_translator.py: the
emitted C++ is plain scalar code, so a 40-line shim of the device structs compiles it with g++ and plays the stage machine; this shim knows
the request kind RQ_VEC = 3 of a named vector field)."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import numpy as np

from oracle import cases as oc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "named_vectors")
NODE = ("time", "depth", "YG", "XG")
NODE2D = ("time", "mockZ", "YG", "XG")  # a field without a vertical axis (wind, Stokes drift at the surface)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _agrid(name, kernels, *, npart=65, spatial="float64", with_w=False, vel=1.0, seed=3, level_dt=86400.0):
    """Currents on the rectilinear A-grid: 12 x 9 x 3 nodes, 3 time levels a day apart, spherical."""
    return oc.rect_agrid_case(name, mesh="spherical", kernels=kernels, seed=seed, nx=12, ny=9, nz=3, nt=3, npart=npart, spatial_dtype=spatial,
                              with_w=with_w, dt=3600.0, runtime=8 * 3600.0, vel=vel, margin=0.3, level_dt=level_dt)


def _same_grid_vector(case, names, *, scale, seed, dtype=np.float64, offset=0.0, like=None, land=False):
    """More fields on the currents' own grid and time axis (the documented wind example: one dataset, two vector fields)."""
    rng = np.random.default_rng(seed)
    shp = np.asarray(case["fields"]["U"]).shape
    for k, n in enumerate(names):
        case["fields"][n] = (oc.smooth_random_field(rng, shp, scale * (0.01 if k == 2 else 1.0)) + (offset if k == 0 else 0.0)).astype(dtype)
        if land:  # a block of zero velocity in the middle of the release area: what the slip interpolators look for
            case["fields"][n][:, :, 3:5, 4:7] = 0.0
        case["field_dims"][n] = NODE if like is None else case["field_dims"][like[k]]  # (like: staggered as the currents' components are)
    return case


def _second_grid(names, *, lon, lat, time_s, scale, seed, offset=0.0, mesh="spherical"):
    """A dataset of its own: 7 x 6 nodes, no vertical axis, its own time axis."""
    rng = np.random.default_rng(seed)
    shp = (len(time_s), 1, 6, 7)
    fields = {n: oc.smooth_random_field(rng, shp, scale) + (offset if k == 0 else 0.0) for k, n in enumerate(names)}
    return dict(mesh=mesh, lon=np.linspace(lon[0], lon[1], 7), lat=np.linspace(lat[0], lat[1], 6), depth=None, time_s=np.asarray(time_s, dtype=float),
                fields=fields, field_dims={n: NODE2D for n in names}, x_pad="low", y_pad="low")


def all_cases() -> dict:
    """name -> spec: `currents` (a case dict of oracle/cases.py; named vectors on its grid in `vectors`), optionally `second` (another
    dataset with `vectors` of its own, added with FieldSet + FieldSet), `kernels` (names: built-in ones or those of named_vector_kernels),
    `variables` [(name, dtype)], `context`; `interp` {vector: 'cgrid' | 'free' | 'partial'} (also inside `second`, which may have a `depth` and
    2-D `lon` / `lat`); release times in `currents["t0"]` (zero when absent)."""
    out = {}
    wind = {"Wind": ("UWind", "VWind")}
    for order, kl in (("adv_wind", ["AdvectionRK2", "WindMidpoint"]), ("wind_adv", ["WindMidpoint", "AdvectionRK2"])):
        c = _same_grid_vector(_agrid(f"nv_a_{order}", kl), ("UWind", "VWind"), scale=8.0, seed=11)
        out[c["name"]] = dict(currents=c, vectors=wind, kernels=kl, context={"windage": 0.03})
    for n in (65, 2):  # b: currents on the curvilinear C-grid, Stokes drift from a second dataset on a small rectilinear grid
        c = oc.curv_cgrid_case(f"nv_b_stokes_{n}", mesh="spherical", kernels=["AdvectionRK4", "StokesEuler"], seed=8, nx=14, ny=11, nz=3, nt=3, npart=n,
                               field_dtype=np.float64, with_w=False, dt=1800.0, runtime=8 * 1800.0, vel=0.3)
        s = _second_grid(("Ustokes", "Vstokes"), lon=(-60.0, 80.0), lat=(0.0, 85.0), time_s=np.arange(4) * 50000.0, scale=0.2, seed=12)
        s["vectors"] = {"UVstokes": ("Ustokes", "Vstokes")}
        out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=c["kernels"], context={})
    c = _same_grid_vector(_agrid("nv_c_three", ["AdvectionRK4_3D", "SampleThree"], with_w=True), ("U2", "V2", "W2"), scale=0.5, seed=13)
    out[c["name"]] = dict(currents=c, vectors={"UVW2": ("U2", "V2", "W2")}, kernels=c["kernels"], context={},
                          variables=[("u2", "float64"), ("v2", "float64"), ("w2", "float64")])
    for n in (65, 2):  # d: float32 particles, float32 wind data
        kl = ["AdvectionRK2", "WindMidpoint"]
        c = _same_grid_vector(_agrid(f"nv_d_f32_{n}", kl, npart=n, spatial="float32"), ("UWind", "VWind"), scale=8.0, seed=11, dtype=np.float32)
        out[c["name"]] = dict(currents=c, vectors=wind, kernels=kl, context={"windage": 0.03})
    kl = ["AdvectionRK2", "Unbeach"]
    c = _same_grid_vector(_agrid("nv_e_unbeach", kl), ("UDisp", "VDisp"), scale=2.0, seed=14, offset=3.0)
    out[c["name"]] = dict(currents=c, vectors={"Disp": ("UDisp", "VDisp")}, kernels=kl, context={"shore": 170.0}, variables=[("beached", "int32")])
    for tail in ((), ("DeleteParticle",)):  # f: a particle leaves the smaller wind grid inside the currents' grid
        kl = ["AdvectionRK2", "WindMidpoint", *tail]
        c = _agrid("nv_f_leaves" + ("_delete" if tail else ""), kl, vel=0.05)
        c["x"][0], c["y"][0] = 269.98, 10.0  # just inside the wind grid's eastern edge, in a steady westerly wind
        s = _second_grid(("UWind", "VWind"), lon=(90.0, 270.0), lat=(-60.0, 60.0), time_s=np.arange(3) * 86400.0, scale=1.0, seed=15, offset=9.0)
        s["vectors"] = wind
        out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={"windage": 0.03})
    kl = ["AdvectionRK2", "WindMidpoint"]  # g: the wind's time axis ends (at 4 h) before the run does (8 h)
    c = _agrid("nv_g_wind_ends", kl)
    s = _second_grid(("UWind", "VWind"), lon=(0.0, 360.0), lat=(-80.0, 80.0), time_s=np.arange(3) * 7200.0, scale=8.0, seed=16)
    s["vectors"] = wind
    out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={"windage": 0.03})
    # h: for a ring of 2 level slots -- currents with a level every 4 h, wind from another dataset with a level every 2 h, 8 h of run
    c = _agrid("nv_h_stream", kl, level_dt=4 * 3600.0)
    s = _second_grid(("UWind", "VWind"), lon=(0.0, 360.0), lat=(-80.0, 80.0), time_s=np.arange(5) * 7200.0, scale=8.0, seed=17)
    s["vectors"] = wind
    out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={"windage": 0.03})
    # j: a C-grid wind (staggered like the currents, CGrid_Velocity, packed on the device) on the curvilinear grid the currents live on
    kl = ["AdvectionRK4", "WindMidpoint"]
    c = oc.curv_cgrid_case("nv_j_cgrid_wind", mesh="spherical", kernels=kl, seed=8, nx=14, ny=11, nz=3, nt=3, npart=65, field_dtype=np.float64,
                           with_w=False, dt=1800.0, runtime=8 * 1800.0, vel=0.3)
    c = _same_grid_vector(c, ("UWind", "VWind"), scale=5.0, seed=18, like=("U", "V"))
    out[c["name"]] = dict(currents=c, vectors=wind, interp={"Wind": "cgrid"}, kernels=kl, context={"windage": 0.03})
    for slip in ("free", "partial"):  # k: a wind with a slip boundary condition (XFreeslip / XPartialslip) next to plain XLinear_Velocity currents
        kl = ["AdvectionRK2", "WindMidpoint"]
        c = _same_grid_vector(_agrid(f"nv_k_{slip}slip", kl), ("UWind", "VWind"), scale=8.0, seed=19, land=True)
        out[c["name"]] = dict(currents=c, vectors=wind, interp={"Wind": slip}, kernels=kl, context={"windage": 0.03})
    # l: g with releases three quarters of a step apart.  In the iteration that finds the early releases at 3 h and the late ones at 3.75 h,
    # the midpoint sample of WindMidpoint asks for 3.5 h and for 4.25 h: only the late ones are past the wind's last level (4 h), and the
    # reference gives the whole view the code (field.py:31-44).  The early releases stop at 3 h although both of their own samples of that
    # step lie inside the axis; a per-particle rule would carry them on to 4 h.
    kl = ["AdvectionRK2", "WindMidpoint"]
    c = _agrid("nv_l_partial_time_end", kl)
    c["t0"] = np.where(np.arange(65) % 3 == 0, 0.0, 2700.0)
    s = _second_grid(("UWind", "VWind"), lon=(0.0, 360.0), lat=(-80.0, 80.0), time_s=np.arange(3) * 7200.0, scale=8.0, seed=16)
    s["vectors"] = wind
    out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={"windage": 0.03})
    # m: two named vectors in one list -- j's C-grid wind on the curvilinear main grid and b's Stokes drift on a second, rectilinear grid
    kl = ["AdvectionRK4", "WindMidpoint", "StokesEuler"]
    c = oc.curv_cgrid_case("nv_m_two_vectors", mesh="spherical", kernels=kl, seed=8, nx=14, ny=11, nz=3, nt=3, npart=65, field_dtype=np.float64,
                           with_w=False, dt=1800.0, runtime=8 * 1800.0, vel=0.3)
    c = _same_grid_vector(c, ("UWind", "VWind"), scale=5.0, seed=18, like=("U", "V"))
    s = _second_grid(("Ustokes", "Vstokes"), lon=(-60.0, 80.0), lat=(0.0, 85.0), time_s=np.arange(4) * 50000.0, scale=0.2, seed=12)
    s["vectors"] = {"UVstokes": ("Ustokes", "Vstokes")}
    out[c["name"]] = dict(currents=c, vectors=wind, interp={"Wind": "cgrid"}, second=s, kernels=kl, context={"windage": 0.03})
    # n: a flat mesh; the Stokes drift (XLinear_Velocity) on a second, CURVILINEAR grid inside the currents' rectilinear one, a steady
    # eastward drift that carries the particles released near its eastern edge out of it
    kl = ["AdvectionRK2", "StokesEuler", "DeleteParticle"]
    c = oc.rect_agrid_case("nv_n_second_curvilinear", mesh="flat", kernels=kl, seed=5, nx=12, ny=9, nz=3, nt=3, npart=130, dt=1800.0, runtime=8 * 1800.0,
                           vel=0.2, margin=0.3, level_dt=86400.0)
    lon2, lat2 = oc.curvilinear_grid(9, 8, mesh="flat")
    lon2, lat2 = lon2 + 1.5e5, lat2 + 0.5e5
    rng = np.random.default_rng(21)
    ci, cj = rng.uniform(0.15, 0.85, 130) * 8, rng.uniform(0.15, 0.85, 130) * 7
    ci[::10] = rng.uniform(7.6, 7.98, 13)  # in the easternmost cells
    i0, j0 = ci.astype(int), cj.astype(int)
    fi, fj = ci - i0, cj - j0
    for key, a in (("x", lon2), ("y", lat2)):
        c[key] = a[j0, i0] * (1 - fi) * (1 - fj) + a[j0, i0 + 1] * fi * (1 - fj) + a[j0 + 1, i0] * (1 - fi) * fj + a[j0 + 1, i0 + 1] * fi * fj
    shp = (3, 1, 8, 9)
    s = dict(mesh="flat", lon=lon2, lat=lat2, depth=None, time_s=np.arange(3) * 20000.0, x_pad="low", y_pad="low",
             fields={"Ustokes": oc.smooth_random_field(rng, shp, 0.05) + 0.4, "Vstokes": oc.smooth_random_field(rng, shp, 0.05)},
             field_dims={"Ustokes": NODE2D, "Vstokes": NODE2D}, vectors={"UVstokes": ("Ustokes", "Vstokes")})
    out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={})
    # o: 257 particles (a block of 256 lanes and one more) with DeleteParticle; f's westerly wind carries one particle of the first, one of
    # a middle and the one of the last wavefront over the wind grid's eastern edge, each on another step
    kl = ["AdvectionRK2", "WindMidpoint", "DeleteParticle"]
    c = _agrid("nv_o_blocks", kl, npart=257, vel=0.05)
    for row, gap in ((3, 0.004), (130, 0.035), (256, 0.053)):  # (the windage moves a particle 0.009 degrees a step here)
        c["x"][row], c["y"][row] = 270.0 - gap, 10.0
    s = _second_grid(("UWind", "VWind"), lon=(90.0, 270.0), lat=(-60.0, 60.0), time_s=np.arange(3) * 86400.0, scale=1.0, seed=15, offset=9.0)
    s["vectors"] = wind
    out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={"windage": 0.03})
    # p: the detached sample (no particles in the key: no state change, no `ei` update) of a wind on a second, rectilinear grid
    kl = ["AdvectionRK2", "WindDetached"]
    c = _agrid("nv_p_detached", kl)
    s = _second_grid(("UWind", "VWind"), lon=(0.0, 360.0), lat=(-80.0, 80.0), time_s=np.arange(5) * 7200.0, scale=8.0, seed=22)
    s["vectors"] = wind
    out[c["name"]] = dict(currents=c, vectors={}, second=s, kernels=kl, context={"windage": 0.03})
    return out


def fixture_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def save_fixture(path, out, err, meta=None):
    arrs = {"out__" + k: np.asarray(v) for k, v in out.items()}
    arrs["meta"] = np.array(json.dumps({"err": err, **(meta or {})}))
    np.savez_compressed(path, **arrs)


def load_fixture(name, path=None):
    """-> (final columns of the reference's run, name of the error it raised or None)"""
    z = np.load(path or fixture_path(name), allow_pickle=False)
    return {k[5:]: z[k] for k in z.files if k.startswith("out__")}, json.loads(str(z["meta"]))["err"]


# ---- the parcels_amd side ------------------------------------------------------------------------------------------------------------
def _pa_fieldset_of(ds_case, vectors):
    """One dataset -> a parcels_amd FieldSet (tests/case_utils.py: build_fieldset, with the vector fields named explicitly)."""
    import parcels_amd as pa

    pad = {"low": pa.Padding.LOW, "high": pa.Padding.HIGH, "both": pa.Padding.BOTH, "none": pa.Padding.NONE}
    depth = ds_case.get("depth")
    md = pa.SGrid2DMetadata(
        node_dimensions=("XG", "YG"), node_coordinates=("lon", "lat"),
        face_dimensions=(pa.FaceNodePadding("XC", "XG", pad[ds_case.get("x_pad", "low")]), pa.FaceNodePadding("YC", "YG", pad[ds_case.get("y_pad", "low")])),
        vertical_dimensions=(pa.FaceNodePadding("ZC", "depth", pad[ds_case.get("z_pad", "both")]),) if depth is not None else None)
    lon, lat = np.asarray(ds_case["lon"]), np.asarray(ds_case["lat"])
    coords = {"lon": ((("XG",) if lon.ndim == 1 else ("YG", "XG")), lon), "lat": ((("YG",) if lat.ndim == 1 else ("YG", "XG")), lat)}
    if depth is not None:
        coords["depth"] = (("depth",), np.asarray(depth))
    coords["time"] = (("time",), np.asarray(ds_case["time_s"], dtype=np.float64))
    data_vars = {}
    for name, arr in ds_case["fields"].items():
        dims, a = tuple(ds_case["field_dims"][name]), np.asarray(arr)
        keep = [i for i, d in enumerate(dims) if not d.startswith("mock")]
        data_vars[name] = (tuple(dims[i] for i in keep), a.reshape([a.shape[i] for i in keep]))
    names = set(data_vars)
    vf = dict(vectors)
    if {"U", "V"} <= names:
        vf["UV"] = ("U", "V")
    if {"U", "V", "W"} <= names:
        vf["UVW"] = ("U", "V", "W")
    fs = pa.FieldSet.from_sgrid_conventions(pa.Dataset(data_vars, coords, sgrid=md), mesh=ds_case["mesh"], vector_fields=vf)
    if ds_case.get("cgrid"):
        for vname in ("UV", "UVW"):
            if vname in fs.fields and not isinstance(fs.fields[vname].interp_method, pa.CGrid_Velocity):
                fs.fields[vname].interp_method = pa.CGrid_Velocity()
    return fs


def _interp_method(how):
    import parcels_amd as pa

    return {"cgrid": pa.CGrid_Velocity, "free": pa.XFreeslip, "partial": pa.XPartialslip}[how]()


def build_fieldset(spec):
    """The FieldSet of a case; a second dataset is added the documented way, `fs_currents + fs_second`."""
    import parcels_amd as pa

    fs = _pa_fieldset_of(spec["currents"], spec["vectors"])
    for vname, how in spec.get("interp", {}).items():
        fs.fields[vname].interp_method = _interp_method(how)
    if spec.get("second"):
        fs2 = _pa_fieldset_of(spec["second"], spec["second"]["vectors"])
        for vname, how in spec["second"].get("interp", {}).items():
            fs2.fields[vname].interp_method = _interp_method(how)
        fs = fs + fs2
    for k, v in spec["context"].items():
        fs.add_context(k, v)
    return fs


def kernel_list(spec):
    import parcels_amd as pa

    import named_vector_kernels as nk

    return [getattr(nk, k) if hasattr(nk, k) else getattr(pa.kernels, k) for k in spec["kernels"]]


def build_pset(spec, fs):
    import parcels_amd as pa

    c = spec["currents"]
    P = pa.get_default_particle(np.dtype(c["spatial_dtype"]).type)
    for vn, dt in spec.get("variables", ()):
        P = P.add_variable(pa.Variable(vn, dtype=np.dtype(dt).type, initial=0))
    t0 = np.zeros(len(c["x"])) if c.get("t0") is None else np.asarray(c["t0"], dtype=np.float64)  # (release times: zero unless the case staggers them)
    return pa.ParticleSet(fs, pclass=P, x=np.asarray(c["x"]), y=np.asarray(c["y"]), z=np.asarray(c["z"]), t=t0)


ERRORS = ("FieldOutOfBoundError", "FieldOutOfBoundSurfaceError", "FieldInterpolationError", "GridSearchingError", "OutsideTimeInterval", "GeneralError")


def run_case(spec, *, jit=True, nslots=None):
    """Run a case through parcels_amd, compiled (the default) or with PARCELS_AMD_JIT=0 on the host path.
    -> (ParticleSet, final columns, name of the error raised or None)"""
    import warnings

    import parcels_amd as pa

    old = os.environ.get("PARCELS_AMD_JIT")
    os.environ["PARCELS_AMD_JIT"] = "1" if jit else "0"
    try:
        fs = build_fieldset(spec)
        if nslots is not None:
            fs.to_device(nslots=nslots)
        pset = build_pset(spec, fs)
        err = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                pset.execute(kernel_list(spec), dt=float(spec["currents"]["dt"]), runtime=float(spec["currents"]["runtime"]))
            except tuple(getattr(pa, e) for e in ERRORS) as e:
                err = type(e).__name__
        return pset, {k: np.array(v) for k, v in pset._data.items()}, err
    finally:
        if old is None:
            os.environ.pop("PARCELS_AMD_JIT", None)
        else:
            os.environ["PARCELS_AMD_JIT"] = old


# ---- the translator on the host ------------------------------------------------------------------------------------------------------
SHIM = r"""
#include <stdint.h>
#include <math.h>
#include <string.h>
#define PK_DEV static inline
enum { RQ_UV = 0, RQ_UVW = 1, RQ_SCALAR = 2, RQ_VEC = 3 };
enum { PK_ERROR = 50 };
struct PState { double t, z, y, x, dz, dy, dx, dt, next_dt; int64_t id; };
struct PCtx { int state; bool pf; int64_t row; int32_t ei0, ei1, ei2, ei3; };
struct Request { int kind, fidx; double t, z, y, x; bool f32; };
struct DParticles { void* extra[4]; };
struct KArgs { DParticles p; };
struct PkUserLocals {
%(decl)s
};
struct KLocal { double r[14]; PkUserLocals ul; };
PK_DEV bool user_prepare(const KArgs& a, int uk, int stage, int kslot, PCtx& c, PState& p, KLocal& L, Request& rq) {
    switch (uk) {
        case 0: {
%(body)s
        }
        default: return true;
    }
}
// A sample of field key fk = kind * 8 + fidx answers component j with the function value(fk, j, point) below (the Python side computes the
// same), raises the state to sstate[fk * n + i] and writes sei[fk * n + i] into ei0 when the particles came along (a sample without them
// is followed by generated code that restores both).  req[(k * 6 + j) * n + i]: t, z, y, x, f32 flag, fk of the k-th request of the kernel.
extern "C" void run(int64_t n, int pf, double* t, double* z, double* y, double* x, double* dz, double* dy, double* dx, double* dt, int32_t* state,
                    int64_t* id, void* e0, void* e1, void* e2, void* e3, const int32_t* sstate, const int32_t* sei, int32_t* ei0, double* req,
                    uint8_t* asked, int32_t maxreq) {
    KArgs a;
    a.p.extra[0] = e0; a.p.extra[1] = e1; a.p.extra[2] = e2; a.p.extra[3] = e3;
    for (int64_t i = 0; i < n; i++) {
        PState p = {t[i], z[i], y[i], x[i], dz[i], dy[i], dx[i], dt[i], 0.0, id[i]};
        PCtx c = {state[i], pf != 0, i, ei0[i], 0, 0, 0};
        KLocal L;
        memset(&L, 0, sizeof(L));
        Request rq;
        for (int stage = 0; !user_prepare(a, 0, stage, 0, c, p, L, rq); stage++) {
            const int k = %(ordinal)s;
            if (k < 0 || k >= maxreq) return;
            const int fk = rq.kind * 8 + rq.fidx;
            for (int j = 0; j < 3; j++) L.r[3 + j] = ((((rq.x * 1.25 + rq.y * 0.5) - rq.z * 0.25) + rq.t * 0.001) + fk) * (j + 1);
            const double r6[6] = {rq.t, rq.z, rq.y, rq.x, rq.f32 ? 1.0 : 0.0, (double)fk};
            for (int j = 0; j < 6; j++) req[((int64_t)k * 6 + j) * n + i] = r6[j];
            asked[(int64_t)k * n + i] = 1;
            if (sstate[(int64_t)fk * n + i] > c.state) c.state = sstate[(int64_t)fk * n + i];
            c.ei0 = sei[(int64_t)fk * n + i];
        }
        ei0[i] = c.ei0;
        t[i] = p.t; z[i] = p.z; y[i] = p.y; x[i] = p.x; dz[i] = p.dz; dy[i] = p.dy; dx[i] = p.dx; dt[i] = p.dt; state[i] = c.state;
    }
}
"""
NKEY = 32


class _Grid:
    is_curvilinear = False


class FakeVector:
    """What the translator and a NumPy run of the kernel need of a vector field: `U` (with a grid), an optional `W`, and `[...]`, which
    answers with a function of the sample point, logs it, and does to the particles what the library's sampling does."""

    def __init__(self, name, key, ncomp, log, effects):
        self.name, self.key, self.ncomp, self.log, self.effects = name, key, ncomp, log, effects
        self.U = self.V = type("F", (), {"grid": _Grid()})()
        self.W = self.U if ncomp == 3 else None

    def __getitem__(self, key):
        particles = key[4] if isinstance(key, tuple) and len(key) == 5 else (None if isinstance(key, tuple) else key)
        rows = None if particles is None else np.asarray(vars(particles)["_rows"])
        t, z, y, x = key[:4] if isinstance(key, tuple) else (particles.t, particles.z, particles.y, particles.x)
        e = {"field": self.key, "rows": rows, "f32": np.asarray(y).dtype == np.float32, "attached": particles is not None,
             **{k: np.asarray(v, dtype=np.float64) for k, v in zip("tzyx", (t, z, y, x))}}
        self.log.append(e)
        if particles is not None:
            sstate, sei = self.effects
            particles.state = np.maximum(np.asarray(particles.state), sstate[self.key][rows])
            vars(particles)["_data"]["ei"][rows, 0] = sei[self.key][rows]
        base = (((e["x"] * 1.25 + e["y"] * 0.5) - e["z"] * 0.25) + e["t"] * 0.001) + self.key
        return tuple(base * (j + 1) for j in range(self.ncomp))


class FakeFieldSet:
    def __init__(self, context, fields):
        self.context, self.fields, self.gridset = dict(context), fields, [_Grid()]

    def __getattr__(self, name):
        d = self.__dict__
        if name in d.get("fields", {}):
            return d["fields"][name]
        if name in d.get("context", {}):
            return d["context"][name]
        raise AttributeError(name)


def run_translated(func, pclass, fieldset, data, var_slot, effects, tmp_path, maxreq=4):
    """Translate `func`, compile it against the shim and run it over the columns `data` -> (columns, requests [maxreq, 6, n], asked
    [maxreq, n], the translated source)."""
    from parcels_amd import jit

    src = jit.translate(func, pclass, fieldset, var_slot, {})
    body = "\n".join("            " + ln for ln in src.case_body().split("\n"))
    code = SHIM % {"decl": "\n".join("    " + d for d in src.decl) or "    char unused;", "body": body,
                   "ordinal": "stage" if src.counter is None else f"{src.counter} - 1"}
    cpp, so = tmp_path / f"{func.__name__}.cpp", tmp_path / f"{func.__name__}.so"
    cpp.write_text(code)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", str(cpp), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    n = len(data["t"])
    cols = {k: np.array(data[k], dtype=np.float64) for k in ("t", "z", "y", "x", "dz", "dy", "dx", "dt")}
    state, pid = data["state"].copy(), data["particle_id"].copy()
    extras = [None] * 4
    for name, (slot, _) in var_slot.items():
        extras[slot] = data[name].copy()
    sstate, sei = (np.ascontiguousarray(a, dtype=np.int32) for a in effects)
    ei0 = np.array(data["ei"][:, 0], dtype=np.int32)
    req, asked = np.zeros((maxreq, 6, n)), np.zeros((maxreq, n), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    lib.run(C.c_int64(n), C.c_int(int(data["x"].dtype == np.float32)), *[ptr(cols[k]) for k in ("t", "z", "y", "x", "dz", "dy", "dx", "dt")], ptr(state),
            ptr(pid), *[ptr(e) for e in extras], ptr(sstate), ptr(sei), ptr(ei0), ptr(req), ptr(asked), C.c_int32(maxreq))
    out = {k: cols[k].astype(data[k].dtype) for k in cols}
    out["state"], out["ei"] = state, ei0.reshape(-1, 1)
    for name, (slot, _) in var_slot.items():
        out[name] = extras[slot]
    return out, req, asked.astype(bool), src
