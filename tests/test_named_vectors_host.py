"""CPU: named vector fields (wind, Stokes drift, ...) without a GPU -- FieldSet + FieldSet, the translator's `fieldset.<Name>[...]`
(compiled for the host against the shim of tests/named_vector_utils.py and compared bit for bit with NumPy running the same kernel), the
reference's documented wind kernel in the survey, and the fixtures of tests/golden/named_vectors against a fresh run of the reference."""
import ast
import os
import sys
import warnings

import numpy as np
import pytest

import named_vector_kernels as nk
import named_vector_utils as nu
import parcels_amd as pa
from oracle import ref_shim
from parcels_amd import StatusCode, jit
from parcels_amd.hostkernels import HostParticles

needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. FieldSet + FieldSet ------------------------------------------------------------------------------------------------------------
def _two(time_b=np.arange(4) * 50000.0):
    specs = nu.all_cases()
    a = nu._pa_fieldset_of(specs["nv_a_adv_wind"]["currents"], {"Wind": ("UWind", "VWind")})
    s = nu._second_grid(("Ustokes", "Vstokes"), lon=(0.0, 360.0), lat=(-80.0, 80.0), time_s=time_b, scale=0.2, seed=1)
    return a, nu._pa_fieldset_of(s, {"UVstokes": ("Ustokes", "Vstokes")})


def test_add_merges_fields_context_models_and_time():
    a, b = _two()
    a.add_context("windage", 0.03)
    b.add_context("stokes_factor", 1.5)
    c = a + b
    assert isinstance(c, pa.FieldSet) and c is not a and c is not b
    assert list(c.fields) == list(a.fields) + list(b.fields) and c.models == a.models + b.models
    assert c.context == {"windage": 0.03, "stokes_factor": 1.5} and c.windage == 0.03
    assert isinstance(c.UVstokes, pa.VectorField) and c.UVstokes.U is c.Ustokes
    assert len(c.gridset) == 2 and c.UV.igrid == 0 and c.UVstokes.igrid == 1 and c.Ustokes.igrid == 1
    ta, tb = a.models[0].time_interval, b.models[0].time_interval
    assert c.time_interval.left == max(ta.left, tb.left) and c.time_interval.right == min(ta.right, tb.right)  # 150000 s of the 172800 s
    assert c.time_interval.right == tb.right != ta.right
    assert c.__dict__["_engine"] is None  # no device copy before the sum is used


def test_iadd():
    a, b = _two()
    a0 = a
    a += b
    assert a is not a0 and "UVstokes" in a.fields and "Wind" in a.fields and len(a.models) == 2


def test_an_operand_is_not_used_after_the_addition():
    a, b = _two()
    c = a + b
    for operand in (a, b):
        with pytest.raises(RuntimeError, match="its fields belong to the sum now"):
            operand._engine_or_create()
        with pytest.raises(RuntimeError, match="use the sum"):
            operand.to_device()
    assert c.__dict__.get("_absorbed") is None and c.Ustokes._fieldset is c
    a2, _ = _two()
    with pytest.raises(ValueError):
        a2 + _two()[0]
    assert a2.__dict__.get("_absorbed") is None  # (a refused addition leaves the operands alone)


def test_add_disjoint_time_axes_have_no_time_interval():
    a, b = _two(time_b=400000.0 + np.arange(3) * 1000.0)
    assert (a + b).time_interval is None


def test_add_refuses_duplicates_and_other_types():
    a, b = _two()
    a2, _ = _two()
    with pytest.raises(ValueError, match=r"Cannot add FieldSets that have field names in common. Duplicate field names are: \['U', 'UV'"):
        a + a2
    a.add_context("k", 1.0)
    b.add_context("k", 2.0)
    with pytest.raises(ValueError, match=r"Cannot add FieldSets that have context value names in common. Duplicate context value names are: \['k'\]"):
        a + b
    assert a.__add__(3) is NotImplemented
    with pytest.raises(TypeError):
        a + 3
    with pytest.raises(TypeError):
        a + {"U": 1}


def test_add_warns_about_mixed_meshes():
    a, _ = _two()
    s = nu._second_grid(("Ustokes", "Vstokes"), lon=(0.0, 4.0e5), lat=(0.0, 2.0e5), time_s=np.arange(3) * 1000.0, scale=0.2, seed=1, mesh="flat")
    with pytest.warns(pa.fieldset.FieldSetWarning, match="multiple different meshes"):
        a + nu._pa_fieldset_of(s, {"UVstokes": ("Ustokes", "Vstokes")})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a2, b2 = _two()
        a2 + b2  # two spherical meshes of one radius are one mesh


def _live(name):
    """A function of the reference's fieldset.py, executed from its source text (the module itself needs xarray to import)."""
    path = os.path.join(ref_shim.REFERENCE_SRC, "parcels", "_core", "fieldset.py")
    text = open(path).read()
    for node in ast.walk(ast.parse(text)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            ns = {}
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), {"FieldSet": object, "__builtins__": __builtins__}, ns)  # noqa: S102
            return ns[name]
    raise LookupError(name)


@needs_reference
def test_add_refusals_against_the_live_reference():
    check = _live("assert_compatible_fieldsets")

    def outcome(f):
        try:
            f()
            return ("ok", None)
        except Exception as e:  # noqa: BLE001
            return (type(e).__name__, str(e))

    a, b = _two()
    a2, _ = _two()
    assert outcome(lambda: check(a, b)) == ("ok", None) and isinstance(a + b, pa.FieldSet)
    assert outcome(lambda: check(a, a2)) == outcome(lambda: a + a2) and outcome(lambda: a + a2)[0] == "ValueError"
    a.add_context("k", 1.0)
    a.add_context("j", 1.0)
    b.add_context("k", 2.0)
    b.add_context("j", 2.0)
    assert outcome(lambda: check(a, b)) == outcome(lambda: a + b) and outcome(lambda: a + b)[0] == "ValueError"


@needs_reference
@pytest.mark.parametrize("pair", [("spherical", "spherical"), ("spherical", "flat"), ("spherical", 6.0e6), ("flat", "flat")], ids=str)
def test_mixed_mesh_warning_against_the_live_reference(pair):
    """the reference's own _warn_if_fields_use_different_meshes on ITS mesh objects: when it warns, and with which words"""
    R = ref_shim.load_reference()["mesh"]

    class FieldSetWarning(UserWarning):
        pass

    path = os.path.join(ref_shim.REFERENCE_SRC, "parcels", "_core", "fieldset.py")
    node = next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name == "_warn_if_fields_use_different_meshes")
    for arg in node.args.args:  # (the annotations name classes of modules that do not import here)
        arg.annotation = None
    ns = {}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"),  # noqa: S102
         {"warnings": warnings, "FieldSetWarning": FieldSetWarning, "__builtins__": __builtins__}, ns)
    from types import SimpleNamespace as NS

    def ref_mesh(m):
        return R.get_mesh(m) if isinstance(m, str) else R.SphericalMesh(m)

    def own_mesh(m):
        return m if isinstance(m, str) else pa.xgrid.SphericalMesh(m)

    with warnings.catch_warnings(record=True) as wr:
        warnings.simplefilter("always")
        ns["_warn_if_fields_use_different_meshes"]([NS(grid=NS(_mesh=ref_mesh(m))) for m in pair])
    a, _ = _two()
    kw = dict(lon=(0.0, 360.0), lat=(-80.0, 80.0)) if pair[1] != "flat" else dict(lon=(0.0, 4.0e5), lat=(0.0, 2.0e5))
    s = nu._second_grid(("Ustokes", "Vstokes"), time_s=np.arange(3) * 1000.0, scale=0.2, seed=1, mesh=own_mesh(pair[1]), **kw)
    if pair[0] == "flat":
        s0 = nu._second_grid(("UA", "VA"), lon=(0.0, 4.0e5), lat=(0.0, 2.0e5), time_s=np.arange(3) * 1000.0, scale=0.2, seed=2, mesh="flat")
        a = nu._pa_fieldset_of(s0, {"UVA": ("UA", "VA")})
    with warnings.catch_warnings(record=True) as wo:
        warnings.simplefilter("always")
        a + nu._pa_fieldset_of(s, {"UVstokes": ("Ustokes", "Vstokes")})
    wo = [w for w in wo if issubclass(w.category, pa.fieldset.FieldSetWarning)]
    assert len(wr) == len(wo) == (0 if pair[0] == pair[1] else 1)
    if wr:  # the same words around the set of meshes, and the same meshes in it (both print as <Kind>Mesh(...))
        mr, mo = str(wr[0].message), str(wo[0].message)
        assert mr.split("{")[0] == mo.split("{")[0] and mr.split("}")[1] == mo.split("}")[1]
        assert sorted(mr.split("{")[1].split("}")[0].split(", ")) == sorted(mo.split("{")[1].split("}")[0].split(", "))


# ---- 2. the translator on the host -----------------------------------------------------------------------------------------------------
KEYS = {"Wind": 3 * 8 + 0, "Disp": 3 * 8 + 0, "UVW2": 3 * 8 + 0, "UVstokes": 3 * 8 + 0}  # RQ_VEC * 8 + j, j = 0: the kernel's only named vector


def _columns(P, n, seed):
    rng = np.random.default_rng(seed)
    data = {}
    for v in P.variables:
        dt = np.dtype(v.dtype)
        if v.name == "ei":
            data["ei"] = np.zeros((n, 1), np.int32)
        elif v.name == "state":
            data["state"] = rng.choice([int(StatusCode.Evaluate), int(StatusCode.Success), 60, 70], size=n).astype(np.int32)
        elif v.name == "particle_id":
            data["particle_id"] = np.arange(n, dtype=np.int64)
        elif dt.kind == "f":
            data[v.name] = rng.normal(scale=3.0, size=n).astype(dt)
        else:
            data[v.name] = rng.integers(-5, 9, size=n).astype(dt)
    data["x"] = (170.0 + rng.normal(scale=30.0, size=n)).astype(data["x"].dtype)  # (some on either side of fieldset.shore)
    data["dt"] = np.full(n, 600.0)
    data.setdefault("ei", np.zeros((n, 1), np.int32))
    return data


@pytest.mark.parametrize("spatial", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", [nk.WindMidpoint, nk.StokesEuler, nk.Unbeach, nk.SampleThree, nk.WindDetached], ids=lambda f: f.__name__)
def test_translated_kernel_is_numpy_bit_for_bit(kernel, spatial, tmp_path):
    n = 65
    P = pa.get_default_particle(spatial).add_variable([pa.Variable("beached", dtype=np.int32, initial=0), pa.Variable("u2", dtype=np.float64, initial=0),
                                                       pa.Variable("v2", dtype=np.float32, initial=0), pa.Variable("w2", dtype=np.float64, initial=0)])
    var_slot = {"beached": (0, "i32"), "u2": (1, "f64"), "v2": (2, "f32"), "w2": (3, "f64")}
    data = _columns(P, n, seed=7)
    rng = np.random.default_rng(8)
    effects = (np.where(rng.random((nu.NKEY, n)) < 0.15, rng.choice([60, 61, 70], size=(nu.NKEY, n)), 0).astype(np.int32),
               rng.integers(1, 1000, size=(nu.NKEY, n)).astype(np.int32))
    log = []
    fields = {name: nu.FakeVector(name, key, 3 if name == "UVW2" else 2, log, effects) for name, key in KEYS.items()}
    fs = nu.FakeFieldSet({"windage": 0.03, "shore": 170.0}, fields)
    got, req, asked, src = nu.run_translated(kernel, P, fs, data, var_slot, effects, tmp_path)
    assert all(isinstance(s, str) and s not in ("UV", "UVW") for s in src.sampled) and len(src.sampled) >= 1
    text = "\n".join(ln for st in src.stages for ln in st)
    assert "rq.kind = RQ_VEC; rq.fidx = 0;" in text and "RQ_UV;" not in text
    ref = {k: v.copy() for k, v in data.items()}
    with np.errstate(all="ignore"):
        kernel(HostParticles(ref, np.arange(n)), fs)
    for k in got:
        assert got[k].dtype == ref[k].dtype, k
        assert np.array_equal(got[k], ref[k], equal_nan=True), (kernel.__name__, k, np.flatnonzero(got[k] != ref[k])[:5])
    # the sample points and field keys NumPy logged are the requests of the translated kernel, for the same particles
    assert len(log) == len(src.sampled)
    for k, e in enumerate(log):
        lanes = np.flatnonzero(asked[k])
        rows = np.arange(n) if e["rows"] is None else e["rows"]
        assert np.array_equal(lanes, rows), (k, lanes[:5], rows[:5])
        for j, c in enumerate("tzyx"):
            assert np.array_equal(req[k, j, lanes], np.broadcast_to(e[c], lanes.shape)), (k, c)
        assert np.all(req[k, 4, lanes] == float(e["f32"])) and np.all(req[k, 5, lanes] == e["field"])
    assert not asked[len(log):].any()


def SwapLocals(particles, fieldset):
    a = particles.dx + 1.0
    b = particles.dy * 3.0
    a, b = (b + 1.0, a * 2.0)  # every value is computed before the first name is bound
    c, d = (-a, np.abs(b) + particles.dz)
    particles.dx = a
    particles.dy = b
    particles.dz = c * d


@pytest.mark.parametrize("spatial", [np.float64, np.float32], ids=["f64", "f32"])
def test_tuple_assignment_of_computed_values_binds_after_all_are_computed(spatial, tmp_path):
    n = 65
    P = pa.get_default_particle(spatial)
    data = _columns(P, n, seed=9)
    fs = nu.FakeFieldSet({}, {})
    zeros = (np.zeros((nu.NKEY, n), np.int32), np.zeros((nu.NKEY, n), np.int32))
    got, req, asked, src = nu.run_translated(SwapLocals, P, fs, data, {}, zeros, tmp_path)
    ref = {k: v.copy() for k, v in data.items()}
    SwapLocals(HostParticles(ref, np.arange(n)), fs)
    for k in got:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=True), k
    assert not np.array_equal(got["dx"], data["dx"]) and not asked.any()


def NameSwap(particles, fieldset):
    a = particles.dx + 1.0
    b = particles.dy + 1.0
    a, b = (b, a)
    particles.dx = a


def test_tuple_assignment_of_bare_names_stays_refused():
    with pytest.raises(jit.NotTranslatable, match="tuple assignment of something other than a vector sample"):
        jit.translate(NameSwap, pa.get_default_particle(np.float64), nu.FakeFieldSet({}, {}), {}, {})


def test_two_kernels_of_one_module_share_the_vector_table():
    P = pa.get_default_particle(np.float64).add_variable(pa.Variable("beached", dtype=np.int32, initial=0))
    fields = {name: nu.FakeVector(name, 0, 2, [], None) for name in ("Wind", "Disp")}
    fs = nu.FakeFieldSet({"windage": 0.03, "shore": 170.0}, fields)
    names = []
    a = jit.translate(nk.Unbeach, P, fs, {"beached": (0, "i32")}, {}, slot_prefix="k0_", vectors=names)
    b = jit.translate(nk.WindMidpoint, P, fs, {"beached": (0, "i32")}, {}, slot_prefix="k1_", vectors=names)
    assert names == ["Disp", "Wind"] and a.sampled == ["Disp"] and b.sampled == ["Wind", "Wind"]
    assert "rq.fidx = 1;" in "\n".join(ln for st in b.stages for ln in st)
    prog = jit.UserProgram([a, b], 0, 1, fast=1, vectors=[("Disp", 4, 5, -1, "double", 0, 0), ("Wind", 2, 3, -1, "float", 1, 3)])
    assert "#define PK_USER_VECTORS 1\n" in prog.source and prog.source.index("PK_USER_VECTORS") < prog.source.index('#include "pk_kernels.h"')
    assert "case 0: eval_vec<double, 0, 0>(a, mc, c, 4, 5, -1, 0, false," in prog.source
    assert "case 1: eval_vec<float, 1, 2>(a, mc, c, 2, 3, -1, 3, false," in prog.source
    assert not prog.flags & 1 and "advect_fast_kernel" not in prog.source  # never rides in a dedicated kernel
    other = jit.UserProgram([a, b], 0, 1, vectors=[("Disp", 4, 5, -1, "double", 0, 0), ("Wind", 2, 3, -1, "double", 1, 3)])
    assert other.digest != prog.digest  # the table is part of what the module cache is keyed by
    with pytest.raises(jit.NotTranslatable, match="^vector field 'Disp'"):
        jit.UserProgram([a, b], jit.PK_USER_KEY_UX, 0, vectors=[("Disp", 4, 5, -1, "double", 0, 0)])
    with pytest.raises(jit.NotTranslatable, match="^vector field 'Disp'"):
        jit.UserProgram([a, b], jit.PK_USER_KEY_SIGMA, 0, vectors=[("Disp", 4, 5, -1, "double", 0, 0)])


def test_module_without_named_vectors_is_unchanged():
    def Age(particles, fieldset):
        particles.dx += 1.0

    P = pa.get_default_particle(np.float64)
    prog = jit.UserProgram([jit.translate(Age, P, nu.FakeFieldSet({}, {}), {}, {})], 0, 1, fast=1)
    assert "PK_USER_VECTORS" not in prog.source and "user_eval_vec" not in prog.source and prog.flags & 1


# ---- 3. the reference's documented kernel ----------------------------------------------------------------------------------------------
@needs_reference
def test_documented_wind_kernel_translates():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import survey_user_kernels as sv

    rows = [r for r in sv.survey() if r[0].endswith("explanation_kernelloop.md") and r[1] == "windRK2"]
    assert len(rows) == 1 and rows[0][2] == "translated", rows


# ---- 4. the fixtures -------------------------------------------------------------------------------------------------------------------
def test_every_case_has_a_fixture():
    assert sorted(os.path.basename(p)[:-4] for p in os.listdir(nu.GOLDEN_DIR) if p.endswith(".npz")) == sorted(nu.all_cases())
    for name in nu.all_cases():
        assert os.path.getsize(nu.fixture_path(name)) < 16 * 1024


@needs_reference
@pytest.mark.parametrize("name", sorted(nu.all_cases()))
def test_fixture_is_reproduced_by_the_generator(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_named_vector_golden as gen

    out, err = gen.run_reference(nu.all_cases()[name])
    ref, rerr = nu.load_fixture(name)
    assert err == rerr and set(out) == set(ref)
    for k in out:
        assert np.asarray(out[k]).dtype == ref[k].dtype and np.array_equal(np.asarray(out[k]), ref[k], equal_nan=True), k
