"""CPU: `pa.random` draws through the Python -> device-kernel translator (parcels_amd/jit.py), checked WITHOUT a GPU.

As in tests/test_jit_translator.py the C++ the translator emits compiles for the host: a shim of the device structs -- here with the launch's
seed in `KArgs::prm` and the kernel's position passed through as `kslot` --, csrc/pk_random.h with PK_DEV = static inline, g++ -O2
-ffp-contract=off, a loop over the particles that plays the stage machine.  The result is compared with the same Python function on
HostParticles carrying the draw context of that seed and position (what hostkernels.execute_hosted hands a kernel): bit for bit where only
`random`, `uniform` and `integers` enter, within 1e-12 where `normal` or `exponential` do (libm's log / cos against NumPy's)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parcels_amd
import parcels_amd as pa
from parcels_amd import StatusCode, jit
from parcels_amd import random as prandom
from parcels_amd.hostkernels import HostParticles
from parcels_amd.random import DrawContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <stdint.h>
#include <math.h>
#include <string.h>
#define PK_DEV static inline
#include "pk_random.h"
using namespace pk;
enum { RQ_UV = 0, RQ_UVW = 1, RQ_SCALAR = 2 };
enum { PK_ERROR = 50 };
struct PState { double t, z, y, x, dz, dy, dx, dt, next_dt; int64_t id; };
struct PCtx { int state; bool pf; int64_t row; int32_t ei0, ei1, ei2, ei3; };
struct Request { int kind, fidx; double t, z, y, x; bool f32; };
struct DParticles { void* extra[4]; };
struct ExecParams { uint64_t seed; };
struct KArgs { DParticles p; ExecParams prm; };
struct PkUserLocals {
%(decl)s
};
struct KLocal { double r[14]; PkUserLocals ul; };
static inline bool user_prepare(const KArgs& a, int uk, int stage, int kslot, PCtx& c, PState& p, KLocal& L, Request& rq) {
    switch (uk) {
        case 0: {
%(body)s
        }
        default: return true;
    }
}
// a sample (the kernels here take scalar samples of one field, for all particles) is answered with sample[i]
extern "C" void run(int64_t n, int pf, uint64_t seed, int kslot, double* t, double* z, double* y, double* x, double* dz, double* dy, double* dx, double* dt,
                    int32_t* state, int64_t* id, void* e0, void* e1, void* e2, void* e3, const double* sample) {
    KArgs a;
    a.prm.seed = seed;
    a.p.extra[0] = e0; a.p.extra[1] = e1; a.p.extra[2] = e2; a.p.extra[3] = e3;
    for (int64_t i = 0; i < n; i++) {
        PState p = {t[i], z[i], y[i], x[i], dz[i], dy[i], dx[i], dt[i], 0.0, id[i]};
        PCtx c = {state[i], pf != 0, i, 0, 0, 0, 0};
        KLocal L;
        memset(&L, 0, sizeof(L));
        Request rq;
        for (int stage = 0; !user_prepare(a, 0, stage, kslot, c, p, L, rq); stage++) L.r[3] = sample[i];
        t[i] = p.t; z[i] = p.z; y[i] = p.y; x[i] = p.x; dz[i] = p.dz; dy[i] = p.dy; dx[i] = p.dx; dt[i] = p.dt; state[i] = c.state;
    }
}
"""

SEED, KSLOT = 2**40 + 7, 3
VAR_SLOT = {"age": (0, "f32"), "acc": (1, "f64"), "count": (2, "i32"), "flag": (3, "i64")}


class _Field:
    def __init__(self, values):
        self.values = values

    def __getitem__(self, particles):
        return self.values[vars(particles)["_rows"]]


class _FieldSet:
    def __init__(self, context, fields):
        self.context, self.fields = dict(context), fields

    def __getattr__(self, name):
        d = self.__dict__
        if name in d.get("fields", {}):
            return d["fields"][name]
        if name in d.get("context", {}):
            return d["context"][name]
        raise AttributeError(name)


def _setup(spatial, n=257):
    P = pa.get_default_particle(spatial).add_variable([
        pa.Variable("age", dtype=np.float32, initial=0), pa.Variable("acc", dtype=np.float64, initial=0),
        pa.Variable("count", dtype=np.int32, initial=0), pa.Variable("flag", dtype=np.int64, initial=0)])
    rng = np.random.default_rng(5)
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    ids[:6] = [0, 1, 2**31, 2**32 + 5, 2**63 - 1, -1]
    t = np.where(np.arange(n) % 4 == 0, 600.0, 0.0)
    t[:5] = [0.0, -0.0, 600.0, -600.0, 1e9 + 0.5]
    data = {"particle_id": ids, "t": t, "dt": np.full(n, 600.0), "state": np.full(n, int(StatusCode.Evaluate), np.int32), "ei": np.zeros((n, 1), np.int32),
            "age": rng.normal(size=n).astype(np.float32), "acc": rng.normal(size=n), "count": rng.integers(-5, 9, n).astype(np.int32),
            "flag": rng.integers(-5, 9, n)}
    for k in ("x", "y", "z", "dx", "dy", "dz"):
        data[k] = rng.normal(scale=3.0, size=n).astype(spatial)
    fs = _FieldSet({"s": 25.0, "p_die": 0.2, "lo": -3, "hi": 12}, {"T": _Field(rng.normal(size=n))})
    return P, data, fs


def _translated(func, P, data, fs, tmp_path):
    src = jit.translate(func, P, fs, VAR_SLOT, {"T": 0})
    assert src.counter is None
    body = "\n".join("            " + ln for ln in src.case_body().split("\n"))
    cpp = tmp_path / f"{func.__name__}.cpp"
    so = tmp_path / f"{func.__name__}.so"
    cpp.write_text(SHIM % {"decl": "\n".join("    " + d for d in src.decl) or "    char unused;", "body": body})
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", f"-I{os.path.join(ROOT, 'parcels_amd', 'csrc')}", str(cpp), "-o",
                    str(so)], check=True)
    lib = C.CDLL(str(so))
    n = len(data["t"])
    cols = {k: np.array(data[k], dtype=np.float64) for k in ("t", "z", "y", "x", "dz", "dy", "dx", "dt")}
    state, pid = data["state"].copy(), data["particle_id"].copy()
    extras = [None] * 4
    for name, (slot, _) in VAR_SLOT.items():
        extras[slot] = data[name].copy()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.run(C.c_int64(n), C.c_int(int(data["x"].dtype == np.float32)), C.c_uint64(SEED), C.c_int(KSLOT), *[ptr(cols[k]) for k in ("t", "z", "y", "x", "dz", "dy", "dx", "dt")],
            ptr(state), ptr(pid), *[ptr(e) for e in extras], ptr(np.ascontiguousarray(fs.fields["T"].values)))
    out = {k: cols[k].astype(data[k].dtype) for k in cols}
    out["state"] = state
    for name, (slot, _) in VAR_SLOT.items():
        out[name] = extras[slot]
    return out, src


def _compare(func, spatial, tmp_path, exact):
    P, data, fs = _setup(spatial)
    got, src = _translated(func, P, data, fs, tmp_path)
    ref = {k: v.copy() for k, v in data.items()}
    func(HostParticles(ref, np.arange(len(ref["t"])), by_mask=True, rng=DrawContext(SEED, KSLOT)), fs)
    changed = 0
    for k in got:
        assert got[k].dtype == ref[k].dtype, k
        if exact or got[k].dtype.kind != "f":
            assert np.array_equal(got[k], ref[k]), (func.__name__, k, np.flatnonzero(got[k] != ref[k])[:5])
        else:
            err = np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64)).max()
            print(f"{func.__name__}.{k}: largest |translated - host| = {err:.3g}")
            assert err <= 1e-12, (func.__name__, k, err)
        changed += int(not np.array_equal(ref[k], data[k]))
    assert changed > 0  # (the kernel did something)
    return src


# ---- kernels: bit for bit -------------------------------------------------------------------------------------------------------------------
def DrawWhole(particles, fieldset):
    particles.acc = pa.random.random(particles)
    particles.dx += pa.random.uniform(-fieldset.s, fieldset.s, particles)
    particles.flag = pa.random.integers(fieldset.lo, fieldset.hi, particles)
    particles.count += pa.random.integers(0, 2**32, particles) > 2**31
    particles.state = np.where(pa.random.random(particles) < fieldset.p_die, StatusCode.Delete, particles.state)


def DrawSelection(particles, fieldset):
    old = particles[particles.age > 0]
    old.acc = prandom.uniform(1.0, 2.0, old)
    particles[particles.count > 2].acc += prandom.random(particles[particles.count > 2])
    r = parcels_amd.random.random(particles)
    particles.dy = np.where(r < 0.5, particles.dy, r)
    young = particles[~(particles.age > 0)]
    young[young.count < 0].flag = prandom.integers(100, 110, young[young.count < 0])


def DrawAcrossSample(particles, fieldset):
    a = pa.random.random(particles)
    temp = fieldset.T[particles]
    b = pa.random.uniform(temp, temp + 1.0, particles)
    particles.acc = a * temp + b
    particles.dz += a


def DrawArrayParamsExact(particles, fieldset):
    particles.acc = pa.random.uniform(particles.acc, particles.acc + np.abs(particles.age), particles)
    sel = particles[particles.count > 0]
    sel.dx = pa.random.uniform(sel.age, 2.0, sel)


# ---- kernels: normal / exponential (1e-12) ----------------------------------------------------------------------------------------------------
def Kick(particles, fieldset):
    particles.dx += pa.random.normal(0, fieldset.s, particles)
    particles.dy += pa.random.standard_normal(particles)
    particles.acc = pa.random.exponential(3.0, particles)


def KickAcrossSample(particles, fieldset):
    z = pa.random.standard_normal(particles)
    temp = fieldset.T[particles]
    particles.acc = z * temp + pa.random.exponential(2.0, particles)


def KickArrayParams(particles, fieldset):
    near = particles[particles.age < 0.5]
    near.acc = pa.random.normal(near.acc, np.abs(near.age) + 1.0, near)
    particles.dz += pa.random.exponential(np.abs(particles.age), particles)


@pytest.mark.parametrize("spatial", [np.float32, np.float64])
@pytest.mark.parametrize("func", [DrawWhole, DrawSelection, DrawAcrossSample, DrawArrayParamsExact])
def test_draws_translate_bit_for_bit(func, spatial, tmp_path):
    src = _compare(func, spatial, tmp_path, exact=True)
    assert len(src.stages) == (2 if func is DrawAcrossSample else 1)  # a draw is no request and no stage


@pytest.mark.parametrize("func", [Kick, KickAcrossSample, KickArrayParams])
def test_normal_and_exponential_translate_within_parity(func, tmp_path):
    # (float64 storage: a float32 column would round a 1e-16 difference of the variate to one float32 ulp now and then)
    _compare(func, np.float64, tmp_path, exact=False)


def test_draw_index_is_the_call_sites_ordinal():
    P, data, fs = _setup(np.float64)
    src = jit.translate(DrawWhole, P, fs, VAR_SLOT, {"T": 0})
    code = "\n".join(ln for st in src.stages for ln in st)
    assert [code.count(f"a.prm.seed, kslot, {k}, p.id, p.t") for k in range(6)] == [1, 1, 1, 1, 1, 0]
    # a value kept across a sample lives in a PkUserLocals slot
    src = jit.translate(DrawAcrossSample, P, fs, VAR_SLOT, {"T": 0})
    assert "random_random(" in "\n".join(src.stages[0]) and "random_random(" not in "\n".join(src.stages[1]) and any("double" in d for d in src.decl)


# ---- what stays on the host path ----------------------------------------------------------------------------------------------------------------
def DrawUnderAny(particles, fieldset):
    mask = particles.age > 0
    if np.any(mask):
        particles[mask].acc = pa.random.random(particles[mask])


def DrawOtherSelection(particles, fieldset):
    particles.acc = pa.random.normal(particles[particles.age > 0].acc, 1.0, particles)


def DrawIntegersArray(particles, fieldset):
    particles.flag = pa.random.integers(particles.flag, particles.flag + 5, particles)


def DrawIntegersSpan(particles, fieldset):
    particles.flag = pa.random.integers(0, 2**32 + 1, particles)


def DrawKeyword(particles, fieldset):
    particles.acc = pa.random.random(particles, stream=2)


def NumpyRandom(particles, fieldset):
    particles.dx += np.random.normal(0, 1, len(particles.x))


def test_what_is_not_translatable():
    P, data, fs = _setup(np.float64)
    tr = lambda f: jit.translate(f, P, fs, VAR_SLOT, {"T": 0})  # noqa: E731
    with pytest.raises(jit.NotTranslatable, match=r"^pa\.random\.random inside a block whose whole-set test is dropped"):
        tr(DrawUnderAny)
    with pytest.raises(jit.NotTranslatable, match=r"^pa\.random\.normal: a parameter array over another selection"):
        tr(DrawOtherSelection)
    with pytest.raises(jit.NotTranslatable, match=r"^pa\.random\.integers: low and high must be integer constants"):
        tr(DrawIntegersArray)
    with pytest.raises(jit.NotTranslatable, match=r"^pa\.random\.integers: high - low must lie in"):
        tr(DrawIntegersSpan)
    with pytest.raises(jit.NotTranslatable, match=r"^pa\.random\.random with keyword arguments"):
        tr(DrawKeyword)
    # np.random keeps doing what it did: the same refusal as before `pa.random` existed
    with pytest.raises(jit.NotTranslatable) as e:
        tr(NumpyRandom)
    assert str(e.value) == "call of something other than a supported numpy function"
    # ... and the host path runs the guarded kernel as Python would: the block is skipped when the selection is empty
    ref = {k: v.copy() for k, v in data.items()}
    ref["age"][:] = -1.0
    DrawUnderAny(HostParticles(ref, np.arange(len(ref["t"])), by_mask=True, rng=DrawContext(SEED, KSLOT)), fs)
    assert np.array_equal(ref["acc"], data["acc"])
