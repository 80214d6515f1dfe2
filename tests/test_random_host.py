"""CPU: the counter-based random stream of user kernels -- `pa.random` (parcels_amd/random.py), csrc/pk_random.h and the host loop.

The NumPy restatement in parcels_amd/random.py is the definition on the host path; csrc/pk_random.h is the same definition for the device
and compiles for the host too (g++ -O2 -ffp-contract=off, PK_DEV = static inline), which is how the two are compared here bit for bit
without a GPU.  Known answers: the published Random123 vectors of Philox4x32-10 and four rows of the (seed, slot, draw, id, t) layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import StatusCode
from parcels_amd.hostkernels import HostParticles
from parcels_amd.random import DrawContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IDS = np.array([0, 1, 2**31, 2**32 + 5, 2**63 - 1, -1], dtype=np.int64)
TIMES = np.array([0.0, -0.0, 600.0, -600.0, 1e9 + 0.5])
SEEDS = [0, 1, 2**40 + 7]


def _hex(w):
    return " ".join(f"{int(v):08x}" for v in np.asarray(w).ravel())


def test_random123_known_answers():
    assert _hex(pa.random.philox4x32([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(pa.random.philox4x32([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(pa.random.philox4x32([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # broadcast: many counters, one key
    many = pa.random.philox4x32(np.zeros((3, 4), np.uint32), [0, 0])
    assert many.shape == (3, 4) and many.dtype == np.uint32 and _hex(many[2]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


@pytest.mark.parametrize("pid, t, expect", [
    (0, 0.0, "75e21b75 634df118 220c1100 601744f1"),
    (1, -0.0, "dd524055 b10b3114 ca0cc903 cc40bd16"),
    (2**32 + 5, 600.0, "e3fb242a c59f425c 61ac56e5 4bf0bcb3"),
    (-1, 1e9 + 0.5, "a4eceedd 67830b9d f312727a 69474820"),
])
def test_layout_known_answers(pid, t, expect):
    w = pa.random.words(1, 0, 0, [pid], [t])
    assert w.shape == (1, 4) and w.dtype == np.uint32
    assert _hex(w) == expect


# ---- csrc/pk_random.h compiled for the host against the restatement -------------------------------------------------------------------------
HARNESS = r"""
#include <stdint.h>
#include <math.h>
#define PK_DEV static inline
#include "pk_random.h"
using namespace pk;
// dist: the PK_RANDOM_* codes of include/parcels_hip.h; out: 4 * n uint32 (words), n int64 (integers) or n double
extern "C" void fill(int dist, uint64_t seed, int slot, int draw, double p0, double p1, int64_t ilow, uint64_t span, const int64_t* ids,
                     const double* t, int64_t n, void* out) {
    for (int64_t i = 0; i < n; i++) {
        switch (dist) {
            case 0: random_words(seed, slot, draw, ids[i], t[i], (uint32_t*)out + 4 * i); break;
            case 1: ((double*)out)[i] = random_random(seed, slot, draw, ids[i], t[i]); break;
            case 2: ((double*)out)[i] = random_uniform(seed, slot, draw, ids[i], t[i], p0, p1); break;
            case 3: ((double*)out)[i] = random_standard_normal(seed, slot, draw, ids[i], t[i]); break;
            case 4: ((double*)out)[i] = random_normal(seed, slot, draw, ids[i], t[i], p0, p1); break;
            case 5: ((double*)out)[i] = random_exponential(seed, slot, draw, ids[i], t[i], p0); break;
            default: ((int64_t*)out)[i] = random_integers(seed, slot, draw, ids[i], t[i], ilow, span); break;
        }
    }
}
extern "C" double unit_of(uint32_t lo, uint32_t hi) { return random_unit(lo, hi); }
#ifdef PK_RANDOM_MAIN
#include <stdio.h>
int main(void) {  // the stand-alone program of the -fsanitize=undefined build: every distribution over edge ids, times, seeds, spans
    const int64_t ids[6] = {0, 1, 2147483648LL, 4294967301LL, 9223372036854775807LL, -1};
    const double t[6] = {0.0, -0.0, 600.0, -600.0, 1e9 + 0.5, 0.0};
    uint32_t w[24];
    double d[6];
    int64_t k[6];
    const uint64_t seeds[3] = {0, 1, (1ull << 40) + 7};
    for (int s = 0; s < 3; s++)
        for (int slot = -1; slot < 8; slot++)
            for (int draw = 0; draw < 4; draw++) {
                fill(0, seeds[s], slot, draw, 0, 0, 0, 1, ids, t, 6, w);
                for (int dist = 1; dist < 6; dist++) fill(dist, seeds[s], slot, draw, -2.5, 3.5, 0, 1, ids, t, 6, d);
                fill(6, seeds[s], slot, draw, 0, 0, INT64_MIN, 1ull << 32, ids, t, 6, k);
                fill(6, seeds[s], slot, draw, 0, 0, INT64_MAX, 1, ids, t, 6, k);
            }
    printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    return 0;
}
#endif
"""


@pytest.fixture(scope="module")
def header_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_random_host")
    cpp = d / "harness.cpp"
    cpp.write_text(HARNESS)
    so = d / "harness.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", f"-I{os.path.join(ROOT, 'parcels_amd', 'csrc')}", str(cpp), "-o",
                    str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.fill.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.unit_of.argtypes = [C.c_uint32, C.c_uint32]
    lib.unit_of.restype = C.c_double
    lib.workdir = d
    return lib


def _fill(lib, dist, seed, slot, draw, ids, t, p0=0.0, p1=0.0, ilow=0, span=1):
    ids, t = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(t, np.float64)
    n = len(ids)
    out = np.empty((n, 4), np.uint32) if dist == 0 else np.empty(n, np.int64 if dist == 6 else np.float64)
    lib.fill(dist, seed, slot, draw, p0, p1, ilow, span, ids.ctypes.data, t.ctypes.data, n, out.ctypes.data)
    return out


def test_header_equals_restatement(header_lib):
    from parcels_amd.random import _variates

    ids, t = (a.ravel() for a in np.meshgrid(IDS, TIMES, indexing="ij"))
    worst = {"normal": 0.0, "exponential": 0.0}
    for seed in SEEDS:
        for slot in range(8):
            for draw in range(4):
                w = pa.random.words(seed, slot, draw, ids, t)
                assert np.array_equal(_fill(header_lib, 0, seed, slot, draw, ids, t), w), (seed, slot, draw)
                assert np.array_equal(_fill(header_lib, 1, seed, slot, draw, ids, t), _variates(1, w))
                assert np.array_equal(_fill(header_lib, 2, seed, slot, draw, ids, t, -2.5, 3.5), _variates(2, w, np.float64(-2.5), np.float64(3.5)))
                for low, span in ((0, 10), (-7, 1), (-2**31, 2**32), (2**63 - 1, 1)):
                    assert np.array_equal(_fill(header_lib, 6, seed, slot, draw, ids, t, ilow=low, span=span), _variates(6, w, np.int64(low), np.uint64(span)))
                z = _variates(3, w)
                assert np.abs(z).max() < 8.66
                worst["normal"] = max(worst["normal"], np.abs(_fill(header_lib, 3, seed, slot, draw, ids, t) - z).max(),
                                      np.abs(_fill(header_lib, 4, seed, slot, draw, ids, t, 1.5, 0.25) - _variates(4, w, np.float64(1.5), np.float64(0.25))).max())
                worst["exponential"] = max(worst["exponential"], np.abs(_fill(header_lib, 5, seed, slot, draw, ids, t, 2.0) - _variates(5, w, np.float64(2.0))).max())
    print("largest |header - restatement|:", worst)
    assert worst["normal"] <= 1e-12 and worst["exponential"] <= 1e-12


def test_header_standalone_under_ubsan(header_lib):
    """The same harness as a stand-alone program built with -fsanitize=undefined (host code only; nothing of it is loaded into Python)."""
    exe = header_lib.workdir / "harness_ubsan"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-DPK_RANDOM_MAIN", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                        f"-I{os.path.join(ROOT, 'parcels_amd', 'csrc')}", str(header_lib.workdir / "harness.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "ubsan" in r.stderr:
        pytest.skip("this toolchain has no libubsan")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
    assert len(r.stdout.split()) == 4


# ---- ranges and errors -----------------------------------------------------------------------------------------------------------------------
def _view(ids, t, seed=1, slot=0):
    ids = np.asarray(ids, np.int64)
    data = {"particle_id": ids, "t": np.broadcast_to(np.asarray(t, np.float64), ids.shape).copy()}
    return HostParticles(data, np.arange(len(ids)), by_mask=True, rng=DrawContext(seed, slot))


def test_ranges_and_errors(header_lib):
    from parcels_amd.random import _unit, _variates

    for word in (0, 0xFFFFFFFF):
        w = np.full((1, 4), word, np.uint32)
        u = _variates(1, w)[0]
        assert 0.0 < u < 1.0 and u == _unit(w[:, 2], w[:, 3])[0] == header_lib.unit_of(word, word)
        assert np.isfinite(_variates(3, w)[0]) and np.isfinite(_variates(5, w, np.float64(1.0))[0])
    n = 4096
    for low, span in ((5, 1), (-3, 10), (-2**31, 2**32), (2**62, 2**32)):
        k = pa.random.integers(low, low + span, _view(np.arange(n), 600.0))
        assert k.dtype == np.int64 and k.shape == (n,) and k.min() >= low and k.max() < low + span
        assert span == 1 or len(np.unique(k)) > 1
    # the extreme words reach both ends of the range and no further
    for low, span in ((5, 1), (-3, 10), (-2**31, 2**32)):
        lo = _variates(6, np.zeros((1, 4), np.uint32), np.int64(low), np.uint64(span))[0]
        hi = _variates(6, np.full((1, 4), 0xFFFFFFFF, np.uint32), np.int64(low), np.uint64(span))[0]
        assert lo == low and hi == low + span - 1
    for low, high in ((3, 3), (0, 2**32 + 1), (5, 4)):
        with pytest.raises(ValueError, match="high - low must lie in"):
            pa.random.integers(low, high, _view(np.arange(4), 0.0))
    with pytest.raises(TypeError, match="ParticleSet"):
        pa.random.random(np.arange(4))
    with pytest.raises(TypeError, match="a selection of them"):
        pa.random.normal(0.0, 1.0)  # (neither a view nor a ParticleSet)
    with pytest.raises(ValueError, match="same selection"):
        pa.random.normal(np.zeros(3), 1.0, _view(np.arange(4), 0.0))


def test_distinct_and_equal_streams():
    base = dict(seed=1, slot=0, draw=0, ids=[7], t=[600.0])
    w0 = pa.random.words(**base)
    for change in (dict(seed=2), dict(seed=1 + 2**32), dict(slot=1), dict(draw=1), dict(ids=[8]), dict(ids=[7 + 2**32]), dict(t=[1200.0]), dict(t=[-600.0])):
        assert not np.array_equal(pa.random.words(**dict(base, **change)), w0), change
    assert np.array_equal(pa.random.words(1, 0, 0, [7, 7], [0.0, -0.0])[0], pa.random.words(1, 0, 0, [7, 7], [0.0, -0.0])[1])
    # a user draw never coincides with the built-in kernels' stream of the same seed and slot (plain hi32(seed) in k1)
    builtin = pa.random.philox4x32([7, 0, *np.array([600.0]).view(np.uint32)], [1 ^ 0x9E3779B9, 0])
    assert all(not np.array_equal(pa.random.words(1, 0, d, [7], [600.0])[0], builtin) for d in range(8))
    # a selection draws what the whole set draws for its rows, at an equal draw index; the counter is shared by the selections
    ids = np.arange(50) * 3 + 1
    mask = ids % 2 == 0
    a, b = _view(ids, 600.0), _view(ids, 600.0)
    whole0, whole1 = pa.random.random(a), pa.random.random(a)
    sel0 = pa.random.random(b[mask])
    sel1 = pa.random.random(b[np.flatnonzero(mask)][::2])
    assert np.array_equal(sel0, whole0[mask]) and np.array_equal(sel1, whole1[mask][::2]) and not np.array_equal(whole0, whole1)
    assert np.array_equal(pa.random.uniform(2.0, 3.5, b), 2.0 + (3.5 - 2.0) * pa.random.random(_advance(_view(ids, 600.0), 2)))  # (b has drawn twice)
    # parameter arrays over the selection
    loc = np.linspace(-1, 1, mask.sum())
    c, d = _view(ids, 600.0), _view(ids, 600.0)
    assert np.array_equal(pa.random.normal(loc, 0.5, c[mask]), loc + 0.5 * pa.random.standard_normal(d[mask]))


def _advance(view, draws):
    object.__getattribute__(view, "_rng").draws = draws
    return view


# ---- moments -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, slot, draw, t", [(1, 0, 0, 0.0), (1, 1, 0, 0.0), (1, 0, 1, 600.0), (2**40 + 7, 3, 2, -600.0)])
def test_moments(seed, slot, draw, t):
    """Each statistic within 5 standard errors of its exact value (N = 100 000; the standard errors are those of the exact distributions:
    var(U) = 1/12, var(U^2 - ...) -> var of the sample variance (mu4 - sigma^4) / N, the lag-1 correlation of independent draws ~ 1 / sqrt(N))."""
    from parcels_amd.random import _variates

    n = 100_000
    w = pa.random.words(seed, slot, draw, np.arange(n), np.full(n, t))
    u = _variates(1, w)
    z = _variates(3, w)
    e = _variates(5, w, np.float64(1.0))
    k = _variates(6, w, np.int64(0), np.uint64(10))
    stats = {
        "mean U": (u.mean() - 0.5, np.sqrt(1 / 12 / n)),
        "var U": (u.var() - 1 / 12, np.sqrt((1 / 80 - 1 / 144) / n)),  # mu4 = 1/80
        "mean Z": (z.mean(), np.sqrt(1 / n)),
        "var Z": (z.var() - 1.0, np.sqrt(2 / n)),  # mu4 = 3
        "mean E": (e.mean() - 1.0, np.sqrt(1 / n)),
        "lag-1 U": (np.corrcoef(u[:-1], u[1:])[0, 1], np.sqrt(1 / n)),
    }
    freq = np.bincount(k, minlength=10) / n
    assert k.min() == 0 and k.max() == 9
    for j in range(10):
        stats[f"bin {j}"] = (freq[j] - 0.1, np.sqrt(0.1 * 0.9 / n))
    for name, (err, se) in stats.items():
        print(f"{name}: {err / se:+.2f} standard errors")
        assert abs(err) <= 5 * se, (name, err, se)


# ---- the host loop -----------------------------------------------------------------------------------------------------------------------------
def Mortality(particles, fieldset):
    particles.state = np.where(pa.random.random(particles) < fieldset.p_die, StatusCode.Delete, particles.state)


def Kick(particles, fieldset):
    particles.dx += pa.random.normal(0, fieldset.s, particles)


def _host_run(order, seed, cuts=(12,), n=40):
    from case_utils import build_fieldset
    from oracle import cases
    from parcels_amd.hostkernels import execute_hosted
    from parcels_amd.kernel import Kernel

    case = cases.rect_agrid_case("random_loop", mesh="flat", kernels=["AdvectionRK4"], seed=1, npart=4, nx=6, ny=5, nz=2, nt=2)
    fs = build_fieldset(case)
    fs.add_context("p_die", 0.04)
    fs.add_context("s", 25.0)
    ids = np.arange(n, dtype=np.int64) * 5 + 2
    x0 = 100.0 + 10.0 * ids
    t0 = np.where(ids % 4 == 0, 600.0, 0.0)  # (a quarter starts one step late)
    o = np.asarray(order)
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x0[o], y=np.full(n, 500.0), z=np.zeros(n), t=t0[o], particle_ids=ids[o], seed=seed)
    pset._data["dt"][:] = 600.0
    done = 0
    for steps in cuts:
        done += steps
        execute_hosted(Kernel([Mortality, Kick], pset), pset, 600.0 * done, 600.0)
    d = pset._data
    return {int(i): (float(x), float(t), int(s)) for i, x, t, s in zip(d["particle_id"], d["x"], d["t"], d["state"])}


def test_host_loop_is_a_function_of_seed_id_and_time():
    n = 40
    a = _host_run(np.arange(n), seed=11)
    assert 0 < len(a) < n  # some died, some live
    assert len({round(x - (100.0 + 10.0 * i), 9) for i, (x, _, _) in a.items()}) == len(a)  # everybody was kicked their own way
    assert _host_run(np.random.default_rng(0).permutation(n), seed=11) == a  # another row order, the same ids
    assert _host_run(np.arange(n), seed=11, cuts=(6, 6)) == a  # 12 steps == 6 + 6
    b = _host_run(np.arange(n), seed=12)
    assert set(b) != set(a) or any(b[i] != a[i] for i in a)
    shared = sorted(set(a) & set(b))
    assert shared and all(a[i][0] != b[i][0] for i in shared)
