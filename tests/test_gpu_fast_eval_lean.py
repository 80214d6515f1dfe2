"""The trimmed evaluation of the dedicated 2-D A-grid kernel's lean build (csrc/pk_fast_agrid.h): corner blocks kept in the polynomial basis
of the bilinear form (lp_field / lp_sum), cos(lat) of the unit conversion as 1 - 2 sin(lat / 2)^2 with cos_lat behind a call beyond +-86
degrees (cos_lat_lean), and a ravelled index with one full-rate product.

Every case runs the kernel with the level-pair cache (option "block_cache" 2), the same arithmetic with the block formed in registers in every
evaluation (0: equal in every bit), the general program and the CPU oracle: positions within 1e-12 on the coordinate scale, the discrete
columns (state, ei, t, dt, ids) and the step / attempt counters exact.  The ravelled index needs no size condition -- the strides it
multiplies are bounded by the coordinate tables the kernel holds in LDS -- so there is no grid "on the other side" to test.

The last test holds the cosine, evaluated on the device (tools/cos_lean_check.hip), to its reasoned bound against cos in extended precision:
4.5 * 2^-53 absolute below 1.5 rad (rounding of sin(lat / 2), doubled by the square, plus the final rounding), 1 ulp beyond (cos_lat)."""

from __future__ import annotations

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from case_utils import compare
from test_gpu_level_pair_cache import _check, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_headline_shaped_case(gpu):
    """The benchmark's field set with three levels and 1e5 of its particles over 28 steps: the level pair changes after 24"""
    from bench import c2_case

    case = c2_case(nt=3, hi=100_000)
    case["name"] = "lean_c2"
    case["runtime"] = 28 * 3600.0
    on, stats = _check(case)
    assert stats["steps"] == 100_000 * 28
    planned, perr, _ = _run(case, -1)  # the planner picks the cache for this grid
    assert perr is None
    compare(planned, on, rtol=0.0, check_state="all", label="planned vs forced cache", skip=())


def _polar_case(dt):
    from oracle import cases

    case = cases.rect_agrid_case("lean_polar", mesh="spherical", kernels=["AdvectionRK4"], seed=17, nx=90, ny=60, nz=4, nt=4, npart=4096,
                                 runtime=12 * 3600.0, dt=dt, level_dt=6 * 3600.0)
    case["lat"] = np.linspace(-89.5, 89.5, len(case["lat"]))
    rng = np.random.default_rng(4)
    n = len(case["x"])
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)  # both hemispheres in every wavefront
    lat = rng.uniform(80.0, 85.9, n)
    far = rng.random(n) < 0.05  # ~3 lanes of a wavefront beyond 1.5 rad: the call to cos_lat runs next to the lean branch
    lat[far] = rng.uniform(86.0, 88.5, int(far.sum()))
    lat[::97] = rng.uniform(0.0, 40.0, len(lat[::97]))  # and some mid-latitude lanes
    case["y"] = sign * lat
    case["x"] = rng.uniform(60.0, 300.0, n)
    if dt < 0:
        case["t0"] = np.full(n, float(case["time_s"][-1]))
    return case, int(far.sum())


def test_high_latitudes_and_fallback(gpu):
    """80 to 85.9 degrees on both sides of the equator in one wavefront, a few lanes beyond 86 degrees (cos_lat), two level-pair changes"""
    case, nfar = _polar_case(3600.0)
    assert nfar > 50
    on, _ = _check(case)
    assert np.abs(on["y"]).max() > 86.0 and np.abs(on["y"]).min() < 45.0


def test_backward_dt(gpu):
    """The same particles backwards in time from the last level"""
    case, _ = _polar_case(-3600.0)
    on, stats = _check(case)
    assert stats["steps"] == len(case["x"]) * 12
    assert float(on["t"].max()) == float(case["time_s"][-1]) - 12 * 3600.0


def test_cells_and_level_pairs_change(gpu):
    """A flow that crosses a cell or more per half step (nearly every evaluation fetches a new block) over levels 5 h apart: three level-pair
    changes inside the run, particles leaving the domain deleted on the way"""
    from oracle import cases

    case = cases.rect_agrid_case("lean_fastflow", mesh="spherical", kernels=["AdvectionRK4", "DeleteParticle"], seed=9, nx=240, ny=120, nz=4, nt=6,
                                 npart=6000, vel=60.0, runtime=18 * 3600.0, dt=3600.0, level_dt=5 * 3600.0)
    _check(case)


def test_cos_lat_lean_on_the_device(gpu, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = str(tmp_path / "cos_lean_check")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-I",
                           os.path.join(ROOT, "parcels_amd", "csrc"), os.path.join(ROOT, "tools", "cos_lean_check.hip"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["samples"] >= 4e6
    edges, ulp, ab = out["band_edges_deg"], out["max_ulp"], out["max_abs_err_in_2^-53"]
    assert len(ulp) == len(ab) == len(edges) - 1
    for lo, u, a in zip(edges[:-1], ulp, ab):
        if lo < 85.95:
            assert a <= 4.5, (lo, a, out)  # lean region (the last such band straddles the switch at 1.5 rad)
        else:
            assert u <= 1.0, (lo, u, out)  # cos_lat
    assert r.returncode == 0, out
