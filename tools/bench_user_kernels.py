#!/usr/bin/env python
"""What a user-written kernel costs: BASELINE config 2 (360 x 180 x 50 x 24 A-grid, fp64, 1e7 particles, AdvectionRK4, 24 steps) with the
two kernels every Parcels tutorial adds -- an ageing kernel and a delete-when-old kernel -- (a) compiled into the fused launch
(parcels_amd/jit.py), (b) on the host path (PARCELS_AMD_JIT=0: the reference's loop on the host columns, the built-in kernel's body on the
GPU), next to (c) AdvectionRK4 alone.  Prints one JSON object.

`bench_user_kernels.py wind [particles] [repeats]`: a kernel that samples a NAMED vector field instead -- [AdvectionRK4, WindMidpoint] (the
midpoint wind kernel of tests/named_vector_kernels.py) on the same A-grid with 1e6 float64 particles, the wind from a second dataset on a
90 x 45 2-D grid added with `fs + fs_wind`, 24 steps -- compiled and with PARCELS_AMD_JIT=0, particle-steps/s as the median over repeated
runs (a fresh ParticleSet each, after one warm-up run that compiles, loads and sorts).

`bench_user_kernels.py random [particles] [repeats]`: stochastic user kernels -- [AdvectionRK4, RandomWalk, Mortality] drawing from
`pa.random` (parcels_amd/random.py) -- at the sizes of the wind mode, compiled and with PARCELS_AMD_JIT=0, next to [AdvectionRK4] alone."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parcels_amd import StatusCode  # noqa: E402
from parcels_amd import random as pa_random  # noqa: E402


def Age(particles, fieldset):
    particles.age += particles.dt


def DeleteOld(particles, fieldset):
    particles.state = np.where(particles.age > fieldset.max_age, StatusCode.Delete, particles.state)


def SampleT(particles, fieldset):
    particles.temp = fieldset.T[particles]


def run(kernels, jit, n, steps):
    import parcels_amd as pa
    try:
        from __main__ import c2_case  # (called from bench.py itself)
    except ImportError:
        from bench import c2_case
    from case_utils import build_fieldset

    os.environ["PARCELS_AMD_JIT"] = "1" if jit else "0"
    case = c2_case(seed=1, lo=0, hi=n)
    case["fields"] = dict(case["fields"])
    case["field_dims"] = dict(case["field_dims"])
    case["fields"]["T"] = np.asarray(case["fields"]["U"]) * 3.0 + 10.0  # a tracer on the velocity grid
    case["field_dims"]["T"] = case["field_dims"]["U"]
    fs = build_fieldset(case)
    fs.add_context("max_age", 20 * 3600.0)
    P = pa.get_default_particle(np.float64).add_variable([pa.Variable("age", dtype=np.float32, initial=0), pa.Variable("temp", dtype=np.float32, initial=0)])
    pset = pa.ParticleSet(fs, pclass=P, x=case["x"], y=case["y"], z=case["z"], sort_by_cell=True)
    dt = float(case["dt"])
    pset.execute(kernels, runtime=2 * dt, dt=dt)  # warm-up: compile / load, cell sort
    t0 = time.perf_counter()
    pset.execute(kernels, runtime=steps * dt, dt=dt)
    wall = time.perf_counter() - t0
    st = pset._last_stats or {}
    return {"wall_s": wall, "steps_per_s_wall": n * steps / wall, "kernel_ms": st.get("kernel_ms"), "launches": st.get("launches"),
            "hosted": bool(st.get("hosted")), "program": st.get("program"), "remaining": len(pset), "jit_report": pset._kernel.jit_report,
            "temp_sum": float(np.sum(pset._data["temp"], dtype=np.float64))}


def RandomWalk(particles, fieldset):
    particles.dx += pa_random.normal(0.0, fieldset.sigma, particles)
    particles.dy += pa_random.normal(0.0, fieldset.sigma, particles)


def Mortality(particles, fieldset):
    particles.state = np.where(pa_random.random(particles) < fieldset.p_die, StatusCode.Delete, particles.state)


def run_random(kernels, jit, n, steps, repeats):
    import parcels_amd as pa
    try:
        from __main__ import c2_case, c2_positions
    except ImportError:
        from bench import c2_case, c2_positions
    from case_utils import build_fieldset

    os.environ["PARCELS_AMD_JIT"] = "1" if jit else "0"
    case = c2_case(seed=1, lo=0, hi=1)
    fs = build_fieldset(case)
    fs.add_context("sigma", 1.0e-3)  # degrees per step
    fs.add_context("p_die", 1.0e-3)  # per step: about 2.4 % of the particles die in 24 steps
    x, y, z = c2_positions(1, 0, n)
    dt = float(case["dt"])
    walls, kms, pset = [], [], None
    for k in range(repeats + 1):  # (run 0 warms up)
        pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x, y=y, z=z, seed=1, sort_by_cell=True)
        t0 = time.perf_counter()
        pset.execute(kernels, runtime=steps * dt, dt=dt)
        if k:
            walls.append(time.perf_counter() - t0)
            kms.append((pset._last_stats or {}).get("kernel_ms"))
    st = pset._last_stats or {}
    wall = float(np.median(walls))
    return {"wall_s_median": wall, "wall_s_all": walls, "steps_per_s_wall": n * steps / wall, "kernel_ms_all": kms, "launches": st.get("launches"),
            "hosted": bool(st.get("hosted")), "program": st.get("program"), "jit_report": pset._kernel.jit_report, "remaining": len(pset),
            "x_sum": float(np.sum(pset._data["x"], dtype=np.float64))}


def wind_fieldset():
    import parcels_amd as pa
    try:
        from __main__ import c2_case
    except ImportError:
        from bench import c2_case
    from case_utils import build_fieldset

    case = c2_case(seed=1, lo=0, hi=1)
    lon, lat, ts = np.asarray(case["lon"], dtype=np.float64), np.asarray(case["lat"], dtype=np.float64), np.asarray(case["time_s"], dtype=np.float64)
    rng = np.random.default_rng(5)
    nt = 9
    md = pa.SGrid2DMetadata(node_dimensions=("XG", "YG"), node_coordinates=("lon", "lat"),
                            face_dimensions=(pa.FaceNodePadding("XC", "XG", pa.Padding.LOW), pa.FaceNodePadding("YC", "YG", pa.Padding.LOW)),
                            vertical_dimensions=None)
    coords = {"lon": (("XG",), np.linspace(lon[0], lon[-1], 90)), "lat": (("YG",), np.linspace(lat[0], lat[-1], 45)),
              "time": (("time",), np.linspace(ts[0], ts[-1], nt))}
    dims = ("time", "YG", "XG")
    data = {"UWind": (dims, 8.0 * rng.standard_normal((nt, 45, 90))), "VWind": (dims, 8.0 * rng.standard_normal((nt, 45, 90)))}
    fs = build_fieldset(case) + pa.FieldSet.from_sgrid_conventions(pa.Dataset(data, coords, sgrid=md), mesh=case["mesh"],
                                                                   vector_fields={"Wind": ("UWind", "VWind")})
    fs.add_context("windage", 0.02)
    return fs, case


def run_wind(jit, n, steps, repeats):
    import parcels_amd as pa
    try:
        from __main__ import c2_positions
    except ImportError:
        from bench import c2_positions
    from named_vector_kernels import WindMidpoint

    os.environ["PARCELS_AMD_JIT"] = "1" if jit else "0"
    fs, case = wind_fieldset()
    case["x"], case["y"], case["z"] = c2_positions(1, 0, n)
    dt = float(case["dt"])
    kernels = [pa.AdvectionRK4, WindMidpoint]
    walls, kms, pset = [], [], None
    for k in range(repeats + 1):  # (run 0 warms up)
        pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=case["x"], y=case["y"], z=case["z"], sort_by_cell=True)
        t0 = time.perf_counter()
        pset.execute(kernels, runtime=steps * dt, dt=dt)
        if k:
            walls.append(time.perf_counter() - t0)
            kms.append((pset._last_stats or {}).get("kernel_ms"))
    st = pset._last_stats or {}
    wall = float(np.median(walls))
    return {"wall_s_median": wall, "wall_s_all": walls, "steps_per_s_wall": n * steps / wall, "kernel_ms_all": kms, "launches": st.get("launches"),
            "hosted": bool(st.get("hosted")), "program": st.get("program"), "jit_report": pset._kernel.jit_report,
            "x_sum": float(np.sum(pset._data["x"], dtype=np.float64))}


if __name__ == "__main__":
    import parcels_amd as pa

    if len(sys.argv) > 1 and sys.argv[1] == "wind":
        n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
        repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
        out = {"particles": n, "steps": 24, "repeats": repeats, "rk4_wind_compiled": run_wind(True, n, 24, repeats),
               "rk4_wind_host_path": run_wind(False, n, 24, repeats)}
        out["compiled_over_host_path"] = out["rk4_wind_compiled"]["steps_per_s_wall"] / out["rk4_wind_host_path"]["steps_per_s_wall"]
        print(json.dumps(out))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "random":
        n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
        repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
        stochastic = [pa.AdvectionRK4, RandomWalk, Mortality]
        out = {"particles": n, "steps": 24, "repeats": repeats, "rk4_alone": run_random([pa.AdvectionRK4], True, n, 24, repeats),
               "rk4_walk_mortality_compiled": run_random(stochastic, True, n, 24, repeats),
               "rk4_walk_mortality_host_path": run_random(stochastic, False, n, 24, repeats)}
        out["compiled_over_host_path"] = out["rk4_walk_mortality_compiled"]["steps_per_s_wall"] / out["rk4_walk_mortality_host_path"]["steps_per_s_wall"]
        out["compiled_over_rk4_alone"] = out["rk4_walk_mortality_compiled"]["steps_per_s_wall"] / out["rk4_alone"]["steps_per_s_wall"]
        print(json.dumps(out))
        sys.exit(0)
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    steps = 24
    out = {"particles": n, "steps": steps,
           "rk4_alone": run([pa.AdvectionRK4], True, n, steps),
           "rk4_age_delete_compiled": run([pa.AdvectionRK4, Age, DeleteOld], True, n, steps),
           "rk4_age_delete_host_path": run([pa.AdvectionRK4, Age, DeleteOld], False, n, steps),
           "rk4_sample_compiled": run([pa.AdvectionRK4, SampleT], True, n, steps),
           "rk4_sample_host_path": run([pa.AdvectionRK4, SampleT], False, max(n // 5, 1), steps)}
    if os.environ.get("PARCELS_AMD_JIT_FAST_WAVES_AB"):
        for w in os.environ["PARCELS_AMD_JIT_FAST_WAVES_AB"].split(","):
            os.environ["PARCELS_AMD_JIT_FAST_WAVES"] = w
            out["rk4_sample_compiled_waves" + w] = run([pa.AdvectionRK4, SampleT], True, n, steps)
    print(json.dumps(out))
