#!/usr/bin/env python
"""Throughput of AdvectionRK4 on an unstructured triangle mesh (UxGrid, csrc/pk_ux.h).

    python tools/bench_ux.py [--particles 1e7] [--repeats 5] [--meshes flat,spherical] [--legs rk4,m1,user,user_host]

Legs: rk4 (the default, described below); m1 = AdvectionDiffusionM1 with face-registered Kh_zonal / Kh_meridional; user = the list
[AdvectionRK4, Age, SampleT] with the two Python kernels compiled into the step loop (parcels_amd/jit.py); user_host = the same list with
PARCELS_AMD_JIT=0, i.e. the host loop.  The user legs also report wall seconds per execute(): the host loop has no single kernel time.

Workload: a 2-D face-registered mesh of ~1e6 triangles (a jittered 708 x 708 lattice split into two triangles per quad), flat and
spherical, 24 time levels resident on the device, 1e7 float64 particles, AdvectionRK4 for 24 steps per launch.  Prints one JSON line per
mesh: median / min / max particle-steps per second over the repeated launches and the kernel milliseconds, plus the register / scratch /
occupancy of the UxGrid kernel from tools/kernel_resources.sh (compile-only, no GPU needed for that part).
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import parcels_amd as pa  # noqa: E402
from tools.make_ux_golden import face_centres, lattice_mesh  # noqa: E402

NLEVELS = 24
STEPS = 24


def Age(particles, fieldset):  # noqa: N802
    particles.age += particles.dt
    particles.state = np.where(particles.age > fieldset.max_age, pa.StatusCode.Delete, particles.state)


def SampleT(particles, fieldset):  # noqa: N802
    particles.temp = fieldset.T[particles]


def fieldset(spherical: bool, leg: str = "rk4"):
    if spherical:
        # (no interior point where the mesh's unit-sphere x, y or z peaks: the reference's hash boxes span the faces' NODES, so a point
        # nearer such a peak than every node quantises above every box but one and is not found -- GridSearchingError, uxgrid.py:113-133)
        lon, lat, faces = lattice_mesh(708, 708, 5.0, 85.0, 5.0, 60.0, jitter=0.3, seed=11)
        u0, v0 = 0.5, 0.2  # m/s
    else:
        lon, lat, faces = lattice_mesh(708, 708, 0.0, 70.7, 0.0, 70.7, jitter=0.3, seed=11)
        u0, v0 = 2e-5, 1e-5  # mesh units / s
    fx, fy = face_centres(lon, lat, faces)
    k = np.arange(NLEVELS)[:, None]
    U = (u0 * (1.0 + 0.3 * np.sin(fy[None, :] / 5.0 + k / 4.0)))[:, None, :]
    V = (v0 * np.cos(fx[None, :] / 7.0 - k / 5.0))[:, None, :]
    data = {"U": (("time", "zc", "n_face"), U), "V": (("time", "zc", "n_face"), V)}
    one = np.ones((NLEVELS, 1, 1))
    if leg == "m1":  # diffusive steps of ~1e-2 of a face per step; m^2/s on the sphere, mesh units^2/s on the plane
        k0 = 50.0 if spherical else 1e-9
        data["Kh_zonal"] = (("time", "zc", "n_face"), one * (k0 * (1.0 + 0.2 * np.sin(fx / 3.0)))[None, None, :])
        data["Kh_meridional"] = (("time", "zc", "n_face"), one * (k0 * (1.0 + 0.2 * np.cos(fy / 4.0)))[None, None, :])
    if leg.startswith("user"):
        data["T"] = (("time", "zc", "n_face"), one * (10.0 + np.sin(fx / 3.0) + 0.1 * fy)[None, None, :])
    ds = pa.Dataset(data,
                    {"time": (("time",), np.arange(NLEVELS) * 86400.0), "zf": (("zf",), np.array([0.0, 1.0])), "zc": (("zc",), np.array([0.5]))},
                    uxgrid=pa.UxMesh(lon, lat, faces))
    fs = pa.FieldSet.from_ugrid_conventions(ds, mesh="spherical" if spherical else "flat")
    if leg == "m1":
        fs.add_context("dres", 0.05)  # about half a face
    if leg.startswith("user"):
        fs.add_context("max_age", 1e30)
    return fs, faces.shape[0], (lon.min(), lon.max(), lat.min(), lat.max())


def kernel_resources():
    try:
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "pk_prog_ux.hip"],
                             capture_output=True, text=True, timeout=600).stdout
    except Exception as e:  # hipcc missing: no resource report
        return f"unavailable: {e}"
    return [l.strip() for l in out.splitlines() if "advect_ux_kernel" in l]


def run(spherical: bool, n: int, repeats: int, dt: float, leg: str = "rk4"):
    t0 = time.time()
    os.environ["PARCELS_AMD_JIT"] = "0" if leg == "user_host" else "1"
    fs, nf, (x0, x1, y0, y1) = fieldset(spherical, leg)
    rng = np.random.default_rng(7)
    wx, wy = x1 - x0, y1 - y0
    x = rng.uniform(x0 + 0.1 * wx, x1 - 0.1 * wx, n)
    y = rng.uniform(y0 + 0.1 * wy, y1 - 0.1 * wy, n)
    pclass = pa.get_default_particle(np.float64)
    kernels = {"rk4": [pa.AdvectionRK4], "m1": [pa.AdvectionDiffusionM1]}.get(leg, [pa.AdvectionRK4, Age, SampleT])
    if leg.startswith("user"):
        pclass = pclass.add_variable([pa.Variable("age", dtype=np.float32, initial=0), pa.Variable("temp", dtype=np.float32, initial=0)])
    pset = pa.ParticleSet(fs, pclass=pclass, x=x, y=y, z=np.full(n, 0.5), t=np.zeros(n))
    setup_s = time.time() - t0
    rates, kms, walls = [], [], []
    for r in range(repeats + 1):  # the first launch also builds the device copy (and compiles the user module): not timed
        w0 = time.time()
        pset.execute(kernels, dt=dt, runtime=STEPS * dt)
        wall = time.time() - w0
        st = pset._last_stats
        if r == 0:
            continue
        walls.append(wall)
        kms.append(float(st["kernel_ms"]))
        if float(st["kernel_ms"]) > 0:  # (the host loop reports no single kernel time: its rate is the wall one)
            rates.append(float(st["steps"]) / (float(st["kernel_ms"]) / 1e3))
    states = np.bincount(np.asarray(pset._data["state"]).ravel(), minlength=80)
    extra = {"leg": leg, "kernels": [k.__name__ for k in kernels], "jit_report": str(pset._kernel.jit_report)[:60] if leg.startswith("user") else None,
             "wall_s": {"median": float(np.median(walls)), "min": float(np.min(walls)), "max": float(np.max(walls))},
             "particle_steps_per_s_wall": float(n * STEPS / np.median(walls))}
    return {**extra, "mesh": "spherical" if spherical else "flat", "n_face": int(nf), "particles": n, "levels_resident": NLEVELS, "steps_per_launch": STEPS,
            "launches": repeats, "particle_steps_per_s": {"median": float(np.median(rates)), "min": float(np.min(rates)), "max": float(np.max(rates))} if rates else None,
            "kernel_ms": {"median": float(np.median(kms)), "min": float(np.min(kms)), "max": float(np.max(kms))},
            "program": int(st.get("program", -1)), "states": {int(k): int(v) for k, v in enumerate(states) if v},
            "floor_1e9": bool(rates and np.median(rates) >= 1e9), "setup_s": round(setup_s, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--meshes", default="flat,spherical")
    ap.add_argument("--dt", type=float, default=600.0)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--legs", default="rk4", help="comma-separated: rk4, m1, user, user_host")
    a = ap.parse_args()
    res = None if a.no_resources else kernel_resources()
    for leg in a.legs.split(","):
        for m in a.meshes.split(","):
            out = run(m == "spherical", int(a.particles), a.repeats, a.dt, leg)
            out["kernel_resources"] = res
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
