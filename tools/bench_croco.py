#!/usr/bin/env python
"""Throughput of the CROCO sigma-grid kernels (csrc/pk_sigma.h).

    python tools/bench_croco.py [--particles 1e6,1e7] [--repeats 5] [--steps 50] [--host-particles 1e5] [--legs a,b,..] [--out profiles/croco_bench.json]

Workload: a 512 x 512 x 33-level float32 CROCO fieldset with 4 time levels (tools/make_croco_golden.py: croco_output, built through
convert.croco_to_sgrid + FieldSet.from_sgrid_conventions), float64 particles, 50 steps of [AdvectionRK2_3D_CROCO, SampleOmegaCroco] per
launch: one cold launch, then the median of the timed ones with min / max, particle-steps per second and kernel milliseconds.  Beside it,
for scale: AdvectionRK2_3D on the same fieldset (2 field evaluations per step against 13 + 3; the particles' z is then a sigma level), the
documented recipe as a Python kernel on the host path at --host-particles, and the registers / scratch / LDS of the kernel from
tools/kernel_resources.sh (compile-only: VGPRs, scratch, waves per SIMD; the dynamic LDS is 16 bytes per sigma level).  Prints one JSON line per leg and writes them all to --out.

Python kernels in the list (parcels_amd/jit.py compiles them into the sigma loop): croco_rk2_3d_python_delete is the list of the reference's
CROCO tutorial, [AdvectionRK2_3D_CROCO, DeleteParticle] with its two-line Python DeleteParticle; croco_rk2_3d_python_recipe is the documented
sampling recipe as a Python function next to AdvectionRK2_3D_CROCO, the twin of croco_rk2_3d_sample_omega (both also at --host-particles,
to stand beside the host-path legs); host_path_python_delete is the tutorial's list with PARCELS_AMD_JIT=0.  --legs picks legs by name;
PARCELS_HIP_LIB runs the built-in and host-path legs on another build of the library (A/B against a parent commit).
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
from tools import make_croco_golden as mg  # noqa: E402

DT = 60.0


def fieldset():
    coords, fields = mg.croco_output(nx=512, ny=512, nw=33, nt=4, dtype=np.float32, tstep=4000.0)
    two = {"x_rho": (("xi_rho",), coords["x_rho"]), "y_rho": (("eta_rho",), coords["y_rho"]), "s_w": (("s_w",), coords["s_w"]),
           "time": (("time",), coords["time"])}
    use = ("u", "v", "w", "omega", "h", "zeta", "Cs_w")
    ds = pa.convert.croco_to_sgrid(fields={mg.FIELD_NAMES.get(k, k): (mg.CROCO_DIMS[k], fields[k]) for k in use}, coords=two)
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="flat")
    fs.add_context("hc", 20.0)
    return fs, coords, fields


def particles(coords, fields, n, sigma_z=False, seed=1):
    x, y, z = mg.interior_particles(coords, fields, n, seed)
    if sigma_z:
        z = np.random.default_rng(seed).uniform(-0.9, -0.1, n)
    return x, y, z


def timed(fs, kernels, x, y, z, steps, repeats, variables=()):
    pclass = pa.get_default_particle(np.float64)
    for v in variables:
        pclass = pclass.add_variable(pa.Variable(v, dtype=np.float64, initial=0))
    res = []
    for rep in range(repeats + 1):  # the first launch is cold (module load, descriptor upload)
        pset = pa.ParticleSet(fs, pclass=pclass, x=x, y=y, z=z, t=np.zeros(x.size))
        t0 = time.perf_counter()
        pset.execute(kernels, dt=DT, runtime=steps * DT)
        wall = time.perf_counter() - t0
        st = pset._last_stats
        res.append({"wall_s": wall, "kernel_ms": float(st.get("kernel_ms", 0.0)), "steps": int(st.get("steps", 0)), "program": st.get("program")})
        if any(pa.kernels.kernel_id(k) is None for k in kernels) and (st.get("hosted") or pset._kernel.user_program is None):
            raise RuntimeError(f"the Python kernels of the list were not compiled: {pset._kernel.jit_report}")
    cold, warm = res[0], res[1:]
    km = sorted(r["kernel_ms"] for r in warm)
    med = km[len(km) // 2]
    steps_done = warm[0]["steps"]
    return {"particles": int(x.size), "steps_per_launch": steps, "particle_steps": steps_done, "program": warm[0]["program"],
            "cold_kernel_ms": cold["kernel_ms"], "kernel_ms": {"median": med, "min": km[0], "max": km[-1]},
            "particle_steps_per_s": {"median": steps_done / (med * 1e-3) if med > 0 else None,
                                     "min": steps_done / (km[-1] * 1e-3) if km[-1] > 0 else None,
                                     "max": steps_done / (km[0] * 1e-3) if km[0] > 0 else None},
            "wall_s_median": sorted(r["wall_s"] for r in warm)[len(warm) // 2]}


def kernel_resources():
    try:
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "pk_prog_sigma.hip"],
                             capture_output=True, text=True, timeout=900).stdout
    except Exception as e:  # hipcc missing: no resource report
        return f"unavailable: {e}"
    return [l.strip() for l in out.splitlines() if "advect_sigma_kernel" in l]


def host_recipe(particles, fieldset):
    sigma = pa.convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
    particles.omega = fieldset.omega[particles.t, sigma, particles.y, particles.x, particles]


def DeleteParticle(particles, fieldset):  # noqa: N802 -- docs/user_guide/examples/tutorial_croco_3D.ipynb
    any_error = particles.state >= 50
    particles[any_error].state = pa.StatusCode.Delete


def hosted(fs, kernels, x, y, z, steps, variables=()):
    """the list on the host path (PARCELS_AMD_JIT=0): one run, wall time"""
    pclass = pa.get_default_particle(np.float64)
    for v in variables:
        pclass = pclass.add_variable(pa.Variable(v, dtype=np.float64, initial=0))
    before = os.environ.get("PARCELS_AMD_JIT")
    os.environ["PARCELS_AMD_JIT"] = "0"
    try:
        t0 = time.perf_counter()
        pset = pa.ParticleSet(fs, pclass=pclass, x=x, y=y, z=z, t=np.zeros(x.size))
        t1 = time.perf_counter()
        pset.execute(kernels, dt=DT, runtime=steps * DT)
        wall, execute_wall = time.perf_counter() - t0, time.perf_counter() - t1
    finally:
        if before is None:
            del os.environ["PARCELS_AMD_JIT"]
        else:
            os.environ["PARCELS_AMD_JIT"] = before
    if not pset._last_stats.get("hosted"):
        raise RuntimeError("the list did not run on the host path")
    # (wall_s includes the construction of the ParticleSet, as the leg always did; execute_wall_s is what `wall_s_median` of a timed leg is)
    return {"particles": int(x.size), "steps": steps, "wall_s": wall, "execute_wall_s": execute_wall, "particle_steps_per_s": x.size * steps / wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1e6,1e7")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--host-particles", default="1e5")
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--legs", default="", help="comma-separated leg names (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fs, coords, fields = fieldset()
    legs = []

    only = {v for v in a.legs.split(",") if v}

    def want(name):
        return not only or name in only

    def emit(leg):
        legs.append(leg)
        print(json.dumps(leg), flush=True)

    nh = int(float(a.host_particles))
    sizes = [int(float(v)) for v in a.particles.split(",") if v]
    for n in sizes:
        x, y, z = particles(coords, fields, n)
        if want("croco_rk2_3d_sample_omega"):
            emit({"leg": "croco_rk2_3d_sample_omega", **timed(fs, [pa.AdvectionRK2_3D_CROCO, pa.SampleOmegaCroco], x, y, z, a.steps, a.repeats, ("omega",))})
        if want("advection_rk2_3d_same_fieldset"):
            xs, ys, zs = particles(coords, fields, n, sigma_z=True)
            emit({"leg": "advection_rk2_3d_same_fieldset", **timed(fs, [pa.AdvectionRK2_3D], xs, ys, zs, a.steps, a.repeats)})
    for n in sizes + ([nh] if nh > 0 and nh not in sizes else []):  # (the Python lists also at the size of the host-path legs)
        x, y, z = particles(coords, fields, n)
        if want("croco_rk2_3d_python_delete"):
            emit({"leg": "croco_rk2_3d_python_delete", **timed(fs, [pa.AdvectionRK2_3D_CROCO, DeleteParticle], x, y, z, a.steps, a.repeats)})
        if want("croco_rk2_3d_python_recipe"):
            emit({"leg": "croco_rk2_3d_python_recipe", **timed(fs, [pa.AdvectionRK2_3D_CROCO, host_recipe], x, y, z, a.steps, a.repeats, ("omega",))})
    if nh > 0:
        x, y, z = particles(coords, fields, nh)
        if want("host_path_recipe_sample_omega"):
            emit({"leg": "host_path_recipe_sample_omega", **hosted(fs, [host_recipe], x, y, z, a.host_steps, ("omega",))})
        if want("host_path_python_delete"):
            emit({"leg": "host_path_python_delete", **hosted(fs, [pa.AdvectionRK2_3D_CROCO, DeleteParticle], x, y, z, a.host_steps)})
    if not a.no_resources and want("kernel_resources"):
        emit({"leg": "kernel_resources", "lds_bytes_per_workgroup": 16 * 33, "kernels": kernel_resources()})
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": "python " + " ".join(["tools/bench_croco.py"] + sys.argv[1:]), "legs": legs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
