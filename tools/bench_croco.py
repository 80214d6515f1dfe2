#!/usr/bin/env python
"""Throughput of the CROCO sigma-grid kernels (csrc/pk_sigma.h).

    python tools/bench_croco.py [--particles 1e6,1e7] [--repeats 5] [--steps 50] [--host-particles 1e5] [--out profiles/croco_bench.json]

Workload: a 512 x 512 x 33-level float32 CROCO fieldset with 4 time levels (tools/make_croco_golden.py: croco_output, built through
convert.croco_to_sgrid + FieldSet.from_sgrid_conventions), float64 particles, 50 steps of [AdvectionRK2_3D_CROCO, SampleOmegaCroco] per
launch: one cold launch, then the median of the timed ones with min / max, particle-steps per second and kernel milliseconds.  Beside it,
for scale: AdvectionRK2_3D on the same fieldset (2 field evaluations per step against 13 + 3; the particles' z is then a sigma level), the
documented recipe as a Python kernel on the host path at --host-particles, and the registers / scratch / LDS of the kernel from
tools/kernel_resources.sh (compile-only: VGPRs, scratch, waves per SIMD; the dynamic LDS is 16 bytes per sigma level).  Prints one JSON line per leg and writes them all to --out.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1e6,1e7")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--host-particles", default="1e5")
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fs, coords, fields = fieldset()
    legs = []

    def emit(leg):
        legs.append(leg)
        print(json.dumps(leg), flush=True)

    for n in [int(float(v)) for v in a.particles.split(",") if v]:
        x, y, z = particles(coords, fields, n)
        emit({"leg": "croco_rk2_3d_sample_omega", **timed(fs, [pa.AdvectionRK2_3D_CROCO, pa.SampleOmegaCroco], x, y, z, a.steps, a.repeats, ("omega",))})
        x, y, z = particles(coords, fields, n, sigma_z=True)
        emit({"leg": "advection_rk2_3d_same_fieldset", **timed(fs, [pa.AdvectionRK2_3D], x, y, z, a.steps, a.repeats)})
    nh = int(float(a.host_particles))
    if nh > 0:
        x, y, z = particles(coords, fields, nh)
        t0 = time.perf_counter()
        pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("omega", dtype=np.float64, initial=0))
        pset = pa.ParticleSet(fs, pclass=pclass, x=x, y=y, z=z, t=np.zeros(nh))
        pset.execute([host_recipe], dt=DT, runtime=a.host_steps * DT)
        wall = time.perf_counter() - t0
        emit({"leg": "host_path_recipe_sample_omega", "particles": nh, "steps": a.host_steps, "wall_s": wall,
              "particle_steps_per_s": nh * a.host_steps / wall})
    if not a.no_resources:
        emit({"leg": "kernel_resources", "lds_bytes_per_workgroup": 16 * 33, "kernels": kernel_resources()})
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": "python " + " ".join(["tools/bench_croco.py"] + sys.argv[1:]), "legs": legs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
