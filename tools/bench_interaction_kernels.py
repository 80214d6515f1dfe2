#!/usr/bin/env python
"""Built-in interaction kernels on the device-resident columns against the same kernel as a Python function in the host loop.

    python tools/bench_interaction_kernels.py [--particles 1e5,1e6] [--repeats 5] [--steps 20] [--out profiles/interaction_kernels_bench.json]

Workload (the method of tools/bench_interaction.py): uniform points in the unit square, radius for a mean of 8 neighbours
(pi r^2 n = 8), every particle a source, float64, `--steps` iterations of [DoNothing, AttractTowards].  Two legs per size, on one box,
alternating: the device path (parcels_amd/interactkernels.py) and the same formulation as a Python kernel on pa.neighbors through the
host loop (parcels_amd/hostkernels.py) -- how the list ran before the built-in kernels existed.  The time is the host clock around
ParticleSet.execute (the one upload before and the one download after the loop included, as a user sees it).  One cold run of each leg,
then --repeats timed runs: median with min - max.  The device path's iteration is broken down by host clock around each call
(every call ends in a stream synchronise): prologue, body launch, build, count + fill + sort + finish, reduce, epilogue.
Prints one JSON line per leg and writes them all to --out.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import parcels_amd as pa  # noqa: E402
from parcels_amd import interactkernels  # noqa: E402

MEAN_NEIGHBOURS = 8.0
PHASES = ("prologue", "body", "build", "pairs", "reduce", "epilogue")


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def python_attract(radius, velocity):
    def attract(particles, fieldset):
        nb = pa.neighbors(particles, radius, sources=np.asarray(particles.attractor) != 0, include_coincident=False)
        particles.dx += nb.sum(nb.dx / nb.dist) * velocity * particles.dt
        particles.dy += nb.sum(nb.dy / nb.dist) * velocity * particles.dt

    return attract


def size_leg(fs, n, repeats, steps):
    rng = np.random.default_rng(1)
    x0, y0 = rng.random(n), rng.random(n)
    radius = float(np.sqrt(MEAN_NEIGHBOURS / (np.pi * n)))
    velocity = 0.01 * radius  # a hundredth of the radius per source and step: the neighbourhoods change slowly
    P = pa.get_default_particle(np.float64).add_variable([pa.Variable("attractor", dtype=np.bool_, initial=True)])
    lists = {"device": [pa.DoNothing, pa.AttractTowards("attractor", radius, velocity)],
             "host_loop": [pa.DoNothing, python_attract(radius, velocity)]}
    times = {k: [] for k in lists}
    phases = []
    final = {}
    for rep in range(repeats + 1):  # the first round is cold (code objects, first allocations)
        for name, kernels in lists.items():  # alternating
            pset = pa.ParticleSet(fs, pclass=P, x=x0.copy(), y=y0.copy(), t=np.zeros(n))
            interactkernels.TIMINGS = {} if name == "device" else None
            t0 = time.perf_counter()
            pset.execute(kernels, dt=1.0, runtime=float(steps))
            times[name].append((time.perf_counter() - t0) * 1e3)
            if name == "device":
                phases.append(dict(interactkernels.TIMINGS))
                interactkernels.TIMINGS = None
            assert pset._last_stats["hosted"] is (name == "host_loop")
            final[name] = (np.array(pset._data["x"]), np.array(pset._data["y"]))
            del pset
    identical = bool(np.array_equal(final["device"][0], final["host_loop"][0]) and np.array_equal(final["device"][1], final["host_loop"][1]))
    dev, host = times["device"][1:], times["host_loop"][1:]
    leg = {"leg": "attract", "n": n, "radius": radius, "steps": steps, "repeats": repeats, "identical_positions": identical,
           "device": dict(stats(dev), cold_ms=round(times["device"][0], 3), runs_ms=[round(v, 3) for v in dev]),
           "host_loop": dict(stats(host), cold_ms=round(times["host_loop"][0], 3), runs_ms=[round(v, 3) for v in host]),
           "ratio_of_medians": round(statistics.median(host) / statistics.median(dev), 2),
           "every_device_run_below_every_host_run": bool(max(dev) < min(host)),
           "device_ms_per_iteration": {k: round(statistics.median([ph.get(k, 0.0) for ph in phases[1:]]) * 1e3 / steps, 4) for k in PHASES}}
    return leg


def main():
    from case_utils import build_fieldset, load_golden

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1e5,1e6")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interaction_kernels_bench.json"))
    a = ap.parse_args()
    case, _, _ = load_golden("agrid_flat_rk4_f64")  # any fieldset: no kernel of the list samples a field
    fs = build_fieldset(case)
    dev = fs._engine_or_create().ctx.device_info()
    legs = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in [int(float(s)) for s in a.particles.split(",") if s]:
        legs.append(size_leg(fs, n, a.repeats, a.steps))
        print(json.dumps(legs[-1]), flush=True)
        res = {"device": dev["name"], "arch": dev["arch"],
               "workload": "uniform points in the unit square, pi r^2 n = 8, every particle a source, float64, [DoNothing, AttractTowards]",
               "timing": "host clock around ParticleSet.execute; legs alternate on one box; one cold run, then the median of the timed runs with "
                         "min / max; device_ms_per_iteration: host clock around each call of the device loop (each ends in a stream synchronise)",
               "legs": legs}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
