#!/usr/bin/env python
"""The `miss_lanes` threshold of the transposed block fetch on the headline launch (pk_fast_agrid.h: lp_fetch_xposed; DESIGN.md §4,
profiles/c2_miss_transposed_ab.txt).

    python tools/miss_transposed_ab.py [--values 0,1,2,4,8,16,64] [--steps 24] [--rounds 3] [--reps 3] [--uv-scale 1.0] [--out FILE]

Kernel ms (HIP events around the launch) of the headline launch of bench.py from the warmed, checkpointed state, as tools/hit_path_trim_ab.py
takes it, under each value of pk_set_option("miss_lanes", v): ONE process, one FieldSet, one particle set; the values take turns inside every
round, so a drift of the clock lands on all of them.  0 is the waterfall alone (the code before the transposed fetch, in the same kernel); -1 is
the planned default.  Every value gives the same bits (tests/test_gpu_miss_transposed.py); the final x column of the first and the last value are
compared here as well.  --out appends the report to a text file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sweep(values, steps, rounds, reps, particles, uv_scale, warmup=2):
    import numpy as np
    import torch

    import parcels_amd as pa
    from bench import c2_case
    from tests.case_utils import build_fieldset, build_pset

    case = c2_case(seed=1, lo=0, hi=int(particles))
    if uv_scale != 1.0:
        case["fields"] = {k: np.ascontiguousarray(v * uv_scale) for k, v in case["fields"].items()}
    dt = case["dt"]
    fs = build_fieldset(case)
    fs.to_device(device=0)
    pset = build_pset(case, fs, sort_by_cell=True)
    kern = pa.Kernel([pa.AdvectionRK4], pset)
    eng = fs._engine_or_create()
    pset._data["dt"][:] = dt
    eng.bind_particles(pset._data)
    eng.h2d()
    eng.execute(kern.kernel_ids, endtime=warmup * dt, dt0=dt, sort_by_cell=1, t_start=0.0)
    eng.ctx.check(eng.lib.pk_particles_checkpoint(eng.ctx.handle), "pk_particles_checkpoint")

    def launch(v):
        eng.ctx.set_option("miss_lanes", v)
        eng.ctx.check(eng.lib.pk_particles_restore(eng.ctx.handle), "pk_particles_restore")
        torch.cuda.synchronize()
        st = eng.execute(kern.kernel_ids, endtime=(warmup + steps) * dt, dt0=dt, sort_by_cell=0, t_start=warmup * dt)
        torch.cuda.synchronize()
        assert int(st["steps"]) == int(particles) * steps, (st["steps"], steps)
        return float(st["kernel_ms"])

    launch(values[0])  # (one untimed launch first: clock ramp, first touch of the levels)
    ms = {v: [] for v in values}
    for _ in range(rounds):
        for v in values:
            ms[v] += [launch(v) for _ in range(reps)]
    finals = {}
    for v in (values[0], values[-1]):  # the same bits at both ends of the sweep
        launch(v)
        eng.d2h()
        finals[v] = np.array(pset._data["x"])
    same = bool(np.array_equal(finals[values[0]], finals[values[-1]], equal_nan=True))
    rows = []
    for v in values:
        k = sorted(ms[v])
        rows.append({"miss_lanes": v, "median": k[(len(k) - 1) // 2], "min": k[0], "max": k[-1], "n": len(k)})
    return {"particles": int(particles), "steps": steps, "uv_scale": uv_scale, "rows": rows, "x_equal_first_last": same}


def report(res, label):
    L = [f"## miss_lanes sweep of the headline launch ({label}; U, V x {res['uv_scale']:g}): {res['particles']} particles x {res['steps']} steps, kernel ms", "",
         "| miss_lanes | median | min | max | launches |", "|---|---|---|---|---|"]
    for r in res["rows"]:
        L.append(f"| {r['miss_lanes']} | {r['median']:.3f} | {r['min']:.3f} | {r['max']:.3f} | {r['n']} |")
    L += ["", f"final x of miss_lanes {res['rows'][0]['miss_lanes']} and {res['rows'][-1]['miss_lanes']} equal in every bit: {res['x_equal_first_last']}"]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", default="0,1,2,4,8,16,64")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--uv-scale", type=float, default=1.0)
    ap.add_argument("--label", default=os.environ.get("PARCELS_HIP_LIB", "the library of this tree"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = sweep([int(v) for v in a.values.split(",")], a.steps, a.rounds, a.reps, a.particles, a.uv_scale)
    text = report(res, a.label)
    print(text)
    print(json.dumps({"sweep": res, "label": a.label}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    if not res["x_equal_first_last"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
