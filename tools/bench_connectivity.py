#!/usr/bin/env python
"""ParticleSet.connectivity (csrc/pk_connectivity.hip) beside what a script does today, on one GPU.

    python tools/bench_connectivity.py [--out profiles/connectivity_bench.json] [--legs cells,regions] [--processes 2] [--repeats 5]

Every leg is measured in `--processes` fresh processes run one after the other; in a process the first call of everything is untimed and
`--repeats` calls are timed, the device call and the host route alternating in the same process.  A cell of the result is the median with
min - max over all timed calls of all processes.  Times are host clocks around calls that end in a device synchronise (the result is
downloaded); the kernel split (key / sort / encode, HIP events) comes from pk_connectivity_info_t.

Workload: 1e7 float64 particles on the C2-size rectilinear grid (360 x 180 x 50 nodes, spherical: 359 x 179 cells), released uniformly, their
cell recorded with ParticleSet.cells in an int32 Variable, then displaced by up to three cells and made resident by one DoNothing step.
Legs:
  cells    cell-to-cell, sparse=True: 64261 origins x 64261 destinations, the sort + run-length-encode path
  regions  a map of 64 regions (8 x 8 blocks of cells), origins relabelled with it: a dense 64 x 64 matrix, the LDS histogram path
`today` beside each: read pset.x / pset.y through the mirror (two columns come down and are marked dirty), pk_search on them, then
np.unique(origin * n_dest + dest, return_counts=True) (cells) or np.bincount of the same keys (regions); and the execute() that follows
either route (one DoNothing step): after the host route it uploads the two columns again.
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

N = 10_000_000
LEGS = ("cells", "regions")


def worker(leg, n, repeats):
    """one process: the timed calls of one leg; one JSON line"""
    import parcels_amd as pa
    from parcels_amd.engine import density_shape
    from tools.bench_density import _rect_fieldset

    rng = np.random.default_rng(7)
    fs = _rect_fieldset(np.linspace(0.0, 360.0, 360), np.linspace(-80.0, 80.0, 180), np.linspace(0.0, 5000.0, 50))
    ny, nx = density_shape(fs.U.grid, False)  # 179 x 359 cells
    x0, y0 = rng.uniform(5.0, 355.0, n), rng.uniform(-75.0, 75.0, n)
    pclass = pa.get_default_particle(np.float64).add_variable(pa.Variable("src", dtype=np.int32, initial=-1))
    pset = pa.ParticleSet(fs, pclass=pclass, x=x0, y=y0, z=np.full(n, 10.0), t=np.zeros(n))
    regions = None
    if leg == "regions":
        regions = ((np.arange(ny) * 8 // ny)[:, None] * 8 + (np.arange(nx) * 8 // nx)[None, :]).astype(np.int32)
    pset.src = pset.cells(regions=regions)  # where every particle is released
    pset.x = np.clip(x0 + rng.uniform(-3.0, 3.0, n), 0.5, 359.5)
    pset.y = np.clip(y0 + rng.uniform(-2.7, 2.7, n), -79.5, 79.5)
    n_dest = 64 if leg == "regions" else ny * nx
    sparse = leg == "cells"

    def step():
        t0 = time.perf_counter()
        pset.execute([pa.DoNothing], dt=60.0, runtime=60.0)
        return (time.perf_counter() - t0) * 1e3

    step()
    eng = fs._engine
    out = {"leg": leg, "particles": n, "n_origin": n_dest, "n_dest": n_dest, "device_ms": [], "device_key_ms": [], "device_sort_ms": [], "device_encode_ms": [],
           "device_exec_after_ms": [], "today_ms": [], "today_read_ms": [], "today_search_ms": [], "today_count_ms": [], "today_exec_after_ms": []}
    matches = True
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        got = pset.connectivity("src", regions=regions, sparse=sparse)
        dt_dev = (time.perf_counter() - t0) * 1e3
        info = dict(pset._last_connectivity_info)
        after = step()
        if r:
            out["device_ms"].append(dt_dev)
            for k in ("key", "sort", "encode"):
                out[f"device_{k}_ms"].append(info[f"{k}_ms"])
            out["device_exec_after_ms"].append(after)
        t0 = time.perf_counter()
        xs, ys = pset.x, pset.y
        t1 = time.perf_counter()
        ei = eng.search(0, np.zeros(n), ys, xs)
        t2 = time.perf_counter()
        src = np.asarray(pset.src, dtype=np.int64)
        ok = (ei >= 0) & (src >= 0)
        cell = ei[ok] % (ny * nx)
        dest = cell.astype(np.int64) if regions is None else regions.ravel()[cell].astype(np.int64)
        key = src[ok] * n_dest + dest
        if sparse:
            keys, counts = np.unique(key, return_counts=True)
            today = (*np.divmod(keys, n_dest), counts)
        else:
            today = np.bincount(key, minlength=n_dest * n_dest).reshape(n_dest, n_dest)
        t3 = time.perf_counter()
        del xs, ys
        after = step()
        if r:
            out["today_ms"].append((t3 - t0) * 1e3)
            out["today_read_ms"].append((t1 - t0) * 1e3)
            out["today_search_ms"].append((t2 - t1) * 1e3)
            out["today_count_ms"].append((t3 - t2) * 1e3)
            out["today_exec_after_ms"].append(after)
        same = all(np.array_equal(a, b) for a, b in zip(got, today)) if sparse else np.array_equal(got, today)
        matches = matches and bool(same)
    out.update(path=info["path"], pairs=int(info["n_pairs"]), tracked=int(info["n_tracked"]), outside=int(info["n_outside"]), atomics=int(info["n_atomics"]),
               matches_today=matches)
    print("RESULT " + json.dumps(out), flush=True)


def _cell(values):
    v = np.asarray(values, dtype=np.float64)
    return None if v.size == 0 else {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connectivity_bench.json"))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the particle count (rehearsals)")
    ap.add_argument("--worker", metavar="LEG")
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds per process")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, max(int(N * a.scale), 1), a.repeats)
        return
    results = {}
    for leg in a.legs.split(","):
        runs = []
        for _ in range(a.processes):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", leg, "--repeats", str(a.repeats), "--scale", str(a.scale)],
                               env=dict(os.environ), capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:  # a failed process ends the run: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"bench_connectivity: worker {leg} ended with status {p.returncode}")
            line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
            runs.append(json.loads(line[7:]))
        keys = [k for k in runs[0] if k.endswith("_ms")]
        c = results[leg] = {**{k: runs[0][k] for k in ("particles", "n_origin", "n_dest", "path", "pairs", "tracked", "outside", "atomics")},
                            "processes": len(runs), "matches_today": all(r["matches_today"] for r in runs),
                            **{k: _cell(sum((r[k] for r in runs), [])) for k in keys}}
        c["today_over_device"] = c["today_ms"]["median"] / c["device_ms"]["median"]
        print(f"{leg:8s} {c['path']:7s} device {c['device_ms']['median']:9.3f} ms ({c['device_ms']['min']:.3f} - {c['device_ms']['max']:.3f}; key {c['device_key_ms']['median']:.3f}"
              f" sort {c['device_sort_ms']['median']:.3f} encode {c['device_encode_ms']['median']:.3f})  today {c['today_ms']['median']:9.3f} ms"
              f" ({c['today_ms']['min']:.3f} - {c['today_ms']['max']:.3f})  x{c['today_over_device']:.1f}  re-upload after today"
              f" {c['today_exec_after_ms']['median'] - c['device_exec_after_ms']['median']:.3f} ms  matches {c['matches_today']}", flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_connectivity.py", "processes_per_leg": a.processes, "timed_calls_per_process": a.repeats,
                       "cell": "median / min / max over all timed calls of all processes, milliseconds", "legs": results}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
