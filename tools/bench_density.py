#!/usr/bin/env python
"""ParticleSet.density (csrc/pk_density.hip) beside what a script does today, on one GPU.

    python tools/bench_density.py [--out profiles/density_bench.json] [--legs c2_1e6,c2_1e7,lds,ux_flat,ux_sph] [--processes 3] [--repeats 5]

Every leg is measured in `--processes` fresh processes run one after the other (the variants of a leg alternate); in a process the first
call of everything is untimed and `--repeats` calls are timed.  A cell of the result is the median with min - max over all timed calls of
all processes.  Times are host clocks around calls that end in a device synchronise (the map is downloaded); the kernel split (bin /
sort / sum, HIP events) comes from pk_density_info_t.

Legs:
  c2_1e6, c2_1e7   the C2-size rectilinear grid (360 x 180 x 50 nodes, spherical), float64 particles: counts and weighted sums, on
                   cell-sorted rows and on rows in host order
  lds              counts on a 64 x 64-cell grid (fits the LDS histogram), 1e7 particles in host order -- the contended case -- without and
                   with the workgroup-private LDS histogram (PK_DENSITY_LDS=1)
  ux_flat, ux_sph  counts on the ~1e6-triangle meshes of tools/bench_ux.py, 1e7 particles
`today` beside each: read pset.x / pset.y (two columns come down and are marked dirty), pk_search on them, np.bincount; and the execute()
that follows either route (one DoNothing step): after the host route it uploads the two columns again.
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


def _rect_fieldset(lon, lat, depth):
    import parcels_amd as pa

    md = pa.SGrid2DMetadata(node_dimensions=("XG", "YG"), node_coordinates=("lon", "lat"),
                            face_dimensions=(pa.FaceNodePadding("XC", "XG", pa.Padding.LOW), pa.FaceNodePadding("YC", "YG", pa.Padding.LOW)),
                            vertical_dimensions=(pa.FaceNodePadding("ZC", "depth", pa.Padding.BOTH),))
    shape = (2, depth.size, lat.size, lon.size)
    dims = ("time", "depth", "YG", "XG")
    ds = pa.Dataset({"U": (dims, np.zeros(shape)), "V": (dims, np.zeros(shape))},
                    {"lon": (("XG",), lon), "lat": (("YG",), lat), "depth": (("depth",), depth), "time": (("time",), np.array([0.0, 86400.0]))}, sgrid=md)
    return pa.FieldSet.from_sgrid_conventions(ds, mesh="spherical")


def _setup(leg, n):
    """-> (fieldset, x, y, z)"""
    rng = np.random.default_rng(7)
    if leg.startswith("c2"):
        fs = _rect_fieldset(np.linspace(0.0, 360.0, 360), np.linspace(-80.0, 80.0, 180), np.linspace(0.0, 5000.0, 50))
        return fs, rng.uniform(5.0, 355.0, n), rng.uniform(-75.0, 75.0, n), rng.uniform(10.0, 4990.0, n)
    if leg == "lds":
        fs = _rect_fieldset(np.linspace(0.0, 64.0, 65), np.linspace(-32.0, 32.0, 65), np.array([0.0, 100.0]))
        return fs, rng.uniform(0.5, 63.5, n), rng.uniform(-31.5, 31.5, n), np.full(n, 50.0)
    from tools import bench_ux

    fs, _, (x0, x1, y0, y1) = bench_ux.fieldset(leg == "ux_sph")
    wx, wy = x1 - x0, y1 - y0
    return fs, rng.uniform(x0 + 0.1 * wx, x1 - 0.1 * wx, n), rng.uniform(y0 + 0.1 * wy, y1 - 0.1 * wy, n), np.full(n, 0.5)


def worker(leg, variant, n, repeats):
    """one process: the timed calls of one (leg, variant); one JSON line"""
    import parcels_amd as pa
    from parcels_amd.engine import density_shape

    fs, x, y, z = _setup(leg, n)
    sort = variant.startswith("sorted")
    pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x, y=y, z=z, t=np.zeros(n), sort_by_cell=sort)
    w = np.random.default_rng(8).standard_normal(n)
    grid = fs.U.grid
    ncells = int(np.prod(density_shape(grid, False)))

    def step():
        t0 = time.perf_counter()
        pset.execute([pa.DoNothing], dt=60.0, runtime=60.0)
        return (time.perf_counter() - t0) * 1e3

    step()
    eng = fs._engine
    out = {"leg": leg, "variant": variant, "particles": n, "cells": ncells, "lds": os.environ.get("PK_DENSITY_LDS", "0"),
           "counts_ms": [], "counts_bin_ms": [], "counts_exec_after_ms": [], "atomics": None, "inside": None,
           "sums_ms": [], "sums_bin_ms": [], "sums_sort_ms": [], "sums_sum_ms": [],
           "today_ms": [], "today_read_ms": [], "today_search_ms": [], "today_bincount_ms": [], "today_exec_after_ms": []}
    want_sums = leg.startswith("c2")
    want_today = variant in ("sorted", "host_order")
    ref = None
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        counts = pset.density()
        dt_counts = (time.perf_counter() - t0) * 1e3
        info = dict(pset._last_density_info)
        after = step()
        if r:
            out["counts_ms"].append(dt_counts)
            out["counts_bin_ms"].append(info["bin_ms"])
            out["counts_exec_after_ms"].append(after)
        out["atomics"], out["inside"] = int(info["n_atomics"]), int(info["n_inside"])
        if want_sums:
            t0 = time.perf_counter()
            pset.density(particle_val=w)
            dt_sums = (time.perf_counter() - t0) * 1e3
            info = dict(pset._last_density_info)
            step()
            if r:
                out["sums_ms"].append(dt_sums)
                for k in ("bin", "sort", "sum"):
                    out[f"sums_{k}_ms"].append(info[f"{k}_ms"])
        if want_today:
            t0 = time.perf_counter()
            xs, ys = pset.x, pset.y
            t1 = time.perf_counter()
            ei = eng.search(0, np.zeros(n) if not leg.startswith("ux") else z, ys, xs)
            t2 = time.perf_counter()
            ok = ei >= 0
            today = np.bincount(ei[ok] % ncells, minlength=ncells)
            t3 = time.perf_counter()
            del xs, ys
            after = step()
            if r:
                out["today_ms"].append((t3 - t0) * 1e3)
                out["today_read_ms"].append((t1 - t0) * 1e3)
                out["today_search_ms"].append((t2 - t1) * 1e3)
                out["today_bincount_ms"].append((t3 - t2) * 1e3)
                out["today_exec_after_ms"].append(after)
            ref = today
    out["matches_today"] = None if ref is None else bool(np.array_equal(np.asarray(counts).ravel(), ref))
    print("RESULT " + json.dumps(out), flush=True)


def _cell(values):
    v = np.asarray(values, dtype=np.float64)
    return None if v.size == 0 else {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


LEGS = {"c2_1e6": (1_000_000, ["sorted", "host_order"]), "c2_1e7": (10_000_000, ["sorted", "host_order"]),
        "lds": (10_000_000, ["host_order", "host_order_lds"]), "ux_flat": (10_000_000, ["host_order"]), "ux_sph": (10_000_000, ["host_order"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_bench.json"))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the particle counts (rehearsals)")
    ap.add_argument("--worker", nargs=2, metavar=("LEG", "VARIANT"))
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per process")
    a = ap.parse_args()
    if a.worker:
        leg, variant = a.worker
        worker(leg, variant, max(int(LEGS[leg][0] * a.scale), 1), a.repeats)
        return
    results = {}
    if os.path.exists(a.out):  # legs measured by an earlier call stay
        with open(a.out) as f:
            results = json.load(f).get("legs", {})
    for leg in a.legs.split(","):
        n, variants = LEGS[leg]
        runs = {v: [] for v in variants}
        for _ in range(a.processes):
            for v in variants:  # the variants of a leg alternate
                env = dict(os.environ, PK_DENSITY_LDS="1" if v.endswith("_lds") else "0")
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", leg, v, "--repeats", str(a.repeats), "--scale", str(a.scale)],
                                   env=env, capture_output=True, text=True, timeout=a.timeout)
                if p.returncode != 0:  # a failed process ends the run: nothing more is started on the device
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"bench_density: worker {leg}/{v} ended with status {p.returncode}")
                line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
                runs[v].append(json.loads(line[7:]))
        results[leg] = {}
        for v, rs in runs.items():
            keys = [k for k in rs[0] if k.endswith("_ms")]
            results[leg][v] = {"particles": rs[0]["particles"], "cells": rs[0]["cells"], "atomics": rs[0]["atomics"], "inside": rs[0]["inside"],
                               "processes": len(rs), "matches_today": rs[0]["matches_today"],
                               **{k: _cell(sum((r[k] for r in rs), [])) for k in keys},
                               "runs": {k: [r[k] for r in rs] for k in ("counts_ms", "counts_bin_ms")}}
            c = results[leg][v]
            print(f"{leg:8s} {v:15s} counts {c['counts_ms']['median']:9.3f} ms (kernel {c['counts_bin_ms']['median']:.3f})"
                  + (f"  sums {c['sums_ms']['median']:9.3f} ms" if c["sums_ms"] else "")
                  + (f"  today {c['today_ms']['median']:9.3f} ms + {c['today_exec_after_ms']['median'] - c['counts_exec_after_ms']['median']:.3f} re-upload" if c["today_ms"] else ""),
                  flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_density.py", "processes_per_variant": a.processes, "timed_calls_per_process": a.repeats,
                       "cell": "median / min / max over all timed calls of all processes, milliseconds", "legs": results}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
