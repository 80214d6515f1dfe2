#!/usr/bin/env python
"""Time of the neighbour search behind particle-particle interaction kernels (parcels_amd/interaction.py, csrc/pk_neighbors.hip).

    python tools/bench_interaction.py [--particles 1e5,1e6,1e7] [--repeats 5] [--brute 2e4] [--out profiles/interaction_bench.json]
    python tools/bench_interaction.py --mesh spherical [--regional 1e6] [--out profiles/interaction_sph_bench.json]

Workload: uniform points in the unit square, radius chosen for a mean of about 8 neighbours (pi r^2 n = 8).  Per size the four
passes of the C ABI are timed on their own -- build (upload + cell list), counts, nearest, pairs (fill + row sort + download; the
count pass it needs is not in its time) -- and `pa.neighbors` as a user calls it.  Every pass ends in a stream synchronise, so a
host clock around the call is the call time, transfers over PCIe included.  One cold call, then the median of --repeats calls with
min / max.  `scaling` is t(largest) / t(next smaller) per pass: 10 is linear.

There is no earlier device implementation to compare with.  The yardstick is what a user writes today: the dense NumPy all-pairs
matrices at --brute points (the same box, one run: it takes seconds and gigabytes), with the device time at that size beside it and
the counts of both compared.  Where scipy is installed, cKDTree.query_pairs at 1e6 is reported too (unordered pairs: half the list).
Prints one JSON line per leg and writes them all to --out.

--mesh spherical times the great-circle search with the same method: points uniform on the sphere, radius in metres chosen for a
mean of 8 neighbours (n (1 - cos(radius / R)) / 2 = 8), and a regional leg of --regional points uniform in a 10 x 10 degree box at
(30 W - 20 W, 40 N - 50 N) with the same mean.  Its yardstick is the flat table at the same n and mean neighbour count (run both
on one machine); the NumPy and scipy legs belong to the flat run only.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import parcels_amd as pa  # noqa: E402
from parcels_amd import interaction  # noqa: E402
from parcels_amd.xgrid import EARTH_RADIUS  # noqa: E402

MEAN_NEIGHBOURS = 8.0


def points(n, seed=1):
    rng = np.random.default_rng(seed)
    return rng.random(n), rng.random(n), float(np.sqrt(MEAN_NEIGHBOURS / (np.pi * n)))


def sphere_points(n, seed=1):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-180.0, 180.0, n), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))
    return x, y, float(EARTH_RADIUS * np.arccos(1.0 - 2.0 * MEAN_NEIGHBOURS / n))


def regional_points(n, seed=3):
    rng = np.random.default_rng(seed)
    s0, s1 = np.sin(np.radians(40.0)), np.sin(np.radians(50.0))
    x, y = rng.uniform(-30.0, -20.0, n), np.degrees(np.arcsin(rng.uniform(s0, s1, n)))  # uniform in area
    area = EARTH_RADIUS**2 * np.radians(10.0) * (s1 - s0)
    return x, y, float(np.sqrt(MEAN_NEIGHBOURS * area / (np.pi * n)))


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def device_leg(n, repeats, make_points=points, spherical=False, name="device"):
    x, y, radius = make_points(n)
    ctx = interaction._context()
    lib, h = ctx.lib, ctx.handle
    p = interaction._ptr
    count = np.zeros(n, dtype=np.int64)
    nj, nd = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
    total = C.c_int64()
    t = {"build": [], "counts": [], "nearest": [], "pairs": [], "neighbors_call": []}
    out = None
    for rep in range(repeats + 1):  # the first round is cold (code objects, first allocations)
        t0 = time.perf_counter()
        if spherical:
            ctx.check(lib.pk_neighbors_build_spherical(h, n, p(x), p(y), None, None, radius, EARTH_RADIUS, 0), "pk_neighbors_build_spherical")
        else:
            ctx.check(lib.pk_neighbors_build(h, n, p(x), p(y), None, None, radius, 0), "pk_neighbors_build")
        t1 = time.perf_counter()
        ctx.check(lib.pk_neighbors_counts(h, p(count), C.byref(total)), "pk_neighbors_counts")
        t2 = time.perf_counter()
        ctx.check(lib.pk_neighbors_nearest(h, p(nj), p(nd)), "pk_neighbors_nearest")
        t3 = time.perf_counter()
        if out is None:
            m = total.value
            out = [np.zeros(n + 1, dtype=np.int64), np.zeros(m, dtype=np.int64)] + [np.zeros(m, dtype=np.float64) for _ in range(3)]
        t4 = time.perf_counter()
        ctx.check(lib.pk_neighbors_pairs(h, total.value, p(out[0]), p(out[1]), p(out[2]), p(out[3]), None, p(out[4])), "pk_neighbors_pairs")
        t5 = time.perf_counter()
        nb = pa.neighbors((x, y), radius, mesh="spherical" if spherical else "flat")
        t6 = time.perf_counter()
        assert nb.total == total.value and np.array_equal(nb.j, out[1])
        del nb
        for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t5 - t4, t6 - t5)):
            t[k].append(v * 1e3)
    if spherical:
        info = interaction.cell_list_info_spherical()
        grid = {"bands": info["bands"], "cells": info["cells"], "band_height_deg": info["band_height"], "periodic": info["periodic"]}
    else:
        info = interaction.cell_list_info()
        grid = {"cells": [info["ncx"], info["ncy"]]}
    leg = {"leg": name, "n": n, "radius": radius, "pairs": int(total.value), "mean_neighbours": total.value / n, **grid,
           "doublings": info["doublings"], "repeats": repeats}
    for k, v in t.items():
        leg[k] = dict(stats(v[1:]), cold_ms=round(v[0], 3))
    return leg


def brute_leg(n):
    """the dense matrices of the tutorial's kernels: distances, the mask, its row sums and the pair arrays"""
    x, y, radius = points(n, seed=2)
    t0 = time.perf_counter()
    dx = x[None, :] - x[:, None]
    dy = y[None, :] - y[:, None]
    dist = dx * dx
    dist += dy * dy  # (in place: three n x n float64 matrices are 9.6 GB at n = 2e4 already)
    np.sqrt(dist, out=dist)
    m = dist < radius
    np.fill_diagonal(m, False)
    count = m.sum(axis=1)
    i, j = np.nonzero(m)
    pdx, pdy, pdist = dx[i, j], dy[i, j], dist[i, j]
    t_brute = (time.perf_counter() - t0) * 1e3
    del dx, dy, dist, m
    pa.neighbors((x, y), radius)  # warm
    t0 = time.perf_counter()
    nb = pa.neighbors((x, y), radius)
    t_dev = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(nb.count, count) and np.array_equal(nb.j, j) and np.array_equal(nb.dx, pdx) and np.array_equal(nb.dy, pdy)
                and np.array_equal(nb.dist, pdist))
    return {"leg": "numpy_all_pairs", "n": n, "radius": radius, "pairs": int(len(j)), "numpy_ms": round(t_brute, 1),
            "device_neighbors_call_ms": round(t_dev, 3), "identical": same}


def scipy_leg(n):
    try:
        from scipy.spatial import cKDTree
    except Exception as e:  # not installed: not required
        return {"leg": "scipy_ckdtree_query_pairs", "n": n, "available": False, "why": type(e).__name__}
    x, y, radius = points(n)
    t0 = time.perf_counter()
    pairs = cKDTree(np.column_stack([x, y])).query_pairs(radius, output_type="ndarray")
    return {"leg": "scipy_ckdtree_query_pairs", "n": n, "available": True, "unordered_pairs": int(len(pairs)),
            "ms": round((time.perf_counter() - t0) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1e5,1e6,1e7")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brute", default="2e4")
    ap.add_argument("--scipy-particles", default="1e6")
    ap.add_argument("--mesh", choices=["flat", "spherical"], default="flat")
    ap.add_argument("--regional", default="1e6", help="points of the regional leg of --mesh spherical (0: none)")
    ap.add_argument("--out", default=None, help="default: profiles/interaction_bench.json, interaction_sph_bench.json for --mesh spherical")
    a = ap.parse_args()
    sph = a.mesh == "spherical"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "interaction_sph_bench.json" if sph else "interaction_bench.json")
    sizes = [int(float(s)) for s in a.particles.split(",") if s]
    legs = []
    dev = interaction._context().device_info()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(leg):  # the file is complete after every leg
        legs.append(leg)
        print(json.dumps(leg), flush=True)
        workload = ("points uniform on the sphere, n (1 - cos(radius / R)) / 2 = 8, great-circle distances in metres, float64, 2-D; regional: "
                    "uniform in a 10 x 10 degree box, same mean") if sph else "uniform points in the unit square, pi r^2 n = 8, float64, 2-D"
        res = {"device": dev["name"], "arch": dev["arch"], "workload": workload,
               "timing": "host clock around calls that end in a stream synchronise (PCIe transfers included); median of the timed calls, "
                         "min / max beside it",
               "device_bytes_per_pair": interaction.device_bytes_per_pair(False), "legs": legs}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for n in sizes:
        emit(device_leg(n, a.repeats, sphere_points, True) if sph else device_leg(n, a.repeats))
    if len(sizes) >= 2:
        big, small = legs[len(sizes) - 1], legs[len(sizes) - 2]
        emit({"leg": "scaling", "n": [small["n"], big["n"]],
              **{k: round(big[k]["median_ms"] / small[k]["median_ms"], 2) for k in ("build", "counts", "nearest", "pairs", "neighbors_call")}})
    if sph and float(a.regional) > 0:
        emit(device_leg(int(float(a.regional)), a.repeats, regional_points, True, name="device_regional"))
    interaction.release()
    if sph:
        return
    if a.brute and float(a.brute) > 0:
        emit(brute_leg(int(float(a.brute))))
    if a.scipy_particles and float(a.scipy_particles) > 0:
        emit(scipy_leg(int(float(a.scipy_particles))))


if __name__ == "__main__":
    main()
