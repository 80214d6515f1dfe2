#!/usr/bin/env python
"""Time of the neighbour search behind particle-particle interaction kernels (parcels_amd/interaction.py, csrc/pk_neighbors.hip).

    python tools/bench_interaction.py [--particles 1e5,1e6,1e7] [--repeats 5] [--brute 2e4] [--out profiles/interaction_bench.json]

Workload: uniform points in the unit square, radius chosen for a mean of about 8 neighbours (pi r^2 n = 8).  Per size the four
passes of the C ABI are timed on their own -- build (upload + cell list), counts, nearest, pairs (fill + row sort + download; the
count pass it needs is not in its time) -- and `pa.neighbors` as a user calls it.  Every pass ends in a stream synchronise, so a
host clock around the call is the call time, transfers over PCIe included.  One cold call, then the median of --repeats calls with
min / max.  `scaling` is t(largest) / t(next smaller) per pass: 10 is linear.

There is no earlier device implementation to compare with.  The yardstick is what a user writes today: the dense NumPy all-pairs
matrices at --brute points (the same box, one run: it takes seconds and gigabytes), with the device time at that size beside it and
the counts of both compared.  Where scipy is installed, cKDTree.query_pairs at 1e6 is reported too (unordered pairs: half the list).
Prints one JSON line per leg and writes them all to --out.
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

MEAN_NEIGHBOURS = 8.0


def points(n, seed=1):
    rng = np.random.default_rng(seed)
    return rng.random(n), rng.random(n), float(np.sqrt(MEAN_NEIGHBOURS / (np.pi * n)))


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def device_leg(n, repeats):
    x, y, radius = points(n)
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
        nb = pa.neighbors((x, y), radius)
        t6 = time.perf_counter()
        assert nb.total == total.value and np.array_equal(nb.j, out[1])
        del nb
        for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t5 - t4, t6 - t5)):
            t[k].append(v * 1e3)
    info = interaction.cell_list_info()
    leg = {"leg": "device", "n": n, "radius": radius, "pairs": int(total.value), "mean_neighbours": total.value / n,
           "cells": [info["ncx"], info["ncy"]], "doublings": info["doublings"], "repeats": repeats}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interaction_bench.json"))
    a = ap.parse_args()
    sizes = [int(float(s)) for s in a.particles.split(",") if s]
    legs = []
    dev = interaction._context().device_info()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(leg):  # the file is complete after every leg
        legs.append(leg)
        print(json.dumps(leg), flush=True)
        res = {"device": dev["name"], "arch": dev["arch"], "workload": "uniform points in the unit square, pi r^2 n = 8, float64, 2-D",
               "timing": "host clock around calls that end in a stream synchronise (PCIe transfers included); median of the timed calls, "
                         "min / max beside it",
               "device_bytes_per_pair": interaction.device_bytes_per_pair(False), "legs": legs}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for n in sizes:
        emit(device_leg(n, a.repeats))
    if len(sizes) >= 2:
        big, small = legs[len(sizes) - 1], legs[len(sizes) - 2]
        emit({"leg": "scaling", "n": [small["n"], big["n"]],
              **{k: round(big[k]["median_ms"] / small[k]["median_ms"], 2) for k in ("build", "counts", "nearest", "pairs", "neighbors_call")}})
    interaction.release()
    if a.brute and float(a.brute) > 0:
        emit(brute_leg(int(float(a.brute))))
    if a.scipy_particles and float(a.scipy_particles) > 0:
        emit(scipy_leg(int(float(a.scipy_particles))))


if __name__ == "__main__":
    main()
