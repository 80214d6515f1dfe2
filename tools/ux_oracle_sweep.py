#!/usr/bin/env python
"""Offline sweep of the NumPy UxGrid oracle (oracle/ux_oracle.py, switches "numpy" / "batch") against the live reference over the
seeded cases of oracle/ux_cases.py -- wider than the 40 seeds tests/test_ux_oracle.py compares on every run.

    python tools/ux_oracle_sweep.py [SEEDS=1200] [POINT_SEEDS=300] [PROCESSES=8] > profiles/ux_oracle_vs_reference.txt

Every column of the final particle arrays, the raised error and the observations of a run, and value / state / masked flag / ei of
Field.eval and UxGrid.search at the points are compared to the bit.
"""

from __future__ import annotations

import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POINT_FIELDS = ("P_fc", "P_ff", "P_nc", "P_nf", "UV", "UVW")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def run_seed(seed):
    import logging

    logging.disable(logging.INFO)  # (the reference announces every output file)
    from oracle import ux_cases, ux_oracle
    from tools import make_ux_golden as mg

    case = ux_cases.draw_case(seed)
    info = dict(seed=seed, mesh=case["mesh"], region=case["region"], kernels=case["kernels"], n=len(case["x"]), sdt=case["spatial_dtype"],
                hole=case["hole"] is not None, nt=len(case["time_s"]), backward=case["dt"] < 0, outputdt=case["outputdt"] is not None)
    try:
        res = ux_oracle.run_case(case, "numpy", "batch")
    except ux_oracle.GuessRuleAmbiguity:
        return dict(info, diff=["oracle refused: guess rules part ways"], err=None, slim=0.0)
    ref, err, _ = mg.run_case(case)
    diff = []
    if res["err"] != err:
        diff.append(f"error {res['err']} vs {err}")
    for k, v in ref.items():
        if k.startswith("obs_"):
            continue
        if k not in res["out"] or not _same(res["out"][k], v):
            diff.append(k)
    if "obs_time" in ref:
        if len(res["obs"]) != len(ref["obs_time"]):
            diff.append("observation count")
        else:
            join = np.concatenate if "obs_offsets" in ref else np.stack
            diff += ["obs_" + k for k in ("particle_id", "t", "z", "y", "x") if not _same(join([o[k] for _, o in res["obs"]]), ref["obs_" + k])]
    return dict(info, diff=diff, err=err, slim=float(res["slim"].mean()), left=len(res["out"]["x"]))


def run_points(seed):
    from oracle import ux_cases, ux_oracle
    from tools import make_ux_golden as mg

    case, pts = ux_cases.draw_points(seed)
    orc = ux_oracle.UxOracle(case, "numpy", "batch")
    diff = []
    nonfinite = 0
    for what in POINT_FIELDS:
        want = mg.eval_points_with_state(case, what, pts)
        got = orc.eval_points(what, pts["t"], pts["z"], pts["y"], pts["x"])
        diff += [f"{what}.{k}" for k in ("state", "ei", "masked") if not _same(got[k], want[k])]
        diff += [f"{what}[{k}]" for k, (a, b) in enumerate(zip(got["values"], want["values"])) if not _same(a, b)]
        nonfinite += int(sum((~np.isfinite(b)).sum() for b in want["values"]))
        if not _same(orc.search_points(pts["z"], pts["y"], pts["x"])[0], want["ei"]):
            diff.append(f"{what}.search")
    return dict(seed=seed, mesh=case["mesh"], diff=diff, n=len(pts["x"]), states=sorted(set(want["state"].tolist())), nonfinite=nonfinite)


def main(nseeds=1200, npoints=300, procs=8):
    import collections

    import numpy

    with mp.Pool(procs) as pool:
        runs = pool.map(run_seed, range(nseeds), chunksize=4)
        points = pool.map(run_points, range(npoints), chunksize=4)
    print("UxGrid: NumPy oracle (oracle/ux_oracle.py, f32_trig='numpy', guess_rule='batch') against the live reference")
    print(f"tools/ux_oracle_sweep.py {nseeds} {npoints}; NumPy {numpy.__version__}")
    print()
    print(f"ParticleSet.execute: seeds 0..{nseeds - 1} of oracle/ux_cases.py: draw_case")
    count = collections.Counter()
    for r in runs:
        count["mesh " + r["mesh"]] += 1
        count["region " + r["region"]] += 1
        count["error " + str(r["err"])] += 1
        count["float32 particles"] += r["sdt"] == "float32"
        count["hole in the mesh"] += r["hole"]
        count["backward"] += r["backward"]
        count["outputdt"] += r["outputdt"]
        count[f"time levels {r['nt']}"] += 1
        count["two advection kernels"] += sum(k.startswith("Advection") for k in r["kernels"]) > 1
        count["3-D kernel"] += any(k.endswith("_3D") for k in r["kernels"])
        count["3-D kernel or two kernels on a multi-level time axis"] += r["nt"] > 2 and (any(k.endswith("_3D") for k in r["kernels"]) or sum(k.startswith("Advection") for k in r["kernels"]) > 1)
        count["particles deleted"] += r.get("left", r["n"]) < r["n"]
    for k in sorted(count):
        print(f"  {k:60s} {count[k]:5d}")
    print(f"  particles in all {sum(r['n'] for r in runs)}")
    sph = [r["slim"] for r in runs if r["mesh"] == "spherical"]
    flat = [r["slim"] for r in runs if r["mesh"] == "flat"]
    print(f"  slim share, spherical seeds: mean {np.mean(sph):.4f} max {np.max(sph):.4f}, seeds over the 2 % cap {sum(s > 0.02 for s in sph)} of {len(sph)}")
    print(f"  slim share, flat seeds (no exclusions there): mean {np.mean(flat):.4f} max {np.max(flat):.4f}")
    bad = [r for r in runs if r["diff"]]
    print(f"  seeds with a difference (any column, any bit): {len(bad)}")
    for r in bad:
        print(f"    seed {r['seed']}: {r['mesh']} {r['kernels']}: {r['diff']}")
    print()
    print(f"Field.eval with fresh particles / UxGrid.search: seeds 0..{npoints - 1} of draw_points, {points[0]['n']} points each, fields {POINT_FIELDS}")
    print(f"  states met: {sorted(set(s for r in points for s in r['states']))}; non-finite values met {sum(r['nonfinite'] for r in points)}")
    bad = [r for r in points if r["diff"]]
    print(f"  seeds with a difference (value, state, masked flag, ei; any bit): {len(bad)}")
    for r in bad:
        print(f"    seed {r['seed']}: {r['mesh']}: {r['diff']}")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
