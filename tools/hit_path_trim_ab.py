#!/usr/bin/env python
"""What the hit path of the headline launch costs, and what its miss branches cost on top (profiles/c2_hit_path_trim_ab.txt).

    python tools/hit_path_trim_ab.py sweep [--uv-scale 1e-4] [--steps 24,96] [--reps 5] [--out FILE] [--label TEXT]
        kernel ms (HIP events around the launch) of the headline launch of bench.py from the warmed, checkpointed state, as
        tools/persistent_waves_ab.py takes it.  --uv-scale S multiplies U and V of the same FieldSet by S for the same particles: with 1e-4
        no lane leaves its cell in 24 steps (at most 1e-4 m/s x 96 h = 35 m), so every wave-evaluation behind the launch's first runs the hit path.
    python tools/hit_path_trim_ab.py pmc [--uv-scale 1e-4] [--steps 24] [--out FILE] [--label TEXT]
        one rocprofv3 --pmc pass per counter group over a child that runs that one launch (a run of its own per group, no other tracing
        than the kernel trace persistent_waves_ab.py uses), then VALU / SALU / LDS / vector-memory reads per wave-evaluation: a launch of n particles x K steps
        runs ceil(n / 64) x K x 4 wave-evaluations.

The library is the one parcels_amd loads: PARCELS_HIP_LIB selects the parent's build.  --out appends the report to a text file.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.persistent_waves_ab import sweep_report  # noqa: E402

PMC_GROUPS = ["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES", "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES",
              "SQ_INSTS_VMEM_RD SQ_INSTS_SMEM"]


def sweep(steps, reps, particles, uv_scale, warmup=2):
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
    rows = []
    for j, K in enumerate([steps[-1]] + list(steps)):  # (one untimed launch first: clock ramp, first touch of the levels)
        kms = []
        for _ in range(1 if j == 0 else reps):
            eng.ctx.check(eng.lib.pk_particles_restore(eng.ctx.handle), "pk_particles_restore")
            torch.cuda.synchronize()
            st = eng.execute(kern.kernel_ids, endtime=(warmup + K) * dt, dt0=dt, sort_by_cell=0, t_start=warmup * dt)
            torch.cuda.synchronize()
            assert int(st["steps"]) == int(particles) * K, (st["steps"], K)
            kms.append(float(st["kernel_ms"]))
        if j:
            kms.sort()
            rows.append({"steps": K, "median": kms[(len(kms) - 1) // 2], "min": kms[0], "max": kms[-1]})
    out = {"particles": int(particles), "reps": reps, "rows": rows, "uv_scale": uv_scale}
    if len(rows) >= 2:
        slope, icpt = np.polyfit([r["steps"] for r in rows], [r["median"] for r in rows], 1)
        out.update(slope_ms_per_step=float(slope), intercept_ms=float(icpt))
    return out


def pmc(steps, particles, uv_scale):
    counters, meta, failed = {}, {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for i, grp in enumerate(PMC_GROUPS):
            d = os.path.join(tmp, f"p{i}")
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", *grp.split(), "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "sweep",
                   "--steps", str(steps), "--reps", "1", "--particles", str(particles), "--uv-scale", repr(uv_scale)]
            try:
                rc = subprocess.run(cmd, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240).returncode
            except subprocess.TimeoutExpired:
                failed.append(grp + " (time limit)")
                break  # (nothing more is started on the GPU behind a run that hung)
            files = glob.glob(os.path.join(d, "**", "p_counter_collection.csv"), recursive=True)
            if rc != 0 or not files:
                failed.append(grp)
                if rc < 0 or rc in (124, 134, 137, 139):
                    break
                continue
            rows = [r for r in csv.DictReader(open(files[0])) if "advect" in r["Kernel_Name"]]
            last = max(int(r["Dispatch_Id"]) for r in rows)  # the last advection dispatch is the measured launch
            for r in rows:
                if int(r["Dispatch_Id"]) == last:
                    counters[r["Counter_Name"]] = counters.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                    meta = {"kernel": r["Kernel_Name"], **{k: int(r[c]) for k, c in (("vgpr", "VGPR_Count"), ("sgpr", "SGPR_Count"), ("scratch", "Scratch_Size")) if r.get(c)}}
    nwe = -(-int(particles) // 64) * steps * 4
    res = {"steps": steps, "particles": int(particles), "uv_scale": uv_scale, "counters": counters, "failed_groups": failed, "wave_evaluations": nwe, **meta}
    for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_SMEM"):
        if k in counters:
            res[k + "_per_wave_evaluation"] = counters[k] / nwe
    return res


def pmc_report(res, label):
    L = [f"## counters of the headline launch ({label}; U, V x {res['uv_scale']:g}): {res['particles']} particles x {res['steps']} steps = {res['wave_evaluations']} wave-evaluations", "",
         f"kernel `{str(res.get('kernel'))[:110]}`: VGPR {res.get('vgpr')}, SGPR {res.get('sgpr')}, scratch {res.get('scratch')} B", "", "| counter | value | per wave-evaluation |", "|---|---|---|"]
    for k, v in sorted(res["counters"].items()):
        per = res.get(k + "_per_wave_evaluation")
        L.append(f"| {k} | {v:.6g} | {'' if per is None else format(per, '.1f')} |")
    if res["failed_groups"]:
        L += ["", "groups that did not run: " + "; ".join(res["failed_groups"])]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sweep", "pmc"])
    ap.add_argument("--steps", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--uv-scale", type=float, default=1.0, help="U and V of the FieldSet are multiplied by this (1e-4: the pure hit path)")
    ap.add_argument("--label", default=os.environ.get("PARCELS_HIP_LIB", "the library of this tree"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "sweep":
        res = sweep([int(s) for s in (a.steps or "24,96").split(",")], a.reps, a.particles, a.uv_scale)
        text = sweep_report(res, f"{a.label}; U, V x {a.uv_scale:g}")
    else:
        res = pmc(int(a.steps or 24), a.particles, a.uv_scale)
        text = pmc_report(res, a.label)
    print(text)
    print(json.dumps({a.mode: res, "label": a.label}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
