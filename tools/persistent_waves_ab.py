#!/usr/bin/env python
"""Where the headline launch spends time outside its step loop, and how full its wave slots are.

    python tools/persistent_waves_ab.py sweep [--steps 2,6,12,24,48,96] [--reps 5] [--out FILE] [--label TEXT]
        kernel ms (HIP events around the launch) of the headline launch of bench.py -- 1e7 particles, cell-sorted, from the state after
        the warm-up, restored from the device checkpoint before every launch -- at each step count: median and min / max of `reps`, then
        the least-squares line through the medians: slope = ms per step, intercept = ms spent outside the step loop.
    python tools/persistent_waves_ab.py pmc [--steps 24] [--out FILE] [--label TEXT]
        one rocprofv3 --pmc pass per counter group over a child that runs that one launch (counters in runs of their own, no other
        tracing, as tools/pmc_summary.py expects them) and, from the first group, the resident waves per SIMD of the launch:
            SQ_WAVE_CYCLES x 4 (it counts quad-cycles) / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs).
        A group this rocprofv3 does not know fails alone.

The library is the one parcels_amd loads: PARCELS_HIP_LIB selects an A/B build.  --out appends the report to a text file.
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
N_SIMD, N_XCD = 1024, 8
# (FETCH_SIZE and WRITE_SIZE in passes of their own, as tools/gpu_profile_c2.sh collects them: asked for together, the pass did not end within its time limit)
PMC_GROUPS = ["SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE", "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS", "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum",
              "FETCH_SIZE", "WRITE_SIZE"]


def sweep(steps, reps, particles, warmup=2):
    import numpy as np
    import torch

    import parcels_amd as pa
    from bench import c2_case
    from tests.case_utils import build_fieldset, build_pset

    case = c2_case(seed=1, lo=0, hi=int(particles))
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
    out = {"particles": int(particles), "reps": reps, "rows": rows}
    if len(rows) >= 2:
        slope, icpt = np.polyfit([r["steps"] for r in rows], [r["median"] for r in rows], 1)
        out.update(slope_ms_per_step=float(slope), intercept_ms=float(icpt))
    return out


def sweep_report(res, label):
    L = [f"## step sweep of the headline launch ({label}): {res['particles']} particles, {res['reps']} launches per point, kernel ms", "",
         "| steps | median | min | max |", "|---|---|---|---|"]
    L += [f"| {r['steps']} | {r['median']:.3f} | {r['min']:.3f} | {r['max']:.3f} |" for r in res["rows"]]
    if "slope_ms_per_step" in res:
        L += ["", f"line through the medians: {res['slope_ms_per_step']:.4f} ms per step, intercept {res['intercept_ms']:.3f} ms"]
    return "\n".join(L) + "\n"


def pmc(steps, particles, groups):
    counters, meta, failed = {}, {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for i, grp in enumerate(groups):
            d = os.path.join(tmp, f"p{i}")
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", *grp.split(), "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "sweep",
                   "--steps", str(steps), "--reps", "1", "--particles", str(particles)]
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
                    meta = {"kernel": r["Kernel_Name"], **{k: int(r[c]) for k, c in (("grid", "Grid_Size"), ("workgroup", "Workgroup_Size"), ("vgpr", "VGPR_Count"),
                                                                                   ("sgpr", "SGPR_Count"), ("lds", "LDS_Block_Size"), ("scratch", "Scratch_Size")) if r.get(c)}}
    res = {"steps": steps, "particles": int(particles), "counters": counters, "failed_groups": failed, **meta}
    if counters.get("SQ_WAVE_CYCLES") and counters.get("GRBM_GUI_ACTIVE"):
        res["resident_waves_per_simd"] = counters["SQ_WAVE_CYCLES"] * 4.0 / (counters["GRBM_GUI_ACTIVE"] / N_XCD * N_SIMD)
    return res


def pmc_report(res, label):
    L = [f"## counters of the headline launch ({label}): {res['particles']} particles x {res['steps']} steps", "",
         f"kernel `{str(res.get('kernel'))[:110]}`: grid {res.get('grid')} work-items in workgroups of {res.get('workgroup')}, VGPR {res.get('vgpr')}, SGPR {res.get('sgpr')}, "
         f"LDS {res.get('lds')} B, scratch {res.get('scratch')} B", "", "| counter | value |", "|---|---|"]
    L += [f"| {k} | {v:.5g} |" for k, v in sorted(res["counters"].items())]
    if "resident_waves_per_simd" in res:
        L += ["", f"resident waves per SIMD = SQ_WAVE_CYCLES x 4 / (GRBM_GUI_ACTIVE / {N_XCD} x {N_SIMD}) = **{res['resident_waves_per_simd']:.3f}** of 4"]
    if res["failed_groups"]:
        L += ["", "groups that did not run: " + "; ".join(res["failed_groups"])]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sweep", "pmc"])
    ap.add_argument("--steps", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--label", default=os.environ.get("PARCELS_HIP_LIB", "the library of this tree"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", default=",".join(str(i) for i in range(len(PMC_GROUPS))), help="pmc: indices of the counter groups to run (group 0 gives the resident waves)")
    a = ap.parse_args()
    if a.mode == "sweep":
        res = sweep([int(s) for s in (a.steps or "2,6,12,24,48,96").split(",")], a.reps, a.particles)
        text = sweep_report(res, a.label)
    else:
        res = pmc(int(a.steps or 24), a.particles, [PMC_GROUPS[int(i)] for i in a.groups.split(",")])
        text = pmc_report(res, a.label)
    print(text)
    print(json.dumps({a.mode: res, "label": a.label}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
