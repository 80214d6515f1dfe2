#!/usr/bin/env python
"""The level stream of a CF-PACKED archive: int16 U, V, W with scale_factor / add_offset / _FillValue in an uncompressed zarr store, streamed
through a ring of device slots by ParticleSet.execute (AdvectionRK4_3D on the curvilinear C-grid of tools/bench_configs.py --config c3).

    python tools/bench_stream_packed.py                       # the c3 grid (4322 x 3059 x 75), 6 levels, ring of 3
    python tools/bench_stream_packed.py --scale 0.25          # the same mesh at a quarter of the resolution per horizontal axis
    python tools/bench_stream_packed.py --shape 75 764 1080   # nz ny nx

Prints one JSON line: wall time of a run (median of --reps timed runs after a cold one, with min - max), field levels uploaded per second,
pk_upload_stats and engine.transfers of the median run, the host seconds of the stream, and -- where the library unpacks on the device and
keeps the counters (pk_unpack_stats, option "unpack_timing") -- the HIP-event time of the DMA and of the decode kernel per field level, taken in
one extra run.  Everything else is API of every commit that has ZarrLevels: the same file measures a commit without the device path
(or this one with PARCELS_AMD_DEVICE_UNPACK=0), which unpacks every level on the host."""

from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FILL = -32767


def write_store(root, nz, ny, nx, nt):
    """U, V, W of bench_configs.nemo_like_dataset, level by level, as int16 zarr v2 arrays (one uncompressed chunk per time level) with a
    float32 scale_factor / add_offset and a fill value in every 7th place.  Returns the coordinates and the seconds it took."""
    from bench_configs import nemo_like_coords

    t0 = time.perf_counter()
    lon, lat, i, j = nemo_like_coords(nx, ny)
    depth = np.concatenate([[0.0], np.cumsum(np.linspace(5.0, 150.0, nz - 1))])
    zprof = np.exp(-depth / 1500.0).astype(np.float32)[:, None, None]
    ii, jj = i.astype(np.float32), j.astype(np.float32)
    planes = {
        "U": (0.5 * np.cos(6 * np.pi * jj) * (1.0 + 0.3 * np.sin(10 * np.pi * ii))).astype(np.float32),
        "V": (0.3 * np.sin(8 * np.pi * ii) * np.cos(4 * np.pi * jj)).astype(np.float32),
        "W": (1e-4 * np.sin(12 * np.pi * ii) * np.sin(12 * np.pi * jj)).astype(np.float32),
    }
    level = np.empty((nz, ny, nx), np.float32)
    raw = np.empty((nz, ny, nx), np.int16)
    for name, plane in planes.items():
        d = os.path.join(root, name)
        os.makedirs(d)
        amp = float(np.abs(plane).max()) * 1.2
        sf, ao = np.float32(amp / 32000.0), np.float32(0.01 * amp)
        json.dump({"zarr_format": 2, "shape": [nt, nz, ny, nx], "chunks": [1, nz, ny, nx], "dtype": "<i2", "compressor": None, "fill_value": None,
                   "order": "C", "filters": None}, open(os.path.join(d, ".zarray"), "w"))
        json.dump({"scale_factor": float(sf), "add_offset": float(ao), "_FillValue": FILL}, open(os.path.join(d, ".zattrs"), "w"))
        for k in range(nt):
            f = np.float32(1.0 + 0.2 * np.sin(2 * np.pi * k / max(nt, 2)))
            np.multiply(zprof, plane[None] * f, out=level)
            level -= ao
            level /= sf
            np.rint(level, out=level)
            raw[...] = level
            raw.reshape(-1)[::7] = FILL
            with open(os.path.join(d, f"{k}.0.0.0"), "wb") as fh:
                fh.write(raw.data)
    return lon, lat, depth, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", type=float, default=1.0, help="of the c3 mesh per horizontal axis")
    ap.add_argument("--shape", type=int, nargs=3, metavar=("NZ", "NY", "NX"), help="instead of the c3 shape")
    ap.add_argument("--nt", type=int, default=6)
    ap.add_argument("--nslots", type=int, default=3)
    ap.add_argument("--particles", type=float, default=1e6)
    ap.add_argument("--days", type=float, default=None, help="model time of a run (default: nt - 1 levels of one day)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the store is written (default: a temporary directory, removed afterwards)")
    a = ap.parse_args()
    nz, ny, nx = a.shape if a.shape else (75, max(int(3059 * a.scale), 32), max(int(4322 * a.scale), 32))
    root = tempfile.mkdtemp(prefix="packed_stream_", dir=a.dir)
    try:
        run(a, root, nz, ny, nx)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def run(a, root, nz, ny, nx):
    import parcels_amd as pa
    from bench_configs import seed_particles

    nt, n = a.nt, int(a.particles)
    lon, lat, depth, write_s = write_store(root, nz, ny, nx, nt)
    md = pa.SGrid2DMetadata(
        node_dimensions=("XG", "YG"), node_coordinates=("lon", "lat"),
        face_dimensions=(pa.FaceNodePadding("XC", "XG", pa.Padding.LOW), pa.FaceNodePadding("YC", "YG", pa.Padding.LOW)),
        vertical_dimensions=(pa.FaceNodePadding("ZC", "depth", pa.Padding.HIGH),),
    )
    src = {c: pa.ZarrLevels(root, c) for c in "UVW"}
    dv = {"U": (("time", "ZC", "YC", "XG"), src["U"]), "V": (("time", "ZC", "YG", "XC"), src["V"]), "W": (("time", "depth", "YC", "XC"), src["W"])}
    ds = pa.Dataset(dv, {"lon": (("YG", "XG"), lon), "lat": (("YG", "XG"), lat), "depth": (("depth",), depth), "time": (("time",), np.arange(nt) * 86400.0)},
                    sgrid=md)
    fs = pa.FieldSet.from_sgrid_conventions(ds, mesh="spherical", skip_field_data_validation=True)
    fs.to_device(0, nslots=a.nslots)
    eng = fs._engine
    levels = [0]
    upload = eng._upload

    def counting_upload(name, level, asynchronous):
        if eng.pack_leader_of.get(name, name) == name:
            levels[0] += len(eng.pack_groups.get(name, [name]))
        return upload(name, level, asynchronous)

    eng._upload = counting_upload
    x, y, z = seed_particles(lon, lat, depth, n, seed=3)
    dt = 3600.0
    runtime = (a.days if a.days is not None else nt - 1) * 86400.0
    has_stats = hasattr(eng.ctx, "unpack_stats")

    def one_run():
        pset = pa.ParticleSet(fs, pclass=pa.get_default_particle(np.float64), x=x, y=y, z=z, t=np.zeros(n), sort_by_cell=True)
        pset.populate_indices()
        levels[0] = 0
        before = eng.ctx.upload_stats()
        transfers0 = dict(eng.transfers)
        unpack0 = eng.ctx.unpack_stats() if has_stats else None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            pset.execute([pa.AdvectionRK4_3D, pa.DeleteParticle], dt=dt, runtime=runtime)
            wall = time.perf_counter() - t0
        after = eng.ctx.upload_stats()
        st = pset._last_stats
        out = {"wall_s": wall, "field_levels": levels[0], "field_levels_per_s": levels[0] / wall, "kernel_ms": float(st["kernel_ms"]),
               "launches": int(st["launches"]), "particle_steps": int(st["steps"]),
               "upload_stats": {k: (after[k] - before[k] if k != "stage_threads" else after[k]) for k in after},
               "transfers": {k: v - transfers0.get(k, 0) for k, v in eng.transfers.items() if k.startswith("levels_")} or None,
               "stream_host_s": {k: st.get(k) for k in ("commit_s", "prefetch_s", "wait_s")}}
        out["staged_bytes_per_field_level"] = out["upload_stats"]["stage_bytes"] / max(levels[0], 1)
        if has_stats:
            u = eng.ctx.unpack_stats()
            out["unpack_stats"] = {k: u[k] - unpack0[k] for k in u}
        return out

    cold = one_run()
    runs = [one_run() for _ in range(max(a.reps, 1))]
    walls = sorted(r["wall_s"] for r in runs)
    med = [r for r in runs if r["wall_s"] == walls[(len(walls) - 1) // 2]][0]
    result = {
        "tool": "bench_stream_packed", "grid": [nx, ny, nz, nt], "nslots": a.nslots, "particles": n, "model_days": runtime / 86400.0,
        "raw_bytes_per_field_level": nz * ny * nx * 2, "device_unpack": bool(med["transfers"] and med["transfers"].get("levels_packed")),
        "wall_s": {"median": med["wall_s"], "min": walls[0], "max": walls[-1], "n": len(walls), "cold": cold["wall_s"], "all": [r["wall_s"] for r in runs]},
        "field_levels_per_s": {"median": med["field_levels_per_s"], "min": min(r["field_levels_per_s"] for r in runs),
                               "max": max(r["field_levels_per_s"] for r in runs)},
        "median_run": med, "store_write_s": write_s,
    }
    if has_stats and result["device_unpack"]:  # one more run with HIP events around every chunk's DMA and decode (it may wait for them)
        eng.ctx.set_option("unpack_timing", 1)
        timed = one_run()
        eng.ctx.set_option("unpack_timing", 0)
        u = timed["unpack_stats"]
        per = max(u["levels"], 1) * (len(eng.pack_groups.get("U", ["U"])))
        result["per_field_level_ms"] = {"dma": u["dma_ms"] / per, "decode": u["decode_ms"] / per, "decode_over_dma": u["decode_ms"] / max(u["dma_ms"], 1e-9),
                                        "field_levels": per, "wall_s_of_that_run": timed["wall_s"]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
