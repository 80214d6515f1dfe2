"""GPU: seeded differential fuzzing of the CROCO sigma-grid program (csrc/pk_sigma.h, pk_prog_sigma.hip: advect_sigma_kernel,
sigma_points_kernel, croco_sigma) against the C oracle's CROCO kernels (oracle/parcels_oracle.c), which tests/test_croco_oracle.py pins to
the reference bit for bit.

Every seed of oracle/croco_cases.py draws a grid (rectilinear | curvilinear, flat | spherical, float32 | float64 data, C-grid | every field
on the nodes: the eight instantiations of launch_sigma), 2 .. 300 sigma levels, the stretching, hc, the amplitude of zeta, 1 .. 600
particles (both sides of a wavefront and of a workgroup, common or scattered release times, a share of starts outside the water column, at
a lateral edge, exactly on a level / the floor / the surface), a kernel list, dt of either sign and the run, and demands what the fixtures
demand: the same raised error, the same particle order, `state`, `ei`, `t` and observation ids / times exactly, positions and sampled
Variables to the bars of tests/croco_utils.py: tolerance_for.  Every particle and every point is compared: the oracle flags no row `slim`.
A drawn subset of the seeds runs a second time with a ring of 3 level slots, another cell-sorted, against the same oracle result.

Needs neither the reference nor scipy.  A whole run with the defaults (96 + 24 seeds, 140 device runs) took 17 s on the
MI355X, the slowest seed 0.7 s; the figures are in DESIGN.md section 12."""

import os
import warnings

import numpy as np
import pytest

import parcels_amd as pa
from croco_utils import PROG_SIGMA, croco_fieldset, run_croco, scales, tolerance_for
from oracle import croco_cases

pytestmark = pytest.mark.gpu

SEED0 = int(os.environ.get("PARCELS_CROCO_FUZZ_SEED0", "0"))
SEEDS = int(os.environ.get("PARCELS_CROCO_FUZZ_SEEDS", "96"))
POINT_SEEDS = int(os.environ.get("PARCELS_CROCO_FUZZ_POINT_SEEDS", "24"))
SLIM_CAP = 0.02


def close(a, b, rtol, scale, what):
    """|a - b| <= rtol (|b| + scale), NaN where the oracle has NaN -> the largest deviation in units of the bar"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
        ok = (d <= rtol * (np.abs(b) + scale)) | (np.isnan(a) & np.isnan(b)) | (a == b)
        dev = np.where(np.isfinite(d), d / (np.abs(b) + scale), 0.0)
    worst = float(dev.max(initial=0.0))
    assert ok.all(), f"{what}: rows {np.flatnonzero(~ok)[:5]}: {a[~ok][:3]} vs {b[~ok][:3]} (largest {worst:.3e}, rtol {rtol:g})"
    return worst / rtol


def compare(case, res, got, gerr, rec, label, by_id=False):
    """-> (largest deviation as a share of the bar, bit-identical)"""
    assert gerr == res["err"], f"{label}: raised {gerr}, the oracle {res['err']}"
    if case["leaves"] and res["err"] == "OutsideTimeInterval":
        return 0.0, True  # (the columns are unspecified once zeta's time interval is left: DESIGN.md section 12)
    ref, slim = res["out"], res["slim"]
    assert slim.mean() <= SLIM_CAP, f"{label}: {slim.sum()} particles slim"
    if by_id:  # a cell-sorted set is handed back in another order
        order = np.argsort(got["particle_id"], kind="stable")
        got = {k: np.asarray(v)[order] for k, v in got.items()}
        assert np.array_equal(got["particle_id"], np.sort(ref["particle_id"])), f"{label}: surviving ids differ"
        order = np.argsort(ref["particle_id"], kind="stable")
        ref = {k: np.asarray(v)[order] for k, v in ref.items()}
    kg, kr = ~slim[got["particle_id"]], ~slim[ref["particle_id"]]
    assert np.array_equal(got["particle_id"][kg], ref["particle_id"][kr]), f"{label}: particle order differs"
    for k in ("state", "ei", "t"):
        a, b = np.asarray(got[k])[kg], np.asarray(ref[k])[kr]
        assert np.array_equal(a, b), f"{label}: {k} differs at rows {np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8]}"
    rtol, sc = tolerance_for(case), scales(case)
    worst, identical = 0.0, True
    for k, scale in sc.items():
        worst = max(worst, close(got[k][kg], ref[k][kr], rtol, scale, f"{label}: {k}"))
        identical = identical and np.array_equal(np.asarray(got[k])[kg], np.asarray(ref[k])[kr], equal_nan=True)
    if case["outputdt"] and not by_id:
        assert rec is not None and len(rec.obs) == len(res["obs"]), f"{label}: {0 if rec is None else len(rec.obs)} observations vs {len(res['obs'])}"
        for j, ((tm, ids, x, y, z, t), (otm, o)) in enumerate(zip(rec.obs, res["obs"])):
            assert tm == otm, f"{label}: observation {j} at {tm} vs {otm}"
            assert np.array_equal(ids, o["particle_id"]), f"{label}: ids of observation {j}"
            assert np.array_equal(t, o["t"]), f"{label}: t of observation {j}"
            for k, v in (("x", x), ("y", y), ("z", z)):
                worst = max(worst, close(v, o[k], rtol, sc[k], f"{label}: {k} of observation {j}"))
                identical = identical and np.array_equal(np.asarray(v), o[k], equal_nan=True)
    return worst, identical


@pytest.mark.parametrize("seed", range(SEED0, SEED0 + SEEDS))
def test_random_croco_configuration_matches_oracle(gpu, seed):
    case = croco_cases.draw_case(seed)
    res = croco_cases.run_oracle(case)
    calls = [float(case["split"]), float(case["runtime"]) - float(case["split"])] if case["split"] else None
    label = f"seed {seed}: key {croco_cases.launch_key(case)} {case['mesh']} nw={len(case['coords']['s_w'])} n={len(case['x'])} {case['kernels']} " \
            f"dt={case['dt']} steps={case['runtime'] / abs(case['dt']):g} sdt={case['spatial_dtype']} outputdt={case['outputdt']} split={case['split']}"
    runs = [("plain", dict(sort_by_cell=False), None)]
    if case["device"] == "ring":
        runs.append(("ring of 3 slots", dict(sort_by_cell=False), "ring"))
    elif case["device"] == "sorted":
        runs.append(("cell-sorted", dict(sort_by_cell=True), None))
    for name, kw, ring in runs:
        fs = croco_fieldset(case)
        if ring:
            fs = fs.to_windowed_arrays()
        got, gerr, rec, stats = run_croco(case, fs=fs, calls=calls, **kw)
        worst, identical = compare(case, res, got, gerr, rec, f"{label} [{name}]", by_id=name == "cell-sorted")
        if any("CROCO" in k.upper() for k in case["kernels"]) and stats is not None:
            assert stats["program"] == PROG_SIGMA, f"{label}: program {stats['program']}"
        print(f"{label} [{name}] err={gerr} largest deviation {worst:.2e} of the bar, bit-identical={identical}")


@pytest.mark.parametrize("seed", range(POINT_SEEDS))
def test_random_croco_points_match_oracle(gpu, seed):
    """pa.convert_z_to_sigma_croco(fs, t, z, y, x, None) (sigma_points_kernel): NaN positions and infinities exactly, finite values to
    |a - b| <= 1e-12 (|b| + 1), the bar of test_gpu_croco.py: test_sigma_at_points_matches_the_reference"""
    case = croco_cases.draw_points(seed)
    res = croco_cases.run_oracle(case)
    want, slim = res["sigma"], res["slim"]
    assert slim.mean() <= SLIM_CAP
    fs = croco_fieldset(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = np.asarray(pa.convert_z_to_sigma_croco(fs, case["t"], case["z"], case["y"], case["x"], None))
    label = f"seed {seed}: key {croco_cases.launch_key(case)} {case['mesh']} nw={len(case['coords']['s_w'])} m={len(case['x'])}"
    assert got.shape == want.shape, label
    got, want = got[~slim], want[~slim]
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label}: NaN at {np.flatnonzero(np.isnan(got) != np.isnan(want))[:8]}"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.isinf(got[~inf]).any(), f"{label}: infinities"
    fin = np.isfinite(want)
    d = np.abs(got[fin] - want[fin]) / (np.abs(want[fin]) + 1.0)
    worst = float(d.max(initial=0.0))
    print(f"{label} largest |a - b| / (|b| + 1) = {worst:.2e}, bit-identical={np.array_equal(got, want, equal_nan=True)}")
    assert np.all(d <= 1e-12), f"{label}: {worst:.3e} at {np.flatnonzero(d > 1e-12)[:8]}"
