"""CPU: the C oracle's CROCO kernels (oracle/parcels_oracle.c: convert_z_to_sigma_croco, SampleOmegaCroco and its per-field form,
AdvectionRK2_3D_CROCO, written from the text of the reference's kernels/_sigmagrids.py) pinned to the reference -- to the fixtures of
tests/golden/croco/ without it, to the live reference on the seeded cases of oracle/croco_cases.py where it is present -- and the conditions
the GPU differential fuzz (tests/test_gpu_croco_fuzz.py) rests on: the generator reaches every axis it names, every deliberately wrong
restatement of the kernels is visible at the GPU comparison's bar on some default seed, and the `slim` exclusions stay under their cap.

Every comparison with the reference in this file is bitwise, positions and sampled Variables included.  Measured (DESIGN.md section 12,
profiles/croco_oracle_vs_reference.txt): every result is equal to the bit, with the reference's particles twinned (its batch of one) and
the oracle's sines and cosines taken from NumPy (c_oracle.numpy_trig)."""

import glob
import os

import numpy as np
import pytest

from oracle import c_oracle, croco_cases, ref_shim
from tools import make_croco_golden as mg

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mg.GOLDEN, "croco_*.npz")))
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference sources not present")
ORACLE_SEEDS = int(os.environ.get("PARCELS_CROCO_ORACLE_SEEDS", "60"))
GPU_SEED0 = int(os.environ.get("PARCELS_CROCO_FUZZ_SEED0", "0"))
GPU_SEEDS = int(os.environ.get("PARCELS_CROCO_FUZZ_SEEDS", "96"))
GPU_POINT_SEEDS = int(os.environ.get("PARCELS_CROCO_FUZZ_POINT_SEEDS", "24"))
COVER = range(GPU_SEED0, GPU_SEED0 + max(GPU_SEEDS, 96))  # coverage and sensitivity: never over fewer than the default number of seeds
SLIM_CAP = 0.02
VARIANTS = [v for v in c_oracle.CROCO_VARIANTS if v is not None]
# float64_arithmetic cannot show on a fieldset the project accepts: the reference forms a float32 operation in _sigmagrids.py only where h
# is a float32 ARRAY, and XLinear returns float64 for h whenever the depth coordinate of the sample is a float64 array -- it always is:
# z = 0 lies on the last node of the float64 s_w axis (bcoord 1 > 0, so the depth interpolation with that float64 bcoord takes place),
# and float32 coordinate arrays are refused at Kernel construction (tests/test_croco_host.py).  Asserted below as exactly that.
UNREACHABLE_VARIANTS = ["float64_arithmetic"]

_RUNS = {}


def default_run(seed):
    """(case, oracle result) of a default GPU-fuzz seed, computed once and left unchanged"""
    if seed not in _RUNS:
        case = croco_cases.draw_case(seed)
        _RUNS[seed] = (case, croco_cases.run_oracle(case))
    return _RUNS[seed]


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    same = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else a == b
    assert same.all(), f"{what}: {int((~same).sum())} of {a.size} differ, first rows {np.flatnonzero(~np.atleast_1d(same))[:5]}"


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_fixture(name):
    """trajectories with error name and observations, the points of croco_sigma_points*, and croco_host_recipe (the recipe is the text of
    the sampling kernel): needs no reference"""
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    ref = case["ref"]
    res = croco_cases.run_oracle(case)
    if case.get("kind") == "sigma_points":
        assert_same_bits(res["sigma"], ref["sigma"], f"{name}: sigma")
        return
    assert res["err"] == case["err"], f"{name}: error {res['err']} vs {case['err']}"
    for k, v in ref.items():
        if not k.startswith("obs_"):
            assert_same_bits(res["out"][k], v, f"{name}: {k}")
    if "obs_time" in ref:
        assert len(res["obs"]) == len(ref["obs_time"])
        assert_same_bits(np.array([tm for tm, _ in res["obs"]]), ref["obs_time"], f"{name}: obs_time")
        join = np.concatenate if "obs_offsets" in ref else np.stack
        for k in ("particle_id", "t", "z", "y", "x"):
            assert_same_bits(join([o[k] for _, o in res["obs"]]), ref["obs_" + k], f"{name}: obs_{k}")


@needs_reference
@pytest.mark.parametrize("seed", range(ORACLE_SEEDS))
def test_oracle_equals_the_live_reference(seed):
    case = croco_cases.draw_case(seed)
    ref, err = croco_cases.run_reference(case)
    with c_oracle.numpy_trig():
        res = croco_cases.run_oracle(case)
    diff = croco_cases.differences(case, res, ref, err)
    assert not diff, f"seed {seed} (key {croco_cases.launch_key(case)}, {case['mesh']}, {case['kernels']}): {diff}"


@needs_reference
@pytest.mark.parametrize("seed", range(ORACLE_SEEDS))
def test_oracle_points_equal_the_live_reference(seed):
    case = croco_cases.draw_points(seed)
    want, _ = croco_cases.run_reference(case)
    assert_same_bits(croco_cases.run_oracle(case)["sigma"], want["sigma"], f"seed {seed} (key {croco_cases.launch_key(case)}, {case['mesh']})")


def test_numpy_trig_changes_nothing_on_a_flat_mesh():
    """the switch the live comparison runs under reaches the spherical unit conversion and the spherical curvilinear search only"""
    seed = next(s for s in COVER if default_run(s)[0]["mesh"] == "flat" and croco_cases.launch_key(default_run(s)[0]) in (2, 3, 6, 7))
    case, res = default_run(seed)
    with c_oracle.numpy_trig():
        again = croco_cases.run_oracle(case)
    assert again["err"] == res["err"]
    for k, v in res["out"].items():
        assert_same_bits(again["out"][k], v, k)


def test_generator_reaches_every_axis():
    """over the seeds the GPU fuzz runs by default: a later edit of the generator cannot silently drop an axis"""
    runs = [default_run(s) for s in COVER]
    cases = [c for c, _ in runs]
    assert {croco_cases.launch_key(c) for c in cases} == set(range(8))
    assert {len(c["coords"]["s_w"]) for c in cases} == set(croco_cases.NW)
    counts = {len(c["x"]) for c in cases}
    assert min(counts) < 64 < max(counts) and 64 in counts and any(64 < n < 256 for n in counts) and 256 in counts and any(n > 256 for n in counts)
    assert {np.sign(c["dt"]) for c in cases} == {-1.0, 1.0}
    assert {tuple(c["kernels"]) for c in cases} == set(croco_cases.KERNEL_LISTS)
    assert {"FieldOutOfBoundError", "FieldOutOfBoundSurfaceError", "OutsideTimeInterval", None} <= {r["err"] for _, r in runs}
    assert any(len(r["out"]["x"]) < len(c["x"]) for c, r in runs if r["err"] is None)
    assert {c["device"] for c in cases} == {None, "ring", "sorted"}
    assert any(c["outputdt"] for c in cases) and any(c["split"] for c in cases)
    assert any(len(np.unique(c["t0"])) > 1 for c in cases) and {c["spatial_dtype"] for c in cases} == {"float32", "float64"}
    assert {k for c in cases for k in c["edge_kinds"]} == {"floor_under", "surface_above", "edge", "on_level", "on_floor", "on_surface"}
    hc_place = {int(c["hc"] < c["fields"]["h"].min()) - int(c["hc"] > c["fields"]["h"].max()) for c in cases}
    assert hc_place == {-1, 0, 1}
    assert any(c["theta_s"] == 0.0 for c in cases) and any(c["theta_s"] > 0.0 for c in cases)
    assert any(c["fields"]["zeta"].min() < 0 < c["fields"]["zeta"].max() for c in cases)
    points = [croco_cases.draw_points(s) for s in range(max(GPU_POINT_SEEDS, 24))]
    assert {len(p["x"]) for p in points} == set(croco_cases.POINT_COUNTS)
    assert {croco_cases.launch_key(p) >> 1 for p in points} == {0, 1, 2, 3}  # (the points kernel has no velocity: data dtype x grid kind)


def visible(case, a, b):
    """the GPU comparison's bar: error name, `state`, `ei`, order exactly, or a float column beyond tolerance_for (tests/croco_utils.py:
    1e-12 for float64 particles, 5e-7 for float32 storage, relative to |reference| + scale)"""
    if a["err"] != b["err"]:
        return True
    x, y = a["out"], b["out"]
    if len(x["state"]) != len(y["state"]) or any(not np.array_equal(x[k], y[k]) for k in ("particle_id", "state", "ei")):
        return True
    rtol = 5e-7 if case["spatial_dtype"] == "float32" else 1e-12
    co, f = case["coords"], case["fields"]
    xy = max(float(np.max(np.abs(co["x_rho"]))), float(np.max(np.abs(co["y_rho"]))))
    sc = {"x": xy, "y": xy, "dx": xy, "dy": xy, "z": float(np.max(f["h"])), "dz": float(np.max(f["h"]))}
    for k in case["kernels"]:
        cs = c_oracle.croco_sample(k)
        if cs is not None:
            sc[cs[1]] = float(np.max(np.abs(f[cs[0]])))
    for k, scale in sc.items():
        p, q = np.asarray(x[k], np.float64), np.asarray(y[k], np.float64)
        with np.errstate(invalid="ignore"):
            ok = (np.abs(p - q) <= rtol * (np.abs(q) + scale)) | (np.isnan(p) & np.isnan(q)) | (p == q)
        if not ok.all():
            return True
    return False


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_restatement_is_visible_on_a_default_seed(variant):
    """each deliberately wrong restatement differs from the oracle by more than the GPU comparison's bar on at least one default seed: the
    cases can tell a subtly wrong kernel.  The one restatement that no accepted fieldset can show (see UNREACHABLE_VARIANTS) must show
    on none -- a seed that did would mean the reference forms float32 operations after all, and the comment above is wrong."""
    seen = []
    for seed in COVER:
        case, res = default_run(seed)
        if case["leaves"]:
            continue
        if visible(case, croco_cases.run_oracle(case, variant=variant), res):
            seen.append(seed)
            if variant not in UNREACHABLE_VARIANTS:
                break
    print(f"{variant}: visible on seeds {seen}")
    if variant in UNREACHABLE_VARIANTS:
        assert not seen, f"{variant} shows on seeds {seen}"
    else:
        assert seen, f"{variant} is invisible on seeds {COVER[0]} .. {COVER[-1]}: the generator misses an input"


def test_a_wrong_restatement_is_visible_at_the_points():
    """the three restatements of the conversion itself, at the points of the default seeds (bar: 1e-12 (|b| + 1), NaN / inf exactly)"""
    for variant in ("wrap_as_level_0", "fallback_n_minus_1", "zvec_without_zeta"):
        seen = False
        for seed in range(max(GPU_POINT_SEEDS, 24)):
            case = croco_cases.draw_points(seed)
            a, b = croco_cases.run_oracle(case, variant=variant)["sigma"], croco_cases.run_oracle(case)["sigma"]
            with np.errstate(invalid="ignore"):
                ok = (np.abs(a - b) <= 1e-12 * (np.abs(b) + 1.0)) | (np.isnan(a) & np.isnan(b)) | (a == b)
            seen = seen or not ok.all()
        assert seen, variant


@pytest.mark.parametrize("seed", range(GPU_SEED0, GPU_SEED0 + GPU_SEEDS, 8))
def test_slim_share_stays_under_the_cap(seed):
    """eight seeds per case of this test: at most 2 % of a seed's particles may be left out of the GPU comparison (none is, so far)"""
    for s in range(seed, min(seed + 8, GPU_SEED0 + GPU_SEEDS)):
        case, res = default_run(s)
        assert res["slim"].shape == (len(case["x"]),) and res["slim"].mean() <= SLIM_CAP, f"seed {s}: {res['slim'].sum()} particles slim"
        placed = np.asarray(case["edge_rows"], dtype=int)
        assert not res["slim"][placed].any(), f"seed {s}: a particle placed on a level on purpose is flagged"
    for s in range(GPU_POINT_SEEDS if seed == GPU_SEED0 else 0):
        assert croco_cases.run_oracle(croco_cases.draw_points(s))["slim"].mean() <= SLIM_CAP
