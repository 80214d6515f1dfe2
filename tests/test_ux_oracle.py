"""CPU: the NumPy oracle of the unstructured-mesh path (oracle/ux_oracle.py) pinned to the reference -- to the fixtures of
tests/golden/ux/ without it, to the live reference on the seeded cases of oracle/ux_cases.py where it is present -- and the conditions
the GPU differential fuzz (tests/test_gpu_ux_fuzz.py) rests on: the two trigonometry modes differ by the documented residual and nothing
else, and the `slim` exclusions stay under their cap.

Measured (profiles/ux_oracle_vs_reference.txt): every result below is equal to the bit, positions included; no NumPy
reduction order had to be bounded."""

import glob
import os

import numpy as np
import pytest

from oracle import ref_shim, ux_cases, ux_oracle
from tools import make_ux_golden as mg
from ux_utils import numpy_f32_trig_differs

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mg.GOLDEN, "ux_*.npz")))
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference sources not present")
ORACLE_SEEDS = int(os.environ.get("PARCELS_UX_ORACLE_SEEDS", "40"))
GPU_SEED0 = int(os.environ.get("PARCELS_UX_FUZZ_SEED0", "0"))
GPU_SEEDS = int(os.environ.get("PARCELS_UX_FUZZ_SEEDS", "128"))
SLIM_CAP = 0.02
POINT_FIELDS = ("P_fc", "P_ff", "P_nc", "P_nf", "UV", "UVW")


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    same = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else a == b
    assert same.all(), f"{what}: {int((~same).sum())} of {a.size} differ, first rows {np.flatnonzero(~np.atleast_1d(same))[:5]}"


def assert_run_equals(res, ref, err, label):
    """error name, state, ei, t, particle order, positions and sampled Variables, observation ids / times / positions: all exactly"""
    assert res["err"] == err, f"{label}: error {res['err']} vs {err}"
    out = res["out"]
    for k, v in ref.items():
        if not k.startswith("obs_"):
            assert k in out, f"{label}: column {k} missing"
            assert_same_bits(out[k], v, f"{label}: {k}")
    if "obs_time" in ref:
        assert len(res["obs"]) == len(ref["obs_time"]), f"{label}: {len(res['obs'])} observations vs {len(ref['obs_time'])}"
        assert_same_bits(np.array([tm for tm, _ in res["obs"]]), ref["obs_time"], f"{label}: obs_time")
        join = np.concatenate if "obs_offsets" in ref else np.stack
        for k in ("particle_id", "t", "z", "y", "x"):
            assert_same_bits(join([o[k] for _, o in res["obs"]]), ref["obs_" + k], f"{label}: obs_{k}")


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_fixture(name):
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    assert_run_equals(ux_oracle.run_case(case, "numpy", "batch"), case["ref"], case["err"], name)


@pytest.mark.parametrize("name", [n for n in FIXTURES if mg.with_eval(n)])
def test_oracle_reproduces_the_fixture_evaluations(name):
    case = mg.load(os.path.join(mg.GOLDEN, name + ".npz"))
    ev = case["eval"]
    orc = ux_oracle.UxOracle(case, "numpy", "batch")
    for fname in case["fields"]:
        assert_same_bits(orc.eval_points(fname, ev["t"], ev["z"], ev["y"], ev["x"])["values"][0], ev["val_" + fname], f"{name}: {fname}")
    u, v = orc.eval_points("UV", ev["t"], ev["z"], ev["y"], ev["x"])["values"]
    assert_same_bits(u, ev["val_UV_u"], f"{name}: UV.u")
    assert_same_bits(v, ev["val_UV_v"], f"{name}: UV.v")


@needs_reference
@pytest.mark.parametrize("seed", range(ORACLE_SEEDS))
def test_oracle_equals_the_live_reference(seed):
    case = ux_cases.draw_case(seed)
    ref, err, _ = mg.run_case(case)
    assert_run_equals(ux_oracle.run_case(case, "numpy", "batch"), ref, err, f"seed {seed} ({case['mesh']}, {case['kernels']})")


@needs_reference
@pytest.mark.parametrize("seed", range(ORACLE_SEEDS))
def test_oracle_points_equal_the_live_reference(seed):
    """Field.eval with fresh particles at the points, and UxGrid.search: value, state, masked flag, ei"""
    case, pts = ux_cases.draw_points(seed)
    orc = ux_oracle.UxOracle(case, "numpy", "batch")
    for what in POINT_FIELDS:
        want = mg.eval_points_with_state(case, what, pts)
        got = orc.eval_points(what, pts["t"], pts["z"], pts["y"], pts["x"])
        label = f"seed {seed} ({case['mesh']}) {what}"
        assert len(got["values"]) == len(want["values"])
        for k, (a, b) in enumerate(zip(got["values"], want["values"])):
            assert_same_bits(a, b, f"{label}: component {k}")
        for k in ("state", "ei", "masked"):
            assert_same_bits(got[k], want[k], f"{label}: {k}")
        ei, _ = orc.search_points(pts["z"], pts["y"], pts["x"])
        assert_same_bits(ei, want["ei"], f"{label}: search")


def test_trig_modes_differ_only_where_numpy_rounds_incorrectly():
    """the unit-sphere query points of the two f32_trig modes are bit-identical at every (y, x) that numpy_f32_trig_differs does not
    flag, and differ by at most one float32 ulp of a component's factors at the others: the "rounded" mode (the device's) differs
    from the pinned one by the documented residual and nothing else"""
    rng = np.random.default_rng(11)
    y = rng.uniform(-90.0, 90.0, 100_000).astype(np.float32)
    x = rng.uniform(-200.0, 200.0, 100_000).astype(np.float32)
    case = mg.load(os.path.join(mg.GOLDEN, "ux_sph_dateline_face_rk4.npz"))
    qn = ux_oracle.UxOracle(case, "numpy", "batch").query_points(y, x)
    qr = ux_oracle.UxOracle(case, "rounded", "batch").query_points(y, x)
    assert qn.dtype == qr.dtype == np.float32
    flagged = numpy_f32_trig_differs(y, x)
    assert 0.02 < flagged.mean() < 0.6  # (the residual exists: NumPy's float32 sin / cos are not correctly rounded)
    assert np.array_equal(qn[~flagged], qr[~flagged])
    assert (qn[flagged] != qr[flagged]).any(axis=1).mean() > 0.5
    # two factors off by an ulp each, and the rounding of their product: 3 float32 spacings of a value of magnitude <= 1
    assert np.max(np.abs(qn.astype(np.float64) - qr.astype(np.float64))) <= 3 * 2.0 ** -24


@pytest.mark.parametrize("seed", range(GPU_SEED0, GPU_SEED0 + GPU_SEEDS))
def test_slim_share_stays_under_the_cap(seed):
    """over the seeds of the GPU fuzz, with its switches: on spherical meshes -- the only ones where `slim` takes a particle out of a
    comparison -- at most 2 % of a seed's particles are slim; and the oracle never strays into the situation where the guess rules part
    ways (it would raise).  Flat meshes are compared whole, whatever their flags."""
    case = ux_cases.draw_case(seed)
    res = ux_oracle.run_case(case, "rounded", "device")
    share = float(res["slim"].mean())
    print(f"seed {seed}: {case['mesh']} {case['kernels']} n={len(case['x'])} slim {share:.4f}")
    if case["mesh"] == "spherical":
        assert share <= SLIM_CAP, f"seed {seed}: {res['slim'].sum()} of {len(case['x'])} particles slim"


@pytest.mark.parametrize("seed", range(int(os.environ.get("PARCELS_UX_FUZZ_POINT_SEEDS", "30"))))
def test_slim_share_of_the_points_stays_under_the_cap(seed):
    case, pts = ux_cases.draw_points(seed)
    orc = ux_oracle.UxOracle(case, "rounded", "device")
    slim = orc.search_points(pts["z"], pts["y"], pts["x"])[1]
    for what in POINT_FIELDS:
        slim = slim | orc.eval_points(what, pts["t"], pts["z"], pts["y"], pts["x"])["slim"]
    assert slim.mean() <= SLIM_CAP, f"seed {seed}: {slim.sum()} of {len(slim)} points slim"


def test_generator_keeps_the_bounds_the_slim_margins_rest_on():
    """lateral extent >= a tenth of the coordinate scale, every face >= 1 / 40 of the extent high (oracle/ux_cases.py)"""
    for seed in range(0, 200, 3):
        m = ux_cases.draw_mesh(seed)
        lon0, lon1, lat0, lat1 = m["box"]
        ext = min(lon1 - lon0, lat1 - lat0)
        scale = max(np.abs(m["node_lon"]).max(), np.abs(m["node_lat"]).max(), np.abs(m["zf"]).max())
        assert ext >= 0.1 * scale, seed
        assert ux_cases.min_altitude(m["node_lon"], m["node_lat"], m["faces"]) >= ext / 40.0, seed
        assert 2 <= len(m["zf"]) <= 6 and np.all(np.diff(m["zf"]) > 0)


def test_guess_rule_ambiguity_raises():
    """a lone particle that stays in face 0 of level 0: every ei is 0 at the second evaluation, where the reference's batch rule and the
    device's rule part ways -- the oracle refuses under either"""
    case = mg.load(os.path.join(mg.GOLDEN, "ux_flat_uniform_ee.npz"))
    f0 = case["faces"][0]
    case = dict(case, x=np.array([case["node_lon"][f0].mean()]), y=np.array([case["node_lat"][f0].mean()]), runtime=600.0)
    for rule in ("batch", "device"):
        with pytest.raises(ux_oracle.GuessRuleAmbiguity):
            ux_oracle.run_case(case, "numpy", rule)
