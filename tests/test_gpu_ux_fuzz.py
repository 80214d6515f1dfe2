"""GPU: seeded differential fuzzing of the unstructured-mesh program (csrc/pk_ux.h, pk_prog_ux.hip) against the NumPy oracle
(oracle/ux_oracle.py), which tests/test_ux_oracle.py pins to the reference bit for bit.

Every seed of oracle/ux_cases.py draws a mesh (flat / spherical, graded, with a hole, across +-180 degrees, next to a pole, around the
peaks of the unit-sphere coordinates), the registration of U, V, W, the axes (with a ring of 3 level slots now and then), a kernel list,
the run and the particles (counts on both sides of a wavefront and of a workgroup), and demands what the fixtures demand: the same raised
error, the same `state`, `ei`, `t`, particle order and observations exactly, positions and sampled Variables to the bars of
tests/ux_utils.py: tolerance_for.  The oracle runs with the device's two documented deviations switched on ("rounded" float32
trigonometry, the per-particle guess rule).

Flat meshes: every particle is compared.  Spherical meshes: the particles the oracle flags `slim` (a decision within 1e-9 of its
threshold, or a float32 rounding within 1e-4 of a spacing from a boundary -- the device's cosine of the unit conversion is its own
polynomial, an ulp of it may send such a particle down another branch) are left out, at most 2 % of a seed's particles.

Needs neither the reference nor scipy."""

import os
import warnings

import numpy as np
import pytest

from case_utils import max_rel
from oracle import ux_cases, ux_oracle
from ux_utils import coordinate_scale, run_ux, tolerance_for, ux_fieldset

pytestmark = pytest.mark.gpu

SEED0 = int(os.environ.get("PARCELS_UX_FUZZ_SEED0", "0"))
SLIM_CAP = 0.02
POINT_FIELDS = ("P_fc", "P_ff", "P_nc", "P_nf", "UV", "UVW")
FLOAT_COLUMNS = ("x", "y", "z", "dx", "dy", "dz", "sampled", "kc")


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isclose(a, b, rtol=rtol, atol=atol, equal_nan=True)
    assert ok.all(), f"{what}: max rel {max_rel(a, b):.3e} (rtol {rtol:g}) at rows {np.flatnonzero(~ok)[:5]}"
    with np.errstate(invalid="ignore"):
        dev = np.abs(a - b) / (np.abs(b) + atol / rtol)
    return float(np.max(dev[np.isfinite(dev)], initial=0.0))


@pytest.mark.parametrize("seed", range(SEED0, SEED0 + int(os.environ.get("PARCELS_UX_FUZZ_SEEDS", "128"))))
def test_random_ux_configuration_matches_oracle(gpu, seed):
    case = ux_cases.draw_case(seed)
    res = ux_oracle.run_case(case, "rounded", "device")
    got, gerr, rec = run_ux(case)
    ref = res["out"]
    label = f"seed {seed}: {case['mesh']}/{case['region']} faces={len(case['faces'])} n={len(case['x'])} {case['kernels']} dt={case['dt']} " \
            f"nt={len(case['time_s'])} nslots={case['nslots']} outputdt={case['outputdt']} sdt={case['spatial_dtype']}"
    assert gerr == res["err"], label
    slim = res["slim"] if case["mesh"] == "spherical" else np.zeros(len(case["x"]), bool)  # flat: no exclusions
    assert slim.mean() <= SLIM_CAP, f"{label}: {slim.sum()} particles slim"
    rtol = tolerance_for(case["name"], case)
    atol = rtol * coordinate_scale(case)

    def rows(ids):
        return ~slim[np.asarray(ids)]

    kg, kr = rows(got["particle_id"]), rows(ref["particle_id"])
    assert np.array_equal(got["particle_id"][kg], ref["particle_id"][kr]), f"{label}: particle order differs"
    for k in ("state", "ei", "t"):
        assert np.array_equal(got[k][kg], ref[k][kr]), f"{label}: {k} differs at rows {np.flatnonzero((got[k][kg] != ref[k][kr]).reshape(int(kg.sum()), -1).any(axis=1))[:8]}"
    worst = 0.0
    for k in FLOAT_COLUMNS:
        if k in ref:
            worst = max(worst, close(got[k][kg], ref[k][kr], rtol, atol, f"{label}: {k}"))
    identical = all(np.array_equal(got[k][kg], ref[k][kr], equal_nan=True) for k in FLOAT_COLUMNS if k in ref)
    if case["outputdt"]:
        assert rec is not None and len(rec.obs) == len(res["obs"]), f"{label}: {len(rec.obs)} observations vs {len(res['obs'])}"
        for j, ((tm, ids, x, y, z, t), (otm, o)) in enumerate(zip(rec.obs, res["obs"])):
            kg, kr = rows(ids), rows(o["particle_id"])
            assert tm == otm, f"{label}: observation {j} at {tm} vs {otm}"
            assert np.array_equal(ids[kg], o["particle_id"][kr]), f"{label}: ids of observation {j}"
            assert np.array_equal(t[kg], o["t"][kr]), f"{label}: t of observation {j}"
            for k, v in (("x", x), ("y", y), ("z", z)):
                worst = max(worst, close(v[kg], o[k][kr], rtol, atol, f"{label}: {k} of observation {j}"))
                identical = identical and np.array_equal(v[kg], o[k][kr], equal_nan=True)
    print(f"{label} err={gerr} slim={int(slim.sum())} largest deviation {worst:.2e} of the bar's scale, bit-identical={identical}")


@pytest.mark.parametrize("seed", range(int(os.environ.get("PARCELS_UX_FUZZ_POINT_SEEDS", "30"))))
def test_random_ux_points_match_oracle(gpu, seed):
    """pk_eval (scalar fields of the four kinds, UV, UVW) and pk_search at interior points, nodes, edge midpoints, points outside the
    mesh and in its hole, z on / above / below the levels, NaN and +-inf: values at rtol 1e-13, state codes with PK_EVAL_MASKED and
    `ei` exactly"""
    case, pts = ux_cases.draw_points(seed)
    orc = ux_oracle.UxOracle(case, "rounded", "device")
    fs = ux_fieldset(case)
    eng = fs._engine_or_create()
    t, z, y, x = pts["t"], pts["z"], pts["y"], pts["x"]
    want_ei, slim = orc.search_points(z, y, x)
    want = {}
    for what in POINT_FIELDS:
        want[what] = orc.eval_points(what, t, z, y, x)
        slim = slim | want[what]["slim"]
    if case["mesh"] != "spherical":
        slim = np.zeros(len(x), bool)  # flat: no exclusions
    assert slim.mean() <= SLIM_CAP, f"seed {seed}: {slim.sum()} points slim"
    keep = ~slim
    label = f"seed {seed}: {case['mesh']}/{case['region']} faces={len(case['faces'])} nt={len(case['time_s'])}"
    assert np.array_equal(eng.search(0, z, y, x)[keep], want_ei[keep]), f"{label}: pk_search"
    worst = 0.0
    for what in POINT_FIELDS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vals = eng.sample(what, t, z, y, x)
        w = want[what]
        assert np.array_equal(np.asarray(eng.last_sample_state)[keep], w["state"][keep]), f"{label}: state of {what}"
        assert np.array_equal(np.asarray(eng.last_sample_masked)[keep], w["masked"][keep]), f"{label}: masked flag of {what}"
        for k, b in enumerate(w["values"]):
            np.testing.assert_allclose(vals[k][keep], b[keep], rtol=1e-13, atol=0, equal_nan=True, err_msg=f"{label}: {what} component {k}")
            worst = max(worst, max_rel(vals[k][keep], b[keep]))
    print(f"{label} slim={int(slim.sum())} largest relative deviation {worst:.2e}")
