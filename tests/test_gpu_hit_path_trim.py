"""The stage weights of the level-pair kernel as one fused operation (csrc/pk_fast_agrid.h: fma3s).

The kernels that keep their block in registers (option "block_cache" 2, float64 particle storage) accumulate the Runge-Kutta sum of the looped
stages as su = fma(wgt, u, su) with wgt = 2 or 1; option 0 goes on computing su + 2*u and su + u.  2*u is exact below 2^1023, so the two round
the same exact sum once and agree in every bit: each case goes through tests/test_gpu_level_pair_cache.py::_check (cache vs registers at
rtol 0 on every column and counter; cache vs the general program and the CPU oracle at that file's tolerances).  The cases are those in
which a weighted sum could differ or a zeroed stage could be lost: velocities from subnormal to 1e3 m/s with both signs and both zeros,
lanes that leave the grid in a looped stage and keep their row (their dx, dy are sums with a stage that counts 0), partial wavefronts,
non-finite positions, float32 particle storage (whose instantiations keep the old form).  (No stage takes `tau` from the stage before it: that
step was not built, so there are no time-sharing cases here; tests/test_gpu_block_registers.py holds those of the time record.)"""

from __future__ import annotations

import numpy as np
import pytest

from case_utils import run_oracle
from test_gpu_level_pair_cache import _check


def _small(name, **kw):
    from oracle import cases

    args = dict(mesh="spherical", kernels=["AdvectionRK4"], nx=12, ny=9, nz=3, nt=4, npart=600, seed=9)
    args.update(kw)
    return cases.rect_agrid_case(name, **args)


def _wide_magnitudes(case, seed=4):
    """U and V node by node: a power of ten from the subnormal 1e-310 to 1e3 m/s, either sign; one node in six holds 0.0 or -0.0"""
    rng = np.random.default_rng(seed)
    expo = np.array([-310.0, -308.0, -300.0, -200.0, -100.0, -30.0, -8.0, -3.0, -1.0, 0.0, 1.0, 2.0, 3.0])
    prob = np.array([3, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 4, 6], dtype=np.float64)
    for k in ("U", "V"):
        f = case["fields"][k]
        with np.errstate(under="ignore"):
            mag = np.power(10.0, rng.choice(expo, size=f.shape, p=prob / prob.sum()))
        val = np.where(rng.random(f.shape) < 0.5, -mag, mag)
        r = rng.random(f.shape)
        val = np.where(r < 1 / 12, 0.0, np.where(r < 1 / 6, -0.0, val))
        f[...] = val
        assert (np.abs(f[f != 0]).min() < 2.3e-308) and np.abs(f).max() == 1e3 and (f == 0).sum() > 50
        assert np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all()
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("delete", [True, False])
def test_weights_over_all_magnitudes(gpu, delete):
    """Subnormal, tiny, ordinary and huge velocities beside exact zeros of both signs in the cells of one field.  With DeleteParticle the lanes
    that leave the grid go; without it the run ends with the reference's error and those lanes keep their row: the dx and dy of a lane that left
    in stage 2, 3 or 4 are formed from a sum in which that stage counts as 0, and are compared like every other column."""
    case = _wide_magnitudes(_small("hp_weights_%d" % delete, kernels=["AdvectionRK4", "DeleteParticle"] if delete else ["AdvectionRK4"], margin=0.02,
                                   runtime=6 * 3600.0))
    n, lon, lat = len(case["x"]), case["lon"], case["lat"]
    rng = np.random.default_rng(12)
    # a third of the rows start within a fifth of a cell of the east side, a sixth near the north side: in reach of a looped stage of the first step
    case["x"][::3] = rng.uniform(lon[-1] - 6.0, lon[-1] - 0.01, len(case["x"][::3]))
    case["y"][1::6] = rng.uniform(lat[-1] - 4.0, lat[-1] - 0.01, len(case["y"][1::6]))
    assert n == 600
    if delete:
        on, stats = _check(case)
        assert 50 < len(on["x"]) < 600 - 50, "some particles were to leave the grid and some to stay"
    else:
        _, eref, _ = run_oracle(case)
        assert eref is not None, "no error in the reference: the test does not test"
        on, stats = _check(case, expect_error=eref)
        bad = on["state"] >= 50
        assert bad.sum() > 20 and ((on["dx"][bad] != 0) | (on["dy"][bad] != 0)).sum() > 10, "no errored lane kept a displacement: the test does not test"


@pytest.mark.gpu
@pytest.mark.parametrize("npart", [1, 63, 65, 130])
def test_partial_wavefronts(gpu, npart):
    """One lane, a wavefront short of one lane, one lane in a second wavefront, two lanes in a third"""
    case = _wide_magnitudes(_small("hp_n%d" % npart, npart=npart, kernels=["AdvectionRK4", "DeleteParticle"], runtime=4 * 3600.0), seed=6)
    _check(case)


@pytest.mark.gpu
def test_non_finite_positions_among_good_ones(gpu):
    """NaN and infinite coordinates in a few lanes: every stage of theirs counts 0 and they end as errors; their neighbours do not notice"""
    case = _small("hp_nan", npart=200, kernels=["AdvectionRK4", "DeleteParticle"], runtime=6 * 3600.0)
    case["x"][3] = np.nan
    case["y"][70] = np.nan
    case["x"][71] = case["y"][71] = np.nan
    case["x"][130] = np.inf
    case["y"][131] = -np.inf
    on, stats = _check(case)
    assert len(on["x"]) == 200 - 5 and stats["steps"] == 195 * 6


@pytest.mark.gpu
def test_float32_particle_storage(gpu):
    """The instantiations for float32 storage keep su + 2*u: they still agree with option 0, the general program and the oracle"""
    case = _wide_magnitudes(_small("hp_f32", spatial_dtype="float32", kernels=["AdvectionRK4", "DeleteParticle"], runtime=5 * 3600.0), seed=7)
    _check(case, rtol=5e-7)
