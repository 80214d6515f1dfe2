"""GPU: differential fuzz of named vector fields.  Every seed of tests/named_vector_fuzz.py runs as one compiled list in the kernel-list
interpreter and is compared with the fixture the REFERENCE wrote for it (tests/golden/named_vectors_fuzz; the only witness that shares no
device function with the code under test): the error raised, state, `ei` of every grid, t, ids and order exactly, positions and sampled
Variables in the project's tolerance classes (case_utils.tolerance_for: 1e-12 for float64, 5e-7 for float32 particles).  The same run on
the host path (PARCELS_AMD_JIT=0) and through a ring of 2 or 3 level slots gives the compiled, resident columns bit for bit."""
import numpy as np
import pytest

import named_vector_fuzz as nf
import named_vector_utils as nu
from case_utils import compare, tolerance_for

pytestmark = pytest.mark.gpu
PROG_GENERIC = 2  # include/parcels_hip.h: pk_exec_stats.program -- the kernel-list interpreter
ROWS = {int(s): r for s, r in nf.load_manifest()["seeds"].items()}


def _same_columns(a, b, label):
    assert set(a) == set(b), label
    for c in a:
        assert a[c].dtype == b[c].dtype and a[c].shape == b[c].shape and np.array_equal(a[c], b[c], equal_nan=True), (label, c, np.flatnonzero(a[c] != b[c])[:5])


@pytest.mark.parametrize("seed", [s for s in nf.SEEDS if ROWS[s]["sub"] is not None])  # (left out: only what the generator refuses on the CPU)
def test_seed(gpu, seed):
    spec = nf.draw_spec(seed)
    name = f"nvf_{seed}"
    pset, got, err = nu.run_case(spec)
    k = pset._kernel
    assert k.jit_report.startswith("compiled") and k.host_functions == [], k.jit_report
    prog = k.user_program
    assert prog.vectors and "PK_USER_VECTORS" in prog.source and not prog.flags & 1
    assert [v[0] for v in prog.vectors] and {v[0] for v in prog.vectors} == {v["name"] for v in ROWS[seed]["dims"]["vectors"]}
    for v in prog.vectors:  # the dispatch instantiates what the manifest's coverage counts
        d = next(x for x in ROWS[seed]["dims"]["vectors"] if x["name"] == v[0])
        assert (v[4], v[5], min(v[6], 2)) == (d["FT"], d["KIND"], d["INTERP"]) and (v[3] >= 0) == (d["ncomp"] == 3), (v, d)
    assert pset._last_stats["program"] == PROG_GENERIC and not pset._last_stats.get("hosted"), pset._last_stats
    ref, rerr = nu.load_fixture(None, nf.fixture_path(seed))
    assert err == rerr, (err, rerr)
    assert got["ei"].shape == ref["ei"].shape and got["ei"].shape[1] == (2 if spec.get("second") else 1)
    compare(got, ref, rtol=tolerance_for(name, spec["currents"]), check_state="all", label=name, skip=())
    ph, host, herr = nu.run_case(spec, jit=False)
    assert ph._kernel.user_program is None and ph._kernel.jit_report == "PARCELS_AMD_JIT=0" and herr == err
    _same_columns(got, host, name + " host path")
    if min(ROWS[seed]["dims"]["time_levels"]) >= 3:
        # (a ring of 2 holds one level interval; releases staggered over a whole interval need the next one too: tests/test_gpu_streaming.py)
        levels = ROWS[seed]["dims"]["time_levels"]
        nslots = 3 if ROWS[seed]["dims"]["staggered"] else 2 + seed % 2
        if nslots >= max(levels):  # (three levels on every axis: only a ring of 2 is a ring)
            nslots = 2
        pr, ring, rerr2 = nu.run_case(spec, nslots=nslots)
        assert rerr2 == err and pr._kernel.jit_report.startswith("compiled")
        eng = pr.fieldset._engine
        assert all(eng.field_nslots[f] == min(nslots, eng.field_host[f].shape[0]) for f in eng.field_nslots)
        assert nslots < max(levels) and eng.windowed  # some field does stream through its ring
        _same_columns(ring, got, f"{name} ring of {nslots}")

