"""CPU: the fuzz fixtures of named vector fields (tests/golden/named_vectors_fuzz, written by tools/make_named_vector_golden.py --fuzz from
the seeded generator tests/named_vector_fuzz.py) -- every seed has one, the reference reproduces each bit for bit, few first draws were
refused, and the manifest shows that the draws reach every branch of eval_vec and of the dispatch the GPU fuzz is there to witness."""
import json
import os
import sys

import numpy as np
import pytest

import named_vector_fuzz as nf
import named_vector_utils as nu
from oracle import ref_shim

needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = nf.load_manifest()
ROWS = {int(s): r for s, r in MANIFEST["seeds"].items()}
USED = {s: r for s, r in ROWS.items() if r["sub"] is not None}


def test_the_table_of_module_shapes_is_small_and_fixed():
    assert len(nf.SHAPES) <= 16
    for s in nf.SHAPES:  # all components of one vector share a dtype (one entry), WindDetached only where the vector's grid is rectilinear
        assert 1 <= len(s["vecs"]) <= 2 and all(v["ncomp"] in (2, 3) for v in s["vecs"])
        if "WindDetached" in s["kernels"]:
            assert all(nf.vector_kind(s, v) == 0 for v in s["vecs"])
        assert all(v["interp"] == "lin" or v["ncomp"] == 2 or s["w"] for v in s["vecs"])


def test_every_seed_has_a_fixture_and_a_manifest_row():
    assert sorted(ROWS) == list(nf.SEEDS) == list(range(64))
    files = sorted(f for f in os.listdir(nf.FUZZ_DIR))
    assert files == sorted([f"nvf_{s}.npz" for s in USED] + ["manifest.json"])
    total = 0
    for f in files:
        size = os.path.getsize(os.path.join(nf.FUZZ_DIR, f))
        total += size
        assert size <= 64 * 1024, (f, size)
    assert total <= 1.5 * 1024 * 1024
    for s, r in USED.items():
        z = np.load(nf.fixture_path(s), allow_pickle=False)  # arrays and one JSON string
        assert all(k == "meta" or k.startswith("out__") for k in z.files) and json.loads(str(z["meta"]))["sub"] == r["sub"]
        assert r["dims"]["npart"] in nf.COUNTS and r["dims"]["npart"] <= 300 and r["dims"]["nsteps"] <= nf.MAX_STEPS
        assert nf.draw(s, r["sub"])[1] == r["dims"]  # the manifest row is what the generator draws today
        assert len(r["refusals"]) == r["sub"] <= nf.MAX_SUB


def test_at_most_a_quarter_of_the_first_draws_were_refused():
    refused = [s for s, r in ROWS.items() if r["sub"] != 0]
    assert MANIFEST["first_draws_refused"] == len(refused) and 4 * len(refused) <= len(ROWS), refused
    for s in refused:
        assert ROWS[s]["refusals"] and all(x["why"] for x in ROWS[s]["refusals"])


def _count(pred):
    return sum(1 for r in USED.values() if pred(r["dims"], r))


def _vec(d, **want):
    return any(all(v[k] == x for k, x in want.items()) for v in d["vectors"])


def test_coverage_from_the_manifest_alone():
    unsupported = {(v["FT"], v["KIND"], v["INTERP"]) for u in MANIFEST["unsupported"] for v in u["vectors"] if len(u["vectors"]) == 1}
    for u in MANIFEST["unsupported"]:  # what the reference does not run is named with the exception it raised
        assert u["why"] and u["vectors"] and u["kernels"]
    hits = {}
    for ft in ("float", "double"):
        for kind in (0, 1):
            for interp in (0, 1, 2):
                hits[(ft, kind, interp)] = _count(lambda d, r: _vec(d, FT=ft, KIND=kind, INTERP=interp))
    missing = {k: n for k, n in hits.items() if n < 2 and k not in unsupported}
    assert not missing, missing
    assert {k for k, n in hits.items() if n < 2} <= unsupported
    for kind in (0, 1):
        assert _count(lambda d, r: _vec(d, KIND=kind, place="main")) >= 2
        assert _count(lambda d, r: any(v["KIND"] == kind and v["place"] != "main" for v in d["vectors"])) >= 2
    for mesh in ("flat", "spherical"):
        assert _count(lambda d, r: d["mesh"] == mesh) >= 2
    assert _count(lambda d, r: d["particles"] == "float32" and _vec(d, KIND=1)) >= 2
    assert _count(lambda d, r: any(v["ncomp"] == 3 and v["INTERP"] in (1, 2) for v in d["vectors"])) >= 2
    assert _count(lambda d, r: d["backward"]) >= 2
    assert _count(lambda d, r: d["staggered"]) >= 2
    assert _count(lambda d, r: _vec(d, place="rect2z")) >= 2
    assert _count(lambda d, r: len(d["vectors"]) == 2) >= 2
    assert _count(lambda d, r: d["detached"]) >= 2
    for n in nf.COUNTS:
        assert _count(lambda d, r: d["npart"] == n) >= 2, n
    assert _count(lambda d, r: r["oob_exit"] and d["delete"]) >= 2
    assert _count(lambda d, r: r["oob_exit"] and not d["delete"]) >= 2
    assert len({r["dims"]["shape"] for r in USED.values()}) <= 16


@needs_reference
@pytest.mark.parametrize("seed", nf.SEEDS)
def test_fuzz_fixture_is_reproduced_by_the_generator(seed):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_named_vector_golden as gen

    row, out, err = gen.run_fuzz_seed(seed)
    assert json.loads(json.dumps(row)) == ROWS[seed]
    if out is None:
        assert not os.path.exists(nf.fixture_path(seed))
        return
    ref, rerr = nu.load_fixture(None, nf.fixture_path(seed))
    assert err == rerr and set(out) == set(ref)
    for k in out:
        assert np.asarray(out[k]).dtype == ref[k].dtype and np.array_equal(np.asarray(out[k]), ref[k], equal_nan=True), k
