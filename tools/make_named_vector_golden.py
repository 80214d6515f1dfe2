"""Writes tests/golden/named_vectors/nv_*.npz: the cases of tests/named_vector_utils.py run by the REFERENCE's own ParticleSet.execute
(through oracle/ref_shim.py; needs the reference's sources), with the user kernels of tests/named_vector_kernels.py.  A fixture holds the
final particle columns, the name of the error the reference raised, and a JSON `meta` string -- arrays only, a few KB.

    python tools/make_named_vector_golden.py [case ...]         write the fixtures (all of them by default)
    python tools/make_named_vector_golden.py --check            compare the committed fixtures with a fresh run, bit for bit

A case is refused where reference and device cannot be expected to agree: a view evaluated with fewer
than 2 particles (NumPy's scalar paths), or -- where the searched grid is curvilinear -- a search after the first that sees no non-zero
guess in its batch (the reference then searches every particle through the hash)."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import named_vector_kernels as nk  # noqa: E402
import named_vector_utils as nu  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from oracle import ref_shim as rs  # noqa: E402


def build_ref_fieldset(spec):
    """The reference's Field / VectorField objects of a case: the currents as oracle/make_golden.py wires them, the named vectors added to
    that RefFieldSet; a second dataset is a second model on a second grid (igrid 1), like make_ref_fieldset's constant-field grid."""
    m = rs.load_reference()
    Field, VectorField, xi = m["field"].Field, m["field"].VectorField, m["xinterp"]
    fs, g = mg.build_ref_fieldset(spec["currents"])
    how = {"cgrid": xi.CGrid_Velocity, "free": xi.XFreeslip, "partial": xi.XPartialslip}
    for vname, comps in spec["vectors"].items():
        interp = how.get(spec.get("interp", {}).get(vname), xi.XLinear_Velocity)
        fs.fields[vname] = VectorField(vname, *[fs.fields[c] for c in comps], interp_method=interp())
    s = spec.get("second")
    if s:
        g2 = rs.make_ref_grid(lon=s["lon"], lat=s["lat"], depth=None, mesh=s["mesh"])
        ts = np.asarray(s["time_s"], dtype=float)
        t64 = (ts * 1e9).round().astype("int64").astype("timedelta64[ns]")
        tint = m["time"].TimeInterval(t64[0], t64[-1])
        data = {}
        for name, arr in s["fields"].items():
            data[name] = rs.DA(np.asarray(arr), dims=tuple(s["field_dims"][name]))
            data[name].coords = {"time": rs.DA(t64, dims=("time",))}
        model = rs._FakeModel(g2, data, tint)
        for name in data:
            f = Field(name, model)
            f.igrid = 1
            f.interp_method = xi.XLinear()
            fs.fields[name] = f
        fs.gridset.append(g2)
        for vname, comps in s["vectors"].items():
            fs.fields[vname] = VectorField(vname, *[fs.fields[c] for c in comps], interp_method=xi.XLinear_Velocity())
    for k, v in spec["context"].items():
        fs.add_context(k, v)
    return fs


class _Watch:
    """Wraps the reference's grid search while a case runs: the size of every evaluated batch and, on a curvilinear grid, whether the
    searches after the first of each grid saw a non-zero guess."""

    def __init__(self):
        self.problems = []

    def __enter__(self):
        m = rs.load_reference()
        self.XGrid = m["xgrid"].XGrid
        self.orig = self.XGrid.search
        seen = {}
        watch = self

        def search(grid, z, y, x, ei=None):
            n = np.size(x)
            if n < 2:
                watch.problems.append(f"a view of {n} particle(s) was evaluated")
            if np.asarray(grid.lon).ndim == 2:
                k = seen.get(id(grid), 0)
                seen[id(grid)] = k + 1
                if k > 0 and (ei is None or not np.any(ei)):
                    watch.problems.append(f"search {k} on the curvilinear grid saw no non-zero guess")
            return watch.orig(grid, z, y, x, ei)

        self.XGrid.search = search
        return self

    def __exit__(self, *a):
        self.XGrid.search = self.orig
        return False


def run_reference(spec):
    m = rs.load_reference()
    fs = build_ref_fieldset(spec)
    kl = [getattr(nk, k) if hasattr(nk, k) else getattr(m["kernels"], k) for k in spec["kernels"]]
    c = spec["currents"]
    extra = [(vn, np.dtype(dt).type, 0) for vn, dt in spec.get("variables", ())] or None
    with _Watch() as w:
        out, err = rs.run_reference(fs, kl, x=np.asarray(c["x"]), y=np.asarray(c["y"]), z=np.asarray(c["z"]), t=None, dt=float(c["dt"]),
                                    runtime=float(c["runtime"]), spatial_dtype=np.dtype(c["spatial_dtype"]).type, extra_vars=extra)
    if w.problems:
        raise SystemExit(f"{c['name']}: refused -- {sorted(set(w.problems))}")
    return out, err


def main(argv):
    check = "--check" in argv
    names = [a for a in argv if not a.startswith("--")]
    specs = nu.all_cases()
    os.makedirs(nu.GOLDEN_DIR, exist_ok=True)
    bad = 0
    for name in names or list(specs):
        out, err = run_reference(specs[name])
        if check:
            ref, rerr = nu.load_fixture(name)
            same = rerr == err and set(ref) == set(out) and all(np.array_equal(ref[k], np.asarray(out[k]), equal_nan=True) for k in out)
            print(f"{name}: {'reproduced' if same else 'DIFFERS'}")
            bad += not same
        else:
            nu.save_fixture(nu.fixture_path(name), out, err, {"kernels": specs[name]["kernels"]})
            states = dict(zip(*np.unique(out["state"], return_counts=True)))
            print(f"{name}: n={len(out['x'])} err={err} states={ {int(k): int(v) for k, v in states.items()} } "
                  f"{os.path.getsize(nu.fixture_path(name))} bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
