"""Writes tests/golden/named_vectors/nv_*.npz: the cases of tests/named_vector_utils.py run by the REFERENCE's own ParticleSet.execute
(through oracle/ref_shim.py; needs the reference's sources), with the user kernels of tests/named_vector_kernels.py.  A fixture holds the
final particle columns, the name of the error the reference raised, and a JSON `meta` string -- arrays only, a few KB.

    python tools/make_named_vector_golden.py [case ...]         write the fixtures (all of them by default)
    python tools/make_named_vector_golden.py --check            compare the committed fixtures with a fresh run, bit for bit
    python tools/make_named_vector_golden.py --fuzz [--check]   the same for tests/golden/named_vectors_fuzz/nvf_<seed>.npz + manifest.json:
                                                                the seeded draws of tests/named_vector_fuzz.py; a refused draw moves to the
                                                                next sub-draw of its seed, and the manifest says what was refused and why

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
        sizes_extra = {d: n for name, dims in s["field_dims"].items() for d, n in zip(dims, np.asarray(s["fields"][name]).shape) if d in ("XC", "YC", "ZC")}
        g2 = rs.make_ref_grid(lon=s["lon"], lat=s["lat"], depth=s.get("depth"), mesh=s["mesh"], x_pad=s.get("x_pad", "low"), y_pad=s.get("y_pad", "low"),
                              z_pad=s.get("z_pad", "both"), sizes_extra=sizes_extra)
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
            interp = how.get(s.get("interp", {}).get(vname), xi.XLinear_Velocity)
            fs.fields[vname] = VectorField(vname, *[fs.fields[c] for c in comps], interp_method=interp())
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


class Refused(Exception):
    """The case is one reference and device cannot be expected to agree on (or one the reference does not run)."""


class Unsupported(Exception):
    """The reference does not run the combination: it raised on setup, or its execute gave up with something that is no particle error."""


def run_reference(spec):
    m = rs.load_reference()
    fs = build_ref_fieldset(spec)
    kl = [getattr(nk, k) if hasattr(nk, k) else getattr(m["kernels"], k) for k in spec["kernels"]]
    c = spec["currents"]
    extra = [(vn, np.dtype(dt).type, 0) for vn, dt in spec.get("variables", ())] or None
    with _Watch() as w:
        try:  # (only the reference's own ParticleSet / execute setup: a mistake in the wiring above is not a refusal)
            out, err = rs.run_reference(fs, kl, x=np.asarray(c["x"]), y=np.asarray(c["y"]), z=np.asarray(c["z"]), t=c.get("t0"), dt=float(c["dt"]),
                                        runtime=float(c["runtime"]), spatial_dtype=np.dtype(c["spatial_dtype"]).type, extra_vars=extra)
        except (ValueError, NotImplementedError) as e:  # what the reference raises for arguments and combinations it refuses
            raise Unsupported(f"{type(e).__name__}: {e}"[:300]) from None
    if err is not None and err not in nu.ERRORS:  # (not a particle's error code: the reference's loop itself gave up)
        raise Unsupported(f"{err} raised by the reference's execute")
    if w.problems:
        raise Refused(f"{c['name']}: refused -- {sorted(set(w.problems))}")
    return out, err


def run_fuzz_seed(seed):
    """The first sub-draw of a seed the reference runs and _Watch lets pass -> (manifest row, final columns, error name); the columns are
    None where every sub-draw was refused."""
    import named_vector_fuzz as nf

    refusals = []
    for sub in range(nf.MAX_SUB + 1):
        spec, dims = nf.draw(seed, sub)
        try:
            out, err = run_reference(spec)
        except Refused as e:
            refusals.append(dict(sub=sub, kind="refused", why=str(e).split(" -- ", 1)[-1]))
            continue
        except Unsupported as e:
            refusals.append(dict(sub=sub, kind="unsupported", why=str(e)))
            continue
        state = np.asarray(out["state"])
        left = bool(len(state) < dims["npart"]) if dims["delete"] else bool(np.any((state == 60) | (state == 61)))
        row = dict(sub=sub, refusals=refusals, dims=dims, err=err, n_final=int(len(state)), oob_exit=left,
                   states={str(int(k)): int(v) for k, v in zip(*np.unique(state, return_counts=True))})
        return row, out, err
    return dict(sub=None, refusals=refusals, dims=nf.draw(seed, 0)[1], err=None, n_final=None, oob_exit=False, states={}), None, None


def _same(ref, rerr, out, err):
    return rerr == err and set(ref) == set(out) and all(np.asarray(out[k]).dtype == ref[k].dtype and np.array_equal(ref[k], np.asarray(out[k]), equal_nan=True)
                                                          for k in out)


def fuzz_main(check):
    """--fuzz: write tests/golden/named_vectors_fuzz/nvf_<seed>.npz and manifest.json; with --check compare them with a fresh run."""
    import json

    import named_vector_fuzz as nf

    os.makedirs(nf.FUZZ_DIR, exist_ok=True)
    rows, bad = {}, 0
    for seed in nf.SEEDS:
        row, out, err = run_fuzz_seed(seed)
        rows[str(seed)] = row
        if check:
            same = (out is None and not os.path.exists(nf.fixture_path(seed))) or (out is not None and os.path.exists(nf.fixture_path(seed))
                                                                                    and _same(*nu.load_fixture(None, nf.fixture_path(seed)), out, err))
            print(f"nvf_{seed}: {'reproduced' if same else 'DIFFERS'}")
            bad += not same
        elif out is not None:
            nu.save_fixture(nf.fixture_path(seed), out, err, {"kernels": row["dims"]["kernels"], "seed": seed, "sub": row["sub"]})
            print(f"nvf_{seed}: sub={row['sub']} n={row['dims']['npart']}->{row['n_final']} err={err} states={row['states']} "
                  f"{os.path.getsize(nf.fixture_path(seed))} bytes" + (f" refused: {[r['why'] for r in row['refusals']]}" if row["refusals"] else ""))
        else:
            print(f"nvf_{seed}: every sub-draw refused: {[r['why'] for r in row['refusals']]}")
    unsupported = [dict(seed=int(s), shape=r["dims"]["shape"], vectors=r["dims"]["vectors"], kernels=r["dims"]["kernels"], why=x["why"])
                   for s, r in rows.items() for x in r["refusals"][:1] if r["sub"] is None and x["kind"] == "unsupported"]
    manifest = dict(seeds=rows, unsupported=unsupported, first_draws_refused=sum(1 for r in rows.values() if r["sub"] != 0))
    if check:
        same = nf.load_manifest() == json.loads(json.dumps(manifest))
        print(f"manifest.json: {'reproduced' if same else 'DIFFERS'}")
        bad += not same
    else:
        with open(nf.MANIFEST, "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"first draws refused: {manifest['first_draws_refused']} of {len(rows)}; unsupported: {len(unsupported)}")
    return 1 if bad else 0


def main(argv):
    check = "--check" in argv
    if "--fuzz" in argv:
        return fuzz_main(check)
    names = [a for a in argv if not a.startswith("--")]
    specs = nu.all_cases()
    os.makedirs(nu.GOLDEN_DIR, exist_ok=True)
    bad = 0
    for name in names or list(specs):
        try:
            out, err = run_reference(specs[name])
        except Refused as e:
            raise SystemExit(str(e)) from None
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
