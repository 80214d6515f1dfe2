"""Every host-side operation on the device-resident particle columns (allocate, copy, sort, checkpoint, snapshot, compact, host order,
the keep-unstepped-rows copy of a launch) moves every column of the schema, at its element size and width, to the row it belongs to.

A characterisation test of the column plumbing of libparcels_hip.so: the expected values come from the NumPy input columns alone --
round trips are identities, compaction is ``arr[state != Delete]``, the filtered snapshot is the rows the host filter of particlefile.py
selects -- and every comparison is bit-exact.  Each case runs once on host-ordered device rows and once on rows a cell sort permuted."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from case_utils import build_fieldset

pytestmark = pytest.mark.gpu

EXTRAS = (("e32", np.float32), ("e64", np.float64), ("i64", np.int64))  # schema (b): device Variables of 4 and 8 bytes
SUCCESS, EVALUATE, DELETE, STOP = 0, 10, 30, 40
DT = 3600.0


@pytest.fixture(scope="module")
def engines(gpu):
    """{ngrids: engine} over a zero velocity field (positions stay put); ngrids = 2: a constant field brings a grid of its own."""
    from oracle import cases

    out = {}
    for ngrids in (1, 2):
        case = cases.rect_agrid_case("column_table", mesh="flat", kernels=["AdvectionRK4"], seed=5, npart=1, nt=2)
        for f in case["fields"].values():
            f[...] = 0.0
        if ngrids == 2:
            case["constants"] = {"Cst": 1.0}
            case["const_mesh"] = "flat"
        fs = build_fieldset(case)
        assert len(fs.gridset) == ngrids
        fs.to_device(0)
        assert not fs._engine.windowed
        out[ngrids] = (case, fs._engine)
    return out


def _columns(case, eng, ngrids, with_optional, sdt, n):
    """Distinct values per row and per column, and still a particle set a launch may step: positions inside the grid, valid `ei`."""
    rng = np.random.default_rng(100 * n + ngrids)
    i = np.arange(n, dtype=np.float64)
    lon, lat = np.asarray(case["lon"]), np.asarray(case["lat"])
    d = {
        "t": (i + 0.25) / (n + 1),
        "z": rng.uniform(200, 4800, n).astype(sdt),
        "y": rng.uniform(lat[0] + 0.2 * (lat[-1] - lat[0]), lat[-1] - 0.2 * (lat[-1] - lat[0]), n).astype(sdt),
        "x": rng.uniform(lon[0] + 0.2 * (lon[-1] - lon[0]), lon[-1] - 0.2 * (lon[-1] - lon[0]), n).astype(sdt),
        "dz": ((i + 1) * 1e-9).astype(sdt),
        "dy": ((i + 1) * 2e-9).astype(sdt),
        "dx": ((i + 1) * 3e-9).astype(sdt),
        "dt": DT + i / (n + 1),
        "state": rng.choice(np.array([SUCCESS, EVALUATE, STOP], np.int32), n),
        "ei": np.zeros((n, ngrids), np.int32),
        "particle_id": 10_000 + 7 * np.arange(n, dtype=np.int64),
    }
    for g in range(ngrids):
        d["ei"][:, g] = eng.search(g, d["z"], d["y"], d["x"])
    if with_optional:
        d["next_dt"] = 1800.0 + 0.5 * i
        d["e32"] = (0.5 * i + 0.125).astype(np.float32)
        d["e64"] = -1.25 * i - 0.5
        d["i64"] = (1 << 40) + 3 * np.arange(n, dtype=np.int64)
    return d


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _clobber(data, keys=None):
    for k in (data if keys is None else keys):
        data[k].reshape(-1).view(np.uint8)[...] = 0xA5


def _clobbered(a):
    return bool(np.all(a.reshape(-1).view(np.uint8) == 0xA5))


def _launch(eng, *, reset_state, sort, endtime=DT):
    import parcels_amd as pa
    from parcels_amd import _hip
    from parcels_amd import kernels as _k

    prm = eng.make_params([_k.kernel_id(pa.AdvectionRK4)], endtime=endtime, dt0=DT, reset_state=reset_state, sort_by_cell=int(sort))
    st = _hip.ExecStats()
    eng.ctx.check(eng.lib.pk_execute_begin(eng.ctx.handle, C.byref(prm)), "pk_execute_begin")
    eng.ctx.check(eng.lib.pk_execute_end(eng.ctx.handle, C.byref(st)), "pk_execute_end")
    return st


def _device_view(eng, names):
    """pk_particles_device: (rows are cell-sorted, the descriptor).  It hands out the named columns; `extra` and n_extra stay the caller's."""
    from parcels_amd import _hip

    d, perm = _hip.ParticlesDesc(), C.c_void_p()
    d.n_extra = 77
    for k in range(_hip.PK_MAX_EXTRA):
        d.extra[k] = 0x1000 + k
    eng.ctx.check(eng.lib.pk_particles_device(eng.ctx.handle, C.byref(d), C.byref(perm)), "pk_particles_device")
    assert d.n_extra == 77 and [d.extra[k] for k in range(_hip.PK_MAX_EXTRA)] == [0x1000 + k for k in range(_hip.PK_MAX_EXTRA)]
    for name in _hip.COLUMN_BITS:
        assert bool(getattr(d, name)) == (name in names), name
    ptrs = [getattr(d, name) for name in _hip.COLUMN_BITS if name in names]
    assert len(set(ptrs)) == len(ptrs)
    return bool(perm.value), d


def _upload(eng, data, exp, changes):
    """The host arrays become `exp` with `changes` applied (exp follows); only the changed columns go up."""
    for k, v in changes.items():
        exp[k] = np.ascontiguousarray(v, dtype=exp[k].dtype)
    for k in data:
        data[k][...] = exp[k]
    eng.h2d_columns(list(changes))


def _download_equals(eng, data, exp, label):
    _clobber(data)
    eng.d2h()
    for k in exp:
        assert _same_bits(data[k], exp[k]), (label, k)


@pytest.mark.parametrize("sort", [False, True], ids=["host_order", "cell_sorted"])
@pytest.mark.parametrize("n", [0, 1, 257, 1000])
@pytest.mark.parametrize("sdt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("schema", ["a", "b"])
def test_every_column_operation_moves_every_column(engines, schema, sdt, n, sort):
    from parcels_amd.particlefile import _to_write_particles

    ngrids = 1 if schema == "a" else 2
    case, eng = engines[ngrids]
    eng.device_variables = [name for name, _ in EXTRAS] if schema == "b" else []
    exp = _columns(case, eng, ngrids, schema == "b", sdt, n)
    assert [exp[name].dtype for name, dt in EXTRAS if schema == "b"] == [np.dtype(dt) for _, dt in EXTRAS if schema == "b"]
    data = {k: v.copy() for k, v in exp.items()}
    names = list(exp)
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.float64)

    # 1. full h2d, full d2h, d2h of a subset -- in the sorted variant with a sorting launch in between: the launch rewrites the columns, so
    # every column then goes up again through h2d_columns, into the permuted rows
    eng.bind_particles(data)
    eng.h2d()
    if sort:
        st = _launch(eng, reset_state=1, sort=True)
        assert st.steps >= n
        _upload(eng, data, exp, {k: exp[k] for k in names})
    _download_equals(eng, data, exp, "h2d/d2h")
    permuted, d = _device_view(eng, names)
    assert permuted == (sort and n >= 2) and (d.n, d.ngrids) == (n, ngrids)
    subset = ["x", "state", "particle_id"] + (["e32", "i64"] if schema == "b" else [])
    _clobber(data)
    eng.d2h(subset)
    for k in names:
        assert _same_bits(data[k], exp[k]) if k in subset else (_clobbered(data[k]) or n == 0), ("d2h subset", k)

    # 2. h2d_columns of a 4-byte and an 8-byte column
    _upload(eng, data, exp, {"state": rng.choice(np.array([SUCCESS, STOP, EVALUATE], np.int32), n), "particle_id": exp["particle_id"][::-1] + 1})
    _download_equals(eng, data, exp, "h2d_columns")

    # 3. checkpoint, a launch that steps every particle (h2d_columns would discard the checkpoint: a launch is what it is for), restore
    eng.ctx.check(eng.lib.pk_particles_checkpoint(eng.ctx.handle), "pk_particles_checkpoint")
    st = _launch(eng, reset_state=1, sort=False)
    assert st.steps >= n
    if n:
        _clobber(data)
        eng.d2h(["t"])
        assert not _same_bits(data["t"], exp["t"])  # the launch did change the columns
    eng.ctx.check(eng.lib.pk_particles_restore(eng.ctx.handle), "pk_particles_restore")
    _download_equals(eng, data, exp, "checkpoint/restore")

    # 4. plain and filtered snapshot, extras included.  The filter (particlefile.py:198-221): |t - T| <= |dt| / 2 and t finite, or dt NaN and
    # t == T -- half of the rows lie far from T, and where there is room one t is NaN and two dt are NaN (one of them at t == T)
    t_out = 0.5
    t_new = np.where(np.arange(n) % 2 == 0, exp["t"], 1e6 + i)
    dt_new = exp["dt"].copy()
    if n >= 4:
        t_new[1], t_new[2], t_new[3] = np.nan, t_out, 0.25
        dt_new[2] = dt_new[3] = np.nan
    _upload(eng, data, exp, {"t": t_new, "dt": dt_new})
    eng.snapshot_begin(names, 0)
    got = eng.snapshot_wait(0)
    assert sorted(got) == sorted(names)
    for k in names:
        assert _same_bits(got[k], exp[k]), ("snapshot", k)
    idx = _to_write_particles(exp, t_out)
    assert n < 4 or 0 < len(idx) < n
    eng.snapshot_begin(names, 1, filter_t=t_out)
    got = eng.snapshot_wait(1)
    for k in names:
        assert _same_bits(got[k], exp[k][idx]), ("filtered snapshot", k)

    # 5. compaction: about a third of the rows are in state Delete
    state = rng.choice(np.array([SUCCESS, STOP], np.int32), n)
    state[1::3] = DELETE
    _upload(eng, data, exp, {"state": state})
    keep = exp["state"] != DELETE
    data = eng.compact_deleted(data)
    exp = {k: np.ascontiguousarray(v[keep]) for k, v in exp.items()}
    assert all(len(data[k]) == int(keep.sum()) for k in names)
    _download_equals(eng, data, exp, "compact")

    # 6. device rows back in host order
    eng.ctx.check(eng.lib.pk_interact_host_order(eng.ctx.handle), "pk_interact_host_order")
    _download_equals(eng, data, exp, "host order")

    # 7. a continued launch (reset_state = 0) in which no row is in state Evaluate: nobody steps, and every column the launch writes
    # comes back as it was (the keep-unstepped-rows copy) -- in the sorted variant after another sort
    _upload(eng, data, exp, {"state": rng.choice(np.array([SUCCESS, STOP], np.int32), len(exp["state"]))})
    st = _launch(eng, reset_state=0, sort=sort)
    assert st.steps == 0
    assert _device_view(eng, names)[0] == (sort and len(exp["t"]) >= 2)
    _download_equals(eng, data, exp, "unstepped launch")
