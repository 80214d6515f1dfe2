"""GPU: CF-packed integer levels unpacked on the device (csrc/pk_unpack.hip) -- every raw / compute / field dtype combination through
pk_field_upload_level_packed and back through pk_field_download_level against sources.unpack_reference bit for bit (unaligned slots,
chunk boundaries, blocking and async), packed groups, and whole runs that must equal the host-unpacked runs in every particle column."""

import ctypes as C
import os

import numpy as np
import pytest

import parcels_amd as pa
from case_utils import build_fieldset, build_pset
from parcels_amd import _hip
from parcels_amd.engine import _LazyLevels
from parcels_amd.sources import PackedArrayLevels, cf_packing, unpack_reference
from unpack_utils import all_values, assert_same_bits, write_int_zarr

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
PAIRS = [(f32(0.001), f32(2.0)), (f32(0.0006103702), f32(20.0))]  # an FMA changes thousands of int16 values (tests/test_unpack_host.py)
NT = 3


class Device:
    """One context for the direct tests: a small rectilinear grid (never searched) and fields of 3 levels in 3 slots made on demand."""

    def __init__(self):
        self.ctx = _hip.Context(0)
        self.lib = self.ctx.lib
        g = _hip.GridDesc()
        g.kind, g.has_x, g.has_y, g.nx, g.ny, g.xdim, g.ydim, g.deg2m = 0, 1, 1, 4, 4, 3, 3, 1.0
        self._axes = np.arange(4, dtype=np.float64)
        g.lon = g.lat = self._axes.ctypes.data_as(C.c_void_p)
        gid = C.c_int32(-1)
        self.ctx.check(self.lib.pk_grid_create(self.ctx.handle, C.byref(g), C.byref(gid)), "pk_grid_create")
        self.grid = gid.value
        self.fields = {}

    def field(self, n, dtype, ncomp=1, tag=""):
        """Field ids of a plain field (ncomp 1) or of the members of a packed group, `n` values per level."""
        key = (n, np.dtype(dtype).name, ncomp, tag)
        if key not in self.fields:
            ids = []
            for c in range(ncomp):
                d = _hip.FieldDesc()
                d.grid, d.dtype = self.grid, _hip.PK_F64 if np.dtype(dtype) == np.float64 else _hip.PK_F32
                d.nt, d.nz, d.ny, d.nx = NT, 1, 1, n
                d.has_t = d.has_z = d.has_y = d.has_x = 1
                d.nslots = NT
                d.pack_count = ncomp if (c == 0 and ncomp > 1) else 0
                d.pack_leader = ids[0] if c > 0 else -1
                t = np.arange(NT, dtype=np.float64)
                d.time = t.ctypes.data_as(C.c_void_p)
                fid = C.c_int32(-1)
                self.ctx.check(self.lib.pk_field_create(self.ctx.handle, C.byref(d), C.byref(fid)), "pk_field_create")
                ids.append(fid.value)
            self.fields[key] = ids
        return self.fields[key]

    def slots(self, fid):
        arr = (C.c_int32 * NT)()
        self.ctx.check(self.lib.pk_field_slots(self.ctx.handle, fid, arr, None), "pk_field_slots")
        return list(arr)

    def download(self, fid, level, n, dtype):
        out = np.full(n, 77, dtype=dtype)
        rc = self.lib.pk_field_download_level(self.ctx.handle, fid, level, out.ctypes.data_as(C.c_void_p))
        return rc, out

    def error(self):
        return self.lib.pk_last_error(self.ctx.handle).decode()


@pytest.fixture(scope="module")
def dev(gpu):
    d = Device()
    yield d
    d.ctx.close()


def raw_levels(dtype, n, seed):
    """NT levels of `n` raw values: every value of an 8 / 16-bit dtype (a seeded draw of int32), shifted per level, behind them a tail."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    base = all_values(dtype) if info.max < 70000 else rng.integers(info.min, info.max, n, endpoint=True).astype(dtype)
    reps = -(-n // len(base))
    return [np.ascontiguousarray(np.roll(np.tile(base, reps), 1000 * k + 7)[:n]) for k in range(NT)]


def attrs_for(raw_dtype, compute, k=0):
    if compute == f64:
        return {"scale_factor": 0.001 * (k + 1), "add_offset": 2.0 + k}  # float64 attributes
    if np.dtype(raw_dtype).itemsize == 4:
        return {"scale_factor": PAIRS[k % 2][0]}  # (an int32 variable with both float32 attributes is float64)
    return {"scale_factor": PAIRS[k % 2][0], "add_offset": PAIRS[k % 2][1]}


def packing_and_desc(raw, attrs, out_dtype, ntz):
    fills = np.asarray([raw[5], raw[len(raw) // 3]], dtype=raw.dtype)
    attrs = dict(attrs, _FillValue=fills)
    pk = cf_packing(raw.dtype, attrs)
    src = PackedArrayLevels(raw.reshape(1, 1, 1, -1), attrs.get("scale_factor"), attrs.get("add_offset"), fills, fill_nan=ntz)
    assert src.packing == pk and len(pk.fills) == 2
    return pk, _LazyLevels(src, out_dtype, fill_nan=ntz).pack_desc(pk)


COMBOS = [(f32, f32), (f32, f64), (f64, f64)]  # (compute dtype, field dtype)


@pytest.mark.parametrize("compute, out", COMBOS, ids=["f32-f32", "f32-f64", "f64-f64"])
@pytest.mark.parametrize("raw_dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
def test_upload_packed_and_download_equal_the_reference(dev, raw_dtype, compute, out):
    """3 levels in 3 slots; the level's value count is odd, so slots 1 and 2 start 4 (float32) or 8 (float64) bytes off a 16-byte
    boundary.  int16 levels hold every int16 value: an FMA in the kernel would change thousands of them."""
    n = 65573 if raw_dtype is np.int16 else 4099
    (fid,) = dev.field(n, out)
    levels = raw_levels(raw_dtype, n, seed=3)
    attrs = attrs_for(raw_dtype, compute)
    for chunk in (0, 1000):  # 1000 -> 992 values per chunk: several chunks and a short last one
        dev.ctx.set_option("unpack_chunk_values", chunk)
        for asynchronous in (0, 1):
            for ntz in (True, False):
                want = []
                for k, raw in enumerate(levels):
                    pk, desc = packing_and_desc(raw, attrs, out, ntz)
                    assert pk.compute_dtype == np.dtype(compute)
                    want.append(unpack_reference(raw, pk, out, ntz))
                    assert np.isnan(want[-1]).any() != ntz
                    rc = dev.lib.pk_field_upload_level_packed(dev.ctx.handle, fid, k, raw.ctypes.data_as(C.c_void_p), C.byref(desc), asynchronous)
                    assert rc == 0, dev.error()
                if asynchronous:
                    assert dev.slots(fid) == [-1] * NT  # pending: not usable, not downloadable
                    rc, _ = dev.download(fid, 1, n, out)
                    assert rc != 0 and "pending" in dev.error()
                    dev.ctx.check(dev.lib.pk_field_sync(dev.ctx.handle), "pk_field_sync")
                assert dev.slots(fid) == list(range(NT))
                for k in range(NT):
                    rc, got = dev.download(fid, k, n, out)
                    assert rc == 0, dev.error()
                    assert_same_bits(got, want[k], f"chunk {chunk} async {asynchronous} nan_to_zero {ntz} level {k}")
    dev.ctx.set_option("unpack_chunk_values", 0)


def test_a_level_that_is_not_resident_is_not_downloadable(dev):
    (fid,) = dev.field(4099, f32, tag="empty")
    rc, _ = dev.download(fid, 1, 4099, f32)
    assert rc != 0 and "not resident" in dev.error()
    rc, _ = dev.download(fid, NT, 4099, f32)
    assert rc != 0 and "out of range" in dev.error()


def test_a_compute_dtype_wider_than_the_field_is_refused(dev):
    (fid,) = dev.field(4099, f32, tag="narrow")
    raw = raw_levels(np.int16, 4099, seed=1)[0]
    _, desc = packing_and_desc(raw, attrs_for(np.int16, f64), f64, True)
    rc = dev.lib.pk_field_upload_level_packed(dev.ctx.handle, fid, 0, raw.ctypes.data_as(C.c_void_p), C.byref(desc), 0)
    assert rc != 0 and "wider" in dev.error()
    assert dev.slots(fid) == [-1] * NT
    desc.raw_dtype = _hip.PK_F32
    rc = dev.lib.pk_field_upload_level_packed(dev.ctx.handle, fid, 0, raw.ctypes.data_as(C.c_void_p), C.byref(desc), 0)
    assert rc != 0 and "raw_dtype" in dev.error()


def upload_group(dev, ids, level, raws, descs, asynchronous):
    ptrs = (C.c_void_p * len(raws))(*[r.ctypes.data for r in raws])
    arr = (_hip.PackDesc * len(raws))(*descs)
    return dev.lib.pk_field_upload_group_level_packed(dev.ctx.handle, ids[0], level, ptrs, arr, len(raws), asynchronous)


@pytest.mark.parametrize("ncomp, raw_dtype, compute, out", [(2, np.int16, f32, f32), (3, np.int16, f32, f64), (3, np.uint8, f64, f64), (2, np.int32, f32, f32)],
                         ids=["UV-int16-f32", "UVW-int16-f32-in-f64", "UVW-uint8-f64", "UV-int32-f32"])
def test_packed_groups_take_one_scale_offset_and_fill_per_component(dev, ncomp, raw_dtype, compute, out):
    n = 4099
    ids = dev.field(n, out, ncomp=ncomp)
    for chunk in (0, 1000):
        dev.ctx.set_option("unpack_chunk_values", chunk)
        for asynchronous in (0, 1):
            want = {}
            for k in range(NT):
                raws, descs = [], []
                for c in range(ncomp):
                    raw = raw_levels(raw_dtype, n, seed=10 * c + 1)[k]
                    pk, desc = packing_and_desc(raw, attrs_for(raw_dtype, compute, k=c), out, bool((c + k) % 2))  # (even nan_to_zero differs)
                    want[c, k] = unpack_reference(raw, pk, out, bool((c + k) % 2))
                    raws.append(raw)
                    descs.append(desc)
                assert upload_group(dev, ids, k, raws, descs, asynchronous) == 0, dev.error()
                if asynchronous:  # the members change state together
                    assert all(dev.slots(f)[k] == -1 for f in ids)
                    assert all(dev.download(f, k, n, out)[0] != 0 for f in ids)
            if asynchronous:
                dev.ctx.check(dev.lib.pk_field_sync(dev.ctx.handle), "pk_field_sync")
            assert all(dev.slots(f) == list(range(NT)) for f in ids)
            for c, f in enumerate(ids):
                for k in range(NT):
                    rc, got = dev.download(f, k, n, out)
                    assert rc == 0, dev.error()
                    assert_same_bits(got, want[c, k], f"component {c} level {k} chunk {chunk} async {asynchronous}")
    dev.ctx.set_option("unpack_chunk_values", 0)
    # one member alone (element-wise strided stores): its neighbours in the structs stay what they were
    raw = raw_levels(raw_dtype, n, seed=99)[0]
    pk, desc = packing_and_desc(raw, attrs_for(raw_dtype, compute, k=1), out, True)
    rc = dev.lib.pk_field_upload_level_packed(dev.ctx.handle, ids[1], 2, raw.ctypes.data_as(C.c_void_p), C.byref(desc), 0)
    assert rc == 0, dev.error()
    assert_same_bits(dev.download(ids[1], 2, n, out)[1], unpack_reference(raw, pk, out, True))
    assert_same_bits(dev.download(ids[0], 2, n, out)[1], want[0, 2])
    assert_same_bits(dev.download(ids[-1], 2, n, out)[1], want[ncomp - 1, 2] if ncomp > 2 else unpack_reference(raw, pk, out, True))


def test_mixed_raw_or_compute_dtypes_in_one_group_are_refused(dev):
    """The decode kernel is instantiated per (raw, compute, field dtype, group size): a group that mixes raw or compute dtypes is refused
    with a message (the engine unpacks such a group on the host)."""
    n = 4099
    ids = dev.field(n, f64, ncomp=2, tag="mixed")
    a, b = raw_levels(np.int16, n, seed=1)[0], raw_levels(np.uint8, n, seed=2)[0]
    da, db = packing_and_desc(a, attrs_for(np.int16, f32), f64, True)[1], packing_and_desc(b, attrs_for(np.uint8, f32), f64, True)[1]
    assert upload_group(dev, ids, 0, [a, b], [da, db], 0) != 0 and "raw dtype" in dev.error()
    dc = packing_and_desc(a, attrs_for(np.int16, f64), f64, True)[1]
    assert upload_group(dev, ids, 0, [a, a], [da, dc], 0) != 0 and "compute dtype" in dev.error()
    assert upload_group(dev, ids, 0, [a], [da], 0) != 0 and "per component" in dev.error()
    assert all(dev.slots(f) == [-1] * NT for f in ids)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
NX, NY, NZ, NLEV, NPART = 8, 6, 3, 5, 40


def make_case(kind):
    from oracle import cases

    if kind == "agrid":
        return cases.rect_agrid_case("unpack_a", mesh="spherical", kernels=["AdvectionRK4"], seed=21, nx=NX, ny=NY, nz=NZ, nt=NLEV, npart=NPART,
                                     field_dtype=np.float32, dt=3600.0, runtime=3.4 * 86400.0)
    return cases.curv_cgrid_case("unpack_c", mesh="spherical", kernels=["AdvectionRK4_3D"], seed=22, nx=NX, ny=NY, nz=NZ, nt=NLEV, npart=NPART,
                                 dt=3600.0, runtime=3.4 * 86400.0)


def pack_fields(case, seed=4):
    """The case's float fields as int16 with a scale, an offset and a fill value per field (a few cells of every level are fill)."""
    rng = np.random.default_rng(seed)
    out = {}
    for j, (name, arr) in enumerate(case["fields"].items()):
        ao = f32(0.01 * (j + 1))
        sf = f32(float(np.abs(arr - ao).max()) / 30000.0)
        raw = np.rint((arr.astype(np.float64) - float(ao)) / float(sf)).astype(np.int16)
        raw[rng.random(raw.shape) < 0.02] = -32767
        out[name] = (raw, sf, ao)
    return out


def sources_for(packed, kind, root, skip=()):
    if kind == "array":
        return {n: PackedArrayLevels(raw, sf, ao, fill_values=(-32767,)) for n, (raw, sf, ao) in packed.items()}
    os.makedirs(root, exist_ok=True)
    for n, (raw, sf, ao) in packed.items():
        write_int_zarr(root, n, raw, {"scale_factor": float(sf), "add_offset": float(ao), "_FillValue": -32767}, skip=skip if n == "U" else ())
    return {n: pa.ZarrLevels(root, n) for n in packed}


def run(case, fields, nslots, kernel):
    lazy = dict(case, fields=fields)
    fs = build_fieldset(lazy)
    fs.to_device(nslots=nslots)
    eng = fs._engine_or_create()
    calls = []
    upload = eng._upload

    def recording_upload(name, level, asynchronous):
        if eng.pack_leader_of.get(name, name) == name:
            calls.append((name, int(level), bool(asynchronous), len(eng.pack_groups.get(name, [name]))))
        return upload(name, level, asynchronous)

    eng._upload = recording_upload
    pset = build_pset(lazy, fs)
    pset.execute([kernel, pa.DeleteParticle], dt=case["dt"], runtime=case["runtime"])
    cols = {k: np.array(v) for k, v in pset._data.items()}
    return cols, eng, calls, pset._last_stats


def assert_same_columns(got, want, label):
    assert set(got) == set(want)
    for k in want:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{label}: column {k} differs"


@pytest.mark.parametrize("nslots", [None, 3], ids=["resident", "ring3"])
@pytest.mark.parametrize("source", ["array", "zarr", "zarr-missing-chunk"])
@pytest.mark.parametrize("grid", ["agrid", "cgrid"])
def test_runs_on_device_unpacked_levels_equal_host_unpacked_runs(gpu, tmp_path, monkeypatch, grid, source, nslots):
    case = make_case(grid)
    kernel = pa.AdvectionRK4 if grid == "agrid" else pa.AdvectionRK4_3D
    nfields = len(case["fields"])
    packed = pack_fields(case)
    raw_level_bytes = NX * NY * NZ * 2
    skip = ("2.1.0.0",) if source == "zarr-missing-chunk" else ()
    fields = lambda tag: sources_for(packed, "array" if source == "array" else "zarr", str(tmp_path / tag), skip)
    monkeypatch.setenv("PARCELS_AMD_DEVICE_UNPACK", "0")
    want, eng0, _, stats0 = run(case, fields("host"), nslots, kernel)
    assert eng0.transfers["levels_packed"] == 0 and eng0.transfers["levels_unpacked"] > 0
    assert stats0["steps"] > 20 * NPART and len(want["x"]) > NPART // 2  # the run crosses the levels and keeps its particles
    monkeypatch.delenv("PARCELS_AMD_DEVICE_UNPACK")
    got, eng, calls, stats = run(case, fields("device"), nslots, kernel)
    assert_same_columns(got, want, f"{grid} {source} nslots={nslots}")
    if grid == "cgrid":
        assert eng.pack_groups == {"U": ["U", "V", "W"]} and str(eng.field_host["U"].dtype) == "float32"
    if nslots is None:
        uploaded, level2 = NLEV * nfields, (nfields if grid == "cgrid" else 1)
    else:
        assert stats["launches"] > 1 and any(a for _, _, a, _ in calls)
        uploaded = sum(m for _, _, _, m in calls)
        level2 = sum(m for name, lv, _, m in calls if lv == 2 and name == "U")
    host_levels = level2 if skip else 0  # the level with the unwritten chunk (and the group it belongs to) is unpacked on the host
    assert eng.transfers["levels_packed"] == uploaded - host_levels and eng.transfers["levels_unpacked"] == host_levels
    assert eng.ctx.unpack_stats()["levels"] == (uploaded - host_levels) // (nfields if grid == "cgrid" else 1)
    if nslots is not None and not skip:  # the staging ring carried raw bytes (288 per plane: a multiple of 16, no padding)
        assert eng.ctx.upload_stats()["stage_bytes"] == sum(m for _, _, a, m in calls if a) * raw_level_bytes
        if grid == "agrid":  # (the float levels of a group go through the ring in blocking uploads as well)
            assert eng0.ctx.upload_stats()["stage_bytes"] == 2 * eng.ctx.upload_stats()["stage_bytes"]


def test_a_widened_float32_component_is_rounded_in_float32_first(gpu, monkeypatch):
    """U unpacks to float32, V (a float64 offset) to float64: the vector field is float64 on the device, U's values are rounded in float32
    and then widened -- and the A-grid run equals the host-unpacked one."""
    case = make_case("agrid")
    packed = pack_fields(case)
    def fields():
        (ru, su, ou), (rv, sv, ov) = packed["U"], packed["V"]
        return {"U": PackedArrayLevels(ru, su, ou, fill_values=(-32767,)), "V": PackedArrayLevels(rv, sv, float(ov), fill_values=(-32767,))}
    monkeypatch.setenv("PARCELS_AMD_DEVICE_UNPACK", "0")
    want, _, _, _ = run(case, fields(), None, pa.AdvectionRK4)
    monkeypatch.delenv("PARCELS_AMD_DEVICE_UNPACK")
    got, eng, _, _ = run(case, fields(), None, pa.AdvectionRK4)
    assert str(eng.field_host["U"].dtype) == "float64" and eng.field_host["U"].packing.compute_dtype == np.float32
    assert eng.field_host["V"].packing.compute_dtype == np.float64
    assert eng.transfers["levels_packed"] == 2 * NLEV and eng.transfers["levels_unpacked"] == 0
    assert_same_columns(got, want, "widened")
    out = np.empty((NZ, NY, NX), np.float64)
    eng.ctx.check(eng.lib.pk_field_download_level(eng.ctx.handle, eng.field_ids["U"], 1, out.ctypes.data_as(C.c_void_p)), "pk_field_download_level")
    assert_same_bits(out, eng.field_host["U"][1])


def test_float_levels_keep_their_path(gpu, tmp_path):
    case = make_case("agrid")
    fields = {}
    for name, arr in case["fields"].items():
        d = tmp_path / name
        d.mkdir()
        for k in range(arr.shape[0]):
            np.save(d / f"{k:04d}.npy", arr[k])
        fields[name] = pa.NpyLevels(str(d))
    _, eng, _, _ = run(case, fields, None, pa.AdvectionRK4)
    assert eng.transfers["levels_packed"] == 0 and eng.transfers["levels_unpacked"] == 2 * NLEV
    assert eng.ctx.unpack_stats()["levels"] == 0
