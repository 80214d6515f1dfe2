"""CPU: CF-packed integer levels -- what the device is told to do (sources.cf_packing), its NumPy restatement (sources.unpack_reference)
against the host path bit for bit, the per-value function of csrc/pk_unpack.h compiled for the host, and the ABI of the new exports."""

import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import sources
from parcels_amd.engine import _LazyLevels
from parcels_amd.sources import PackedArrayLevels, cf_packing, cf_unpack, unpack_reference
from unpack_utils import all_values, assert_same_bits, write_int_zarr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
# (scale_factor, add_offset) of the bit-identity tests: pairs for which an FMA gives other bits than NumPy's two roundings
PAIRS = [(f32(0.001), f32(2.0)), (f32(0.0006103702), f32(20.0))]
PAIRS64 = (0.001, 2.0)  # float64 attributes: the compute dtype is float64


def test_cf_packing_chooses_the_dtype_cf_unpack_chooses():
    table = [
        (np.int16, {"scale_factor": f32(0.5), "add_offset": f32(1.0)}, f32),
        (np.int32, {"scale_factor": f32(0.5), "add_offset": f32(1.0)}, f64),
        (np.int16, {"scale_factor": f64(0.5), "add_offset": f64(1.0)}, f64),
        (np.int16, {"add_offset": f32(1.0)}, f64),
        (np.int16, {"scale_factor": f32(0.5), "add_offset": f64(1.0)}, f64),
        (np.int16, {"scale_factor": f32(0.5)}, f32),
        (np.int8, {"_FillValue": np.int8(3)}, f32),
        (np.int16, {"_FillValue": np.int16(3)}, f32),
        (np.int32, {"_FillValue": np.int32(3)}, f64),
        (np.uint8, {"scale_factor": f32(0.25), "add_offset": f32(-3.0)}, f32),
        (np.uint16, {"scale_factor": f32(0.25), "add_offset": f32(-3.0), "_FillValue": np.uint16(65535)}, f32),
        (np.uint16, {"scale_factor": 0.25}, f64),
        (np.int8, {"scale_factor": f32(0.5), "missing_value": np.int8(-128)}, f32),
        (np.int32, {"scale_factor": f32(0.5)}, f32),
        (np.dtype(">i2"), {"scale_factor": f32(0.5), "add_offset": f32(1.0)}, f32),
    ]
    for raw, attrs, want in table:
        pk = cf_packing(raw, attrs)
        assert pk is not None, (raw, attrs)
        assert pk.compute_dtype == cf_unpack(np.arange(4).astype(raw), attrs).dtype == np.dtype(want), (raw, attrs)
        assert pk.raw_dtype == np.dtype(raw).newbyteorder("=") and pk.raw_dtype.isnative
        assert (pk.scale is None) == ("scale_factor" not in attrs) and (pk.offset is None) == ("add_offset" not in attrs)
    pk = cf_packing(np.int16, {"scale_factor": f32(0.001), "add_offset": f32(2.0), "_FillValue": np.int16(-32767), "missing_value": np.int16(7)})
    assert pk.scale == float(f32(0.001)) and pk.offset == 2.0 and pk.fills == (-32767, 7)


def test_cf_packing_refuses_what_the_device_cannot_do():
    sf = {"scale_factor": f32(0.5)}
    for dt in (np.float32, np.float64, np.int64, np.uint32, np.uint64):
        assert cf_packing(dt, sf) is None
    assert cf_packing(np.int16, {}) is None and cf_packing(np.int16, {"units": "m"}) is None  # no packing attribute at all
    assert cf_packing(np.int16, dict(sf, _FillValue=np.arange(5, dtype=np.int16))) is None   # more than 4 distinct fill values
    assert cf_packing(np.int16, dict(sf, _FillValue=np.arange(3, dtype=np.int16), missing_value=np.arange(2, 5, dtype=np.int16))) is None
    four = cf_packing(np.int16, dict(sf, _FillValue=np.arange(3, dtype=np.int16), missing_value=np.arange(1, 4, dtype=np.int16)))
    assert four.fills == (0, 1, 2, 3)
    assert cf_packing(np.int16, {"scale_factor": f32(np.inf)}) is None and cf_packing(np.int16, {"add_offset": np.nan}) is None
    assert cf_packing(np.int16, {"scale_factor": f32(3e35)}) is None  # 32768 * 3e35 overflows float32: nan_to_num would rewrite the inf
    # a fill value the raw dtype cannot hold can never match: dropped (as is a NaN, and a value with a fraction)
    assert cf_packing(np.int16, dict(sf, _FillValue=np.int32(40000))).fills == ()
    assert cf_packing(np.uint8, dict(sf, _FillValue=np.int8(-1), missing_value=np.uint8(255))).fills == (255,)
    assert cf_packing(np.int16, dict(sf, _FillValue=np.float32(-999.0), missing_value=np.array([np.nan, 0.5]))).fills == (-999,)
    assert pa.LevelSource.packing.fget(object()) is None and pa.LevelSource().read_level_packed(0) is None


def _host_path(raw4, attrs, target, fill_nan):
    src = PackedArrayLevels(raw4, attrs.get("scale_factor"), attrs.get("add_offset"), attrs.get("_FillValue", ()), fill_nan=fill_nan)
    return _LazyLevels(src, target, fill_nan=fill_nan)[0], src


CASES = [
    ("int16-a", np.int16, {"scale_factor": PAIRS[0][0], "add_offset": PAIRS[0][1]}),
    ("int16-b", np.int16, {"scale_factor": PAIRS[1][0], "add_offset": PAIRS[1][1]}),
    ("int16-f64", np.int16, {"scale_factor": PAIRS64[0], "add_offset": PAIRS64[1]}),
    ("int8", np.int8, {"scale_factor": PAIRS[0][0], "add_offset": PAIRS[0][1]}),
    ("uint8", np.uint8, {"scale_factor": PAIRS[1][0], "add_offset": PAIRS[1][1]}),
    ("uint8-fill-only", np.uint8, {}),
    ("int32-f32-scale", np.int32, {"scale_factor": PAIRS[0][0]}),
    ("int32-f64", np.int32, {"scale_factor": PAIRS[0][0], "add_offset": PAIRS[0][1]}),
    ("int32-offset-only", np.int32, {"add_offset": PAIRS[1][1]}),
]


@pytest.mark.parametrize("fill_nan", [True, False])
@pytest.mark.parametrize("label, dtype, attrs", CASES, ids=[c[0] for c in CASES])
def test_unpack_reference_equals_the_host_path_bit_for_bit(label, dtype, attrs, fill_nan):
    info = np.iinfo(dtype)
    raw = all_values(dtype) if info.max < 70000 else np.random.default_rng(11).integers(info.min, info.max, 100000, endpoint=True).astype(dtype)
    fills = (raw[3], raw[len(raw) // 2])
    raw = np.concatenate([raw, np.repeat(np.asarray(fills, dtype=dtype), 5)])
    attrs = dict(attrs, _FillValue=np.asarray(fills, dtype=dtype))
    raw4 = raw.reshape(1, 1, 1, -1)
    pk = cf_packing(dtype, attrs)
    assert pk.fills == tuple(int(v) for v in fills)
    for target in (f32, f64) if pk.compute_dtype == np.float32 else (f64,):
        want, src = _host_path(raw4, attrs, target, fill_nan)
        assert src.packing == pk and src.dtype == pk.compute_dtype
        got = unpack_reference(src.read_level_packed(0), pk, target, fill_nan)
        assert_same_bits(got, want)
        assert np.isnan(want).sum() == (0 if fill_nan else 12)
        if fill_nan:
            assert (want[0, 0, -10:] == 0).all()


def _fused_f32(raw, sf, ao):
    """float32(raw * sf + ao) with ONE rounding: the products (16 x 24 bits) and the sums are exact in float64."""
    return (raw.astype(f64) * f64(sf) + f64(ao)).astype(f32)


@pytest.mark.parametrize("sf, ao", PAIRS)
def test_a_contracted_evaluation_would_change_the_int16_inputs(sf, ao):
    raw = all_values(np.int16)
    two_step = raw.astype(f32) * sf + ao
    exact = [Fraction(int(r)) * Fraction(float(sf)) + Fraction(float(ao)) for r in raw[::997]]
    assert all(Fraction(float(v)) == e for v, e in zip(raw[::997].astype(f64) * f64(sf) + f64(ao), exact))  # the float64 route IS exact
    assert int((_fused_f32(raw, sf, ao) != two_step).sum()) >= 1000


def test_a_contracted_evaluation_would_change_the_float64_inputs():
    """float64 attributes (53-bit scale): the product of the two-step evaluation is rounded, then the sum.  (With float32-exact attributes
    in float64 the sum is exact whenever the product was rounded, and a fused evaluation changes nothing.)"""
    raw = all_values(np.int16)
    sf, ao = PAIRS64
    two_step = raw.astype(f64) * sf + ao
    fused = np.array([float(Fraction(int(r)) * Fraction(sf) + Fraction(ao)) for r in raw])  # float(Fraction) rounds once, to nearest even
    assert int((fused != two_step).sum()) >= 1000


def test_netcdf_levels_give_the_raw_level_and_its_packing():
    path = os.path.join(ROOT, "tests", "golden", "hdf5", "default_v0.h5")
    for fill_nan in (True, False):
        src = pa.NetCDFLevels(path, "V", fill_nan=fill_nan)
        pk = src.packing
        assert pk is not None and pk.raw_dtype == np.int16 and pk.compute_dtype == src.dtype and pk.fills == (-32767,)
        lazy = _LazyLevels(src, src.dtype, fill_nan=fill_nan)
        for k in range(src.shape[0]):
            raw, pk2 = lazy.packed(k)
            assert pk2 == pk and raw.dtype == np.int16 and raw.flags["C_CONTIGUOUS"] and raw.shape == src.shape[1:] and raw.dtype.isnative
            assert_same_bits(unpack_reference(raw, pk, src.dtype, fill_nan), lazy[k])
        assert (src.read_level_packed(3) == -32767).all()  # the level that was never written
        src.close()
    u = pa.NetCDFLevels(path, "U")
    assert u.packing is None and u.read_level_packed(0) is None and _LazyLevels(u, np.float32).packed(0) is None
    u.close()


def test_zarr_levels_give_the_raw_level_unless_a_chunk_is_missing(tmp_path):
    rng = np.random.default_rng(5)
    raw = rng.integers(-32768, 32767, (4, 3, 6, 8), endpoint=True).astype(np.int16)
    raw[:, :, 2, 3] = -32767
    write_int_zarr(str(tmp_path), "uo", raw, {"scale_factor": 0.001, "add_offset": 2.0, "_FillValue": -32767}, skip=("2.1.0.0",))
    for fill_nan in (True, False):
        src = pa.ZarrLevels(str(tmp_path), "uo", fill_nan=fill_nan)
        pk = src.packing
        assert pk.raw_dtype == np.int16 and pk.compute_dtype == src.dtype == np.float32 and pk.fills == (-32767,)
        lazy = _LazyLevels(src, np.float32, fill_nan=fill_nan)
        for k in range(4):
            got = lazy.packed(k)
            if k == 2:  # NaN where no raw value says so: the host path
                assert got is None and src.read_level_packed(k) is None
                assert np.isnan(src.read_level(k)[2]).all()
                continue
            assert np.array_equal(got[0], raw[k]) and got[0].flags["C_CONTIGUOUS"]
            assert_same_bits(unpack_reference(got[0], pk, np.float32, fill_nan), lazy[k])
    wide = _LazyLevels(pa.ZarrLevels(str(tmp_path), "uo"), np.float64)  # a float32 component of a vector field widened to float64
    assert_same_bits(unpack_reference(wide.packed(0)[0], pk, np.float64, True), wide[0])


def test_a_compute_dtype_wider_than_the_field_keeps_the_host_path():
    src = PackedArrayLevels(np.zeros((2, 1, 2, 2), np.int16), scale_factor=0.5)  # a float64 attribute
    assert src.packing.compute_dtype == np.float64
    assert _LazyLevels(src, np.float32).packed(0) is None and _LazyLevels(src, np.float64).packed(0) is not None


HOST_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "pk_unpack.h"
int main(int argc, char** argv) {
    const float pairs[2][2] = {{0.001f, 2.0f}, {0.0006103702f, 20.0f}};
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 1;
    for (int k = 0; k < 2; k++)
        for (int ntz = 0; ntz < 2; ntz++) {
            pk::UnpackParams<int16_t, float> p{};
            p.scale = pairs[k][0]; p.offset = pairs[k][1];
            p.has_scale = p.has_offset = 1;
            p.fill[0] = -32767; p.fill[1] = 12345; p.nfill = 2;
            p.nan_to_zero = ntz;
            std::vector<float> out(65536);
            for (int r = -32768; r <= 32767; r++) out[r + 32768] = pk::unpack_value<int16_t, float>((int16_t)r, p);
            std::fwrite(out.data(), sizeof(float), out.size(), f);
        }
    pk::UnpackParams<int16_t, double> q{};
    q.scale = 0.001; q.offset = 2.0; q.has_scale = q.has_offset = 1;
    std::vector<double> out(65536);
    for (int r = -32768; r <= 32767; r++) out[r + 32768] = pk::unpack_value<int16_t, double>((int16_t)r, q);
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    return std::fclose(f);
}
"""


def test_the_per_value_function_compiled_for_the_host_gives_numpys_bits(tmp_path):
    src = tmp_path / "unpack_host.cpp"
    src.write_text(HOST_PROGRAM)
    flags = ["-O2"]
    if os.path.exists("/proc/cpuinfo") and re.search(r"^flags\s*:.*\bfma\b", open("/proc/cpuinfo").read(), re.M):
        flags.append("-mfma")  # let the compiler fuse where the header does not forbid it
    exe, out = tmp_path / "unpack_host", tmp_path / "out.bin"
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "parcels_amd", "csrc"), str(src), "-o", str(exe)])
    subprocess.check_call([str(exe), str(out)])
    blob = out.read_bytes()
    got32 = np.frombuffer(blob[: 4 * 4 * 65536], dtype=np.float32).reshape(2, 2, 65536)
    raw = all_values(np.int16)
    for k, (sf, ao) in enumerate(PAIRS):
        pk = cf_packing(np.int16, {"scale_factor": sf, "add_offset": ao, "_FillValue": np.array([-32767, 12345], np.int16)})
        for ntz in (0, 1):
            assert_same_bits(got32[k, ntz], unpack_reference(raw, pk, np.float32, bool(ntz)))
    got64 = np.frombuffer(blob[4 * 4 * 65536:], dtype=np.float64)
    pk = cf_packing(np.int16, {"scale_factor": PAIRS64[0], "add_offset": PAIRS64[1]})
    assert_same_bits(got64, unpack_reference(raw, pk, np.float64, False))


NEW_SYMBOLS = ["pk_field_upload_level_packed", "pk_field_upload_group_level_packed", "pk_field_download_level"]


def test_the_exports_are_declared_listed_and_exported():
    from parcels_amd import _hip

    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _hip.load()
    for sym in NEW_SYMBOLS + ["pk_unpack_stats"]:
        assert sym in _hip.ABI_SYMBOLS, sym
        assert re.search(r"^int32_t\s+" + sym + r"\s*\(", header, flags=re.M), f"{sym} is not declared in include/parcels_hip.h"
        assert hasattr(lib, sym) and getattr(lib, sym).argtypes, sym
        assert f"`{sym}`" in notes, f"{sym} has no row in INTEGRATION.md"
    assert lib.pk_abi_version() == _hip.PK_ABI_VERSION == 9  # exports were only added
    for name in ("PK_I8", "PK_U8", "PK_I16", "PK_U16", "PK_I32"):
        assert re.search(rf"#define\s+{name}\s+{getattr(_hip, name)}\b", header), name
    assert len({_hip.PK_F32, _hip.PK_F64, _hip.PK_I8, _hip.PK_U8, _hip.PK_I16, _hip.PK_U16, _hip.PK_I32}) == 7


def test_pack_desc_matches_the_header_layout(tmp_path):
    from parcels_amd import _hip

    members = [name for name, _ in _hip.PackDesc._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "parcels_hip.h"\nint main(void){printf("%zu", sizeof(pk_pack_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(pk_pack_desc, {m}));\n' for m in members) + "return 0;}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *offs = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert C.sizeof(_hip.PackDesc) == size
    assert [getattr(_hip.PackDesc, m).offset for m in members] == offs


def test_the_engine_builds_the_descriptor_from_the_packing():
    from parcels_amd import _hip

    src = PackedArrayLevels(np.zeros((2, 1, 2, 2), np.uint16), scale_factor=f32(0.25), fill_values=(65535, 7), fill_nan=False)
    lazy = _LazyLevels(src, np.float64, fill_nan=False)
    d = lazy.pack_desc(src.packing)
    assert (d.raw_dtype, d.compute_dtype, d.has_scale, d.has_offset, d.nfill, d.nan_to_zero) == (_hip.PK_U16, _hip.PK_F32, 1, 0, 2, 0)
    assert d.scale == 0.25 and list(d.fill)[:2] == [65535, 7]
    assert sources.Packing._fields == ("raw_dtype", "compute_dtype", "scale", "offset", "fills")
