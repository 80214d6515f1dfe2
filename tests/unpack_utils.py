"""Shared by tests/test_unpack_host.py and tests/test_gpu_unpack.py: bit comparison and a hand-written zarr store of packed integers."""

import json
import os

import numpy as np


def all_values(dtype):
    info = np.iinfo(dtype)
    return np.arange(info.min, info.max + 1, dtype=np.int64).astype(dtype)


def assert_same_bits(got, want, label=""):
    """The NaN masks agree, and everything else agrees as integers (so -0.0 is not 0.0)."""
    assert got.dtype == want.dtype and got.shape == want.shape, label
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    view = np.uint32 if want.dtype == np.float32 else np.uint64
    assert np.array_equal(got[~nan].view(view), want[~nan].view(view)), label


def write_int_zarr(root, name, raw, attrs, skip=()):
    """An uncompressed zarr v2 array (t, z, y, x) of integers, fill_value null, chunked (1, ceil(nz / 2), ny, nx); the chunk keys in
    `skip` stay unwritten.  (zarr / numcodecs are not needed.)"""
    nt, nz, ny, nx = raw.shape
    cz = (nz + 1) // 2
    d = os.path.join(root, name)
    os.makedirs(d)
    meta = {"zarr_format": 2, "shape": list(raw.shape), "chunks": [1, cz, ny, nx], "dtype": raw.dtype.str, "compressor": None, "fill_value": None,
            "order": "C", "filters": None}
    json.dump(meta, open(os.path.join(d, ".zarray"), "w"))
    json.dump(attrs, open(os.path.join(d, ".zattrs"), "w"))
    for t in range(nt):
        for c in range((nz + cz - 1) // cz):
            key = f"{t}.{c}.0.0"
            if key in skip:
                continue
            chunk = np.zeros((cz, ny, nx), raw.dtype)
            part = raw[t, c * cz:(c + 1) * cz]
            chunk[: part.shape[0]] = part
            open(os.path.join(d, key), "wb").write(chunk.tobytes())
