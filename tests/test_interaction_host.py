"""CPU: the host side of the neighbour search (parcels_amd/interaction.py): public names, argument validation (which happens before
anything touches the device), the C ABI additions and the CSR helper.  The numerics have no CPU path: tests/test_gpu_interaction.py."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import parcels_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pk_neighbors_build", "pk_neighbors_counts", "pk_neighbors_nearest", "pk_neighbors_pairs", "pk_neighbors_info",
               "pk_neighbors_release"]
XY = (np.zeros(4), np.zeros(4))
CALLS = ["neighbors", "neighbor_counts", "nearest_neighbor"]


def test_public_names():
    from parcels_amd import interaction

    for name in CALLS:
        assert callable(getattr(pa, name)) and getattr(pa, name) is getattr(interaction, name)
    assert pa.Neighbors is interaction.Neighbors
    assert 0 < interaction.MAX_PAIRS_MEMORY_SHARE < 1
    assert interaction.device_bytes_per_pair(False) == 44 and interaction.device_bytes_per_pair(True) == 52


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan"), float("inf")])
def test_radius_must_be_finite_and_positive(call, radius):
    with pytest.raises(ValueError, match="radius"):
        getattr(pa, call)(XY, radius)


@pytest.mark.parametrize("call", CALLS)
def test_radius_must_be_a_number(call):
    for radius in ("1", None, True, [1.0]):
        with pytest.raises(TypeError, match="radius"):
            getattr(pa, call)(XY, radius)


@pytest.mark.parametrize("call", CALLS)
def test_arrays_must_be_one_dimensional_and_of_one_length(call):
    f = getattr(pa, call)
    with pytest.raises(ValueError, match="particles.*length"):
        f((np.zeros(4), np.zeros(5)), 1.0)
    with pytest.raises(ValueError, match="particles.*z has length"):
        f((np.zeros(4), np.zeros(4), np.zeros(3)), 1.0, z=True)
    with pytest.raises(ValueError, match="particles.*1-D"):
        f((np.zeros((2, 2)), np.zeros((2, 2))), 1.0)
    with pytest.raises(TypeError, match="particles"):
        f((np.zeros(4),), 1.0)
    with pytest.raises(TypeError, match="particles"):
        f(object(), 1.0)
    with pytest.raises(TypeError, match="particles"):
        f((np.array(["a"]), np.array(["b"])), 1.0)


@pytest.mark.parametrize("call", CALLS)
def test_sources_must_be_a_boolean_mask_of_length_n(call):
    f = getattr(pa, call)
    with pytest.raises(TypeError, match="sources"):
        f(XY, 1.0, sources=np.ones(4, dtype=np.int8))
    with pytest.raises(ValueError, match="sources"):
        f(XY, 1.0, sources=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="sources"):
        f(XY, 1.0, sources=np.ones((4, 1), dtype=bool))


@pytest.mark.parametrize("call", CALLS)
def test_z_needs_a_z(call):
    with pytest.raises(ValueError, match="z"):
        getattr(pa, call)(XY, 1.0, z=True)

    class NoZ:
        x = np.zeros(3)
        y = np.zeros(3)

    with pytest.raises(ValueError, match="z"):
        getattr(pa, call)(NoZ(), 1.0, z=True)


def test_max_pairs_must_be_a_count():
    with pytest.raises(TypeError, match="max_pairs"):
        pa.neighbors(XY, 1.0, max_pairs=1.5)
    with pytest.raises(ValueError, match="max_pairs"):
        pa.neighbors(XY, 1.0, max_pairs=-1)


def test_valid_arguments_reach_the_device_and_fail_loudly_without_one():
    """No CPU path for the numerics: once validation has passed, the call needs the GPU like every other device call."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from parcels_amd.hostkernels import HostParticles

    view = HostParticles({"x": np.zeros(3, np.float32), "y": np.zeros(3, np.float32), "z": np.zeros(3, np.float32), "particle_id": np.arange(3)},
                         np.arange(3), by_mask=True)
    for particles, kw in ((XY, {}), (view, {"z": True}), ((np.zeros(2), np.zeros(2), np.zeros(2)), {"z": True, "sources": np.ones(2, dtype=bool)})):
        for call in CALLS:
            with pytest.raises(pa._hip.HipLibraryError):
                getattr(pa, call)(particles, 1.0, **kw)


def test_symbols_are_listed_declared_and_exported():
    from parcels_amd import _hip

    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    lib = _hip.load()
    for sym in NEW_SYMBOLS:
        assert sym in _hip.ABI_SYMBOLS, sym
        assert re.search(r"^int32_t\s+" + sym + r"\s*\(", header, flags=re.M), f"{sym} is not declared in include/parcels_hip.h"
        assert hasattr(lib, sym), f"libparcels_hip.so does not export {sym}"
        assert getattr(lib, sym).argtypes, f"{sym} has no ctypes prototype"
    assert lib.pk_abi_version() == _hip.PK_ABI_VERSION == 9  # exports were only added
    assert "tutorial_interaction" in header and _hip.PK_NEIGHBORS_NO_COINCIDENT == 1
    assert re.search(r"#define\s+PK_NEIGHBORS_NO_COINCIDENT\s+1\b", header)


def test_info_struct_matches_the_header_layout(tmp_path):
    from parcels_amd import _hip

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "parcels_hip.h"\nint main(void){printf("%zu %zu %zu\\n", '
                   "sizeof(pk_neighbors_info_t), offsetof(pk_neighbors_info_t, cell_size), offsetof(pk_neighbors_info_t, doublings));return 0;}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_h, off_d = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert C.sizeof(_hip.NeighborsInfo) == size
    assert _hip.NeighborsInfo.cell_size.offset == off_h and _hip.NeighborsInfo.doublings.offset == off_d


def test_sum_on_a_hand_made_csr():
    count = np.array([2, 0, 3, 1], dtype=np.int64)
    starts = np.array([0, 2, 2, 5, 6], dtype=np.int64)
    j = np.array([1, 2, 0, 1, 3, 2], dtype=np.int64)
    d = np.arange(6, dtype=np.float64)
    nb = pa.Neighbors(count, starts, j, d, d, None, d)
    assert nb.n == 4 and nb.total == 6 and not hasattr(nb, "dz")
    assert np.array_equal(nb.i, [0, 0, 2, 2, 2, 3]) and nb.i.dtype == np.int64
    w = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    s = nb.sum(w)
    assert s.dtype == np.float64 and np.array_equal(s, [3.0, 0.0, 28.0, 32.0])
    # added in pair order, one rounding per addition: 1e16 + 1 + 1 stays 1e16, 1 + 1 + 1e16 does not
    assert np.array_equal(nb.sum([0, 0, 1e16, 1.0, 1.0, 0]), [0.0, 0.0, 1e16, 0.0])
    assert np.array_equal(nb.sum([0, 0, 1.0, 1.0, 1e16, 0]), [0.0, 0.0, 1e16 + 2.0, 0.0])
    with pytest.raises(ValueError, match="per_pair_values"):
        nb.sum(np.zeros(5))
    empty = pa.Neighbors(np.zeros(3, np.int64), np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    assert np.array_equal(empty.sum(np.zeros(0)), np.zeros(3)) and np.array_equal(empty.dz, np.zeros(0))


def test_build_lists_name_the_new_object():
    """The library links its objects by name in two places."""
    assert "pk_neighbors.o" in open(os.path.join(ROOT, "parcels_amd", "csrc", "Makefile")).read()
    assert " pk_neighbors " in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
