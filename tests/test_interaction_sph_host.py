"""CPU: the host side of the great-circle neighbour search (the `mesh` keyword of parcels_amd/interaction.py): validation, which happens
before anything touches the device, and the C ABI additions.  The numerics have no CPU path: tests/test_gpu_interaction_sph.py."""

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd.xgrid import EARTH_RADIUS, SphericalMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pk_neighbors_build_spherical", "pk_neighbors_info_spherical"]
XY = (np.zeros(4), np.zeros(4))
CALLS = ["neighbors", "neighbor_counts", "nearest_neighbor"]


@pytest.mark.parametrize("call", CALLS)
def test_mesh_must_be_a_mesh(call):
    for mesh in ("sphere", None, 1.0, np.zeros(3), object()):
        with pytest.raises(ValueError, match=r"mesh must be 'flat', 'spherical', or a SphericalMesh object\. Got mesh="):
            getattr(pa, call)(XY, 1.0, mesh=mesh)


def test_a_fieldset_without_fields_has_no_mesh():
    fs = pa.FieldSet([])
    with pytest.raises(ValueError, match="mesh.*FieldSet has no field"):
        pa.neighbor_counts(XY, 1.0, mesh=fs)


@pytest.mark.parametrize("call", CALLS)
def test_radius_must_be_below_a_quarter_of_the_circumference(call):
    f = getattr(pa, call)
    quarter = 0.5 * math.pi * EARTH_RADIUS
    for radius in (quarter, 2.0e7):
        with pytest.raises(ValueError, match="radius") as ei:
            f(XY, radius, mesh="spherical")
        assert repr(float(radius)) in str(ei.value) and repr(quarter) in str(ei.value)  # both numbers
    with pytest.raises(ValueError, match="radius") as ei:
        f(XY, 2.0, mesh=SphericalMesh(radius=1.0))  # the radius of a custom sphere counts, not the Earth's
    assert repr(2.0) in str(ei.value) and repr(0.5 * math.pi) in str(ei.value)
    with pytest.raises(ValueError, match="radius"):
        f(XY, -1.0, mesh="spherical")  # the flat checks still come first


@pytest.mark.parametrize("call", CALLS)
def test_z_needs_a_z(call):
    with pytest.raises(ValueError, match="z"):
        getattr(pa, call)(XY, 1.0, z=True, mesh="spherical")


def test_valid_arguments_reach_the_device_and_fail_loudly_without_one():
    """No CPU path: once validation has passed, a spherical call needs the GPU like every other device call."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from parcels_amd.xgrid import FlatMesh

    xyz = (np.zeros(2), np.zeros(2), np.zeros(2))
    just_below = math.nextafter(0.5 * math.pi * EARTH_RADIUS, 0.0)
    for particles, radius, kw in ((XY, 1.0e5, {"mesh": "spherical"}), (XY, just_below, {"mesh": SphericalMesh()}),
                                  (xyz, 1.0, {"mesh": SphericalMesh(radius=1.0), "z": True, "sources": np.ones(2, dtype=bool)}),
                                  (XY, 1.0, {"mesh": FlatMesh()})):
        for call in CALLS:
            with pytest.raises(pa._hip.HipLibraryError):
                getattr(pa, call)(particles, radius, **kw)


def test_symbols_are_listed_declared_prototyped_and_exported():
    from parcels_amd import _hip

    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _hip.load()
    for sym in NEW_SYMBOLS:
        assert sym in _hip.ABI_SYMBOLS, sym
        assert re.search(r"^int32_t\s+" + sym + r"\s*\(", header, flags=re.M), f"{sym} is not declared in include/parcels_hip.h"
        assert hasattr(lib, sym), f"libparcels_hip.so does not export {sym}"
        assert getattr(lib, sym).argtypes, f"{sym} has no ctypes prototype"
        assert sym in integration, f"{sym} has no row in INTEGRATION.md"
    assert len(lib.pk_neighbors_build_spherical.argtypes) == 9
    assert lib.pk_abi_version() == _hip.PK_ABI_VERSION == 9  # exports were only added


def test_info_struct_matches_the_header_layout(tmp_path):
    from parcels_amd import _hip

    fields = ["n", "nvalid", "bands", "cells", "total", "band_height", "periodic", "doublings"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "parcels_hip.h"\nint main(void){printf("%zu", sizeof(pk_neighbors_info_spherical_t));\n'
                   + "".join(f'printf(" %zu", offsetof(pk_neighbors_info_spherical_t, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *offsets = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert C.sizeof(_hip.NeighborsSphInfo) == size
    assert [getattr(_hip.NeighborsSphInfo, f).offset for f in fields] == offsets
    assert [name for name, _ in _hip.NeighborsSphInfo._fields_] == fields
    # the flat struct did not move
    assert C.sizeof(_hip.NeighborsInfo) == 56 and _hip.NeighborsInfo.cell_size.offset == 40


def test_the_spherical_code_is_in_the_listed_object():
    """No new object: the spherical kernels live in pk_neighbors.hip, which both build lists already name."""
    csrc = os.path.join(ROOT, "parcels_amd", "csrc")
    assert "pk_neighbors_build_spherical" in open(os.path.join(csrc, "pk_api_analysis.hip")).read()
    assert "neighbors_build_spherical" in open(os.path.join(csrc, "pk_neighbors.hip")).read()
    assert not os.path.exists(os.path.join(csrc, "pk_neighbors_sph.hip"))
    assert "pk_neighbors.o" in open(os.path.join(csrc, "Makefile")).read()
    assert " pk_neighbors " in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
