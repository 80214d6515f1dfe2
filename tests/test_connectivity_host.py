"""CPU: ParticleSet.cells / ParticleSet.connectivity -- the refusals that are raised before the device is touched, the NumPy restatement the
GPU tests compare with against a hand-written case, and the C ABI of the two exports."""

import ctypes
import os
import re

import numpy as np
import pytest

import parcels_amd as pa
from connectivity_utils import connectivity_numpy, same_arrays, sparse_to_dense
from density_utils import density_fieldset, density_pset, fixture
from parcels_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- refusals raised before the device is touched ------------------------------------------------------------------------------------------
def _pset():
    case = fixture("dens_rect_flat")
    fs = density_fieldset(case)
    pclass = pa.get_default_particle(np.float64).add_variable([pa.Variable("src", dtype=np.int32, initial=0), pa.Variable("src64", dtype=np.int64, initial=0),
                                                               pa.Variable("mass", dtype=np.float64, initial=1.0), pa.Variable("flag", dtype=np.int16, initial=1)])
    return case, fs, density_pset(case, fs, pclass=pclass)


def test_connectivity_refusals_name_the_reason(monkeypatch):
    case, fs, pset = _pset()
    monkeypatch.setattr(type(pset), "_engine", lambda self: pytest.fail("the device was asked for before the refusal"))
    n = len(pset)
    shape = tuple(case["shape"])
    ncells = int(np.prod(shape))
    with pytest.raises(ValueError, match="no Variable 'nope'"):
        pset.connectivity("nope")
    with pytest.raises(TypeError, match="float64"):
        pset.connectivity("mass")
    with pytest.raises(TypeError, match="int16"):
        pset.connectivity("flag")
    with pytest.raises(ValueError, match=rf"expected \({n},\)"):
        pset.connectivity(np.zeros(n + 1, np.int64))
    with pytest.raises(ValueError, match="one label per particle"):
        pset.connectivity(np.zeros((n, 1), np.int64))
    with pytest.raises(TypeError, match="float64"):
        pset.connectivity(np.zeros(n))
    with pytest.raises(ValueError, match="one label per cell"):
        pset.connectivity("src", regions=np.zeros(shape[::-1] + (1,), np.int32))
    with pytest.raises(ValueError, match=rf"expected \({shape[0]}, {shape[1]}\)"):
        pset.connectivity("src", regions=np.zeros(ncells, np.int32))
    with pytest.raises(ValueError, match="one label per cell"):
        pset.connectivity("src", regions=np.zeros(shape, np.int32), levels=True)  # (levels: the shape has the vertical dimension in front)
    with pytest.raises(TypeError, match="float32"):
        pset.connectivity("src", regions=np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="no field 'W'"):
        pset.connectivity("src", "W")
    with pytest.raises(TypeError, match="field must be"):
        pset.connectivity("src", 3)
    other = density_fieldset(case)
    for f in (other.U, other.UV):
        with pytest.raises(ValueError, match="not a field of this ParticleSet's FieldSet"):
            pset.connectivity("src", f)
    with pytest.raises(ValueError, match="normalize must be None or 'origin'"):
        pset.connectivity("src", normalize="dest")
    with pytest.raises(ValueError, match=rf"n_origin = {ncells} by n_dest = {ncells}.*max_dense = 100.*sparse=True"):
        pset.connectivity("src", max_dense=100)
    with pytest.raises(ValueError, match="62-bit"):
        pset.connectivity("src64", n_origin=2**61, sparse=True)
    with pytest.raises(ValueError, match="n_origin must not be negative"):
        pset.connectivity("src", n_origin=-1)
    sharded = density_pset(case, fs, shard=(0, 2))
    with pytest.raises(NotImplementedError, match="ParticleSet.connectivity on a sharded"):
        sharded.connectivity(np.zeros(len(sharded), np.int64))


def test_cells_refusals_name_the_reason(monkeypatch):
    case, fs, pset = _pset()
    monkeypatch.setattr(type(pset), "_engine", lambda self: pytest.fail("the device was asked for before the refusal"))
    shape = tuple(case["shape"])
    with pytest.raises(ValueError, match="no field 'W'"):
        pset.cells("W")
    with pytest.raises(TypeError, match="field must be"):
        pset.cells(3.5)
    with pytest.raises(ValueError, match="not a field of this ParticleSet's FieldSet"):
        pset.cells(density_fieldset(case).U)
    with pytest.raises(ValueError, match="cells: regions has shape"):
        pset.cells(regions=np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError, match="cells: regions has shape"):
        pset.cells(regions=np.zeros(shape, np.int64), levels=True)
    with pytest.raises(TypeError, match="bool"):
        pset.cells(regions=np.zeros(shape, bool))
    sharded = density_pset(case, fs, shard=(1, 2))
    with pytest.raises(NotImplementedError, match="ParticleSet.cells on a sharded"):
        sharded.cells()


# ---- the NumPy restatement -------------------------------------------------------------------------------------------------------------------
def test_numpy_restatement_on_a_hand_written_case():
    """3 origins x 3 destinations; origin 1 is empty, one row is untracked, two rows are outside"""
    origin = np.array([2, 0, 0, -1, 2, 2, 0, 2, 0, -7])
    dest = np.array([1, 0, 2, 1, -1, 1, 0, 0, -1, -1])
    t, outside = connectivity_numpy(origin, dest, 3, 3, return_outside=True)
    assert same_arrays(t, np.array([[2, 0, 1], [0, 0, 0], [1, 2, 0]], np.int64))
    assert same_arrays(outside, np.array([1, 0, 1], np.int64))
    assert t.sum() + outside.sum() == np.count_nonzero(origin >= 0) == 8
    assert same_arrays(connectivity_numpy(origin, dest, 3, 3), t)
    norm = connectivity_numpy(origin, dest, 3, 3, normalize="origin")
    assert same_arrays(norm, np.array([[2 / 3, 0.0, 1 / 3], [0.0, 0.0, 0.0], [1 / 3, 2 / 3, 0.0]]))  # the empty row stays 0, outside rows do not count
    (i, j, c), (io, co) = connectivity_numpy(origin, dest, 3, 3, sparse=True, return_outside=True)
    assert same_arrays(i, np.array([0, 0, 2, 2], np.int64)) and same_arrays(j, np.array([0, 2, 0, 1], np.int64))  # sorted by (i, j)
    assert same_arrays(c, np.array([2, 1, 1, 2], np.int64))
    assert same_arrays(io, np.array([0, 2], np.int64)) and same_arrays(co, np.array([1, 1], np.int64))
    assert same_arrays(sparse_to_dense(i, j, c, 3, 3), t)
    # "exactly np.unique(origin * n_dest + dest, return_counts=True), split again with divmod" over the tracked rows that are inside
    ok = (origin >= 0) & (dest >= 0)
    keys, counts = np.unique(origin[ok] * 3 + dest[ok], return_counts=True)
    assert np.array_equal(np.divmod(keys, 3), (i, j)) and np.array_equal(counts, c)
    i2, j2, cn = connectivity_numpy(origin, dest, 3, 3, sparse=True, normalize="origin")
    assert np.array_equal(i2, i) and np.array_equal(j2, j) and same_arrays(cn, np.array([2 / 3, 1 / 3, 1 / 3, 2 / 3]))
    # more origins than destinations, and nothing tracked
    wide = connectivity_numpy(origin, dest, 5, 3)
    assert wide.shape == (5, 3) and same_arrays(wide[:3], t) and not wide[3:].any()
    none, out = connectivity_numpy(-np.ones(4, np.int64), np.zeros(4, np.int64), 3, 3, return_outside=True)
    assert not none.any() and not out.any()
    (i, j, c), (io, co) = connectivity_numpy(-np.ones(4, np.int64), np.zeros(4, np.int64), 3, 3, sparse=True, return_outside=True)
    assert i.size == j.size == c.size == io.size == co.size == 0 and c.dtype == np.int64


def test_the_engine_chooses_the_path_by_size(monkeypatch):
    from parcels_amd.engine import CONNECTIVITY_LDS_BINS, connectivity_path

    monkeypatch.delenv("PK_CONNECTIVITY_PATH", raising=False)
    assert CONNECTIVITY_LDS_BINS == 8192
    assert connectivity_path(64, 127, False) == _hip.PK_CONN_LDS  # 64 * 128 = 8192 keys
    assert connectivity_path(64, 128, False) == _hip.PK_CONN_GLOBAL
    assert connectivity_path(64, 64, False) == _hip.PK_CONN_LDS and connectivity_path(64, 64, True) == _hip.PK_CONN_SPARSE
    for name, code in (("lds", _hip.PK_CONN_LDS), ("global", _hip.PK_CONN_GLOBAL), ("sparse", _hip.PK_CONN_SPARSE)):
        monkeypatch.setenv("PK_CONNECTIVITY_PATH", name)
        assert connectivity_path(64, 64, False) == connectivity_path(64, 64, True) == code
    monkeypatch.setenv("PK_CONNECTIVITY_PATH", "fast")
    with pytest.raises(ValueError, match="PK_CONNECTIVITY_PATH"):
        connectivity_path(64, 64, False)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_documented_and_bound():
    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    assert int(re.search(r"#define\s+PK_ABI_VERSION\s+(\d+)", header).group(1)) == 9 == _hip.PK_ABI_VERSION
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    docs = {}
    for sym in ("pk_particles_cells", "pk_particles_connectivity"):
        assert sym in _hip.ABI_SYMBOLS and f"| `{sym}` |" in notes
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct \{[^}]*\}\s*pk_connectivity_info_t;\s*)*int32_t " + sym + r"\(", header, re.S)
        assert m, f"the declaration of {sym} follows its comment"
        docs[sym] = m.group(1)
    for word in ("grid.search", "populate_indices", "pset.x", "HOST row order", "non-finite", "negative", "-1"):
        assert word in docs["pk_particles_cells"], word  # what host code the export replaces, and its rules
    for word in ("np.unique", "np.bincount", "n_dest + 1", "o < 0", "n_above", "PK_CONN_LDS", "8192", "2^62", "run-length", "ascending"):
        assert word in docs["pk_particles_connectivity"], word
    order = [header.index(f"int32_t {s}(") for s in ("pk_particles_density", "pk_particles_cells", "pk_particles_connectivity", "pk_measure_copy_bandwidth")]
    assert order == sorted(order)
    for name, value in (("PK_CONN_LDS", 0), ("PK_CONN_GLOBAL", 1), ("PK_CONN_SPARSE", 2)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value == getattr(_hip, name)
    fields = re.search(r"typedef struct \{([^}]*)\}\s*pk_connectivity_info_t;", header).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names == [n for n, _ in _hip.ConnectivityInfo._fields_] and ctypes.sizeof(_hip.ConnectivityInfo) == 72
    mk = open(os.path.join(ROOT, "parcels_amd", "csrc", "Makefile")).read()
    assert "pk_connectivity.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    deps = re.search(r"^%\.o: (.*)$", mk, re.M).group(1)
    assert "pk_connectivity.h" in deps and "pk_density_cell.h" in deps
    lib = _hip.load()
    assert hasattr(lib, "pk_particles_cells") and hasattr(lib, "pk_particles_connectivity")


def test_the_cell_rule_is_stated_once():
    """density_cell lives in the header both translation units include"""
    csrc = os.path.join(ROOT, "parcels_amd", "csrc")
    defined = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")) and re.search(r"long long density_cell\(", open(os.path.join(csrc, f)).read())]
    assert defined == ["pk_density_cell.h"]
    for f in ("pk_density.hip", "pk_connectivity.hip"):
        assert '#include "pk_density_cell.h"' in open(os.path.join(csrc, f)).read()
