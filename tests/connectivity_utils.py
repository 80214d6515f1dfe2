"""Helpers shared by tests/test_connectivity_host.py and tests/test_gpu_connectivity.py: a NumPy restatement of ParticleSet.connectivity that
turns origin labels and expected destination labels into the matrix, its sorted-COO form and the outside counts."""

import numpy as np


def connectivity_numpy(origin, dest, n_origin, n_dest, sparse=False, normalize=None, return_outside=False):
    """ParticleSet.connectivity restated.  `origin`: per particle its origin label (negative: not tracked); `dest`: per particle its
    destination label, or -1 (outside).  The key of a tracked row is origin * (n_dest + 1) + d with d = n_dest for an outside row, so the
    outside counts are one more column; dense is np.bincount of the keys, sparse np.unique(..., return_counts=True) split with divmod."""
    origin, dest = np.asarray(origin, dtype=np.int64), np.asarray(dest, dtype=np.int64)
    assert origin.shape == dest.shape and origin.ndim == 1
    assert not np.any(origin >= n_origin) and not np.any(dest >= n_dest)
    tracked = origin >= 0
    d = np.where(dest[tracked] < 0, n_dest, dest[tracked])
    key = origin[tracked] * (n_dest + 1) + d
    if not sparse:
        full = np.bincount(key, minlength=n_origin * (n_dest + 1)).astype(np.int64).reshape(n_origin, n_dest + 1)
        t, outside = np.ascontiguousarray(full[:, :n_dest]), full[:, n_dest].copy()
        if normalize == "origin":
            total = t.sum(axis=1, keepdims=True)
            t = np.divide(t, total, out=np.zeros(t.shape, np.float64), where=total != 0)
        return (t, outside) if return_outside else t
    keys, counts = np.unique(key, return_counts=True)
    i, j = np.divmod(keys.astype(np.int64), n_dest + 1)
    counts = counts.astype(np.int64)
    inside = j < n_dest
    out = (i[~inside], counts[~inside])
    i, j, counts = i[inside], j[inside], counts[inside]
    if normalize == "origin":
        total = {int(r): counts[i == r].sum() for r in np.unique(i)}
        counts = counts / np.array([total[int(r)] for r in i], dtype=np.float64) if i.size else counts.astype(np.float64)
    return ((i, j, counts), out) if return_outside else (i, j, counts)


def sparse_to_dense(i, j, counts, n_origin, n_dest):
    t = np.zeros((n_origin, n_dest), np.asarray(counts).dtype)
    t[i, j] = counts
    return t


def same_arrays(a, b):
    """exact: dtype, shape and every value"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
