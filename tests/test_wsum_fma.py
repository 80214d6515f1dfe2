"""fma(w, u, s) == s + w*u in every bit for w = 1 and w = 2 (csrc/pk_fast_agrid.h: fma3s), on the host.

w*u is exact for w = 1, and for w = 2 whenever |u| < 2^1023 (a change of the exponent; a subnormal doubles exactly), so both forms round the
same exact sum once.  |u| >= 2^1023 is the documented exception (2*u overflows before the addition) and is left out.  A small C function, built
with the oracle's compiler and -ffp-contract=off so that `s + w*u` stays two roundings, evaluates both forms; the results are compared as bit
patterns, NaNs as NaNs (their payload and sign are not part of any result column's contract)."""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

SRC = r"""
#include <math.h>
#include <stdint.h>
void wsum_both(int64_t n, double w, const double* u, const double* s, double* fused, double* plain) {
    for (int64_t i = 0; i < n; i++) {
        volatile double p = w * u[i];
        plain[i] = s[i] + p;
        fused[i] = fma(w, u[i], s[i]);
    }
}
"""


def _lib(tmp_path):
    src, so = os.path.join(tmp_path, "wsum.c"), os.path.join(tmp_path, "wsum.so")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    lib.wsum_both.argtypes = [C.c_int64, C.c_double] + [C.c_void_p] * 4
    return lib


def _inputs():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2**64, size=(2, 1_000_000), dtype=np.uint64)
    u, s = bits[0].view(np.float64), bits[1].view(np.float64)
    tiny = np.nextafter(0.0, 1.0)
    special = np.array([0.0, -0.0, tiny, -tiny, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 1.5, 1e3, -1e3,
                        np.nextafter(2.0**1023, 0.0), -np.nextafter(2.0**1023, 0.0), np.inf, -np.inf, np.nan, np.finfo(np.float64).max, -np.finfo(np.float64).max])
    su, ss = np.meshgrid(special, special)
    # subnormal u against s of every size; an s that cancels w*u exactly or nearly
    sub = (rng.integers(1, 2**52, size=20_000, dtype=np.uint64) | (rng.integers(0, 2, size=20_000, dtype=np.uint64) << np.uint64(63))).view(np.float64)
    u = np.concatenate([u, su.ravel(), sub, sub, u[:20_000], u[:20_000]])
    s = np.concatenate([s, ss.ravel(), s[:20_000], -sub, -u[:20_000], -2 * u[:20_000]])
    keep = ~(np.abs(u) >= 2.0**1023)  # (NaN and every |u| below 2^1023 stay; infinities go with the overflow range)
    inf_u = np.isinf(u)
    return np.ascontiguousarray(u[keep | inf_u]), np.ascontiguousarray(s[keep | inf_u])


def test_fused_weighted_sum_equals_two_roundings(tmp_path):
    lib = _lib(str(tmp_path))
    u, s = _inputs()
    assert len(u) > 1_000_000 and (np.abs(u[np.isfinite(u)]) < 2.0**1023).all()
    assert ((u != 0) & (np.abs(u) < 2.2250738585072014e-308)).sum() > 40_000 and np.isnan(u).any() and np.isinf(u).any() and (u == 0).any()
    for w in (1.0, 2.0):
        fused, plain = np.empty_like(u), np.empty_like(u)
        with np.errstate(all="ignore"):
            lib.wsum_both(len(u), w, u.ctypes.data, s.ctypes.data, fused.ctypes.data, plain.ctypes.data)
        nan = np.isnan(plain)
        assert np.array_equal(nan, np.isnan(fused))
        same = fused.view(np.uint64) == plain.view(np.uint64)
        assert same[~nan].all(), (w, u[~nan & ~same][:5], s[~nan & ~same][:5])
