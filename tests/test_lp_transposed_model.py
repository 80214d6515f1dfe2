"""The transposed block fetch of the level-pair cache (csrc/pk_fast_agrid.h: lp_fetch_xposed) forms lp_field's bits, on the host.

Sixteen helper lanes hold one corner row {cx, cy} each of a missing lane's cell -- lane j: bit 0 = k (depth row), bit 1 = r (lat row), bit 2 = l
(time level), bit 3 = f (U / V) -- and run three exchange steps: the z lerp with lane j^1, the level difference with lane j^4, the polynomial basis
with lane j^2.  The k = 0 lane (f, l, r) then holds entry q = 4f + 2l + r of the slot: p0, p1, d0, d1 of U, then of V.  A small C function emulates
the sixteen lanes (every step reads the values all lanes held BEFORE it, as a cross-lane read does); a second one transcribes lp_field for the four
(lenT, lenZ) cases.  Both are built with -ffp-contract=off -- the fused operations are the explicit fma() calls, as in the kernel's translation unit
-- and compared as bit patterns, NaNs as NaNs.  Rows the reference does not read (level ti + 1 without lenT, the lower depth row without lenZ) are
poisoned in the model's input: a helper masked out of the load must not reach the result.  The kernel follows this lane map and operation order."""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
typedef struct { double x, y; } pair;

/* lp_field (pk_fast_agrid.h) for one field: rows[l][k][r] = the two x-neighbours of (level ti + l, depth zi + k, lat yi + r) */
static void lp_field_ref(const pair rows[2][2][2], int LT, int LZ, double zeta, pair out[4]) {
    double a00 = rows[0][0][0].x, a01 = rows[0][0][0].y, a10 = rows[0][0][1].x, a11 = rows[0][0][1].y;
    if (LZ) {
        a00 = fma(zeta, rows[0][1][0].x - a00, a00); a01 = fma(zeta, rows[0][1][0].y - a01, a01);
        a10 = fma(zeta, rows[0][1][1].x - a10, a10); a11 = fma(zeta, rows[0][1][1].y - a11, a11);
    }
    out[0].x = a00; out[0].y = a01 - a00; out[1].x = a10 - a00; out[1].y = (a11 - a10) - (a01 - a00);
    out[2].x = out[2].y = out[3].x = out[3].y = 0.0;
    if (LT) {
        double b00 = rows[1][0][0].x, b01 = rows[1][0][0].y, b10 = rows[1][0][1].x, b11 = rows[1][0][1].y;
        if (LZ) {
            b00 = fma(zeta, rows[1][1][0].x - b00, b00); b01 = fma(zeta, rows[1][1][0].y - b01, b01);
            b10 = fma(zeta, rows[1][1][1].x - b10, b10); b11 = fma(zeta, rows[1][1][1].y - b11, b11);
        }
        const double e00 = b00 - a00, e01 = b01 - a01, e10 = b10 - a10, e11 = b11 - a11;
        out[2].x = e00; out[2].y = e01 - e00; out[3].x = e10 - e00; out[3].y = (e11 - e10) - (e01 - e00);
    }
}

/* the sixteen helper lanes; c[j]: what lane j loaded ({0, 0} where it is masked out of the load) */
static void lanes16(const pair in[16], int LT, int LZ, double zeta, pair out[8]) {
    pair c[16], n[16];
    for (int j = 0; j < 16; j++) {
        const int k = j & 1, l = (j >> 2) & 1;
        const int reads = (!k || LZ) && (!l || LT);
        c[j].x = reads ? in[j].x : 0.0;
        c[j].y = reads ? in[j].y : 0.0;
    }
    /* 1: the k = 0 lanes lerp in z with the pair of lane j^1 */
    for (int j = 0; j < 16; j++) {
        const pair d = c[j ^ 1];
        n[j] = c[j];
        if (!(j & 1) && LZ) { n[j].x = fma(zeta, d.x - c[j].x, c[j].x); n[j].y = fma(zeta, d.y - c[j].y, c[j].y); }
    }
    memcpy(c, n, sizeof c);
    /* 2: the l = 1 lanes subtract the pair of lane j^4 (level ti), or hold zero */
    for (int j = 0; j < 16; j++) {
        const pair a = c[j ^ 4];
        n[j] = c[j];
        if (j & 4) {
            if (LT) { n[j].x = c[j].x - a.x; n[j].y = c[j].y - a.y; }
            else n[j].x = n[j].y = 0.0;
        }
    }
    memcpy(c, n, sizeof c);
    /* 3: h = cy - cx everywhere; the r = 1 lanes subtract {cx, h} of lane j^2 */
    for (int j = 0; j < 16; j++) c[j].y = c[j].y - c[j].x;
    for (int j = 0; j < 16; j++) {
        const pair o = c[j ^ 2];
        n[j] = c[j];
        if (j & 2) { n[j].x = c[j].x - o.x; n[j].y = c[j].y - o.y; }
    }
    for (int j = 0; j < 16; j += 2) {
        const int r = (j >> 1) & 1, l = (j >> 2) & 1, f = (j >> 3) & 1;
        out[4 * f + 2 * l + r] = n[j];
    }
}

/* rows: n x 16 pairs in lane order; poison: what the rows the reference does not read hold in the model's input */
void lp_both(int64_t n, int LT, int LZ, const double* rows, const double* zeta, double poison, double* model, double* ref) {
    for (int64_t i = 0; i < n; i++) {
        pair in[16], fr[2][2][2][2];
        for (int j = 0; j < 16; j++) {
            const int k = j & 1, r = (j >> 1) & 1, l = (j >> 2) & 1, f = (j >> 3) & 1;
            in[j].x = rows[(i * 16 + j) * 2];
            in[j].y = rows[(i * 16 + j) * 2 + 1];
            fr[f][l][k][r] = in[j];
            if ((k && !LZ) || (l && !LT)) in[j].x = in[j].y = poison;
        }
        lanes16(in, LT, LZ, zeta[i], (pair*)(model + i * 16));
        lp_field_ref(fr[0], LT, LZ, zeta[i], (pair*)(ref + i * 16));
        lp_field_ref(fr[1], LT, LZ, zeta[i], (pair*)(ref + i * 16 + 8));
    }
}
"""


def _lib(tmp_path):
    src, so = os.path.join(tmp_path, "lpx.c"), os.path.join(tmp_path, "lpx.so")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    lib.lp_both.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    return lib


def _inputs():
    rng = np.random.default_rng(7)
    n = 100_000
    tiny = np.nextafter(0.0, 1.0)
    special = np.array([0.0, -0.0, tiny, -tiny, 1e-310, -1e-310, 2.2250738585072014e-308, 1.0, -1.0, 0.1, np.inf, -np.inf, np.nan, 1e300, -1e300])
    sets = [
        rng.normal(0.0, 1.0, size=(n, 32)),                                       # velocities
        rng.integers(0, 2**64, size=(20_000, 32), dtype=np.uint64).view(np.float64),  # every exponent, NaNs and infinities among them
        special[rng.integers(0, len(special), size=(20_000, 32))],                 # +-0, subnormals, infinities, NaN corners
        np.repeat(rng.normal(0.0, 1.0, size=(5_000, 1)), 32, axis=1),              # equal corners: every difference cancels to +-0
        np.repeat(special[:, None], 32, axis=1),
        (rng.integers(1, 2**52, size=(10_000, 32), dtype=np.uint64) | (rng.integers(0, 2, size=(10_000, 32), dtype=np.uint64) << np.uint64(63))).view(np.float64),
    ]
    # equal rows in pairs (z, t or y neighbours alike) and a single NaN corner in otherwise ordinary cells
    pairs = rng.normal(0.0, 1.0, size=(10_000, 32))
    for bit in (1, 2, 4):
        p = pairs[:3_000].copy().reshape(-1, 16, 2)
        idx = np.arange(16)
        p[:, idx | bit] = p[:, idx & ~bit]
        sets.append(p.reshape(-1, 32))
    one_nan = rng.normal(0.0, 1.0, size=(3_200, 32))
    one_nan[np.arange(3_200), np.arange(3_200) % 32] = np.nan
    sets.append(one_nan)
    rows = np.ascontiguousarray(np.concatenate(sets))
    m = len(rows)
    zeta = rng.random(m)
    zeta[0::5] = 0.0
    zeta[1::5] = 1.0
    zeta[2::50] = np.nextafter(1.0, 0.0)
    zeta[3::50] = tiny
    return rows, np.ascontiguousarray(zeta)


def test_sixteen_lane_exchange_forms_lp_field_bits(tmp_path):
    lib = _lib(str(tmp_path))
    rows, zeta = _inputs()
    m = len(rows)
    assert m >= 100_000 and np.isnan(rows).any() and np.isinf(rows).any() and (rows == 0).any()
    assert ((rows != 0) & (np.abs(rows) < 2.2250738585072014e-308)).sum() > 100_000
    for LT in (0, 1):
        for LZ in (0, 1):
            for poison in (np.nan, 1e308):
                model, ref = np.empty((m, 16)), np.empty((m, 16))
                with np.errstate(all="ignore"):
                    lib.lp_both(m, LT, LZ, rows.ctypes.data, zeta.ctypes.data, poison, model.ctypes.data, ref.ctypes.data)
                nan = np.isnan(ref)
                assert np.array_equal(nan, np.isnan(model)), (LT, LZ)
                same = model.view(np.uint64) == ref.view(np.uint64)
                bad = ~nan & ~same
                assert not bad.any(), (LT, LZ, np.argwhere(bad)[:5], model[bad][:5], ref[bad][:5])
                if not LT:  # level ti + 1 is not read: D is +0 in every bit
                    assert (model.reshape(m, 2, 4, 2)[:, :, 2:].view(np.uint64) == 0).all()
