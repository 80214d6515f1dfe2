// pk_fast_agrid.h -- VectorField.eval for the headline configuration: XLinear_Velocity on a rectilinear A-grid with
// float64 coordinates (BASELINE config 2; field.py:250-304, index_search.py:20-91, _xinterpolators.py:25-190).
//
// Same arithmetic, expression by expression, as the general eval_uvw<FT, 0, 0, false> of pk_device.h -- the parity tests run
// both against the same fixtures -- but laid out for the CDNA4 issue ports:
//   * everything the general path re-derives per evaluation from the field / grid descriptors (strides, extents, slot
//     arithmetic, layout comparisons) is folded into one small `FastA` block of wave-uniform values by the host;
//   * the 1-D coordinate vectors are staged into LDS as {a[i], 1 / (a[i+1] - a[i])} pairs: the barycentric quotient
//     (x - a[i]) / (a[i+1] - a[i]) is formed with the correctly rounded reciprocal and two fused residual steps (Markstein's
//     theorem: identical to the IEEE quotient) -- 5 fp64 issue slots instead of the ~14 of v_div_scale / v_rcp / v_div_fmas;
//   * the time level, and whether the second time / depth level takes part, is made wave-uniform with a readfirstlane
//     waterfall (one pass unless particles of one wavefront sit on different time levels): level base addresses live in
//     SGPRs, every corner-pair load is `global_load_dwordx4 v, v_off, s[base]` with ONE shared 32-bit lane offset, and the
//     lenT / lenZ selects of the general path become scalar branches;
//   * the particle storage dtype is a template parameter.
#pragma once
#include "pk_device.h"

namespace pk {

// interleaved coordinate table entry: node value and reciprocal of the width of the cell that starts there
typedef double pk_tab2 __attribute__((ext_vector_type(2)));

struct FastTabs {  // LDS-resident {a, 1/width} tables of the main grid and the velocity field's time axis
    const pk_tab2* time;
    const pk_tab2* depth;
    const pk_tab2* lat;
    const pk_tab2* lon;
    pk_tab2* blk;  // this lane's corner-block cache (FCtx::bei): 4 x 16 bytes at stride FAST_WG (stage-pair block), or 8 x 16 bytes at stride
                   // FAST_WG_LP (level-pair cache: the Z0 and D rows of U and V, eval_uvw_lp); NULL = none
    uint32_t fl;   // FA_* bits of the wave-uniform yes / no questions of one evaluation (fast_flags)
    // Scalars of FastA that every evaluation reads, copied by the kernel (copy_scalars).  Built and not kept: pinning them in scalar registers
    // behind an opaque asm, so that no evaluation re-loads them from the kernel-argument segment -- measured (profiles/r06c_*), the pinned
    // build was no faster than the one that re-loads them (7.92-7.97 vs 7.60-7.63 ms on two boxes whose round-5 baselines differ by 2 %).
    double tlen;
    int32_t gny, gnx;
    // the two factors of the unit conversion, made opaque scalars once per step by the step loop of the kernels that hold their block
    // (fast_held; pk_kernels.h)
    double deg2m, inv_deg2m;
};
PK_DEV void copy_scalars(FastTabs& T, const FastA& F) {
    T.tlen = F.tlen;
    T.gny = F.gny;
    T.gnx = F.gnx;
}
// The wave-uniform booleans of an evaluation as bits of ONE scalar register.  Kept as separate loop-invariant i1 values the compiler
// holds each of them as a 64-bit lane mask (`s_cselect_b64 -1, 0`): two SGPRs per question, 46 SGPRs spilled to VGPR lanes in round 5's
// kernel and a `v_readlane_b32` -- a VALU instruction -- for every use inside the stage loop.  The evaluators re-read the word through
// an opaque scalar at their top, so every test is an `s_bitcmp` + `s_cbranch_scc` where it is used.
enum : uint32_t {
    FA_TI = 1u, FA_Z = 2u, FA_Y = 4u, FA_X = 8u, FA_SPH = 16u, FA_RING = 32u, FA_BLK = 64u,
    FA_NT2 = 128u, FA_NZ2 = 256u, FA_NY2 = 512u, FA_NX2 = 1024u,  // the axis has at least two nodes (index_search.py:45-46)
    FA_WIN = 2048u, FA_FWD = 4096u, FA_MAXIT = 8192u               // step loop: some ring streams; dt0 > 0; an iteration limit is set
};
PK_DEV uint32_t fast_flags(const FastA& F) {
    return (F.has_ti ? FA_TI : 0u) | (F.has_z ? FA_Z : 0u) | (F.has_y ? FA_Y : 0u) | (F.has_x ? FA_X : 0u) | (F.spherical ? FA_SPH : 0u) |
           (F.nslots < F.nt ? FA_RING : 0u) | (F.lds_blk != 0 ? FA_BLK : 0u) | (F.nt >= 2 ? FA_NT2 : 0u) | (F.gnz >= 2 ? FA_NZ2 : 0u) |
           (F.gny >= 2 ? FA_NY2 : 0u) | (F.gnx >= 2 ? FA_NX2 : 0u);
}
// Square root, quotient and reciprocal WITHOUT the library's range scaling and final fix-up (PK_CG_LEAN / PK_FAST_LEAN, round 6; the tolerance
// argument of pk_fast_cgrid.h: sincos_near): the operands here are lengths in metres, squared or not, determinants and Jacobians of cells -- far from the
// subnormal and overflow ranges the library's 20-instruction sqrt and 10-instruction division guard -- and one Goldschmidt / Newton
// step + one residual correction on the hardware's v_rsq_f64 / v_rcp_f64 leaves < 1 ulp (not always the correctly rounded bit).
#ifndef PK_CG_LEAN
#define PK_CG_LEAN 1
#endif
PK_DEV double sqrt_lean(double x) {  // x > 0 (0, negative, NaN: the caller selects)
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    return fma(fma(-g, g, x), h, g);
}
PK_DEV double rcp_lean(double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = fma(r, fma(-b, r, 1.0), r);
    return fma(r, fma(-b, r, 1.0), r);
}
PK_DEV double div_lean(double a, double b) {
    const double r = rcp_lean(b), q = a * r;
    return fma(fma(-b, q, a), r, q);
}

// Barycentric coordinate of x in the cell [a, a1] of an {a, 1 / width} table.  PK_FAST_LEAN (round 6, default): (x - a) * RN(1 / width), one
// multiplication, within 1.5 ulp of the reference's (x - a) / (a1 - a) and never above 1 for x <= a1 (n * RN(1 / d) <= RN(1 + 2^-53) = 1);
// 0: the correctly rounded quotient (div_by_recip: five fused operations + a guard), the bits of the general program.  The index, the
// out-of-bounds codes and "exactly on a node / level" (bc == 0) do not depend on the choice.
#ifndef PK_FAST_LEAN
#define PK_FAST_LEAN 1
#endif
// (Contracting the lerps and bilinear sums of this kernel into fused multiply-adds -- `#pragma clang fp contract(fast)` in lerp_rows / uvw_fast,
// 70 of its 286 fp64 instructions -- was measured and is not done: 6.99 -> 6.98 ms, profiles/r06v_contraction_ab.txt.  The C-grid
// evaluation is contracted: pk_fast_cgrid.h, PK_CG_FMA.)
PK_DEV double fast_bary(double x, double a, double a1, double rw) {
    if constexpr (PK_FAST_LEAN != 0) return (x - a) * rw;
    else return div_by_recip(x - a, a1 - a, rw);
}
// cos(lat) of the unit conversion (PK_FAST_LEAN builds): with h = lat * pi / 360, cos(2h) = 1 - 2 sin(h)^2 and sin(h) from the minimax kernel cos_lat
// uses beyond 45 degrees (S1..S6, valid to |h| <= pi/4): ONE region without a branch for |lat * pi / 180| <= 1.5 where cos_lat has three, 12 VALU
// instructions where the ISA of cos_lat shows 25-27 plus two exec-mask regions.
//   * The coefficients are handed over in scalar registers at the place of use (an SGPR pair is a legal addend of v_fma_f64).  As loop-invariant
//     values they sat in VGPRs across the stage loop, each copied (v_mov_b64) in front of the v_fmac_f64 that would have destroyed it.
//   * Beyond 1.5 rad (unlikely: +-86 degrees, or a stray particle) cos_lat itself, behind a CALL: inlined, the nine coefficients of its two
//     kernels are kept in 18 VGPRs across the stage loop for a block that almost never runs.  The callee is a leaf without scratch and the call
//     site saves nothing: advect_fast_kernel<double, 0, false, FAST_LP_CACHE> went from 126 VGPRs + 12 B of scratch to 114 and none.
// Accuracy: the cancellation in 1 - 2 s^2 leaves an ABSOLUTE error of at most (1 - cos) * 2^-51 + ulp / 2, so more ulps the smaller the cosine.
// Measured on the device against cosl() of the same argument (tools/cos_lean_check.hip, 4.7e6 latitudes; tests/test_gpu_fast_eval_lean.py holds
// the bound), maximum in ulps of the result per band of |lat| in degrees:
//   0-30: 0.76   30-60: 1.07   60-76: 6.1   76-80: 6.6   80-84: 13.7   84-85.94: 14.2 (1.6e-15 relative)   beyond (cos_lat): 0.51
// and never more than 1.8 * 2^-53 absolute.
static __device__ __attribute__((noinline)) double cos_lat_far(double x) { return cos_lat(x); }
PK_DEV double cos_lat_lean(double lat_deg) {
    const double h = lat_deg * (0.5 * DEG2RAD);  // (halving RN(pi / 180) is exact: h == 0.5 * (lat * DEG2RAD), the argument of cos_lat, halved)
    if (__builtin_expect(!(fabs(h) <= 0.75), 0)) return cos_lat_far(lat_deg * DEG2RAD);
    double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
           S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    asm volatile("" : "+s"(S1), "+s"(S2), "+s"(S3), "+s"(S4), "+s"(S5), "+s"(S6));
    const double z = h * h;
    const double r = fma(z, fma(z, fma(z, fma(z, fma(z, S6, S5), S4), S3), S2), S1);
    const double s = fma(z * h, r, h);
    return fma(-2.0 * s, s, 1.0);
}

constexpr int FAST_WG = 256;                          // lanes per workgroup of advect_fast_kernel
constexpr int FAST_BLK_BYTES = FAST_WG * 8 * 8;       // LDS of the corner-block cache per workgroup (8 doubles per lane)
// Modes of the 2-D kernel's corner cache (template parameter LP of advect_fast_kernel, which calls eval_uvw_fast for the first and eval_uvw_lp for the other two; pk_set_option "block_cache"):
//   FAST_LP_OFF   the stage-pair block of FCtx::bei, or nothing (wave-uniform at run time: FA_BLK), lerps in the reference's order;
//   FAST_LP_REGS  the level-pair arithmetic (lp_field) with Z0 / D formed in registers in every evaluation: the A/B partner of the cache;
//   FAST_LP_CACHE the level-pair cache: Z0 / D of the lane's cell live in its LDS slot across evaluations.
// The cache needs 128 bytes per lane: with 256-lane workgroups the 32 KB + tables allow three workgroups per CU (12 waves), so this mode
// runs 512-lane workgroups, two of which fill the 16 wave slots of a CU (4 per SIMD) when 2 x (tables + 64 KB) fit in the 160 KB of LDS.
constexpr int FAST_LP_OFF = 0, FAST_LP_REGS = 1, FAST_LP_CACHE = 2;
constexpr int FAST_WG_LP = 512;                       // lanes per workgroup of advect_fast_kernel<.., FAST_LP_CACHE>
constexpr int FAST_LP_BYTES = FAST_WG_LP * 16 * 8;    // LDS of the level-pair cache per workgroup (16 doubles per lane)
constexpr int fast_wg(int lp) { return lp == FAST_LP_CACHE ? FAST_WG_LP : FAST_WG; }

// clip(searchsorted(arr, x, "left") - 1, 0, n-2) over the interleaved table.  Cold (a lane that moved two cells or more, or holds a
// NaN): one bisection loop -- the unrolled three-step walk of rounds 1-5 found the same index and cost the hot path seven nesting
// levels of saved exec masks (14 SGPRs) at each of its four inlined copies.
PK_DEV int cell_index_tab(const pk_tab2* tab, int n, double x) {
    asm volatile("" : "+s"(n));  // (wave-uniform; opaque so that `0 < n` of the loop entry is not hoisted into a saved lane mask)
    if (x != x) return n - 2;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].x < x) lo = mid + 1; else hi = mid;
    }
    return clampi(lo - 1, 0, n - 2);
}

// _search_1d_array (index_search.py:20-62) for a float64 coordinate: the hinted cell is right for all but the lanes that just
// crossed a cell edge.  `cell` (in / out): a valid cell index 0..n-2, the hint on entry and the cell found on exit; idx: that
// cell or the out-of-bounds code.  The cell test is NaN-proof as written: a NaN fails it unless the hint already is the
// last cell (NumPy sorts NaN last), and cell_index_tab answers n-2.
// FLAGGED: the caller answers "n >= 2" itself (`two`, a bit of FastTabs::fl tested where it is used).
template <bool FLAGGED = false>
PK_DEV void fast_search(const pk_tab2* tab, int n, double first, double last, double x, int& cell, int& idx, double& bc, bool two = true,
                        pk_tab2* kept = nullptr, double* kept1 = nullptr) {
    if (FLAGGED ? !two : n < 2) {  // :45-46
        idx = 0;
        bc = 0.0;
        return;
    }
    int i = cell;
    pk_tab2 e = tab[i];
    double a1 = tab[i + 1].x;
    const bool lo_ok = e.x < x || i == 0, hi_ok = x <= a1 || i == n - 2;
    if (!(lo_ok && hi_ok)) {
        // Some lane of nearly every wavefront crosses a cell edge in nearly every evaluation, so this block is hot: the neighbour
        // cell the failed test points at is probed without a loop (one LDS round trip for the whole wave); only lanes that moved
        // further, or hold a NaN, take the walk + bisect of cell_index_tab.  (!hi_ok implies i < n-2, !lo_ok implies i > 0.)
        int j = i + (hi_ok ? 0 : 1) - (lo_ok ? 0 : 1);
        pk_tab2 e2 = tab[j];
        double b1 = tab[j + 1].x;
        asm volatile("" : "+v"(b1));  // both reads in flight together (not the second one behind the first compare's short circuit)
        if (__builtin_expect(!((e2.x < x || j == 0) && (x <= b1 || j == n - 2)), 0)) {
            j = cell_index_tab(tab, n, x);
            e2 = tab[j];
            b1 = tab[j + 1].x;
        }
        i = j;
        e = e2;
        a1 = b1;
    }
    bc = fast_bary(x, e.x, a1, e.y);
    cell = i;
    if (kept) {  // (a compile-time NULL for the callers that do not ask: the entries of the cell found, FCtx::ta)
        *kept = e;
        *kept1 = a1;
    }
    // :55-58.  A point left of the first node is in cell 0, one right of the last node in cell n-2 (the clip of :47), so only lanes in
    // an edge cell pay the two fp64 compares (a divergent block most wavefronts skip: the particles live in the interior)
    if (__builtin_expect(i == 0 || i == n - 2, 0)) {
        if (x < first) i = LEFT_OUT_OF_BOUNDS;
        if (x > last) i = RIGHT_OUT_OF_BOUNDS;
    }
    idx = i;
}

// Two axes at once (lat and lon of one evaluation; both with n >= 2): the same answers as two fast_search calls, but the LDS round trips of
// the two axes overlap -- all four hint-cell reads are in flight together, and so are the four reads of the neighbour probes when some lane
// crossed an edge on either axis (which happens in nearly every wave-evaluation: round 5's kernel walked through up to six dependent
// ~100-cycle LDS round trips per evaluation here; the PMC pass showed 0.36 of its wave cycles in s_waitcnt and no gain from fewer VALU
// instructions alone, profiles/r06a_c2_flags_pmc.md).
// `kept` (a compile-time NULL for the callers that do not ask): the table entries of the cells found, for a caller that holds them (FCtx::ya).
struct CellEntries {
    pk_tab2 ea, eb;   // {a[i], 1 / width} of lat, lon
    double a1a, a1b;  // a[i + 1]
};
PK_DEV void fast_search2(const pk_tab2* taba, int na, double firsta, double lasta, double xa, int& cella, int& idxa, double& bca,
                         const pk_tab2* tabb, int nb, double firstb, double lastb, double xb, int& cellb, int& idxb, double& bcb,
                         CellEntries* kept = nullptr) {
    int ia = cella, ib = cellb;
    pk_tab2 ea = taba[ia], eb = tabb[ib];
    double a1a = taba[ia + 1].x, a1b = tabb[ib + 1].x;
    const bool lo_a = ea.x < xa || ia == 0, hi_a = xa <= a1a || ia == na - 2;
    const bool lo_b = eb.x < xb || ib == 0, hi_b = xb <= a1b || ib == nb - 2;
    if (!(lo_a && hi_a && lo_b && hi_b)) {
        // (an axis that passed keeps its cell: j == i, and the probe below re-reads the same entries)
        int ja = ia + (hi_a ? 0 : 1) - (lo_a ? 0 : 1), jb = ib + (hi_b ? 0 : 1) - (lo_b ? 0 : 1);
        pk_tab2 e2a = taba[ja], e2b = tabb[jb];
        double b1a = taba[ja + 1].x, b1b = tabb[jb + 1].x;
        asm volatile("" : "+v"(b1a), "+v"(b1b));  // all four reads issued before the first compare (not sunk behind its short circuit)
        if (__builtin_expect(!((e2a.x < xa || ja == 0) && (xa <= b1a || ja == na - 2)), 0)) {
            ja = cell_index_tab(taba, na, xa);
            e2a = taba[ja];
            b1a = taba[ja + 1].x;
        }
        if (__builtin_expect(!((e2b.x < xb || jb == 0) && (xb <= b1b || jb == nb - 2)), 0)) {
            jb = cell_index_tab(tabb, nb, xb);
            e2b = tabb[jb];
            b1b = tabb[jb + 1].x;
        }
        ia = ja; ea = e2a; a1a = b1a;
        ib = jb; eb = e2b; a1b = b1b;
    }
    bca = fast_bary(xa, ea.x, a1a, ea.y);
    bcb = fast_bary(xb, eb.x, a1b, eb.y);
    cella = ia;
    cellb = ib;
    if (__builtin_expect(ia == 0 || ia == na - 2 || ib == 0 || ib == nb - 2, 0)) {  // :55-58, see fast_search
        if (xa < firsta) ia = LEFT_OUT_OF_BOUNDS;
        if (xa > lasta) ia = RIGHT_OUT_OF_BOUNDS;
        if (xb < firstb) ib = LEFT_OUT_OF_BOUNDS;
        if (xb > lastb) ib = RIGHT_OUT_OF_BOUNDS;
    }
    idxa = ia;
    idxb = ib;
    if (kept) {
        kept->ea = ea; kept->a1a = a1a;
        kept->eb = eb; kept->a1b = a1b;
    }
}

// The two x-corners of one (level, z, y) row at byte offset `off` from a wave-uniform base: one wide load in saddr form.
template <class FT>
PK_DEV void ldrow(const char* base, uint32_t off, double& a, double& b) {
    ldpair(reinterpret_cast<const FT*>(base + off), a, b);
}

// XLinear.interp (_xinterpolators.py:112-153) for one field; LT / LZ: the second time / depth level takes part (wave-uniform,
// compile-time here so that the whole gather + interpolation of a field is ONE basic block of up to 8 wide loads).
// l0 / l1: wave-uniform bases of the two time levels; b00: byte offset of corner (zi, yi, xi) inside a level; dyb / dzb: byte
// strides to the yi+1 row / zi+1 plane (0 on an axis the field does not have).
struct Rows {  // the (up to) 16 corner values of one field: [time level][z][y] rows of two x-neighbours
    double c00, c01, c10, c11, t00, t01, t10, t11, d00, d01, d10, d11, e00, e01, e10, e11;
};
template <class FT, bool LT, bool LZ>
PK_DEV void load_rows(Rows& r, const char* l0, const char* l1, uint32_t b00, uint32_t dyb, uint32_t dzb) {
    ldrow<FT>(l0, b00, r.c00, r.c01);
    ldrow<FT>(l0 + dyb, b00, r.c10, r.c11);
    if (LT) {
        ldrow<FT>(l1, b00, r.t00, r.t01);
        ldrow<FT>(l1 + dyb, b00, r.t10, r.t11);
    }
    if (LZ) {
        ldrow<FT>(l0 + dzb, b00, r.d00, r.d01);
        ldrow<FT>(l0 + dzb + dyb, b00, r.d10, r.d11);
        if (LT) {
            ldrow<FT>(l1 + dzb, b00, r.e00, r.e01);
            ldrow<FT>(l1 + dzb + dyb, b00, r.e10, r.e11);
        }
    }
}
// lerp in t, then z, then bilinear in (eta, xsi) with the weights (1-xsi)(1-eta), xsi(1-eta), (1-xsi)eta, xsi*eta shared by U, V, W
// (lerp_rows: the t / z part -- a function of the cell and of (t, z) only; interp_rows: all of it)
template <bool LT, bool LZ>
PK_DEV void lerp_rows(const Rows& r, double tau, double omt, double zeta, double omz, double& c00, double& c01, double& c10, double& c11) {
    c00 = r.c00; c01 = r.c01; c10 = r.c10; c11 = r.c11;
    if (LT) {
        c00 = c00 * omt + r.t00 * tau; c01 = c01 * omt + r.t01 * tau;
        c10 = c10 * omt + r.t10 * tau; c11 = c11 * omt + r.t11 * tau;
    }
    if (LZ) {
        double d00 = r.d00, d01 = r.d01, d10 = r.d10, d11 = r.d11;
        if (LT) {
            d00 = d00 * omt + r.e00 * tau; d01 = d01 * omt + r.e01 * tau;
            d10 = d10 * omt + r.e10 * tau; d11 = d11 * omt + r.e11 * tau;
        }
        c00 = c00 * omz + d00 * zeta; c01 = c01 * omz + d01 * zeta;
        c10 = c10 * omz + d10 * zeta; c11 = c11 * omz + d11 * zeta;
    }
}
template <bool LT, bool LZ>
PK_DEV double interp_rows(const Rows& r, double tau, double omt, double zeta, double omz, double w00, double w01, double w10, double w11) {
    double c00, c01, c10, c11;
    lerp_rows<LT, LZ>(r, tau, omt, zeta, omz, c00, c01, c10, c11);
    return w00 * c00 + w01 * c01 + w10 * c10 + w11 * c11;
}

// U, V (and W) of one evaluation.  The corner rows of one field are requested back to back (one memory round trip per field; those of
// U and V together took more registers); the fences keep the machine scheduler from sinking the loads back between the arithmetic.
template <class FT, bool D3, bool LT, bool LZ>
PK_DEV void uvw_fast(const FastA& F, int64_t o0, int64_t o1, uint32_t b00, double tau, double omt, double zeta, double omz, double w00,
                     double w01, double w10, double w11, double& uu, double& vv, double& ww, pk_tab2* blk) {
    // keep the 32-bit lane offset opaque up to here: its zero-extension must sit in the basic block of the loads for the
    // instruction selector to fold it into the `saddr + voffset` addressing mode (otherwise one 64-bit VALU add per load)
    uint32_t bo = b00;
    asm volatile("" : "+v"(bo));
    Rows ru, rv, rw;
    load_rows<FT, LT, LZ>(ru, F.U + o0, F.U + o1, bo, F.dyb, F.dzb);
    PK_FIELD_FENCE();
    // the t / z-lerped corner blocks of U and V go to the lane's block cache (FCtx::bei) as soon as they exist; blk: wave-uniform NULL or not
    double c00, c01, c10, c11;
    lerp_rows<LT, LZ>(ru, tau, omt, zeta, omz, c00, c01, c10, c11);
    if (!D3 && blk) {
        pk_tab2 b;
        b.x = c00; b.y = c01; blk[0] = b;
        b.x = c10; b.y = c11; blk[FAST_WG] = b;
    }
    uu = w00 * c00 + w01 * c01 + w10 * c10 + w11 * c11;
    load_rows<FT, LT, LZ>(rv, F.V + o0, F.V + o1, bo, F.dyb, F.dzb);
    PK_FIELD_FENCE();
    lerp_rows<LT, LZ>(rv, tau, omt, zeta, omz, c00, c01, c10, c11);
    if (!D3 && blk) {
        pk_tab2 b;
        b.x = c00; b.y = c01; blk[2 * FAST_WG] = b;
        b.x = c10; b.y = c11; blk[3 * FAST_WG] = b;
    }
    vv = w00 * c00 + w01 * c01 + w10 * c10 + w11 * c11;
    if (D3) {
        load_rows<FT, LT, LZ>(rw, F.W + o0, F.W + o1, bo, F.dyb, F.dzb);
        PK_FIELD_FENCE();
        ww = interp_rows<LT, LZ>(rw, tau, omt, zeta, omz, w00, w01, w10, w11);
    }
}

// ---- level-pair cache (2-D kernel, PK_FAST_LEAN builds) --------------------------------------------------------------------------
// The z-lerped corner values of the two time levels, Z0[c] = zlerp(level ti), Z1[c] = zlerp(level ti + 1) (c: the four (y, x) corners, for U
// and V), depend on the cell, on z (which a 2-D kernel never moves) and on the level pair only -- not on the stage time.  They are kept
// per lane as Z0 and D = Z1 - Z0 and only the last lerp runs per evaluation:
//     Zk[c] = fma(zeta, d_k[c] - c_k[c], c_k[c])   (lenZ; else c_k[c])        D[c] = Z1[c] - Z0[c]   (lenT; else 0: level ti + 1 is not read)
//     v[c]  = fma(tau, D[c], Z0[c])
// ONE arithmetic whether the values come out of LDS or were just formed (FAST_LP_REGS forms them in every evaluation): a lane's result does
// not depend on its wavefront's other lanes, on launch splits or on the cache.  Against the reference's order (t first, then z, each
// a*(1-w) + b*w) the positions move by a few 1e-15 relative (the class of change PK_FAST_LEAN is).
// The block is kept in the POLYNOMIAL basis of the bilinear form, not as corner values: with a00, a01, a10, a11 the corners (y, x), (y, x+1),
// (y+1, x), (y+1, x+1) of Z0,
//     P0 = a00    Px = a01 - a00    Py = a10 - a00    Pxy = (a11 - a10) - (a01 - a00)
// and the same four combinations of D.  An evaluation then needs no weights: p* = fma(tau, D*, P*) four times and
//     value = fma(eta, fma(xsi, pxy, py), fma(xsi, px, p0))
// -- 7 fused operations per field where the corner form took 4 + 7, plus 6 for the weights U and V shared (28 -> 14 VALU per evaluation).  The
// differences are formed once per block, where it is fetched.  Against long double the absolute error is 7.6e-16 of the largest corner (the
// weights form: 4.0e-16): the class of change the level-pair arithmetic itself was.
// (Folding 1 / deg2m into the eight stored values of V would save one multiplication per evaluation and cost eight per fetch, which runs for
// the whole wavefront in ~0.2 of the wave-evaluations: not free, not done.)
struct LpField {  // {P0, Px}, {Py, Pxy} of Z0 and of D
    pk_tab2 p0, p1, d0, d1;
};
template <class FT, bool LT, bool LZ>
PK_DEV void lp_field(LpField& f, const char* l0, const char* l1, uint32_t bo, uint32_t dyb, uint32_t dzb, double zeta) {
    Rows r;
    load_rows<FT, LT, LZ>(r, l0, l1, bo, dyb, dzb);
    PK_FIELD_FENCE();
    double a00 = r.c00, a01 = r.c01, a10 = r.c10, a11 = r.c11;
    if (LZ) {
        a00 = fma(zeta, r.d00 - a00, a00); a01 = fma(zeta, r.d01 - a01, a01);
        a10 = fma(zeta, r.d10 - a10, a10); a11 = fma(zeta, r.d11 - a11, a11);
    }
    f.p0.x = a00; f.p0.y = a01 - a00; f.p1.x = a10 - a00; f.p1.y = (a11 - a10) - (a01 - a00);
    f.d0.x = f.d0.y = f.d1.x = f.d1.y = 0.0;
    if (LT) {
        double b00 = r.t00, b01 = r.t01, b10 = r.t10, b11 = r.t11;
        if (LZ) {
            b00 = fma(zeta, r.e00 - b00, b00); b01 = fma(zeta, r.e01 - b01, b01);
            b10 = fma(zeta, r.e10 - b10, b10); b11 = fma(zeta, r.e11 - b11, b11);
        }
        const double e00 = b00 - a00, e01 = b01 - a01, e10 = b10 - a10, e11 = b11 - a11;
        f.d0.x = e00; f.d0.y = e01 - e00; f.d1.x = e10 - e00; f.d1.y = (e11 - e10) - (e01 - e00);
    }
}
// Z0 / D of U and V at the lane's cell
template <class FT, bool LT, bool LZ>
PK_DEV void lp_fetch(const FastA& F, int64_t o0, int64_t o1, uint32_t b00, double zeta, LpField& fu, LpField& fv) {
    uint32_t bo = b00;  // (opaque lane offset: see uvw_fast)
    asm volatile("" : "+v"(bo));
    lp_field<FT, LT, LZ>(fu, F.U + o0, F.U + o1, bo, F.dyb, F.dzb, zeta);
    lp_field<FT, LT, LZ>(fv, F.V + o0, F.V + o1, bo, F.dyb, F.dzb, zeta);
}
PK_DEV double lp_sum(const LpField& f, double tau, double eta, double xsi) {
    const double p0 = fma(tau, f.d0.x, f.p0.x), px = fma(tau, f.d0.y, f.p0.y), py = fma(tau, f.d1.x, f.p1.x), pxy = fma(tau, f.d1.y, f.p1.y);
    return fma(eta, fma(xsi, pxy, py), fma(xsi, px, p0));
}

// lp_sum on a block that stays in its registers (fast_held): the four fma(tau, D*, P*) as the three-address v_fma_f64.  The compiler
// selects the two-address v_fmac_f64, which accumulates into P* -- dead behind the sum when the block came out of LDS, live here: it put a
// v_mov_b64 in front of each of the eight.  The same fused operation on the same operands.
PK_DEV double fma3(double a, double b, double c) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
PK_DEV double lp_sum_held(const LpField& f, double tau, double eta, double xsi) {
    const double p0 = fma3(tau, f.d0.x, f.p0.x), px = fma3(tau, f.d0.y, f.p0.y), py = fma3(tau, f.d1.x, f.p1.x), pxy = fma3(tau, f.d1.y, f.p1.y);
    return fma(eta, fma(xsi, pxy, py), fma(xsi, px, p0));
}

PK_DEV int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- cell record in registers (FAST_LP_CACHE only) ---------------------------------------------------------------------------------
// A lane's cell changes in under 1 % of its evaluations (tests/test_gpu_level_pair_cache.py: the premise), yet every evaluation read the
// two table entries per axis of that cell from LDS, compared, handled the edge cells and ravelled the index again -- one dependent LDS round
// trip and ~27 VALU instructions in front of the block read.  The cache kernel keeps the entries in registers (FCtx::ya ..):
//   * a lane with ya < y <= yb and xa < x <= xb is in the cell of its previous evaluation: indices, `ei` and the block test stay as they
//     are and eta, xsi are the same (x - a) * RN(1 / width) on the same operands.  The strict test accepts a subset of what the table test
//     accepts for that cell and the search is a pure function of the coordinate, so every other lane -- first evaluation, new cell,
//     exactly on a node, outside an edge cell, NaN -- runs fast_search2 as before and renews the record from the entries it fetched;
//   * a search that answered an out-of-bounds code (or a depth outside the grid) leaves no record: such a lane takes the table path and
//     its status rules in every evaluation;
//   * depth is searched when the particle's z is new, not in every evaluation: the 2-D stages never move z, so FCtx::mz and its compare leave
//     the stage loop and the search is keyed on FAST_Z_UNSEARCHED.  z does move where the step loop adds a dz the particle brought into the
//     launch (ParticleSet(..., dz=...), a dz an earlier kernel left): the position update re-arms the search there (fctx_depth_moved), one
//     compare per step.  It drops the record as well -- a same-cell lane tests no index, and the new depth may lie outside the grid.
// FAST_LP_REGS, FAST_LP_OFF and modules with user kernels search the table in every evaluation.  (Measured step by step -- the record alone,
// then without ravel and tests on a same-cell lane, then with an early block read: profiles/c2_cell_registers_ab.txt.)

// ---- block and time cell in registers (FAST_LP_CACHE, float64 particle storage: fast_held) ------------------------------------------------------
// With the cell record every evaluation still read the lane's 128-byte block from LDS -- the sixteen doubles the same lane had held in the
// same registers one evaluation earlier: 0.79 of the wave-evaluations have no missing lane -- and every second one (stages 2 and 4 bring a
// new t) searched the time table for the cell the wavefront has sat in since the launch began.
// The block: Z0 / D of U and V (FCtx::fu, fv) are lane state that survives from one evaluation to the next and from one step to the
// next; the LDS slot is their backing store.
//   * Invariant: whenever ei == bei and the level pair is that of bkey, the registers hold what the slot holds.  A wave-evaluation without a
//     missing lane touches LDS for nothing but a time-cell miss.
//   * A wave-evaluation with a missing lane does what it did: the missing lanes fetch and write their slot behind the waterfall, then ALL
//     lanes load the block from their slot -- so the hit lanes' registers are dead across the miss branch, whose corner rows need them.
//   * The early returns (time error, out-of-bounds code) leave registers and slot as they are.
//   * The final sums use the three-address v_fma_f64 (lp_sum_held): the compiler's v_fmac_f64 accumulates into P*, which now stays live, and
//     cost a v_mov_b64 in front of each of the eight -- with them this kernel was 2 % SLOWER than the early block read it replaced.
//   * The 32 registers come out of the depth memo: of hz, zi, zez and mzeta one register stays, FCtx::zi = zi * 2 + lenZ.  The hit path needs
//     neither index nor weight (a new depth drops the block: lenZ is no part of the hit test, FCtx::bkey holds the level pair only); the table
//     path forms zi * ez for its ravel; the miss branch and the out-of-bounds rules read the depth cell's entry again and form zeta from the
//     operands the search had (depth_zeta).  Without this the headline kernel spilled 4 VGPRs once per step (16 B of scratch).
//   * Not in the instantiations for float32 particle storage, which start 6 VGPRs higher: they read the block from their slot in every
//     evaluation and keep the time and depth memo.
// The time record: the entries of the lane's time cell -- first node, second node, 1 / width (FCtx::ta, tb, tr), index FCtx::ht -- instead of the
// memo (mt, mtau).  A lane with ta < t <= tb takes ti from the record and tau = (t - ta) * tr, the operands and the operation of fast_bary
// inside fast_search: the same bits.  Every other lane -- first evaluation, new level pair, t exactly on a node, t == 0, NaN, a one-level
// axis -- runs fast_search unchanged and renews the record from the entry the search holds; the range test stays in front.  One record per
// lane: one per wavefront in scalar registers (renewed under a ballot from the first lane outside it) was built, measured and not kept.
// Measured: profiles/c2_block_registers_ab.txt.
constexpr bool fast_held(int lp, bool pf) { return lp == FAST_LP_CACHE && !pf; }  // this kernel holds its block and time cell in registers

// ---- the hit path's non-arithmetic VALU (fast_held kernels only) -----------------------------------------------------------------------------
// Counted on the path a wave-evaluation of the looped stages 2-4 takes when every lane stays in its cell and its time cell (0.79 of them):
// 96 VALU, of which the reference's arithmetic needs about 68 (profiles/c2_hit_path_trim_ab.txt).  FAST_LP_REGS -- the bit-for-bit partner
// of the tests --, FAST_LP_OFF, the instantiations for float32 particle storage and modules with user kernels are not touched by the two
// steps that were kept.
// Stage weights: the stage weights of su = u1 + 2*u2 + 2*u3 + u4 as ONE fused operation, su = fma(wgt, u, su) with wgt = 2.0 or 1.0 in a
// scalar register pair (fma3s: the three-address v_fma_f64; the translation unit is built with -ffp-contract=off, so the compiler forms
// none itself).  The stage loop is not unrolled: for `su + 2*u` / `su + u` it formed u + u, chose between u and 2u with two v_cndmask_b32
// and added -- 8 VALU for U and V where 2 suffice.  The same bits: 2*u is exact for every finite |u| < 2^1023, subnormals included, so
// both forms round the same exact sum once (tests/test_wsum_fma.py).  The ONE exception: |u| >= 2^1023, where 2*u overflows to infinity
// before the addition and the fused form may stay finite (a velocity of 1e308 m/s).
// Unit factors: deg2m and 1 / deg2m of the unit conversion become opaque scalars at the top of every STEP (FastTabs::deg2m, inv_deg2m;
// pk_kernels.h).  As kernel arguments they lived across the whole kernel, were spilled to VGPR lanes and came back through six v_readlane_b32
// in front of every conversion; a pair that lives for one step the allocator keeps in scalar registers: 6 VALU less per evaluation, 58 -> 48
// v_readlane_b32 inside the stage loop, one scalar load per step.
// Built and not kept: u = v = 0 filled only on the paths that return early (time error, out-of-bounds code) -- the allocator answered with
// 48 B of scratch per lane in both float64-storage instantiations, alone and beside the other steps; the stage position reading the
// registers the evaluation leaves u and v in (no lu, lv) -- the two copies stayed, for as long as the zero fill stands in front of them.
PK_DEV double fma3s(double wgt, double b, double c) {  // fma(wgt, b, c), wgt wave-uniform: read from its scalar register pair
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "s"(wgt), "v"(b), "v"(c));
    return r;
}

// ---- the miss branch, transposed (fast_held kernels only) ----------------------------------------------------------------------------------------
// 0.21 of the headline launch's wave-evaluations hold a missing lane, ~1.3 of them each, and the waterfall above runs lp_fetch for them at wave
// width: 16 wide loads in two dependent batches, ~56 fp64 operations and 64-bit scalar row bases for one or two working lanes.  The 16 corner
// rows of ONE missing lane are 16 independent loads, and lp_field applies the same three operations to pairs of them: work for 16 lanes.
// The transposed fetch: when the wavefront is complete (all 64 lanes active), no ring is in use and at most `miss_lanes` lanes miss
// (pk_set_option; FastTabs::fl carries it), each row of 16 lanes serves one missing lane m per pass -- row g the g-th set bit of the miss mask:
//   * m's b00, zeta and key (ti, lenT, lenZ) reach the row through ds_bpermute_b32 (the crossbar: no LDS memory);
//   * helper j = k | r << 1 | l << 2 | f << 3 (depth row, lat row, time level, U / V) forms its own 64-bit address and issues ONE ldpair, masked
//     out where the reference does not read the row (level ti + 1 without lenT, depth row zi + 1 without lenZ): one vmem instruction and one
//     round trip for both fields and both levels of up to four lanes, on whichever level pairs they sit -- no waterfall;
//   * three exchange steps (DPP), each run once by the whole wavefront, are lp_field's operations on lp_field's operands: the z lerp with
//     lane j^1, the level difference with lane j^4, the polynomial basis with lane j^2 (tests/test_lp_transposed_model.py pins map and order);
//   * the k = 0 lane (f, l, r) holds entry 4f + 2l + r of m's slot and writes it: one ds_write_b128 per pass.
// Every other wave-evaluation with a missing lane -- a chunk's first one (64 missing lanes), a wavefront with deleted or finished lanes, a ring
// launch -- takes the waterfall: the same bits, so the threshold is a speed knob only.
// Built and not kept: the hit lanes' block (FCtx::fu, fv) live across the transposed fetch, only the lanes that were served reading
// their slot back.  The 32 registers do not fit beside the lane state and the helpers' values: 128 VGPRs and 160 B (float fields: 128 B) of scratch
// per lane in the two instantiations, where the rule is none (profiles/c2_miss_transposed_ab.txt).
constexpr int FAST_MISS_LANES_DEFAULT = 4;      // pk_set_option "miss_lanes" -1: one pass (profiles/c2_miss_transposed_ab.txt)
constexpr uint32_t FA_MISS_LANES_SHIFT = 16u;   // FastTabs::fl bits 16-22: the threshold, 0..64
// DPP controls: quad_perm [1,0,3,2] (lane j^1), quad_perm [2,3,0,1] (lane j^2), row_shr:4 (lane j - 4: j^4 for the lanes with bit 2 set)
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_SHR4 = 0x114;
template <int CTRL, int BANKS>
PK_DEV double dpp_f64(double v) {  // lanes of the banks not in BANKS keep v (all banks: every lane has a source, no old value to carry)
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const int lo = (int)(uint32_t)b, hi = (int)(uint32_t)(b >> 32);
    uint32_t rlo, rhi;
    if constexpr (BANKS == 0xf) {
        rlo = (uint32_t)__builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
        rhi = (uint32_t)__builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    } else {
        rlo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, BANKS, false);
        rhi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, BANKS, false);
    }
    return __builtin_bit_cast(double, (uint64_t)rlo | ((uint64_t)rhi << 32));
}
// ldpair (pk_device.h) at an address formed as an integer: the pointer says "global memory" (flat loads otherwise)
PK_DEV void ldpair_at(uint64_t addr, double& a, double& b, double) {
    const pk_double2 v = *reinterpret_cast<const __attribute__((address_space(1))) pk_double2*>((uintptr_t)addr);
    a = v.x;
    b = v.y;
}
PK_DEV void ldpair_at(uint64_t addr, double& a, double& b, float) {
    const pk_float2 v = *reinterpret_cast<const __attribute__((address_space(1))) pk_float2*>((uintptr_t)addr);
    a = (double)v.x;
    b = (double)v.y;
}
PK_DEV uint32_t lane_u32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }
// mm: the miss mask (wave-uniform, not 0); wkey, b00, zeta: each lane's own.  Requires all 64 lanes active and resident levels (no ring).
// Written to hold FEW SCALAR REGISTERS: the stage loop around it already spills 121 SGPRs to VGPR lanes, and a first form of this block -- the lane's
// bits k, r, l, f and its row as lane masks across the pass loop, the field bases and strides as scalars -- pushed 19 more out and put 205 more
// v_readlane_b32 into the kernel, the hit path included: 7 % SLOWER than the parent with this block never taken.  So the lane's constants are VGPR
// integers (opaque: not turned back into masks or scalars), the four lane numbers of a pass travel in ONE scalar, a byte each, and every mask is
// formed where it is used.
template <class FT>
PK_DEV void lp_fetch_xposed(const FastA& F, const FastTabs& T, uint64_t mm, int wkey, uint32_t b00, double zeta) {
    uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint64_t zb = __builtin_bit_cast(uint64_t, zeta);
    // lane constants: the field's base, the byte offset of the lane's (depth, lat) row, the level stride (fill_fast: < 2^32)
    const uint32_t kb = 0u - (lane & 1u), rb = 0u - ((lane >> 1) & 1u), fb = 0u - ((lane >> 3) & 1u);  // all ones where the bit is set
    const uint64_t du = (uint64_t)(uintptr_t)F.U, dv = (uint64_t)(uintptr_t)F.V - du;
    uint64_t fbase = du + ((uint64_t)((uint32_t)dv & fb) | ((uint64_t)((uint32_t)(dv >> 32) & fb) << 32));
    uint64_t rowoff = (uint64_t)(F.dzb & kb) + (uint64_t)(F.dyb & rb);
    uint32_t lvl_b = (uint32_t)F.lvl_b;
    asm volatile("" : "+v"(fbase), "+v"(rowoff), "+v"(lvl_b), "+v"(lane));
    do {
        uint32_t four = 0u;  // the next four set bits of the mask, a byte each, 0xff = none (scalar)
        for (int q = 0; q < 4; q++) {
            four |= (mm ? (uint32_t)__builtin_ctzll(mm) : 0xffu) << (8 * q);
            mm &= mm - 1;
        }
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));  // (per pass: what is derived from it below is not hoisted into masks that live across the loop)
        const uint32_t m = (four >> ((ln >> 4) * 8u)) & 0xffu;  // row g serves the g-th of them
        const int src = (int)(m & 63u);
        const uint32_t mb00 = lane_u32(b00, src), mkey = lane_u32((uint32_t)wkey, src);
        const double mzeta = __builtin_bit_cast(double, (uint64_t)lane_u32((uint32_t)zb, src) | ((uint64_t)lane_u32((uint32_t)(zb >> 32), src) << 32));
        const uint32_t lbit = (ln >> 2) & 1u;
        const uint64_t addr = fbase + ((uint64_t)((mkey >> 2) + lbit) * (uint64_t)lvl_b + rowoff + (uint64_t)mb00);
        // masked out of the load: a row without a lane to serve, the lower depth row without lenZ, level ti + 1 without lenT
        const uint32_t skip = (m >> 7) | (ln & 1u & ~mkey) | (lbit & ~(mkey >> 1));
        double cx = 0.0, cy = 0.0;
        if (skip == 0u) ldpair_at(addr, cx, cy, FT());
        // 1: the z lerp (k = 0 lanes with the row of lane j^1; what the k = 1 lanes form is read by nobody)
        const double dx = dpp_f64<DPP_XOR1, 0xf>(cx), dy = dpp_f64<DPP_XOR1, 0xf>(cy);
        const double zx = fma(mzeta, dx - cx, cx), zy = fma(mzeta, dy - cy, cy);
        const bool lenZ = (mkey & 1u) != 0;
        cx = lenZ ? zx : cx;
        cy = lenZ ? zy : cy;
        // 2: level ti + 1 minus level ti (l = 1 lanes: banks 1 and 3 of the row take lane j - 4), or zero where it was not read
        const double ax = dpp_f64<DPP_SHR4, 0xa>(cx), ay = dpp_f64<DPP_SHR4, 0xa>(cy);
        const bool lenT = (mkey & 2u) != 0;
        const double ex = lenT ? cx - ax : 0.0, ey = lenT ? cy - ay : 0.0;
        const bool l = lbit != 0;
        cx = l ? ex : cx;
        cy = l ? ey : cy;
        // 3: the polynomial basis {P0, Px} (r = 0), {Py, Pxy} (r = 1)
        const double h = cy - cx;
        const double ox = dpp_f64<DPP_XOR2, 0xf>(cx), oh = dpp_f64<DPP_XOR2, 0xf>(h);
        const bool r = (ln & 2u) != 0;
        pk_tab2 e;
        e.x = r ? cx - ox : cx;
        e.y = r ? h - oh : h;
        // the k = 0 lane (f, l, r) holds entry 4f + 2l + r of lane m's slot
        if (((m >> 7) | (ln & 1u)) == 0u) (T.blk + ((int)m - (int)ln))[((ln >> 1) & 7u) * FAST_WG_LP] = e;
    } while (mm);
}

// The status rules of the evaluators for an evaluation some index of which carries an out-of-bounds code (-1 right, -2 left; field.py:307-356)
PK_DEV int fast_oob_state(int s, int xi, int yi, int zi, double xsi, double eta, double zeta, double tau) {
    if ((xi == RIGHT_OUT_OF_BOUNDS || yi == RIGHT_OUT_OF_BOUNDS || zi == RIGHT_OUT_OF_BOUNDS) && s < PK_ERROROUTOFBOUNDS) s = PK_ERROROUTOFBOUNDS;
    if (zi == LEFT_OUT_OF_BOUNDS && s < PK_ERRORTHROUGHSURFACE) s = PK_ERRORTHROUGHSURFACE;
    // field.py:359-378: a non-finite barycentric coordinate makes the (wrapped-around) gather NaN, then everything is zeroed
    const bool bad = !(isfinite(xsi) && isfinite(eta) && isfinite(zeta) && isfinite(tau));
    if (bad && s < PK_ERRORINTERPOLATION) s = PK_ERRORINTERPOLATION;
    return s;
}

// Per-particle evaluation context of the fast kernels.  Besides the status code and the `ei` entry of the velocity grid it holds
// the cells of the previous evaluation (always valid cell indices: the search hints) and a memo of the last time and depth
// searched: the search is a pure function of the coordinate, and the Runge-Kutta stages revisit t (stages 2 and 3 share
// t + dt/2; stage 4 of one step and stage 1 of the next share t + dt) and, in the 2-D kernels, never move z.
struct FCtx {
    // both evaluators (and eval_scalar_fast): status, ravelled index, search hints, the time / depth memo and the cell of the lane's block
    int state;
    int32_t ei;
    int ht, hz, hy, hx;
    int zi;                      // memo: index (or out-of-bounds code) of the last depth searched
    uint32_t zez;                // ... and its term zi * ez of the ravelled index (wrapped 32-bit product)
    double mt, mtau, mz, mzeta;  // memo keys (bitwise-equal coordinate => same answer) and barycentric values
    // Corner-block cache of eval_uvw_fast (2-D kernels): the t / z-lerped corner values c00..c11 of U and V -- 8 doubles in the lane's LDS slot
    // FastTabs::blk -- are a function of the cell and of (t, z) only.  Stages 2 and 3 of a Runge-Kutta step share t, stage 4 and stage 1 of the
    // next step too, their sample points lie a fraction of a cell apart and z does not move: when EVERY lane of the wavefront samples the
    // cell (`bei`, its ravelled index) at the (mt, mz) its cached block was formed at, the 16 corner loads and the level lerps are skipped
    // and the bilinear sum runs on the same values -- the same operations, so the same bits (measured: 0.998 / 1.000 of the wave-evaluations
    // of those two stage pairs on BASELINE config 2).  Invariant: bei >= 0 => the slot holds the block of cell bei at (mt, mz).
    // Level-pair cache of eval_uvw_lp (FAST_LP_CACHE): the slot holds Z0 / D of cell `bei` at depth mz for the key `bkey`.
    int32_t bei;
    // eval_uvw_lp only: the key of the block (ti << 2 | lenT << 1 | lenZ; a new depth drops the block, a new time alone does not), the cell
    // record, and for fast_held the block and the time record
    int32_t bkey;
    // Cell record (FAST_LP_CACHE): the table entries of the lane's cell (hy, hx) -- first node, second node, 1 / width of lat and
    // of lon -- held in registers for as long as the lane stays inside it.  ya = +inf: no record (the test of eval_uvw_lp fails).
    double ya, yb, yr, xa, xb, xr;
    // fast_held: the block itself -- what the slot holds whenever ei == bei and bkey names the level pair.  FCtx::zi is zi * 2 + lenZ then.
    LpField fu, fv;
    // fast_held: the entries of the lane's time cell `ht` -- first node, second node, 1 / width.  ta = +inf: no record.
    double ta, tb, tr;
};
constexpr int32_t FAST_NO_BLOCK = -0x7fffffff - 1;
constexpr int FAST_Z_UNSEARCHED = -3;  // FCtx::zi before the launch's one depth search (FAST_LP_CACHE; no index, no out-of-bounds code)
constexpr int FAST_Z_UNSEARCHED_PACKED = -0x7fffffff - 1;  // the same for the packed depth cell of fast_held (zi * 2 + lenZ)
// FAST_LP_CACHE: the step loop moved z by a non-zero dz -- search depth again in the next evaluation (which drops the block of the old
// depth and forms `zez`, `ei` anew), on the table path
PK_DEV void fctx_depth_moved(FCtx& c, bool held) {
    c.zi = held ? FAST_Z_UNSEARCHED_PACKED : FAST_Z_UNSEARCHED;
    c.ya = __builtin_inf();
}
PK_DEV void fctx_init(FCtx& c, int state, int32_t ei, bool cache, bool held) {  // cache: LP == FAST_LP_CACHE; held: fast_held(LP, PF)
    c.state = state;
    c.ei = ei;
    c.ht = c.hz = c.hy = c.hx = 0;
    c.zi = held ? FAST_Z_UNSEARCHED_PACKED : cache ? FAST_Z_UNSEARCHED : 0;
    c.ya = c.xa = c.ta = __builtin_inf();
    c.yb = c.xb = c.yr = c.xr = c.tb = c.tr = 0.0;
    c.zez = 0u;
    c.mt = c.mz = __builtin_nan("");  // equal to nothing
    c.mtau = c.mzeta = 0.0;
    c.bei = FAST_NO_BLOCK;
    c.bkey = -1;
    c.fu.p0 = c.fu.p1 = c.fu.d0 = c.fu.d1 = c.fv.p0 = c.fv.p1 = c.fv.d0 = c.fv.d1 = pk_tab2{0.0, 0.0};
}

// ---- what the two evaluators share ------------------------------------------------------------------------------------------------------
// (The two helpers that end an evaluation answer through ONE flag at ONE return: written with an early `return false` they compiled every
// kernel that calls them to other code, the cache kernels to 230 instructions more -- tools/kernel_code_diff.py against the inlined form.)
// _search_time_index (index_search.py:65-91), the range test.  -> true: t lies outside the field's time interval (the status is set).
// (it, klo): the key of this sample (pk_device.h: twe_note -- a launch with LISTED samples runs the general program, pk_api.hip)
PK_DEV bool fast_time_outside(const KArgs& a, const FastTabs& T, FCtx& c, double t, unsigned it, int klo) {
    const bool out = !(0 <= t) || !(t <= T.tlen);
    if (__builtin_expect(out, 0)) {
        c.state = PK_ERROROUTSIDETIMEINTERVAL;
        twe_note(a, it, klo);
    }
    return out;
}
// ... and the time memo: FCtx::ht, mtau answer for t.  drop: a new t drops the lane's block (the stage-pair block is one of (t, z))
PK_DEV void fast_time_memo(const FastTabs& T, const FastA& F, FCtx& c, uint32_t fl, double t, bool drop) {
    if (t != c.mt) {
        int idx;
        fast_search<true>(T.time, F.nt, F.t0, F.t1, t, c.ht, idx, c.mtau, (fl & FA_NT2) != 0);  // level times start at 0 (host check): idx == c.ht
        c.mt = t;
        if (drop) c.bei = FAST_NO_BLOCK;
    }
}
// The depth memo's search: FCtx::zi, zez, mzeta answer for z; a block formed at another depth is dropped.  The caller knows when z is new:
// by the key FCtx::mz (keyed), or because the step loop said so (FAST_Z_UNSEARCHED)
PK_DEV void fast_depth_search(const FastTabs& T, const FastA& F, FCtx& c, uint32_t fl, double z, bool keyed) {
    fast_search<true>(T.depth, F.gnz, F.z0, F.z1, z, c.hz, c.zi, c.mzeta, (fl & FA_NZ2) != 0);
    c.zez = (uint32_t)c.zi * F.ez;
    if (keyed) c.mz = z;
    c.bei = FAST_NO_BLOCK;
}
// lat and lon in their tables, the ravelled index FCtx::ei and the status rules.  -> true: some index carries an out-of-bounds code
constexpr uint32_t FA_YX2 = FA_Y | FA_X | FA_NY2 | FA_NX2;
PK_DEV bool fast_search_yx(const FastTabs& T, const FastA& F, FCtx& c, uint32_t fl, double y, double x, int zi, double zeta, double tau, int& yi,
                           int& xi, double& eta, double& xsi) {
    if ((fl & FA_YX2) == FA_YX2) {
        fast_search2(T.lat, T.gny, F.y0, F.y1, y, c.hy, yi, eta, T.lon, T.gnx, F.x0, F.x1, x, c.hx, xi, xsi);
    } else {
        if (fl & FA_Y) fast_search<true>(T.lat, T.gny, F.y0, F.y1, y, c.hy, yi, eta, (fl & FA_NY2) != 0);
        if (fl & FA_X) fast_search<true>(T.lon, T.gnx, F.x0, F.x1, x, c.hx, xi, xsi, (fl & FA_NX2) != 0);
    }
    // ravel_index (basegrid.py:83-152): the low 32 bits of the int64 sum are the wrapped 32-bit sum.  Of its three 32-bit products (v_mul_lo_u32
    // each) one is left, and that one at full rate: ex == 1 (the fast path needs an x axis: pk_api.hip fill_fast, ravel_strides), zi * ez changes
    // only with the depth memo (FCtx::zez), and for an in-bounds yi both yi and ey are below the 3840 nodes a 60 KB coordinate table holds, far
    // inside the 24 bits of v_mad_u32_u24.  An out-of-bounds code (negative) takes the wrapped 32-bit product.
    c.ei = (int32_t)((uint32_t)xi + __umul24((uint32_t)yi, F.ey) + c.zez);
    const bool out = (xi | yi | zi) < 0;
    if (__builtin_expect(out, 0)) {
        c.ei = (int32_t)((uint32_t)xi + (uint32_t)yi * F.ey + c.zez);
        c.state = fast_oob_state(c.state, xi, yi, zi, xsi, eta, zeta, tau);
    }
    return out;
}
// The unit conversion of a spherical mesh (_xinterpolators.py:183-187).  STEP: deg2m and 1 / deg2m are the step's scalars (FastTabs::deg2m)
template <bool PF, bool STEP>
PK_DEV void fast_convert(const FastTabs& T, const FastA& F, double y, bool pos_f32, double& uu, double& vv) {
    double conv;
    if (PF && pos_f32) conv = (double)((float)F.deg2m * cosf((float)y * DEG2RADF));
    else if constexpr (STEP) conv = T.deg2m * cos_lat_lean(y);
    else if constexpr (PK_FAST_LEAN != 0) conv = F.deg2m * cos_lat_lean(y);
    else conv = F.deg2m * cos_lat(y * DEG2RAD);
    if constexpr (PK_FAST_LEAN != 0) {  // u / conv, v / deg2m within 1.5 ulp: 7 operations instead of 22
        uu = uu * rcp_lean(conv);
        vv = vv * (STEP ? T.inv_deg2m : F.inv_deg2m);
    } else {
        uu /= conv;
        vv = div_by_recip(vv, F.deg2m, F.inv_deg2m);
    }
}
// field.py:373-378 (one unordered compare answers "uu or vv is NaN"; ww: 0 in a 2-D kernel)
PK_DEV void fast_nan_state(FCtx& c, double uu, double vv, double ww) {
    if (__builtin_expect(__builtin_isunordered(uu, vv) || ww != ww, 0)) {
        if (c.state < PK_ERRORINTERPOLATION) c.state = PK_ERRORINTERPOLATION;
    }
}

// VectorField.eval (field.py:250-304) + XLinear_Velocity.interp (_xinterpolators.py:169-190), the stage-pair evaluator: lerps in the
// reference's order, with the stage-pair block of FCtx::bei or nothing (FAST_LP_OFF; every user-kernel module).  PF: the sample point may
// come straight from float32 particle storage (pos_f32); D3: sample W as well.  bmode (wave-uniform; FCtx::bei): bit 0 = this sample may
// share (t, z) with the previous one -- test the cached corner block; bit 1 = the next one may share them with this one -- keep the block.
template <class FT, bool PF, bool D3>
PK_DEV void eval_uvw_fast(const KArgs& a, const FastTabs& T, FCtx& c, double t, double z, double y, double x, bool pos_f32, double& u,
                          double& v, double& w, unsigned it, int klo, int bmode = 0) {
    const FastA& F = a.fast;
    uint32_t fl = T.fl;
    asm volatile("" : "+s"(fl));  // opaque: every FA_* test below is a scalar bit test HERE, not a loop-invariant lane mask (FastTabs::fl)
    u = v = w = 0.0;
    int ti = 0;
    double tau = 0.0;
    if (fl & FA_TI) {
        if (fast_time_outside(a, T, c, t, it, klo)) return;
        fast_time_memo(T, F, c, fl, t, true);
        ti = c.ht;
        tau = c.mtau;
    }
    int zi = 0, yi = 0, xi = 0;
    double zeta = 0.0, eta = 0.0, xsi = 0.0;
    if (fl & FA_Z) {
        if (!(z == c.mz)) {
            fast_depth_search(T, F, c, fl, z, true);
        }
        zi = c.zi;
        zeta = c.mzeta;
    }
    if (fast_search_yx(T, F, c, fl, y, x, zi, zeta, tau, yi, xi, eta, xsi)) return;
    const bool lenT = tau > 0, lenZ = !(zeta <= 0);
    const int key = (ti << 2) | (lenT ? 2 : 0) | (lenZ ? 1 : 0);
    const uint32_t b00 = ((uint32_t)zi * F.st_z + (uint32_t)yi * F.st_y + (uint32_t)xi) * (uint32_t)sizeof(FT);
    const double omt = 1 - tau, omz = 1 - zeta, omx = 1 - xsi, ome = 1 - eta;
    const double w00 = omx * ome, w01 = xsi * ome, w10 = omx * eta, w11 = xsi * eta;
    double uu = 0.0, vv = 0.0, ww = 0.0;
    const bool bc = !D3 && (fl & FA_BLK) != 0;
    // (in-bounds indices ravel to a non-negative `ei` that names the cell; the memo updates above already dropped a block of another (t, z))
    bool reuse = false;
    if (bc && (bmode & 1)) reuse = __builtin_amdgcn_ballot_w64(c.ei != c.bei) == 0;  // every active lane: same cell, same (t, z)
    if (reuse) {
        const pk_tab2 b0 = T.blk[0], b1 = T.blk[FAST_WG], b2 = T.blk[2 * FAST_WG], b3 = T.blk[3 * FAST_WG];
        uu = w00 * b0.x + w01 * b0.y + w10 * b1.x + w11 * b1.y;
        vv = w00 * b2.x + w01 * b2.y + w10 * b3.x + w11 * b3.y;
    } else {
        const bool keep = bc && (bmode & 2);
        pk_tab2* const blk = keep ? T.blk : nullptr;
        for (bool done = false; !done;) {
            // everything derived from the wave-uniform key is formed BEFORE the lane test: inside `if (key == uk)` the optimiser
            // may substitute the (divergent) key for uk, which would move the level arithmetic back into vector registers
            const int uk = uniform_i32(key);
            const int uti = uk >> 2;
            int s0 = uti, s1 = uti + 1;  // has_ti: 0 <= ti <= nt-2; otherwise ti == 0 and the second level is never read
            if (fl & FA_RING) {          // ring of time levels: level L lives in slot L % nslots
                s0 = (int)((uint32_t)s0 % (uint32_t)F.nslots);
                s1 = (int)((uint32_t)s1 % (uint32_t)F.nslots);
            }
            int64_t o0 = (int64_t)s0 * F.lvl_b, o1 = (int64_t)s1 * F.lvl_b;
            int lens = uk & 3;
            asm volatile("" : "+s"(o0), "+s"(o1), "+s"(lens));  // opaque scalars: no path back to the divergent key
            if (key == uk) {
                if (lens == 3) uvw_fast<FT, D3, true, true>(F, o0, o1, b00, tau, omt, zeta, omz, w00, w01, w10, w11, uu, vv, ww, blk);
                else if (lens == 2) uvw_fast<FT, D3, true, false>(F, o0, o1, b00, tau, omt, zeta, omz, w00, w01, w10, w11, uu, vv, ww, blk);
                else if (lens == 1) uvw_fast<FT, D3, false, true>(F, o0, o1, b00, tau, omt, zeta, omz, w00, w01, w10, w11, uu, vv, ww, blk);
                else uvw_fast<FT, D3, false, false>(F, o0, o1, b00, tau, omt, zeta, omz, w00, w01, w10, w11, uu, vv, ww, blk);
                done = true;
            }
        }
        if (keep) c.bei = c.ei;
    }
    if (fl & FA_SPH) fast_convert<PF, false>(T, F, y, pos_f32, uu, vv);
    fast_nan_state(c, uu, vv, ww);
    u = uu;
    v = vv;
    w = ww;
}

// The same for the 2-D kernel in the level-pair arithmetic (PK_FAST_LEAN builds), the level-pair evaluator.  LP: FAST_LP_REGS -- the block is
// formed in registers in every evaluation -- or FAST_LP_CACHE -- it lives in the lane's LDS slot and, for float64 particle storage (fast_held),
// in the lane's registers.
template <class FT, bool PF, int LP>
PK_DEV void eval_uvw_lp(const KArgs& a, const FastTabs& T, FCtx& c, double t, double z, double y, double x, bool pos_f32, double& u, double& v,
                        unsigned it, int klo) {
    static_assert(LP == FAST_LP_REGS || LP == FAST_LP_CACHE, "a level-pair mode (2-D: z must not move inside a step)");
    const FastA& F = a.fast;
    uint32_t fl = T.fl;
    asm volatile("" : "+s"(fl));  // (opaque: see eval_uvw_fast)
    u = v = 0.0;
    constexpr bool CACHE = LP == FAST_LP_CACHE, HELD = fast_held(LP, PF);
    LpField fu, fv;
    int ti = 0;
    double tau = 0.0;
    if (fl & FA_TI) {
        if (fast_time_outside(a, T, c, t, it, klo)) return;
        if constexpr (HELD) {
            if (__builtin_expect((c.ta < t) & (t <= c.tb), 1)) {
                tau = fast_bary(t, c.ta, c.tb, c.tr);
            } else {
                int idx;
                pk_tab2 e;
                double a1;
                const bool two = (fl & FA_NT2) != 0;
                fast_search<true>(T.time, F.nt, F.t0, F.t1, t, c.ht, idx, tau, two, &e, &a1);
                c.ta = __builtin_inf();
                if (two && idx >= 0) { c.ta = e.x; c.tb = a1; c.tr = e.y; }
            }
        } else {
            fast_time_memo(T, F, c, fl, t, false);  // (the level-pair block does not depend on t: its key holds ti and lenT)
            tau = c.mtau;
        }
        ti = c.ht;
    }
    int zi = 0, yi = 0, xi = 0;
    double zeta = 0.0, eta = 0.0, xsi = 0.0;
    // fast_held: zeta of the packed depth cell FCtx::zi, from the operands the search had (the miss branch and the out-of-bounds rules)
    auto depth_zeta = [&]() -> double {
        if ((fl & (FA_Z | FA_NZ2)) != (FA_Z | FA_NZ2)) return 0.0;
        const int q = c.zi >> 1;  // the cell an out-of-bounds code was found in: the first one (left) or the last one (right), fast_search
        const int h = q >= 0 ? q : (q == LEFT_OUT_OF_BOUNDS ? 0 : F.gnz - 2);
        const pk_tab2 e = T.depth[h];
        return fast_bary(z, e.x, T.depth[h + 1].x, e.y);
    };
    if (fl & FA_Z) {
        if constexpr (HELD) {
            if (c.zi == FAST_Z_UNSEARCHED_PACKED) {
                int hz = 0, idx;
                double bz;
                fast_search<true>(T.depth, F.gnz, F.z0, F.z1, z, hz, idx, bz, (fl & FA_NZ2) != 0);
                c.zi = idx * 2 + (!(bz <= 0) ? 1 : 0);
                c.bei = FAST_NO_BLOCK;
            }
            zi = c.zi >> 1;
        } else {
            if (CACHE ? c.zi == FAST_Z_UNSEARCHED : !(z == c.mz)) {
                fast_depth_search(T, F, c, fl, z, !CACHE);
            }
            zi = c.zi;
            zeta = c.mzeta;
        }
    }
    if constexpr (CACHE) {  // the cell record
        const bool yx2 = (fl & FA_YX2) == FA_YX2;
        // (bitwise: four compares and three s_and, no short-circuit exec-mask blocks; a NaN fails)
        const bool same = yx2 & (c.ya < y) & (y <= c.yb) & (c.xa < x) & (x <= c.xb);
        if (__builtin_expect(same, 1)) {
            eta = fast_bary(y, c.ya, c.yb, c.yr);
            xsi = fast_bary(x, c.xa, c.xb, c.xr);
        } else {
            CellEntries e;
            if (yx2) {
                fast_search2(T.lat, T.gny, F.y0, F.y1, y, c.hy, yi, eta, T.lon, T.gnx, F.x0, F.x1, x, c.hx, xi, xsi, &e);
            } else {
                if (fl & FA_Y) fast_search<true>(T.lat, T.gny, F.y0, F.y1, y, c.hy, yi, eta, (fl & FA_NY2) != 0);
                if (fl & FA_X) fast_search<true>(T.lon, T.gnx, F.x0, F.x1, x, c.hx, xi, xsi, (fl & FA_NX2) != 0);
            }
            // (cold: the wrapped 32-bit product serves indices and codes alike)
            c.ei = (int32_t)((uint32_t)xi + (uint32_t)yi * F.ey + (HELD ? (uint32_t)zi * F.ez : c.zez));
            if (__builtin_expect((xi | yi | zi) < 0, 0)) {
                if (HELD) zeta = depth_zeta();
                c.state = fast_oob_state(c.state, xi, yi, zi, xsi, eta, zeta, tau);
                c.ya = __builtin_inf();
                return;
            }
            if (yx2) {
                c.ya = e.ea.x; c.yb = e.a1a; c.yr = e.ea.y;
                c.xa = e.eb.x; c.xb = e.a1b; c.xr = e.eb.y;
            }
        }
        // (a same-cell lane formed no indices: past the out-of-bounds return they are the hints)
        yi = c.hy;
        xi = c.hx;
    } else {
        if (fast_search_yx(T, F, c, fl, y, x, zi, zeta, tau, yi, xi, eta, xsi)) return;
    }
    const bool lenT = tau > 0, lenZ = HELD ? (c.zi & 1) != 0 : !(zeta <= 0);
    // (fast_held: the hit test leaves lenZ out -- FCtx::bkey holds the level pair only, the waterfall's key has all three)
    const int key = (ti << 2) | (lenT ? 2 : 0) | (!HELD && lenZ ? 1 : 0);
    const uint32_t b00 = ((uint32_t)zi * F.st_z + (uint32_t)yi * F.st_y + (uint32_t)xi) * (uint32_t)sizeof(FT);
    double uu = 0.0, vv = 0.0;
    // FAST_LP_CACHE: only the lanes whose cell, depth or level pair changed since their block was formed fetch (a divergent branch most
    // wave-evaluations of the odd stages skip and ~1.3 lanes take in the even ones); FAST_LP_REGS: every lane, every evaluation
    const bool miss = !CACHE || c.ei != c.bei || key != c.bkey;
    const bool some_miss = !CACHE || __builtin_amdgcn_ballot_w64(miss) != 0;
    if (some_miss) {
        if (HELD) zeta = depth_zeta();  // (its two reads are under way while the corner rows are requested)
        const int wkey = HELD ? key | (lenZ ? 1 : 0) : key;
        [[maybe_unused]] bool xposed = false;  // (wave-uniform) the transposed fetch served this wave-evaluation's missing lanes
        if constexpr (HELD) {  // few missing lanes of a complete wavefront, resident levels: sixteen helpers per missing lane
            const uint64_t mm = __builtin_amdgcn_ballot_w64(miss);
            xposed = __builtin_amdgcn_ballot_w64(true) == ~0ull && !(fl & FA_RING) &&
                     (uint32_t)__builtin_popcountll(mm) <= ((fl >> FA_MISS_LANES_SHIFT) & 127u);
            if (xposed) {
                lp_fetch_xposed<FT>(F, T, mm, wkey, b00, zeta);
                if (miss) {
                    c.bei = c.ei;
                    c.bkey = key;
                }
            }
        }
        // the waterfall over the key, as in eval_uvw_fast (level bases stay in SGPRs); a lane that hit starts as done
        for (bool done = !miss || xposed; !done;) {
            const int uk = uniform_i32(wkey);
            const int uti = uk >> 2;
            int s0 = uti, s1 = uti + 1;
            if (fl & FA_RING) {
                s0 = (int)((uint32_t)s0 % (uint32_t)F.nslots);
                s1 = (int)((uint32_t)s1 % (uint32_t)F.nslots);
            }
            int64_t o0 = (int64_t)s0 * F.lvl_b, o1 = (int64_t)s1 * F.lvl_b;
            int lens = uk & 3;
            asm volatile("" : "+s"(o0), "+s"(o1), "+s"(lens));
            if (wkey == uk) {
                if (lens == 3) lp_fetch<FT, true, true>(F, o0, o1, b00, zeta, fu, fv);
                else if (lens == 2) lp_fetch<FT, true, false>(F, o0, o1, b00, zeta, fu, fv);
                else if (lens == 1) lp_fetch<FT, false, true>(F, o0, o1, b00, zeta, fu, fv);
                else lp_fetch<FT, false, false>(F, o0, o1, b00, zeta, fu, fv);
                done = true;
            }
        }
        // The block goes to LDS BEHIND the waterfall, from the registers FAST_LP_REGS uses.  (Written inside it -- U's entries between the two
        // load batches, 4 VGPRs and 12 B of scratch less -- lanes of a wavefront that spans several level pairs read back other values
        // than they had formed: tests/test_gpu_level_pair_cache.py::test_staggered_release_times_and_ring.)
        if (CACHE && miss && !xposed) {
            T.blk[0] = fu.p0; T.blk[FAST_WG_LP] = fu.p1; T.blk[2 * FAST_WG_LP] = fu.d0; T.blk[3 * FAST_WG_LP] = fu.d1;
            T.blk[4 * FAST_WG_LP] = fv.p0; T.blk[5 * FAST_WG_LP] = fv.p1; T.blk[6 * FAST_WG_LP] = fv.d0; T.blk[7 * FAST_WG_LP] = fv.d1;
            c.bei = c.ei;
            c.bkey = key;
        }
    }
    if constexpr (HELD) {
        if (some_miss) {
            c.fu.p0 = T.blk[0]; c.fu.p1 = T.blk[FAST_WG_LP]; c.fu.d0 = T.blk[2 * FAST_WG_LP]; c.fu.d1 = T.blk[3 * FAST_WG_LP];
            c.fv.p0 = T.blk[4 * FAST_WG_LP]; c.fv.p1 = T.blk[5 * FAST_WG_LP]; c.fv.d0 = T.blk[6 * FAST_WG_LP]; c.fv.d1 = T.blk[7 * FAST_WG_LP];
        }
        uu = lp_sum_held(c.fu, tau, eta, xsi);
        vv = lp_sum_held(c.fv, tau, eta, xsi);
    } else {
        if (CACHE) {
            fu.p0 = T.blk[0]; fu.p1 = T.blk[FAST_WG_LP]; fu.d0 = T.blk[2 * FAST_WG_LP]; fu.d1 = T.blk[3 * FAST_WG_LP];
            fv.p0 = T.blk[4 * FAST_WG_LP]; fv.p1 = T.blk[5 * FAST_WG_LP]; fv.d0 = T.blk[6 * FAST_WG_LP]; fv.d1 = T.blk[7 * FAST_WG_LP];
        }
        uu = lp_sum(fu, tau, eta, xsi);
        vv = lp_sum(fv, tau, eta, xsi);
    }
    if (fl & FA_SPH) fast_convert<PF, HELD>(T, F, y, pos_f32, uu, vv);
    fast_nan_state(c, uu, vv, 0.0);
    u = uu;
    v = vv;
}

#ifdef PK_USER_KERNELS
// Field.eval (field.py:145-185) with XLinear for scalar field `slot` of FastA::S at the same evaluation site: the searches, hints, memo
// and state rules of eval_uvw_fast, one gather, no unit conversion.  Only in run-time compiled modules (a user kernel that samples a
// scalar field rides in the dedicated kernel); the arithmetic is xlinear<FT>'s, which the parity tests compare it with at rtol 0.
template <class FT, bool PF>
PK_DEV double eval_scalar_fast(const KArgs& a, const FastTabs& T, FCtx& c, int slot, double t, double z, double y, double x, unsigned it,
                               int klo) {
    const FastA& F = a.fast;
    int ti = 0;
    double tau = 0.0;
    if (F.has_ti) {
        if (!(0 <= t) || !(t <= F.tlen)) {
            c.state = PK_ERROROUTSIDETIMEINTERVAL;
            twe_note(a, it, klo);
            return 0.0;
        }
        if (t != c.mt) {
            int idx;
            fast_search(T.time, F.nt, F.t0, F.t1, t, c.ht, idx, c.mtau);
            c.mt = t;
            c.bei = FAST_NO_BLOCK;
        }
        ti = c.ht;
        tau = c.mtau;
    }
    int zi = 0, yi = 0, xi = 0;
    double zeta = 0.0, eta = 0.0, xsi = 0.0;
    if (F.has_z) {
        if (!(z == c.mz)) {
            fast_search(T.depth, F.gnz, F.z0, F.z1, z, c.hz, c.zi, c.mzeta);
            c.zez = (uint32_t)c.zi * F.ez;
            c.mz = z;
            c.bei = FAST_NO_BLOCK;
        }
        zi = c.zi;
        zeta = c.mzeta;
    }
    if (F.has_y) fast_search(T.lat, F.gny, F.y0, F.y1, y, c.hy, yi, eta);
    if (F.has_x) fast_search(T.lon, F.gnx, F.x0, F.x1, x, c.hx, xi, xsi);
    c.ei = (int32_t)((uint32_t)xi * F.ex + (uint32_t)yi * F.ey + (uint32_t)zi * F.ez);
    if ((xi | yi | zi) < 0) {
        c.state = fast_oob_state(c.state, xi, yi, zi, xsi, eta, zeta, tau);
        return 0.0;
    }
    const bool lenT = tau > 0, lenZ = !(zeta <= 0);
    const uint32_t b00 = ((uint32_t)zi * F.st_z + (uint32_t)yi * F.st_y + (uint32_t)xi) * (uint32_t)sizeof(FT);
    const double omt = 1 - tau, omz = 1 - zeta, omx = 1 - xsi, ome = 1 - eta;
    const double w00 = omx * ome, w01 = xsi * ome, w10 = omx * eta, w11 = xsi * eta;
    int s0 = ti, s1 = ti + 1;
    if (F.nslots < F.nt) {
        s0 = (int)((uint32_t)s0 % (uint32_t)F.nslots);
        s1 = (int)((uint32_t)s1 % (uint32_t)F.nslots);
    }
    const char* base = F.S[slot];
    const char* l0 = base + (int64_t)s0 * F.lvl_b;
    const char* l1 = base + (int64_t)s1 * F.lvl_b;
    Rows r;
    double val;
    if (lenT && lenZ) { load_rows<FT, true, true>(r, l0, l1, b00, F.dyb, F.dzb); val = interp_rows<true, true>(r, tau, omt, zeta, omz, w00, w01, w10, w11); }
    else if (lenT) { load_rows<FT, true, false>(r, l0, l1, b00, F.dyb, F.dzb); val = interp_rows<true, false>(r, tau, omt, zeta, omz, w00, w01, w10, w11); }
    else if (lenZ) { load_rows<FT, false, true>(r, l0, l1, b00, F.dyb, F.dzb); val = interp_rows<false, true>(r, tau, omt, zeta, omz, w00, w01, w10, w11); }
    else { load_rows<FT, false, false>(r, l0, l1, b00, F.dyb, F.dzb); val = interp_rows<false, false>(r, tau, omt, zeta, omz, w00, w01, w10, w11); }
    if (__builtin_expect(val != val, 0)) {
        if (c.state < PK_ERRORINTERPOLATION) c.state = PK_ERRORINTERPOLATION;
    }
    return val;
}
#endif

}  // namespace pk
