// pk_unpack.h -- CF unpacking of ONE packed integer value (scale_factor, add_offset, _FillValue / missing_value), the per-value
// function of the decode kernel (pk_unpack.hip) and of the stand-alone host check (tests/test_unpack_host.py).  It restates
// parcels_amd/sources.py: cf_unpack followed by the NaN -> 0 of the level stream:
//     fill values -> NaN;  raw.astype(compute) * scale, then + offset: TWO separately rounded operations in the compute dtype;
//     NaN -> 0 when the model asks for it.
// NumPy never fuses a * b + c, hipcc does by default: the device goes through the round-to-nearest intrinsics, the host through
// contraction switched off for this header, so the result does not depend on the flags of the unit that includes it.
// Plain C++: includes nothing of HIP, so a host compiler takes it as it is.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PK_UNPACK_HD __host__ __device__
#else
#define PK_UNPACK_HD
#endif

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace pk {

// what one component needs, in the types the arithmetic runs in: the attributes cast to the compute dtype (np.asarray(sf, dtype=out_dt)),
// the fill values in the raw dtype (one that the raw dtype cannot hold can never match and is not listed)
template <class Raw, class Cmp>
struct UnpackParams {
    Cmp scale, offset;
    Raw fill[4];
    int32_t nfill, has_scale, has_offset, nan_to_zero;
};

PK_UNPACK_HD inline float unpack_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
#endif
}
PK_UNPACK_HD inline float unpack_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
#endif
}
PK_UNPACK_HD inline double unpack_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
#endif
}
PK_UNPACK_HD inline double unpack_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
#endif
}

PK_UNPACK_HD inline float unpack_nan(float) { return __builtin_nanf(""); }
PK_UNPACK_HD inline double unpack_nan(double) { return __builtin_nan(""); }

template <class Raw, class Cmp>
PK_UNPACK_HD inline Cmp unpack_value(Raw r, const UnpackParams<Raw, Cmp>& p) {
    bool filled = false;
    for (int k = 0; k < 4; k++) filled |= (k < p.nfill) & (r == p.fill[k]);
    Cmp v = (Cmp)r;  // round to nearest even, like ndarray.astype (int32 -> float32 is the one inexact case)
    if (p.has_scale) v = unpack_mul(v, p.scale);
    if (p.has_offset) v = unpack_add(v, p.offset);
    if (filled) v = unpack_nan(Cmp(0));
    if (p.nan_to_zero && v != v) v = Cmp(0);
    return v;
}

}  // namespace pk

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif
