// pk_random.h -- the counter-based random stream of user kernels (`pa.random`, parcels_amd/random.py).
//
// ONE definition for three readers: the modules parcels_amd/jit.py generates (a translated `pa.random.normal(0, s, particles)` is an inline
// call of random_normal below), the fill kernel of pk_random.hip (pk_random_fill: `pa.random.*(pset)` on the resident columns) and the host
// (g++ -O2 -ffp-contract=off with PK_DEV = static inline: tests/test_random_host.py compares it bit for bit with the NumPy restatement in
// parcels_amd/random.py, which is what a Python kernel on the host path computes).
//
// Philox4x32-10, stateless:
//   key      k0 = lo32(seed) ^ (0x9E3779B9 * (slot + 1))    -- the k0 of the built-in stochastic kernels (pk_device.h: normal_pair)
//            k1 = hi32(seed) ^ (0x85EBCA6B * (draw + 1))    -- theirs is plain hi32(seed): a user draw never coincides with a built-in one
//            slot: the kernel's position in the list (-1 outside a kernel), draw >= 0: the ordinal of the draw within the kernel function
//   counter  (lo32(id), hi32(id), lo32(tb), hi32(tb)), id = particle_id as uint64, tb = bits of (double)t + 0.0 (-0.0 and 0.0 are one time)
//   rounds   ten, the key bumped by (0x9E3779B9, 0xBB67AE85) behind each, as normal_pair does them -> w0 .. w3
//   uniforms a = w1 << 32 | w0, b = w3 << 32 | w2;  u1 = ((a >> 11) + 0.5) * 2^-53, u2 likewise from b: strictly inside (0, 1) -- in float64
//            the sum rounds to even; the one value of a >> 11 for which that gives 1.0 (2^53 - 1) takes 1 - 2^-53 instead (random_unit)
// The stream does not depend on launch partitioning, the cell sort or sharding.  A kernel repeated at the same t (RK45 Repeat) draws the same
// numbers again, as the built-in kernels do.  Build with -ffp-contract=off: `low + (high - low) * u1` and `loc + scale * z` are two roundings.
#pragma once
#include <stdint.h>
#ifndef PK_DEV  // the host build
#include <math.h>
#define PK_DEV static inline
#endif

namespace pk {

PK_DEV void random_round(uint32_t c[4], const uint32_t k[2]) {  // (pk_device.h: philox_round, restated so that this header stands alone)
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// ten rounds on (counter, key); the key is bumped behind every round
PK_DEV void random_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
    uint32_t k[2] = {k0, k1};
#pragma unroll
    for (int r = 0; r < 10; r++) {
        random_round(c, k);
        k[0] += 0x9E3779B9u;
        k[1] += 0xBB67AE85u;
    }
}

PK_DEV void random_words(uint64_t seed, int slot, int draw, int64_t particle_id, double t, uint32_t w[4]) {
    const double tz = t + 0.0;
    uint64_t tb;
    __builtin_memcpy(&tb, &tz, 8);
    const uint64_t id = (uint64_t)particle_id;
    w[0] = (uint32_t)id; w[1] = (uint32_t)(id >> 32); w[2] = (uint32_t)tb; w[3] = (uint32_t)(tb >> 32);
    random_philox(w, (uint32_t)seed ^ (0x9E3779B9u * (uint32_t)(slot + 1)), (uint32_t)(seed >> 32) ^ (0x85EBCA6Bu * (uint32_t)(draw + 1)));
}

PK_DEV double random_unit(uint32_t lo, uint32_t hi) {
    const uint64_t a = ((uint64_t)hi << 32) | lo;
    // (53 bits + 0.5 needs 54: the sum is rounded to even, and for a >> 11 = 2^53 - 1 that is 2^53 -- the one input of 2^53 that would give
    // 1.0, whose exact value 1 - 2^-54 lies between 1 - 2^-53 and 1: it takes the lower neighbour, so the result is strictly inside (0, 1))
    const double u = ((double)(a >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return u < 1.0 ? u : 0x1.fffffffffffffp-1;
}

// the variates of four words
PK_DEV double random_normal_of(const uint32_t w[4]) {
    const double u1 = random_unit(w[0], w[1]), u2 = random_unit(w[2], w[3]);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}
PK_DEV double random_exponential_of(const uint32_t w[4], double scale) { return scale * (-log(random_unit(w[0], w[1]))); }
// low + ((w0 * span) >> 32), 1 <= span <= 2^32: exact integer arithmetic; value k is too likely by at most 2^-32 (a bias of span / 2^32 in all)
PK_DEV int64_t random_integers_of(const uint32_t w[4], int64_t low, uint64_t span) {
    return (int64_t)((uint64_t)low + (((uint64_t)w[0] * span) >> 32));
}

// ... and of (seed, slot, draw, id, t): what a translated call becomes
PK_DEV double random_random(uint64_t seed, int slot, int draw, int64_t id, double t) {
    uint32_t w[4];
    random_words(seed, slot, draw, id, t, w);
    return random_unit(w[0], w[1]);
}
PK_DEV double random_uniform(uint64_t seed, int slot, int draw, int64_t id, double t, double low, double high) {
    return low + (high - low) * random_random(seed, slot, draw, id, t);
}
PK_DEV double random_standard_normal(uint64_t seed, int slot, int draw, int64_t id, double t) {
    uint32_t w[4];
    random_words(seed, slot, draw, id, t, w);
    return random_normal_of(w);
}
PK_DEV double random_normal(uint64_t seed, int slot, int draw, int64_t id, double t, double loc, double scale) {
    return loc + scale * random_standard_normal(seed, slot, draw, id, t);
}
PK_DEV double random_exponential(uint64_t seed, int slot, int draw, int64_t id, double t, double scale) {
    uint32_t w[4];
    random_words(seed, slot, draw, id, t, w);
    return random_exponential_of(w, scale);
}
PK_DEV int64_t random_integers(uint64_t seed, int slot, int draw, int64_t id, double t, int64_t low, uint64_t span) {
    uint32_t w[4];
    random_words(seed, slot, draw, id, t, w);
    return random_integers_of(w, low, span);
}

}  // namespace pk
