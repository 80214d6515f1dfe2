// pk_random.hip -- pk_random_fill: the counter-based stream of pk_random.h, one lane per row.
//
// `pa.random.uniform(0.5, 1.5, pset)` outside a kernel (initial masses, release jitter) on a set whose columns are device-resident: the
// kernel reads particle_id and t where they are -- in whichever row order the cell sort left them -- and writes the values in HOST row order
// through the row permutation; nothing is written to the particle columns.  With ids and t given it draws for device copies of those
// arrays instead, and PK_RANDOM_WORDS writes the four raw words of every row: what tests/test_gpu_random.py compares with the NumPy
// restatement of parcels_amd/random.py.
#include "pk_api_ctx.h"

#include "pk_random.h"

namespace pk {

__global__ void __launch_bounds__(256) random_fill_kernel(int dist, uint64_t seed, int slot, int draw, double p0, double p1, int64_t ilow, uint64_t span,
                                                          const int64_t* __restrict__ ids, const double* __restrict__ t,
                                                          const int64_t* __restrict__ perm, int64_t n, void* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = perm ? perm[i] : i;  // device row -> host row
    uint32_t w[4];
    random_words(seed, slot, draw, ids[i], t[i], w);
    if (dist == PK_RANDOM_WORDS) {
        ((uint4*)out)[j] = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    if (dist == PK_RANDOM_INTEGERS) {
        ((int64_t*)out)[j] = random_integers_of(w, ilow, span);
        return;
    }
    double v;
    switch (dist) {
        case PK_RANDOM_RANDOM: v = random_unit(w[0], w[1]); break;
        case PK_RANDOM_UNIFORM: v = p0 + (p1 - p0) * random_unit(w[0], w[1]); break;
        case PK_RANDOM_STANDARD_NORMAL: v = random_normal_of(w); break;
        case PK_RANDOM_NORMAL: v = p0 + p1 * random_normal_of(w); break;
        default: v = random_exponential_of(w, p0); break;  // PK_RANDOM_EXPONENTIAL
    }
    ((double*)out)[j] = v;
}

namespace {
struct RandomScratch {  // per call: freed on every way out
    void *out = nullptr, *ids = nullptr, *t = nullptr;
    ~RandomScratch() {
        for (void* q : {out, ids, t})
            if (q) (void)hipFree(q);
    }
};
}  // namespace

}  // namespace pk

extern "C" {

int32_t pk_random_fill(pk_ctx* ctx, int32_t dist, uint64_t seed, int32_t slot, int32_t draw, double p0, double p1, int64_t ilow, uint64_t span,
                       const int64_t* ids, const double* t, int64_t n, void* out) {
    if (!ctx) return -2;
    if (dist < PK_RANDOM_WORDS || dist > PK_RANDOM_INTEGERS) return ctx->fail("pk_random_fill: dist must be one of PK_RANDOM_WORDS .. PK_RANDOM_INTEGERS");
    if (draw < 0 || slot < -1) return ctx->fail("pk_random_fill: draw must not be negative and slot not below -1");
    if (dist == PK_RANDOM_INTEGERS && (span < 1 || span > (1ull << 32))) return ctx->fail("pk_random_fill: PK_RANDOM_INTEGERS needs 1 <= span <= 2^32");
    if ((ids == nullptr) != (t == nullptr)) return ctx->fail("pk_random_fill: ids and t go together (both NULL: the bound particles)");
    if (n < 0) return ctx->fail("pk_random_fill: n must not be negative");
    const bool bound = ids == nullptr;
    if (bound) {
        if (!ctx->bound) return ctx->fail("pk_random_fill: no particles bound");
        if (ctx->in_flight) return ctx->fail("pk_random_fill: a launch is in flight (call pk_execute_end)");
        if (n != ctx->dev.n) return ctx->fail("pk_random_fill: n is not the number of bound rows");
    }
    if (n == 0) return 0;
    if (!out) return ctx->fail("pk_random_fill: out is NULL");
    if (n > (int64_t)0x7FFFFFFF * 256) return ctx->fail("pk_random_fill: too many rows for one launch");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    RandomScratch s;
    const size_t bytes = (size_t)n * (dist == PK_RANDOM_WORDS ? 16 : 8);
    PK_HIP(ctx, hipMalloc(&s.out, bytes));
    const int64_t* d_ids = ctx->dev.particle_id;
    const double* d_t = ctx->dev.t;
    const int64_t* d_perm = ctx->has_perm ? ctx->d_perm : nullptr;
    if (!bound) {
        PK_HIP(ctx, hipMalloc(&s.ids, (size_t)n * 8));
        PK_HIP(ctx, hipMalloc(&s.t, (size_t)n * 8));
        PK_HIP(ctx, hipMemcpyAsync(s.ids, ids, (size_t)n * 8, hipMemcpyHostToDevice, ctx->compute));
        PK_HIP(ctx, hipMemcpyAsync(s.t, t, (size_t)n * 8, hipMemcpyHostToDevice, ctx->compute));
        d_ids = (const int64_t*)s.ids;
        d_t = (const double*)s.t;
        d_perm = nullptr;
    }
    hipLaunchKernelGGL(random_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->compute, (int)dist, seed, (int)slot, (int)draw, p0, p1, ilow,
                       span, d_ids, d_t, d_perm, n, s.out);
    PK_HIP(ctx, hipGetLastError());
    PK_HIP(ctx, hipMemcpyAsync(out, s.out, bytes, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

}  // extern "C"
