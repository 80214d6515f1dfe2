// pk_select.inc -- the write filter of ParticleFile (particlefile.py:198-221: `|t_p - t| <= |dt|/2`, finite t) on the DEVICE rows, and the
// packing of the rows that pass it in HOST row order (whatever the cell sort did to the device order).  Two callers: the filtered snapshot of
// the asynchronous write-out (pk_particles_snapshot_filtered: only the rows a table holds cross PCIe, and the writer thread has nothing to
// filter) and the multi-GPU exchange (pk_comm.inc).  Included by pk_api.hip.
namespace pk {

// flag[host row] = the device row passes the filter (apply = 0: every row)
__global__ void write_filter_kernel(const double* __restrict__ tp, const double* __restrict__ dt, const int64_t* __restrict__ perm, int64_t n,
                                    double t, int apply, uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 1u;
    if (apply) {
        const double p = tp[i], d = dt[i];
        const double h = fabs(d / 2);
        const bool sel = ((t - h <= p) && (t + h >= p)) || (d != d && p == t);
        f = (sel && isfinite(p)) ? 1u : 0u;
    }
    flag[perm ? perm[i] : i] = f;
}
// dst[offs[host row]] = src[device row] for the flagged rows: the selected rows in host row order, packed
template <class T>
__global__ void select_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, const int64_t* __restrict__ perm, const uint32_t* __restrict__ flag,
                                   const uint32_t* __restrict__ offs, int64_t n, int width) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t h = perm ? perm[i] : i;
    if (!flag[h]) return;
    const int64_t o = (int64_t)offs[h];
    for (int w = 0; w < width; w++) dst[o * width + w] = src[i * width + w];
}

}  // namespace pk

// flags + exclusive scan of the bound device rows at output time t; -> the number of selected rows (one small read-back)
static int32_t select_flags(pk_ctx* ctx, double t, int apply_filter, int64_t* n_sel) {
    using namespace pk;
    PkSelect& S = ctx->sel;
    const int64_t n = ctx->dev.n;
    *n_sel = 0;
    if (n >= (1ll << 31)) return ctx->fail("the device write filter supports < 2^31 particles per device");
    if (n == 0) return 0;
    if (S.cap < n) {
        if (S.d_flag) PK_HIP(ctx, hipFree(S.d_flag));
        if (S.d_offs) PK_HIP(ctx, hipFree(S.d_offs));
        S.d_flag = S.d_offs = nullptr;
        S.cap = 0;
        PK_HIP(ctx, hipMalloc((void**)&S.d_flag, sizeof(uint32_t) * (size_t)n));
        PK_HIP(ctx, hipMalloc((void**)&S.d_offs, sizeof(uint32_t) * (size_t)n));
        S.cap = n;
    }
    const int64_t* perm = ctx->has_perm ? ctx->d_perm : nullptr;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(write_filter_kernel, grid, dim3(256), 0, ctx->compute, (const double*)ctx->dev.t, (const double*)ctx->dev.dt, perm, n, t,
                       apply_filter, S.d_flag);
    PK_HIP(ctx, hipGetLastError());
    size_t tmp = 0;
    PK_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, S.d_flag, S.d_offs, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->compute));
    if (S.tmp_bytes < tmp || !S.d_tmp) {
        if (S.d_tmp) PK_HIP(ctx, hipFree(S.d_tmp));
        S.d_tmp = nullptr;
        PK_HIP(ctx, hipMalloc(&S.d_tmp, std::max<size_t>(tmp, 256)));
        S.tmp_bytes = std::max<size_t>(tmp, 256);
    }
    PK_HIP(ctx, rocprim::exclusive_scan(S.d_tmp, tmp, S.d_flag, S.d_offs, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->compute));
    uint32_t last[2] = {0, 0};
    PK_HIP(ctx, hipMemcpyAsync(&last[0], S.d_offs + (n - 1), 4, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(&last[1], S.d_flag + (n - 1), 4, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    *n_sel = (int64_t)last[0] + (int64_t)last[1];
    return 0;
}
// the selected rows of one column into `dst` (room for them: the caller's business), on the compute stream
static void select_column(pk_ctx* ctx, const ColRef& c, void* dst) {
    using namespace pk;
    const int64_t n = ctx->dev.n;
    const int64_t* perm = ctx->has_perm ? ctx->d_perm : nullptr;
    PK_LAUNCH_ROWS(ctx, select_rows_kernel, c.elem, n, c.d, dst, perm, ctx->sel.d_flag, ctx->sel.d_offs, n, c.width);
}
