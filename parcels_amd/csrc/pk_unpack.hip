// pk_unpack.hip -- CF-packed integer field levels (int8 / uint8 / int16 / uint16 / int32 with scale_factor, add_offset, fill values) are
// unpacked on the device: the raw integers cross PCIe, a decode kernel on the copy stream writes the float32 / float64 level straight into
// its ring slot -- a plain array, or the interleaved {U,V[,W]} structs of a packed group in ONE launch.  The per-value arithmetic is
// pk_unpack.h (two separately rounded operations, the bits of sources.cf_unpack); slot bookkeeping and the async semantics are those of
// pk_field_upload_level / _group_level (pk_api.hip).  gfx950 only.
#include "pk_api_ctx.h"
#include "pk_unpack.h"

#include <limits>

using namespace pkapi;
using pkhost::parallel_memcpy;

namespace pk {

template <class Raw, class Cmp, int NC>
struct UnpackArgs {
    const Raw* raw[NC];  // one 16-byte aligned plane per component
    UnpackParams<Raw, Cmp> p[NC];
};

// Streaming decode of `n` values per component.  A lane takes one 16-byte load per plane (V = 16 / sizeof(Raw) values), unpacks them and
// writes the V output elements / V {c0, c1, ..} structs as ONE contiguous run of V * NC * sizeof(Out) bytes -- a multiple of 16, so every
// lane's run has the alignment of `out`: 16-byte stores when `out` is 16-byte aligned, else 8- or 4-byte stores of the same registers
// (a ring slot starts at slot * level_bytes * ncomp: 4- or 8-byte aligned only when the level's value count is odd).  The n % V values
// behind the last complete load are written one by one.  ostride != 1 (NC == 1 only): one component of a packed group, element-wise.
template <class Raw, class Cmp, class Out, int NC>
__global__ void __launch_bounds__(256) unpack_kernel(const UnpackArgs<Raw, Cmp, NC> a, Out* __restrict__ out, int64_t n, int ostride) {
    constexpr int V = 16 / (int)sizeof(Raw);
    constexpr int NO = V * NC;
    constexpr int W = NO * (int)sizeof(Out) / 4;
    static_assert(W % 4 == 0, "a lane's run is a whole number of 16-byte stores");
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    if (NC == 1 && ostride != 1) {
        for (int64_t i = tid; i < n; i += nthreads) out[i * ostride] = (Out)unpack_value(a.raw[0][i], a.p[0]);
        return;
    }
    const int64_t ngroups = n / V;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(out) & 15u);
    for (int64_t g = tid; g < ngroups; g += nthreads) {
        union { Out o[NO]; uint4 q[W / 4]; uint2 d[W / 2]; uint32_t w[W]; } u;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            union { uint4 q; Raw r[V]; } in;
            in.q = *reinterpret_cast<const uint4*>(a.raw[c] + g * V);
#pragma unroll
            for (int j = 0; j < V; j++) u.o[j * NC + c] = (Out)unpack_value(in.r[j], a.p[c]);
        }
        Out* dst = out + g * NO;
        if (mis == 0) {
#pragma unroll
            for (int k = 0; k < W / 4; k++) reinterpret_cast<uint4*>(dst)[k] = u.q[k];
        } else if (mis == 8) {
#pragma unroll
            for (int k = 0; k < W / 2; k++) reinterpret_cast<uint2*>(dst)[k] = u.d[k];
        } else {
#pragma unroll
            for (int k = 0; k < W; k++) reinterpret_cast<uint32_t*>(dst)[k] = u.w[k];
        }
    }
    const int64_t i = ngroups * V + tid;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < NC; c++) out[i * NC + c] = (Out)unpack_value(a.raw[c][i], a.p[c]);
    }
}

// one component of a packed group back as a plain array (pk_field_download_level)
template <class T>
__global__ void __launch_bounds__(256) deinterleave_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t n, int ncomp) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i * ncomp];
}

}  // namespace pk

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
size_t align16(size_t b) { return (b + 15) / 16 * 16; }

int raw_size(int32_t dt) {
    switch (dt) {
        case PK_I8: case PK_U8: return 1;
        case PK_I16: case PK_U16: return 2;
        case PK_I32: return 4;
        default: return 0;
    }
}

struct UnpackJob {
    const void* raw[3];
    const pk_pack_desc* desc;  // nc of them
    int nc;
    void* out;
    int64_t n;
    int ostride;
    unsigned max_blocks;
    hipStream_t stream;
};

template <class Raw, class Cmp>
UnpackParams<Raw, Cmp> make_params(const pk_pack_desc& d) {
    UnpackParams<Raw, Cmp> p{};
    p.scale = d.has_scale ? (Cmp)d.scale : Cmp(1);
    p.offset = d.has_offset ? (Cmp)d.offset : Cmp(0);
    p.has_scale = d.has_scale != 0;
    p.has_offset = d.has_offset != 0;
    p.nan_to_zero = d.nan_to_zero != 0;
    for (int k = 0; k < d.nfill; k++)  // a value the raw dtype cannot hold never matches
        if (d.fill[k] >= (int64_t)std::numeric_limits<Raw>::min() && d.fill[k] <= (int64_t)std::numeric_limits<Raw>::max())
            p.fill[p.nfill++] = (Raw)d.fill[k];
    return p;
}

template <class Raw, class Cmp, class Out, int NC>
void launch_unpack(const UnpackJob& j) {
    UnpackArgs<Raw, Cmp, NC> a;
    for (int c = 0; c < NC; c++) {
        a.raw[c] = (const Raw*)j.raw[c];
        a.p[c] = make_params<Raw, Cmp>(j.desc[c]);
    }
    constexpr int V = 16 / (int)sizeof(Raw);
    const int64_t work = (NC == 1 && j.ostride != 1) ? j.n : j.n / V;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, j.max_blocks));
    hipLaunchKernelGGL((unpack_kernel<Raw, Cmp, Out, NC>), dim3(grid), dim3(256), 0, j.stream, a, (Out*)j.out, j.n, j.ostride);
}

template <class Raw, class Cmp, class Out>
void launch_nc(const UnpackJob& j) {
    if (j.nc == 1) launch_unpack<Raw, Cmp, Out, 1>(j);
    else if (j.nc == 2) launch_unpack<Raw, Cmp, Out, 2>(j);
    else launch_unpack<Raw, Cmp, Out, 3>(j);
}

template <class Raw>
void launch_types(const UnpackJob& j, bool cmp64, bool out64) {
    if (cmp64) launch_nc<Raw, double, double>(j);
    else if (out64) launch_nc<Raw, float, double>(j);  // rounded in float32, then widened (exact)
    else launch_nc<Raw, float, float>(j);
}

void launch_decode(const UnpackJob& j, bool cmp64, bool out64) {
    switch (j.desc[0].raw_dtype) {
        case PK_I8: launch_types<int8_t>(j, cmp64, out64); break;
        case PK_U8: launch_types<uint8_t>(j, cmp64, out64); break;
        case PK_I16: launch_types<int16_t>(j, cmp64, out64); break;
        case PK_U16: launch_types<uint16_t>(j, cmp64, out64); break;
        default: launch_types<int32_t>(j, cmp64, out64); break;
    }
}

// read the events of the timed chunks (option "unpack_timing") into the counters; the copy stream has been synchronised
int32_t drain_events(pk_ctx* ctx) {
    for (size_t k = 0; k + 2 < ctx->unpack_ev.size(); k += 3) {
        float dma = 0, dec = 0;
        PK_HIP(ctx, hipEventElapsedTime(&dma, ctx->unpack_ev[k], ctx->unpack_ev[k + 1]));
        PK_HIP(ctx, hipEventElapsedTime(&dec, ctx->unpack_ev[k + 1], ctx->unpack_ev[k + 2]));
        ctx->unpack_dma_ms += dma;
        ctx->unpack_decode_ms += dec;
    }
    ctx->unpack_ev_free.insert(ctx->unpack_ev_free.end(), ctx->unpack_ev.begin(), ctx->unpack_ev.end());
    ctx->unpack_ev.clear();
    return 0;
}

int32_t mark(pk_ctx* ctx) {
    hipEvent_t e;
    if (!ctx->unpack_ev_free.empty()) {
        e = ctx->unpack_ev_free.back();
        ctx->unpack_ev_free.pop_back();
    } else {
        PK_HIP(ctx, hipEventCreate(&e));
    }
    ctx->unpack_ev.push_back(e);
    PK_HIP(ctx, hipEventRecord(e, ctx->copy));
    return 0;
}

// The raw planes of one level -> `dst` (the field's element of value 0 in the slot), chunk by chunk on the copy stream: DMA of the raw
// bytes into the device staging buffer, then the decode.  nc planes are written as {c0, c1, ..} structs (ostride unused), one plane with
// the element stride `ostride`.
int32_t transfer_packed(pk_ctx* ctx, const std::string& who, const HostField& F, char* dst, int ostride, const void* const* raw,
                        const pk_pack_desc* descs, int nc, int32_t async) {
    const int rsz = raw_size(descs[0].raw_dtype);
    if (!rsz) return ctx->fail(who + ": raw_dtype must be PK_I8, PK_U8, PK_I16, PK_U16 or PK_I32");
    for (int c = 0; c < nc; c++) {
        const pk_pack_desc& d = descs[c];
        if (d.raw_dtype != descs[0].raw_dtype) return ctx->fail(who + ": the components of a packed group must share one raw dtype");
        if (d.compute_dtype != PK_F32 && d.compute_dtype != PK_F64) return ctx->fail(who + ": compute_dtype must be PK_F32 or PK_F64");
        if (d.compute_dtype != descs[0].compute_dtype) return ctx->fail(who + ": the components of a packed group must share one compute dtype");
        if (d.nfill < 0 || d.nfill > 4) return ctx->fail(who + ": at most 4 fill values");
    }
    const bool cmp64 = descs[0].compute_dtype == PK_F64, out64 = F.desc.dtype == PK_F64;
    if (cmp64 && !out64) return ctx->fail(who + ": compute_dtype float64 is wider than the field's float32");
    const size_t esz = out64 ? 8 : 4;
    const int64_t level_elems = (int64_t)(F.level_bytes / esz);
    int64_t chunk = std::max<int64_t>(level_elems, 16);
    if (async) {  // the pinned ring bounds a chunk; a context that never streamed a float level pins no more than this level needs
        const size_t mib = (size_t)1 << 20;
        if (!ctx->stage_chunk) ctx->stage_chunk = std::min(PK_STAGE_CHUNK_BYTES, ((size_t)level_elems * rsz * nc + mib - 1) / mib * mib);
        chunk = std::min<int64_t>(chunk, (int64_t)(ctx->stage_chunk / ((size_t)rsz * nc)) / 16 * 16);
    }
    if (ctx->unpack_chunk_values) chunk = std::min(chunk, ctx->unpack_chunk_values);
    const size_t need = (size_t)nc * align16((size_t)std::min(chunk, level_elems) * rsz);
    if (ctx->unpack_tmp_bytes < need) {
        PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
        if (ctx->d_unpack_tmp) PK_HIP(ctx, hipFree(ctx->d_unpack_tmp));
        ctx->d_unpack_tmp = nullptr;
        ctx->unpack_tmp_bytes = 0;
        PK_HIP(ctx, hipMalloc(&ctx->d_unpack_tmp, need));
        ctx->unpack_tmp_bytes = need;
    }
    UnpackJob j{};
    j.desc = descs;
    j.nc = nc;
    j.ostride = ostride;
    j.max_blocks = (unsigned)std::max(1, ctx->prop.multiProcessorCount) * 8;
    j.stream = ctx->copy;
    char* tmp = (char*)ctx->d_unpack_tmp;
    for (int64_t off = 0; off < level_elems; off += chunk) {
        const int64_t len = std::min(chunk, level_elems - off);
        const size_t plane = (size_t)len * rsz, pstride = align16(plane);
        if (async) {  // pageable memory cannot be DMA'd asynchronously: bounce the raw planes through the ring of pinned chunks
            int k;
            if (int32_t rc = stage_acquire(ctx, &k)) return rc;
            const double t0 = now_s();
            for (int c = 0; c < nc; c++) parallel_memcpy((char*)ctx->stage[k] + c * pstride, (const char*)raw[c] + (size_t)off * rsz, plane);
            ctx->stage_fill_s += now_s() - t0;
            if (ctx->unpack_timing)
                if (int32_t rc = mark(ctx)) return rc;
            if (int32_t rc = stage_submit(ctx, k, tmp, (size_t)nc * pstride)) return rc;
        } else {
            if (ctx->unpack_timing)
                if (int32_t rc = mark(ctx)) return rc;
            for (int c = 0; c < nc; c++)
                PK_HIP(ctx, hipMemcpyAsync(tmp + c * pstride, (const char*)raw[c] + (size_t)off * rsz, plane, hipMemcpyHostToDevice, ctx->copy));
        }
        if (ctx->unpack_timing)
            if (int32_t rc = mark(ctx)) return rc;
        for (int c = 0; c < nc; c++) j.raw[c] = tmp + c * pstride;
        j.out = dst + (size_t)off * esz * (nc > 1 ? nc : ostride);
        j.n = len;
        launch_decode(j, cmp64, out64);
        PK_HIP(ctx, hipGetLastError());
        if (ctx->unpack_timing) {
            if (int32_t rc = mark(ctx)) return rc;
            if (ctx->unpack_ev.size() >= 3 * 256) {  // a measurement option: reading the events waits for the stream
                PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
                if (int32_t rc = drain_events(ctx)) return rc;
            }
        }
    }
    if (!async) PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
    ctx->unpack_levels += 1;
    ctx->unpack_raw_bytes += (double)level_elems * rsz * nc;
    return 0;
}

}  // namespace

extern "C" {

int32_t pk_field_upload_level_packed(pk_ctx* ctx, int32_t field_id, int32_t level, const void* raw, const pk_pack_desc* desc, int32_t async) {
    if (!ctx || !raw || !desc) return -2;
    if (field_id < 0 || field_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    HostField& f = ctx->fields[field_id];
    if (level < 0 || level >= f.desc.nt) return ctx->fail("time level out of range");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int slot = level % f.d.nslots;
    const int ncomp = f.d.ncomp;
    const size_t esz = f.desc.dtype == PK_F64 ? 8 : 4;
    char* dst = (char*)f.dev_data + ((size_t)slot * f.level_bytes * ncomp) + (size_t)f.d.comp * esz;
    if (int32_t rc = transfer_packed(ctx, "pk_field_upload_level_packed", f, dst, ncomp, &raw, desc, 1, async)) return rc;
    f.slot_gen[slot] = ++ctx->upload_counter;
    if (async) {  // usable only after pk_field_sync(); the level that lived in this slot is gone as of now
        f.slot_level[slot] = -1;
        f.slot_pending[slot] = level;
        ctx->copy_pending = true;
    } else {
        f.slot_level[slot] = level;
        f.slot_pending[slot] = -1;
    }
    return 0;
}

int32_t pk_field_upload_group_level_packed(pk_ctx* ctx, int32_t leader_id, int32_t level, const void* const* raw, const pk_pack_desc* descs,
                                           int32_t ncomp_given, int32_t async) {
    if (!ctx || !raw || !descs) return -2;
    if (leader_id < 0 || leader_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    HostField& L = ctx->fields[leader_id];
    const int ncomp = L.d.ncomp;
    if (ncomp <= 1 || !L.owns_data) return ctx->fail("pk_field_upload_group_level_packed: the field does not lead a packed group");
    if (ncomp_given != ncomp || L.pack_used != ncomp)
        return ctx->fail("pk_field_upload_group_level_packed: one raw level per component of the complete group is required");
    if (ncomp > 3) return ctx->fail("pk_field_upload_group_level_packed: at most 3 components");
    if (level < 0 || level >= L.desc.nt) return ctx->fail("time level out of range");
    for (int k = 0; k < ncomp; k++)
        if (!raw[k]) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int slot = level % L.d.nslots;
    char* dst = (char*)L.dev_data + (size_t)slot * L.level_bytes * ncomp;
    if (int32_t rc = transfer_packed(ctx, "pk_field_upload_group_level_packed", L, dst, 1, raw, descs, ncomp, async)) return rc;
    for (size_t f = 0; f < ctx->fields.size(); f++) {  // the leader and its followers change slot state together
        HostField& F = ctx->fields[f];
        if ((int)f != leader_id && F.desc.pack_leader != leader_id) continue;
        F.slot_gen[slot] = ++ctx->upload_counter;
        F.slot_level[slot] = async ? -1 : level;
        F.slot_pending[slot] = async ? level : -1;
    }
    if (async) ctx->copy_pending = true;
    return 0;
}

int32_t pk_field_download_level(pk_ctx* ctx, int32_t field_id, int32_t level, void* out) {
    if (!ctx || !out) return -2;
    if (field_id < 0 || field_id >= (int)ctx->fields.size()) return ctx->fail("unknown field id");
    HostField& f = ctx->fields[field_id];
    if (level < 0 || level >= f.desc.nt) return ctx->fail("time level out of range");
    const int slot = level % f.d.nslots;
    if (f.slot_level[slot] != level)
        return ctx->fail("pk_field_download_level: level " + std::to_string(level) + " of field " + std::to_string(field_id) +
                         (f.slot_pending[slot] == level ? " is pending, not resident (pk_field_sync commits it)" : " is not resident"));
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int ncomp = f.d.ncomp;
    const size_t esz = f.desc.dtype == PK_F64 ? 8 : 4;
    const char* src = (const char*)f.dev_data + ((size_t)slot * f.level_bytes * ncomp) + (size_t)f.d.comp * esz;
    if (ncomp > 1) {  // one component of the {U,V,W} structs: gather it into the device staging buffer of the per-field uploads
        if (ctx->pack_tmp_bytes < f.level_bytes) {
            PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
            if (ctx->d_pack_tmp) PK_HIP(ctx, hipFree(ctx->d_pack_tmp));
            ctx->d_pack_tmp = nullptr;
            ctx->pack_tmp_bytes = 0;
            PK_HIP(ctx, hipMalloc(&ctx->d_pack_tmp, f.level_bytes));
            ctx->pack_tmp_bytes = f.level_bytes;
        }
        const int64_t n = (int64_t)(f.level_bytes / esz);
        const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32);
        if (esz == 8) hipLaunchKernelGGL((deinterleave_kernel<double>), dim3(grid), dim3(256), 0, ctx->copy, (const double*)src, (double*)ctx->d_pack_tmp, n, ncomp);
        else hipLaunchKernelGGL((deinterleave_kernel<float>), dim3(grid), dim3(256), 0, ctx->copy, (const float*)src, (float*)ctx->d_pack_tmp, n, ncomp);
        PK_HIP(ctx, hipGetLastError());
        src = (const char*)ctx->d_pack_tmp;
    }
    PK_HIP(ctx, hipMemcpyAsync(out, src, f.level_bytes, hipMemcpyDeviceToHost, ctx->copy));
    PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
    return 0;
}

int32_t pk_unpack_stats(pk_ctx* ctx, double* out4) {
    if (!ctx || !out4) return -2;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->unpack_ev.empty()) {
        PK_HIP(ctx, hipStreamSynchronize(ctx->copy));
        if (int32_t rc = drain_events(ctx)) return rc;
    }
    out4[0] = ctx->unpack_levels;     // levels (group levels count once) that took the packed entry points
    out4[1] = ctx->unpack_raw_bytes;  // their raw bytes
    out4[2] = ctx->unpack_dma_ms;     // option "unpack_timing": milliseconds of the chunks' DMAs ...
    out4[3] = ctx->unpack_decode_ms;  // ... and of their decode kernels, from HIP events on the copy stream
    return 0;
}

}  // extern "C"
