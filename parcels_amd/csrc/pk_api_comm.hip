// pk_api_comm.hip -- the multi-GPU exchange of the path through the C ABI (pk_allgather_output; 8e): RCCL over xGMI, one
// pk_ctx (= one process, one GPU) per rank.  It works on pk_ctx's device columns, streams and row permutation (pk_api_ctx.h).
//
// What is exchanged (the path has no data-path collective: particles are independent, fields replicated):
//   * the periodic write-out: the rows that pass the reference's write filter |t_p - t| <= |dt|/2 (particlefile.py:198-221) -- applied ON THE
//     DEVICE, in host row order -- of the to-write columns, gathered to rank 0 (what ParticleFile.write needs: pk_gather_rows_to_root) or to
//     every rank (the all-gather the north star names: pk_allgather_output);
//   * the batch agreements of Kernel.execute (first erring iteration, first failing sample, error codes present): pk_comm_allreduce_i64.
// librccl.so is opened with dlopen at pk_comm_init: a single-GPU host never loads it, and the library has no link-time dependency on it.
// Ranks may hold different, also zero, row counts (the counts are all-gathered first; the rows travel as grouped ncclSend / ncclRecv of
// bytes -- an all-gather-v).  Rounds 1-5 did all of this in Python over torch.distributed (parcels_amd/distributed.py); that module is now a
// thin caller of these entry points whenever the process group is RCCL, and keeps its torch path for gloo (the N > 1 CPU tests).
#include "pk_api_ctx.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

using namespace pkapi;

namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

RcclApi& rccl() {
    static RcclApi api;
    return api;
}

bool rccl_load() {
    RcclApi& a = rccl();
    if (a.lib) return true;
    if (!a.error.empty()) return false;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* n : names) {
        a.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (a.lib) break;
    }
    if (!a.lib) {
        a.error = std::string("cannot open librccl.so: ") + (dlerror() ? dlerror() : "?");
        return false;
    }
    bool ok = true;
    auto sym = [&](const char* name) {
        void* p = dlsym(a.lib, name);
        if (!p) {
            ok = false;
            a.error = std::string("librccl.so lacks ") + name;
        }
        return p;
    };
    a.GetUniqueId = (decltype(a.GetUniqueId))sym("ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))sym("ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))sym("ncclCommDestroy");
    a.GetVersion = (decltype(a.GetVersion))sym("ncclGetVersion");
    a.AllReduce = (decltype(a.AllReduce))sym("ncclAllReduce");
    a.AllGather = (decltype(a.AllGather))sym("ncclAllGather");
    a.Send = (decltype(a.Send))sym("ncclSend");
    a.Recv = (decltype(a.Recv))sym("ncclRecv");
    a.GroupStart = (decltype(a.GroupStart))sym("ncclGroupStart");
    a.GroupEnd = (decltype(a.GroupEnd))sym("ncclGroupEnd");
    a.GetErrorString = (decltype(a.GetErrorString))sym("ncclGetErrorString");
    if (!ok) {
        dlclose(a.lib);
        a.lib = nullptr;
    }
    return ok;
}

}  // namespace

// per-context state of the exchange (pk_ctx::comm)
struct PkComm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    // device staging: this rank's selected rows (pk_api.hip: select_column) and the gathered rows, per column
    void* d_sel[PK_NCOLS] = {};
    size_t sel_bytes[PK_NCOLS] = {};
    void* d_all[PK_NCOLS] = {};
    size_t all_bytes[PK_NCOLS] = {};
    long long* d_counts = nullptr;  // [world] (+ 1: this rank's count as the all-gather's send buffer)
    long long* d_red = nullptr;     // pk_comm_allreduce_i64
    int red_cap = 0;
    std::vector<int64_t> counts;    // of the last exchange
    int64_t total = 0;              // rows this rank holds gathered (0 on the ranks a gather-to-root skipped)
    uint32_t mask = 0;
    size_t elem[PK_NCOLS] = {};
    int width[PK_NCOLS] = {};
};

#define PK_NCCL(ctx, call)                                                                            \
    do {                                                                                              \
        ncclResult_t r_ = (call);                                                                     \
        if (r_ != ncclSuccess) return (ctx)->fail(std::string(#call) + ": " + rccl().GetErrorString(r_)); \
    } while (0)

static int32_t comm_grow(pk_ctx* ctx, void** p, size_t* have, size_t need) {
    if (*have >= need && *p) return 0;
    if (*p) PK_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *have = 0;
    const size_t cap = std::max<size_t>(need + need / 8, 256);
    PK_HIP(ctx, hipMalloc(p, cap));
    *have = cap;
    return 0;
}

// The selected rows of the masked columns, packed in host row order in PkComm::d_sel (pk_api.hip: select_flags, select_column); -> their number
static int32_t comm_select(pk_ctx* ctx, PkComm& cm, double t, int apply_filter, uint32_t mask, int64_t* n_sel) {
    const std::vector<ColRef> cols = particle_columns(ctx);
    cm.mask = 0;
    for (int k = 0; k < PK_NCOLS; k++) {
        cm.elem[k] = cols[k].elem;
        cm.width[k] = cols[k].width;
        if (((mask >> k) & 1u) && cols[k].d) cm.mask |= 1u << k;
    }
    int64_t ns = 0;
    int32_t rc = select_flags(ctx, t, apply_filter, &ns);
    if (rc) return rc;
    for (int k = 0; k < PK_NCOLS && ns > 0; k++) {
        if (!((cm.mask >> k) & 1u)) continue;
        const ColRef& c = cols[k];
        rc = comm_grow(ctx, &cm.d_sel[k], &cm.sel_bytes[k], (size_t)ns * c.elem * c.width);
        if (rc) return rc;
        select_column(ctx, c, cm.d_sel[k]);
    }
    PK_HIP(ctx, hipGetLastError());
    *n_sel = ns;
    return 0;
}

// counts of all ranks (all-gather of one int64), then the rows: to rank 0 only (to_all = 0) or to every rank
static int32_t comm_exchange(pk_ctx* ctx, PkComm& cm, int64_t n_sel, int to_all, int64_t* counts_out) {
    RcclApi& R = rccl();
    const int W = cm.world, me = cm.rank;
    if (!cm.d_counts) PK_HIP(ctx, hipMalloc((void**)&cm.d_counts, sizeof(long long) * (size_t)(W + 1)));
    const long long mine = (long long)n_sel;
    PK_HIP(ctx, hipMemcpyAsync(cm.d_counts + W, &mine, 8, hipMemcpyHostToDevice, ctx->compute));
    PK_NCCL(ctx, R.AllGather(cm.d_counts + W, cm.d_counts, 1, ncclInt64, cm.comm, ctx->compute));
    std::vector<long long> cnt((size_t)W);
    PK_HIP(ctx, hipMemcpyAsync(cnt.data(), cm.d_counts, sizeof(long long) * (size_t)W, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    cm.counts.assign(cnt.begin(), cnt.end());
    int64_t total = 0;
    std::vector<int64_t> start((size_t)W);
    for (int r = 0; r < W; r++) {
        start[r] = total;
        total += cnt[r];
        if (counts_out) counts_out[r] = cnt[r];
    }
    const bool receiver = to_all || me == 0;
    cm.total = receiver ? total : 0;
    for (int k = 0; k < PK_NCOLS; k++) {
        if (!((cm.mask >> k) & 1u)) continue;
        const size_t row = cm.elem[k] * (size_t)cm.width[k];
        if (receiver && total > 0) {
            int32_t rc = comm_grow(ctx, &cm.d_all[k], &cm.all_bytes[k], (size_t)total * row);
            if (rc) return rc;
            if (n_sel > 0)
                PK_HIP(ctx, hipMemcpyAsync((char*)cm.d_all[k] + (size_t)start[me] * row, cm.d_sel[k], (size_t)n_sel * row, hipMemcpyDeviceToDevice, ctx->compute));
        }
        if (W == 1) continue;
        PK_NCCL(ctx, R.GroupStart());
        for (int r = 0; r < W; r++) {
            if (r == me) continue;
            const bool r_receives = to_all || r == 0;
            if (r_receives && n_sel > 0) PK_NCCL(ctx, R.Send(cm.d_sel[k], (size_t)n_sel * row, ncclInt8, r, cm.comm, ctx->compute));
            if (receiver && cnt[r] > 0)
                PK_NCCL(ctx, R.Recv((char*)cm.d_all[k] + (size_t)start[r] * row, (size_t)cnt[r] * row, ncclInt8, r, cm.comm, ctx->compute));
        }
        PK_NCCL(ctx, R.GroupEnd());
    }
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

extern "C" {

int32_t pk_comm_unique_id(uint8_t* id128) {
    if (!id128) return -2;
    if (!rccl_load()) {
        g_init_error = rccl().error;
        return -2;
    }
    ncclUniqueId id;
    const ncclResult_t r = rccl().GetUniqueId(&id);
    if (r != ncclSuccess) {
        g_init_error = std::string("ncclGetUniqueId: ") + rccl().GetErrorString(r);
        return -1;
    }
    static_assert(sizeof(id.internal) == PK_COMM_ID_BYTES, "PK_COMM_ID_BYTES is NCCL_UNIQUE_ID_BYTES");
    memcpy(id128, id.internal, PK_COMM_ID_BYTES);
    return 0;
}

int32_t pk_comm_init(pk_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id128) {
    if (!ctx || !id128) return -2;
    if (world < 1 || rank < 0 || rank >= world) return ctx->fail("pk_comm_init: rank / world out of range");
    if (ctx->comm) return ctx->fail("pk_comm_init: this context already has a communicator (pk_comm_destroy first)");
    if (!rccl_load()) return ctx->fail(rccl().error);
    PK_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId id;
    memcpy(id.internal, id128, PK_COMM_ID_BYTES);
    PkComm* cm = new PkComm();
    cm->rank = rank;
    cm->world = world;
    const ncclResult_t r = rccl().CommInitRank(&cm->comm, world, id, rank);
    if (r != ncclSuccess) {
        delete cm;
        return ctx->fail(std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
    }
    ctx->comm = cm;
    return 0;
}

int32_t pk_comm_destroy(pk_ctx* ctx) {
    if (!ctx) return -2;
    PkComm* cm = ctx->comm;
    if (!cm) return 0;
    (void)hipSetDevice(ctx->device);
    if (cm->comm) (void)rccl().CommDestroy(cm->comm);
    for (int k = 0; k < PK_NCOLS; k++) {
        if (cm->d_sel[k]) (void)hipFree(cm->d_sel[k]);
        if (cm->d_all[k]) (void)hipFree(cm->d_all[k]);
    }
    if (cm->d_counts) (void)hipFree(cm->d_counts);
    if (cm->d_red) (void)hipFree(cm->d_red);
    delete cm;
    ctx->comm = nullptr;
    return 0;
}

int32_t pk_comm_info(pk_ctx* ctx, int32_t* rank, int32_t* world, int32_t* rccl_version) {
    if (!ctx) return -2;
    if (!ctx->comm) return ctx->fail("no communicator (pk_comm_init)");
    if (rank) *rank = ctx->comm->rank;
    if (world) *world = ctx->comm->world;
    if (rccl_version) {
        int v = 0;
        (void)rccl().GetVersion(&v);
        *rccl_version = v;
    }
    return 0;
}

int32_t pk_comm_allreduce_i64(pk_ctx* ctx, int64_t* values, int32_t n, int32_t op) {
    if (!ctx || !values || n < 0) return -2;
    PkComm* cm = ctx->comm;
    if (!cm) return ctx->fail("no communicator (pk_comm_init)");
    if (op != PK_OP_MIN && op != PK_OP_MAX && op != PK_OP_SUM) return ctx->fail("pk_comm_allreduce_i64: op must be PK_OP_MIN / PK_OP_MAX / PK_OP_SUM");
    if (n == 0) return 0;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    if (cm->red_cap < n) {
        if (cm->d_red) PK_HIP(ctx, hipFree(cm->d_red));
        cm->d_red = nullptr;
        PK_HIP(ctx, hipMalloc((void**)&cm->d_red, sizeof(long long) * (size_t)std::max(n, 64)));
        cm->red_cap = std::max(n, 64);
    }
    PK_HIP(ctx, hipMemcpyAsync(cm->d_red, values, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->compute));
    const ncclRedOp_t rop = op == PK_OP_MIN ? ncclMin : (op == PK_OP_MAX ? ncclMax : ncclSum);
    PK_NCCL(ctx, rccl().AllReduce(cm->d_red, cm->d_red, (size_t)n, ncclInt64, rop, cm->comm, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(values, cm->d_red, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

// every rank's n int64 to every rank, in rank order (the key exchange of the batch agreements: count + keys per rank)
int32_t pk_comm_allgather_i64(pk_ctx* ctx, const int64_t* send, int32_t n, int64_t* recv) {
    if (!ctx || !send || !recv || n < 0) return -2;
    PkComm* cm = ctx->comm;
    if (!cm) return ctx->fail("no communicator (pk_comm_init)");
    if (n == 0) return 0;
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const int need = n * (cm->world + 1);
    if (cm->red_cap < need) {
        if (cm->d_red) PK_HIP(ctx, hipFree(cm->d_red));
        cm->d_red = nullptr;
        PK_HIP(ctx, hipMalloc((void**)&cm->d_red, sizeof(long long) * (size_t)std::max(need, 64)));
        cm->red_cap = std::max(need, 64);
    }
    long long* d_send = cm->d_red + (size_t)n * cm->world;
    PK_HIP(ctx, hipMemcpyAsync(d_send, send, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->compute));
    PK_NCCL(ctx, rccl().AllGather(d_send, cm->d_red, (size_t)n, ncclInt64, cm->comm, ctx->compute));
    PK_HIP(ctx, hipMemcpyAsync(recv, cm->d_red, sizeof(int64_t) * (size_t)n * cm->world, hipMemcpyDeviceToHost, ctx->compute));
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

static int32_t comm_gather(pk_ctx* ctx, double t, int32_t apply_filter, uint32_t mask, int64_t* counts, int to_all) {
    if (!ctx) return -2;
    PkComm* cm = ctx->comm;
    if (!cm) return ctx->fail("no communicator (pk_comm_init)");
    if (!ctx->bound) return ctx->fail("no particles bound");
    if (ctx->in_flight) return ctx->fail("the write-out exchange: a launch is in flight (call pk_execute_end)");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    int64_t n_sel = 0;
    int32_t rc = comm_select(ctx, *cm, t, apply_filter, mask, &n_sel);
    if (rc) return rc;
    return comm_exchange(ctx, *cm, n_sel, to_all, counts);
}

int32_t pk_gather_rows_to_root(pk_ctx* ctx, double t, int32_t apply_filter, uint32_t mask, int64_t* counts) {
    return comm_gather(ctx, t, apply_filter, mask, counts, 0);
}

int32_t pk_allgather_output(pk_ctx* ctx, double t, int32_t apply_filter, uint32_t mask, int64_t* counts) {
    return comm_gather(ctx, t, apply_filter, mask, counts, 1);
}

int32_t pk_gathered_fetch(pk_ctx* ctx, const pk_particles_desc* out, int64_t capacity) {
    if (!ctx || !out) return -2;
    PkComm* cm = ctx->comm;
    if (!cm) return ctx->fail("no communicator (pk_comm_init)");
    if (capacity < cm->total) return ctx->fail("pk_gathered_fetch: the arrays are shorter than the gathered rows");
    PK_HIP(ctx, hipSetDevice(ctx->device));
    const auto dst = column_pointers(*out);
    for (int k = 0; k < PK_NCOLS; k++) {
        if (!((cm->mask >> k) & 1u)) continue;
        if (!dst[k]) return ctx->fail("pk_gathered_fetch: a gathered column has no destination array");
        if (cm->total > 0)
            PK_HIP(ctx, hipMemcpyAsync(dst[k], cm->d_all[k], (size_t)cm->total * cm->elem[k] * (size_t)cm->width[k], hipMemcpyDeviceToHost, ctx->compute));
    }
    PK_HIP(ctx, hipStreamSynchronize(ctx->compute));
    return 0;
}

}  // extern "C"
