// pk_api_ctx.h -- private to the host side of libparcels_hip.so (pk_api.hip and the pk_api_*.hip units split off it: the C ABI of
// include/parcels_hip.h): the context every entry point works on, the table of the particle columns, and the host functions one unit
// calls in another.  The context owns device memory (grids, field-level rings, particle columns), two HIP streams (compute + copy, so
// that the upload of the next time level overlaps the RK sub-steps of the current one) and the state of the launch in flight.
// gfx950 only; no CUDA/other-backend paths.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "pk_hashbuild.h"
#include "pk_neighbors.h"
#include "pk_interact.h"
#include "pk_density.h"
#include "pk_connectivity.h"
#include "pk_host_stage.h"
#include "pk_kernels.h"
#include "pk_ux.h"
#include "pk_sigma.h"

using namespace pk;

struct HostGrid {
    pk_grid_desc desc;
    DGrid d;
    std::vector<void*> allocs;
    int64_t h_nentries = 0;
};

struct HostField {
    pk_field_desc desc;
    DField d;
    void* dev_data = nullptr;
    double* dev_time = nullptr;
    size_t level_bytes = 0;
    std::vector<double> time;
    bool owns_data = true;   // false for followers of a packed group (the leader owns the interleaved buffer)
    int pack_used = 1;       // leader: components handed out so far
    std::vector<int32_t> slot_level;    // committed (usable) level per ring slot, -1 = empty
    std::vector<int32_t> slot_pending;  // level being copied into the slot (async upload), -1 = none
    std::vector<uint64_t> slot_gen;     // stamp of the last upload into the slot (pk_ctx::upload_counter): tells a re-upload of the same level apart
};

// ---- the particle columns: ONE table -------------------------------------------------------------------
// Every operation on the particle columns (allocate, free, copy, sort, compact, checkpoint, snapshot, exchange) walks this list, in this
// order: it is the bit order of the PK_COL_* masks, the layout of the checkpoint buffer and the order of the exchange.
//   X(member of pk_particles_desc and of DParticles, mask bit, element bytes, `ngrids` values per row, exists only where the host binds one)
// COL_SPATIAL: 4 or 8 bytes by pk_particles_desc::spatial_dtype.  Behind these rows come the PK_MAX_EXTRA user columns (index
// PK_COL_EXTRA_FIRST + k, bit PK_COL_EXTRA0 << k, 4 or 8 bytes by extra_dtype[k], optional, no launch writes them) and the device-only
// `iter` (index PK_NCOLS of particle_columns: no bit, 4 bytes, written by a launch).
constexpr int COL_SPATIAL = 0;
// the columns an advection launch writes: with `iter`, the members of DPOut (pk_device.h)
#define PK_LAUNCH_COLUMNS(X)                       \
    X(t, PK_COL_T, 8, false, false)                \
    X(z, PK_COL_Z, COL_SPATIAL, false, false)      \
    X(y, PK_COL_Y, COL_SPATIAL, false, false)      \
    X(x, PK_COL_X, COL_SPATIAL, false, false)      \
    X(dz, PK_COL_DZ, COL_SPATIAL, false, false)    \
    X(dy, PK_COL_DY, COL_SPATIAL, false, false)    \
    X(dx, PK_COL_DX, COL_SPATIAL, false, false)    \
    X(dt, PK_COL_DT, 8, false, false)              \
    X(next_dt, PK_COL_NEXT_DT, 8, false, true)     \
    X(state, PK_COL_STATE, 4, false, false)        \
    X(ei, PK_COL_EI, 4, true, false)
#define PK_COLUMNS(X) PK_LAUNCH_COLUMNS(X) X(particle_id, PK_COL_PARTICLE_ID, 8, false, false)

struct ColInfo { uint32_t bit; int elem; bool per_grid, optional; };
#define X(m, bit, elem, per_grid, optional) {bit, elem, per_grid, optional},
constexpr ColInfo PK_COL_INFO[] = {PK_COLUMNS(X)};
#undef X
#define X(m, bit, elem, per_grid, optional) | bit
constexpr uint32_t PK_LAUNCH_MASK = 0u PK_LAUNCH_COLUMNS(X);
#undef X
constexpr int PK_COL_EXTRA_FIRST = (int)(sizeof(PK_COL_INFO) / sizeof(PK_COL_INFO[0]));
constexpr int PK_NCOLS = PK_COL_EXTRA_FIRST + PK_MAX_EXTRA;
constexpr bool col_bits_in_table_order() {
    for (int k = 0; k < PK_COL_EXTRA_FIRST; k++)
        if (PK_COL_INFO[k].bit != 1u << k) return false;
    return PK_COL_EXTRA0 == 1u << PK_COL_EXTRA_FIRST;
}
static_assert(col_bits_in_table_order(), "the table lists the columns in the bit order of the PK_COL_* masks (parcels_hip.h)");

constexpr int PK_STAGE_BUFFERS = 3;  // pinned staging chunks of the level stream (see stage_acquire)
constexpr size_t PK_STAGE_CHUNK_BYTES = (size_t)256 << 20;  // the most one of them holds

// device scratch of the write filter (pk_api.hip: select_flags): flag per host row, exclusive scan of the flags
struct PkSelect {
    uint32_t* d_flag = nullptr;
    uint32_t* d_offs = nullptr;
    int64_t cap = 0;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
};
struct PkComm;
// {a, 1/width} rows of the coordinate vectors a dedicated kernel stages in LDS, built once per (grid, field) by coord_table
struct CoordTable {
    double* d = nullptr;  // device copy, `cap` doubles
    size_t cap = 0;
    int grid = -1, field = -1;
    bool ok = false;       // every cell width has a well-scaled reciprocal and the table fits the kernel's LDS
    int32_t off[5] = {};   // first row of each vector, then the row count
};
struct pk_ctx {
    int device = 0;
    hipStream_t compute = nullptr, copy = nullptr;
    hipStream_t probe = nullptr;     // the clock probe runs beside the advection kernel (created on first use)
    hipEvent_t ev_probe = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;  // around the pair-copy packing of a launch (ensure_velocity_pairs)
    int fl_packs = 0;                             // pairs packed ahead of the launch in flight
    bool copy_pending = false;
    std::string err;
    std::vector<HostGrid> grids;
    std::vector<HostField> fields;
    // particles
    pk_particles_desc host{};
    DParticles dev{};
    int64_t capacity = 0;
    bool bound = false;
    // sorted-order bookkeeping
    int64_t* d_perm = nullptr;      // device row -> host row (valid when has_perm)
    bool has_perm = false;
    int64_t* d_perm_alt = nullptr;
    DParticles alt{};               // second set of columns (ping-pong target of the cell sort, staging of d2h)
    unsigned long long *d_keys = nullptr, *d_keys_alt = nullptr;
    uint32_t *d_idx = nullptr, *d_idx_alt = nullptr;
    void* d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    void* d_pack_tmp = nullptr;  // device staging of one field level before it is interleaved into a packed group
    size_t pack_tmp_bytes = 0;
    // packed integer levels (pk_unpack.hip): device staging of the raw planes of one chunk -- the copy stream is ordered, so the decode of
    // chunk k has read it before the DMA of chunk k + 1 lands -- and the knobs / counters of that path
    void* d_unpack_tmp = nullptr;
    size_t unpack_tmp_bytes = 0;
    int64_t unpack_chunk_values = 0;  // option "unpack_chunk_values": cap of the values per staged chunk, 0 = what fits a staging chunk
    int unpack_timing = 0;            // option "unpack_timing": HIP events around every chunk's DMA and decode (pk_unpack_stats)
    std::vector<hipEvent_t> unpack_ev;      // three per timed chunk, not yet read: before the DMA, between DMA and decode, after the decode
    std::vector<hipEvent_t> unpack_ev_free;
    double unpack_dma_ms = 0, unpack_decode_ms = 0, unpack_levels = 0, unpack_raw_bytes = 0;
    // scratch
    DCounters* d_counters = nullptr;
    // device copy of the grid / field descriptors the kernels read through KArgs::grids / fields (pk_device.h), and its pinned source
    char *d_desc = nullptr, *h_desc = nullptr;
    size_t desc_bytes = 0;
    unsigned long long* d_summary = nullptr;  // PK_NUM_STATE_CODES counts + 2 ordered-double slots
    // pinned staging ring for async level uploads
    void* stage[PK_STAGE_BUFFERS] = {};
    size_t stage_bytes[PK_STAGE_BUFFERS] = {};
    size_t stage_chunk = 0;  // bytes per staging chunk: the largest streamed level (x its packed components), at most PK_STAGE_CHUNK_BYTES
    hipEvent_t stage_ev[PK_STAGE_BUFFERS] = {};
    int stage_next = 0;
    double stage_fill_s = 0, stage_wait_s = 0, stage_bytes_total = 0;  // pk_upload_stats
    hipDeviceProp_t prop;
    // an advection launch in flight (pk_execute_begin .. pk_execute_end)
    bool in_flight = false;
    int32_t call_have_guess0 = 0;  // have_guess0 of the call's first launch (reset_state): what a continued launch inherits
    int fl_launches = 0;
    int fl_program = 0;
    // the last advection launch wrote into the second column set, which now is `dev`; `alt` still holds what it read
    bool rerun_valid = false;
    pk_exec_params rerun_prm{};
    // launcher of the run-time compiled kernel-list interpreter that carries the user kernels (pk_set_user_program)
    void (*user_launch)(const void*, int32_t, int32_t, int32_t, uint64_t, void*) = nullptr;
    int32_t user_flags = 0;
    int32_t user_nsample = 0;       // scalar fields the module's user kernels sample (PK_USER_RIDE modules)
    int32_t user_sample_fid[4] = {0, 0, 0, 0};
    // pk_particles_checkpoint: one packed device copy of every column (+ the row permutation of the cell sort)
    char* d_chk = nullptr;
    size_t chk_bytes = 0;
    bool chk_valid = false, chk_has_perm = false;
    int64_t chk_n = 0;
    bool fl_sorted = false;
    int64_t fl_n = 0;
    DCounters* h_counters = nullptr;          // pinned: the async D2H of the counters must not block the host
    DCounters h_counters0;                    // initial values of a launch's counters (pageable: the H2D copy stages it at once)
    unsigned long long* d_twe = nullptr;      // PK_MAX_TWE keys: the failing samples a launch knows (pk_exec_params.twe_key)
    unsigned long long* d_twe_found = nullptr;  // TWE_FOUND_SLOTS: hash set of the unlisted failing samples of a launch (pk_device.h: twe_note_all)
    unsigned int* d_twe_hit = nullptr;          // PK_MAX_TWE: listed sample k was justified by a lane of the launch (twe_justify)
    std::vector<int64_t> twe_found_host;        // ... of the last completed launch, ascending (pk_execute_twe_report)
    std::vector<uint8_t> twe_hit_host;
    bool twe_overflow_host = false;
    int fl_twe_n = 0;                           // listed keys of the launch in flight
    std::vector<int64_t> rerun_keys;          // the keys of the last launch (pk_execute_rerun repeats it with them)
    unsigned long long* h_summary = nullptr;  // pinned
    unsigned long long* d_tstats = nullptr;   // pk_particles_t_stats: {ordered min, ordered max, NaN count} (its own 24 bytes: not the clock-probe buffer)
    unsigned long long* d_clk = nullptr;      // clock probes around the advection kernel: [before | after][XCD 0..7]{shader-clock counter, 100 MHz counter}
    unsigned long long* h_clk = nullptr;      // pinned
    // CROCO sigma grids (pk_set_croco): the {s_k, Cs_k} pairs on the device and what the kernels need beside them (pk_sigma.h)
    double* d_sigma = nullptr;
    SigmaA sigma{};
    bool has_sigma = false;
    int sort_horizontal_major = -1;  // tuning knobs (environment: PK_SORT_HORIZONTAL = 0/1 forces, PK_NO_SPECIAL, PK_NO_CELL_CACHE)
    int no_special = 0;
    bool eval_points_f32 = false;  // pk_eval: the sample points are float32 particle columns (np.cos(np.deg2rad(y)) is then a float32 cosine)
    int no_cell_cache = 0;
    int no_hash_dir = 0;
    int no_cell_table = 0;
    int no_fast = 0;
    int no_fast_cgrid = 0;
    bool no_block_cache = false;  // PK_NO_BLOCK_CACHE: the 2-D A-grid kernel without its per-lane corner-block cache
    int block_cache = -1;         // option "block_cache": -1 plan_launch's rule, 0 none, 1 stage-pair block, 2 level-pair cache or fail
    int miss_lanes = -1;          // option "miss_lanes": the most missing lanes of a wavefront the level-pair cache fetches transposed, -1 planned
    int fast_grid = 0;            // option "fast_grid": workgroups of the persistent A-grid launch -- 0 what is resident at once (pk_kernels.h), v > 0 at most v
    // asynchronous write-out snapshots (pk_particles_snapshot_begin / _wait): two sets of device staging columns (host row order)
    // + pinned host columns, so that the D2H and the encode of interval k overlap the launch of interval k+1
    struct Snapshot {
        void* dev[PK_NCOLS] = {};
        void* host[PK_NCOLS] = {};
        int64_t capacity = 0;  // rows the buffers were sized for
        int64_t n = 0;         // rows of the snapshot in flight
        uint32_t mask = 0;
        int ngrids = 0;
        size_t ss = 0;
        size_t extra_elem[PK_MAX_EXTRA] = {};
        hipEvent_t ready = nullptr, done = nullptr;
        bool in_flight = false;
    } snap[2];
    // coordinate tables of the fast A-grid path (pk_fast_agrid.h: time | depth | lat | lon) and of the fast C-grid path (pk_fast_cgrid.h:
    // time | depth), cached per (main grid, main field)
    CoordTable tab_a, tab_c;
    // fast C-grid path: per-cell records of one grid
    double* d_ct2 = nullptr;
    int ct2_grid = -1;
    int ct2_near = 0;  // FastC::near_edges of that grid
    // cell-packed pair copies of the staggered velocity for the 2-D dedicated C-grid kernels (pk_device.h: FastC::vp)
    char* d_vp = nullptr;
    size_t vp_bytes = 0;
    int vp_fU = -1, vp_fV = -1;
    std::vector<int32_t> vp_level;        // pair held by every pair slot, -1 = none
    std::vector<uint64_t> vp_gen;         // 4 stamps per pair slot: U and V uploads of both levels it was packed from
    int clock_probe = 0;        // measure the shader clock behind every advection kernel (option "clock_probe"; bench.py switches it on)
    bool fl_clock_probe = false;
    int no_velocity_pairs = 1;  // OPT-IN since round 5 (option "velocity_pairs" / PK_VELOCITY_PAIRS=1): packing a pair costs more than the
                                // launch it serves saves at BASELINE config 5 (pk_exec_stats.pack_ms)
    uint64_t upload_counter = 0;

    PkSelect sel;                   // write filter on the device rows (pk_api.hip: select_flags): the filtered snapshot and the multi-GPU exchange use it
    struct PkComm* comm = nullptr;  // the multi-GPU exchange (pk_api_comm.hip: RCCL communicator + staging), NULL until pk_comm_init
    pk::Neighbors* nbr = nullptr;   // neighbour search (pk_neighbors.hip: cell list + scratch), NULL until pk_neighbors_build
    pk::Interact* inter = nullptr;  // counters of the interaction loop (pk_interact.hip), NULL until pk_interact_prologue

    int32_t fail(const char* where, hipError_t e) {
        err = std::string(where) + ": " + hipGetErrorString(e);
        return -1;
    }
    int32_t fail(const std::string& msg) {
        err = msg;
        return -2;
    }
};

#define PK_HIP(ctx, call)                                  \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) return (ctx)->fail(#call, e_); \
    } while (0)

// Every per-column operation (pk_api.hip) derives from the table above (PK_COLUMNS).  The column pointers of a descriptor or of a device column set, in table order: named columns, then the extras
template <class S>
static std::array<void*, PK_NCOLS> column_pointers(const S& s) {
    std::array<void*, PK_NCOLS> p{};
    int k = 0;
#define X(m, bit, elem, per_grid, optional) p[k++] = s.m;
    PK_COLUMNS(X)
#undef X
    for (int e = 0; e < PK_MAX_EXTRA; e++) p[k++] = s.extra[e];
    return p;
}
// ... and the way back: every column member of `s` <- p[0 .. n_cols), n_cols = PK_COL_EXTRA_FIRST (named columns only) or PK_NCOLS
template <class S>
static void set_column_pointers(S& s, void* const* p, int n_cols) {
    int k = 0;
#define X(m, bit, elem, per_grid, optional) s.m = static_cast<decltype(s.m)>(p[k++]);
    PK_COLUMNS(X)
#undef X
    for (; k < n_cols; k++) s.extra[k - PK_COL_EXTRA_FIRST] = p[k];
}

// one column: host array, device column, alt/staging device column; launch_output: an advection launch writes it (pk_device.h: DPOut)
struct ColRef { void *h, *d, *a; size_t elem; int width; bool launch_output; };

// ---- host functions called across units, by the unit that defines them ---------------------------------------------------
// Hidden: none of them is a symbol of the library.
#pragma GCC visibility push(hidden)
namespace pkapi {

// pk_api.hip: the context
extern std::string g_init_error;  // pk_last_error(NULL): why no context (or no RCCL id) could be made

// pk_api.hip: the particle columns and the write filter
std::vector<ColRef> particle_columns(pk_ctx* ctx);
int32_t ensure_alt(pk_ctx* ctx);
void swap_column_sets(pk_ctx* ctx);
void scatter_rows(pk_ctx* ctx, const ColRef& c, void* dst, int64_t n);
int32_t select_flags(pk_ctx* ctx, double t, int apply_filter, int64_t* n_sel);
void select_column(pk_ctx* ctx, const ColRef& c, void* dst);

// pk_api.hip: the pinned staging ring of the level stream
int32_t stage_acquire(pk_ctx* ctx, int* out);
int32_t stage_submit(pk_ctx* ctx, int k, void* dst, size_t bytes);

// pk_api.hip: the launch planner
bool ctx_is_typed(const pk_ctx* ctx);
bool ctx_has_ugrid(const pk_ctx* ctx);
int32_t launch_args(pk_ctx* ctx, const pk_exec_params* prm, KArgs& a, size_t& lds_bytes, int& use_lds, bool planning = false);
int32_t upload_descriptors(pk_ctx* ctx, KArgs& a);

// pk_api_sample.hip
void sort_keys(pk_ctx* ctx, const DGrid& g, int horizontal_major);

// pk_prog_eval_attached.hip: the sampler of pk_eval_attached on structured grids (ik: 0 XLinear_Velocity / scalar, 1 CGrid_Velocity, 2 slip)
void launch_eval_attached(bool f32, int ik, bool typed, const KArgs& a, int what, int64_t m, const double* t, const double* z, const double* y,
                          const double* x, int32_t* ei, double* ou, double* ov, double* ow, int32_t* ost, hipStream_t stream);

}  // namespace pkapi
#pragma GCC visibility pop
