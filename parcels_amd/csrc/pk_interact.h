// Built-in particle-particle interaction kernels on the device-resident particle columns (parcels_amd/kernels.py: AttractTowards,
// MergeNearest) and the two ends of one host-driven iteration of the loop of Kernel.execute (reference: src/parcels/_core/kernel.py:
// 188-230; restated on the host columns in parcels_amd/hostkernels.py: execute_hosted).  Semantics: DESIGN.md section 13.2.
//
// Every function works on the caller's stream and returns 0, or a negative code with *err set.  No particle column crosses PCIe: the
// prologue and the epilogue bring back a few counters, the neighbour search the bounding-box partials and the pair total.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pk_neighbors.h"

namespace pk {

// The device columns of the bound particles in HOST row order (pk_device.h: DParticles), as far as this file touches them.
struct InteractColumns {
    int64_t n = 0;
    int32_t f32 = 0;  // storage dtype of x, y, z, dx, dy, dz: 1 float32, 0 float64
    double* t = nullptr;
    void *x = nullptr, *y = nullptr, *z = nullptr, *dx = nullptr, *dy = nullptr, *dz = nullptr;
    double* dt = nullptr;
    int32_t* state = nullptr;
    int32_t* mask = nullptr;  // the `iter` column: the `evaluate_particles` mask that body_only launches read
};

struct Interact;  // a few counters on the device + their pinned host mirror; freed with the context
Interact* interact_create();
void interact_free(Interact* it);

// kernel.py:188 (reset_state: state[:] = Evaluate); *n_evaluated: rows with state in {Success, Evaluate} and sign * (endtime - t) >= 0
// (:193-195); *n_active: rows in Evaluate or Repeat (the condition of the while loop, :190).  clip != 0 (the iteration goes ahead: the
// reference leaves before clipping when nothing is evaluated, :196-197): the mask is written into the mask column and dt is clipped for
// EVERY row (:199-203).
int interact_prologue(Interact* it, hipStream_t stream, const InteractColumns& c, double endtime, double dt0, int32_t reset_state, int32_t clip,
                      int64_t* n_evaluated, int64_t* n_active, std::string* err);

// kernel.py:219-230 for the rows of the mask: position update in the storage dtype, t += dt, dx = dy = dz = 0; then for every row
// dt = dt0 and Evaluate -> EndofLoop at t == endtime.  A step that would not advance t before endtime becomes PK_ERROR (the guard of
// advect_kernel: the loop must not spin).  *steps: rows updated; state_counts[PK_NUM_STATE_CODES]: histogram of the states after it;
// *next_evaluated, *next_active: what interact_prologue would count now, so that the loop needs one read-back per iteration.
int interact_epilogue(Interact* it, hipStream_t stream, const InteractColumns& c, double endtime, double dt0, int64_t* steps,
                      int64_t* state_counts, int64_t* next_evaluated, int64_t* next_active, std::string* err);

// AttractTowards: cell list over the rows of the mask (sources: the flags of neighbors_set_sources when use_sources), count pass; when
// the total exceeds max_pairs nothing more happens (*total tells).  Else fill, row sort and finish, then one lane per row of the mask:
// s = 0.0; s += dx / dist over its pairs in ascending j; dx column = storage(dx + (s * velocity) * dt); the same for dy (and dz with z).
// phase_ms (may be NULL): host clock of build | count, fill, sort, finish | reduce.
int interact_attract(Neighbors* nb, hipStream_t stream, const InteractColumns& c, double radius, double velocity, double sphere_radius,
                     int32_t use_z, int32_t use_sources, int64_t max_pairs, int64_t* total, double* phase_ms, std::string* err);

// MergeNearest: cell list over the rows of the mask, nearest pass (coincident points excluded), then one lane per row i: j = nn[i], go on
// iff j > i and nn[j] == i; the heavier of the two (equal masses: i) receives mass[keeper] + mass[other] in the storage dtype of the mass
// column, the other row's state becomes PK_DELETE.  phase_ms (may be NULL): build | nearest and merge.
int interact_merge(Neighbors* nb, hipStream_t stream, const InteractColumns& c, void* mass, int32_t mass_f32, double radius, double sphere_radius,
                   int32_t use_z, double* phase_ms, std::string* err);

}  // namespace pk
