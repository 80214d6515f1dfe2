// ParticleSet.cells / ParticleSet.connectivity on the device-resident particle columns: the label of every row (its cell by density's rule,
// or the region of that cell), and the number of rows per (origin label, destination label) pair.  The cell rule is density's
// (pk_density_cell.h); what the counts must equal is np.bincount / np.unique over origin * (n_dest + 1) + d.  Semantics and measurements:
// DESIGN.md section 15.
//
// Both calls work on the caller's stream and return 0, or a negative code with *err set.  No particle column crosses PCIe: n labels, or the
// matrix (or its non-zero pairs), a few counters and three event times come back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pk_density.h"

namespace pk {

// The labels of the cells and of the rows.  regions / origin_host are HOST arrays (copied to the device for the call); origin_dev is a
// device column in DEVICE row order.  dtype: PK_DENSITY_I32 or PK_DENSITY_I64.
struct ConnLabels {
    const void* regions = nullptr;  // ncells labels, NULL: the label of a cell is the cell
    int32_t regions_dtype = 0;
    const void* origin_dev = nullptr;
    const void* origin_host = nullptr;  // n labels in HOST row order (read through perm)
    int32_t origin_dtype = 0;
    int64_t n_origin = 0, n_dest = 0;
};

// labels_out: n int64 on the host in HOST row order; -1 = outside or a cell whose region label is negative.
int cells_run(hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const ConnLabels& l, int64_t ncells, int64_t* labels_out,
              std::string* err);

// path PK_CONN_LDS / PK_CONN_GLOBAL: dense_out = n_origin * (n_dest + 1) int64 on the host, row-major, the last column = outside.
// path PK_CONN_SPARSE: keys_out / counts_out = room for max_pairs int64 each on the host; info->n_pairs of them are written, ascending by key
// = origin * (n_dest + 1) + d (d = n_dest: outside).
int connectivity_run(hipStream_t stream, const DGrid& g, const DensityColumns& c, int32_t levels, const ConnLabels& l, int64_t ncells, int32_t path,
                     int64_t* dense_out, int64_t* keys_out, int64_t* counts_out, int64_t max_pairs, pk_connectivity_info_t* info, std::string* err);

}  // namespace pk
