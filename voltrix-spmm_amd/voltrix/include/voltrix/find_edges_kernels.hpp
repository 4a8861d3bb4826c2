// Voltrix-SpMM for MI355X (gfx950) -- the lookup from (row, column) to the CSR entry id: what turns a link-prediction batch's edges
// into their reverses' entry ids, the exclusion list of neighbor_sample_kernels.hpp (DGL's edge_ids / has_edges_between).
//   out [Q] = for every query (rows[i], cols[i]), the id of the first entry of that row with that column, or -1
// No reference counterpart.  voltrix/negative.py and DESIGN.md 3.26 restate the contract, tests/exclude_oracle.py is the numpy
// restatement.
//
// (ROW, COLUMN) -> ENTRY.  The package keeps no [nnz] key array, so this is a search, like entry_row:
// find_entry<SORTED>(r, c) is the id of the FIRST entry of row r whose column is c, or -1 if there is none or r is outside
// [0, num_rows).  SORTED = true is the precondition of negative_sample (every row's columns ascend, duplicates allowed): a lower
// bound, O(log d).  SORTED = false: a linear scan by the query's one lane, O(d): the slow path, not tuned.  On sorted input both give
// the same bits.  find_edges_kernel<SORTED>: one lane per query; every element of out is written.
//
// No atomics; no host synchronisation.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "voltrix/launch_geometry.hpp"

namespace voltrix {

// The id of the first entry of row r whose column is c, or -1.  The kernel and a host program run this code.
template <bool SORTED>
__host__ __device__ inline int find_entry(const int* indptr, const int* indices, int num_rows, int r, int c) {
  if (r < 0 || r >= num_rows) return -1;
  const int begin = indptr[r];
  const int d = indptr[r + 1] - begin;
  const int* row = indices + begin;
  if constexpr (SORTED) {
    int lo = 0, hi = d;       // the first position whose column is not below c
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (row[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < d && row[lo] == c ? begin + lo : -1;
  } else {
    for (int i = 0; i < d; ++i)
      if (row[i] == c) return begin + i;
    return -1;
  }
}

template <bool SORTED>
static __global__ __launch_bounds__(256) void find_edges_kernel(const int* indptr, const int* indices, const int* rows, const int* cols,
                                                                int num_rows, int num_queries, int* out) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= num_queries) return;
  out[i] = find_entry<SORTED>(indptr, indices, num_rows, rows[i], cols[i]);
}

// out = device int32 [num_queries], every element written.  num_entries = the CSR's entry count (indices may be null only where it
// is 0).  num_queries == 0: kOk without a launch.
inline int launch_find_edges(const int* indptr, const int* indices, int num_rows, long long num_entries, const int* rows, const int* cols,
                             int num_queries, int assume_sorted, int* out, hipStream_t stream) {
  if (num_rows < 0 || num_queries < 0 || num_entries < 0 || num_entries > INT_MAX) return kErrBadShape;
  if (assume_sorted != 0 && assume_sorted != 1) return kErrBadShape;
  if (num_queries == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(rows, 3) || bad_ptr(cols, 3) || bad_ptr(out, 3)) return kErrBadShape;
  if (num_entries > 0 ? bad_ptr(indices, 3) : misaligned(indices, 3)) return kErrBadShape;
  const dim3 grid((unsigned)(((long long)num_queries + 255) / 256));
  if (assume_sorted)
    hipLaunchKernelGGL((find_edges_kernel<true>), grid, dim3(256), 0, stream, indptr, indices, rows, cols, num_rows, num_queries, out);
  else
    hipLaunchKernelGGL((find_edges_kernel<false>), grid, dim3(256), 0, stream, indptr, indices, rows, cols, num_rows, num_queries, out);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
