// libvoltrix_hip.so -- neighbour sampling that leaves a set of CSR entries out, and the (row, column) -> entry id lookup
// (include/voltrix_capi.h; voltrix/neighbor_sample_exclude_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/neighbor_sample_exclude_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_sample_neighbors_excluding(void* indptr, void* indices, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                               int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* exclude,
                                               int num_exclude, void* s_indices, void* s_entries, void* stream, int* return_code) {
  *return_code = voltrix::launch_sample_neighbors_excluding(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, static_cast<const int*>(seeds), num_seeds,
      static_cast<const int*>(s_indptr), (long long)num_sampled, fanout, replace, seed, offset, static_cast<const int*>(exclude),
      num_exclude, static_cast<int*>(s_indices), static_cast<int*>(s_entries), static_cast<hipStream_t>(stream));
}

void voltrix_launch_find_edges(void* indptr, void* indices, int num_rows, int64_t num_entries, void* rows, void* cols, int num_queries,
                               int assume_sorted, void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_find_edges(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                            (long long)num_entries, static_cast<const int*>(rows), static_cast<const int*>(cols),
                                            num_queries, assume_sorted, static_cast<int*>(out), static_cast<hipStream_t>(stream));
}

}  // extern "C"
