// libvoltrix_hip.so -- weighted neighbour sampling on a device CSR and its integer weight table
// (include/voltrix_capi.h; voltrix/weighted_sample_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/weighted_sample_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_sample_neighbors_weighted(void* indptr, void* indices, void* cum, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                       int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* s_indices,
                                       void* s_entries, void* stream, int* return_code) {
  *return_code = voltrix::launch_sample_neighbors_weighted(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), static_cast<const long long*>(cum), num_rows,
      static_cast<const int*>(seeds), num_seeds, static_cast<const int*>(s_indptr), (long long)num_sampled, fanout, replace, seed, offset,
      static_cast<int*>(s_indices), static_cast<int*>(s_entries), static_cast<hipStream_t>(stream));
}

}  // extern "C"
