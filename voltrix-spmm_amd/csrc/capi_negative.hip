// libvoltrix_hip.so -- negative sampling on a device CSR and the endpoints of CSR entries (include/voltrix_capi.h;
// voltrix/negative_sample_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/negative_sample_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_negative_sample(void* indptr, void* indices, int num_rows, int num_cols, int64_t num_entries, void* src, int num_src,
                                    int k, int max_tries, int exclude_self, int assume_sorted, uint64_t seed, uint64_t offset, void* neg,
                                    void* stream, int* return_code) {
  *return_code = voltrix::launch_negative_sample(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, num_cols,
                                                 (long long)num_entries, static_cast<const int*>(src), num_src, k, max_tries,
                                                 exclude_self, assume_sorted, seed, offset, static_cast<int*>(neg),
                                                 static_cast<hipStream_t>(stream));
}

void voltrix_launch_edge_endpoints(void* indptr, void* indices, int num_rows, int64_t num_entries, void* entries, int num_ids, void* rows,
                                   void* cols, void* stream, int* return_code) {
  *return_code = voltrix::launch_edge_endpoints(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                                (long long)num_entries, static_cast<const int*>(entries), num_ids,
                                                static_cast<int*>(rows), static_cast<int*>(cols), static_cast<hipStream_t>(stream));
}

}  // extern "C"
