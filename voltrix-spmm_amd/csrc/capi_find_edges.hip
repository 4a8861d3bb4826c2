// libvoltrix_hip.so -- the (row, column) -> entry id lookup (include/voltrix_capi.h; voltrix/find_edges_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/find_edges_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_find_edges(void* indptr, void* indices, int num_rows, int64_t num_entries, void* rows, void* cols, int num_queries,
                               int assume_sorted, void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_find_edges(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                            (long long)num_entries, static_cast<const int*>(rows), static_cast<const int*>(cols),
                                            num_queries, assume_sorted, static_cast<int*>(out), static_cast<hipStream_t>(stream));
}

}  // extern "C"
