// libvoltrix_hip.so -- induced subgraphs and random walks on a device CSR (include/voltrix_capi.h;
// voltrix/induced_subgraph_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/induced_subgraph_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_subgraph_count(void* indptr, void* indices, int num_rows, void* rows, int num_sub_rows, void* table, int num_cols,
                                   int group, void* counts, void* stream, int* return_code) {
  *return_code = voltrix::launch_subgraph_count(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                                static_cast<const int*>(rows), num_sub_rows, static_cast<const int*>(table), num_cols,
                                                group, static_cast<int*>(counts), static_cast<hipStream_t>(stream));
}

void voltrix_launch_subgraph_fill(void* indptr, void* indices, int num_rows, void* rows, int num_sub_rows, void* table, int num_cols,
                                  int group, void* s_indptr, int64_t num_selected, void* s_local, void* s_entries, void* stream,
                                  int* return_code) {
  *return_code = voltrix::launch_subgraph_fill(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                               static_cast<const int*>(rows), num_sub_rows, static_cast<const int*>(table), num_cols,
                                               group, static_cast<const int*>(s_indptr), (long long)num_selected,
                                               static_cast<int*>(s_local), static_cast<int*>(s_entries), static_cast<hipStream_t>(stream));
}

void voltrix_launch_random_walk(void* indptr, void* indices, int num_rows, void* starts, int num_walkers, int length, uint64_t seed,
                                uint64_t offset, void* nodes, void* entries, int step_major, void* stream, int* return_code) {
  *return_code = voltrix::launch_random_walk(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                             static_cast<const int*>(starts), num_walkers, length, seed, offset, static_cast<int*>(nodes),
                                             static_cast<int*>(entries), step_major, static_cast<hipStream_t>(stream));
}

}  // extern "C"
