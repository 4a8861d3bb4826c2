// libvoltrix_hip.so -- neighbour sampling on a device CSR and the relabelling of a sampled block
// (include/voltrix_capi.h; voltrix/neighbor_sample_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/neighbor_sample_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_sample_neighbors_excluding(void* indptr, void* indices, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                               int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* exclude,
                                               int num_exclude, void* s_indices, void* s_entries, void* stream, int* return_code) {
  *return_code = voltrix::launch_sample_neighbors(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, static_cast<const int*>(seeds), num_seeds,
      static_cast<const int*>(s_indptr), (long long)num_sampled, fanout, replace, seed, offset, static_cast<const int*>(exclude),
      num_exclude, static_cast<int*>(s_indices), static_cast<int*>(s_entries), static_cast<hipStream_t>(stream));
}

// the same launch without a list
void voltrix_launch_sample_neighbors(void* indptr, void* indices, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                     int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* s_indices,
                                     void* s_entries, void* stream, int* return_code) {
  voltrix_launch_sample_neighbors_excluding(indptr, indices, num_rows, seeds, num_seeds, s_indptr, num_sampled, fanout, replace, seed,
                                            offset, nullptr, 0, s_indices, s_entries, stream, return_code);
}

void voltrix_launch_block_mark(void* cols, int64_t num_sampled, int num_cols, void* table, void* stream, int* return_code) {
  *return_code = voltrix::launch_block_mark(static_cast<const int*>(cols), (long long)num_sampled, num_cols, static_cast<int*>(table),
                                            static_cast<hipStream_t>(stream));
}

void voltrix_launch_block_mark_seeds(void* seeds, int num_seeds, int num_cols, void* table, void* stream, int* return_code) {
  *return_code = voltrix::launch_block_mark_seeds(static_cast<const int*>(seeds), num_seeds, num_cols, static_cast<int*>(table),
                                                  static_cast<hipStream_t>(stream));
}

void voltrix_launch_block_relabel(void* cols, int64_t num_sampled, void* seeds, int num_seeds, void* table, void* rank, int num_cols,
                                  int num_src, void* local, void* src_ids, void* stream, int* return_code) {
  *return_code = voltrix::launch_block_relabel(static_cast<const int*>(cols), (long long)num_sampled, static_cast<const int*>(seeds),
                                               num_seeds, static_cast<const int*>(table), static_cast<const int*>(rank), num_cols, num_src,
                                               static_cast<int*>(local), static_cast<int*>(src_ids), static_cast<hipStream_t>(stream));
}

}  // extern "C"
