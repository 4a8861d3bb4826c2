// libvoltrix_hip.so -- max / min / mean neighbour aggregation on a CSR pattern and the backward of max / min on its transpose
// (include/voltrix_capi.h; voltrix/spmm_csr_reduce_kernels.hpp).
#include <hip/hip_runtime.h>

#include "voltrix/spmm_csr_reduce_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_spmm_csr_reduce(void* indptr, void* indices, int num_rows, int embedding_dim, void* input, int dtype, int op,
                                    void* output, void* arg, void* stream, int* return_code) {
  *return_code = voltrix::launch_spmm_csr_reduce(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                                 embedding_dim, input, dtype, op, static_cast<float*>(output), static_cast<int*>(arg),
                                                 static_cast<hipStream_t>(stream));
}

void voltrix_launch_spmm_csr_reduce_backward(void* t_indptr, void* t_indices, void* t_order, int num_cols, int64_t num_entries,
                                             int embedding_dim, void* grad_out, void* arg, void* output, void* stream,
                                             int* return_code) {
  *return_code = voltrix::launch_spmm_csr_reduce_backward(
      static_cast<const int*>(t_indptr), static_cast<const int*>(t_indices), static_cast<const int*>(t_order), num_cols,
      (long long)num_entries, embedding_dim, static_cast<const float*>(grad_out), static_cast<const int*>(arg),
      static_cast<float*>(output), static_cast<hipStream_t>(stream));
}

}  // extern "C"
