// libvoltrix_hip.so -- aggregation with a feature vector per edge on a CSR pattern (mul / add / add_relu / copy, and gate for the
// backward on the transpose) and the gradient for the edge features (include/voltrix_capi.h; voltrix/spmm_edge_kernels.hpp).  The two
// entry points RETURN their status code.
#include <hip/hip_runtime.h>

#include "voltrix/spmm_edge_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

int voltrix_spmm_edge_csr(void* indptr, void* indices, void* order, int num_rows, int64_t num_entries, int embedding_dim, void* input,
                          int input_dtype, void* efeat, int efeat_dtype, void* self, int op, void* output, void* stream) {
  return voltrix::launch_spmm_edge(static_cast<const int*>(indptr), static_cast<const int*>(indices), static_cast<const int*>(order),
                                   num_rows, (long long)num_entries, embedding_dim, input, input_dtype, efeat, efeat_dtype, self, op,
                                   static_cast<float*>(output), static_cast<hipStream_t>(stream));
}

int voltrix_spmm_edge_grad_efeat_csr(void* indptr, void* indices, int num_rows, int64_t num_entries, int embedding_dim, void* grad_out,
                                     void* feat, void* efeat, int dtype, int op, void* output, void* stream) {
  return voltrix::launch_spmm_edge_grad_efeat(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                              (long long)num_entries, embedding_dim, static_cast<const float*>(grad_out), feat, efeat,
                                              dtype, op, static_cast<float*>(output), static_cast<hipStream_t>(stream));
}

}  // extern "C"
