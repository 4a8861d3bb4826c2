// libvoltrix_hip.so -- relational (R-GCN) aggregation over typed edges on a CSR pattern with basis decomposition: the forward, the
// contraction behind the gradient for the features, and the dots behind the gradient for the coefficients (include/voltrix_capi.h;
// voltrix/spmm_rel_kernels.hpp).  The three entry points RETURN their status code.
#include <hip/hip_runtime.h>

#include "voltrix/spmm_rel_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

int voltrix_spmm_rel_csr(void* indptr, void* indices, void* etype, void* weight, int num_rows, int64_t num_entries, int embedding_dim,
                         int num_types, int num_bases, void* input, int dtype, void* coef, void* output, void* stream) {
  return voltrix::launch_spmm_rel(static_cast<const int*>(indptr), static_cast<const int*>(indices), static_cast<const int*>(etype),
                                  static_cast<const float*>(weight), num_rows, (long long)num_entries, embedding_dim, num_types,
                                  num_bases, input, dtype, static_cast<const float*>(coef), static_cast<float*>(output),
                                  static_cast<hipStream_t>(stream));
}

int voltrix_spmm_rel_contract_csr(void* t_indptr, void* t_indices, void* order, void* etype, void* weight, int num_cols,
                                  int64_t num_entries, int embedding_dim, int num_types, int num_bases, void* grad_out, void* coef,
                                  void* output, void* stream) {
  return voltrix::launch_spmm_rel_contract(static_cast<const int*>(t_indptr), static_cast<const int*>(t_indices),
                                           static_cast<const int*>(order), static_cast<const int*>(etype),
                                           static_cast<const float*>(weight), num_cols, (long long)num_entries, embedding_dim,
                                           num_types, num_bases, static_cast<const float*>(grad_out),
                                           static_cast<const float*>(coef), static_cast<float*>(output),
                                           static_cast<hipStream_t>(stream));
}

int voltrix_spmm_rel_dots_csr(void* indptr, void* indices, void* weight, int num_rows, int64_t num_entries, int embedding_dim,
                              int num_bases, void* grad_out, void* feat, int dtype, void* output, void* stream) {
  return voltrix::launch_spmm_rel_dots(static_cast<const int*>(indptr), static_cast<const int*>(indices),
                                       static_cast<const float*>(weight), num_rows, (long long)num_entries, embedding_dim, num_bases,
                                       static_cast<const float*>(grad_out), feat, dtype, static_cast<float*>(output),
                                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
