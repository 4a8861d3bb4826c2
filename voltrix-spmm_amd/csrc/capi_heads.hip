// libvoltrix_hip.so -- the multi-head forms of the three attention operators on a CSR pattern (include/voltrix_capi.h;
// voltrix/sddmm_heads_kernels.hpp, edge_softmax_heads_kernels.hpp, spmm_csr_heads_kernels.hpp): node tensors [n, heads, head_dim], edge
// tensors [nnz, heads] in CSR order with the head index fastest.
#include <hip/hip_runtime.h>

#include "voltrix/edge_softmax_heads_kernels.hpp"
#include "voltrix/sddmm_heads_kernels.hpp"
#include "voltrix/spmm_csr_heads_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_sddmm_heads_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, int head_dim, void* x, int x_dtype,
                                    void* y, int y_dtype, void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_sddmm_heads_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                                 (long long)nnz, heads, head_dim, x, x_dtype, y, y_dtype, static_cast<float*>(out),
                                                 static_cast<hipStream_t>(stream));
}

int64_t voltrix_edge_softmax_heads_workspace_bytes(int num_rows, int64_t nnz, int heads) {
  if (num_rows < 0 || nnz <= 0 || heads < 1) return 0;
  return (int64_t)voltrix::edge_softmax_heads_workspace_bytes((long long)nnz, heads);
}

void voltrix_launch_edge_softmax_heads_csr(void* indptr, int num_rows, int64_t nnz, int heads, void* scores, float scale, void* out,
                                           void* workspace, void* stream, int* return_code) {
  *return_code = voltrix::launch_edge_softmax_heads_csr(static_cast<const int*>(indptr), num_rows, (long long)nnz, heads,
                                                        static_cast<const float*>(scores), scale, static_cast<float*>(out), workspace,
                                                        static_cast<hipStream_t>(stream));
}

void voltrix_launch_edge_softmax_heads_backward_csr(void* indptr, int num_rows, int64_t nnz, int heads, void* alpha, void* grad_alpha,
                                                    float scale, void* grad_scores, void* workspace, void* stream, int* return_code) {
  *return_code = voltrix::launch_edge_softmax_heads_backward_csr(
      static_cast<const int*>(indptr), num_rows, (long long)nnz, heads, static_cast<const float*>(alpha),
      static_cast<const float*>(grad_alpha), scale, static_cast<float*>(grad_scores), workspace, static_cast<hipStream_t>(stream));
}

void voltrix_launch_spmm_csr_heads(void* indptr, void* indices, void* values, int num_rows, int heads, int head_dim, void* input,
                                   int dtype, void* output, void* stream, int* return_code) {
  *return_code = voltrix::launch_spmm_csr_heads(static_cast<const int*>(indptr), static_cast<const int*>(indices),
                                                static_cast<const float*>(values), num_rows, heads, head_dim, input, dtype,
                                                static_cast<float*>(output), static_cast<hipStream_t>(stream));
}

}  // extern "C"
