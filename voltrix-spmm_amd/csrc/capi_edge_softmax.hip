// libvoltrix_hip.so -- edge softmax on a CSR pattern and its backward (include/voltrix_capi.h; voltrix/edge_softmax_kernels.hpp):
// alpha[e] = softmax over row r of scale * scores, fp32 in CSR order; grad_scores = scale * alpha * (grad_alpha - rowsum(alpha * grad_alpha)).
#include <hip/hip_runtime.h>

#include "voltrix/edge_softmax_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

int64_t voltrix_edge_softmax_workspace_bytes(int num_rows, int64_t nnz) {
  if (num_rows < 0 || nnz <= 0) return 0;
  return (int64_t)voltrix::edge_softmax_workspace_bytes((long long)nnz);
}

void voltrix_launch_edge_softmax_csr(void* indptr, int num_rows, int64_t nnz, void* scores, float scale, void* out, void* workspace,
                                     void* stream, int* return_code) {
  *return_code = voltrix::launch_edge_softmax_csr(static_cast<const int*>(indptr), num_rows, (long long)nnz,
                                                  static_cast<const float*>(scores), scale, static_cast<float*>(out), workspace,
                                                  static_cast<hipStream_t>(stream));
}

void voltrix_launch_edge_softmax_backward_csr(void* indptr, int num_rows, int64_t nnz, void* alpha, void* grad_alpha, float scale,
                                              void* grad_scores, void* workspace, void* stream, int* return_code) {
  *return_code = voltrix::launch_edge_softmax_backward_csr(static_cast<const int*>(indptr), num_rows, (long long)nnz,
                                                           static_cast<const float*>(alpha), static_cast<const float*>(grad_alpha), scale,
                                                           static_cast<float*>(grad_scores), workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
