// libvoltrix_hip.so -- GAT edge scores on a CSR pattern and the segment sums of their backward (include/voltrix_capi.h;
// voltrix/gat_score_kernels.hpp): out[e, h] = leaky_relu(el[row_e, h] + er[indices[e], h], slope), fp32 [nnz, heads] in CSR order;
// out[r, h] = sum_{e in row r} gate(a[r, h] + b[indices[e], h]) grad[order ? order[e] : e, h].
#include <hip/hip_runtime.h>

#include "voltrix/gat_score_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

int64_t voltrix_gat_score_workspace_bytes(int num_rows, int64_t nnz, int heads) {
  if (num_rows < 0 || nnz <= 0 || heads < 1) return 0;
  return (int64_t)voltrix::gat_score_workspace_bytes((long long)nnz, heads);
}

void voltrix_launch_gat_score_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, void* el, void* er, float slope,
                                  void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_gat_score_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                               (long long)nnz, heads, static_cast<const float*>(el), static_cast<const float*>(er), slope,
                                               static_cast<float*>(out), static_cast<hipStream_t>(stream));
}

void voltrix_launch_gat_score_rowsum_csr(void* indptr, void* indices, void* order, int num_rows, int64_t nnz, int heads, void* a, void* b,
                                         void* grad, float slope, void* out, void* workspace, void* stream, int* return_code) {
  *return_code = voltrix::launch_gat_score_rowsum_csr(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), static_cast<const int*>(order), num_rows, (long long)nnz, heads,
      static_cast<const float*>(a), static_cast<const float*>(b), static_cast<const float*>(grad), slope, static_cast<float*>(out),
      workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
