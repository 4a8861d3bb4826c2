// libvoltrix_hip.so -- GATv2 edge scores on a CSR pattern and the gated row sum of their backward (include/voltrix_capi.h;
// voltrix/gatv2_score_kernels.hpp): out[e, h] = sum_d a[h, d] leaky_relu(xl[row_e, h, d] + xr[indices[e], h, d], slope), fp32 [nnz, heads]
// in CSR order; out[r, h, d] = sum_{e in row r} gate(p[r, h, d] + q[indices[e], h, d]) grad[order ? order[e] : e, h].
#include <hip/hip_runtime.h>

#include "voltrix/gatv2_score_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_gatv2_score_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, int head_dim, void* xl, void* xr,
                                    int dtype, void* a, float slope, void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_gatv2_score_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows,
                                                 (long long)nnz, heads, head_dim, xl, xr, dtype, static_cast<const float*>(a), slope,
                                                 static_cast<float*>(out), static_cast<hipStream_t>(stream));
}

void voltrix_launch_gatv2_rowsum_csr(void* indptr, void* indices, void* order, int num_rows, int64_t nnz, int heads, int head_dim, void* p,
                                     void* q, int dtype, void* grad, float slope, void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_gatv2_rowsum_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices),
                                                  static_cast<const int*>(order), num_rows, (long long)nnz, heads, head_dim, p, q, dtype,
                                                  static_cast<const float*>(grad), slope, static_cast<float*>(out),
                                                  static_cast<hipStream_t>(stream));
}

}  // extern "C"
