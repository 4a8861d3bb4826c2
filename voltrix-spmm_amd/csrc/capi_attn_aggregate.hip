// libvoltrix_hip.so -- edge softmax and multi-head aggregation in one launch on a CSR pattern, and the two launches of its backward
// (include/voltrix_capi.h; voltrix/attn_aggregate_kernels.hpp): out[r, h, :] = sum_{e in row r} alpha[e, h] feat[indices[e], h, :] with
// alpha the row softmax of scale * scores, never stored; d_s and d_feat recompute it from scores and the row statistics m and l.
#include <hip/hip_runtime.h>

#include "voltrix/attn_aggregate_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_attn_aggregate_csr(void* indptr, void* indices, void* scores, int num_rows, int64_t nnz, int heads, int head_dim,
                                       void* feat, int dtype, float scale, void* out, void* m, void* l, void* stream, int* return_code) {
  *return_code = voltrix::launch_attn_aggregate_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices),
                                                    static_cast<const float*>(scores), num_rows, (long long)nnz, heads, head_dim, feat,
                                                    dtype, scale, static_cast<float*>(out), static_cast<float*>(m),
                                                    static_cast<float*>(l), static_cast<hipStream_t>(stream));
}

void voltrix_launch_attn_aggregate_grad_scores_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, int head_dim,
                                                   void* grad_out, void* feat, int dtype, void* scores, void* m, void* l, void* delta,
                                                   float scale, void* grad_scores, void* stream, int* return_code) {
  *return_code = voltrix::launch_attn_aggregate_grad_scores_csr(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, (long long)nnz, heads, head_dim,
      static_cast<const float*>(grad_out), feat, dtype, static_cast<const float*>(scores), static_cast<const float*>(m),
      static_cast<const float*>(l), static_cast<const float*>(delta), scale, static_cast<float*>(grad_scores),
      static_cast<hipStream_t>(stream));
}

void voltrix_launch_attn_aggregate_grad_feat_csr(void* t_indptr, void* t_indices, void* order, int num_cols, int64_t nnz, int heads,
                                                 int head_dim, void* grad_out, int dtype, void* scores, void* m, void* l, float scale,
                                                 void* grad_feat, void* stream, int* return_code) {
  *return_code = voltrix::launch_attn_aggregate_grad_feat_csr(
      static_cast<const int*>(t_indptr), static_cast<const int*>(t_indices), static_cast<const int*>(order), num_cols, (long long)nnz,
      heads, head_dim, grad_out, dtype, static_cast<const float*>(scores), static_cast<const float*>(m), static_cast<const float*>(l),
      scale, static_cast<float*>(grad_feat), static_cast<hipStream_t>(stream));
}

}  // extern "C"
