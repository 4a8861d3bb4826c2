// libvoltrix_hip.so -- attention dropout (include/voltrix_capi.h): the packed keep mask's generator (voltrix/dropout_mask_kernels.hpp)
// and the three launches of attn_aggregate with a mask (voltrix/attn_aggregate_dropout.hpp: attn_aggregate_kernels.hpp with DROP = true): m and l stay those of the
// undropped softmax, a kept entry weighs alpha * keep_scale, a dropped entry's operand row is not read.
#include <hip/hip_runtime.h>

#include "voltrix/attn_aggregate_dropout.hpp"
#include "voltrix/dropout_mask_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_dropout_mask(int64_t nnz, int heads, uint32_t threshold, uint64_t seed, uint64_t offset, void* mask, void* stream,
                                 int* return_code) {
  *return_code = voltrix::launch_dropout_mask((long long)nnz, heads, threshold, seed, offset, mask, static_cast<hipStream_t>(stream));
}

void voltrix_launch_attn_aggregate_dropout_csr(void* indptr, void* indices, void* scores, int num_rows, int64_t nnz, int heads,
                                               int head_dim, void* feat, int dtype, float scale, void* out, void* m, void* l, void* mask,
                                               float keep_scale, void* stream, int* return_code) {
  *return_code = voltrix::launch_attn_aggregate_dropout_csr(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), static_cast<const float*>(scores), num_rows, (long long)nnz,
      heads, head_dim, feat, dtype, scale, static_cast<float*>(out), static_cast<float*>(m), static_cast<float*>(l), mask, keep_scale,
      static_cast<hipStream_t>(stream));
}

void voltrix_launch_attn_aggregate_dropout_grad_scores_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads,
                                                           int head_dim, void* grad_out, void* feat, int dtype, void* scores, void* m,
                                                           void* l, void* delta, float scale, void* grad_scores, void* mask,
                                                           float keep_scale, void* stream, int* return_code) {
  *return_code = voltrix::launch_attn_aggregate_dropout_grad_scores_csr(
      static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, (long long)nnz, heads, head_dim,
      static_cast<const float*>(grad_out), feat, dtype, static_cast<const float*>(scores), static_cast<const float*>(m),
      static_cast<const float*>(l), static_cast<const float*>(delta), scale, static_cast<float*>(grad_scores), mask, keep_scale,
      static_cast<hipStream_t>(stream));
}

void voltrix_launch_attn_aggregate_dropout_grad_feat_csr(void* t_indptr, void* t_indices, void* order, int num_cols, int64_t nnz,
                                                         int heads, int head_dim, void* grad_out, int dtype, void* scores, void* m,
                                                         void* l, float scale, void* grad_feat, void* mask, float keep_scale,
                                                         void* stream, int* return_code) {
  *return_code = voltrix::launch_attn_aggregate_dropout_grad_feat_csr(
      static_cast<const int*>(t_indptr), static_cast<const int*>(t_indices), static_cast<const int*>(order), num_cols, (long long)nnz,
      heads, head_dim, grad_out, dtype, static_cast<const float*>(scores), static_cast<const float*>(m), static_cast<const float*>(l),
      scale, static_cast<float*>(grad_feat), mask, keep_scale, static_cast<hipStream_t>(stream));
}

}  // extern "C"
