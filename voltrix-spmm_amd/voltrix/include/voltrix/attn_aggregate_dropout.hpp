// Voltrix-SpMM for MI355X (gfx950) -- attn_aggregate with attention dropout: the launchers that instantiate the three kernels of
// attn_aggregate_kernels.hpp with DROP = true (the contract is in that header and in DESIGN.md 3.19).  Kept apart so that including
// attn_aggregate_kernels.hpp alone emits the kernels without a mask and nothing else.
#pragma once

#include "voltrix/attn_aggregate_kernels.hpp"

namespace voltrix {

// The same with attention dropout: mask = device int32 [nnz, ceil(heads / 32)] keep bits (dropout_mask_kernels.hpp), keep_scale = the
// factor of a kept entry (finite, >= 0).  m and l are those of the call without a mask; out = sum over the kept entries of
// alpha keep_scale feat.  With nnz == 0 the mask is not read.
inline int launch_attn_aggregate_dropout_csr(const int* indptr, const int* indices, const float* scores, int num_rows, long long nnz,
                                             int heads, int head_dim, const void* input, int dtype, float scale, float* output, float* m,
                                             float* l, const void* mask, float keep_scale, hipStream_t stream) {
  return launch_attn_aggregate_csr_impl<true>(indptr, indices, scores, num_rows, nnz, heads, head_dim, input, dtype, scale, output, m, l,
                                              mask, keep_scale, stream);
}

// The same with attention dropout: d_s[e, h] = scale alpha[e, h] (k[e, h] <grad_out[row_e, h], feat[indices[e], h]> - delta[row_e, h]),
// k = keep_scale where the mask's bit is set and 0 elsewhere; delta is the dense product with the dropped out.
inline int launch_attn_aggregate_dropout_grad_scores_csr(const int* indptr, const int* indices, int num_rows, long long nnz, int heads,
                                                         int head_dim, const float* grad_out, const void* feat, int dtype,
                                                         const float* scores, const float* m, const float* l, const float* delta,
                                                         float scale, float* out, const void* mask, float keep_scale,
                                                         hipStream_t stream) {
  return launch_attn_aggregate_grad_scores_csr_impl<true>(indptr, indices, num_rows, nnz, heads, head_dim, grad_out, feat, dtype, scores,
                                                          m, l, delta, scale, out, mask, keep_scale, stream);
}

// The same with attention dropout: the weight of entry e is alpha[order[e], h] k[order[e], h] -- the mask stays in CSR order.
inline int launch_attn_aggregate_dropout_grad_feat_csr(const int* t_indptr, const int* t_indices, const int* order, int num_rows,
                                                       long long nnz, int heads, int head_dim, const void* grad_out, int dtype,
                                                       const float* scores, const float* m, const float* l, float scale, float* out,
                                                       const void* mask, float keep_scale, hipStream_t stream) {
  return launch_attn_aggregate_grad_feat_csr_impl<true>(t_indptr, t_indices, order, num_rows, nnz, heads, head_dim, grad_out, dtype,
                                                        scores, m, l, scale, out, mask, keep_scale, stream);
}

}  // namespace voltrix
