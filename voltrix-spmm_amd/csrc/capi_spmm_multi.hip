// libvoltrix_hip.so -- sum / mean / max / min / var / std of every row's neighbours from one gather of the CSR, and their joint
// backward on the transposed CSR (include/voltrix_capi.h; voltrix/spmm_multi_kernels.hpp).  The two entry points RETURN their status
// code.
#include <hip/hip_runtime.h>

#include "voltrix/spmm_multi_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

int voltrix_spmm_multi_csr(void* indptr, void* indices, int num_rows, int64_t num_entries, int embedding_dim, void* input, int dtype,
                           int slot_sum, int slot_mean, int slot_max, int slot_min, int slot_var, int slot_std, int num_slots,
                           float eps, void* output, void* argmax, void* argmin, void* stream) {
  const int slots[voltrix::kMultiAggregates] = {slot_sum, slot_mean, slot_max, slot_min, slot_var, slot_std};
  return voltrix::launch_spmm_multi(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, (long long)num_entries,
                                    embedding_dim, input, dtype, slots, num_slots, eps, static_cast<float*>(output),
                                    static_cast<int*>(argmax), static_cast<int*>(argmin), static_cast<hipStream_t>(stream));
}

int voltrix_spmm_multi_backward_csr(void* t_indptr, void* t_indices, void* t_order, int num_cols, int64_t num_entries, int embedding_dim,
                                    void* x, void* u, void* w, void* mean, int64_t mean_ld, void* g_max, void* argmax, void* g_min,
                                    void* argmin, void* output, void* stream) {
  return voltrix::launch_spmm_multi_backward(
      static_cast<const int*>(t_indptr), static_cast<const int*>(t_indices), static_cast<const int*>(t_order), num_cols,
      (long long)num_entries, embedding_dim, static_cast<const float*>(x), static_cast<const float*>(u), static_cast<const float*>(w),
      static_cast<const float*>(mean), (long long)mean_ld, static_cast<const float*>(g_max), static_cast<const int*>(argmax),
      static_cast<const float*>(g_min), static_cast<const int*>(argmin), static_cast<float*>(output), static_cast<hipStream_t>(stream));
}

}  // extern "C"
