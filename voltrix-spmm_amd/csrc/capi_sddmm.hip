// libvoltrix_hip.so -- the sampled dense-dense product on a CSR pattern (include/voltrix_capi.h; voltrix/sddmm_kernels.hpp):
// out[e] = <x[row_e], y[indices[e]]>, fp32 / fp16 / bf16 operands, fp32 result in CSR order.
#include <hip/hip_runtime.h>

#include "voltrix/sddmm_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

void voltrix_launch_sddmm_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int embedding_dim, void* x, int x_dtype, void* y,
                              int y_dtype, void* out, void* stream, int* return_code) {
  *return_code = voltrix::launch_sddmm_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices), num_rows, (long long)nnz,
                                           embedding_dim, x, x_dtype, y, y_dtype, static_cast<float*>(out),
                                           static_cast<hipStream_t>(stream));
}

}  // extern "C"
