// libvoltrix_hip.so -- FP8 (OCP e4m3fn) feature rows: the row-major quantiser and the aggregation that gathers such rows straight from
// the CSR (include/voltrix_capi.h; voltrix/spmm_fp8_kernels.hpp).  The two entry points RETURN their status code.
#include <hip/hip_runtime.h>

#include "voltrix/spmm_fp8_kernels.hpp"
#include "voltrix_capi.h"

extern "C" {

int voltrix_quantize_fp8_rows(void* input, int dtype, int num_rows, int embedding_dim, int64_t input_ld, void* inv_scale, void* output,
                              int64_t output_ld, void* stream) {
  return voltrix::launch_quantize_fp8_rows(input, dtype, num_rows, embedding_dim, (long long)input_ld,
                                           static_cast<const float*>(inv_scale), output, (long long)output_ld,
                                           static_cast<hipStream_t>(stream));
}

int voltrix_spmm_fp8_csr(void* indptr, void* indices, void* values, int num_rows, int embedding_dim16, void* input, void* scale,
                         void* output, int out_dtype, int xcd_ranges, int64_t num_entries, void* stream) {
  return voltrix::launch_spmm_fp8_csr(static_cast<const int*>(indptr), static_cast<const int*>(indices),
                                      static_cast<const float*>(values), num_rows, embedding_dim16, input,
                                      static_cast<const float*>(scale), output, out_dtype, xcd_ranges, (long long)num_entries,
                                      static_cast<hipStream_t>(stream));
}

}  // extern "C"
