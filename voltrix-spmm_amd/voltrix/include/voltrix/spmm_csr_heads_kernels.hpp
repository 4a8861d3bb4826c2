// Voltrix-SpMM for MI355X (gfx950) -- multi-head aggregation straight from the CSR: out[r, h, :] = sum_{e in row r} v[e, h] feat[col_e, h, :]
// for feat [*, H, D] (rows of H D), v [nnz, H] fp32 with the head index fastest, out [num_rows, H, D] fp32.
//
// Why it exists.  It is the last step of a multi-head attention layer (scores: sddmm_heads_kernels.hpp, weights:
// edge_softmax_heads_kernels.hpp) and the backward of the multi-head SDDMM.  Through the single-head operators every head is a pass of
// its own at F = D: H reads of indptr / indices, H gathers of a D-wide slice, and -- on the block-format path -- the head's values
// scattered into the value planes of A and A^T first.  Here nothing is installed: the values are read where they are used.
//
// Shape.  The row-gather skeleton of csr_row_gather.hpp (V = 16 bytes of the operand, UNROLL = 4) over rows of H D elements, where a
// lane multiplies by the value of ITS head, piece / (D / V).  One indices read and one gathered row per edge serve all heads; the H
// values of an edge are 4 H consecutive bytes, read by every lane as the one float of its head (the lanes of a head share the address,
// the group shares the one or two 32-byte sectors).
//
// Numerics.  fp32 products, one fused multiply-add per element, summed in CSR edge order: out[:, h] has the BITS of
// spmm_csr_rows_kernel<T, 4, true> on the contiguous slices v[:, h], feat[:, h].  |out - ref| <= deg_r 2^-23 sum_e |v[e, h]| |feat[col_e, h, d]|.
// Offsets e H + h and row H D are 64-bit.
//
// Bound and known limit: the CUs' line-request rate / HBM; a row per lane group keeps the single-head kernel's weakness on hub rows (a
// hub row of a web graph serialises its wave).  Splitting hub rows with a fixed-order combine is the follow-up.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_csr_kernels.hpp"

namespace voltrix {

template <typename T>
struct CsrHeadsArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz] column ids = rows of `input`
  const T* input;       // [*, H, D] row-major, rows 16-byte aligned
  float* output;        // [num_rows, H, D]
  const float* values;  // [nnz, H] fp32 edge values in CSR order (duplicate entries add)
  int num_rows;
  int heads;            // H
  int head_pieces;      // D / V
  int F;                // H * D
  int lanes_per_row;    // power of two <= 64
  int groups_per_xcd;   // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
};

template <typename T, int UNROLL>
static __global__ __launch_bounds__(256) void spmm_csr_heads_kernel(const CsrHeadsArgs<T> a) {
  constexpr int V = 16 / (int)sizeof(T);
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;
  const long long H = a.heads;
  const float* const vals = a.values + p.piece / a.head_pieces;        // this lane's head: v[e, head] = vals[e H]
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  const T* const base = a.input + p.col0;
  const long long F = a.F;
  struct Slot {
    uint4_t raw;
    float v;
  };
  csr_for_each_batch<UNROLL, Slot>(
      a.indptr[p.row], a.indptr[p.row + 1],
      [&](Slot& s, const int ee) {
        s.raw = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F);
        s.v = vals[(long long)ee * H];
      },
      [&](const Slot& s, int, const bool live) {
        if (live) csr_accumulate_scaled<T>(acc, s.raw, s.v);
      });
  csr_store_piece(a.output + p.row * F + p.col0, acc);
}

// dtype: 0 fp32, 1 fp16, 2 bfloat16.  head_dim % (16 / sizeof(T)) == 0 (a head is a whole number of 16-byte pieces).  Every row of
// `output` is written (empty rows: zeros).  Nothing is checked on the device: indptr must be a valid CSR of num_rows rows whose last
// entry is the number of rows of `values`, and every index a row of `input`.
inline int launch_spmm_csr_heads(const int* indptr, const int* indices, const float* values, int num_rows, int heads, int head_dim,
                                 const void* input, int dtype, float* output, hipStream_t stream) {
  if (num_rows < 0 || head_dim < 0 || heads < 1 || dtype < 0 || dtype > 2 || (long long)heads * head_dim > INT_MAX) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (head_dim % v) return kErrBadShape;
  if (num_rows == 0 || head_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(values, 3) || bad_ptr(input, 15) || bad_ptr(output, 15)) return kErrBadShape;
  const int head_pieces = head_dim / v;
  const int pieces = heads * head_pieces;                // 16-byte pieces per row
  const RowGroupGrid g = row_group_grid(num_rows, pieces);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    const CsrHeadsArgs<T> a{indptr, indices, static_cast<const T*>(input), output, values, num_rows, heads, head_pieces,
                            heads * head_dim, g.lanes, (int)g.per_xcd};
    hipLaunchKernelGGL((spmm_csr_heads_kernel<T, 4>), grid, dim3(256), 0, stream, a);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
