// Voltrix-SpMM for MI355X (gfx950) -- what the launch_* host functions of the CSR / attention kernels share: the operand checks and the
// two launch geometries, and the dispatch over the operand's type.  Host code only: plain C++17, no HIP, nothing for the device.  The
// callers build their kernel arguments and their dim3 from the integers returned here -- the row-group grid through
// csr_row_gather.hpp's row_group_dim3, beside the device code that inverts it (tests/test_launch_geometry.py restates both formulas).
#pragma once

#include <cstdint>

#include "voltrix/traits.hpp"

namespace voltrix {

// elements per 16-byte piece of a row: dtype 0 fp32, 1 fp16, 2 bfloat16
inline int piece_elems(int dtype) { return dtype == 0 ? 4 : 8; }

// null, or not on the boundary `mask + 1`
inline bool bad_ptr(const void* p, uintptr_t mask) { return p == nullptr || ((uintptr_t)p & mask) != 0; }
// the same for a pointer that may be null
inline bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// Row-per-lane-group kernels (spmm_csr_heads, attn_aggregate forward and d_feat, gatv2_rowsum): a group of `lanes` = min(64,
// next_pow2(pieces)) lanes owns one row, grid.y walks `slabs` slabs of 64 pieces, a workgroup holds `rows_per_group` rows and XCD x owns
// the row groups [x per_xcd, (x + 1) per_xcd).  grid = (per_xcd * kNumXcd, slabs); !ok: a grid dimension would overflow.
struct RowGroupGrid {
  int lanes, slabs, rows_per_group;
  long long per_xcd;
  bool ok;
};

inline RowGroupGrid row_group_grid(int num_rows, int pieces) {
  const int slab_pieces = pieces < 64 ? pieces : 64;
  int lanes = 1;
  while (lanes < slab_pieces) lanes <<= 1;
  const int slabs = (pieces + 63) / 64;
  const int rows_per_group = 256 / lanes;
  const long long groups = ((long long)num_rows + rows_per_group - 1) / rows_per_group;
  const long long per_xcd = (groups + kNumXcd - 1) / kNumXcd;
  return {lanes, slabs, rows_per_group, per_xcd, !(per_xcd * kNumXcd > 0x7fffffffLL || slabs > 65535)};
}

// Kernels split by edges (sddmm, sddmm_heads, gatv2_score, attn_aggregate d_s): a head of `pieces` 16-byte pieces takes `head_lanes` =
// min(64, next_pow2(pieces)) = 1 << head_shift lanes for `rounds` pieces each, a lane group of `lanes` lanes holds `slab_heads` heads
// and `chunk_edges` consecutive edges, grid.y walks `slabs` slabs of heads; `wgs` workgroups hold chunks, `per_xcd` of them per XCD.
// grid = (per_xcd * kNumXcd, slabs); !ok: a grid dimension would overflow.
struct EdgeChunkGrid {
  int head_lanes, head_shift, rounds, slab_heads, lanes, slabs;
  long long wgs, per_xcd;
  bool ok;
};

inline EdgeChunkGrid edge_chunk_grid(long long nnz, int heads, int pieces, int chunk_edges) {
  int head_lanes = 1, head_shift = 0;
  while (head_lanes < pieces && head_lanes < 64) head_lanes <<= 1, ++head_shift;
  const int rounds = (pieces + head_lanes - 1) / head_lanes;
  const int slab_heads = heads < 64 / head_lanes ? heads : 64 / head_lanes;
  int lanes = head_lanes;
  while (lanes < slab_heads * head_lanes) lanes <<= 1;
  const int slabs = (heads + slab_heads - 1) / slab_heads;
  const long long chunks = (nnz + chunk_edges - 1) / chunk_edges;
  const long long groups_per_wg = 256 / lanes;
  const long long wgs = (chunks + groups_per_wg - 1) / groups_per_wg;
  const long long per_xcd = (wgs + kNumXcd - 1) / kNumXcd;
  return {head_lanes, head_shift, rounds, slab_heads, lanes, slabs, wgs, per_xcd, !(per_xcd * kNumXcd > 0x7fffffffLL || slabs > 65535)};
}

// ---- dispatch over the type tag of a dense operand: dtype 0 fp32, 1 fp16, 2 bfloat16 (the caller has checked the range).  fn gets a
// ---- value of the kernels' template argument: float, _Float16, or the bfloat16 storage type (spmm_kernels.hpp's bfloat16_bits).
template <class Fn>
inline void dispatch_feature_type(int dtype, Fn&& fn) {
  if (dtype == 0) fn(float{});
  else if (dtype == 1) fn(_Float16{});
  else fn(uint16_t{});
}

// the (x, y) operand pairs of the SDDMM kernels: (fp32, fp32 / fp16 / bf16), (fp16, fp16), (bf16, bf16)
inline bool sddmm_pair_ok(int x, int y) { return (x == 0 && (y == 0 || y == 1 || y == 2)) || (x == 1 && y == 1) || (x == 2 && y == 2); }

template <class Fn>
inline void dispatch_sddmm_pair(int x, int y, Fn&& fn) {
  if (x == 0 && y == 0) fn(float{}, float{});
  else if (x == 0 && y == 1) fn(float{}, _Float16{});
  else if (x == 0) fn(float{}, uint16_t{});
  else if (x == 1) fn(_Float16{}, _Float16{});
  else fn(uint16_t{}, uint16_t{});
}

}  // namespace voltrix
