// Voltrix-SpMM for MI355X (gfx950) -- the skeleton the row-per-lane-group CSR kernels share: which row and which 16 bytes of it a lane
// owns (csr_lane_place, the device half of launch_geometry.hpp's row_group_grid), the batch loop over a row's entries
// (csr_for_each_batch), and the 16-byte piece helpers (to fp32, accumulate, store).  Device code, and the one host line that turns a
// RowGroupGrid into the dim3 csr_lane_place inverts.  What a kernel does with an entry -- its operator, its numerics, its bounds -- is
// its own header's business; DESIGN.md 3.32 lists which kernels take both halves and which only the prologue.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_kernels.hpp"

namespace voltrix {

// grid = (per_xcd * kNumXcd, slabs, z): z is 1 but for a kernel that walks a third axis of its own (spmm_rel_kernel's basis tiles)
inline dim3 row_group_dim3(const RowGroupGrid& g, unsigned z = 1) { return dim3((unsigned)(g.per_xcd * kNumXcd), (unsigned)g.slabs, z); }

// ---- the lane's place ------------------------------------------------------------------------------------------------------------------
// A group of L = lanes_per_row = min(64, next_pow2(slab pieces)) lanes owns one row, a 256-thread workgroup 256 / L consecutive rows (a
// row group), grid.y walks column slabs of 64 pieces; a lane owns one piece -- V elements, 16 bytes of the gathered operand -- of the
// row and of every row gathered for it.  XCD x = blockIdx.x % 8 owns the row groups [x groups_per_xcd, (x + 1) groups_per_xcd):
// neighbouring rows, which reference neighbouring rows of B on band / community graphs, share an L2.  Equal or better than workgroup
// b = row group b (consecutive groups going round the XCDs) on every graph measured: amazon0505-like x 128 fp32 0.297 -> 0.256 ms,
// ppi-like x 512 0.166 -> 0.111.  xcd_ranges = false is that round-robin order, kept for the two entry points whose C signature
// carries the switch.
struct CsrLanePlace {
  long long row;    // of the CSR at hand
  long long col0;   // the lane's first element of a row: piece * V
  int piece;        // the lane's 16-byte piece of a row; piece / (pieces per head) is its head
  bool work;        // false: the row or the piece does not exist, the lane leaves
};

template <int V>
__device__ __forceinline__ CsrLanePlace csr_lane_place(const int lanes_per_row, const int groups_per_xcd, const int num_rows,
                                                       const long long F, const bool xcd_ranges = true) {
  const int rows_per_group = 256 / lanes_per_row;
  const long long group = xcd_ranges ? (long long)(blockIdx.x % kNumXcd) * groups_per_xcd + blockIdx.x / kNumXcd : (long long)blockIdx.x;
  const long long row = group * rows_per_group + (int)threadIdx.x / lanes_per_row;
  const int lane = (int)threadIdx.x & (lanes_per_row - 1);
  const long long col0 = ((long long)blockIdx.y * 64 + lane) * V;
  return {row, col0, (int)blockIdx.y * 64 + lane, row < num_rows && col0 < F};
}

// ---- the batch loop --------------------------------------------------------------------------------------------------------------------
// The entries [e, end) of a row in batches of UNROLL: full batches, then ONE more batch for the tail whose surplus slots read the
// row's last entry (ids clamped to end - 1).  Every issue of a batch -- unconditional loads into a Slot -- comes before its first
// consume.  consume(slot, entry, live) runs in entry order; live is the constant true in a full batch and false for a surplus slot of
// the tail: an accumulating kernel writes `if (live)`, a selecting kernel makes it part of its predicate (csr_select), so the tail has
// no branch around its selects.  Why this shape: at mean degree 5 a row is one or two batches with all their loads in flight.  A scalar
// tail loop ran most rows of such graphs one load at a time; a tail whose LOADS were predicated serialised them (ppi-like x 128:
// 0.150 ms against 0.091; profiles/r06/experiment_csr_mapping.log).
template <int UNROLL, class Slot, class Issue, class Consume>
__device__ __forceinline__ void csr_for_each_batch(int e, const int end, Issue&& issue, Consume&& consume) {
  for (; end - e >= UNROLL; e += UNROLL) {
    Slot slot[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) issue(slot[u], e + u);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) consume(slot[u], e + u, true);
  }
  if (e < end) {
    Slot slot[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) issue(slot[u], u < end - e ? e + u : end - 1);
    // No instruction: a line the loads may not cross.  Without it the compiler sinks a slot's load into the `live` branch of its
    // consume, where it waits alone behind its own id -- the predicated tail of the measurement above (seen with ROCm's clang in
    // spmm_csr_rows_kernel<float>: 0.1965 ms against 0.1906 on amazon0601-like x 128).  No test sees this: with another compiler,
    // read the tail's ISA again -- every id and every row load of the batch must stand before its first add or select
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) consume(slot[u], e + u, u < end - e);
  }
}

// ---- 16-byte pieces --------------------------------------------------------------------------------------------------------------------
// the 16 bytes of a lane as fp32 (exact for every T)
template <typename T>
__device__ __forceinline__ void csr_piece_as_float(float (&v)[16 / sizeof(T)], const uint4_t raw) {
  if constexpr (std::is_same<T, float>::value) {
    const float4_t x = __builtin_bit_cast(float4_t, raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = x[i];
  } else if constexpr (std::is_same<T, _Float16>::value) {
    const half8_t x = __builtin_bit_cast(half8_t, raw);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
  } else {   // bfloat16 as bits: a 16-bit shift is the conversion
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __builtin_bit_cast(float, raw[i] << 16);
      v[2 * i + 1] = __builtin_bit_cast(float, raw[i] & 0xffff0000u);
    }
  }
}

// acc += row piece: fp32 additions
template <typename T>
__device__ __forceinline__ void csr_accumulate(float (&acc)[16 / sizeof(T)], const uint4_t raw) {
  float x[16 / sizeof(T)];
  csr_piece_as_float<T>(x, raw);
#pragma unroll
  for (int i = 0; i < 16 / (int)sizeof(T); ++i) acc[i] += x[i];
}

// acc += v * row piece: one fused multiply-add per element, a single fp32 rounding
template <typename T>
__device__ __forceinline__ void csr_accumulate_scaled(float (&acc)[16 / sizeof(T)], const uint4_t raw, const float v) {
  float x[16 / sizeof(T)];
  csr_piece_as_float<T>(x, raw);
#pragma unroll
  for (int i = 0; i < 16 / (int)sizeof(T); ++i) acc[i] = __builtin_fmaf(v, x[i], acc[i]);
}

// a lane's V results (float or int) to 16-byte aligned `to`, as 16-byte pieces
template <typename E, int V>
__device__ __forceinline__ void csr_store_piece(E* const to, const E (&r)[V]) {
  static_assert((std::is_same<E, float>::value || std::is_same<E, int>::value) && V % 4 == 0, "whole 16-byte pieces");
  using vec4_t = typename std::conditional<std::is_same<E, float>::value, float4_t, int4_t>::type;
#pragma unroll
  for (int i = 0; i < V / 4; ++i) reinterpret_cast<vec4_t*>(to)[i] = vec4_t{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
}

}  // namespace voltrix
