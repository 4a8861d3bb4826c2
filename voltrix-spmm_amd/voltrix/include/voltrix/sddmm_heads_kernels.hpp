// Voltrix-SpMM for MI355X (gfx950) -- multi-head sampled dense-dense product on a CSR pattern:
// out[e, h] = <x[row_e, h, :], y[indices[e], h, :]> for every entry e of the CSR and every head h; x [num_rows, H, D], y [*, H, D]
// (rows of H D), out [nnz, H] with the head index fastest.
//
// Why it exists.  Attention is multi-head in practice (GAT: 8 heads of 8; graph transformers: 4-8 heads of 16-64).  Looping
// sddmm_csr_kernel over the heads reads indptr / indices H times and gathers a D-wide slice per edge -- 16 bytes of a 128-byte line for
// D = 8 fp16 -- from a contiguous copy of every slice.  One edge's H scores belong together: one index read, one gathered row, H results.
//
// Shape.  sddmm_csr_kernel's, with the lane group cut into heads.  A head takes Lh = min(64, next_pow2(D / V)) lanes (V = 16 bytes of y);
// a group of G = next_pow2(heads_per_slab Lh) <= 64 lanes owns kSddmmChunkEdges consecutive edges, finds their rows with the same
// window of row ends, and gathers the whole slab of y[col] once per edge, 16 bytes per lane.  The xor butterfly stops at the head's Lh
// lanes and lane 0 of every head stores: the stores of one instruction cover the H consecutive floats of an edge.  Rows wider than 64
// pieces go out as slabs of whole heads (grid.y, 64 / Lh heads each); a head wider than 64 pieces is a slab of its own and its lanes
// walk ceil(D / (64 V)) pieces (R = 0).  R = 1 keeps the lane's piece of x[row] in registers until the row changes.
//
// Numerics.  Per head exactly sddmm_csr_kernel on the head's slice: the same lanes per head, the same fused multiply-adds in column
// order, the same butterfly -- out[:, h] has the BITS of the single-head kernel on contiguous x[:, h], y[:, h], duplicates included.
// |out - ref| <= D 2^-23 (|x| |y|)[e, h].  Element offsets e H + h and row H D are 64-bit.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "voltrix/sddmm_kernels.hpp"

namespace voltrix {

struct SddmmHeadsArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [nnz] column ids = rows of y
  const void* x;         // [num_rows, H, D] row-major, rows 16-byte aligned
  const void* y;         // [*, H, D]
  float* out;            // [nnz, H]
  int num_rows;
  int nnz;
  int heads;             // H
  int head_pieces;       // D / V
  int head_lanes;        // Lh: power of two <= 64
  int head_shift;        // log2(Lh)
  int head_rounds;       // pieces per lane: ceil(head_pieces / Lh)
  int slab_heads;        // heads per slab (grid.y): min(H, 64 / Lh)
  int lanes;             // G: power of two <= 64, >= slab_heads * Lh
  long long num_wgs;     // workgroups with chunks
  long long wgs_per_xcd; // ceil(num_wgs / 8): sizes the grid
};

// X, Y: float / _Float16 / bfloat16_bits.  R = 1: one piece per lane, x held in registers; 0: any number, x loaded per edge.
template <typename X, typename Y, int R>
static __global__ __launch_bounds__(256) void sddmm_heads_csr_kernel(const SddmmHeadsArgs a) {
  constexpr int V = 16 / (int)sizeof(Y);            // columns per piece
  constexpr int XW = (int)sizeof(X) * V / 16;       // 16-byte loads per piece of x: 1 or 2
  constexpr int U = 4;                              // edges in flight
  const int L = a.lanes;
  const long long wg = (long long)(blockIdx.x % kNumXcd) * a.wgs_per_xcd + blockIdx.x / kNumXcd;
  if (wg >= a.num_wgs) return;
  const long long chunk = wg * (256 / L) + (int)threadIdx.x / L;
  if (chunk * kSddmmChunkEdges >= a.nnz) return;    // the whole group leaves together
  const int e_begin = (int)(chunk * kSddmmChunkEdges);
  const int e_end = a.nnz - e_begin < kSddmmChunkEdges ? a.nnz : e_begin + kSddmmChunkEdges;
  const int lane = (int)threadIdx.x & (L - 1);
  const int group_base = ((int)threadIdx.x & 63) & ~(L - 1);
  const unsigned long long group_bits = L == 64 ? ~0ull : ((1ull << L) - 1);
  const int head_lane = lane & (a.head_lanes - 1);  // this lane's place among its head's lanes
  const int slab_head = lane >> a.head_shift;
  const int head = (int)blockIdx.y * a.slab_heads + slab_head;
  const bool live = slab_head < a.slab_heads && head < a.heads;   // lanes past the slab's heads only vote in row_of
  const long long F = (long long)a.heads * a.head_pieces * V;
  const long long head0 = (long long)head * a.head_pieces * V;    // first column of this lane's head
  const X* const x = static_cast<const X*>(a.x);
  const Y* const y = static_cast<const Y*>(a.y);

  // the row holding e_begin: the last r with indptr[r] <= e_begin (skips empty rows)
  int lo = 0, hi = a.num_rows;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (a.indptr[mid] <= e_begin) lo = mid;
    else hi = mid;
  }
  int window = lo;                                  // lane j holds the end of row window + j
  int bound = a.indptr[window + 1 + lane < a.num_rows ? window + 1 + lane : a.num_rows];
  auto row_of = [&](const int e) {
    while (true) {
      const int past = __popcll((__ballot(e >= bound) >> group_base) & group_bits);
      if (past < L) return window + past;
      window += L;
      bound = a.indptr[window + 1 + lane < a.num_rows ? window + 1 + lane : a.num_rows];
    }
  };

  float xc[V];                                      // x[cur_row, head], this lane's piece (R = 1)
#pragma unroll
  for (int i = 0; i < V; ++i) xc[i] = 0.0f;
  int cur_row = -1;

  for (int i = 0; i < e_end - e_begin; i += U) {     // counted: e + U may pass INT_MAX in the last chunk
    const int e = e_begin + i;
    int rows[U], cols[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ee = e + u < e_end ? e + u : e_end - 1;
      cols[u] = a.indices[ee];
      rows[u] = row_of(ee);
    }
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0f;
    if constexpr (R == 1) {
      const bool mine = live && head_lane < a.head_pieces;
      const long long k0 = head0 + (long long)head_lane * V;
      uint4_t yr[U], xr[U][XW];
      bool fresh[U];
#pragma unroll
      for (int u = 0; u < U; ++u) fresh[u] = rows[u] != (u == 0 ? cur_row : rows[u - 1]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        yr[u] = uint4_t{0u, 0u, 0u, 0u};
        if (mine) yr[u] = *reinterpret_cast<const uint4_t*>(y + (long long)cols[u] * F + k0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (fresh[u] && mine) {
#pragma unroll
          for (int w = 0; w < XW; ++w) xr[u][w] = reinterpret_cast<const uint4_t*>(x + (long long)rows[u] * F + k0)[w];
        }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (fresh[u] && mine) sddmm_to_float<X, XW>(xr[u], xc);
        float yv[V];
        sddmm_to_float<Y, 1>({yr[u]}, yv);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[u] = __builtin_fmaf(xc[i], yv[i], acc[u]);
      }
      cur_row = rows[U - 1];
    } else {
      for (int p = 0; p < a.head_rounds; ++p) {
        const int piece = head_lane + p * a.head_lanes;
        if (!live || piece >= a.head_pieces) break;   // lane-local: no cross-lane operation below
        const long long k0 = head0 + (long long)piece * V;
        uint4_t yr[U], xr[U][XW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          yr[u] = *reinterpret_cast<const uint4_t*>(y + (long long)cols[u] * F + k0);
#pragma unroll
          for (int w = 0; w < XW; ++w) xr[u][w] = reinterpret_cast<const uint4_t*>(x + (long long)rows[u] * F + k0)[w];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float xv[V], yv[V];
          sddmm_to_float<X, XW>(xr[u], xv);
          sddmm_to_float<Y, 1>({yr[u]}, yv);
#pragma unroll
          for (int i = 0; i < V; ++i) acc[u] = __builtin_fmaf(xv[i], yv[i], acc[u]);
        }
      }
    }
    // fixed-order butterfly over the head's lanes: lanes i and i ^ m add the same two numbers, so every lane of a head ends with the
    // same bits (a head's lanes are aligned to Lh: the xor stays inside the head)
    for (int m = 1; m < a.head_lanes; m <<= 1) {
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] += __shfl_xor(acc[u], m, 64);
    }
    if (head_lane == 0 && live) {                   // one lane per head: the H floats of an edge are consecutive
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (e + u < e_end) a.out[(long long)(e + u) * a.heads + head] = acc[u];
    }
  }
}

// dtype codes and pairs as launch_sddmm_csr.  head_dim % 8 == 0 when either operand is 16-bit, else head_dim % 4 == 0 (a head is a whole
// number of 16-byte pieces).  Every element of out[nnz, heads] is written.  Nothing is checked on the device: indptr must be a valid
// CSR of num_rows rows ending at nnz, and every index a row of y.
inline int launch_sddmm_heads_csr(const int* indptr, const int* indices, int num_rows, long long nnz, int heads, int head_dim,
                                  const void* x, int x_dtype, const void* y, int y_dtype, float* out, hipStream_t stream) {
  if (num_rows < 0 || nnz < 0 || head_dim < 0 || heads < 1 || nnz > INT_MAX || (long long)heads * head_dim > INT_MAX)
    return kErrBadShape;
  if (!sddmm_pair_ok(x_dtype, y_dtype)) return kErrBadShape;
  const int v = piece_elems(y_dtype);
  if (head_dim % v) return kErrBadShape;
  if (nnz == 0 || head_dim == 0) return kOk;
  if (num_rows == 0 || bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(x, 15) || bad_ptr(y, 15) || bad_ptr(out, 3))
    return kErrBadShape;
  const int pieces = head_dim / v;
  const EdgeChunkGrid g = edge_chunk_grid(nnz, heads, pieces, kSddmmChunkEdges);
  if (!g.ok) return kErrBadShape;
  const SddmmHeadsArgs a{indptr, indices, x, y, out, num_rows, (int)nnz, heads, pieces, g.head_lanes, g.head_shift, g.rounds,
                         g.slab_heads, g.lanes, g.wgs, g.per_xcd};
  const dim3 grid((unsigned)(g.per_xcd * kNumXcd), (unsigned)g.slabs);
  auto go = [&](auto xtag, auto ytag) {
    using X = decltype(xtag);
    using Y = decltype(ytag);
    if (g.rounds == 1) hipLaunchKernelGGL((sddmm_heads_csr_kernel<X, Y, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((sddmm_heads_csr_kernel<X, Y, 0>), grid, dim3(256), 0, stream, a);
  };
  dispatch_sddmm_pair(x_dtype, y_dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
