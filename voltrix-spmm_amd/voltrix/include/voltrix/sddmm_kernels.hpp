// Voltrix-SpMM for MI355X (gfx950) -- sampled dense-dense product (SDDMM) on a CSR pattern: out[e] = <x[row_e], y[indices[e]]> for every
// entry e of the CSR, in CSR order.
//
// Why it exists.  It is the one operation a model that LEARNS its edge values needs beside the weighted SpMM: the gradient of C = csr(v) B
// with respect to the values is dv[e] = <dC[row_e], B[col_e]>, and dot-product attention scores are S[e] = <Q[row_e], K[col_e]>.  Its own
// backward is the weighted SpMM (spmm_csr_rows_kernel<T, 4, true> on the CSR and on its transpose).
//
// Shape.  Work is split by EDGES, not rows: every edge's output is independent (no sum over a row), so a hub row needs no combine and
// no atomics, and it cannot serialise a wave the way it does in the CSR row kernel.  A group of L = min(64, next_pow2(F / V)) lanes
// (V = 16 bytes of y: 4 fp32 or 8 fp16 / bf16 columns; x is read over the same V columns, 16 or 32 bytes) owns a chunk of
// kSddmmChunkEdges consecutive edges.  The chunk's first row is a binary search in indptr; the group then holds a window of L row
// ends (lane j: indptr[row + 1 + j]) and a row is the popcount of a ballot over it, so runs of short or empty rows cost no search.
// A lane keeps its F / (V L) pieces of x[row] in registers (R = 1 or 2; wider operands reload x per edge) and loads them again only
// when the row changes; it gathers 16 bytes of y[col] per piece, a batch of 4 edges in flight and a clamped tail like the CSR kernel.
// An xor butterfly over the L lanes finishes each edge and lane 0 of the group stores it.  Workgroup -> chunks: XCD x = blockIdx.x % 8
// owns a contiguous eighth of the chunks, so neighbouring rows, which share columns on band / community graphs, share an L2.
//
// Numerics.  x and y are converted to fp32 exactly; a lane sums x * y over its pieces in column order with one fused multiply-add per
// element, then the butterfly adds the L lane sums in a fixed order.  The result depends only on x[row_e], y[col_e] and F -- not on the
// edge's position or chunk: duplicate entries get identical bits, and two launches give identical bits.  |out - ref| <= F 2^-23 (|x| |y|)[e].
//
// Bound: the CUs' line-request rate / HBM, as for the CSR row kernel: one gathered row of y per edge ("SDDMM").
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_kernels.hpp"

namespace voltrix {

constexpr int kSddmmChunkEdges = 128;     // consecutive edges per lane group

struct SddmmArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [nnz] column ids = rows of y
  const void* x;         // [num_rows, F] row-major, rows 16-byte aligned
  const void* y;         // [*, F] row-major, rows 16-byte aligned
  float* out;            // [nnz]
  int num_rows;
  int nnz;
  int F;
  int pieces;            // F / V
  int lanes;             // L: power of two <= 64
  int rounds;            // pieces per lane: ceil(pieces / L)
  long long num_wgs;     // workgroups with chunks
  long long wgs_per_xcd; // ceil(num_wgs / 8): sizes the grid
};

// 16 * N bytes of T -> fp32 (exact)
template <typename T, int N>
__device__ __forceinline__ void sddmm_to_float(const uint4_t (&raw)[N], float (&v)[16 * N / sizeof(T)]) {
#pragma unroll
  for (int w = 0; w < N; ++w) {
    if constexpr (std::is_same<T, float>::value) {
      const float4_t f = __builtin_bit_cast(float4_t, raw[w]);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * w + i] = f[i];
    } else if constexpr (std::is_same<T, _Float16>::value) {
      const half8_t h = __builtin_bit_cast(half8_t, raw[w]);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[8 * w + i] = (float)h[i];
    } else {   // bfloat16 as bits: a 16-bit shift is the conversion
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[8 * w + 2 * i] = __builtin_bit_cast(float, raw[w][i] << 16);
        v[8 * w + 2 * i + 1] = __builtin_bit_cast(float, raw[w][i] & 0xffff0000u);
      }
    }
  }
}

// X, Y: float / _Float16 / bfloat16_bits.  R: pieces of x held in registers per lane (1 or 2); 0: any number, x loaded per edge.
template <typename X, typename Y, int R>
static __global__ __launch_bounds__(256) void sddmm_csr_kernel(const SddmmArgs a) {
  constexpr int V = 16 / (int)sizeof(Y);            // columns per piece
  constexpr int XW = (int)sizeof(X) * V / 16;       // 16-byte loads per piece of x: 1 or 2
  constexpr int U = 4;                              // edges in flight
  constexpr int RR = R > 0 ? R : 1;
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
  const long long F = a.F;
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

  float xc[RR][V];                                  // x[cur_row], this lane's pieces (R > 0)
#pragma unroll
  for (int p = 0; p < RR; ++p)
#pragma unroll
    for (int i = 0; i < V; ++i) xc[p][i] = 0.0f;
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
    if constexpr (R > 0) {
      uint4_t yr[R][U], xr[R][U][XW];
      bool fresh[U];
#pragma unroll
      for (int u = 0; u < U; ++u) fresh[u] = rows[u] != (u == 0 ? cur_row : rows[u - 1]);
#pragma unroll
      for (int p = 0; p < R; ++p) {
        const int piece = lane + p * L;
        const long long k0 = (long long)piece * V;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          yr[p][u] = uint4_t{0u, 0u, 0u, 0u};
          if (piece < a.pieces) yr[p][u] = *reinterpret_cast<const uint4_t*>(y + (long long)cols[u] * F + k0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (fresh[u] && piece < a.pieces) {
#pragma unroll
            for (int w = 0; w < XW; ++w)
              xr[p][u][w] = reinterpret_cast<const uint4_t*>(x + (long long)rows[u] * F + k0)[w];
          }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int p = 0; p < R; ++p) {
          if (fresh[u] && lane + p * L < a.pieces) sddmm_to_float<X, XW>(xr[p][u], xc[p]);
          float yv[V];
          sddmm_to_float<Y, 1>({yr[p][u]}, yv);
#pragma unroll
          for (int i = 0; i < V; ++i) acc[u] = __builtin_fmaf(xc[p][i], yv[i], acc[u]);
        }
      }
      cur_row = rows[U - 1];
    } else {
      for (int p = 0; p < a.rounds; ++p) {
        const int piece = lane + p * L;
        if (piece >= a.pieces) break;               // lane-local: no cross-lane operation below
        const long long k0 = (long long)piece * V;
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
    // fixed-order butterfly: lanes i and i ^ m add the same two numbers, so every lane ends with the same bits
    for (int m = 1; m < L; m <<= 1) {
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] += __shfl_xor(acc[u], m, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (e + u < e_end) a.out[e + u] = acc[u];
    }
  }
}

// dtype codes: 0 fp32, 1 fp16, 2 bfloat16.  Pairs (x, y): (fp32, fp16), (fp32, bf16), (fp16, fp16), (bf16, bf16), (fp32, fp32).
// F % 8 == 0 when either operand is 16-bit, else F % 4 == 0.  Every element of out[nnz] is written.  Nothing is checked on the device:
// indptr must be a valid CSR of num_rows rows ending at nnz, and every index a row of y.
inline int launch_sddmm_csr(const int* indptr, const int* indices, int num_rows, long long nnz, int embedding_dim, const void* x,
                            int x_dtype, const void* y, int y_dtype, float* out, hipStream_t stream) {
  if (num_rows < 0 || nnz < 0 || embedding_dim < 0 || nnz > INT_MAX) return kErrBadShape;
  if (!sddmm_pair_ok(x_dtype, y_dtype)) return kErrBadShape;
  const int v = piece_elems(y_dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (nnz == 0 || embedding_dim == 0) return kOk;
  if (num_rows == 0 || bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(x, 15) || bad_ptr(y, 15) || bad_ptr(out, 3))
    return kErrBadShape;
  const int pieces = embedding_dim / v;
  const EdgeChunkGrid g = edge_chunk_grid(nnz, 1, pieces, kSddmmChunkEdges);      // one head: one slab, lanes == head_lanes
  if (!g.ok) return kErrBadShape;
  const SddmmArgs a{indptr, indices, x, y, out, num_rows, (int)nnz, embedding_dim, pieces, g.lanes, g.rounds, g.wgs, g.per_xcd};
  const dim3 grid((unsigned)(g.per_xcd * kNumXcd));
  auto go = [&](auto xtag, auto ytag) {
    using X = decltype(xtag);
    using Y = decltype(ytag);
    if (g.rounds == 1) hipLaunchKernelGGL((sddmm_csr_kernel<X, Y, 1>), grid, dim3(256), 0, stream, a);
    else if (g.rounds == 2) hipLaunchKernelGGL((sddmm_csr_kernel<X, Y, 2>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((sddmm_csr_kernel<X, Y, 0>), grid, dim3(256), 0, stream, a);
  };
  dispatch_sddmm_pair(x_dtype, y_dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
