// Voltrix-SpMM for MI355X (gfx950) -- GATv2 edge scores on a CSR pattern and the gated row sum of their backward.
//
//   forward   z[e, h, d] = xl[row_e, h, d] + xr[col_e, h, d]                    (one fp32 add)
//             s[e, h]    = sum_d a[h, d] leaky(z[e, h, d]),  leaky(z) = z > 0 ? z : slope z   (z == 0 and NaN take the slope branch)
//   backward  G[r, h, d] = sum_{e in row r} gate(p[r, h, d] + q[indices[e], h, d]) g[order ? order[e] : e, h],  gate(z) = z > 0 ? 1 : slope
//
// Why it exists.  GATv2 (Brody et al.) puts the non-linearity inside the sum over d, so s is neither gat_score (per-node scalars) nor
// sddmm (a bilinear form); written in torch it materialises [nnz, H, D].  Here xl [num_rows, H, D], xr [num_cols, H, D] (one type:
// fp32 / fp16 / bf16), a [H, D] fp32, s [nnz, H] fp32 with the head index fastest, and nothing of size [nnz, H, D] exists in either
// direction.  From leaky(z) = gate(z) z:  d_xl = a G_l,  d_xr = a G_r,  d_a = sum_r xl G_l + sum_c xr G_r, with G_l the row sum on the
// CSR with (p, q) = (xl, xr) and G_r the row sum on the transposed CSR with (p, q) = (xr, xl) and order = the transposed edge order
// (int32); g is never permuted, and fp32 addition commutes, so the gate is the forward's decision to the bit on both sides.
//
// Forward (gatv2_score_csr_kernel).  sddmm_heads_csr_kernel's shape with a third operand.  A head takes Lh = min(64, next_pow2(D / V))
// lanes (V = 16 bytes of xr); a group of G = next_pow2(slab_heads Lh) <= 64 lanes owns kSddmmChunkEdges consecutive edges, finds their
// rows with the window of row ends, reads `indices` once per edge and gathers 16 bytes of xr[col] per lane.  R = 1 keeps the lane's
// piece of xl[row] in registers until the row changes and its piece of a[h] (V floats) for the whole kernel; R = 0 (a head above 64
// pieces) walks the pieces.  Slabs of whole heads go through grid.y; XCD x = blockIdx.x % 8 owns a contiguous eighth of the chunks.  The
// xor butterfly stops at Lh and lane 0 of every head stores: the H floats of an edge leave in one store instruction.
//
// Row sum (gatv2_rowsum_csr_kernel), one family for both sides.  The row-gather skeleton of csr_row_gather.hpp over rows of H D
// elements, UNROLL = 4.  The lane holds its piece of p[r] as floats, reads the one float g[., head] of its head and slope g once per
// edge, and adds z > 0 ? g : slope g in CSR edge order.  Every row of G is written (empty rows: +0); no workspace.
//
// Known limit.  A row per lane group keeps the weakness of spmm_csr_rows_kernel / spmm_csr_heads_kernel on hub rows: a hub row (or,
// for G_r, a hub column) serialises its wave.  Splitting hub rows with a fixed-order combine is the follow-up for this kernel and
// spmm_csr_heads_kernel together.
//
// Numerics (contraction off: the add, the product with slope and the select are separate operations).  Forward: per element one rounded
// add, one rounded product with float(slope) on the slope branch, one fused multiply-add into the lane's sum in column order, then the
// fixed butterfly:  |s - ref| <= (D + 2) 2^-23 sum_d |a_d| |leaky(z_d)| + 2^-149.  Per head the lanes, the order and the butterfly are
// those of the single-head call on the contiguous slices, so out[:, h] has its bits.  Row sum: every term is g or the one rounded
// product slope g, deg - 1 additions in CSR edge order:  |G - ref| <= deg 2^-23 sum_e |term_e| + 2^-149.  A NaN in xl[r, h, d] reaches
// only s[row r, h]; a NaN in g[e, h] only G[row_e, h, :].  No LDS, no scratch, no float atomics, no host synchronisation; offsets
// e H + h and row H D are 64-bit; the same inputs give the same bits on every launch.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "voltrix/csr_row_gather.hpp"
#include "voltrix/sddmm_kernels.hpp"

namespace voltrix {

struct Gatv2ScoreArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [nnz] column ids = rows of xr
  const void* xl;        // [num_rows, H, D] row-major, rows 16-byte aligned
  const void* xr;        // [*, H, D], the type of xl
  const float* a;        // [H, D]
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
  float slope;
  long long num_wgs;     // workgroups with chunks
  long long wgs_per_xcd; // ceil(num_wgs / 8): sizes the grid
};

__device__ __forceinline__ float gatv2_leaky(float z, float slope) { return z > 0.0f ? z : slope * z; }

// V consecutive floats from a 16-byte aligned address
template <int V>
__device__ __forceinline__ void gatv2_load_floats(const float* p, float (&v)[V]) {
#pragma unroll
  for (int w = 0; w < V / 4; ++w) {
    const float4_t f = reinterpret_cast<const float4_t*>(p)[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[4 * w + i] = f[i];
  }
}

// T: float / _Float16 / bfloat16_bits (xl and xr).  R = 1: one piece per lane, xl and a held in registers; 0: any number, loaded per edge.
template <typename T, int R>
static __global__ __launch_bounds__(256) void gatv2_score_csr_kernel(const Gatv2ScoreArgs a) {
#pragma clang fp contract(off)   // z, slope z and the select are separate operations; the one fused operation is the explicit fma
  constexpr int V = 16 / (int)sizeof(T);            // columns per piece
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
  const T* const xl = static_cast<const T*>(a.xl);
  const T* const xr = static_cast<const T*>(a.xr);
  const float slope = a.slope;

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

  float xc[V], ac[V];                               // xl[cur_row, head] and a[head], this lane's piece (R = 1)
#pragma unroll
  for (int i = 0; i < V; ++i) xc[i] = ac[i] = 0.0f;
  if constexpr (R == 1) {
    if (live && head_lane < a.head_pieces) gatv2_load_floats<V>(a.a + head0 + (long long)head_lane * V, ac);
  }
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
      uint4_t rr[U], lr[U][1];
      bool fresh[U];
#pragma unroll
      for (int u = 0; u < U; ++u) fresh[u] = rows[u] != (u == 0 ? cur_row : rows[u - 1]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        rr[u] = uint4_t{0u, 0u, 0u, 0u};
        if (mine) rr[u] = *reinterpret_cast<const uint4_t*>(xr + (long long)cols[u] * F + k0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (fresh[u] && mine) lr[u][0] = *reinterpret_cast<const uint4_t*>(xl + (long long)rows[u] * F + k0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (fresh[u] && mine) sddmm_to_float<T, 1>(lr[u], xc);
        float rv[V];
        sddmm_to_float<T, 1>({rr[u]}, rv);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[u] = __builtin_fmaf(ac[i], gatv2_leaky(xc[i] + rv[i], slope), acc[u]);
      }
      cur_row = rows[U - 1];
    } else {
      for (int p = 0; p < a.head_rounds; ++p) {
        const int piece = head_lane + p * a.head_lanes;
        if (!live || piece >= a.head_pieces) break;   // lane-local: no cross-lane operation below
        const long long k0 = head0 + (long long)piece * V;
        uint4_t rr[U], lr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          rr[u] = *reinterpret_cast<const uint4_t*>(xr + (long long)cols[u] * F + k0);
          lr[u] = *reinterpret_cast<const uint4_t*>(xl + (long long)rows[u] * F + k0);
        }
        float av[V];
        gatv2_load_floats<V>(a.a + k0, av);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float lv[V], rv[V];
          sddmm_to_float<T, 1>({lr[u]}, lv);
          sddmm_to_float<T, 1>({rr[u]}, rv);
#pragma unroll
          for (int i = 0; i < V; ++i) acc[u] = __builtin_fmaf(av[i], gatv2_leaky(lv[i] + rv[i], slope), acc[u]);
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

// dtype: 0 fp32, 1 fp16, 2 bfloat16 (xl and xr).  head_dim % (16 / sizeof(T)) == 0 (a head is a whole number of 16-byte pieces).  Every
// element of out[nnz, heads] is written.  Nothing is checked on the device: indptr must be a valid CSR of num_rows rows ending at nnz,
// and every index a row of xr.
inline int launch_gatv2_score_csr(const int* indptr, const int* indices, int num_rows, long long nnz, int heads, int head_dim,
                                  const void* xl, const void* xr, int dtype, const float* a, float slope, float* out,
                                  hipStream_t stream) {
  if (num_rows < 0 || nnz < 0 || head_dim < 0 || heads < 1 || nnz > INT_MAX || (long long)heads * head_dim > INT_MAX)
    return kErrBadShape;
  if (dtype < 0 || dtype > 2 || !std::isfinite(slope)) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (head_dim % v) return kErrBadShape;
  if (nnz == 0 || head_dim == 0) return kOk;
  if (num_rows == 0 || bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(xl, 15) || bad_ptr(xr, 15) || bad_ptr(a, 15) ||
      bad_ptr(out, 3))
    return kErrBadShape;
  const int pieces = head_dim / v;
  const EdgeChunkGrid grid_of = edge_chunk_grid(nnz, heads, pieces, kSddmmChunkEdges);
  if (!grid_of.ok) return kErrBadShape;
  const Gatv2ScoreArgs args{indptr, indices, xl, xr, a, out, num_rows, (int)nnz, heads, pieces, grid_of.head_lanes, grid_of.head_shift,
                            grid_of.rounds, grid_of.slab_heads, grid_of.lanes, slope, grid_of.wgs, grid_of.per_xcd};
  const dim3 grid((unsigned)(grid_of.per_xcd * kNumXcd), (unsigned)grid_of.slabs);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    if (grid_of.rounds == 1) hipLaunchKernelGGL((gatv2_score_csr_kernel<T, 1>), grid, dim3(256), 0, stream, args);
    else hipLaunchKernelGGL((gatv2_score_csr_kernel<T, 0>), grid, dim3(256), 0, stream, args);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

template <typename T>
struct Gatv2RowsumArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz] column ids = rows of q
  const int* order;     // [nnz] or null: g's edge of entry e
  const T* p;           // [num_rows, H, D] row-major, rows 16-byte aligned
  const T* q;           // [*, H, D]
  const float* g;       // [nnz, H]
  float* out;           // [num_rows, H, D]
  int num_rows;
  int heads;            // H
  int head_pieces;      // D / V
  int F;                // H * D
  int lanes_per_row;    // power of two <= 64
  int groups_per_xcd;   // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
  float slope;
};

template <typename T, int UNROLL>
static __global__ __launch_bounds__(256) void gatv2_rowsum_csr_kernel(const Gatv2RowsumArgs<T> a) {
#pragma clang fp contract(off)   // every term is g or the one rounded product slope g: no product fused into the sum
  constexpr int V = 16 / (int)sizeof(T);
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;
  const long long H = a.heads;
  const long long F = a.F;
  const float* const gh = a.g + p.piece / a.head_pieces;               // this lane's head: g[e, head] = gh[e H]
  const float slope = a.slope;
  float acc[V], pv[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  sddmm_to_float<T, 1>({*reinterpret_cast<const uint4_t*>(a.p + p.row * F + p.col0)}, pv);
  const T* const base = a.q + p.col0;
  struct Slot {
    uint4_t raw;
    float gv;
  };
  csr_for_each_batch<UNROLL, Slot>(
      a.indptr[p.row], a.indptr[p.row + 1],
      [&](Slot& s, const int ee) {
        s.raw = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F);
        s.gv = gh[(long long)(a.order != nullptr ? a.order[ee] : ee) * H];
      },
      [&](const Slot& s, int, const bool live) {
        if (live) {
          float qv[V];
          sddmm_to_float<T, 1>({s.raw}, qv);
          const float gs = slope * s.gv;                               // one rounded product per edge
#pragma unroll
          for (int i = 0; i < V; ++i) acc[i] += (pv[i] + qv[i] > 0.0f) ? s.gv : gs;
        }
      });
  csr_store_piece(a.out + p.row * F + p.col0, acc);
}

// dtype: 0 fp32, 1 fp16, 2 bfloat16 (p and q).  order: null, or int32 [nnz].  Every row of out[num_rows, heads, head_dim] is written
// (empty rows: zeros); with nnz == 0 every row is empty and indices, q and g are not read (they may be null).  Nothing is checked on the
// device: indptr must be a valid CSR of num_rows rows ending at nnz, every index a row of q and every order[e] a row of g.
inline int launch_gatv2_rowsum_csr(const int* indptr, const int* indices, const int* order, int num_rows, long long nnz, int heads,
                                   int head_dim, const void* p, const void* q, int dtype, const float* g, float slope, float* out,
                                   hipStream_t stream) {
  if (num_rows < 0 || nnz < 0 || head_dim < 0 || heads < 1 || nnz > INT_MAX || (long long)heads * head_dim > INT_MAX)
    return kErrBadShape;
  if (dtype < 0 || dtype > 2 || !std::isfinite(slope)) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (head_dim % v) return kErrBadShape;
  if (nnz > 0 && num_rows == 0) return kErrBadShape;
  if (num_rows == 0 || head_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(p, 15) || bad_ptr(out, 15)) return kErrBadShape;
  if (nnz > 0 && (indices == nullptr || q == nullptr || g == nullptr)) return kErrBadShape;
  if (misaligned(indices, 3) || misaligned(order, 3) || misaligned(q, 15) || misaligned(g, 3)) return kErrBadShape;
  const int head_pieces = head_dim / v;
  const int pieces = heads * head_pieces;                // 16-byte pieces per row
  const RowGroupGrid grid_of = row_group_grid(num_rows, pieces);
  if (!grid_of.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(grid_of);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    const Gatv2RowsumArgs<T> args{indptr, indices, order, static_cast<const T*>(p), static_cast<const T*>(q), g, out, num_rows, heads,
                                  head_pieces, heads * head_dim, grid_of.lanes, (int)grid_of.per_xcd, slope};
    hipLaunchKernelGGL((gatv2_rowsum_csr_kernel<T, 4>), grid, dim3(256), 0, stream, args);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
