// Voltrix-SpMM for MI355X (gfx950) -- relational (R-GCN) aggregation over TYPED edges with basis decomposition, and its two gradients:
//   out[i, b, f] = sum over the entries e of row i of c(e, b) * feat[col_e, f]            c(e, b) = w_e * coef[etype_e, b]
//   dF[c, f]     = sum over the entries e of column c, over b, of c(e, b) * g[row_e, b, f]  (spmm_rel_contract_kernel on the transpose)
//   s[e, b]      = w_e * <g[row_e, b, :], feat[col_e, :]>                                   (spmm_rel_dots_kernel; dC[r, b] = sum of
//                                                                                           s[e, b] over the entries of type r)
// h' = out.view(n, B F) @ V.view(B F, F_out) is then R-GCN's sum_r sum_{j in N_r(i)} 1 / c_{i,r} W_r h_j with W_r = sum_b coef[r, b] V_b
// (Schlichtkrull et al.).  With coef = I_R the same kernel gives the plain per-relation sums [n, R, F].
//
// Semantics.  indptr / indices: int32 CSR of [num_rows, num_cols], rectangular patterns and duplicate entries allowed.  etype: int32
// [nnz] in CSR entry order, 0 <= etype < R (for a sampled block: etype[block.entries]).  feat: [num_cols, F] fp32 / fp16 / bf16, read
// as stored.  coef: fp32 [R, B_pad], B_pad = B rounded up to 4 (whole 16-byte pieces per row; the padding is read and ignored).
// weight: fp32 [nnz] or NULL (the normaliser 1 / c_{i,r}; NULL: 1, c(e, b) is coef itself).  Outputs are fp32, every element written; a
// row without entries gives 0; a type without entries gets a zero gradient.  weight has no gradient.  fp32 throughout: c(e, b) is one
// rounded product, every term one more (or one fused multiply-add), sums in a fixed order -- CSR order per row in the forward; per column
// the transposed CSR's entries in batches of 4, inside a batch basis tile by basis tile, inside a tile entry by entry, basis by basis;
// per dot the lane's pieces slab by slab, then a butterfly over the group.  No float atomics, the same bits on every call; NaN and inf
// propagate as the arithmetic does.  |out - ref| <= (k + 2) 2^-23 sum |terms| for the k entries of a row; dF: (k B + 2); dC: (m_r + F +
// 2) for the m_r entries of type r.
//
// Geometry: the lane's place of csr_row_gather.hpp.  The loops are these kernels' own -- a single loop whose every batch clamps its
// ids to the row's last entry, every load issued before the first is consumed, surplus slots skipped -- with UNROLL = 4.  Offsets
// row B F, col F and e B_pad are 64-bit.
//
// Forward, spmm_rel_kernel<T, BT>.  A lane owns V = 16 / sizeof(T) features and BT x V fp32 accumulators for a tile of BT bases.  Per
// entry: one 16-byte load of feat[col], one etype read (and the weight read), and BT / 4 16-byte loads of that type's row of coef.
// grid.z walks the basis tiles when B > BT: THE GATHERED ROW IS READ AGAIN PER TILE (from L2 after the first).  The loop over the tile
// is unrolled under the wave-uniform predicate b < B: no accumulator is indexed at run time, nothing goes to scratch.  BT is 4 for
// B <= 4 and 8 (kRelBasisTile) beyond.  The compiler's report (profiles/spmm_rel/resource_usage.txt): the 4-tile takes 66 VGPRs for
// fp32 and 84 for 16-bit features (7 and 5 waves per SIMD), the 8-tile 98 and 132 (4 and 3 waves; 64 accumulators for 16-bit); a
// 16-tile would take 128 accumulators alone (not built).  Nothing spills.  Measured (harness/experiments/exp_spmm_rel_table.py,
// VOLTRIX_SPMM_REL_TILE = 4 against 8 at (R, B) = (46, 8) and (46, 30)): the 4-tile for every B is 0.99-1.16 times the
// 8-tile's time -- equal at F = 32, B = 8, 7-16 % slower at F = 128 -- for all its extra waves: the second read of the gathered rows
// costs more than the occupancy brings.  8 stays.
//
// How the R x B table reaches the lanes: plain loads.  The lanes of a group share the address (a broadcast inside the texture path),
// the table is R B_pad 4 bytes (46 x 32: 5.9 KB) and stays in L1 / L2, and the loads are issued with the batch's gathers, so their
// latency hides behind the same wait.  A copy in LDS (VOLTRIX_SPMM_REL_COEF_LDS = 1: every workgroup copies the table first, one
// barrier, tables of at most 32 KB) was measured by the same experiment: 0.99-1.08 times the plain loads' time, within 1.5 % at nine of
// twelve points and 2-8 % slower at the other three (fp32 features on amazon0601-like).  Nothing to win, a cap on R B and a barrier: the loads
// stay plain, and the switch remains for the experiment alone.
//
// Contract, spmm_rel_contract_kernel<BT> (grad_feat): on the transposed CSR, a lane group owns a column, a lane 4 fp32 features.
// Per entry it reads etype[order[e]] (and weight[order[e]]) through the nullable `order` indirection (t_order; NULL: e itself), gathers
// the B pieces g[row_e, b, piece] (fp32, stride F) and adds sum_b c(e, b) g into one accumulator piece.  Tiles of BT = 4 bases are
// walked INSIDE the kernel (the output has no basis axis): 4 entries x 4 bases x 16 bytes are in flight per lane.
//
// Dots, spmm_rel_dots_kernel<T>: row-parallel, the same groups; s is fp32 [nnz, B_pad], the padding written as 0.  Per tile of 4 bases
// (one 16-byte piece of s[e]; a tile of 8 took 214 VGPRs and spilled SGPRs) the group keeps its piece of g[row, b, :] in registers,
// gathers feat[col] per entry, and reduces every basis across the group with a butterfly of xor shuffles under constant masks (DPP / swizzles where the compiler finds them).  For F beyond one slab it loops over
// the slabs inside the kernel (g is then read again per batch and slab); it does not split over grid.y, which would need a combine.
// Lane 0 of the group writes 16-byte pieces of s[e].  dC is then two fixed-order sums of rows of s by voltrix_launch_spmm_csr_rows on
// tables built once (voltrix/spmm_rel.py::TypeIndex): chunks of at most CHUNK entries of one type, then a type's chunks in order.
//
// Bound: the CUs' line-request rate / L2 for the gathered rows, HBM for the [n, B, F] output (forward) or grad_out (contract).  Known
// limit: a hub row (contract: a hub column) serialises its wave, like spmm_csr_heads.  Nothing is checked on the device.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_csr_reduce_kernels.hpp"

// The two measured choices of the forward kernel, as switches of harness/experiments/exp_spmm_rel_table.py
#ifndef VOLTRIX_SPMM_REL_TILE
#define VOLTRIX_SPMM_REL_TILE 8           // the forward's largest tile of bases: 8, or 4 (one kernel for every B)
#endif
#ifndef VOLTRIX_SPMM_REL_COEF_LDS
#define VOLTRIX_SPMM_REL_COEF_LDS 0       // 1: every workgroup copies the coefficient table into LDS first (tables of at most 32 KB)
#endif

namespace voltrix {

constexpr int kRelBasisTile = VOLTRIX_SPMM_REL_TILE;      // voltrix.spmm_rel.BASIS_TILE
constexpr int kRelLdsFloats = 8192;                       // the LDS copy of the experiment: 32 KB
static_assert(kRelBasisTile == 8 || kRelBasisTile == 4, "tile");
constexpr int kRelContractTile = 4;
constexpr int kRelDotsTile = 4;
constexpr int kRelMaxTypes = 65536;       // num_types: 1 .. 65 536
constexpr int kRelMaxBases = 1024;        // num_bases: 0 .. 1 024

inline int rel_padded_bases(int num_bases) { return (num_bases + 3) / 4 * 4; }

template <typename T>
struct SpmmRelArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [nnz] column ids = rows of `input`
  const int* etype;      // [nnz]
  const float* weight;   // [nnz] or NULL
  const T* input;        // [*, F]
  const float* coef;     // [R, B_pad]
  float* output;         // [num_rows, B, F]
  int num_rows;
  int F;
  int B;
  int B_pad;
  int lanes_per_row;     // power of two <= 64
  int groups_per_xcd;    // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
  int table_pieces;      // R * B_pad / 4: the 16-byte pieces of coef (read by the LDS build alone)
};

template <typename T, int BT, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_rel_kernel(const SpmmRelArgs<T> a) {
  static_assert(BT % 4 == 0, "whole 16-byte pieces of a row of coef");
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int NC = BT / 4;
#if VOLTRIX_SPMM_REL_COEF_LDS
  __shared__ float4_t table[kRelLdsFloats / 4];                       // before any thread leaves: all 256 copy, then one barrier
  for (int i = (int)threadIdx.x; i < a.table_pieces; i += 256) table[i] = reinterpret_cast<const float4_t*>(a.coef)[i];
  __syncthreads();
#endif
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);   // a lane: V features
  if (!p.work) return;
  const long long row = p.row, col0 = p.col0;
  const long long F = a.F;
  const int b0 = (int)blockIdx.z * BT;
  const int live = a.B - b0 < BT ? a.B - b0 : BT;                    // bases of this tile; wave-uniform
  int coff[NC];                                                       // the tile's pieces of a row of coef, clamped into the row
#pragma unroll
  for (int j = 0; j < NC; ++j) coff[j] = b0 + 4 * j < a.B_pad - 4 ? b0 + 4 * j : a.B_pad - 4;
  int e = a.indptr[row];
  const int end = a.indptr[row + 1];
  const bool weighted = a.weight != nullptr;
  const T* const base = a.input + col0;
  float acc[BT][V];
#pragma unroll
  for (int j = 0; j < BT; ++j)
#pragma unroll
    for (int i = 0; i < V; ++i) acc[j][i] = 0.0f;

  // batches of UNROLL entries, the last one with clamped ids: every load is issued before the first is consumed
  for (; e < end; e += UNROLL) {
    const int n = end - e;
    uint4_t xraw[UNROLL];
    float4_t craw[UNROLL][NC];
    float w[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int ee = u < n ? e + u : end - 1;
      const long long t = a.etype[ee];
      w[u] = weighted ? a.weight[ee] : 1.0f;
      xraw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
#if VOLTRIX_SPMM_REL_COEF_LDS
        craw[u][j] = table[(t * a.B_pad + coff[j]) >> 2];
#else
        craw[u][j] = *reinterpret_cast<const float4_t*>(a.coef + t * a.B_pad + coff[j]);
#endif
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (u < n) {
        float x[V];
        csr_piece_as_float<T>(x, xraw[u]);
#pragma unroll
        for (int j = 0; j < BT; ++j) {
          if (j < live) {
            const float c = w[u] * craw[u][j / 4][j % 4];
#pragma unroll
            for (int i = 0; i < V; ++i) acc[j][i] += c * x[i];
          }
        }
      }
    }
  }
  float* const out = a.output + (row * a.B + b0) * F + col0;
#pragma unroll
  for (int j = 0; j < BT; ++j) {
    if (j < live) {
      csr_store_piece(out + j * F, acc[j]);
    }
  }
}

// what the three entry points check alike, before anything else: sizes and limits
inline bool rel_sizes_ok(int num_rows, long long num_entries, int embedding_dim, int num_types, int num_bases) {
  return num_rows >= 0 && embedding_dim >= 0 && num_entries >= 0 && num_entries <= INT_MAX && num_types >= 1 &&
         num_types <= kRelMaxTypes && num_bases >= 0 && num_bases <= kRelMaxBases;
}

// dtype: 0 fp32, 1 fp16, 2 bfloat16.  embedding_dim % (16 / sizeof(T)) == 0; 1 <= num_types <= 65 536; 0 <= num_bases <= 1 024; coef is
// [num_types, B_pad] with B_pad = num_bases rounded up to 4.  Every element of `output` [num_rows, num_bases, embedding_dim] is written;
// on a pattern without entries it is zero-filled and neither `indices`, `etype`, `weight`, `input` nor `coef` is read (they must still be
// valid pointers).  `weight` may be NULL.  Nothing is checked on the device: indptr must be a valid CSR of num_rows rows with
// num_entries entries, every index a row of `input`, every etype a row of `coef`.
inline int launch_spmm_rel(const int* indptr, const int* indices, const int* etype, const float* weight, int num_rows,
                           long long num_entries, int embedding_dim, int num_types, int num_bases, const void* input, int dtype,
                           const float* coef, float* output, hipStream_t stream) {
  if (!rel_sizes_ok(num_rows, num_entries, embedding_dim, num_types, num_bases) || dtype < 0 || dtype > 2) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0 || num_bases == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(etype, 3) || misaligned(weight, 3) || bad_ptr(input, 15) ||
      bad_ptr(coef, 15) || bad_ptr(output, 15))
    return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / v);
  if (!g.ok) return kErrBadShape;
  const int table_pieces = num_types * (rel_padded_bases(num_bases) / 4);
  if (VOLTRIX_SPMM_REL_COEF_LDS && table_pieces > kRelLdsFloats / 4) return kErrBadShape;   // the experiment's build: the table must fit
  const int tile = num_bases <= 4 ? 4 : kRelBasisTile;
  const dim3 grid = row_group_dim3(g, (unsigned)((num_bases + tile - 1) / tile));
  dispatch_feature_type(dtype, [&](auto tag) {
    using T = decltype(tag);
    const SpmmRelArgs<T> a{indptr, indices, etype, weight, static_cast<const T*>(input), coef, output, num_rows, embedding_dim,
                           num_bases, rel_padded_bases(num_bases), g.lanes, (int)g.per_xcd, table_pieces};
    if (tile == 4) hipLaunchKernelGGL((spmm_rel_kernel<T, 4>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((spmm_rel_kernel<T, kRelBasisTile>), grid, dim3(256), 0, stream, a);
  });
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- grad_feat: the contraction over the bases, on the transposed CSR -----------------------------------------------------------------
struct SpmmRelContractArgs {
  const int* indptr;       // [num_rows + 1] of the CSR at hand (the transpose: a row is a column of the forward's pattern)
  const int* indices;      // [nnz] rows of `grad_out`
  const int* order;        // [nnz] the entry of etype / weight that entry e uses, or NULL: e itself
  const int* etype;        // [nnz]
  const float* weight;     // [nnz] or NULL
  const float* grad_out;   // [*, B, F]
  const float* coef;       // [R, B_pad]
  float* output;           // [num_rows, F]
  int num_rows;
  int F;
  int B;
  int B_pad;
  int lanes_per_row;
  int groups_per_xcd;
};

template <int BT, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_rel_contract_kernel(const SpmmRelContractArgs a) {
  static_assert(BT % 4 == 0, "whole 16-byte pieces of a row of coef");
  constexpr int V = 4;
  constexpr int NC = BT / 4;
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;
  const long long row = p.row, col0 = p.col0;
  const long long F = a.F;
  const long long BF = (long long)a.B * F;
  int e = a.indptr[row];
  const int end = a.indptr[row + 1];
  const bool weighted = a.weight != nullptr, ordered = a.order != nullptr;
  float acc[V] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (; e < end; e += UNROLL) {
    const int n = end - e;
    const float* gp[UNROLL];
    const float* cp[UNROLL];
    float w[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int ee = u < n ? e + u : end - 1;
      const int id = ordered ? a.order[ee] : ee;
      gp[u] = a.grad_out + (long long)a.indices[ee] * BF + col0;
      cp[u] = a.coef + (long long)a.etype[id] * a.B_pad;
      w[u] = weighted ? a.weight[id] : 1.0f;
    }
    for (int b0 = 0; b0 < a.B; b0 += BT) {
      float4_t g[UNROLL][BT], c[UNROLL][NC];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int j = 0; j < NC; ++j)
          c[u][j] = *reinterpret_cast<const float4_t*>(cp[u] + (b0 + 4 * j < a.B_pad - 4 ? b0 + 4 * j : a.B_pad - 4));
#pragma unroll
        for (int j = 0; j < BT; ++j)
          g[u][j] = *reinterpret_cast<const float4_t*>(gp[u] + (long long)(b0 + j < a.B ? b0 + j : a.B - 1) * F);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (u < n) {
#pragma unroll
          for (int j = 0; j < BT; ++j) {
            if (b0 + j < a.B) {
              const float cc = w[u] * c[u][j / 4][j % 4];
#pragma unroll
              for (int i = 0; i < V; ++i) acc[i] += cc * g[u][j][i];
            }
          }
        }
      }
    }
  }
  csr_store_piece(a.output + row * F + col0, acc);
}

// The CSR at hand is the TRANSPOSE of the forward's pattern: num_rows = the forward's num_cols.  embedding_dim % 4 == 0; the limits of
// launch_spmm_rel.  Every element of `output` [num_rows, embedding_dim] is written; on a pattern without entries it is zero-filled and
// nothing but indptr is read.  `order` and `weight` may be NULL.  Nothing is checked on the device: every index must be a row of
// `grad_out` [*, num_bases, embedding_dim], every order[e] (or e) an entry of `etype` / `weight`, every etype a row of `coef`.
inline int launch_spmm_rel_contract(const int* indptr, const int* indices, const int* order, const int* etype, const float* weight,
                                    int num_rows, long long num_entries, int embedding_dim, int num_types, int num_bases,
                                    const float* grad_out, const float* coef, float* output, hipStream_t stream) {
  if (!rel_sizes_ok(num_rows, num_entries, embedding_dim, num_types, num_bases) || embedding_dim % 4) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0 || num_bases == 0) return kOk;   // num_bases == 0: the caller zero-fills (nothing is launched)
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || misaligned(order, 3) || bad_ptr(etype, 3) || misaligned(weight, 3) ||
      bad_ptr(grad_out, 15) || bad_ptr(coef, 15) || bad_ptr(output, 15))
    return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / 4);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  const SpmmRelContractArgs a{indptr, indices, order, etype, weight, grad_out, coef, output, num_rows, embedding_dim,
                              num_bases, rel_padded_bases(num_bases), g.lanes, (int)g.per_xcd};
  hipLaunchKernelGGL((spmm_rel_contract_kernel<kRelContractTile>), grid, dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- the dots behind grad_coef: row-parallel, one [nnz, B_pad] fp32 result ---------------------------------------------------------------
template <typename T>
struct SpmmRelDotsArgs {
  const int* indptr;       // [num_rows + 1]
  const int* indices;      // [nnz] rows of `feat`
  const float* weight;     // [nnz] or NULL
  const float* grad_out;   // [num_rows, B, F]
  const T* feat;           // [*, F]
  float* output;           // [nnz, B_pad]
  int num_rows;
  int F;
  int B;
  int B_pad;
  int lanes_per_row;
  int groups_per_xcd;
  int slabs;               // ceil(F / V / 64), walked inside the kernel
};

template <typename T, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_rel_dots_kernel(const SpmmRelDotsArgs<T> a) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int DT = kRelDotsTile;
  const int L = a.lanes_per_row;
  const int rows_per_group = 256 / L;
  const long long group = (long long)(blockIdx.x % kNumXcd) * a.groups_per_xcd + blockIdx.x / kNumXcd;
  const long long row = group * rows_per_group + (int)threadIdx.x / L;
  if (row >= a.num_rows) return;               // a whole lane group leaves together: the shuffles below stay inside a group
  const int lane = (int)threadIdx.x & (L - 1);
  const long long F = a.F;
  const int begin = a.indptr[row], end = a.indptr[row + 1];
  if (begin == end) return;
  const bool weighted = a.weight != nullptr;
  const float* const grow = a.grad_out + row * a.B * F;

  for (int b0 = 0; b0 < a.B_pad; b0 += DT) {
    float g[DT][V];
    // this lane's piece of g[row, b0 .. b0 + DT) in slab `slab`; zeros past F; bases past B read the last one and are not stored
    auto load_g = [&](const int slab) {
      const long long col0 = ((long long)slab * 64 + lane) * V;
#pragma unroll
      for (int j = 0; j < DT; ++j) {
        if (col0 < F) {
          const float4_t* p = reinterpret_cast<const float4_t*>(grow + (long long)(b0 + j < a.B ? b0 + j : a.B - 1) * F + col0);
#pragma unroll
          for (int i = 0; i < V / 4; ++i) {
            const float4_t piece = p[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) g[j][4 * i + k] = piece[k];
          }
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) g[j][i] = 0.0f;
        }
      }
    };
    load_g(0);
    for (int e = begin; e < end; e += UNROLL) {
      const int n = end - e;
      long long col[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) col[u] = a.indices[u < n ? e + u : end - 1];
      float p[UNROLL][DT];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < DT; ++j) p[u][j] = 0.0f;
      for (int slab = 0; slab < a.slabs; ++slab) {
        const long long col0 = ((long long)slab * 64 + lane) * V;
        if (a.slabs > 1) load_g(slab);
        if (col0 < F) {
          uint4_t xraw[UNROLL];
#pragma unroll
          for (int u = 0; u < UNROLL; ++u) xraw[u] = *reinterpret_cast<const uint4_t*>(a.feat + col[u] * F + col0);
#pragma unroll
          for (int u = 0; u < UNROLL; ++u) {
            float x[V];
            csr_piece_as_float<T>(x, xraw[u]);
#pragma unroll
            for (int j = 0; j < DT; ++j)
#pragma unroll
              for (int i = 0; i < V; ++i) p[u][j] += g[j][i] * x[i];
          }
        }
      }
      // the group's sum of every p: xor butterfly, constant masks under the uniform predicate m < L
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        if (m < L) {
#pragma unroll
          for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < DT; ++j) p[u][j] += __shfl_xor(p[u][j], m, 64);
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          if (u < n) {
            const float w = weighted ? a.weight[e + u] : 1.0f;
            float* const out = a.output + (long long)(e + u) * a.B_pad + b0;
#pragma unroll
            for (int q = 0; q < DT / 4; ++q) {
              if (b0 + 4 * q < a.B_pad) {
                float r[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = b0 + 4 * q + k < a.B ? w * p[u][4 * q + k] : 0.0f;
                reinterpret_cast<float4_t*>(out)[q] = float4_t{r[0], r[1], r[2], r[3]};
              }
            }
          }
        }
      }
    }
  }
}

// dtype (of feat): 0 fp32, 1 fp16, 2 bfloat16.  embedding_dim % (16 / sizeof(T)) == 0 (so % 4: grad_out's rows are whole pieces too);
// 0 <= num_bases <= 1 024.  Every element of `output` [num_entries, B_pad] is written, the padding as 0 (a row of the pattern writes its
// own entries).  `weight` may be NULL.  Nothing is checked on the device: indptr must be a valid CSR of num_rows rows with num_entries
// entries and every index a row of `feat`.
inline int launch_spmm_rel_dots(const int* indptr, const int* indices, const float* weight, int num_rows, long long num_entries,
                                int embedding_dim, int num_bases, const float* grad_out, const void* feat, int dtype, float* output,
                                hipStream_t stream) {
  if (!rel_sizes_ok(num_rows, num_entries, embedding_dim, 1, num_bases) || dtype < 0 || dtype > 2) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0 || num_bases == 0 || num_entries == 0) return kOk;   // embedding_dim == 0: the caller zero-fills
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || misaligned(weight, 3) || bad_ptr(grad_out, 15) || bad_ptr(feat, 15) ||
      bad_ptr(output, 15))
    return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / v);
  if (!g.ok) return kErrBadShape;
  const dim3 grid((unsigned)(g.per_xcd * kNumXcd));
  dispatch_feature_type(dtype, [&](auto tag) {
    using T = decltype(tag);
    const SpmmRelDotsArgs<T> a{indptr, indices, weight, grad_out, static_cast<const T*>(feat), output, num_rows, embedding_dim,
                               num_bases, rel_padded_bases(num_bases), g.lanes, (int)g.per_xcd, g.slabs};
    hipLaunchKernelGGL((spmm_rel_dots_kernel<T>), grid, dim3(256), 0, stream, a);
  });
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
