// Voltrix-SpMM for MI355X (gfx950) -- aggregation with a feature VECTOR per edge, and its two gradients:
//   out[r, f]        = sum over the entries e of row r of m(input[indices[e], f], efeat[e, f])            (fp32 [num_rows, F])
//   grad_efeat[e, f] = grad_out[row_e, f] * dm/dw                                                         (fp32 [nnz, F])
//   grad_feat[c, f]  = sum over the entries e of column c of grad_out[row_e, f] * dm/dx                   (this kernel on the transpose)
// with m = x * w (mul; DGL's u_mul_e_sum), x + w (add; u_add_e_sum), max(x + w, 0) (add_relu; GINE's message) or w (copy; copy_e_sum).
//
// Why it exists.  Every other operator here takes at most one scalar per edge (spmm_csr_rows weighted, spmm_csr_heads, attn_aggregate)
// or none (spmm_csr_reduce).  GINE, NNConv / MPNN, CGConv and every molecular GNN aggregate messages built from efeat [nnz, F].  The
// composite -- feat[cols] ([nnz, F] materialised), an elementwise op, index_add_ -- moves the gathered rows three times, needs int64
// row ids per entry, and its float atomics give other bits on every run.
//
// Forward shape.  The row-gather skeleton of csr_row_gather.hpp with UNROLL = 4 (the forward kernel takes the lane's place from it and
// writes the batch loop out, for one instantiation's registers: see the kernel).  A lane owns V = 16 / sizeof(TE) consecutive
// features: one 16-byte load of efeat[id], the matching V elements of input[col] (16 bytes; 32 where TI is fp32 and TE is 16-bit) and
// V / 4 float4 stores.  fp32 additions in CSR order: |out - ref| <= (k + 1) 2^-23 sum |terms| for the k terms of an element (each term
// one rounding, k - 1 additions; holds with and without contraction of the product into the sum).  No LDS, no workspace, no atomics:
// the same bits on every call.  Every element of `output` is written; a row without entries gives 0.
//
// One kernel for both directions.  `order` (nullable, int32 [nnz]): entry e of the CSR at hand reads efeat[order[e]]; NULL means
// efeat[e].  The forward passes NULL, the backward on the transposed CSR passes t_order (the branch is wave-uniform).  `self` (op gate
// only): [num_rows, F] of type TE, read once per row.
//   gate: acc += (self[row, f] + w) > 0 ? x : 0 -- the gradient of add_relu for feat, on the transpose: x = grad_out[row_e] (fp32),
//         self = feat[c], w = efeat[t_order[e]].
// The gate (a + b) > 0 is one fp32 addition of the exactly converted operands: its sign is the sign of the exact sum (a rounded sum is
// zero only where the exact one is), so it agrees with a float64 oracle element for element; at an exact zero it is closed, as
// torch.relu's gradient.  A closed gate passes nothing (a select, not a product with 0).  add_relu is a compare and a select, not fmaxf /
// v_max_f32, which return the non-NaN operand (spmm_csr_reduce_kernels.hpp): max(NaN + w, 0) gives NaN.
//
// Pairs (TI, TE): (T, T) for fp32 / fp16 / bf16 and (fp32, fp16 | bf16) -- grad_out is fp32 while efeat keeps its stored type, so the
// backward never copies [nnz, F].  gate is instantiated for TI = fp32 only (its x is always grad_out); copy per TE.
//
// grad_efeat.  spmm_edge_grad_efeat_kernel: row-parallel, the same geometry; the lane group keeps its piece of grad_out[row] (fp32) in
// registers, walks the row's entries with the same batched loads and writes grad_efeat[e, piece] with 16-byte stores:
//   mul: g * feat[col_e]    add, copy: g (reads neither feat nor efeat)    add_relu: (feat[col_e] + efeat[e]) > 0 ? g : 0
// |grad_efeat - ref| <= 2^-23 |ref| for mul (one rounding); exact for the others.  Every element written, no atomics.
//
// Offsets row F, col F and id F are 64-bit.  efeat is streamed exactly once; VOLTRIX_SPMM_EDGE_NT = 1 compiles its loads as non-temporal
// ones.  Measured both ways (harness/experiments/exp_spmm_edge_nt.py): non-temporal is 6-11 % faster on the mid-degree
// stand-in at F = 128 and 2-10 % slower on the low-degree molecular ones and at F = 32 -- no winner, so the loads stay plain.  Bound: HBM for efeat,
// the CUs' line-request rate / L2 for the gathered rows; bytes 4 (n + 1) + 4 nnz + nnz F (sizeof TI + sizeof TE) + 4 n F.  Known limit:
// a hub row (a hub column in grad_feat) serialises its wave, like spmm_csr_heads.  Nothing is checked on the device.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_csr_reduce_kernels.hpp"

#ifndef VOLTRIX_SPMM_EDGE_NT
#define VOLTRIX_SPMM_EDGE_NT 0
#endif

namespace voltrix {

constexpr int kEdgeMul = 0, kEdgeAdd = 1, kEdgeAddRelu = 2, kEdgeCopy = 3, kEdgeGate = 4;
constexpr bool kEdgeEfeatNontemporal = VOLTRIX_SPMM_EDGE_NT != 0;

template <typename TI, typename TE>
struct SpmmEdgeArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz] column ids = rows of `input`
  const int* order;     // [nnz] the row of `efeat` entry e uses, or NULL: e itself
  const TI* input;      // [*, F] row-major; unused by copy
  const TE* efeat;      // [nnz, F]
  const TE* self;       // gate: [num_rows, F]; else unused
  float* output;        // [num_rows, F]
  int num_rows;
  int F;
  int lanes_per_row;    // power of two <= 64
  int groups_per_xcd;   // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
};

// 16 bytes of the streamed operand
__device__ __forceinline__ uint4_t edge_stream_load(const void* p) {
  if constexpr (kEdgeEfeatNontemporal) return __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(p));
  else return *reinterpret_cast<const uint4_t*>(p);
}

// V elements of type T from NR = V sizeof(T) / 16 registers of 16 bytes, as fp32 (exact)
template <typename T, int V>
__device__ __forceinline__ void edge_as_float(float (&x)[V], const uint4_t (&raw)[V * (int)sizeof(T) / 16]) {
  if constexpr (V * (int)sizeof(T) == 16) {
    csr_piece_as_float<T>(x, raw[0]);
  } else {   // fp32 beside a 16-bit efeat: 8 floats
    static_assert(std::is_same<T, float>::value && V == 8, "32 bytes of fp32");
    const float4_t lo = __builtin_bit_cast(float4_t, raw[0]), hi = __builtin_bit_cast(float4_t, raw[1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = lo[i], x[4 + i] = hi[i];
  }
}

template <typename TI, typename TE, int OP, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_edge_kernel(const SpmmEdgeArgs<TI, TE> a) {
  static_assert(OP >= kEdgeMul && OP <= kEdgeGate, "op");
  constexpr int V = 16 / (int)sizeof(TE);
  constexpr int NR = OP == kEdgeCopy ? 1 : V * (int)sizeof(TI) / 16;     // 16-byte registers of input[col] per entry
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);   // a lane: V features
  if (!p.work) return;
  const long long row = p.row, col0 = p.col0;
  const long long F = a.F;
  int e = a.indptr[row];
  const int end = a.indptr[row + 1];
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  float own[V];   // gate: self[row]'s piece
  if constexpr (OP == kEdgeGate) csr_piece_as_float<TE>(own, *reinterpret_cast<const uint4_t*>(a.self + row * F + col0));
  const TE* const ebase = a.efeat + col0;
  const bool ordered = a.order != nullptr;

  auto consume = [&](const uint4_t (&xraw)[NR], const uint4_t wraw) {
    float w[V];
    csr_piece_as_float<TE>(w, wraw);
    if constexpr (OP == kEdgeCopy) {
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] += w[i];
    } else {
      float x[V];
      edge_as_float<TI, V>(x, xraw);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if constexpr (OP == kEdgeMul) {
          acc[i] += x[i] * w[i];
        } else if constexpr (OP == kEdgeAdd) {
          acc[i] += x[i] + w[i];
        } else if constexpr (OP == kEdgeAddRelu) {
          const float s = x[i] + w[i];
          acc[i] += s < 0.0f ? 0.0f : s;          // a NaN stays a NaN
        } else {
          acc[i] += own[i] + w[i] > 0.0f ? x[i] : 0.0f;
        }
      }
    }
  };
  auto issue = [&](uint4_t (&xraw)[NR], uint4_t& wraw, const int ee) {
    const long long id = ordered ? a.order[ee] : ee;
    wraw = edge_stream_load(ebase + id * F);
    if constexpr (OP != kEdgeCopy) {
      const TI* const x = a.input + col0 + (long long)a.indices[ee] * F;
#pragma unroll
      for (int j = 0; j < NR; ++j) xraw[j] = reinterpret_cast<const uint4_t*>(x)[j];
    }
  };
  // csr_for_each_batch's loop and csr_store_piece's store, written out: the (bf16, bf16, add_relu) instantiation sits at 80 VGPRs, the
  // most that keep 6 waves per SIMD, and either helper costs it two more and a wave (profiles/csr_row_gather/README.md)
  for (; end - e >= UNROLL; e += UNROLL) {
    uint4_t xraw[UNROLL][NR], wraw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) issue(xraw[u], wraw[u], e + u);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) consume(xraw[u], wraw[u]);
  }
  if (e < end) {
    uint4_t xraw[UNROLL][NR], wraw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) issue(xraw[u], wraw[u], u < end - e ? e + u : end - 1);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (u < end - e) consume(xraw[u], wraw[u]);
  }
  float4_t* out = reinterpret_cast<float4_t*>(a.output + row * F + col0);
#pragma unroll
  for (int i = 0; i < V / 4; ++i) out[i] = float4_t{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]};
}

// the pairs (input, efeat) the forward kernel is instantiated for: (T, T) and (fp32, 16-bit); gate: fp32 input only
inline bool spmm_edge_pair_ok(int input_dtype, int efeat_dtype, int op) {
  if (efeat_dtype < 0 || efeat_dtype > 2) return false;
  if (op == kEdgeCopy) return true;                      // input is not read, its dtype not looked at
  if (input_dtype < 0 || input_dtype > 2) return false;
  if (op == kEdgeGate) return input_dtype == 0;
  return input_dtype == efeat_dtype || input_dtype == 0;
}

// dtypes: 0 fp32, 1 fp16, 2 bfloat16; op: 0 mul, 1 add, 2 add_relu, 3 copy, 4 gate.  embedding_dim % (16 / sizeof(TE)) == 0.  Every
// element of `output` is written; on a pattern without entries it is zero-filled and neither `indices`, `input`, `efeat` nor `order` is
// read (they must still be valid pointers).  `order` may be NULL, `input` with copy, `self` without gate.  Nothing is checked on the
// device: indptr must be a valid CSR of num_rows rows with num_entries entries, every index a row of `input`, every order[e] (or e) a
// row of `efeat`.
inline int launch_spmm_edge(const int* indptr, const int* indices, const int* order, int num_rows, long long num_entries,
                            int embedding_dim, const void* input, int input_dtype, const void* efeat, int efeat_dtype, const void* self,
                            int op, float* output, hipStream_t stream) {
  if (num_rows < 0 || embedding_dim < 0 || num_entries < 0 || num_entries > INT_MAX || op < kEdgeMul || op > kEdgeGate)
    return kErrBadShape;
  if (!spmm_edge_pair_ok(input_dtype, efeat_dtype, op)) return kErrBadShape;
  const int v = piece_elems(efeat_dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(efeat, 15) || bad_ptr(output, 15) || misaligned(order, 3) ||
      misaligned(input, 15) || misaligned(self, 15))
    return kErrBadShape;
  if ((op == kEdgeGate && self == nullptr) || (op != kEdgeCopy && input == nullptr)) return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / v);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  auto go = [&](auto itag, auto etag) {
    using TI = decltype(itag);
    using TE = decltype(etag);
    const SpmmEdgeArgs<TI, TE> a{indptr, indices, order, static_cast<const TI*>(input), static_cast<const TE*>(efeat),
                                 static_cast<const TE*>(self), output, num_rows, embedding_dim, g.lanes, (int)g.per_xcd};
    if (op == kEdgeMul) hipLaunchKernelGGL((spmm_edge_kernel<TI, TE, kEdgeMul>), grid, dim3(256), 0, stream, a);
    else if (op == kEdgeAdd) hipLaunchKernelGGL((spmm_edge_kernel<TI, TE, kEdgeAdd>), grid, dim3(256), 0, stream, a);
    else if (op == kEdgeAddRelu) hipLaunchKernelGGL((spmm_edge_kernel<TI, TE, kEdgeAddRelu>), grid, dim3(256), 0, stream, a);
    else if constexpr (std::is_same<TI, float>::value) hipLaunchKernelGGL((spmm_edge_kernel<TI, TE, kEdgeGate>), grid, dim3(256), 0, stream, a);
  };
  if (op == kEdgeCopy) {
    dispatch_feature_type(efeat_dtype, [&](auto etag) {
      using TE = decltype(etag);
      const SpmmEdgeArgs<TE, TE> a{indptr, indices, order, nullptr, static_cast<const TE*>(efeat), nullptr, output, num_rows,
                                   embedding_dim, g.lanes, (int)g.per_xcd};
      hipLaunchKernelGGL((spmm_edge_kernel<TE, TE, kEdgeCopy>), grid, dim3(256), 0, stream, a);
    });
  } else if (input_dtype == efeat_dtype) {
    dispatch_feature_type(efeat_dtype, [&](auto tag) { go(tag, tag); });
  } else {
    dispatch_feature_type(efeat_dtype, [&](auto etag) {
      if constexpr (!std::is_same<decltype(etag), float>::value) go(float{}, etag);
    });
  }
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- the gradient for efeat: row-parallel, one [nnz, F] fp32 result --------------------------------------------------------------------
template <typename T>
struct SpmmEdgeGradArgs {
  const int* indptr;       // [num_rows + 1]
  const int* indices;      // [nnz]; unused by add
  const float* grad_out;   // [num_rows, F]
  const T* feat;           // [*, F]; mul and add_relu
  const T* efeat;          // [nnz, F]; add_relu
  float* output;           // [nnz, F]
  int num_rows;
  int F;
  int lanes_per_row;
  int groups_per_xcd;
};

template <typename T, int OP, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_edge_grad_efeat_kernel(const SpmmEdgeGradArgs<T> a) {
  static_assert(OP == kEdgeMul || OP == kEdgeAdd || OP == kEdgeAddRelu, "copy is add");
  constexpr int V = 16 / (int)sizeof(T);
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;
  const long long row = p.row, col0 = p.col0;
  const long long F = a.F;
  int e = a.indptr[row];
  const int end = a.indptr[row + 1];
  if (e == end) return;
  float g[V];
#pragma unroll
  for (int i = 0; i < V / 4; ++i) {
    const float4_t piece = reinterpret_cast<const float4_t*>(a.grad_out + row * F + col0)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[4 * i + j] = piece[j];
  }
  float* const out = a.output + col0;
  if constexpr (OP == kEdgeAdd) {
    for (; e < end; ++e) csr_store_piece(out + (long long)e * F, g);
  } else {
    struct Slot {
      uint4_t xraw, wraw;   // wraw: add_relu
    };
    csr_for_each_batch<UNROLL, Slot>(
        e, end,
        [&](Slot& s, const int ee) {
          s.xraw = *reinterpret_cast<const uint4_t*>(a.feat + (long long)a.indices[ee] * F + col0);
          if constexpr (OP == kEdgeAddRelu) s.wraw = edge_stream_load(a.efeat + (long long)ee * F + col0);
        },
        [&](const Slot& s, const int entry, const bool live) {
          if (!live) return;
          float x[V], r[V];
          csr_piece_as_float<T>(x, s.xraw);
          if constexpr (OP == kEdgeMul) {
#pragma unroll
            for (int i = 0; i < V; ++i) r[i] = g[i] * x[i];
          } else {
            float w[V];
            csr_piece_as_float<T>(w, s.wraw);
#pragma unroll
            for (int i = 0; i < V; ++i) r[i] = x[i] + w[i] > 0.0f ? g[i] : 0.0f;
          }
          csr_store_piece(out + (long long)entry * F, r);
        });
  }
}

// dtype (of feat and efeat): 0 fp32, 1 fp16, 2 bfloat16; op: 0 mul, 1 add, 2 add_relu, 3 copy (= add).  embedding_dim % (16 /
// sizeof(T)) == 0.  Every element of `output` [num_entries, embedding_dim] is written (a row of the pattern writes its own entries).
// feat is read by mul and add_relu, efeat by add_relu, indices by both; what an op does not read may be NULL.  Nothing is checked on
// the device: indptr must be a valid CSR of num_rows rows with num_entries entries and every index a row of `feat`.
inline int launch_spmm_edge_grad_efeat(const int* indptr, const int* indices, int num_rows, long long num_entries, int embedding_dim,
                                       const float* grad_out, const void* feat, const void* efeat, int dtype, int op, float* output,
                                       hipStream_t stream) {
  if (num_rows < 0 || embedding_dim < 0 || num_entries < 0 || num_entries > INT_MAX || op < kEdgeMul || op > kEdgeCopy || dtype < 0 ||
      dtype > 2)
    return kErrBadShape;
  const int v = piece_elems(dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0 || num_entries == 0) return kOk;
  const bool gathers = op == kEdgeMul || op == kEdgeAddRelu;
  if (bad_ptr(indptr, 3) || bad_ptr(grad_out, 15) || bad_ptr(output, 15) || misaligned(indices, 3) || misaligned(feat, 15) ||
      misaligned(efeat, 15))
    return kErrBadShape;
  if (gathers && (indices == nullptr || feat == nullptr)) return kErrBadShape;
  if (op == kEdgeAddRelu && efeat == nullptr) return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / v);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  dispatch_feature_type(dtype, [&](auto tag) {
    using T = decltype(tag);
    const SpmmEdgeGradArgs<T> a{indptr, indices, grad_out, static_cast<const T*>(feat), static_cast<const T*>(efeat), output,
                                num_rows, embedding_dim, g.lanes, (int)g.per_xcd};
    if (op == kEdgeMul) hipLaunchKernelGGL((spmm_edge_grad_efeat_kernel<T, kEdgeMul>), grid, dim3(256), 0, stream, a);
    else if (op == kEdgeAddRelu) hipLaunchKernelGGL((spmm_edge_grad_efeat_kernel<T, kEdgeAddRelu>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((spmm_edge_grad_efeat_kernel<T, kEdgeAdd>), grid, dim3(256), 0, stream, a);
  });
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
