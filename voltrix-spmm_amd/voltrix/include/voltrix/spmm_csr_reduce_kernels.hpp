// Voltrix-SpMM for MI355X (gfx950) -- max / min / mean neighbour aggregation straight from the CSR, with the backward of max / min:
//   out[r, f] = max | min | mean over the entries e of row r of feat[col_e, f]        (fp32 [num_rows, F])
//   arg[r, f] = the CSR ENTRY id e of the winner (max / min only; int32 [num_rows, F])
//   d_feat[c, f] = sum over the entries e of column c with arg[row_e, f] == e of grad_out[row_e, f]
//
// Why it exists.  Every other operator here sums its neighbours (spmm_csr_kernels.hpp, spmm_csr_heads_kernels.hpp,
// attn_aggregate_kernels.hpp).  Max-pool GraphSAGE, PNA's towers, GIN-max and edge convolutions select.  The composite -- feat[cols]
// ([nnz, F] materialised) + scatter_reduce -- moves the gathered rows three times and has an index_add backward with float atomics.
//
// Forward shape.  The row-gather skeleton of csr_row_gather.hpp (V = 16 bytes of the operand, UNROLL = 4); a surplus slot of the tail
// batch never takes part in the selection.  No workspace.
//
// Selection (max; min mirrors it).  Per element `best` (float) and `arg` (int32) start at (-inf, indptr[row]); entry e with value v is
// taken when v > best || (v != v && best == best).  Strict, so the first entry in CSR order wins ties (+0 and -0 tie); the first NaN
// wins and stays (what torch.amax returns); a row whose entries are all -inf keeps -inf with arg at its first entry.  A compare and two
// selects per element -- not fmaxf / v_max_f32, which return the non-NaN operand and get canonicalising ops around them.  A selection
// does not round: out has the bits of the winning element converted to fp32.  A row without entries gives 0 and arg = -1 (the zeros
// every other operator writes for an empty row).  arg is the ENTRY id, not the column: on a pattern with duplicate (row, col) entries a
// column id would match both in the backward and count the gradient twice.  arg == NULL: neither computed nor stored (a template flag).
//
// mean.  csr_accumulate<T> (the sum kernel's fp32 additions in CSR order), then one fp32 division by the row's entry count per element:
// |out - ref| <= (deg + 1) 2^-23 sum_e |feat_e| / deg.  Duplicates count twice, as in spmm_csr_rows; empty rows give 0; no arg.
//
// Backward of max / min.  On the TRANSPOSED CSR, so a gather without atomics: a lane group owns column c, a lane 4 consecutive
// features (16 bytes of arg and of fp32 grad_out).  For every entry e of column c: r = t_indices[e], id = t_order[e]; where
// arg[r, f] == id, d_feat[c, f] += grad_out[r, f], in the transposed CSR's order.  grad_out[r] is loaded only where one of the lane's
// four components matched (no load for an entry that contributes nothing: about one entry in deg_r does).  Every row of d_feat is
// written, columns without entries get zeros.  The same bits on every call.  The backward of mean needs no kernel: spmm_csr_rows on the
// transposed CSR applied to grad_out / deg.
//
// Offsets row F and e-based offsets are 64-bit.  Bound: the CUs' line-request rate / HBM; forward bytes 4 (n + 1) + 4 nnz + nnz F
// sizeof(T) + 8 n F (4 n F without arg).  Known limit: a hub row in the forward, or a hub column in the backward, serialises its wave,
// like spmm_csr_heads.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_csr_kernels.hpp"

namespace voltrix {

constexpr int kReduceMax = 0, kReduceMin = 1, kReduceMean = 2;

template <typename T>
struct CsrReduceArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz] column ids = rows of `input`
  const T* input;       // [*, F] row-major, rows 16-byte aligned
  float* output;        // [num_rows, F]
  int* arg;             // WITH_ARG kernels: [num_rows, F] CSR entry id of the winner, -1 for a row without entries; else unused
  int num_rows;
  int F;
  int lanes_per_row;    // power of two <= 64
  int groups_per_xcd;   // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
};

// entry `e`'s piece against the running winner: strict, first wins ties, the first NaN wins and stays.  `live` = false: a surplus slot
// of the tail batch, never taken (part of the predicate, so the tail has no branch around its selects)
template <typename T, int OP, bool WITH_ARG>
__device__ __forceinline__ void csr_select(float (&best)[16 / sizeof(T)], int (&arg)[WITH_ARG ? 16 / sizeof(T) : 1], const uint4_t raw,
                                           const int e, const bool live = true) {
  constexpr int V = 16 / (int)sizeof(T);
  float v[V];
  csr_piece_as_float<T>(v, raw);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    // v > best || (v != v && best == best), in two compares: !(v <= best) holds for v > best and for an unordered pair, and
    // best == best leaves of those v > best (both numbers) and "v is the first NaN"
    const bool take = live && !(OP == kReduceMax ? v[i] <= best[i] : v[i] >= best[i]) && best[i] == best[i];
    best[i] = take ? v[i] : best[i];
    if constexpr (WITH_ARG) arg[i] = take ? e : arg[i];
  }
}

template <typename T, int OP, bool WITH_ARG, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_csr_reduce_kernel(const CsrReduceArgs<T> a) {
  static_assert(OP == kReduceMax || OP == kReduceMin || (OP == kReduceMean && !WITH_ARG), "mean has no arg");
  constexpr int V = 16 / (int)sizeof(T);
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;
  const int begin = a.indptr[p.row];
  const int end = a.indptr[p.row + 1];
  float acc[V];   // the sum (mean) or the winner (max / min)
  int arg[WITH_ARG ? V : 1];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = OP == kReduceMean ? 0.0f : OP == kReduceMax ? -__builtin_inff() : __builtin_inff();
  if constexpr (WITH_ARG) {
#pragma unroll
    for (int i = 0; i < V; ++i) arg[i] = begin;
  }
  const T* const base = a.input + p.col0;
  const long long F = a.F;
  struct Slot {
    uint4_t raw;
  };
  csr_for_each_batch<UNROLL, Slot>(
      begin, end, [&](Slot& s, const int ee) { s.raw = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F); },
      [&](const Slot& s, const int entry, const bool live) {
        if constexpr (OP == kReduceMean) {
          if (live) csr_accumulate<T>(acc, s.raw);
        } else {
          csr_select<T, OP, WITH_ARG>(acc, arg, s.raw, entry, live);
        }
      });
  const int deg = end - begin;
  if constexpr (OP == kReduceMean) {
    const float count = (float)(deg > 0 ? deg : 1);
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = acc[i] / count;
  } else if (deg == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc[i] = 0.0f;
      if constexpr (WITH_ARG) arg[i] = -1;
    }
  }
  csr_store_piece(a.output + p.row * F + p.col0, acc);
  if constexpr (WITH_ARG) csr_store_piece(a.arg + p.row * F + p.col0, arg);
}

// dtype: 0 fp32, 1 fp16, 2 bfloat16; op: 0 max, 1 min, 2 mean.  embedding_dim % (16 / sizeof(T)) == 0 (16-byte row pieces).  Every
// element of `output` (and of `arg`, where given: max / min only) is written; a pattern without entries fills them (0, arg = -1) and
// reads neither `indices` nor `input`.  Nothing is checked on the device: indptr must be a valid CSR of num_rows rows and every index a
// row of `input`.
inline int launch_spmm_csr_reduce(const int* indptr, const int* indices, int num_rows, int embedding_dim, const void* input, int dtype,
                                  int op, float* output, int* arg, hipStream_t stream) {
  if (num_rows < 0 || embedding_dim < 0 || dtype < 0 || dtype > 2 || op < 0 || op > 2) return kErrBadShape;
  if (op == kReduceMean && arg != nullptr) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(input, 15) || bad_ptr(output, 15) || misaligned(arg, 15)) return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / v);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    const CsrReduceArgs<T> a{indptr, indices, static_cast<const T*>(input), output, arg, num_rows, embedding_dim, g.lanes, (int)g.per_xcd};
    if (op == kReduceMean)
      hipLaunchKernelGGL((spmm_csr_reduce_kernel<T, kReduceMean, false>), grid, dim3(256), 0, stream, a);
    else if (op == kReduceMax && arg != nullptr)
      hipLaunchKernelGGL((spmm_csr_reduce_kernel<T, kReduceMax, true>), grid, dim3(256), 0, stream, a);
    else if (op == kReduceMax)
      hipLaunchKernelGGL((spmm_csr_reduce_kernel<T, kReduceMax, false>), grid, dim3(256), 0, stream, a);
    else if (arg != nullptr)
      hipLaunchKernelGGL((spmm_csr_reduce_kernel<T, kReduceMin, true>), grid, dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((spmm_csr_reduce_kernel<T, kReduceMin, false>), grid, dim3(256), 0, stream, a);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- backward of max / min on the transposed CSR ------------------------------------------------------------------------------------
struct CsrReduceBackwardArgs {
  const int* t_indptr;     // [num_cols + 1]
  const int* t_indices;    // [nnz] row ids of the forward = rows of `grad_out` and `arg`
  const int* t_order;      // [nnz] the entry of the CSR that entry e of the transpose is
  const float* grad_out;   // [*, F]
  const int* arg;          // [*, F] the forward's
  float* output;           // [num_cols, F]
  int num_cols;
  int F;
  int lanes_per_row;
  int groups_per_xcd;
};

template <int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_csr_reduce_backward_kernel(const CsrReduceBackwardArgs a) {
  const CsrLanePlace p = csr_lane_place<4>(a.lanes_per_row, a.groups_per_xcd, a.num_cols, a.F);   // row: the column c; a lane: 4 features
  if (!p.work) return;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const long long F = a.F;
  // the winners of a batch of entries are loaded before the first is compared; the gradient's row only where a component matched
  struct Slot {
    int4_t won;
    int id;
    long long offset;
  };
  csr_for_each_batch<UNROLL, Slot>(
      a.t_indptr[p.row], a.t_indptr[p.row + 1],
      [&](Slot& s, const int ee) {
        s.offset = (long long)a.t_indices[ee] * F + p.col0;
        s.id = a.t_order[ee];
        s.won = *reinterpret_cast<const int4_t*>(a.arg + s.offset);
      },
      [&](const Slot& s, int, const bool live) {
        if (live && (s.won[0] == s.id || s.won[1] == s.id || s.won[2] == s.id || s.won[3] == s.id)) {
          const float4_t g = *reinterpret_cast<const float4_t*>(a.grad_out + s.offset);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (s.won[i] == s.id) acc[i] += g[i];
        }
      });
  csr_store_piece(a.output + p.row * F + p.col0, acc);
}

// embedding_dim % 4 == 0.  Every row of `output` is written (columns without entries: zeros); with nnz == 0 nothing but t_indptr is
// read.  Nothing is checked on the device: t_indptr must be a valid CSR of num_cols rows with nnz entries, every t_indices a row of
// `grad_out` and `arg`.  `arg` is only compared, never used as an index.
inline int launch_spmm_csr_reduce_backward(const int* t_indptr, const int* t_indices, const int* t_order, int num_cols, long long nnz,
                                           int embedding_dim, const float* grad_out, const int* arg, float* output, hipStream_t stream) {
  if (num_cols < 0 || nnz < 0 || nnz > INT_MAX || embedding_dim < 0 || embedding_dim % 4) return kErrBadShape;
  if (num_cols == 0 || embedding_dim == 0) return kOk;
  if (bad_ptr(t_indptr, 3) || bad_ptr(output, 15)) return kErrBadShape;
  if (nnz > 0 && (bad_ptr(t_indices, 3) || bad_ptr(t_order, 3) || bad_ptr(grad_out, 15) || bad_ptr(arg, 15))) return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_cols, embedding_dim / 4);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  const CsrReduceBackwardArgs a{t_indptr, t_indices, t_order, grad_out, arg, output, num_cols, embedding_dim, g.lanes, (int)g.per_xcd};
  hipLaunchKernelGGL((spmm_csr_reduce_backward_kernel<4>), grid, dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
