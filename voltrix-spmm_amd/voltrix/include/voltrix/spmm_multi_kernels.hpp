// Voltrix-SpMM for MI355X (gfx950) -- several neighbour aggregates from ONE gather of the CSR, and their joint backward:
//   out[r, s, f] = sum | mean | max | min | var | std over the entries e of row r of feat[col_e, f]     (fp32 [num_rows, A, F])
//   argmax / argmin[r, f] = the CSR ENTRY id of the winner                                              (optional; int32 [num_rows, F])
//   d_feat[c, f] = sum over the entries e of column c of u[r_e] + w[r_e] (x_c - mean[r_e]) + [argmax[r_e] == id_e] g_max[r_e]
//                                                        + [argmin[r_e] == id_e] g_min[r_e]
//
// Why it exists.  PNA's default aggregators (mean, max, min, std) -- PyG's MultiAggregation, DGL's PNAConv -- cost four to five gathers
// with the operators so far, and nothing computed a second moment: E[x^2] - E[x]^2 from two sum gathers cancels on every feature with a
// mean (after a ReLU or a bias).  These kernels are bound by the gather (nnz F sizeof(T) bytes, the CUs' line-request rate); the ALU
// work of all aggregates on a 16-byte piece is small beside it, so one pass keeps every accumulator in registers.
//
// Forward shape.  spmm_csr_reduce_kernel's: a group of L = min(64, next_pow2(F / V)) lanes owns one row, grid.y walks slabs of 64
// pieces, a lane owns 16 bytes of every gathered row (V = 4 fp32, 8 fp16 / bf16), XCD x owns a contiguous range of row groups, batches
// of UNROLL = 4 entries are issued before the first is consumed, the tail batch reads clamped ids and its surplus slots are skipped.
// Row and entry offsets are 64-bit.  No LDS, no workspace, no atomics: the same bits on every call.
//
// The aggregates, per row r with d entries (duplicates count twice) and per element:
//   sum   csr_accumulate<T>: fp32 additions in CSR order from 0 -- the bits of spmm_csr_rows with fp32 output.
//   mean  sum / d, one fp32 division -- the bits of spmm_csr_reduce_kernel's mean.
//   max, min, argmax, argmin   csr_select unchanged: strict, the first entry wins ties, the first NaN wins and stays -- the bits of
//         spmm_csr_reduce_kernel.  Both selections run when either is stored.
//   var   max(S2 / d - (S1 / d)^2, 0) from SHIFTED moments: k = the row's first entry in CSR order (per element), y_e = x_e - k,
//         S1 = sum y_e, S2 = sum y_e^2 (one fused multiply-add per entry) in CSR order, in accumulators of their own, so `sum` keeps
//         its bits.  var = fma(-m, m, S2 / d) with m = S1 / d, clamped by `var < 0 ? 0 : var` -- a compare and a select, which lets a
//         NaN through (fmaxf / v_max_f32 return the non-NaN operand: spmm_csr_reduce_kernels.hpp).  A row with one entry gives 0
//         exactly; a row that holds a NaN or +-inf entry gives NaN (inf - k, then inf - inf).
//         |var - ref| <= (d + 4) 2^-23 (2 / d) sum_e (x_e - x_first)^2.
//   std   sqrt(var + eps), eps finite and > 0 (PyG and DGL: 1e-5).
// A row without entries gives 0 in every aggregate -- std included, where PyG gives sqrt(eps) -- and -1 in both args.  The products
// and the final subtraction are written as explicit fused multiply-adds, so no instantiation depends on the compiler's contraction:
// every aggregate has the same bits whichever others are stored.
//
// Output.  out[row * row_stride + slot * F + f] with row_stride = A F and one slot index per aggregate, -1 for "not stored":
// out.view(n, A F) @ W is the layer (spmm_rel's [n, B, F] convention).
//
// Instantiations: <T, HAS_M2, SELECT in {none, values, values + args}> = 18.  The first moment is always computed.
//
// Backward.  One launch on the TRANSPOSED CSR: a lane group owns column c, a lane 4 features (16 bytes of every fp32 / int32 row), as
// spmm_csr_reduce_backward_kernel.  u = g_sum + g_mean / d and w = 2 g_var / d + g_std / (d std) are fp32 [n, F] arrays the caller
// forms with dense ops.  Per entry, in the transposed CSR's order and in this order: acc += u[r]; acc = fma(w[r], x_c - mean[r], acc);
// acc += g_max[r] where argmax[r] == id; acc += g_min[r] where argmin[r] == id (id = t_order[e]).  The form w (x_c - mean_r) per entry,
// not x_c sum w - sum w mean: the latter cancels on exactly the features with a mean the shifted forward exists for.  g_max / g_min
// rows are loaded only where a component matched; u, w and mean only in the variants that use them (<HAS_U, HAS_W, HAS_SEL>, 7
// kernels).  Every row of d_feat is written, columns without entries get zeros.
// x_c is read once per column as FP32: feat itself where it is fp32, one dense cast of [num_cols, F] where it is 16-bit.  The cast
// moves 6 bytes per element once, beside 32 to 80 gathered bytes per entry and lane, and keeps the backward at 7 kernels instead of 15
// with 16-byte loads throughout; a 16-bit read would save that pass and nothing in the gather.
//
// Bound: the CUs' line-request rate / HBM; forward bytes 4 (n + 1) + 4 nnz + nnz F sizeof(T) + 4 n A F (+ 8 n F with both args).
// Known limit: a hub row in the forward, or a hub column in the backward, serialises its wave, like spmm_csr_reduce.  Nothing is
// checked on the device.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_csr_reduce_kernels.hpp"

namespace voltrix {

constexpr int kMultiSum = 0, kMultiMean = 1, kMultiMax = 2, kMultiMin = 3, kMultiVar = 4, kMultiStd = 5, kMultiAggregates = 6;
constexpr int kMultiSelectNone = 0, kMultiSelectValues = 1, kMultiSelectArgs = 2;

template <typename T>
struct SpmmMultiArgs {
  const int* indptr;        // [num_rows + 1]
  const int* indices;       // [nnz] column ids = rows of `input`
  const T* input;           // [*, F] row-major, rows 16-byte aligned
  float* output;            // [num_rows, A, F]
  int* argmax;              // [num_rows, F] or NULL
  int* argmin;              // [num_rows, F] or NULL
  long long row_stride;     // A F
  int slot[kMultiAggregates];   // the slot of sum, mean, max, min, var, std in a row of `output`; -1: not stored
  float eps;
  int num_rows;
  int F;
  int lanes_per_row;        // power of two <= 64
  int groups_per_xcd;       // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
};

template <typename T, bool HAS_M2, int SELECT, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_multi_kernel(const SpmmMultiArgs<T> a) {
  static_assert(SELECT >= kMultiSelectNone && SELECT <= kMultiSelectArgs, "select");
  constexpr int V = 16 / (int)sizeof(T);
  constexpr bool HAS_SEL = SELECT != kMultiSelectNone, WITH_ARG = SELECT == kMultiSelectArgs;
  constexpr int VS = HAS_SEL ? V : 1, VM = HAS_M2 ? V : 1, VA = WITH_ARG ? V : 1;
  const int L = a.lanes_per_row;
  const int rows_per_group = 256 / L;
  // XCD x owns the row groups [x * groups_per_xcd, (x + 1) * groups_per_xcd)
  const long long group = (long long)(blockIdx.x % kNumXcd) * a.groups_per_xcd + blockIdx.x / kNumXcd;
  const long long row = group * rows_per_group + (int)threadIdx.x / L;
  if (row >= a.num_rows) return;
  const int lane = (int)threadIdx.x & (L - 1);
  const long long col0 = ((long long)blockIdx.y * 64 + lane) * V;     // this lane's 16 bytes of every gathered row
  if (col0 >= a.F) return;
  int e = a.indptr[row];
  const int begin = e;
  const int end = a.indptr[row + 1];
  float sum[V], hi[VS], lo[VS], shift[VM], s1[VM], s2[VM];
  int arg_hi[VA], arg_lo[VA];
#pragma unroll
  for (int i = 0; i < V; ++i) sum[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < VS; ++i) hi[i] = -__builtin_inff(), lo[i] = __builtin_inff();
#pragma unroll
  for (int i = 0; i < VM; ++i) shift[i] = s1[i] = s2[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < VA; ++i) arg_hi[i] = arg_lo[i] = begin;
  const T* const base = a.input + col0;
  const long long F = a.F;

  // slot u of the batch that starts at entry e; `live` = false: a surplus slot of the tail batch
  auto consume = [&](const uint4_t raw, const int u, const bool live) {
    if (live) csr_accumulate<T>(sum, raw);
    if constexpr (HAS_SEL) {
      csr_select<T, kReduceMax, WITH_ARG>(hi, arg_hi, raw, e + u, live);
      csr_select<T, kReduceMin, WITH_ARG>(lo, arg_lo, raw, e + u, live);
    }
    if constexpr (HAS_M2) {
      float v[V];
      csr_piece_as_float<T>(v, raw);
      if (u == 0) {                       // the row's first entry is slot 0 of its first batch: the shift
#pragma unroll
        for (int i = 0; i < V; ++i) shift[i] = e == begin ? v[i] : shift[i];
      }
      if (live) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float y = v[i] - shift[i];
          s1[i] += y;
          s2[i] = __builtin_fmaf(y, y, s2[i]);
        }
      }
    }
  };
  // full batches of UNROLL entries, then one more batch for the tail with clamped ids: every load issued before the first is consumed
  for (; end - e >= UNROLL; e += UNROLL) {
    uint4_t raw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) raw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[e + u] * F);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) consume(raw[u], u, true);
  }
  if (e < end) {
    uint4_t raw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int ee = u < end - e ? e + u : end - 1;
      raw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) consume(raw[u], u, u < end - e);
  }

  const int deg = end - begin;
  const float count = (float)(deg > 0 ? deg : 1);
  float* const out = a.output + row * a.row_stride + col0;
  auto store = [&](const int which, const float (&r)[V]) {
    if (a.slot[which] < 0) return;
    float4_t* p = reinterpret_cast<float4_t*>(out + a.slot[which] * F);
#pragma unroll
    for (int i = 0; i < V / 4; ++i) p[i] = float4_t{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
  };
  store(kMultiSum, sum);
  {
    float mean[V];
#pragma unroll
    for (int i = 0; i < V; ++i) mean[i] = sum[i] / count;
    store(kMultiMean, mean);
  }
  if constexpr (HAS_SEL) {
    if (deg == 0) {
#pragma unroll
      for (int i = 0; i < V; ++i) hi[i] = lo[i] = 0.0f;
#pragma unroll
      for (int i = 0; i < VA; ++i) arg_hi[i] = arg_lo[i] = -1;
    }
    store(kMultiMax, hi);
    store(kMultiMin, lo);
    if constexpr (WITH_ARG) {
      auto store_arg = [&](int* const to, const int (&r)[VA]) {
        if (to == nullptr) return;
        int4_t* p = reinterpret_cast<int4_t*>(to + row * F + col0);
#pragma unroll
        for (int i = 0; i < V / 4; ++i) p[i] = int4_t{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
      };
      store_arg(a.argmax, arg_hi);
      store_arg(a.argmin, arg_lo);
    }
  }
  if constexpr (HAS_M2) {
    float var[V], sd[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float m = s1[i] / count;
      const float raw_var = __builtin_fmaf(-m, m, s2[i] / count);
      var[i] = raw_var < 0.0f ? 0.0f : raw_var;                       // a NaN stays a NaN
      sd[i] = deg > 0 ? __builtin_sqrtf(var[i] + a.eps) : 0.0f;
    }
    store(kMultiVar, var);
    store(kMultiStd, sd);
  }
}

// dtype: 0 fp32, 1 fp16, 2 bfloat16.  slots[6]: the slot of sum, mean, max, min, var, std in a row of `output`
// [num_rows, num_slots, embedding_dim], -1 for an aggregate that is not stored; the stored ones fill 0 .. num_slots - 1, each once.
// argmax / argmin (nullable): int32 [num_rows, embedding_dim]; one that is given needs its max / min stored.  embedding_dim % (16 /
// sizeof(T)) == 0.  Every element of `output` and of the args is written; on a pattern without entries they are filled (0, -1) and
// neither `indices` nor `input` is read (they must still be valid pointers).  Nothing is checked on the device: indptr must be a valid
// CSR of num_rows rows with num_entries entries and every index a row of `input`.
inline int launch_spmm_multi(const int* indptr, const int* indices, int num_rows, long long num_entries, int embedding_dim,
                             const void* input, int dtype, const int (&slots)[kMultiAggregates], int num_slots, float eps, float* output,
                             int* argmax, int* argmin, hipStream_t stream) {
  if (num_rows < 0 || embedding_dim < 0 || num_entries < 0 || num_entries > INT_MAX || dtype < 0 || dtype > 2) return kErrBadShape;
  if (num_slots < 1 || num_slots > kMultiAggregates) return kErrBadShape;
  int used = 0, stored = 0;
  for (int i = 0; i < kMultiAggregates; ++i) {
    if (slots[i] < -1 || slots[i] >= num_slots) return kErrBadShape;
    if (slots[i] < 0) continue;
    if (used >> slots[i] & 1) return kErrBadShape;                    // two aggregates in one slot
    used |= 1 << slots[i];
    ++stored;
  }
  if (stored != num_slots) return kErrBadShape;                       // a slot nobody writes
  if ((argmax != nullptr && slots[kMultiMax] < 0) || (argmin != nullptr && slots[kMultiMin] < 0)) return kErrBadShape;
  if (slots[kMultiStd] >= 0 && !(std::isfinite(eps) && eps > 0.0f)) return kErrBadShape;
  const int v = piece_elems(dtype);
  if (embedding_dim % v) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(input, 15) || bad_ptr(output, 15) || misaligned(argmax, 15) ||
      misaligned(argmin, 15))
    return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim / v);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  const bool m2 = slots[kMultiVar] >= 0 || slots[kMultiStd] >= 0;
  const int select = argmax != nullptr || argmin != nullptr ? kMultiSelectArgs
                     : slots[kMultiMax] >= 0 || slots[kMultiMin] >= 0 ? kMultiSelectValues : kMultiSelectNone;
  dispatch_feature_type(dtype, [&](auto tag) {
    using T = decltype(tag);
    SpmmMultiArgs<T> a{indptr, indices, static_cast<const T*>(input), output, argmax, argmin, (long long)num_slots * embedding_dim,
                       {}, eps, num_rows, embedding_dim, g.lanes, (int)g.per_xcd};
    for (int i = 0; i < kMultiAggregates; ++i) a.slot[i] = slots[i];
    auto go = [&](auto m2_tag, auto select_tag) {
      hipLaunchKernelGGL((spmm_multi_kernel<T, decltype(m2_tag)::value, decltype(select_tag)::value>), grid, dim3(256), 0, stream, a);
    };
    auto by_select = [&](auto m2_tag) {
      if (select == kMultiSelectNone) go(m2_tag, std::integral_constant<int, kMultiSelectNone>{});
      else if (select == kMultiSelectValues) go(m2_tag, std::integral_constant<int, kMultiSelectValues>{});
      else go(m2_tag, std::integral_constant<int, kMultiSelectArgs>{});
    };
    if (m2) by_select(std::true_type{});
    else by_select(std::false_type{});
  });
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- the joint backward on the transposed CSR ---------------------------------------------------------------------------------------
struct SpmmMultiBackwardArgs {
  const int* t_indptr;     // [num_cols + 1]
  const int* t_indices;    // [nnz] row ids of the forward = rows of u, w, mean, g_max, g_min and the args
  const int* t_order;      // [nnz] the entry of the CSR that entry e of the transpose is; HAS_SEL only
  const float* x;          // [num_cols, F] the forward's input as fp32; HAS_W only
  const float* u;          // [*, F]; HAS_U only
  const float* w;          // [*, F]; HAS_W only
  const float* mean;       // rows of mean_ld floats; HAS_W only
  const float* g_max;      // [*, F] or NULL (with argmax)
  const int* argmax;
  const float* g_min;      // [*, F] or NULL (with argmin)
  const int* argmin;
  float* output;           // [num_cols, F]
  long long mean_ld;       // the row stride of `mean` in floats (a slot of the forward's output: A F)
  int num_cols;
  int F;
  int lanes_per_row;
  int groups_per_xcd;
};

template <bool HAS_U, bool HAS_W, bool HAS_SEL, int UNROLL = 4>
static __global__ __launch_bounds__(256) void spmm_multi_backward_kernel(const SpmmMultiBackwardArgs a) {
  static_assert(HAS_U || HAS_W || HAS_SEL, "nothing to do");
  const int L = a.lanes_per_row;
  const int rows_per_group = 256 / L;
  const long long group = (long long)(blockIdx.x % kNumXcd) * a.groups_per_xcd + blockIdx.x / kNumXcd;
  const long long col = group * rows_per_group + (int)threadIdx.x / L;
  if (col >= a.num_cols) return;
  const int lane = (int)threadIdx.x & (L - 1);
  const long long f0 = ((long long)blockIdx.y * 64 + lane) * 4;       // this lane's 4 features
  if (f0 >= a.F) return;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int e = a.t_indptr[col];
  const int end = a.t_indptr[col + 1];
  const long long F = a.F;
  float4_t x = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (HAS_W) {
    if (e < end) x = *reinterpret_cast<const float4_t*>(a.x + col * F + f0);
  }
  const bool with_max = HAS_SEL && a.argmax != nullptr, with_min = HAS_SEL && a.argmin != nullptr;   // wave-uniform

  struct Entry {
    long long offset;
    int id;
    float4_t u, w, mean;
    int4_t won_max, won_min;
  };
  auto issue = [&](Entry& t, const int ee) {
    const long long r = a.t_indices[ee];
    t.offset = r * F + f0;
    if constexpr (HAS_U) t.u = *reinterpret_cast<const float4_t*>(a.u + t.offset);
    if constexpr (HAS_W) {
      t.w = *reinterpret_cast<const float4_t*>(a.w + t.offset);
      t.mean = *reinterpret_cast<const float4_t*>(a.mean + r * a.mean_ld + f0);
    }
    if constexpr (HAS_SEL) {
      t.id = a.t_order[ee];
      if (with_max) t.won_max = *reinterpret_cast<const int4_t*>(a.argmax + t.offset);
      if (with_min) t.won_min = *reinterpret_cast<const int4_t*>(a.argmin + t.offset);
    }
  };
  auto route = [&](const int4_t won, const int id, const float* const g) {
    if (won[0] == id || won[1] == id || won[2] == id || won[3] == id) {
      const float4_t got = *reinterpret_cast<const float4_t*>(g);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (won[i] == id) acc[i] += got[i];
    }
  };
  auto consume = [&](const Entry& t) {
    if constexpr (HAS_U) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += t.u[i];
    }
    if constexpr (HAS_W) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(t.w[i], x[i] - t.mean[i], acc[i]);
    }
    if constexpr (HAS_SEL) {
      if (with_max) route(t.won_max, t.id, a.g_max + t.offset);
      if (with_min) route(t.won_min, t.id, a.g_min + t.offset);
    }
  };
  // the rows of a batch of entries are loaded before the first is consumed (the tail: clamped ids, surplus slots skipped)
  for (; end - e >= UNROLL; e += UNROLL) {
    Entry t[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) issue(t[u], e + u);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) consume(t[u]);
  }
  if (e < end) {
    Entry t[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) issue(t[u], u < end - e ? e + u : end - 1);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (u < end - e) consume(t[u]);
  }
  *reinterpret_cast<float4_t*>(a.output + col * F + f0) = float4_t{acc[0], acc[1], acc[2], acc[3]};
}

// embedding_dim % 4 == 0.  u (nullable): the gradient every entry of a row passes on; w with x and mean (nullable together): the
// centred term; g_max with argmax and g_min with argmin (nullable in pairs): the routed gradients; at least one of the four groups is
// given.  mean_ld >= embedding_dim, a multiple of 4.  Every row of `output` is written (columns without entries: zeros); with
// num_entries == 0 nothing but t_indptr is read.  Nothing is checked on the device: t_indptr must be a valid CSR of num_cols rows with
// num_entries entries, every t_indices a row of the row-indexed operands.  The args are only compared, never used as an index.
inline int launch_spmm_multi_backward(const int* t_indptr, const int* t_indices, const int* t_order, int num_cols, long long num_entries,
                                      int embedding_dim, const float* x, const float* u, const float* w, const float* mean,
                                      long long mean_ld, const float* g_max, const int* argmax, const float* g_min, const int* argmin,
                                      float* output, hipStream_t stream) {
  if (num_cols < 0 || num_entries < 0 || num_entries > INT_MAX || embedding_dim < 0 || embedding_dim % 4) return kErrBadShape;
  const bool has_u = u != nullptr, has_w = w != nullptr, has_max = g_max != nullptr, has_min = g_min != nullptr;
  if (has_w != (x != nullptr) || has_w != (mean != nullptr) || has_max != (argmax != nullptr) || has_min != (argmin != nullptr))
    return kErrBadShape;
  if (!(has_u || has_w || has_max || has_min)) return kErrBadShape;
  if (has_w && (mean_ld < embedding_dim || mean_ld % 4)) return kErrBadShape;
  if (num_cols == 0 || embedding_dim == 0) return kOk;
  if (bad_ptr(t_indptr, 3) || bad_ptr(output, 15) || misaligned(t_indices, 3) || misaligned(t_order, 3) || misaligned(x, 15) ||
      misaligned(u, 15) || misaligned(w, 15) || misaligned(mean, 15) || misaligned(g_max, 15) || misaligned(argmax, 15) ||
      misaligned(g_min, 15) || misaligned(argmin, 15))
    return kErrBadShape;
  if (num_entries > 0 && (t_indices == nullptr || ((has_max || has_min) && t_order == nullptr))) return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_cols, embedding_dim / 4);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  const SpmmMultiBackwardArgs a{t_indptr, t_indices, t_order, x, u, w, mean, g_max, argmax, g_min, argmin, output, mean_ld,
                                num_cols, embedding_dim, g.lanes, (int)g.per_xcd};
  const int variant = (has_u ? 4 : 0) | (has_w ? 2 : 0) | (has_max || has_min ? 1 : 0);
  switch (variant) {
    case 1: hipLaunchKernelGGL((spmm_multi_backward_kernel<false, false, true>), grid, dim3(256), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((spmm_multi_backward_kernel<false, true, false>), grid, dim3(256), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((spmm_multi_backward_kernel<false, true, true>), grid, dim3(256), 0, stream, a); break;
    case 4: hipLaunchKernelGGL((spmm_multi_backward_kernel<true, false, false>), grid, dim3(256), 0, stream, a); break;
    case 5: hipLaunchKernelGGL((spmm_multi_backward_kernel<true, false, true>), grid, dim3(256), 0, stream, a); break;
    case 6: hipLaunchKernelGGL((spmm_multi_backward_kernel<true, true, false>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((spmm_multi_backward_kernel<true, true, true>), grid, dim3(256), 0, stream, a); break;
  }
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
