// Voltrix-SpMM for MI355X (gfx950) -- edge softmax and multi-head aggregation in one launch, and the two launches of its backward:
//
//   forward   out[r, h, :] = sum_{e in row r} alpha[e, h] feat[col_e, h, :],  alpha = row softmax of z = scale s
//             m[r, h] = max_{e in row r} sigma s[e, h] (sigma = sign of scale; -inf for a row without entries),
//             l[r, h] = sum_{e in row r} exp(|scale| (sigma s[e, h] - m[r, h]))
//   d_s       d_s[e, h] = scale alpha[e, h] (<dC[row_e, h], feat[col_e, h]> - delta[row_e, h]),  delta[r, h] = <dC[r, h], out[r, h]>
//   d_feat    d_feat[c, h, :] = sum_{e in column c} alpha[order[e], h] dC[row_e, h, :]          (on the transposed CSR)
//
// Why it exists.  The chain edge softmax -> spmm_csr_heads moves alpha [nnz, H] through memory in both directions and grad_alpha
// [nnz, H] in the backward, and takes four launches forward and five backward.  alpha[e, h] is a function of s[e, h],
// m[row_e, h] and l[row_e, h], so it is recomputed where it is used and never stored; and sum_e alpha_e <dC_r, feat_e> = <dC_r, out_r>,
// so the softmax backward's row reduction is the dense product delta (torch, [n, H, D]) instead of a segmented scan over the edges.
//
// Forward (attn_aggregate_csr_kernel).  spmm_csr_heads_kernel<T, 4>'s shape: the lane's place of csr_row_gather.hpp over rows of H D
// elements, a lane owns the head piece / (D / V).  Two passes per row.
// Pass 1: the row maximum of the lane's head -- a maximum is exact in any order, so when a head is a power of two of pieces (<= 64)
// its lanes split the row's entries and combine with an xor tree; any other head width has every lane read all of them.  Pass 2:
// w_e = exp(|scale| (sigma s_e - m)), acc = fma(w_e, feat, acc) and l += w_e in CSR edge order, batches of 4 edges with a clamped
// tail; then out = acc (1 / l), zeros where l = 0.  The lane holding the first piece of a head writes m and l.  Two passes rather
// than an online rescale: the second read of a row's scores comes from cache for every row that is not a hub, and a weight is
// computed once against the final maximum, which is what the backward recomputes.
//
// d_s (attn_aggregate_grad_scores_kernel).  sddmm_heads_csr_kernel<float, T, R>'s shape: 128 consecutive edges per lane group, the
// window of row ends, one gathered row of feat per edge, the butterfly to the head's lanes; lane 0 of every head then reads s, m, l and
// delta of its edge and stores scale (alpha (dot - delta)).  Split by edges: a hub row costs what its edges cost.
//
// d_feat (attn_aggregate_grad_feat_kernel).  spmm_csr_heads_kernel on the transposed CSR: the lane's value is recomputed from
// scores[order[e] H + h], m[row H + h] and l[row H + h] with row = t_indices[e]; dC is never permuted and alpha[t_order] never exists.
//
// One weight function (aa_weight) serves the three kernels: the forward's w is aa_weight(s, m, 1) and the backward's alpha is
// aa_weight(s, m, 1 / l) -- the same expression, the same bits of exp.
//
// Special values, those of spmm_csr_heads(edge_softmax_heads(s, scale), feat): s = -inf weighs 0; a row or a row's head holding only
// -inf has l = 0 and gives zeros (and d_s = 0: the test sigma s == -inf comes before (-inf) - (-inf)); a row without entries gives
// zeros, m = -inf, l = 0; a NaN or +inf score makes out, d_s and its columns' d_feat NaN in its own row and head and nowhere else;
// scale = 0 gives the mean over the entries that are not -inf.  The maximum and the differences are taken on sigma s, the scaling by
// |scale| after, as in edge_softmax_kernels.hpp.
//
// Numerics (contraction off; the one fused operation is the explicit fma of the accumulation).  u = 2^-23.  A weight carries the
// relative error (1.5 |z - m| + 2) u (difference, scale, log2 e: 1.5 |z - m| u; v_exp_f32 and one more rounding: 2 u), and
// x exp(-x) <= 1/e bounds its absolute error by 2.6 u.  acc and l take deg_r fused accumulations each, l >= 1 (the maximum's
// term is exactly 1), and the epilogue is one reciprocal and one product:
//   |out - ref| <= 2 (deg_r + 3) u sum_e alpha_e |feat_e| + u sum_e |feat_e| / l + 2^-126
// d_s and d_feat: DESIGN.md 3.17.  Per head, the lanes, the order of the sums and the butterfly are those of the H = 1 call on the
// contiguous slices, so out[:, h], m[:, h], l[:, h], d_s[:, h] and d_feat[:, h] have its bits.  No LDS, no scratch, no float atomics,
// no workspace, no host synchronisation; offsets e H + h and row H D are 64-bit.
//
// Attention dropout (DROP = true, the trailing template argument of the three kernels).  k[e, h] = keep_scale where bit
// h & 31 of word h >> 5 of mask[e] is set, 0 elsewhere (dropout_mask_kernels.hpp).  Dropout acts on alpha, after the normalisation: m and
// l are computed over every entry exactly as without a mask; out = sum_e alpha_e k_e feat_e, so sum_e alpha_e k_e <dC_r, feat_e> =
// <dC_r, out_r> = delta still; d_s = scale alpha (k dot - delta); d_feat weighs by alpha k with the mask read at order[e].  A dropped
// entry is a predicate on the bit, not a product with 0: the lane's 16 bytes are not loaded and nothing is accumulated, so a NaN there
// reaches nothing, and the bytes the gathers request fall with the kept fraction (what that does to time: DESIGN.md 3.19).  The
// batch's ids, mask words and scores are loaded unconditionally and first; only the 16-byte gathers are predicated, issued back to back.
// With every bit set and keep_scale = 1 the bits are those of DROP = false (w * 1.0f is exact).  The launchers that instantiate
// DROP = true live in attn_aggregate_dropout.hpp, so a translation unit that includes this header alone emits the kernels it always did.
//
// Known limit.  The forward and d_feat keep the weakness of spmm_csr_heads_kernel: a wave walks a whole hub row (for d_feat, a hub
// column), and the forward walks it twice.  The hub-row split is the follow-up for all row-per-group kernels together.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "voltrix/edge_softmax_kernels.hpp"
#include "voltrix/launch_geometry.hpp"
#include "voltrix/sddmm_kernels.hpp"
#include "voltrix/spmm_csr_kernels.hpp"

namespace voltrix {

// exp(a (sigma s - m)) inv_l, 0 inv_l for sigma s = -inf.  inv_l = 1: the forward's weight; inv_l = aa_inv(l): alpha.
__device__ __forceinline__ float aa_weight(const float s, const float m, const float inv_l, const float sign, const float a) {
#pragma clang fp contract(off)
  const float key = sign * s;
  const float w = key == -INFINITY ? 0.0f : es_exp(a * (key - m));
  return w * inv_l;
}

// 1 / l, and 0 for l = 0 (a row or head without a weight: every alpha is 0); NaN stays NaN
__device__ __forceinline__ float aa_inv(const float l) { return l == 0.0f ? 0.0f : __builtin_amdgcn_rcpf(l); }

template <typename T>
struct AttnAggregateArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz] column ids = rows of `input`
  const T* input;       // [*, H, D] row-major, rows 16-byte aligned
  float* output;        // [num_rows, H, D]
  const float* scores;  // [nnz, H] fp32 in CSR order
  float* m;             // [num_rows, H]
  float* l;             // [num_rows, H]
  int num_rows;
  int heads;            // H
  int head_pieces;      // D / V
  int F;                // H * D
  int lanes_per_row;    // power of two <= 64
  int groups_per_xcd;   // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
  int max_lanes;        // lanes of a head that share pass 1: head_pieces when it is a power of two <= 64, else 1
  float sign;           // +1 / -1 = sign of scale
  float a;              // |scale|
  const uint32_t* mask; // DROP: [nnz, mask_words] keep bits in CSR order (dropout_mask_kernels.hpp)
  int mask_words;       // DROP: ceil(H / 32)
  float keep_scale;     // DROP: the factor of a kept entry
};

// Keeps the load of `id` where the source puts it: the compiler would otherwise sink an id that only a predicated gather uses into
// the predicated block, and every gather would wait for its own id instead of the batch's ids being fetched together.  No instruction.
__device__ __forceinline__ void aa_pin(int& id) { asm volatile("" : "+v"(id)); }

// bit `bit` of a mask word
__device__ __forceinline__ bool aa_kept(const uint32_t word, const int bit) { return ((word >> bit) & 1u) != 0u; }

// DROP: attention dropout.  m and l are those of the undropped softmax; a kept entry accumulates with the weight
// w keep_scale, a dropped entry's piece of feat is neither loaded nor accumulated.
template <typename T, int UNROLL, bool DROP = false>
static __global__ __launch_bounds__(256) void attn_aggregate_csr_kernel(const AttnAggregateArgs<T> a) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;                                                 // whole heads leave: a head's lanes stay together below
  const long long row = p.row, col0 = p.col0;
  const int piece = p.piece;
  const long long H = a.heads;
  const int head = piece / a.head_pieces;
  const float* const sc = a.scores + head;                             // this lane's head: s[e, head] = sc[e H]
  const int begin = a.indptr[row];
  const int end = a.indptr[row + 1];

  // pass 1: the row maximum of sigma s.  The head's max_lanes lanes (aligned: max_lanes divides 64) take every max_lanes-th entry.
  float m = -INFINITY;
  for (long long e = (long long)begin + (piece & (a.max_lanes - 1)); e < end; e += a.max_lanes) m = fmaxf(m, a.sign * sc[e * H]);
  for (int x = 1; x < a.max_lanes; x <<= 1) m = fmaxf(m, __shfl_xor(m, x, 64));

  // pass 2: weights against the final maximum, accumulated in CSR edge order
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  float l = 0.0f;
  int e = begin;
  const T* const base = a.input + col0;
  const long long F = a.F;
  [[maybe_unused]] const uint32_t* mk = nullptr;                       // DROP: this lane's word of every edge and its bit in it
  [[maybe_unused]] long long W = 0;
  [[maybe_unused]] int bit = 0;
  if constexpr (DROP) {
    mk = a.mask + (head >> 5);
    W = a.mask_words;
    bit = head & 31;
  }
  // full batches of UNROLL edges, then one more batch for the tail with clamped ids (spmm_csr_heads_kernel: every load issued before
  // the first is consumed)
  for (; end - e >= UNROLL; e += UNROLL) {
    uint4_t raw[UNROLL];
    float s[UNROLL];
    [[maybe_unused]] bool keep[UNROLL];
    if constexpr (DROP) {      // the batch's column ids, mask words and scores first, unconditionally; then the predicated gathers
      int col[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        col[u] = a.indices[e + u];
        keep[u] = aa_kept(mk[(long long)(e + u) * W], bit);
        s[u] = sc[(long long)(e + u) * H];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) aa_pin(col[u]);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (keep[u]) raw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)col[u] * F);   // a dropped entry's raw is never read
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        raw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[e + u] * F);
        s[u] = sc[(long long)(e + u) * H];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float w = aa_weight(s[u], m, 1.0f, a.sign, a.a);
      if constexpr (DROP) {
        if (keep[u]) csr_accumulate_scaled<T>(acc, raw[u], w * a.keep_scale);
      } else {
        csr_accumulate_scaled<T>(acc, raw[u], w);
      }
      l += w;
    }
  }
  if (e < end) {
    uint4_t raw[UNROLL];
    float s[UNROLL];
    [[maybe_unused]] bool keep[UNROLL];
    if constexpr (DROP) {
      int col[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int ee = u < end - e ? e + u : end - 1;
        col[u] = a.indices[ee];
        keep[u] = aa_kept(mk[(long long)ee * W], bit) && u < end - e;
        s[u] = sc[(long long)ee * H];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) aa_pin(col[u]);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (keep[u]) raw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)col[u] * F);   // a dropped entry's raw is never read
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int ee = u < end - e ? e + u : end - 1;
        raw[u] = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F);
        s[u] = sc[(long long)ee * H];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (u < end - e) {
        const float w = aa_weight(s[u], m, 1.0f, a.sign, a.a);
        if constexpr (DROP) {
          if (keep[u]) csr_accumulate_scaled<T>(acc, raw[u], w * a.keep_scale);
        } else {
          csr_accumulate_scaled<T>(acc, raw[u], w);
        }
        l += w;
      }
  }
  const float inv = aa_inv(l);
  float4_t* out = reinterpret_cast<float4_t*>(a.output + row * F + col0);
#pragma unroll
  for (int i = 0; i < V / 4; ++i) out[i] = float4_t{acc[4 * i] * inv, acc[4 * i + 1] * inv, acc[4 * i + 2] * inv, acc[4 * i + 3] * inv};
  if (piece == head * a.head_pieces) {                                 // the head's first piece: one lane per (row, head)
    a.m[row * H + head] = m;
    a.l[row * H + head] = l;
  }
}

// The checks the three entry points share.  v: elements per 16-byte piece of the gathered operand.
inline int attn_aggregate_check_shape(int num_rows, long long nnz, int heads, int head_dim, int dtype, float scale, int* v) {
  if (num_rows < 0 || nnz < 0 || head_dim < 0 || heads < 1 || dtype < 0 || dtype > 2 || nnz > INT_MAX ||
      (long long)heads * head_dim > INT_MAX || !std::isfinite(scale))
    return kErrBadShape;
  *v = piece_elems(dtype);
  if (head_dim % *v) return kErrBadShape;
  if (nnz > 0 && num_rows == 0) return kErrBadShape;
  return kOk;
}

// the factor of a kept entry: finite and not negative (checked with the shape, before "nothing to do")
inline bool attn_aggregate_bad_keep_scale(float keep_scale) { return !std::isfinite(keep_scale) || keep_scale < 0.0f; }

// dtype: 0 fp32, 1 fp16, 2 bfloat16.  head_dim % (16 / sizeof(T)) == 0.  Every element of output, m and l is written (rows without
// entries: zeros, m = -inf, l = 0); with nnz == 0 indices, scores and input are not read.  Nothing is checked on the device: indptr
// must be a valid CSR of num_rows rows ending at nnz, and every index a row of `input`.
template <bool DROP>
inline int launch_attn_aggregate_csr_impl(const int* indptr, const int* indices, const float* scores, int num_rows, long long nnz,
                                          int heads, int head_dim, const void* input, int dtype, float scale, float* output, float* m,
                                          float* l, const void* mask, float keep_scale, hipStream_t stream) {
  int v = 0;
  const int rc = attn_aggregate_check_shape(num_rows, nnz, heads, head_dim, dtype, scale, &v);
  if (rc != kOk) return rc;
  if (DROP && attn_aggregate_bad_keep_scale(keep_scale)) return kErrBadShape;
  if (num_rows == 0 || head_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(output, 15) || bad_ptr(m, 3) ||
      bad_ptr(l, 3))
    return kErrBadShape;
  if (nnz > 0 && (bad_ptr(indices, 3) || bad_ptr(scores, 3) || bad_ptr(input, 15) || (DROP && bad_ptr(mask, 3))))
    return kErrBadShape;
  const int head_pieces = head_dim / v;
  const int pieces = heads * head_pieces;                // 16-byte pieces per row
  const RowGroupGrid g = row_group_grid(num_rows, pieces);
  if (!g.ok) return kErrBadShape;
  const int max_lanes = head_pieces <= 64 && (head_pieces & (head_pieces - 1)) == 0 ? head_pieces : 1;
  const dim3 grid = row_group_dim3(g);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    const AttnAggregateArgs<T> a{indptr, indices, static_cast<const T*>(input), output, scores, m, l, num_rows, heads, head_pieces,
                                 heads * head_dim, g.lanes, (int)g.per_xcd, max_lanes, scale < 0.0f ? -1.0f : 1.0f, std::fabs(scale),
                                 static_cast<const uint32_t*>(mask), (heads + 31) / 32, keep_scale};
    hipLaunchKernelGGL((attn_aggregate_csr_kernel<T, 4, DROP>), grid, dim3(256), 0, stream, a);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

inline int launch_attn_aggregate_csr(const int* indptr, const int* indices, const float* scores, int num_rows, long long nnz, int heads,
                                     int head_dim, const void* input, int dtype, float scale, float* output, float* m, float* l,
                                     hipStream_t stream) {
  return launch_attn_aggregate_csr_impl<false>(indptr, indices, scores, num_rows, nnz, heads, head_dim, input, dtype, scale, output, m, l,
                                               nullptr, 1.0f, stream);
}

struct AttnAggregateGradScoresArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [nnz] column ids = rows of y
  const float* x;        // dC [num_rows, H, D] fp32, rows 16-byte aligned
  const void* y;         // feat [*, H, D]
  const float* scores;   // [nnz, H]
  const float* m;        // [num_rows, H]
  const float* l;        // [num_rows, H]
  const float* delta;    // [num_rows, H]
  float* out;            // d_s [nnz, H]
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
  float scale;
  float sign;            // +1 / -1 = sign of scale
  float a;               // |scale|
  const uint32_t* mask;  // DROP: [nnz, mask_words] keep bits
  int mask_words;        // DROP: ceil(H / 32)
  float keep_scale;      // DROP: the factor of a kept entry
};

// Y: float / _Float16 / bfloat16_bits.  R = 1: one piece per lane, dC held in registers; 0: any number, dC loaded per edge.
// DROP: d_s = scale (alpha (k dot - delta)); a dropped entry's row of feat is not read and its dot is +0.
template <typename Y, int R, bool DROP = false>
static __global__ __launch_bounds__(256) void attn_aggregate_grad_scores_kernel(const AttnAggregateGradScoresArgs a) {
#pragma clang fp contract(off)
  using X = float;
  constexpr int V = 16 / (int)sizeof(Y);            // columns per piece
  constexpr int XW = (int)sizeof(X) * V / 16;       // 16-byte loads per piece of dC: 1 or 2
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
  const X* const x = a.x;
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

  float xc[V];                                      // dC[cur_row, head], this lane's piece (R = 1)
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
    [[maybe_unused]] bool keep[U];                    // DROP: the bit of (edge, this lane's head); the lanes of a head agree
    if constexpr (DROP) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ee = e + u < e_end ? e + u : e_end - 1;
        keep[u] = live && aa_kept(a.mask[(long long)ee * a.mask_words + (head >> 5)], head & 31);
      }
    }
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
        if constexpr (DROP) {
          if (mine && keep[u]) yr[u] = *reinterpret_cast<const uint4_t*>(y + (long long)cols[u] * F + k0);
        } else {
          if (mine) yr[u] = *reinterpret_cast<const uint4_t*>(y + (long long)cols[u] * F + k0);
        }
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
          if constexpr (DROP) {
            yr[u] = uint4_t{0u, 0u, 0u, 0u};
#pragma unroll
            for (int w = 0; w < XW; ++w) xr[u][w] = uint4_t{0u, 0u, 0u, 0u};
            if (!keep[u]) continue;
          }
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
        if (e + u < e_end) {
          const long long eh = (long long)(e + u) * a.heads + head;
          const long long rh = (long long)rows[u] * a.heads + head;
          const float alpha = aa_weight(a.scores[eh], a.m[rh], aa_inv(a.l[rh]), a.sign, a.a);
          if constexpr (DROP) a.out[eh] = a.scale * (alpha * ((keep[u] ? a.keep_scale * acc[u] : 0.0f) - a.delta[rh]));
          else a.out[eh] = a.scale * (alpha * (acc[u] - a.delta[rh]));
        }
    }
  }
}

// d_s[e, h] = scale alpha[e, h] (<grad_out[row_e, h], feat[indices[e], h]> - delta[row_e, h]) with alpha recomputed from scores, m, l.
// grad_out fp32 [num_rows, H, D]; feat dtype 0 fp32 / 1 fp16 / 2 bfloat16.  Every element of out[nnz, heads] is written.
template <bool DROP>
inline int launch_attn_aggregate_grad_scores_csr_impl(const int* indptr, const int* indices, int num_rows, long long nnz, int heads,
                                                      int head_dim, const float* grad_out, const void* feat, int dtype,
                                                      const float* scores, const float* m, const float* l, const float* delta,
                                                      float scale, float* out, const void* mask, float keep_scale, hipStream_t stream) {
  int v = 0;
  const int rc = attn_aggregate_check_shape(num_rows, nnz, heads, head_dim, dtype, scale, &v);
  if (rc != kOk) return rc;
  if (DROP && attn_aggregate_bad_keep_scale(keep_scale)) return kErrBadShape;
  if (nnz == 0 || head_dim == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(grad_out, 15) ||
      bad_ptr(feat, 15) || bad_ptr(scores, 3) || bad_ptr(m, 3) ||
      bad_ptr(l, 3) || bad_ptr(delta, 3) || bad_ptr(out, 3) || (DROP && bad_ptr(mask, 3)))
    return kErrBadShape;
  const int pieces = head_dim / v;
  const EdgeChunkGrid g = edge_chunk_grid(nnz, heads, pieces, kSddmmChunkEdges);
  if (!g.ok) return kErrBadShape;
  const AttnAggregateGradScoresArgs a{indptr, indices, grad_out, feat, scores, m, l, delta, out, num_rows, (int)nnz, heads, pieces,
                                      g.head_lanes, g.head_shift, g.rounds, g.slab_heads, g.lanes, g.wgs, g.per_xcd, scale,
                                      scale < 0.0f ? -1.0f : 1.0f, std::fabs(scale), static_cast<const uint32_t*>(mask),
                                      (heads + 31) / 32, keep_scale};
  const dim3 grid((unsigned)(g.per_xcd * kNumXcd), (unsigned)g.slabs);
  auto go = [&](auto ytag) {
    using Y = decltype(ytag);
    if (g.rounds == 1) hipLaunchKernelGGL((attn_aggregate_grad_scores_kernel<Y, 1, DROP>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((attn_aggregate_grad_scores_kernel<Y, 0, DROP>), grid, dim3(256), 0, stream, a);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

inline int launch_attn_aggregate_grad_scores_csr(const int* indptr, const int* indices, int num_rows, long long nnz, int heads,
                                                 int head_dim, const float* grad_out, const void* feat, int dtype, const float* scores,
                                                 const float* m, const float* l, const float* delta, float scale, float* out,
                                                 hipStream_t stream) {
  return launch_attn_aggregate_grad_scores_csr_impl<false>(indptr, indices, num_rows, nnz, heads, head_dim, grad_out, feat, dtype, scores,
                                                           m, l, delta, scale, out, nullptr, 1.0f, stream);
}

template <typename T>
struct AttnAggregateGradFeatArgs {
  const int* indptr;    // [num_rows + 1]: the TRANSPOSED CSR, num_rows = the columns of the pattern
  const int* indices;   // [nnz] rows of the pattern = rows of `input`, m and l
  const int* order;     // [nnz] the entry of the CSR that entry e of the transpose is
  const T* input;       // dC [*, H, D] row-major, rows 16-byte aligned
  float* output;        // d_feat [num_rows, H, D]
  const float* scores;  // [nnz, H] in CSR order
  const float* m;       // [*, H]
  const float* l;       // [*, H]
  int num_rows;
  int heads;            // H
  int head_pieces;      // D / V
  int F;                // H * D
  int lanes_per_row;    // power of two <= 64
  int groups_per_xcd;   // ceil(row groups / 8)
  float sign;
  float a;
  const uint32_t* mask; // DROP: [nnz, mask_words] keep bits in CSR order: read at order[e]
  int mask_words;       // DROP: ceil(H / 32)
  float keep_scale;     // DROP: the factor of a kept entry
};

// DROP: the weight is alpha keep_scale for a kept entry; a dropped entry's piece of dC is neither loaded nor accumulated.
template <typename T, int UNROLL, bool DROP = false>
static __global__ __launch_bounds__(256) void attn_aggregate_grad_feat_kernel(const AttnAggregateGradFeatArgs<T> a) {
#pragma clang fp contract(off)
  constexpr int V = 16 / (int)sizeof(T);
  const CsrLanePlace p = csr_lane_place<V>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F);
  if (!p.work) return;
  const long long row = p.row, col0 = p.col0;
  const int piece = p.piece;
  const long long H = a.heads;
  const int head = piece / a.head_pieces;
  const float* const sc = a.scores + head;
  const float* const mh = a.m + head;
  const float* const lh = a.l + head;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  int e = a.indptr[row];
  const int end = a.indptr[row + 1];
  const T* const base = a.input + col0;
  const long long F = a.F;
  [[maybe_unused]] const uint32_t* mk = nullptr;
  [[maybe_unused]] long long W = 0;
  [[maybe_unused]] int bit = 0;
  if constexpr (DROP) {
    mk = a.mask + (head >> 5);
    W = a.mask_words;
    bit = head & 31;
  }
  for (; end - e >= UNROLL; e += UNROLL) {
    uint4_t raw[UNROLL];
    float s[UNROLL], m[UNROLL], l[UNROLL];
    [[maybe_unused]] bool keep[UNROLL];
    if constexpr (DROP) {      // every id, then every word that hangs on one, then the four predicated gathers back to back
      int ri[UNROLL];
      long long r[UNROLL], o[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        ri[u] = a.indices[e + u];
        o[u] = a.order[e + u];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        aa_pin(ri[u]);
        r[u] = ri[u];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        keep[u] = aa_kept(mk[o[u] * W], bit);
        s[u] = sc[o[u] * H];
        m[u] = mh[r[u] * H];
        l[u] = lh[r[u] * H];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (keep[u]) raw[u] = *reinterpret_cast<const uint4_t*>(base + r[u] * F);   // a dropped entry's raw is never read
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const long long r = a.indices[e + u];
        raw[u] = *reinterpret_cast<const uint4_t*>(base + r * F);
        s[u] = sc[(long long)a.order[e + u] * H];
        m[u] = mh[r * H];
        l[u] = lh[r * H];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if constexpr (DROP) {
        if (keep[u]) csr_accumulate_scaled<T>(acc, raw[u], aa_weight(s[u], m[u], aa_inv(l[u]), a.sign, a.a) * a.keep_scale);
      } else {
        csr_accumulate_scaled<T>(acc, raw[u], aa_weight(s[u], m[u], aa_inv(l[u]), a.sign, a.a));
      }
    }
  }
  if (e < end) {
    uint4_t raw[UNROLL];
    float s[UNROLL], m[UNROLL], l[UNROLL];
    [[maybe_unused]] bool keep[UNROLL];
    if constexpr (DROP) {
      int ri[UNROLL];
      long long r[UNROLL], o[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int ee = u < end - e ? e + u : end - 1;
        ri[u] = a.indices[ee];
        o[u] = a.order[ee];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        aa_pin(ri[u]);
        r[u] = ri[u];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        keep[u] = aa_kept(mk[o[u] * W], bit) && u < end - e;
        s[u] = sc[o[u] * H];
        m[u] = mh[r[u] * H];
        l[u] = lh[r[u] * H];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (keep[u]) raw[u] = *reinterpret_cast<const uint4_t*>(base + r[u] * F);   // a dropped entry's raw is never read
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int ee = u < end - e ? e + u : end - 1;
        const long long r = a.indices[ee];
        raw[u] = *reinterpret_cast<const uint4_t*>(base + r * F);
        s[u] = sc[(long long)a.order[ee] * H];
        m[u] = mh[r * H];
        l[u] = lh[r * H];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (u < end - e) {
        if constexpr (DROP) {
          if (keep[u]) csr_accumulate_scaled<T>(acc, raw[u], aa_weight(s[u], m[u], aa_inv(l[u]), a.sign, a.a) * a.keep_scale);
        } else {
          csr_accumulate_scaled<T>(acc, raw[u], aa_weight(s[u], m[u], aa_inv(l[u]), a.sign, a.a));
        }
      }
  }
  csr_store_piece(a.output + row * F + col0, acc);
}

// d_feat[c, h, :] = sum_{e in row c of the transposed CSR} alpha[order[e], h] grad_out[t_indices[e], h, :], alpha recomputed from
// scores (CSR order), m and l.  grad_out dtype 0 fp32 / 1 fp16 / 2 bfloat16.  Every row of out is written (rows without entries:
// zeros); with nnz == 0 nothing but t_indptr is read.
template <bool DROP>
inline int launch_attn_aggregate_grad_feat_csr_impl(const int* t_indptr, const int* t_indices, const int* order, int num_rows,
                                                    long long nnz, int heads, int head_dim, const void* grad_out, int dtype,
                                                    const float* scores, const float* m, const float* l, float scale, float* out,
                                                    const void* mask, float keep_scale, hipStream_t stream) {
  int v = 0;
  const int rc = attn_aggregate_check_shape(num_rows, nnz, heads, head_dim, dtype, scale, &v);
  if (rc != kOk) return rc;
  if (DROP && attn_aggregate_bad_keep_scale(keep_scale)) return kErrBadShape;
  if (num_rows == 0 || head_dim == 0) return kOk;
  if (bad_ptr(t_indptr, 3) || bad_ptr(out, 15)) return kErrBadShape;
  if (nnz > 0 && (bad_ptr(t_indices, 3) || bad_ptr(order, 3) || bad_ptr(grad_out, 15) ||
                  bad_ptr(scores, 3) || bad_ptr(m, 3) || bad_ptr(l, 3) || (DROP && bad_ptr(mask, 3))))
    return kErrBadShape;
  const int head_pieces = head_dim / v;
  const int pieces = heads * head_pieces;
  const RowGroupGrid g = row_group_grid(num_rows, pieces);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    const AttnAggregateGradFeatArgs<T> a{t_indptr, t_indices, order, static_cast<const T*>(grad_out), out, scores, m, l, num_rows,
                                         heads, head_pieces, heads * head_dim, g.lanes, (int)g.per_xcd, scale < 0.0f ? -1.0f : 1.0f,
                                         std::fabs(scale), static_cast<const uint32_t*>(mask), (heads + 31) / 32, keep_scale};
    hipLaunchKernelGGL((attn_aggregate_grad_feat_kernel<T, 4, DROP>), grid, dim3(256), 0, stream, a);
  };
  dispatch_feature_type(dtype, go);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

inline int launch_attn_aggregate_grad_feat_csr(const int* t_indptr, const int* t_indices, const int* order, int num_rows, long long nnz,
                                               int heads, int head_dim, const void* grad_out, int dtype, const float* scores,
                                               const float* m, const float* l, float scale, float* out, hipStream_t stream) {
  return launch_attn_aggregate_grad_feat_csr_impl<false>(t_indptr, t_indices, order, num_rows, nnz, heads, head_dim, grad_out, dtype,
                                                         scores, m, l, scale, out, nullptr, 1.0f, stream);
}

}  // namespace voltrix
